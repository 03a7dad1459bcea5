"""The hit sort's shortcut for queries without tied keys.  A query whose seed hits share no (extId, curPos) has exactly
one sorted order, so the sort need not follow std::sort's trajectory: k_fill writes a tie-free flag per query, and
sortSegments sends flagged segments of SORT_CAP < n <= 65 536 hits to k_sort_radix (stable 8-bit passes over the record
bits; the emission order is already ascending in curPos) instead of the introsort emulation.

* fg_debug_sort_pairs32 on crafted segments (keys ``rec << cur_bits | cur``, cur ascending inside a segment) against
  ``oracle.std_sort_perm`` per segment: the LDS / radix boundary, the kernel's tile size, the radix / level-loop
  boundary, degenerate digit distributions, one, two and three passes, and one call that mixes flagged segments with
  unflagged segments holding planted ties, empty and one-hit segments.  The radix counts returned are what the
  thresholds say.  The same inputs with FG_SORT_TIEFREE=0 in a fresh process give the same arrays and no radix segment.
* the flag itself: per query it equals "no two exported seed hits (fg_probe_hits) share (ext_id, cur_pos)", on a small
  read set with planted tandems in which both kinds of query occur (checked here on the CPU for the chosen seed), and on
  a crafted index where the self-entry skip decides.
* end to end on that read set: records identical with the switch on and off and identical to the oracle's;
  k_sort_radix launched with the switch on.

Run as a program (`python tests/test_sort_tiefree.py sort|overlaps OUT.npz`) this file is the child of the parity tests."""
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import cpu_seed_hits as _cpu_seed_hits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SORT_CAP = 448          # fg_overlap.hip: pieces up to this size are sorted in LDS
TILE = 2048             # k_sort_radix: hits per tile (256 threads x 8)
RADIX_MAX = 65536       # FG_SORT_RADIX_MAX default
SEED = 7                # workloads.ecoli_pb50 seed of the flag tests (test_seed_has_both_kinds_of_query)
SCALE = 0.02


# ---- crafted segments --------------------------------------------------------------------------------------------
def _segment(rng, n, cur_bits, records):
    """n distinct keys rec << cur_bits | cur, rec drawn from ``records``, in emission order: cur ascending, several
    records at one cur where the draw has it so."""
    records = np.asarray(records, np.uint64)
    m = len(records)
    space = (1 << cur_bits) * m
    assert n <= space
    codes = np.empty(0, np.int64)
    while len(codes) < n:
        codes = np.unique(np.concatenate([codes, rng.integers(0, space, size=n + n // 4 + 16)]))
    codes = np.sort(rng.choice(codes, n, replace=False))
    cur, idx = codes // m, codes % m
    # inside one cur the records come in any order, as the lists of different k-mers do not: shuffle them
    order = np.lexsort((rng.random(n), cur))
    cur, idx = cur[order], idx[order]
    assert np.all(np.diff(cur) >= 0)
    return ((records[idx] << np.uint64(cur_bits)) | cur.astype(np.uint64)).astype(np.uint32)


def _plant_ties(rng, keys, count):
    """copies of the key before them at ``count`` places: equal keys, neighbours in emission order"""
    keys = keys.copy()
    for j in rng.choice(np.arange(1, len(keys)), min(count, len(keys) - 1), replace=False):
        keys[j] = keys[j - 1]
    return keys


def _case(name):
    """(keys, seg_off, cur_bits, rec_bits, flags) of a named case, the same in every process"""
    rng = np.random.default_rng(hash_name(name))
    cur_bits, rec_bits = 16, 16
    every = np.arange(1 << 16)
    if name == "lds_boundary":
        segs = [(n, every, True, 0) for n in (SORT_CAP, SORT_CAP + 1, SORT_CAP + 2)]
    elif name == "tile":
        segs = [(n, every, True, 0) for n in (TILE - 1, TILE, TILE + 1)]
    elif name == "radix_max":
        segs = [(n, every, True, 0) for n in (RADIX_MAX, RADIX_MAX + 1)]
    elif name == "one_bucket":
        segs = [(3000, [0xA5C3], True, 0)]
    elif name == "low_byte_only":
        segs = [(5000, 0x3A00 + np.arange(256), True, 0)]
    elif name == "high_byte_only":
        segs = [(5000, (np.arange(256) << 8) + 0x5C, True, 0)]
    elif name == "rec_bits_9":
        rec_bits = 9
        segs = [(5000, np.arange(1 << 9), True, 0)]
    elif name == "rec_bits_16":
        segs = [(20000, every, True, 0)]
    elif name == "rec_bits_17":
        cur_bits, rec_bits = 15, 17
        segs = [(5000, np.arange(1 << 17), True, 0), (SORT_CAP + 1, np.arange(1 << 17), True, 0)]
    elif name == "mixed":
        segs = [(1000, every, True, 0), (1000, every, False, 40), (0, every, True, 0), (1, every, True, 0),
                (5000, every, False, 300), (SORT_CAP + 1, every, True, 0), (SORT_CAP + 1, every, False, 5),
                (0, every, False, 0), (300, every, True, 0), (1, every, False, 0), (100, every, False, 10),
                (7000, every, True, 0), (3000, np.arange(4), False, 1000)]
    else:
        raise KeyError(name)
    keys, flags, off = [], [], [0]
    for n, records, flagged, ties in segs:
        k = _segment(rng, n, cur_bits, records) if n else np.empty(0, np.uint32)
        if ties:
            k = _plant_ties(rng, k, ties)
            assert len(np.unique(k)) < len(k)
        if flagged:
            assert len(np.unique(k)) == len(k)
        keys.append(k)
        flags.append(1 if flagged else 0)
        off.append(off[-1] + n)
    return np.concatenate(keys), np.asarray(off, np.uint64), cur_bits, rec_bits, np.asarray(flags, np.uint32)


def hash_name(name):
    return int.from_bytes(name.encode()[:7], "little")


CASES = ["lds_boundary", "tile", "radix_max", "one_bucket", "low_byte_only", "high_byte_only", "rec_bits_9",
         "rec_bits_16", "rec_bits_17", "mixed"]


def _expected_radix(off, flags):
    n = np.diff(off.astype(np.int64))
    took = (flags != 0) & (n > SORT_CAP) & (n <= RADIX_MAX)
    return int(took.sum()), int(n[took].sum())


# ---- the read set of the flag and end-to-end tests ------------------------------------------------------------------
def _reads():
    from flye_amd import workloads
    return workloads.ecoli_pb50(seed=SEED, scale=SCALE)[0]


def _all_queries(rs):
    return np.arange(0, 2 * rs.n, dtype=np.uint32)


def _tie_free_from_hits(counts, hits):
    """per query: no two of its hits share (ext_id, cur_pos)"""
    off = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    out = np.zeros(len(counts), np.uint32)
    for i in range(len(counts)):
        h = hits[off[i]:off[i + 1]]
        pair = (h["ext_id"].astype(np.uint64) << np.uint64(32)) | h["cur_pos"].astype(np.uint64)
        out[i] = 1 if len(np.unique(pair)) == len(pair) else 0
    return out


# ---- child processes ------------------------------------------------------------------------------------------------
def _run_sort_cases(ctx):
    out = {}
    for name in CASES:
        keys, off, cur_bits, rec_bits, flags = _case(name)
        k, v, segs, hits = ctx.debug_sort_pairs32(keys, off, cur_bits, rec_bits, flags)
        out[name + "_k"], out[name + "_v"], out[name + "_c"] = k, v, np.array([segs, hits], np.uint64)
    return out


def _run_overlaps():
    from flye_amd import config, gpu
    rs = _reads()
    cfg = config.preset("raw")
    k = int(cfg["kmer_size"])
    ctx = gpu.Context(k, 0)
    ctx.set_reads(rs)
    vi = gpu.VertexIndex(ctx, float(int(cfg["assemble_kmer_sample"])))
    vi.build(cfg)
    det = gpu.OverlapDetector.for_assemble(ctx, vi, cfg)
    res = det.getSeqOverlapsBatch(_all_queries(rs))
    times = ctx.kernel_times()
    out = dict(recs=np.frombuffer(res.recs.tobytes(), np.uint8), query_off=res.query_off, stat_off=res.stat_off,
               stats=res.stats.view(np.uint32),
               counters=np.array([res.query_kmers, res.seed_hits, res.dp_groups, res.dp_elements, res.dp_elements_small],
                                 np.uint64),
               radix_launches=np.array([times.get("k_sort_radix", (0.0, 0))[1]], np.uint64))
    return ctx, det, res, out


def _child_main(what, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from flye_amd import gpu
    if what == "sort":
        ctx = gpu.Context(17, 0)
        out = _run_sort_cases(ctx)
    else:
        ctx, _, _, out = _run_overlaps()
    np.savez(out_path, **out)
    ctx.close()


if __name__ == "__main__":
    _child_main(sys.argv[1], sys.argv[2])
    sys.exit(0)


def _child(tmp_path, what, tiefree):
    out = str(tmp_path / f"{what}_{tiefree}.npz")
    env = dict(os.environ, FG_SORT_TIEFREE=str(tiefree))
    env.pop("FG_SORT_RADIX_MAX", None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), what, out], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out)


# ---- fg_debug_sort_pairs32 ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sort_ctx(built):
    from flye_amd import gpu
    ctx = gpu.Context(17, 0)
    yield ctx
    ctx.close()


def _check_sorted(name, keys, off, flags, k, v):
    from oracle import oracle as O
    for i in range(len(off) - 1):
        a, b = int(off[i]), int(off[i + 1])
        seg = keys[a:b]
        perm = O.std_sort_perm(seg.astype(np.uint64))
        if flags[i]:
            assert np.array_equal(perm, np.argsort(seg, kind="stable")), (name, i)     # distinct keys: one order
        assert np.array_equal(v[a:b], perm), (name, i, b - a)
        assert np.array_equal(k[a:b], seg[perm]), (name, i, b - a)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_sort_pairs32_against_std_sort(sort_ctx, monkeypatch, name):
    monkeypatch.delenv("FG_SORT_TIEFREE", raising=False)
    monkeypatch.delenv("FG_SORT_RADIX_MAX", raising=False)
    keys, off, cur_bits, rec_bits, flags = _case(name)
    k, v, segs, hits = sort_ctx.debug_sort_pairs32(keys, off, cur_bits, rec_bits, flags)
    print(f"{name}: {len(off) - 1} segments, {len(keys)} hits, radix path {segs} segments / {hits} hits")
    _check_sorted(name, keys, off, flags, k, v)
    assert (segs, hits) == _expected_radix(off, flags)
    if name == "radix_max":
        assert (segs, hits) == (1, RADIX_MAX)          # the larger segment stayed in the level loop
    if name != "mixed":
        assert segs > 0


@pytest.mark.gpu
def test_sort_pairs32_without_flags_is_the_emulation(sort_ctx, monkeypatch):
    monkeypatch.delenv("FG_SORT_TIEFREE", raising=False)
    keys, off, cur_bits, rec_bits, flags = _case("mixed")
    k, v, segs, hits = sort_ctx.debug_sort_pairs32(keys, off, cur_bits, rec_bits, None)
    _check_sorted("mixed", keys, off, np.zeros_like(flags), k, v)
    assert (segs, hits) == (0, 0)


@pytest.mark.gpu
def test_sort_pairs32_switch_off_gives_identical_arrays(sort_ctx, monkeypatch, tmp_path):
    monkeypatch.delenv("FG_SORT_TIEFREE", raising=False)
    monkeypatch.delenv("FG_SORT_RADIX_MAX", raising=False)
    on = _run_sort_cases(sort_ctx)
    off = _child(tmp_path, "sort", 0)
    for name in CASES:
        assert on[name + "_k"].tobytes() == off[name + "_k"].tobytes(), name
        assert on[name + "_v"].tobytes() == off[name + "_v"].tobytes(), name
        assert tuple(off[name + "_c"]) == (0, 0), name
    assert sum(int(on[name + "_c"][0]) for name in CASES) > 0


# ---- the flag ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world(built):
    from flye_amd import config
    from oracle import oracle as O
    rs = _reads()
    cfg = config.preset("raw")
    k = int(cfg["kmer_size"])
    o = O.Oracle(k)
    o.set_reads(rs)
    o.build_index(cfg)
    q = _all_queries(rs)
    return dict(rs=rs, cfg=cfg, k=k, o=o, q=q)


def test_seed_has_both_kinds_of_query(world):
    """CPU: with SEED the read set holds tied and tie-free queries, and tie-free ones of a size the radix path takes"""
    counts, hits = _cpu_seed_hits(world["rs"], world["o"].export_index(), world["k"], world["q"])
    flags = _tie_free_from_hits(counts, hits)
    n = counts.astype(np.int64)
    radix = (flags == 1) & (n > SORT_CAP) & (n <= RADIX_MAX)
    from oracle import oracle as O
    assert int(counts.sum()) == world["o"].overlaps(O.detector_params(world["cfg"]), world["q"]).seed_hits
    print(f"{len(flags)} queries: {int(flags.sum())} tie-free, {int(radix.sum())} of them with {SORT_CAP} < hits <= {RADIX_MAX}")
    assert 0 < int(flags.sum()) < len(flags)
    assert int(radix.sum()) > 0


@pytest.mark.gpu
def test_flag_equals_the_statement_on_exported_hits(world, monkeypatch):
    from flye_amd import gpu
    monkeypatch.delenv("FG_SORT_TIEFREE", raising=False)
    for sw in ("FG_HIT_BUDGET", "FG_KMER_BUDGET", "FG_LANE_MIN_HITS", "FG_FORCE_KEY64"):
        monkeypatch.delenv(sw, raising=False)
    rs, cfg, q = world["rs"], world["cfg"], world["q"]
    ctx = gpu.Context(world["k"], 0)
    ctx.set_reads(rs)
    vi = gpu.VertexIndex(ctx, float(int(cfg["assemble_kmer_sample"])))
    vi.build(cfg)
    det = gpu.OverlapDetector.for_assemble(ctx, vi, cfg)
    det.getSeqOverlapsBatch(q)
    q0, flags = ctx.debug_tie_free(len(q))
    assert q0 == 0 and len(flags) == len(q)                   # one sub-range: the whole call
    counts, ptr, n = det.probe_hits(q)
    want = _tie_free_from_hits(counts, gpu.seed_hits_to_host(ptr, n))
    print(f"{len(q)} queries, {int(want.sum())} tie-free")
    assert np.array_equal(flags, want)
    assert 0 < int(want.sum()) < len(want)
    # and the CPU statement the seed was chosen with says the same
    ccounts, chits = _cpu_seed_hits(rs, world["o"].export_index(), world["k"], q)
    assert np.array_equal(ccounts, counts) and np.array_equal(_tie_free_from_hits(ccounts, chits), want)
    ctx.close()


def _self_skip_case():
    """Read 0 holds k-mer X twice and read 1 once: seen from either X of read 0 the list is (0, p1), (0, p2), (1, t) with
    the query's own entry beside another entry of its record -- what is emitted, (0, other), (1, t), holds no tie, while
    read 1 sees (0, p1), (0, p2) at one position: a tie.  Read 2 holds k-mer Y three times: seen from the middle one the
    own entry sits between (2, a) and (2, c), which are emitted and tie.  Read 3 holds Z once and read 4 twice: query 3
    emits (4, u), (4, w), a tie without any skip, and read 4 is tie-free as read 0 is."""
    import chain_craft as cc
    case = cc.Case("self_skip", 12)
    X, Y, Z = case.rand(cc.K), case.rand(cc.K), case.rand(cc.K)
    r0 = np.concatenate([case.rand(300), X, case.rand(200), X, case.rand(400)])
    r1 = np.concatenate([case.rand(250), X, case.rand(500)])
    r2 = np.concatenate([case.rand(100), Y, case.rand(150), Y, case.rand(250), Y, case.rand(300)])
    r3 = np.concatenate([case.rand(120), Z, case.rand(600)])
    r4 = np.concatenate([case.rand(220), Z, case.rand(100), Z, case.rand(350)])
    for r, pos in ((r0, [300]), (r2, [100]), (r3, [120])):
        case.add_read(r)
        case.add_keys(r, pos)
    case.seqs = [r0, r1, r2, r3, r4]
    case.queries = [0, 2, 4, 6, 8]
    return case, np.array([1, 0, 0, 0, 1], np.uint32)


def test_self_skip_case_is_what_it_says(built):
    import chain_craft as cc
    case, want = _self_skip_case()
    groups = cc.enumerate_groups(case)
    got = []
    for q in case.queries:
        pairs = [(t, c) for (qq, t), hits in groups.items() if qq == q for c, _ in hits]
        got.append(1 if len(set(pairs)) == len(pairs) else 0)
    assert got == list(want)
    ex = case.index()
    assert len(ex.keys) == 3 and sorted(np.diff(ex.key_off.astype(np.int64))) == [3, 3, 3]


@pytest.mark.gpu
def test_flag_with_the_self_entry_between_two_entries_of_one_record(built, monkeypatch):
    import chain_craft as cc
    from flye_amd import config, gpu
    monkeypatch.delenv("FG_SORT_TIEFREE", raising=False)
    monkeypatch.delenv("FG_FORCE_KEY64", raising=False)
    case, want = _self_skip_case()
    rs, ex, q = case.readset(), case.index(), case.query_ids()
    ctx = gpu.Context(cc.K, 0)
    ctx.set_reads(rs, case.first_id)
    vi = gpu.VertexIndex(ctx, 1.0)
    vi.import_index(gpu.IndexExport(ex.keys, ex.key_off, ex.entries, ex.repetitive), 1.0)
    det = gpu.OverlapDetector.for_assemble(ctx, vi, config.preset("raw"), min_overlap=cc.MIN_OVERLAP)
    det.getSeqOverlapsBatch(q)
    q0, flags = ctx.debug_tie_free(len(q))
    assert q0 == 0 and np.array_equal(flags, want)
    counts, ptr, n = det.probe_hits(q)
    assert np.array_equal(_tie_free_from_hits(counts, gpu.seed_hits_to_host(ptr, n)), want)
    ctx.close()


# ---- end to end -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_overlaps_identical_with_the_switch_on_and_off(world, monkeypatch, tmp_path):
    from oracle import oracle as O
    from helpers import check_overlaps_equal
    monkeypatch.delenv("FG_SORT_TIEFREE", raising=False)
    monkeypatch.delenv("FG_SORT_RADIX_MAX", raising=False)
    ctx, _, res, on = _run_overlaps()
    ctx.close()
    off = _child(tmp_path, "overlaps", 0)
    for f in ("recs", "query_off", "stat_off", "stats", "counters"):
        assert np.asarray(on[f]).tobytes() == off[f].tobytes(), f
    assert len(on["recs"]) > 0
    assert int(on["radix_launches"][0]) > 0 and int(off["radix_launches"][0]) == 0
    check_overlaps_equal(res, world["o"].overlaps(O.detector_params(world["cfg"]), world["q"]), False)
