"""The hit sort's screen for queries whose tied keys all lie in target groups the chaining prefilter drops.  The order
std::sort leaves tied (extId, curPos) keys in is read only inside a group that reaches the DP; a group with fewer than
minUnique distinct query positions or a query span below minOverlap is dropped before anything reads its hits.  Both are
set properties, so k_sort_screen decides them on the hits in emission order, ahead of the sort, and sortSegments sends
the queries it passes to k_sort_radix together with the tie-free ones.

* ``order_free``: the kernel's statement in numpy over exported hits; on the seed-7 read set of test_sort_tiefree.py it
  finds tie-free, tied-but-order-free and must-emulate queries, and for every query it passes the reference's FULL
  prefilter (oracle/flye_oracle.cpp:713-736, ``prev = 0`` quirk included) drops every group that holds a tie (CPU).
* fg_debug_sort_screen on crafted segments against the same statement: threshold edges, tie positions, the set's
  capacity and colliding records, sizes, key widths, flagged segments.
* end to end on that read set, assemble and repeat-stage detector: results byte-identical between the default,
  FG_SORT_SCREEN=0 and FG_SORT_TIEFREE=0 (fresh child processes) and equal to the oracle's; the reason words equal the
  statement; the radix path took tie-free-in-range + order-free-in-range segments.

Run as a program (`python tests/test_sort_screen.py OUT.npz`) this file is the child of the parity tests."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_sort_tiefree import (RADIX_MAX, SORT_CAP, _all_queries, _cpu_seed_hits, _reads,  # noqa: E402
                               _tie_free_from_hits)

WG = 256                # k_sort_screen: threads per block = the stride of a sweep
TILE = 4 * WG           # SCREEN_TILE: hits a block loads per step of a sweep
CAP = 256               # SCREEN_CAP: tied records a query may have
SLOTS = 512             # SCREEN_SLOTS
MIN_OVERLAP = 1000
MIN_UNIQUE = np.float32(0.01) * np.float32(MIN_OVERLAP)      # overlap.cpp:110, as fgChainMinUnique computes it
NONE, FREE, SURVIVOR, FULL = 0, 1, 2, 3


def screen_hash(rec):
    """fg_overlap.hip screen_hash: the slot a record's walk through the set starts at"""
    return ((int(rec) * 0x9E3779B1) & 0xFFFFFFFF) >> 23


# ---- the statement ----------------------------------------------------------------------------------------------------
def _reason(rec, cur, tie_free, min_unique, min_overlap, cap):
    """one query: records and query positions of its hits in emission order -> reason word"""
    n = len(rec)
    if tie_free or not (SORT_CAP < n <= RADIX_MAX):
        return NONE
    tie = np.zeros(n, bool)
    tie[1:] = (rec[1:] == rec[:-1]) & (cur[1:] == cur[:-1])
    ids = np.unique(rec[tie])
    if len(ids) > cap:
        return FULL
    member = np.isin(rec, ids)
    slot = np.searchsorted(ids, rec[member])
    uniq = np.bincount(slot, weights=~tie[member], minlength=len(ids)).astype(np.int64)
    lo = np.full(len(ids), np.iinfo(np.int64).max)
    hi = np.full(len(ids), -1)
    np.minimum.at(lo, slot, cur[member])
    np.maximum.at(hi, slot, cur[member])
    survives = (uniq.astype(np.float32) >= np.float32(min_unique)) & (hi - lo >= min_overlap)
    return SURVIVOR if survives.any() else FREE


def order_free(counts, hits, min_unique, min_overlap, cap=CAP):
    """What k_sort_screen says per query, from exported seed hits (query after query, each in emission order)."""
    off = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    flags = _tie_free_from_hits(counts, hits)
    out = np.zeros(len(counts), np.uint32)
    for i in range(len(counts)):
        h = hits[off[i]:off[i + 1]]
        out[i] = _reason(h["ext_id"].astype(np.int64), h["cur_pos"].astype(np.int64), flags[i], min_unique, min_overlap, cap)
    return out


def order_free_keys(keys, off, cur_bits, flags, min_unique, min_overlap, cap=CAP):
    """the same over crafted 32-bit keys rec << cur_bits | cur"""
    out = np.zeros(len(off) - 1, np.uint32)
    for i in range(len(off) - 1):
        k = keys[int(off[i]):int(off[i + 1])].astype(np.int64)
        out[i] = _reason(k >> cur_bits, k & ((1 << cur_bits) - 1), flags[i], min_unique, min_overlap, cap)
    return out


def full_prefilter_keeps_a_tied_group(h, cur_len, length, min_overlap, max_overhang):
    """one query's hits: does the reference's prefilter (flye_oracle.cpp:713-736, no forceLocal) keep a group that holds
    two hits of one (ext_id, cur_pos)?"""
    ext_id, cur, ext = h["ext_id"].astype(np.int64), h["cur_pos"].astype(np.int64), h["ext_pos"].astype(np.int64)
    order = np.lexsort((cur, ext_id))                   # the prefilter's figures do not depend on the order of ties
    ext_id, cur, ext = ext_id[order], cur[order], ext[order]
    starts = np.concatenate([[0], np.nonzero(np.diff(ext_id))[0] + 1, [len(ext_id)]])
    for a, b in zip(starts[:-1], starts[1:]):
        c, e = cur[a:b], ext[a:b]
        if not np.any(c[1:] == c[:-1]):
            continue
        unique = int(np.count_nonzero(np.diff(np.concatenate([[0], c]))))        # prev starts at 0
        if np.float32(unique) < np.float32(0.01) * np.float32(min_overlap):
            continue
        if c[-1] - c[0] < min_overlap or e.max() - e.min() < min_overlap:
            continue
        if max_overhang > 0:
            if min(c[0], e.min()) > max_overhang:
                continue
            if min(cur_len - c[-1], int(length[ext_id[a] >> 1]) - e.max()) > max_overhang:
                continue
        return True
    return False


# ---- crafted segments ---------------------------------------------------------------------------------------------------
FILL = 20000 + np.arange(977)       # records of the filler hits: never tied, never a group of the case


def craft(n, groups, cur_bits=16, fill=FILL):
    """n keys in emission order: the hits of ``groups`` ([(record, [cur, ...])], a repeated cur is a tie) and filler
    hits of distinct (record, cur) from ``fill``; ascending cur, equal keys neighbours"""
    rec = [np.full(len(c), r, np.int64) for r, c in groups]
    cur = [np.asarray(c, np.int64) for _, c in groups]
    m = n - sum(len(c) for c in cur)
    assert m >= 0
    j = np.arange(m, dtype=np.int64)
    span = min(60000, (1 << cur_bits) - 1)
    rec.append(np.asarray(fill, np.int64)[j % len(fill)])
    cur.append((j * 61) % span)
    rec, cur = np.concatenate(rec), np.concatenate(cur)
    assert not set(int(r) for r, _ in groups) & set(int(f) for f in fill)
    assert not len(cur) or cur.max() < (1 << cur_bits)
    order = np.lexsort((rec, cur))
    return ((rec[order] << cur_bits) | cur[order]).astype(np.uint32)


def spread(count, span, first=100):
    """count distinct positions from ``first`` to ``first + span``"""
    return list(np.unique(np.linspace(first, first + span, count).astype(np.int64)))


def group(rec, distinct, span, ties=1, first=100, tie_at_end=False):
    """a group on ``distinct`` positions over ``span`` with ``ties`` extra hits, each on a position another hit has"""
    pos = spread(distinct, span, first)
    assert len(pos) == distinct and pos[-1] - pos[0] == span
    extra = [pos[-1]] * ties if tie_at_end else [pos[i % distinct] for i in range(ties)]
    return (rec, pos + extra)


def colliding_records():
    """two records below 2^16 that start their walk at one slot"""
    seen = {}
    for r in range(1, 20000):
        h = screen_hash(r)
        if h in seen:
            return seen[h], r
        seen[h] = r
    raise AssertionError


def _planted(n, j_list, big, run=2):
    """n hits on ascending distinct positions (every eighth of record ``big``: 10+ positions over more than MIN_OVERLAP
    when big is not None), hit j made equal to the ``run - 1`` hits before it for each j listed"""
    j = np.arange(n, dtype=np.int64)
    cur = j * 4
    rec = 1000 + (j % 500)
    if big is not None:
        rec = np.where(j % 8 == 0, big, rec)
    for p in j_list:
        rec[p - run + 1:p + 1] = big if big is not None else 77
        cur[p - run + 1:p + 1] = cur[p - run + 1]
    return ((rec << 16) | cur).astype(np.uint32)


def _cases():
    """name -> (segments, cur_bits, rec_bits, expected reason per segment or None where only the statement speaks);
    a segment is (keys, tie-free flag)"""
    a, b = colliding_records()
    n0 = 600
    out = {}
    out["thresholds"] = ([
        (craft(n0, [group(5, 9, 2000)]), 0),                     # uniq == minSize - 1
        (craft(n0, [group(5, 10, 2000)]), 0),                    # uniq == minSize
        (craft(n0, [group(5, 9, 2000, ties=3)]), 0),             # 12 hits on 9 positions: size passes, uniq does not
        (craft(n0, [group(5, 15, MIN_OVERLAP - 1)]), 0),
        (craft(n0, [group(5, 15, MIN_OVERLAP)]), 0),
        (craft(n0, [group(5, 10, 2000, tie_at_end=True)]), 0),   # nine untied hits, then the only tie: ten positions
        (craft(n0, [group(5, 30, 3000), group(6, 3, 5000)]), 0),
        (craft(n0, [group(5, 30, 900), group(6, 3, 5000), group(9, 9, 4000, ties=5)]), 0),
    ], 16, 16, [FREE, SURVIVOR, FREE, FREE, SURVIVOR, SURVIVOR, SURVIVOR, FREE])
    n1 = 2 * TILE + 52
    places = [1, 63, 64, 65, 2 * 64, WG - 1, WG, WG + 1, 2 * WG, TILE - 1, TILE, TILE + 1, TILE + WG, 2 * TILE, n1 - 1]
    out["tie_positions"] = (
        [(_planted(n1, [p], 7), 0) for p in places] + [(_planted(n1, [p], None), 0) for p in places] +
        [(_planted(n1, [p], 7, run=3), 0) for p in (2, 64, 65, WG, WG + 1, TILE, TILE + 1, n1 - 1)] +
        [(_planted(n1, [1, n1 - 1], 7), 0), (_planted(n1, [], 7), 0)],
        16, 16, [SURVIVOR] * len(places) + [FREE] * len(places) + [SURVIVOR] * 8 + [SURVIVOR, FREE])
    small = lambda r, at: (r, [at, at])                          # noqa: E731  one tied pair: one position
    out["capacity"] = ([
        (craft(2000, [small(100 + i, 10 + 7 * i) for i in range(CAP)]), 0),
        (craft(2000, [small(100 + i, 10 + 7 * i) for i in range(CAP + 1)]), 0),
        (craft(2000, [small(100 + i, 10 + 7 * i) for i in range(CAP - 1)] + [group(9000, 12, 1500)]), 0),
        (craft(2000, [small(100 + i, 10 + 7 * i) for i in range(CAP + 1)] + [group(9000, 12, 1500)]), 0),
        (craft(4000, [small(100 + i, 10 + 7 * i) for i in range(2 * SLOTS + 3)]), 0),      # more than the set has slots
    ], 16, 16, [FREE, FULL, SURVIVOR, FULL, FULL])
    out["collisions"] = ([
        (craft(n0, [small(a, 500), small(b, 700)]), 0),
        (craft(n0, [group(a, 12, 1500), small(b, 700)]), 0),
        (craft(n0, [small(a, 500), group(b, 12, 1500)]), 0),
        (craft(n0, [group(a, 12, 900), group(b, 9, 3000)]), 0),
    ], 16, 16, [FREE, SURVIVOR, SURVIVOR, FREE])
    keep = [group(5, 12, 1500)]
    out["sizes"] = ([(craft(n, keep), 0) for n in (SORT_CAP, SORT_CAP + 1, RADIX_MAX, RADIX_MAX + 1)] +
                    [(craft(0, []), 0), (craft(1, []), 0), (craft(n0, []), 1), (craft(n0, []), 0)],
                    16, 16, [NONE, SURVIVOR, SURVIVOR, NONE, NONE, NONE, NONE, FREE])
    out["flagged"] = ([(craft(n0, []), 1), (craft(n0, keep), 0), (craft(5000, []), 1)], 16, 16, [NONE, SURVIVOR, NONE])
    f9 = 300 + np.arange(200)
    out["rec_bits_9"] = ([(craft(n0, [group(511, 12, 1500)], 16, f9), 0), (craft(n0, [group(511, 9, 1500)], 16, f9), 0)],
                         16, 9, [SURVIVOR, FREE])
    top = (1 << 17) - 1
    f17 = (1 << 16) + np.arange(977)
    out["rec_bits_17"] = ([(craft(n0, [group(top, 12, 1500)], 15, f17), 0), (craft(n0, [group(top, 9, 1500)], 15, f17), 0),
                           (craft(n0, [group(top - (1 << 16), 9, 1500), group(top, 3, 1500)], 15, f17), 0)],
                          15, 17, [SURVIVOR, FREE, FREE])
    # a first position of 0 is one the reference's count (prev starts at 0) leaves out: nine there, ten here
    out["first_cur_0"] = ([(craft(n0, [group(5, 10, 2000, first=0)]), 0)], 16, 16, None)
    return out


CASES = ["thresholds", "tie_positions", "capacity", "collisions", "sizes", "flagged", "rec_bits_9", "rec_bits_17",
         "first_cur_0"]


def _arrays(segments):
    keys = np.concatenate([k for k, _ in segments]) if segments else np.empty(0, np.uint32)
    off = np.concatenate([[0], np.cumsum([len(k) for k, _ in segments])]).astype(np.uint64)
    return keys, off, np.asarray([f for _, f in segments], np.uint32)


@pytest.mark.parametrize("name", CASES)
def test_crafted_cases_are_what_they_say(name):
    """CPU: emission order, the flags and the expected reason words, by the statement"""
    segments, cur_bits, rec_bits, want = _cases()[name]
    keys, off, flags = _arrays(segments)
    assert int(keys.max() >> cur_bits) < (1 << rec_bits)
    for i, (k, f) in enumerate(segments):
        cur = k.astype(np.int64) & ((1 << cur_bits) - 1)
        assert np.all(np.diff(cur) >= 0), (name, i)
        distinct = len(np.unique(k))
        assert distinct == (1 + np.count_nonzero(np.diff(k)) if len(k) else 0), (name, i)      # equal keys are neighbours
        assert not f or distinct == len(k), (name, i)                                           # a flag promises no tie
    got = order_free_keys(keys, off, cur_bits, flags, MIN_UNIQUE, MIN_OVERLAP)
    if want is not None:
        assert list(got) == want
    else:
        assert list(got) == [SURVIVOR]          # conservative: the reference would count nine positions and drop it


# ---- the read set -----------------------------------------------------------------------------------------------------------
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
    counts, hits = _cpu_seed_hits(rs, o.export_index(), k, q)
    return dict(rs=rs, cfg=cfg, k=k, o=o, q=q, counts=counts, hits=hits,
                reasons=order_free(counts, hits, MIN_UNIQUE, MIN_OVERLAP))


def test_read_set_has_all_three_kinds_and_the_claim_holds(world):
    """CPU: tie-free, tied-but-order-free and must-emulate queries all occur, and in every query the statement passes
    the reference's full prefilter drops each group that holds a tie"""
    rs, cfg, q, counts, hits, reasons = (world[f] for f in ("rs", "cfg", "q", "counts", "hits", "reasons"))
    n = counts.astype(np.int64)
    assert len(q) == 844 and n.min() > SORT_CAP and n.max() <= RADIX_MAX
    off = np.concatenate([[0], np.cumsum(n)])
    flags = _tie_free_from_hits(counts, hits)
    max_overhang = int(cfg["maximum_overhang"])
    kept = np.array([flags[i] == 0 and full_prefilter_keeps_a_tied_group(hits[off[i]:off[i + 1]], int(rs.length[int(q[i]) >> 1]),
                                                                         rs.length, MIN_OVERLAP, max_overhang)
                     for i in range(len(q))])
    full_free = (flags == 0) & ~kept
    print(f"{len(q)} queries: {int(flags.sum())} tie-free; full prefilter: {int(full_free.sum())} tied but order-free, "
          f"{int(kept.sum())} need the emulation; the kernel's rule: {int((reasons == FREE).sum())} order-free, "
          f"{int((reasons == SURVIVOR).sum())} with a tied group that may survive, {int((reasons == FULL).sum())} over the cap")
    assert np.array_equal(reasons == NONE, flags == 1)
    assert int(flags.sum()) > 0 and int(kept.sum()) > 0
    assert int((reasons == FREE).sum()) >= 50
    assert not np.any((reasons == FREE) & kept)                 # soundness: what the screen passes, the prefilter drops
    assert int((reasons == FREE).sum()) <= int(full_free.sum())


# ---- fg_debug_sort_screen -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def screen_ctx(built):
    from flye_amd import gpu
    ctx = gpu.Context(17, 0)
    yield ctx
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_screen_on_crafted_segments(screen_ctx, monkeypatch, name):
    for sw in ("FG_SORT_SCREEN", "FG_SORT_TIEFREE", "FG_SORT_RADIX_MAX"):
        monkeypatch.delenv(sw, raising=False)
    segments, cur_bits, rec_bits, want = _cases()[name]
    keys, off, flags = _arrays(segments)
    got = screen_ctx.debug_sort_screen(keys, off, cur_bits, rec_bits, flags, MIN_UNIQUE, MIN_OVERLAP)
    stated = order_free_keys(keys, off, cur_bits, flags, MIN_UNIQUE, MIN_OVERLAP)
    print(f"{name}: kernel {list(got)}, statement {list(stated)}")
    if want is None:
        # only "kernel passes => statement passes" is asked of a group that starts at position 0
        assert all(g in (FREE, SURVIVOR) and (g != FREE or s == FREE) for g, s in zip(got, stated))
        return
    assert list(got) == list(stated) == want


@pytest.mark.gpu
def test_screen_feeds_the_radix_path_and_the_order_is_a_sorted_one(screen_ctx, monkeypatch):
    """sortSegments with the screen's verdict as flags: passed segments take the radix path and come out sorted by key,
    ties in emission order"""
    for sw in ("FG_SORT_SCREEN", "FG_SORT_TIEFREE", "FG_SORT_RADIX_MAX"):
        monkeypatch.delenv(sw, raising=False)
    segments, cur_bits, rec_bits, _ = _cases()["thresholds"]
    keys, off, flags = _arrays(segments)
    reason = screen_ctx.debug_sort_screen(keys, off, cur_bits, rec_bits, flags, MIN_UNIQUE, MIN_OVERLAP)
    free = (flags != 0) | (reason == FREE)
    k, v, segs, hits = screen_ctx.debug_sort_pairs32(keys, off, cur_bits, rec_bits, free.astype(np.uint32))
    assert segs == int(free.sum()) == screen_ctx.debug_sort_radix_segments() and segs > 0
    for i in np.nonzero(free)[0]:
        a, b = int(off[i]), int(off[i + 1])
        perm = np.argsort(keys[a:b], kind="stable")
        assert np.array_equal(v[a:b], perm) and np.array_equal(k[a:b], keys[a:b][perm])


# ---- end to end -----------------------------------------------------------------------------------------------------------
def _detector(ctx, vi, cfg, repeat_stage):
    from flye_amd import gpu
    if not repeat_stage:
        return gpu.OverlapDetector.for_assemble(ctx, vi, cfg, MIN_OVERLAP)
    # the repeat stage's detector form: every overlap of a pair, kmerMatches kept
    return gpu.OverlapDetector(ctx, vi, int(cfg["maximum_jump"]), MIN_OVERLAP, int(cfg["maximum_overhang"]), True, False, 1.0,
                               bool(cfg["reads_base_alignment"]), False, bool(cfg["hpc_scoring_on"]))


def _run_overlaps():
    """both detector forms on the read set -> (live objects of the assemble form, arrays to compare)"""
    from flye_amd import config, gpu
    rs = _reads()
    cfg = config.preset("raw")
    ctx = gpu.Context(int(cfg["kmer_size"]), 0)
    ctx.set_reads(rs)
    vi = gpu.VertexIndex(ctx, float(int(cfg["assemble_kmer_sample"])))
    vi.build(cfg)
    q = _all_queries(rs)
    out, live = {}, {}
    for form in ("repeat", "assemble"):
        det = _detector(ctx, vi, cfg, form == "repeat")
        res = det.getSeqOverlapsBatch(q)
        times = ctx.kernel_times()                      # of this call
        out.update({form + "_recs": np.frombuffer(res.recs.tobytes(), np.uint8), form + "_query_off": res.query_off,
                    form + "_stat_off": res.stat_off, form + "_stats": res.stats.view(np.uint32),
                    form + "_counters": np.array([res.query_kmers, res.seed_hits, res.dp_groups, res.dp_elements,
                                                  res.dp_elements_small], np.uint64),
                    form + "_launches": np.array([times.get("k_sort_radix", (0.0, 0))[1], times.get("k_sort_screen", (0.0, 0))[1]],
                                                 np.uint64)})
        if form == "repeat":
            out["repeat_match_off"], out["repeat_matches"] = res.match_off, np.ascontiguousarray(res.matches)
        live[form] = (det, res)
    return ctx, live, out


FIELDS = ["recs", "query_off", "stat_off", "stats", "counters"]


def _child_main(out_path):
    sys.path.insert(0, ROOT)
    ctx, _, out = _run_overlaps()
    np.savez(out_path, **out)
    ctx.close()


if __name__ == "__main__":
    _child_main(sys.argv[1])
    sys.exit(0)


def _child(tmp_path, switch):
    out = str(tmp_path / f"{switch}.npz")
    env = dict(os.environ)
    for sw in ("FG_SORT_SCREEN", "FG_SORT_TIEFREE", "FG_SORT_RADIX_MAX"):
        env.pop(sw, None)
    env[switch] = "0"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out)


@pytest.fixture(scope="module")
def runs(world, tmp_path_factory):
    """the default in this process (context kept open for the hooks), each switch in a fresh child process"""
    saved = {sw: os.environ.pop(sw) for sw in ("FG_SORT_SCREEN", "FG_SORT_TIEFREE", "FG_SORT_RADIX_MAX", "FG_HIT_BUDGET",
                                               "FG_KMER_BUDGET", "FG_LANE_MIN_HITS", "FG_FORCE_KEY64") if sw in os.environ}
    ctx, live, on = _run_overlaps()
    tmp = tmp_path_factory.mktemp("sort_screen")
    yield dict(ctx=ctx, live=live, on=on, screen_off=_child(tmp, "FG_SORT_SCREEN"), tiefree_off=_child(tmp, "FG_SORT_TIEFREE"))
    ctx.close()
    os.environ.update(saved)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["assemble", "repeat"])
def test_overlaps_identical_with_the_screen_on_and_off(world, runs, form):
    from oracle import oracle as O
    from helpers import check_overlaps_equal
    on = runs["on"]
    fields = FIELDS + (["match_off", "matches"] if form == "repeat" else [])
    for other in ("screen_off", "tiefree_off"):
        for f in fields:
            assert np.asarray(on[f"{form}_{f}"]).tobytes() == runs[other][f"{form}_{f}"].tobytes(), (other, f)
    assert len(on[form + "_recs"]) > 0
    radix, screen = (int(x) for x in on[form + "_launches"])
    assert radix > 0 and screen > 0
    assert [int(x) for x in runs["screen_off"][form + "_launches"]] == [radix, 0]
    assert [int(x) for x in runs["tiefree_off"][form + "_launches"]] == [0, 0]
    params = O.detector_params(world["cfg"], min_overlap=MIN_OVERLAP, only_max_ext=form == "assemble",
                               keep_alignment=form == "repeat")
    check_overlaps_equal(runs["live"][form][1], world["o"].overlaps(params, world["q"]), form == "repeat")


@pytest.mark.gpu
def test_reason_words_equal_the_statement_and_count_the_radix_segments(world, runs):
    from flye_amd import gpu
    ctx, q = runs["ctx"], world["q"]
    det = runs["live"]["assemble"][0]                    # the last call on the context
    q0, reasons = ctx.debug_order_free(len(q))
    t0, flags = ctx.debug_tie_free(len(q))
    segs = ctx.debug_sort_radix_segments()
    assert q0 == t0 == 0 and len(reasons) == len(flags) == len(q)          # one sub-range: the whole call
    counts, ptr, n = det.probe_hits(q)
    hits = gpu.seed_hits_to_host(ptr, n)
    want = order_free(counts, hits, MIN_UNIQUE, MIN_OVERLAP)
    share = {r: (int((want == r).sum()), float(counts[want == r].sum()) / float(counts.sum())) for r in (NONE, FREE, SURVIVOR, FULL)}
    print(f"{len(q)} queries, (queries, share of hits) per reason: {share}")
    assert np.array_equal(reasons, want)
    assert np.array_equal(want, world["reasons"]) and np.array_equal(counts, world["counts"])      # the CPU statement's run
    size = counts.astype(np.int64)
    in_range = (size > SORT_CAP) & (size <= RADIX_MAX)
    assert segs == int((in_range & (flags == 1)).sum()) + int((in_range & (reasons == FREE)).sum())
    assert int((reasons == FREE).sum()) >= 50
