"""The device path at k-mer sizes other than 17.

Everything else under tests/ builds its context with k = 17: the narrow lookup table, 5 radix passes of the index
sort, key bins cut at bit 22, the direct counter.  Here: the wide table of k >= 18 ({key, index} slots probed one at a
time, its repetitive marker, the imported-index search), k-mer extraction at other widths (k = 32 included), the sort
over 2k key bits, the bins of binShiftFor(k) under every sharded layout, the counter below 17 in both forms, and what
carries k downstream (L - k k-mers per read, the rc position, curEnd, the chaining score and jump terms).

(a) the reference's own vectors (tests/golden/make_golden.py, cases with k != 17) through the device; (b)-(h) the
device against the CPU oracle, which tests/test_oracle_golden.py and tests/test_oracle_vs_ref.py pin to the reference
at k = 11, 13, 15, 18, 25, 31.  k = 16 and k = 32 rest on the oracle alone (at 32 the reference's k-mer mask
1 << 2k is undefined); nothing below 11 is tested."""
import functools

import numpy as np
import pytest

from helpers import (bits_to_float, canonical_kmers, case_config, case_queries, check_index_stats, check_overlaps_equal,
                     check_repeat_stage_result, edges_setup, golden_lines, golden_queries, golden_reads, index_digest,
                     repeat_stage_setup)
from test_gpu_parity import _gpu_setup, _same_index
from test_group import _params, _same

pytestmark = pytest.mark.gpu

STAT_FIELDS = ("total_kmers", "selected_kmers", "index_entries", "repetitive_kmers", "repetitive_frequency")


# ---- shared inputs: about 0.6 Mbp of reads each, made once -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reads(kind, seed, genome_len=30_000, coverage=20, read_seed=0):
    from flye_amd import synth
    return synth.simulate(seed=seed, genome_len=genome_len, coverage=coverage, kind=kind, n_repeat_families=4,
                          n_tandems=3, n_homopolymers=3, read_seed=read_seed).filter_min_len(1000)


def _cfg(preset, k):
    from flye_amd import config
    return dict(config.preset(preset), kmer_size=float(k))


def _mixed(n_reads, first=0):
    """every read once, the strands alternating"""
    i = np.arange(n_reads)
    return (first + 2 * i + (i & 1)).astype(np.uint32)


def _oracle(rs, cfg, first=0):
    from oracle import oracle as O
    o = O.Oracle(int(cfg["kmer_size"]))
    o.set_reads(rs, first)
    return o, o.build_index(cfg)


def _reach(ctx, build_times, res):
    """the kernels the test is about did run, on something: the table insert of the build, the probe and the chaining
    DP of the overlap call (kernel_times() holds the last call's launches)"""
    assert "k_table_insert" in build_times, sorted(build_times)
    kt = ctx.kernel_times()
    assert "k_probe" in kt, sorted(kt)
    assert {"k_chain_small", "k_chain_dp"} & set(kt), sorted(kt)
    assert len(res.recs) > 0 and res.seed_hits > 0


def _same_stats(gst, ost):
    for f in STAT_FIELDS:
        assert gst[f] == ost[f], (f, gst[f], ost[f])
    assert np.float32(gst["sample_rate"]).tobytes() == np.float32(ost["sample_rate"]).tobytes()


def _entries_decode_to_keys(ex, rs, k):
    """every index entry (record << 32 | position on the record's strand) names a k-mer whose canonical form, taken
    from the packed reads by helpers.canonical_kmers, is the entry's key: the extraction at width k and the
    reverse-complement position len - pos - k, without the oracle"""
    canon = [canonical_kmers(rs, r, k) for r in range(rs.n)]
    start = np.zeros(rs.n + 1, np.int64)
    start[1:] = np.cumsum([len(c) for c in canon])
    canon = np.concatenate(canon)
    rec = (ex.entries >> np.uint64(32)).astype(np.int64)
    pos = (ex.entries & np.uint64(0xFFFFFFFF)).astype(np.int64)
    read = rec >> 1
    L = rs.length[read].astype(np.int64)
    q = np.where(rec & 1, L - pos - k, pos)
    assert np.all((q >= 0) & (q < L - k))              # the read's last k-mer is never indexed (kmer.h:193-198)
    key_of_entry = np.repeat(ex.keys, np.diff(ex.key_off.astype(np.int64)))
    assert len(key_of_entry) == len(ex.entries) > 0
    assert np.array_equal(canon[start[read] + q], key_of_entry)


def _bytes(res):
    return (res.recs.tobytes(), res.query_off.tobytes(), res.stat_off.tobytes(), res.stats.tobytes(), res.seed_hits,
            res.query_kmers, res.dp_groups, res.dp_elements)


# ---- (a) the reference's vectors through the device ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["subasm", "subasm_rc_max", "corrected_k18", "raw_k15"])
def test_golden_reference_vectors(built, golden_cases, name):
    case = golden_cases[name]
    rs = golden_reads(case)
    cfg = case_config(case)
    ctx, vi, st, det = _gpu_setup(rs, cfg)
    build_times = ctx.kernel_times()
    assert ctx.k == int(cfg["kmer_size"]) != 17
    check_index_stats(st, case["index"])
    assert index_digest(vi.export()) == case["index"]["sha256"]
    det.p.max_divergence = bits_to_float(case["max_div_bits"])
    res = det.getSeqOverlapsBatch(case_queries(case, rs.n), maxOverlaps=case.get("max_overlaps", 0))
    assert res.lines() == golden_lines(name)
    assert len(res.recs) == case["n_overlaps"]
    _reach(ctx, build_times, res)
    if name != "raw_k15":
        assert st["repetitive_kmers"] > 0         # the wide probe's repetitive marker is looked up
    ctx.close()


def test_read_aligner_style_golden_subasm(built, golden_cases):
    """edges_subasm_aln: reads of a second container against an index of edge sequences at k = 31, every primary,
    kmerMatches kept (count and digest of every list are part of the vectors' lines)"""
    from flye_amd import gpu
    from oracle import oracle as O
    case = golden_cases["edges_subasm_aln"]
    edges, reads = golden_reads(case), golden_queries(case)
    cfg = case_config(case)
    wnd, dk = edges_setup(case, cfg)
    k = int(cfg["kmer_size"])
    ctx = gpu.Context(k, 0)
    ctx.set_reads(edges, 0)
    vi = gpu.VertexIndex(ctx, float(int(cfg["assemble_kmer_sample"])))
    st = vi.buildIndexMinimizers(1, wnd, cfg["repeat_kmer_rate"])
    build_times = ctx.kernel_times()
    check_index_stats(st, case["index"])
    assert index_digest(vi.export()) == case["index"]["sha256"]
    ctx.set_queries(reads, 2 * edges.n)
    det = gpu.OverlapDetector(ctx, vi, int(cfg["maximum_jump"]), dk["min_overlap"], dk["max_overhang"], True,
                              dk["only_max_ext"], 1.0, dk["nucl_alignment"], False, bool(cfg["hpc_scoring_on"]))
    q = (2 * edges.n + np.arange(0, 2 * reads.n)).astype(np.uint32)      # both strands
    res = det.getSeqOverlapsBatch(q)
    lines = res.lines()
    fwd = np.nonzero(res.query_ids % 2 == 0)[0]
    assert [l for i in fwd for l in lines[int(res.query_off[i]):int(res.query_off[i + 1])]] == golden_lines(case["name"])
    _reach(ctx, build_times, res)
    o = O.Oracle(k)
    o.set_reads(edges, 0)
    o.build_index_minimizers(1, wnd, cfg["repeat_kmer_rate"])
    o.set_queries(reads, 2 * edges.n)
    check_overlaps_equal(res, o.overlaps(O.detector_params(cfg, **dk), q), True)
    ctx.close()


def test_repeat_stage_golden_subasm(built, golden_cases):
    """repeat_subasm: the RepeatGraph::build flag set at k = 31; the unmarked records are the reference's, the marks
    (needs_trim) and the kmerMatches the oracle's"""
    from flye_amd import gpu
    from oracle import oracle as O
    case = golden_cases["repeat_subasm"]
    seqs = golden_reads(case)
    cfg = case_config(case)
    wnd, dk = repeat_stage_setup(case, cfg)
    k = int(cfg["kmer_size"])
    ctx = gpu.Context(k, 0)
    ctx.set_reads(seqs, 0)
    vi = gpu.VertexIndex(ctx, float(int(cfg["assemble_kmer_sample"])))
    st = vi.buildIndexMinimizers(1, wnd, cfg["repeat_kmer_rate"])
    build_times = ctx.kernel_times()
    check_index_stats(st, case["index"])
    assert index_digest(vi.export()) == case["index"]["sha256"]
    det = gpu.OverlapDetector(ctx, vi, int(cfg["maximum_jump"]), dk["min_overlap"], dk["max_overhang"], True,
                              dk["only_max_ext"], dk["max_divergence"], dk["nucl_alignment"], True,
                              bool(cfg["hpc_scoring_on"]))
    q = np.arange(0, 2 * seqs.n, dtype=np.uint32)
    res = det.getSeqOverlapsBatch(q)
    _reach(ctx, build_times, res)
    o = O.Oracle(k)
    o.set_reads(seqs, 0)
    o.build_index_minimizers(1, wnd, cfg["repeat_kmer_rate"])
    ores = o.overlaps(O.detector_params(cfg, **dk), q)
    check_overlaps_equal(res, ores, True)
    assert np.array_equal(res.needs_trim, ores.needs_trim)
    check_repeat_stage_result(det.getSeqOverlapsBatch(q[::2]), case, golden_cases)
    ctx.close()


# ---- (b) minimizer builds over the widths, against the oracle -------------------------------------------------------------
SWEEP = [
    (11, "corrected", "hifi", dict(max_overlaps=6)),
    (11, "hifi", "hifi03", dict()),
    (15, "corrected", "hifi03", dict()),
    (15, "hifi", "hifi", dict()),
    (16, "corrected", "hifi", dict()),
    (16, "hifi", "hifi03", dict(keep_aln=True)),
    (18, "corrected", "hifi03", dict(keep_aln=True)),
    (18, "hifi", "hifi", dict()),
    (24, "corrected", "hifi", dict()),
    (24, "hifi", "hifi03", dict(max_overlaps=6)),
    (31, "corrected", "hifi03", dict()),
    (31, "hifi", "hifi", dict(keep_aln=True, all_primaries=True)),
]


def _minimizer_parity(k, preset, kind, opts):
    from oracle import oracle as O
    rs = _reads(kind, 300 + k)
    cfg = _cfg(preset, k)
    ctx, vi, gst, det = _gpu_setup(rs, cfg)
    build_times = ctx.kernel_times()
    assert ctx.k == k
    keep, mo = bool(opts.get("keep_aln")), opts.get("max_overlaps", 0)
    det.p.max_divergence = 0.05
    det.p.only_max_ext = 0 if opts.get("all_primaries") else 1
    det.p.keep_alignment = int(keep)
    o, ost = _oracle(rs, cfg)
    ex = vi.export()
    assert _same_index(ex, o.export_index())
    _entries_decode_to_keys(ex, rs, k)
    _same_stats(gst, ost)
    q = _mixed(rs.n)
    gres = det.getSeqOverlapsBatch(q, maxOverlaps=mo)
    _reach(ctx, build_times, gres)
    ores = o.overlaps(O.detector_params(cfg, max_divergence=0.05, only_max_ext=not opts.get("all_primaries"),
                                        keep_alignment=keep), q, max_overlaps=mo)
    check_overlaps_equal(gres, ores, keep, counts=not mo)      # with a limit the reference stops visiting groups early
    # any sub-batch gives the same per-read lists
    sub = q[5:40:3]
    part = det.getSeqOverlapsBatch(sub, maxOverlaps=mo)
    pos = {int(x): i for i, x in enumerate(q)}
    for j, rid in enumerate(sub):
        a, b = part.of(j), gres.of(pos[int(rid)])
        assert a.tobytes() == b.tobytes()
        if keep:
            ia, ib = int(part.query_off[j]), int(gres.query_off[pos[int(rid)]])
            for t in range(len(a)):
                assert np.array_equal(part.kmerMatches(ia + t), gres.kmerMatches(ib + t))
    ctx.close()
    return gst


@pytest.mark.parametrize("k,preset,kind,opts", SWEEP)
def test_minimizer_builds_against_oracle(built, k, preset, kind, opts):
    _minimizer_parity(k, preset, kind, opts)


# ---- (c) the solid build through the counter, below 17 ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _solid_world(k):
    """pb_raw reads, the raw settings: the oracle's index and every read's records on both strands (shared, never
    modified)"""
    from oracle import oracle as O
    rs = _reads("pb_raw", 400 + k)
    cfg = _cfg("raw", k)
    o, ost = _oracle(rs, cfg)
    q = np.arange(0, 2 * rs.n, dtype=np.uint32)
    return dict(rs=rs, cfg=cfg, ost=ost, index=o.export_index(), q=q, ores=o.overlaps(O.detector_params(cfg), q))


@pytest.mark.parametrize("mode", ["direct", "hash", None])
@pytest.mark.parametrize("k", [11, 13, 15, 16])
def test_solid_build_counter_forms(built, monkeypatch, k, mode):
    """KmerCounter as a direct-addressed array of 4^k counters and as a hashed table, forced and as the library picks
    by itself (direct at 11, hashed from 13 on at this size)"""
    w = _solid_world(k)
    if mode is None:
        monkeypatch.delenv("FG_COUNT_MODE", raising=False)
    else:
        monkeypatch.setenv("FG_COUNT_MODE", mode)
    ctx, vi, gst, det = _gpu_setup(w["rs"], w["cfg"])
    build_times = ctx.kernel_times()
    assert ctx.k == k and "k_count" in build_times
    assert _same_index(vi.export(), w["index"])
    _same_stats(gst, w["ost"])
    clear, bad = ctx.debug_probe_skip_check()
    assert bad == 0 and clear > 0          # minFreq = 2: the positions of k-mers seen once are skipped, none has a slot
    gres = det.getSeqOverlapsBatch(w["q"])
    _reach(ctx, build_times, gres)
    check_overlaps_equal(gres, w["ores"], False)
    ctx.close()


def test_solid_build_refused_above_17(built):
    """vertex_index.cpp:504-507: the flat counter holds k <= 17"""
    import ctypes as C
    from flye_amd import gpu
    rs = _reads("pb_raw", 413)
    cfg = _cfg("raw", 18)
    ctx = gpu.Context(18, 0)
    ctx.set_reads(rs)
    vi = gpu.VertexIndex(ctx, 1.0)
    with pytest.raises(gpu.FlyeGpuError) as e:
        vi.build(cfg)
    assert e.value.code == -6
    st = gpu.IndexStats()       # the library itself, not only the Python mirror of countKmers()
    assert ctx.L.fg_build_index_solid(ctx.h, 2, cfg["meta_read_top_kmer_rate"], int(cfg["meta_read_filter_kmer_freq"]),
                                      cfg["repeat_kmer_rate"], 1.0, C.byref(st)) == -6
    with pytest.raises(RuntimeError, match="-6"):
        _oracle(rs, cfg)
    ctx.close()


@pytest.mark.parametrize("k,preset,kind,seed", [(15, "raw", "pb_raw", 415), (31, "hifi", "hifi", 331)])
def test_partitioned_probes_at_other_widths(built, monkeypatch, k, preset, kind, seed):
    """FG_PROBE_PARTITION=1 is taken for the narrow table only (k <= 17): same records at 15 through the partitioned
    probe, same records at 31 where the switch is ignored"""
    rs = _reads(kind, seed)
    cfg = _cfg(preset, k)
    ctx, vi, st, det = _gpu_setup(rs, cfg)
    build_times = ctx.kernel_times()
    q = np.arange(0, 2 * rs.n, dtype=np.uint32)
    plain = det.getSeqOverlapsBatch(q)
    _reach(ctx, build_times, plain)
    assert "k_probe_emit" not in ctx.kernel_times()
    monkeypatch.setenv("FG_PROBE_PARTITION", "1")
    monkeypatch.setenv("FG_PROBE_SUB_KMERS", str(int(rs.total_bases) // 7))
    part = det.getSeqOverlapsBatch(q)
    assert ("k_probe_emit" in ctx.kernel_times()) == (k <= 17)
    assert _bytes(part) == _bytes(plain)
    ctx.close()


# ---- (d), (h) reads around k --------------------------------------------------------------------------------------------------
def _bases(rs, r):
    L = int(rs.length[r])
    w = rs.words[int(rs.word_off[r]):int(rs.word_off[r + 1])]
    sh = np.arange(32, dtype=np.uint64) * np.uint64(2)
    return ((w[:, None] >> sh[None, :]) & np.uint64(3)).reshape(-1)[:L].astype(np.uint8)


def _short_lengths(k, w):
    return sorted({k - 1, k, k + 1, k + w - 1, k + w, 63, 64, 65})


def _with_short_reads(rs, lengths, at):
    """the reads of ``rs`` followed by one piece of read 0 per length, cut at base ``at`` + 7 * i: reads that do hit
    the index where they have a k-mer at all"""
    from flye_amd import synth
    b0 = _bases(rs, 0)
    seqs = [_bases(rs, r) for r in range(rs.n)]
    seqs += [b0[at + 7 * i:at + 7 * i + L] for i, L in enumerate(lengths)]
    return synth.ReadSet.from_arrays(seqs)


def _short_read_parity(k):
    """Index reads and queries of a second container with lengths k-1, k, k+1, k+w-1, k+w, 63, 64, 65 beside normal
    reads: a read of length L has L - k k-mers (the iteration drops the last one), so k-1, k have none.  Minimum
    overlap 20 and every primary, so that the short reads do get records."""
    from flye_amd import gpu
    from oracle import oracle as O
    cfg = _cfg("hifi", k)
    w = int(cfg["minimizer_window"])
    lengths = _short_lengths(k, w)
    normal = _reads("hifi03", 500 + k, 20_000, 6)
    rs = _with_short_reads(normal, lengths, 1000)
    qs = _with_short_reads(_reads("hifi03", 500 + k, 20_000, 4, read_seed=5), lengths, 2000)
    ctx = gpu.Context(k, 0)
    ctx.set_reads(rs, 0)
    vi = gpu.VertexIndex(ctx, float(int(cfg["assemble_kmer_sample"])))
    gst = vi.build(cfg)
    build_times = ctx.kernel_times()
    o, ost = _oracle(rs, cfg)
    assert _same_index(vi.export(), o.export_index())
    _same_stats(gst, ost)
    assert gst["index_entries"] > 0
    det = gpu.OverlapDetector(ctx, vi, int(cfg["maximum_jump"]), 20, 0, True, False, 1.0, False, False, False)
    p = O.detector_params(cfg, min_overlap=20, max_overhang=0, only_max_ext=False, nucl_alignment=False, keep_alignment=True)
    p.use_hpc = 0
    length_of = {}
    for first, container in ((0, rs), (2 * rs.n, qs)):
        for i in range(container.n):
            length_of[first + 2 * i] = length_of[first + 2 * i + 1] = int(container.length[i])

    def check(q, gres, ores):
        check_overlaps_equal(gres, ores, True)
        for f in ("cur_id", "ext_id"):
            lens = np.array([length_of[int(x)] for x in gres.recs[f]])
            assert np.all(lens > k), f                                       # no record of a read without a k-mer
        cur_len = np.array([length_of[int(x)] for x in gres.recs["cur_id"]])
        ext_len = np.array([length_of[int(x)] for x in gres.recs["ext_id"]])
        return int((cur_len <= 65).sum()), int((ext_len <= 65).sum())

    # the indexed reads against themselves, both strands
    q1 = np.arange(0, 2 * rs.n, dtype=np.uint32)
    g1 = det.getSeqOverlapsBatch(q1)
    _reach(ctx, build_times, g1)
    short_cur, short_ext = check(q1, g1, o.overlaps(p, q1))
    assert short_cur > 0 and short_ext > 0          # the short reads with k-mers are found, as query and as target
    # the second container
    ctx.set_queries(qs, 2 * rs.n)
    o.set_queries(qs, 2 * rs.n)
    q2 = (2 * rs.n + np.arange(0, 2 * qs.n)).astype(np.uint32)
    g2 = det.getSeqOverlapsBatch(q2)
    short_cur, _ = check(q2, g2, o.overlaps(p, q2))
    assert short_cur > 0 and len(g2.recs) > 0
    ctx.close()


@pytest.mark.parametrize("k", [18, 31])
def test_reads_around_k(built, k):
    _short_read_parity(k)


# ---- (e) the imported index at k = 31 -------------------------------------------------------------------------------------------
def test_imported_index_wide_table(built):
    """fg_import_index builds the wide table and searches the lists for the "owns an entry" bits (k_indexed_search):
    from host arrays and from device arrays, the records are the builder's"""
    from flye_amd import gpu
    k = 31
    rs = _reads("hifi", 300 + k)
    cfg = _cfg("hifi", k)
    ctx, vi, st, det = _gpu_setup(rs, cfg)
    build_times = ctx.kernel_times()
    q = np.arange(0, 2 * rs.n, dtype=np.uint32)
    want = det.getSeqOverlapsBatch(q)
    _reach(ctx, build_times, want)
    ex = vi.export()
    counts, ptrs = vi.device_arrays()
    assert counts == (len(ex.keys), len(ex.entries), len(ex.repetitive)) and st["repetitive_kmers"] == len(ex.repetitive)
    for on_device in (False, True):
        ctx2 = gpu.Context(k, 0)
        ctx2.set_reads(rs)
        vi2 = gpu.VertexIndex(ctx2, float(int(cfg["assemble_kmer_sample"])))
        if on_device:
            vi2.import_index(counts, vi.getSampleRate(), on_device=True, ptrs=ptrs)
        else:
            vi2.import_index(ex, vi.getSampleRate())
        import_times = ctx2.kernel_times()
        assert "k_indexed_bits" in import_times
        assert _same_index(vi2.export(), ex)
        det2 = gpu.OverlapDetector.for_assemble(ctx2, vi2, cfg)
        got = det2.getSeqOverlapsBatch(q)
        _reach(ctx2, import_times, got)
        assert _bytes(got) == _bytes(want), on_device
        ctx2.close()
    ctx.close()


# ---- (f) internal cuts are invisible at k = 31 -------------------------------------------------------------------------------
def test_internal_cuts_are_invisible_wide(built, monkeypatch):
    """selection batches and sort slices of the build, k-mer and hit budgets of the overlap call, two lanes: the
    values of the k = 17 tests (test_gpu_parity.py, test_record_tail.py)"""
    k = 31
    rs = _reads("hifi", 300 + k)
    cfg = _cfg("hifi", k)
    ctx, vi, st, det = _gpu_setup(rs, cfg)
    build_times = ctx.kernel_times()
    det.p.keep_alignment = 1
    q = np.arange(0, 2 * rs.n, dtype=np.uint32)
    whole = det.getSeqOverlapsBatch(q, maxOverlaps=11)
    _reach(ctx, build_times, whole)
    base = _bytes(whole) + (whole.match_off.tobytes(), whole.matches.tobytes())
    digest = index_digest(vi.export())
    # the build in dozens of batches and slices
    monkeypatch.setenv("FG_INDEX_BATCH_KMERS", str(int(rs.total_bases) // 37))
    monkeypatch.setenv("FG_INDEX_SLICE_ENTRIES", str(max(1000, int(st["index_entries"]) // 23)))
    ctx2, vi2, st2, det2 = _gpu_setup(rs, cfg)
    monkeypatch.delenv("FG_INDEX_BATCH_KMERS")
    monkeypatch.delenv("FG_INDEX_SLICE_ENTRIES")
    assert index_digest(vi2.export()) == digest
    _same_stats(st2, st)
    det2.p.keep_alignment = 1
    cut = det2.getSeqOverlapsBatch(q, maxOverlaps=11)
    assert _bytes(cut) + (cut.match_off.tobytes(), cut.matches.tobytes()) == base
    ctx2.close()
    # the overlap call in chunks and sub-ranges, on one lane and two
    envs = [{"FG_KMER_BUDGET": str(kb), "FG_HIT_BUDGET": str(hb)} for kb, hb in ((200_000, 1 << 40), (1 << 40, 50_000), (90_000, 30_000))]
    envs.append({"FG_HIT_BUDGET": str(max(1, whole.seed_hits // 7)), "FG_KMER_BUDGET": str(1 << 30), "FG_LANES": "2"})
    for env in envs:
        for k_, v_ in env.items():
            monkeypatch.setenv(k_, v_)
        part = det.getSeqOverlapsBatch(q, maxOverlaps=11)
        assert _bytes(part) + (part.match_off.tobytes(), part.matches.tobytes()) == base, env
        for k_ in env:
            monkeypatch.delenv(k_)
    ctx.close()


# ---- (g) sharded layouts cut by the key bins of k ------------------------------------------------------------------------------
SHARDED = [(31, "hifi", "hifi", 331), (13, "raw", "pb_raw", 413)]


@pytest.mark.parametrize("k,preset,kind,seed", SHARDED)
def test_group_of_three(built, k, preset, kind, seed):
    """gpu.Group with three members on one GPU: the direct build of the target shards (key ranges cut at the bins of
    binShiftFor(k)) and the overlap stage over them, against one context field for field"""
    from flye_amd import gpu
    world = 3
    rs = _reads(kind, seed)
    cfg = _cfg(preset, k)
    rate = float(int(cfg["assemble_kmer_sample"]))
    ctx, vi, st, det = _gpu_setup(rs, cfg)
    build_times = ctx.kernel_times()
    g = gpu.Group([0] * world, k)
    g.set_reads(rs)
    gst = g.build(cfg)
    assert len(g) == world
    for f in STAT_FIELDS + ("mean_frequency", "sample_rate"):
        assert np.asarray(gst[f]).tobytes() == np.asarray(st[f]).tobytes(), (f, gst[f], st[f])
    total = 0
    for r in range(world):
        c1, v1, _, _ = _gpu_setup(rs, cfg)
        kept = v1.keep_targets(world, r)
        mv = gpu.VertexIndex(g.member(r), rate)
        assert mv.shard() == (world, r)
        assert _same_index(mv.export(), v1.export()), r
        total += kept
        c1.close()
    assert total == st["index_entries"] > 0
    p = _params(cfg)
    det.p = p
    q = _mixed(rs.n)
    want = det.getSeqOverlapsBatch(q)
    _reach(ctx, build_times, want)
    _same(g.overlaps(p, q), want)
    assert g.stats()["hits_total"] == want.seed_hits
    p2 = _params(cfg, only_max_ext=0, keep_alignment=1)
    det.p = p2
    allq = np.arange(0, 2 * rs.n, dtype=np.uint32)
    _same(g.overlaps(p2, allq, maxOverlaps=5), det.getSeqOverlapsBatch(allq, maxOverlaps=5))
    g.close()
    ctx.close()


@pytest.mark.parametrize("k,preset,kind,seed", SHARDED)
def test_key_range_pieces_and_bin_histogram(built, k, preset, kind, seed):
    """fg_index_kmer_hist: every k-mer position in the bin of its canonical k-mer's top 12 bits (bit 2k - 12 up);
    fg_index_build_range over three uneven bin ranges, one context each: every piece holds the keys of its range
    only, and the pieces put together are the one-call index"""
    from flye_amd import dist, gpu
    rs = _reads(kind, seed)
    cfg = _cfg(preset, k)
    rate = float(int(cfg["assemble_kmer_sample"]))
    ctx, vi, st, det = _gpu_setup(rs, cfg)
    build_times = ctx.kernel_times()
    one = vi.export()
    shift = np.uint64(2 * k - 12)
    hist = vi.kmer_hist()          # (on the built context: the histogram reads the reads only)
    canon = np.concatenate([canonical_kmers(rs, r, k)[:-1] for r in range(rs.n)])
    assert int(hist.sum()) == len(canon) == int(np.maximum(rs.length.astype(np.int64) - k, 0).sum())
    assert np.array_equal(hist, np.bincount((canon >> shift).astype(np.int64), minlength=4096).astype(np.uint64))
    used = np.nonzero(np.bincount((one.keys >> shift).astype(np.int64), minlength=4096))[0]
    assert len(used) > 100
    # uneven: a tenth of the used bins, half of them, the rest
    cuts = [0, int(used[len(used) // 10]), int(used[(6 * len(used)) // 10]), 4096]
    pieces, sums, members = [], np.zeros(2, np.uint64), []
    for r in range(3):
        c = gpu.Context(k, 0)
        c.set_reads(rs)
        v = gpu.VertexIndex(c, rate)
        sel = v.begin(cfg)
        assert int(sel.sum()) >= st["index_entries"]
        sums += v.build_range(cuts[r], cuts[r + 1])
        members.append((c, v))
    for r, (c, v) in enumerate(members):
        v.finish(sums)
        assert "k_table_insert" in c.kernel_times()
        piece = v.export()
        bins = (piece.keys >> shift).astype(np.int64)
        assert len(bins) > 0 and bins.min() >= cuts[r] and bins.max() < cuts[r + 1], r
        rbins = (piece.repetitive >> shift).astype(np.int64)
        assert np.all((rbins >= cuts[r]) & (rbins < cuts[r + 1])), r
        assert v.stats["repetitive_frequency"] == st["repetitive_frequency"]
        pieces.append(piece)
    assert _same_index(dist.concat_pieces(pieces), one)
    for c, _ in members:
        c.close()
    res = det.getSeqOverlapsBatch(_mixed(rs.n))
    _reach(ctx, build_times, res)
    ctx.close()


# ---- (h) k = 32: the oracle alone defines it ------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,kind,opts", [("hifi", "hifi", dict(keep_aln=True)), ("corrected", "hifi03", dict())])
def test_k32_minimizer_build_against_oracle(built, preset, kind, opts):
    """a k-mer fills the 64-bit word: no mask, fg_rev2 shifts by 0, 8 full radix passes, bins from bit 52"""
    st = _minimizer_parity(32, preset, kind, opts)
    assert st["index_entries"] > 0


def test_k32_reads_around_k(built):
    _short_read_parity(32)
