"""The flat listing of target groups and primaries (fg_overlap.hip: k_group_count_flat, k_group_fill_flat, k_group_off,
k_prim_count_flat, k_prim_gather_flat, the fgprim::scan calls between them) at the shapes where a listing by tiles of
hits can go wrong where one by queries cannot: a target shared across a query boundary, empty queries, groups and
queries that end on a tile edge, many queries in one tile, the last group of a call, several primaries per group and
scans that recurse.  Every call is compared with the oracle on the same index and with the per-query form
(FG_GROUP_FLAT=0), under the switches that change the key form and the chaining path."""
import os
import re

import numpy as np
import pytest

import chain_craft as cc
from helpers import ROOT, check_overlaps_equal, sub_index

pytestmark = pytest.mark.gpu

SETTINGS = [
    {},
    {"FG_VAL16": "0"},
    {"FG_FORCE_KEY64": "1"},
    {"FG_FORCE_KEY64": "1", "FG_PACKED_KEYS": "0"},
    {"FG_CHAIN_FUSED": "0"},
    {"FG_GROUP_FLAT": "0"},
]
SWITCHES = sorted({k for s in SETTINGS for k in s})


def _constant(source, name):
    with open(os.path.join(ROOT, "flye_amd", "csrc", source)) as f:
        m = re.search(r"constexpr int %s = (\d+);" % name, f.read())
    assert m, (source, name)
    return int(m.group(1))


T = 256 * _constant("fg_overlap.hip", "FG_GROUP_GF")                                            # hits per tile
SCAN_TILE = _constant("fg_devprim.h", "SCAN_THREADS") * _constant("fg_devprim.h", "SCAN_ITEMS")  # elements per scan tile


def _arrays(res):
    return dict(recs=res.recs.tobytes(), query_off=np.asarray(res.query_off).tobytes(),
                stats=np.asarray(res.stats).view(np.uint32).tobytes())


def _run(case, monkeypatch, q=None, totals=None, records=None):
    """Every (only_max_ext, keep_alignment, setting) call of ``case`` on the queries ``q`` (default: the declared
    ones): the oracle's records and counters, the declared totals, the same arrays as the default setting's, and
    the kernels that tell which listing ran.  ``records``: the number of records with only_max_ext on."""
    from flye_amd import config, gpu
    from oracle import oracle as O
    rs, ex = case.readset(), case.index()
    q = case.query_ids() if q is None else np.asarray(q, np.uint32)
    totals = case.totals() if totals is None else totals
    cfg = config.preset("raw")
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    ctx = gpu.Context(cc.K, 0)
    ctx.set_reads(rs, case.first_id)
    vi = gpu.VertexIndex(ctx, 1.0)
    vi.import_index(gpu.IndexExport(ex.keys, ex.key_off, ex.entries, ex.repetitive), 1.0)
    det = gpu.OverlapDetector.for_assemble(ctx, vi, cfg, min_overlap=cc.MIN_OVERLAP)
    o = O.Oracle(cc.K)
    o.set_reads(rs, case.first_id)
    o.import_index(ex, 1.0)
    for only_max in (True, False):
        for keep in (0, 1):
            ores = o.overlaps(O.detector_params(cfg, min_overlap=cc.MIN_OVERLAP, only_max_ext=only_max,
                                                keep_alignment=bool(keep)), q)
            if records is not None and only_max:
                assert len(ores.recs) == records
            det.p.only_max_ext, det.p.keep_alignment = int(only_max), keep
            first = None
            for env in SETTINGS:
                for k, v in env.items():
                    monkeypatch.setenv(k, v)
                try:
                    where = (case.name, only_max, keep, env)
                    gres = det.getSeqOverlapsBatch(q)
                    check_overlaps_equal(gres, ores, keep)
                    assert (gres.seed_hits, gres.dp_groups, gres.dp_elements) == totals, where
                    kt = ctx.kernel_times()
                    flat = "FG_GROUP_FLAT" not in env
                    assert ("k_group_scan" in kt) == (flat and totals[0] > 0), where
                    assert ("k_prim_scan" in kt) == flat, where
                    got = _arrays(gres)
                    first = got if first is None else first
                    assert got == first, where
                finally:
                    for k in env:
                        monkeypatch.delenv(k)
    ctx.close()


def _small_pair(c, **kw):
    """a query and a target of its own with one 12-hit group that reaches the DP"""
    return cc.pair(c, 1300, cc.spread(12, 1250), **kw)


def _big(n):
    """(segment length, key offsets) of a collinear n-hit group"""
    seg = n + 60
    return seg, cc.spread(n, seg - cc.K - 20)


# ---- 1. the same target across a query boundary ----------------------------------------------------------------------
def same_target_case():
    """The target is the container's first read; each of the two queries shares a segment of its own with it and
    with nothing else, so the first query's only group and the second's only group carry one target record."""
    c = cc.Case("same_target", 101)
    offs = cc.spread(12, 1250)
    S1, S2 = c.rand(1300), c.rand(1300)
    tr = c.add_read(np.concatenate([c.rand(200), S1, c.rand(100), S2, c.rand(200)]))
    Q1 = np.concatenate([c.rand(500), S1, c.rand(300)])
    Q2 = np.concatenate([c.rand(400), S2, c.rand(300)])
    q1, q2 = c.add_read(Q1), c.add_read(Q2)
    c.add_keys(Q1, 500 + offs)
    c.add_keys(Q2, 400 + offs)
    c.declare(2 * q1, 2 * tr, [(500 + o, 200 + o) for o in offs])
    c.declare(2 * q2, 2 * tr, [(400 + o, 1600 + o) for o in offs])
    return c


def test_same_target_across_a_query_boundary(built, monkeypatch):
    c = same_target_case()
    assert all(p for _, _, p in c.verdicts().values())
    _run(c, monkeypatch, records=2)


# ---- 2. empty queries ------------------------------------------------------------------------------------------------
def test_empty_queries(built, monkeypatch):
    """queries without a keyed k-mer in front of, between (two in a row) and behind the queries with hits"""
    c = cc.Case("empty_queries", 103)
    e = [2 * c.add_read(c.rand(1500)) for _ in range(2)]
    qa, _ = _small_pair(c)
    e += [2 * c.add_read(c.rand(1500)) for _ in range(2)]
    qb, _ = _small_pair(c)
    e.append(2 * c.add_read(c.rand(1500)))
    _run(c, monkeypatch, q=[e[0], 2 * qa, e[1], e[2], 2 * qb, e[3], e[4]], records=2)


def test_only_empty_queries(built, monkeypatch):
    """a call without a hit: no tile, no group, no record"""
    c = cc.Case("only_empty", 107)
    _small_pair(c)
    e = [2 * c.add_read(c.rand(1500)) for _ in range(4)]
    _run(c, monkeypatch, q=e, totals=(0, 0, 0), records=0)


# ---- 3. tile edges ---------------------------------------------------------------------------------------------------
def group_edge_case(n):
    """The call's first group has n hits; a 12-hit group of the same query on the next target and a second query
    follow.  n = T - 1, T, T + 1: the tile's last hit is the next group's head, the group's last hit, its last but one."""
    c = cc.Case("group_edge_%d" % n, 109 + n)
    seg, offs = _big(n)
    q = c.add_read(c.rand(500 + 1300 + 200 + seg + 300))
    cc.pair(c, seg, offs, left_q=2000, q_read=q)                        # the lower target id: sorted first
    cc.pair(c, 1300, cc.spread(12, 1250), left_q=500, q_read=q, t_len=1800)
    _small_pair(c)
    return c


def query_edge_case(n):
    """the same with the query boundary on the tile edge: the first query has the n-hit group only"""
    c = cc.Case("query_edge_%d" % n, 113 + n)
    seg, offs = _big(n)
    cc.pair(c, seg, offs)
    _small_pair(c)
    return c


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_group_boundary_on_a_tile_edge(built, monkeypatch, delta):
    c = group_edge_case(T + delta)
    assert all(p for _, _, p in c.verdicts().values())
    _run(c, monkeypatch, records=3)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_query_boundary_on_a_tile_edge(built, monkeypatch, delta):
    _run(query_edge_case(T + delta), monkeypatch, records=2)


# ---- 4. many queries in one tile -------------------------------------------------------------------------------------
def test_many_queries_in_one_tile(built, monkeypatch):
    c = cc.Case("many_queries", 127)
    for _ in range(40):
        _small_pair(c)
    assert c.totals()[0] == 40 * 12 < T
    _run(c, monkeypatch, records=40)


# ---- 5. the last group of the call -----------------------------------------------------------------------------------
@pytest.mark.parametrize("last", ["one_hit", "twelve_hits"])
def test_last_group_of_the_call(built, monkeypatch, last):
    """The last query has a 12-hit group and a one-hit group (never listed for the DP), in either order: the last
    group's final query position comes from the call's last hit."""
    c = cc.Case("last_group_" + last, 131)
    _small_pair(c)
    q = c.add_read(c.rand(2200))
    if last == "one_hit":
        cc.pair(c, 1300, cc.spread(12, 1250), left_q=300, q_read=q, t_len=1800)
        cc.pair(c, 100, [10], left_q=1800, q_read=q, t_len=400)
    else:
        cc.pair(c, 100, [10], left_q=1800, q_read=q, t_len=400)
        cc.pair(c, 1300, cc.spread(12, 1250), left_q=300, q_read=q, t_len=1800)
    assert sorted(n for n, _, _ in c.verdicts().values()) == [1, 12, 12]
    _run(c, monkeypatch, records=2)


# ---- 6. more than one primary per group ------------------------------------------------------------------------------
def test_tandem_shapes_with_every_primary(built, monkeypatch):
    """chain_craft.tandem_case with only_max_ext on and off (the oracle keeps one primary per group on these shapes
    either way: the groups with more are test_several_primaries_per_group's)"""
    _run(cc.tandem_case(), monkeypatch)


def test_several_primaries_per_group(built, monkeypatch):
    """chain_craft.ties_case: a target with two exact copies of the query's segment keeps two primaries with
    only_max_ext off, so the flat gather's loop over a group's primaries writes more than one record"""
    from flye_amd import config
    from oracle import oracle as O
    c = cc.ties_case()
    o = O.Oracle(cc.K)
    o.set_reads(c.readset(), c.first_id)
    o.import_index(c.index(), 1.0)
    ores = o.overlaps(O.detector_params(config.preset("raw"), min_overlap=cc.MIN_OVERLAP, only_max_ext=False), c.query_ids())
    per_group = np.unique(np.stack([ores.recs["cur_id"], ores.recs["ext_id"]]), axis=1, return_counts=True)[1]
    assert per_group.max() > 1
    _run(c, monkeypatch)


# ---- 7. scans that recurse -------------------------------------------------------------------------------------------
# workloads.ecoli_pb50 at this scale: 440 queries, 9.9 M hits = 4833 hit tiles, 52,707 groups that reach the DP -- a good
# factor of two over the 2048 elements of one scan tile (half the scale would sit at that edge); the pass takes 0.2 s
RECURSE_SCALE = 0.02


def test_recursing_scans(built, monkeypatch):
    """A pass with more hit tiles than one scan tile holds and more groups than that: both fgprim::scan calls recurse.
    The index is built on the device; the flat and the per-query form agree array by array, the first 20 queries
    agree with the oracle."""
    from flye_amd import config, gpu, workloads
    from oracle import oracle as O
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    rs = workloads.ecoli_pb50(scale=RECURSE_SCALE)[0]
    cfg = config.preset("raw")
    k = int(cfg["kmer_size"])
    ctx = gpu.Context(k, 0)
    ctx.set_reads(rs)
    vi = gpu.VertexIndex(ctx, float(int(cfg["assemble_kmer_sample"])))
    vi.build(cfg)
    det = gpu.OverlapDetector.for_assemble(ctx, vi, cfg)
    q = np.arange(0, 2 * rs.n, 2, dtype=np.uint32)
    flat = det.getSeqOverlapsBatch(q)
    kt = ctx.kernel_times()
    assert "k_group_scan" in kt and "k_prim_scan" in kt
    print(f"recursing scans: {len(q)} queries, {flat.seed_hits} hits = {flat.seed_hits / T:.0f} tiles, {flat.dp_groups} DP groups")
    assert flat.seed_hits > T * SCAN_TILE           # one sub-range (far below the hit budget): its tiles
    assert flat.dp_groups > SCAN_TILE               # the groups that pass the prefilter are a part of all groups
    monkeypatch.setenv("FG_GROUP_FLAT", "0")
    per_query = det.getSeqOverlapsBatch(q)
    monkeypatch.delenv("FG_GROUP_FLAT")
    assert "k_group_scan" not in ctx.kernel_times()
    assert _arrays(flat) == _arrays(per_query)
    assert ((flat.query_kmers, flat.seed_hits, flat.dp_groups, flat.dp_elements, flat.dp_elements_small) ==
            (per_query.query_kmers, per_query.seed_hits, per_query.dp_groups, per_query.dp_elements, per_query.dp_elements_small))
    sample = np.arange(20)
    sub = sub_index(vi.export(), rs, (q[sample] // 2).astype(np.int64), k)
    o = O.Oracle(k)
    o.set_reads(rs)
    o.import_index(sub, vi.getSampleRate())
    ores = o.overlaps(O.detector_params(cfg, min_overlap=det.p.min_overlap, max_divergence=det.p.max_divergence), q[sample])
    got = np.concatenate([flat.of(int(i)) for i in sample])
    assert len(got) == len(ores.recs) > 0
    for f in ("cur_id", "ext_id", "cur_begin", "cur_end", "cur_len", "ext_begin", "ext_end", "ext_len", "score",
              "chain_length", "filtered_positions", "edit_distance"):
        assert np.array_equal(got[f], ores.recs[f]), f
    assert np.array_equal(got["seq_divergence"].view(np.uint32), ores.recs["seq_divergence"].view(np.uint32))
    ctx.close()
