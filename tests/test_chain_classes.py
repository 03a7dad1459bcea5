"""Every chaining size class and its edges (fg_chain.hip fgChainStage) against the oracle, on the crafted
indexes of tests/chain_craft.py, under the switches that move the class boundaries.  Each call is
compared record for record with the oracle, and the chaining kernels launched are exactly the ones the
declared group sizes and the switches select -- so each class demonstrably ran, and no group is ever
listed for two paths at once."""
import numpy as np
import pytest

import chain_craft as cc
from helpers import check_overlaps_equal

pytestmark = pytest.mark.gpu

SETTINGS = [
    {},
    {"FG_CHAIN_FUSED": "0"},
    {"FG_FUSED_CAP": "64"}, {"FG_FUSED_CAP": "255"}, {"FG_FUSED_CAP": "320"}, {"FG_FUSED_CAP": "321"},
    {"FG_FUSED_CAP": "448"}, {"FG_FUSED_CAP": "1024"},
    {"FG_CHAIN_NO_SMALL_CALL": "1"},
    {"FG_CHAIN_HUGE_MIN": "100"}, {"FG_CHAIN_HUGE_MIN": "300"}, {"FG_CHAIN_HUGE_MIN": "5000"},
    {"FG_CHAIN_FUSED": "0", "FG_CHAIN_HUGE_MIN": "100"},
    {"FG_FUSED_CAP": "448", "FG_CHAIN_HUGE_MIN": "300"},
    {"FG_CHAIN_STREAMS": "1"},
    {"FG_CHAIN_STREAMS": "1", "FG_CHAIN_FUSED": "0"},
    {"FG_FORCE_KEY64": "1"},
    {"FG_FORCE_KEY64": "1", "FG_PACKED_KEYS": "0"},
    # the 64-bit hit forms where a case needs them (key33, key33_high: hit keys above 2^32 in the latter): the packed
    # sort without its narrowing, the 64-bit key + value form, and both read through the per-query listing kernels
    {"FG_NARROW_MAX": "0"},
    {"FG_PACKED_KEYS": "0"},
    {"FG_GROUP_FLAT": "0"},
    {"FG_PACKED_KEYS": "0", "FG_GROUP_FLAT": "0"},
]
SWITCHES = sorted({k for s in SETTINGS for k in s})
CHAIN_KERNELS = ("k_chain_small", "k_group_prep", "k_chain_dp", "k_chain_finish<lds256>",
                 "k_chain_finish<lds1024>", "k_chain_finish<global>")


def expected_kernels(listed, passing, env):
    """The chaining kernels fgChainStage launches for groups of these sizes (listed: n >= minSize and query
    span >= minOverlap; passing: through the prefilter) under the switches in ``env``."""
    if env.get("FG_CHAIN_FUSED") == "0":
        fused_max = 0
    elif "FG_FUSED_CAP" in env:
        fused_max = max(64, min(1024, int(env["FG_FUSED_CAP"])))
    else:
        fused_max = cc.FIN_CAP_S
    small_call = len(listed) < 65536 and "FG_CHAIN_NO_SMALL_CALL" not in env
    huge_min = int(env["FG_CHAIN_HUGE_MIN"]) if "FG_CHAIN_HUGE_MIN" in env else (cc.FIN_CAP_M if small_call else 4096)
    out = set()
    if any(n <= fused_max for n in listed):
        out.add("k_chain_small")
    if any(n > fused_max for n in listed):
        out.add("k_group_prep")
    rest = [n for n in passing if n > fused_max]            # what k_chain_small has not finished
    small = [n for n in rest if n <= cc.FIN_CAP_S]
    mid = [n for n in rest if cc.FIN_CAP_S < n <= huge_min]
    huge = [n for n in rest if n > max(huge_min, cc.FIN_CAP_S)]
    if rest:
        out.add("k_chain_dp")
    if small:
        out.add("k_chain_finish<lds256>")
    if mid:
        out.add("k_chain_finish<lds1024>" if small_call and huge_min <= cc.FIN_CAP_M else "k_chain_finish<global>")
    if huge:
        out.add("k_chain_finish<global>")
    return out, sum(n for n in passing if n <= fused_max)


@pytest.mark.parametrize("name", cc.CASE_NAMES)
def test_chain_classes_against_oracle(built, monkeypatch, name):
    from flye_amd import config, gpu
    from oracle import oracle as O
    case = cc.make_case(name)
    rs, ex, q = case.readset(), case.index(), case.query_ids()
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
    seen = set()
    for run in case.runs:
        fl, mo, only_max = run.get("force_local", False), run.get("max_overlaps", 0), run.get("only_max", True)
        listed, passing = case.sizes(fl)
        totals = case.totals(fl)
        for keep in (0, 1):
            ores = o.overlaps(O.detector_params(cfg, min_overlap=cc.MIN_OVERLAP, only_max_ext=only_max,
                                                keep_alignment=bool(keep)), q, max_overlaps=mo, force_local=fl)
            det.p.only_max_ext, det.p.keep_alignment = int(only_max), keep
            for env in SETTINGS:
                for k, v in env.items():
                    monkeypatch.setenv(k, v)
                try:
                    where = (name, run, keep, env)
                    gres = det.getSeqOverlapsBatch(q, forceLocal=fl, maxOverlaps=mo)
                    check_overlaps_equal(gres, ores, keep, counts=not mo)
                    assert (gres.seed_hits, gres.dp_groups, gres.dp_elements) == totals, where
                    kt = ctx.kernel_times()
                    # the two overlaps of the size classes that were possible before they were made disjoint
                    if env.get("FG_FUSED_CAP") == "448" and max(listed) <= 448:
                        assert "k_group_prep" not in kt, where
                    if env.get("FG_CHAIN_HUGE_MIN") == "100" and max(passing) <= cc.FIN_CAP_S:
                        assert "k_chain_finish<global>" not in kt, where
                    ran = {k for k in CHAIN_KERNELS if k in kt}
                    want, small_elems = expected_kernels(listed, passing, env)
                    assert ran == want, where
                    assert gres.dp_elements_small == small_elems, where
                    seen |= ran
                finally:
                    for k in env:
                        monkeypatch.delenv(k)
    assert len(ores.recs) > 0
    if name == "sizes_s":       # <= 256 hits: the fused kernel, or prefilter + DP + the 256-hit LDS finish
        assert seen == {"k_chain_small", "k_group_prep", "k_chain_dp", "k_chain_finish<lds256>"}
    if name == "sizes_l":       # > 448 hits: every path but the 256-hit LDS finish
        assert seen == set(CHAIN_KERNELS) - {"k_chain_finish<lds256>"}


def test_bulk_call_classification(built):
    """A call that lists >= 65536 groups takes the bulk classes (257..4096 hits: DP + finish on global
    scratch, no LDS-1024 class) with no switch set; compared in full against the oracle."""
    from flye_amd import config, gpu, synth
    from oracle import oracle as O
    rs = synth.simulate(seed=808, genome_len=10_000, coverage=160, kind="ont_raw", median_len=2000, min_len=1100,
                        max_len=3500, n_repeat_families=0, n_tandems=0, n_homopolymers=0).filter_min_len(1000)
    cfg = config.preset("raw")
    ctx = gpu.Context(17, 0)
    ctx.set_reads(rs)
    vi = gpu.VertexIndex(ctx, float(int(cfg["assemble_kmer_sample"])))
    vi.build(cfg)
    det = gpu.OverlapDetector.for_assemble(ctx, vi, cfg)
    q = np.arange(0, 2 * rs.n, dtype=np.uint32)
    gres = det.getSeqOverlapsBatch(q)
    kt = ctx.kernel_times()
    o = O.Oracle(17)
    o.set_reads(rs)
    o.build_index(cfg)
    ores = o.overlaps(O.detector_params(cfg), q)
    check_overlaps_equal(gres, ores, False)
    assert gres.dp_groups >= 65536
    assert "k_chain_finish<global>" in kt and "k_chain_finish<lds1024>" not in kt
