"""The lazy primary of the chaining stage (fg_chain.hip lazy_primary; switch FG_CHAIN_LAZY, default on): with
only_max_ext the primary of a group is taken straight from the DP tables when the rule of DESIGN 4.4 applies, and the
full backtracking stage runs from the untouched arrays otherwise.  On the crafted indexes of tests/chain_craft.py and
on cases built here with its helpers, every call is compared record for record (and kmerMatches element by element)
with the oracle, with the switch on and off, in every size class; fg_debug_chain_lazy says which way the groups went.

What element 0 can root: the reference's DP gives an element a back pointer only when its best predecessor scores
MORE than k (overlap.cpp:318-322), and a step from element 0 (score 0) scores at most k.  So no element ever points at
element 0 and the rule's second condition (tests/test_lazy_primary_rule.py shows why the rule needs it on arbitrary
tables) cannot fail on tables this DP made: no input can be crafted for that fallback, and the tests here assert
that its counter stays 0 -- also on ``zero_root``, whose group starts with two hits 5 bases apart on one diagonal,
the closest an input comes to a chain rooted at element 0.
"""
import numpy as np
import pytest

import chain_craft as cc
from helpers import check_overlaps_equal, golden_reads

pytestmark = pytest.mark.gpu

SETTINGS = [
    {},
    {"FG_CHAIN_FUSED": "0"},
    {"FG_CHAIN_NO_SMALL_CALL": "1"},
    {"FG_CHAIN_HUGE_MIN": "100"},
    {"FG_CHAIN_STREAMS": "1"},
    {"FG_FORCE_KEY64": "1"},
]
SWITCHES = sorted({k for s in SETTINGS for k in s} | {"FG_CHAIN_LAZY", "FG_FUSED_CAP", "FG_PACKED_KEYS"})

# every size class and its edges: the fused kernel's register tiers (<= 64, <= 128, <= 256), the LDS prefilter
# (<= 320), the 1024-hit LDS class / the LDS walk of the global-scratch class (<= 1024), beyond, a few thousand
LAZY_SIZES = [10, 63, 64, 65, 128, 129, 256, 257, 320, 321, 1024, 1025, 3000]


def clean_sizes_case():
    """One collinear copy per group, at every size of LAZY_SIZES, ext-sorted (target longer) and not: a single chain
    over all hits whose scores rise strictly along it.  Its tip is the strict maximum, and the candidate of the whole
    chain, which passes overlapTest, is the group's only one: every group must take the fast path."""
    c = cc.Case("lazy_sizes", 83)
    for n in LAZY_SIZES:
        for rel in (1, -1):
            seg = max(1300, n + 60)
            cc.pair(c, seg, cc.spread(n, seg - cc.K - 20), rel=rel)
    return c


# best_fails: what the case adds to the hit lists cc.pair declares, declared up front.  Per group (dense chain's key
# step, hits of the passing chain): 166 + 60 hits (the fused kernel's class) and 666 + 200 (beyond 256 hits)
DENSE_AT, DENSE_LEN = 1600, 2000
BEST_FAILS = [(12, 60), (3, 200)]


def dense_hits(step):
    return [(DENSE_AT + o, DENSE_AT + o) for o in range(0, DENSE_LEN - cc.K, step)]


def best_fails_case():
    """Groups of two chains that cannot be joined (the second lies later on the query and earlier on the target):
    a dense chain over 2000 bases that starts 1600 bases into both reads -- the highest score by far, and a left
    overhang above maxOverhang, so overlapTest rejects it -- and a chain over 1260 bases that reaches both reads'
    ends closely enough.  The lazy path must fall back, and the primary is the lower chain."""
    c = cc.Case("best_fails", 89)
    seg = 1300
    for step, n_pass in BEST_FAILS:
        # query: 200 | S | 100 | dense | 300      target: 1600 | dense | 50 | S | 40 | 160
        qr, tr = cc.pair(c, seg, cc.spread(n_pass, seg - cc.K - 20), left_q=200, right_q=100 + DENSE_LEN + 300,
                         left_t=DENSE_AT + DENSE_LEN + 50, t_len=DENSE_AT + DENSE_LEN + 50 + seg + 200)
        D = c.rand(DENSE_LEN)
        Q, T = c.seqs[qr], c.seqs[tr]
        assert 200 + seg + 100 == DENSE_AT
        Q[DENSE_AT:DENSE_AT + DENSE_LEN] = D
        T[DENSE_AT:DENSE_AT + DENSE_LEN] = D
        hits = dense_hits(step)
        c.add_keys(Q, [h[0] for h in hits])
        c.groups[(2 * qr, 2 * tr)] += hits
    return c


# tied_top: hits of the pattern chain per group (the fused kernel's class, beyond 256 hits) and where the case plants
# the second chain, declared up front
TIED_TOP = [40, 300]
TIED_Q, TIED_T, TIED_LEAD = 200, 1550, 30


def tied_hits(pattern):
    return [(TIED_Q + o, TIED_T + o) for o in [0] + [TIED_LEAD + int(p) for p in pattern]]


def tied_top_case():
    """Groups of two chains that cannot be joined and whose ends share the top score: the same key pattern twice,
    and in front of the chain that holds the group's first hit one hit more -- element 0 has score 0 and roots
    nothing, so that chain effectively starts at its second hit (score k) and repeats the other's scores exactly.
    (The ``tandem`` and ``ties`` cases of chain_craft have tied scores, but none at the top of a group.)  The
    target is shorter than the query, so the DP runs in query order and element 0 is the planted chain's."""
    c = cc.Case("tied_top", 101)
    seg = 1300
    for n in TIED_TOP:
        pattern = cc.spread(n, seg - cc.K - 20)
        # query: 200 | lead + S' | 100 | S | 300      target: 200 | S | 50 | lead + S' | 120
        qr, tr = cc.pair(c, seg, pattern, left_q=TIED_Q + TIED_LEAD + seg + 100, left_t=200,
                         t_len=TIED_T + TIED_LEAD + seg + 120)
        A = c.rand(TIED_LEAD + seg)
        Q, T = c.seqs[qr], c.seqs[tr]
        assert len(Q) > len(T) and 200 + seg + 50 == TIED_T
        Q[TIED_Q:TIED_Q + len(A)] = A
        T[TIED_T:TIED_T + len(A)] = A
        hits = tied_hits(pattern)
        c.add_keys(Q, [h[0] for h in hits])
        c.groups[(2 * qr, 2 * tr)] += hits
    return c


def zero_root_case():
    """Groups whose first two hits are 5 bases apart on one diagonal (see the module's docstring)."""
    c = cc.Case("zero_root", 97)
    for n, rel in ((40, 1), (40, -1), (300, 1)):
        seg = 1300
        offs = np.unique(np.concatenate([[0, 5], 30 + cc.spread(n - 2, seg - cc.K - 60)]))
        assert len(offs) == n
        cc.pair(c, seg, offs, rel=rel)
    return c


EXTRA = {"lazy_sizes": clean_sizes_case, "best_fails": best_fails_case, "tied_top": tied_top_case,
         "zero_root": zero_root_case}
CASES = cc.CASE_NAMES + list(EXTRA)
FALLBACKS = ("tied_top", "root", "overlap_test")


def test_extra_cases_declare_their_groups():
    """The hit lists declared for the cases built here are what the crafted index really yields."""
    for make in EXTRA.values():
        case = make()
        got = cc.enumerate_groups(case)
        assert {g: sorted(h) for g, h in case.groups.items()} == got, case.name


@pytest.mark.parametrize("name", CASES)
def test_lazy_primary_against_oracle(built, monkeypatch, name):
    from flye_amd import config, gpu
    from oracle import oracle as O
    case = EXTRA[name]() if name in EXTRA else cc.make_case(name)
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
    seen = dict.fromkeys(("fast",) + FALLBACKS, 0)
    for run in case.runs:
        fl, mo, only_max = run.get("force_local", False), run.get("max_overlaps", 0), run.get("only_max", True)
        for keep in (0, 1):
            ores = o.overlaps(O.detector_params(cfg, min_overlap=cc.MIN_OVERLAP, only_max_ext=only_max,
                                                keep_alignment=bool(keep)), q, max_overlaps=mo, force_local=fl)
            det.p.only_max_ext, det.p.keep_alignment = int(only_max), keep
            for env in SETTINGS:
                for k, v in env.items():
                    monkeypatch.setenv(k, v)
                try:
                    res = {}
                    for lazy in ("1", "0"):
                        where = (name, run, keep, env, lazy)
                        monkeypatch.setenv("FG_CHAIN_LAZY", lazy)
                        gres = det.getSeqOverlapsBatch(q, forceLocal=fl, maxOverlaps=mo)
                        cnt = ctx.debug_chain_lazy()
                        print(where, cnt)
                        check_overlaps_equal(gres, ores, keep, counts=not mo)
                        assert cnt["entered"] == gres.dp_groups == case.totals(fl)[1], where
                        if lazy == "1" and only_max:
                            assert cnt["fast"] + cnt["no_live"] + sum(cnt[f] for f in FALLBACKS) == cnt["entered"], where
                            assert cnt["root"] == 0, where
                            for f in seen:
                                seen[f] += cnt[f]
                            if name.startswith("sizes_") or name == "lazy_sizes":
                                assert cnt["fast"] > 0, where
                            if name == "lazy_sizes":      # every group of every class
                                assert cnt["fast"] == cnt["entered"] == len(case.groups), where
                            if name == "best_fails":
                                assert cnt["overlap_test"] == len(BEST_FAILS) and cnt["fast"] == 0, where
                            if name == "tied_top":
                                assert cnt["tied_top"] == len(TIED_TOP) and cnt["fast"] == 0, where
                        else:
                            assert cnt["fast"] == cnt["no_live"] == 0 and not any(cnt[f] for f in FALLBACKS), where
                        res[lazy] = gres
                    # on against off
                    assert res["1"].lines() == res["0"].lines()
                    assert np.array_equal(res["1"].recs, res["0"].recs)
                    if keep:
                        assert np.array_equal(res["1"].matches, res["0"].matches)
                        assert np.array_equal(res["1"].match_off, res["0"].match_off)
                finally:
                    monkeypatch.delenv("FG_CHAIN_LAZY", raising=False)
                    for k in env:
                        monkeypatch.delenv(k)
    assert len(ores.recs) > 0
    assert seen["fast"] > 0 or name in ("best_fails", "tied_top")
    assert seen["root"] == 0


def test_lazy_primary_whole_path(built, golden_cases, monkeypatch):
    """A raw-read golden input through the whole path, both strands of every read as queries: the same records as
    the oracle with the switch on and off; the fast path and both fallbacks that real tables can reach all occur."""
    from flye_amd import config, gpu
    from oracle import oracle as O
    case = golden_cases["raw_pb"]
    rs = golden_reads(case)
    cfg = config.preset(case["preset"])
    ctx = gpu.Context(int(cfg["kmer_size"]), 0)
    ctx.set_reads(rs)
    vi = gpu.VertexIndex(ctx, float(int(cfg["assemble_kmer_sample"])))
    vi.build(cfg)
    det = gpu.OverlapDetector.for_assemble(ctx, vi, cfg)
    o = O.Oracle(int(cfg["kmer_size"]))
    o.set_reads(rs)
    o.build_index(cfg)
    q = np.arange(0, 2 * rs.n, dtype=np.uint32)
    for keep in (0, 1):
        det.p.keep_alignment = keep
        ores = o.overlaps(O.detector_params(cfg, keep_alignment=bool(keep)), q)
        for lazy in ("1", "0"):
            monkeypatch.setenv("FG_CHAIN_LAZY", lazy)
            gres = det.getSeqOverlapsBatch(q)
            cnt = ctx.debug_chain_lazy()
            print(keep, lazy, cnt)
            check_overlaps_equal(gres, ores, keep)
            assert cnt["entered"] == gres.dp_groups
            if lazy == "1":
                assert cnt["fast"] + cnt["no_live"] + sum(cnt[f] for f in FALLBACKS) == cnt["entered"]
                assert cnt["root"] == 0
                assert cnt["fast"] > 0 and cnt["overlap_test"] > 0 and cnt["tied_top"] > 0
            else:
                assert cnt["fast"] == cnt["no_live"] == 0 and not any(cnt[f] for f in FALLBACKS)
