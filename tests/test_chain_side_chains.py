"""The side chains of the chaining stage (fg_chain.hip fgChainStage, fused configuration): k_group_list fixes the
size classes by the groups' raw sizes, the mid and the huge class each run prefilter -> DP -> backtracking on a side
stream of their own, and a listed group that the prefilter drops (dpSize stays 0) returns at once in k_chain_dp and
k_chain_finish.  On one crafted index (tests/chain_craft.py) with groups at every class boundary of both call forms
(hugeMin = 1024 with k_chain_finish<lds1024>, and 4096 under FG_CHAIN_NO_SMALL_CALL=1), each with the target longer
and shorter than the query, and with dropped groups between surviving neighbours.  Calls over subsets of the queries
leave classes empty.  Every switch setting runs in a child process of its own; its records are compared with the
oracle's field by field, and with the default's byte by byte."""
import os
import pickle
import subprocess
import sys
import types

import numpy as np
import pytest

import chain_craft as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HUGE_MIN_SMALL, HUGE_MIN_BULK = cc.FIN_CAP_M, 4096

SETTINGS = {
    "default": {},
    "no_small_call": {"FG_CHAIN_NO_SMALL_CALL": "1"},          # bulk form: the mid class in two parts, one per side stream
    "no_small_call_split0": {"FG_CHAIN_NO_SMALL_CALL": "1", "FG_CHAIN_SPLIT": "0"},
    "streams1": {"FG_CHAIN_STREAMS": "1"},
    "streams1_no_small_call": {"FG_CHAIN_STREAMS": "1", "FG_CHAIN_NO_SMALL_CALL": "1"},
    "fused0": {"FG_CHAIN_FUSED": "0"},
}
SWITCHES = sorted({k for s in SETTINGS.values() for k in s} |
                  {"FG_FUSED_CAP", "FG_CHAIN_HUGE_MIN", "FG_CHAIN_LAZY", "FG_FORCE_KEY64", "FG_PACKED_KEYS", "FG_LANES"})

# fusedMax, fusedMax + 1, PREP_CAP, PREP_CAP + 1, hugeMin2, hugeMin2 + 1 of both call forms
EDGE_SIZES = [cc.FIN_CAP_S, cc.FIN_CAP_S + 1, cc.PREP_CAP, cc.PREP_CAP + 1, HUGE_MIN_SMALL, HUGE_MIN_SMALL + 1,
              HUGE_MIN_BULK, HUGE_MIN_BULK + 1]
VARIANTS = [(1, 0), (0, 1)]         # (only_max_ext, keep_alignment)


def _overhang_pair(c, n):
    """n collinear hits whose left overhang is maxOverhang + 1 on the query (more on the target): listed, dropped."""
    seg = max(1300, n + 60)
    return cc.pair(c, seg, cc.spread(n, seg - cc.K - 20), left_q=cc.MAX_OVERHANG + 1, left_t=cc.MAX_OVERHANG + 100)


def make_case():
    """(case, {tag: [query read, ...]}): the tags name the query subsets of the calls."""
    c = cc.Case("side_chains", 132)
    tags = {}

    def add(tag, qr):
        tags.setdefault(tag, []).append(qr)
        return qr

    # the boundaries, ext-sorted (target one base longer) and not (one shorter), collinear and with a stray hit
    for n in EDGE_SIZES:
        for rel in (1, -1):
            for asc in (True, False):
                seg = max(1300, n + 60)
                offs = cc.spread(n if asc else n - 1, seg - cc.K - 20)
                add("edges", cc.pair(c, seg, offs, rel=rel, strays=0 if asc else 1)[0])
    # a mid group whose target span is minOverlap - 1 (query span minOverlap, one deleted base), between survivors
    add("mid_ok", cc.pair(c, 1300, cc.spread(400, 1250))[0])
    offs = np.concatenate([np.arange(0, 200), np.arange(501, 700), [cc.MIN_OVERLAP]])
    add("mid_dropped", cc.pair(c, 1100, offs, edits=[(500, -1)])[0])
    add("mid_ok", cc.pair(c, 1300, cc.spread(600, 1250), rel=-1)[0])
    # ... and one dropped for its overhang
    add("mid_dropped", _overhang_pair(c, 700)[0])
    add("mid_ok", cc.pair(c, 1300, cc.spread(300, 1250))[0])
    # huge groups of either call form dropped for their overhang, between survivors
    add("huge_ok", cc.pair(c, 4700, cc.spread(4600, 4650))[0])
    add("huge_dropped", _overhang_pair(c, 1500)[0])
    add("huge_ok", cc.pair(c, 1600, cc.spread(1500, 1550), rel=-1)[0])
    add("huge_dropped", _overhang_pair(c, 4500)[0])
    add("huge_ok", cc.pair(c, 4400, cc.spread(4300, 4350))[0])
    # small groups; one that k_group_list does not list at all (query span minOverlap - 1)
    for n in (12, 100, 200):
        add("fused", cc.pair(c, 1300, cc.spread(n, 1250))[0])
    add("unlisted", cc.pair(c, 1100, cc.spread(12, cc.MIN_OVERLAP - 1))[0])
    return c, tags


def group_size(case, qr):
    (n, listed, passes), = [v for g, v in case.verdicts().items() if g[0] == 2 * qr]
    return n, listed, passes


def make_calls(case, tags):
    """{call name: query reads}: everything, and subsets that leave size classes of either call form empty."""
    edges = {qr: group_size(case, qr)[0] for qr in tags["edges"]}
    every = [q >> 1 for q in case.queries]
    return {
        "all": every,
        "only_fused": tags["fused"] + [q for q, n in edges.items() if n <= cc.FIN_CAP_S],
        "only_257_1024": [q for q, n in edges.items() if cc.FIN_CAP_S < n <= HUGE_MIN_SMALL] + tags["mid_ok"],
        "only_1025_4096": [q for q, n in edges.items() if HUGE_MIN_SMALL < n <= HUGE_MIN_BULK],
        "only_above_4096": [q for q, n in edges.items() if n > HUGE_MIN_BULK],
        "only_dropped_mid": tags["mid_dropped"],
        "only_dropped_huge": tags["huge_dropped"],
        "only_dropped": tags["mid_dropped"] + tags["huge_dropped"] + tags["unlisted"],
        "none_listed": tags["unlisted"],
    }


def query_ids(case, reads):
    return (2 * np.asarray(sorted(reads), np.int64) + case.first_id).astype(np.uint32)


def expected_kernels(sizes, env):
    """The chaining kernels of the fused configuration for LISTED groups of these sizes: the classes are fixed before
    the prefilter, so a class whose groups are all dropped still launches (and every wave returns at once)."""
    small_call = len(sizes) < 65536 and "FG_CHAIN_NO_SMALL_CALL" not in env
    huge_min = HUGE_MIN_SMALL if small_call else HUGE_MIN_BULK
    big = [n for n in sizes if n > cc.FIN_CAP_S]
    out = set()
    if any(n <= cc.FIN_CAP_S for n in sizes):
        out.add("k_chain_small")
    if big:
        out |= {"k_group_prep", "k_chain_dp"}
    if any(n <= huge_min for n in big):
        out.add("k_chain_finish<lds1024>" if small_call else "k_chain_finish<global>")
    if any(n > huge_min for n in big):
        out.add("k_chain_finish<global>")
    return out


CHAIN_KERNELS = ("k_chain_small", "k_group_prep", "k_dp_list", "k_chain_dp", "k_chain_finish<lds256>",
                 "k_chain_finish<lds1024>", "k_chain_finish<global>")


# ---- what the case declares (no device) ------------------------------------------------------------------------------
def test_case_declares_its_groups():
    case, tags = make_case()
    assert {g: sorted(h) for g, h in case.groups.items()} == cc.enumerate_groups(case)
    assert sorted(group_size(case, q)[0] for q in tags["edges"]) == sorted(4 * EDGE_SIZES)
    assert all(group_size(case, q)[1:] == (True, True) for q in tags["edges"] + tags["mid_ok"] + tags["huge_ok"] + tags["fused"])
    for q in tags["mid_dropped"]:
        n, listed, passes = group_size(case, q)
        assert cc.FIN_CAP_S < n <= HUGE_MIN_SMALL and listed and not passes
    assert sorted(group_size(case, q)[0] for q in tags["huge_dropped"]) == [1500, 4500]     # huge in either call form
    assert all(group_size(case, q)[1:] == (True, False) for q in tags["huge_dropped"])
    assert [group_size(case, q)[1:] for q in tags["unlisted"]] == [(False, False)]
    # each dropped group lies between surviving neighbours of its class (group ids follow the query ids)
    order = [q >> 1 for q in case.queries]
    for q in tags["mid_dropped"] + tags["huge_dropped"]:
        i = order.index(q)
        assert group_size(case, order[i - 1])[2] and group_size(case, order[i + 1])[2]
    calls = make_calls(case, tags)
    assert all(len(v) > 0 for v in calls.values())


# ---- child process: one switch setting, every call -------------------------------------------------------------------
def _child_main(out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from flye_amd import config, gpu
    case, tags = make_case()
    rs, ex = case.readset(), case.index()
    cfg = config.preset("raw")
    ctx = gpu.Context(cc.K, 0)
    ctx.set_reads(rs, case.first_id)
    vi = gpu.VertexIndex(ctx, 1.0)
    vi.import_index(gpu.IndexExport(ex.keys, ex.key_off, ex.entries, ex.repetitive), 1.0)
    det = gpu.OverlapDetector.for_assemble(ctx, vi, cfg, min_overlap=cc.MIN_OVERLAP)
    out = {}
    for name, reads in make_calls(case, tags).items():
        for only_max, keep in VARIANTS:
            det.p.only_max_ext, det.p.keep_alignment = only_max, keep
            g = det.getSeqOverlapsBatch(query_ids(case, reads))
            kt = ctx.kernel_times()
            out[(name, only_max, keep)] = dict(
                lines=g.lines(), recs=np.array(g.recs), query_off=np.array(g.query_off), stats=np.array(g.stats),
                match_off=None if g.match_off is None else np.array(g.match_off),
                matches=None if g.match_off is None else np.array(g.matches),
                counters=(g.query_kmers, g.seed_hits, g.dp_groups, g.dp_elements, g.dp_elements_small),
                kernels=sorted(k for k in CHAIN_KERNELS if k in kt))
            del g
    with open(out_path, "wb") as f:
        pickle.dump(out, f)
    ctx.close()


if __name__ == "__main__":
    _child_main(sys.argv[1])
    sys.exit(0)


@pytest.fixture(scope="module")
def crafted(built):
    """The case, its calls and the oracle's result of every call, computed once."""
    from flye_amd import config
    from oracle import oracle as O
    case, tags = make_case()
    calls = make_calls(case, tags)
    cfg = config.preset("raw")
    o = O.Oracle(cc.K)
    o.set_reads(case.readset(), case.first_id)
    o.import_index(case.index(), 1.0)
    want = {}
    for name, reads in calls.items():
        for only_max, keep in VARIANTS:
            want[(name, only_max, keep)] = o.overlaps(
                O.detector_params(cfg, min_overlap=cc.MIN_OVERLAP, only_max_ext=bool(only_max), keep_alignment=bool(keep)),
                query_ids(case, reads))
    return types.SimpleNamespace(case=case, tags=tags, calls=calls, want=want, runs={})


def _run_setting(crafted, tmp_path_factory, setting):
    if setting not in crafted.runs:
        out = str(tmp_path_factory.mktemp("side_chains") / (setting + ".pkl"))
        env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
        env.update(SETTINGS[setting])
        r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        with open(out, "rb") as f:
            crafted.runs[setting] = pickle.load(f)
    return crafted.runs[setting]


def _as_result(d):
    r = types.SimpleNamespace(**{k: v for k, v in d.items() if k not in ("lines", "counters", "kernels")})
    r.lines = lambda: d["lines"]
    r.query_kmers, r.seed_hits, r.dp_groups, r.dp_elements, r.dp_elements_small = d["counters"]
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_side_chains_against_oracle(crafted, tmp_path_factory, setting):
    """Every call of the case under one switch setting: the oracle's records, no record of a dropped group, the
    kernels the listed sizes select (no k_dp_list in the fused configuration), and the default's bytes."""
    from helpers import check_overlaps_equal
    got = _run_setting(crafted, tmp_path_factory, setting)
    base = _run_setting(crafted, tmp_path_factory, "default")
    case, tags, env = crafted.case, crafted.tags, SETTINGS[setting]
    dropped = {int(2 * q + case.first_id) for q in tags["mid_dropped"] + tags["huge_dropped"] + tags["unlisted"]}
    for key, d in got.items():
        name, only_max, keep = key
        ores = crafted.want[key]
        check_overlaps_equal(_as_result(d), ores, keep)
        assert not dropped & set(d["recs"]["cur_id"].tolist()), key
        if name in ("only_dropped_mid", "only_dropped_huge", "only_dropped", "none_listed"):
            assert len(d["recs"]) == 0, key
        else:
            assert len(d["recs"]) > 0, key
        sizes = [n for n, listed, _ in (group_size(case, q) for q in crafted.calls[name]) if listed]
        if "FG_CHAIN_FUSED" in env:
            assert ("k_dp_list" in d["kernels"]) == any(n > 0 for n in sizes), key
        else:
            assert set(d["kernels"]) == expected_kernels(sizes, env), key
        b = base[key]
        assert d["lines"] == b["lines"] and d["recs"].tobytes() == b["recs"].tobytes(), key
        assert d["counters"][:4] == b["counters"][:4], key         # (the fifth is the fused kernel's share)
        assert d["counters"][4] == (0 if "FG_CHAIN_FUSED" in env else b["counters"][4]), key
        if keep:
            assert d["matches"].tobytes() == b["matches"].tobytes(), key
            assert d["match_off"].tobytes() == b["match_off"].tobytes(), key
    # every boundary group and every survivor beside a dropped group gave a record in the full call
    every = got[("all", 1, 0)]
    have = set(every["recs"]["cur_id"].tolist())
    for q in tags["edges"] + tags["mid_ok"] + tags["huge_ok"]:
        assert int(2 * q + case.first_id) in have, q
