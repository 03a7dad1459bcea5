"""fg_read_coverage / fg_edge_coverage: the window coverage of ChimeraDetector (reference src/assemble/chimera.cpp:
31-343) and of MultiplicityInferer::estimateCoverage (src/repeat_graph/multiplicity_inferer.cpp:14-90) on the device, the
two host-only float steps (fg_coverage_windows / fg_coverage_verdict) and the ChimeraDetector mirror on top of them.

No program of the reference that is built here prints coverage vectors, so the yardstick is a restatement pinned in two
independent forms (tests/coverage_restate.py: numpy difference arrays with np.float32, and tests/native/
coverage_driver.cpp: the reference's loops on std::vector::at with std::sort, std::ceil and std::lround).  The first
test pins that they agree on every case the device tests use; it needs no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import coverage_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ_SEEDS = list(range(8))
EDGE_FUZZ_SEEDS = list(range(4))
EDGE_COUNTS = [1, 255, 256, 257]
THR_NAMES = ["thr_%d_%d_%d" % (r, c, u) for r, c in ((2, 1), (2, 3), (2, 5), (5, 12), (5, 13), (4, 6), (4, 10)) for u in (0, 1)]
CRAFTED_NAMES = ["window_counts", "overhang", "skips", "intervals", "pileup", "median", "flank0", "flank5", "flank15", "tiles"] + THR_NAMES
NEW_SYMBOLS = ("fg_read_coverage", "fg_release_coverage", "fg_coverage_windows", "fg_coverage_verdict", "fg_edge_coverage",
               "fg_release_edge_coverage")

_CACHE = {}


def crafted():
    if "crafted" not in _CACHE:
        _CACHE["crafted"] = R.crafted_reads()
        assert sorted(_CACHE["crafted"]) == sorted(CRAFTED_NAMES)
    return _CACHE["crafted"]


def expected(name):
    """The restatement's result for a crafted batch (computed once, never changed)"""
    key = ("want", name)
    if key not in _CACHE:
        _CACHE[key] = R.restate_reads(crafted()[name])
    return _CACHE[key]


def fuzz(seed):
    """(batch, the native form's result) of a fuzz seed, computed once"""
    key = ("fuzz", seed)
    if key not in _CACHE:
        b = R.fuzz_reads(seed)
        _CACHE[key] = (b, R.native_reads(b))
    return _CACHE[key]


def edge_cases():
    """name -> (batch, the numpy form's result)"""
    if "edges" not in _CACHE:
        cases = dict(R.crafted_edges())
        for seed in EDGE_FUZZ_SEEDS:
            cases["fuzz%d" % seed] = R.fuzz_edges(seed)
        for n in EDGE_COUNTS:
            cases["edges%d" % n] = R.fuzz_edges(50 + n, n)
        _CACHE["edges"] = {k: (b, R.restate_edges(b)) for k, b in cases.items()}
    return _CACHE["edges"]


EDGE_NAMES = ["rules", "no_paths", "window7"] + ["fuzz%d" % s for s in EDGE_FUZZ_SEEDS] + ["edges%d" % n for n in EDGE_COUNTS]


def check_crafted_expectations(name, want):
    """What each crafted group is there to show, read off the restatement's result"""
    nw = np.diff(want["win_off"].astype(np.int64)).tolist()
    total, chim = want["sum"].tolist(), want["chimeric"].tolist()
    if name == "window_counts":
        assert nw == [1, 1, 1, 1, 1, 63, 63, 64, 64, 65, 65, 255, 255, 256, 256, 257, 257]
        assert want["degenerate"].tolist() == [True, True, True] + [False] * 14
        assert total[3] == 0 and total[4] == 0 and chim[:5]   # one real window: no record of the read reaches it
        assert chim[:5] == [True] * 5 and all(t == 0 for t in total[6::2])
        assert want["max"].tolist()[5::2] == [3] * 6
    elif name == "overhang":            # 50 = max_overhang counts as full, 51 as a junction, through each term
        junction = [int(want["junction"][want["win_off"][q]:want["win_off"][q + 1]].sum()) for q in range(8)]
        assert all(t > 0 for t in total[:4]) and junction[:4] == [0] * 4
        assert total[4:] == [0] * 4 and junction[4:] == total[:4]
    elif name == "skips":
        assert total == [0, 0, 58, 0, 0, 58] and want["max"].tolist() == [0, 0, 2, 0, 0, 2]
    elif name == "intervals":
        assert total == [0, 1, 9, 0, 0, 1, 1, 2] and want["max"].tolist()[2] == 1
    elif name == "pileup":
        full = want["full"][:19].tolist()
        assert full == [0] * 5 + [5000, 5000] + [0] * 12 and want["max"][0] == 5000 and total[0] == 10000
    elif name == "median":              # [1, 1, 2, 2] -> the upper one; five values; ties below the middle; n = 1; n = 2
        assert nw == [4, 5, 4, 1, 2] and want["median"].tolist() == [2, 2, 1, 7, 2]
    elif name.startswith("flank"):
        flank = int(name[5:])
        assert R.max_flank(crafted()[name].params["max_overhang"], 100) == flank
        dips = sorted({max(flank - 1, 0), flank, 40 - flank - 1, min(40 - flank, 39), 20})
        inside = [flank <= d <= 40 - flank - 1 for d in dips]
        assert chim[:len(dips)] == inside and True in inside and (flank == 0 or False in inside)
        assert want["min_good"].tolist()[:len(dips)] == [2 if i else 3 for i in inside]
        assert chim[len(dips):] == ([True, False] if flank == 0 else [True, True, False])       # good_end <, ==, > good_start
    elif name == "tiles":
        full = want["full"][:257]
        assert full[59:72].tolist() == [2] + [4] * 11 + [3] and full[201] == 1 and full[256] == 1
        assert want["junction"][60:67].tolist() == [0, 0, 0, 1, 1, 0, 0]
    else:                               # thresholds at and around the lround ties
        rate, cov, uneven = (int(x) for x in name.split("_")[1:])
        thr = {(2, 1): 1, (2, 3): 2, (2, 5): 3, (5, 12): 2, (5, 13): 3, (4, 6): 2, (4, 10): 3}[(rate, cov)]
        if not uneven:
            assert want["threshold"].tolist() == [thr] * 4 and chim == [False, thr > 1, False, False]
        else:
            assert want["threshold"][0] == thr and chim == [False] * 4


# ---- 1. the two forms of the yardstick agree (no GPU) ---------------------------------------------------------------
def test_restatements_agree_on_every_case(built):
    for name in CRAFTED_NAMES:
        want = expected(name)
        assert R.same(want, R.native_reads(crafted()[name]), R.READ_FIELDS), name
        check_crafted_expectations(name, want)
    for seed in FUZZ_SEEDS:
        b, native = fuzz(seed)
        py = R.restate_reads(b)
        assert R.same(py, native, R.READ_FIELDS), seed
        sizes = np.diff(b.query_off.astype(np.int64))
        assert sizes.min() == 0 and sizes.max() > 250 and py["chimeric"].any() and not py["chimeric"].all() and py["degenerate"].any()
        assert py["junction"].any() and py["full"].any()
        if b.params["window"] == 100:
            assert int(py["win_off"][-1] - py["win_off"][-2]) == 167772        # (float)16777301 rounds down: not 167773
    assert {fuzz(s)[0].params["window"] for s in FUZZ_SEEDS} == {100, 7, 1}
    assert {fuzz(s)[0].params["uneven_coverage"] for s in FUZZ_SEEDS} == {0, 1}
    # threads change nothing in the native form (tools/coverage_bench.py times it on 1 and on 16)
    b, native = fuzz(FUZZ_SEEDS[0])
    assert R.same(R.native_reads(b, threads=5), native, R.READ_FIELDS)
    for name in EDGE_NAMES:
        b, want = edge_cases()[name]
        assert R.same(want, R.native_edges(b), R.EDGE_FIELDS), name
    check_edge_expectations()


def check_edge_expectations():
    b, want = edge_cases()["rules"]
    nw = np.diff(want["win_off"].astype(np.int64)).tolist()
    assert nw == [10, 25, 0, 0, 7, 10, 1]
    assert want["median"].tolist()[2:4] == [0, 0] and want["sum"].tolist()[2:4] == [0, 0]         # edges without windows
    assert want["sum"][5] == 0 and want["max"][5] == 0                                            # the edge no path touches
    assert np.array_equal(edge_cases()["no_paths"][1]["cov"], np.zeros(53, np.int32))
    for n in EDGE_COUNTS:
        assert len(edge_cases()["edges%d" % n][0].edge_len) == n


# ---- 2. exported and declared (no GPU; fails without the feature) ---------------------------------------------------
def _header_fields(text, name):
    body = re.search(r"struct " + name + r"\s*\{(.*?)\};", text, re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"[*\s]|\[\d+\]", "", n) for n in decl.split(None, 1)[1].split(",")]
    return names


def test_symbols_and_struct_layouts(built):
    from flye_amd import gpu
    lib = gpu.load_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flye_gpu.h")).read(), flags=re.S)
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b" + sym + r"\s*\(", header), sym + " is not declared in include/flye_gpu.h"
        assert hasattr(lib, sym) and sym in gpu.ABI_SYMBOLS
    assert lib.fg_abi_version() == 4 and "#define FG_ABI_VERSION 4" in header
    for cname, cls, size in (("fg_coverage_params", gpu.CoverageParams, 20), ("fg_coverage_batch", gpu.CoverageBatch, 96),
                             ("fg_edge_coverage_batch", gpu.EdgeCoverageBatch, 56)):
        assert _header_fields(header, cname) == [n for n, _ in cls._fields_], cname
        assert C.sizeof(cls) == size, cname
    # no context, no call; releasing nothing is harmless
    assert lib.fg_read_coverage(None, None, None, None, 0, None, None) == -3
    assert lib.fg_edge_coverage(None, 100, None, 0, None, None, 0, 0, 0, None, 0, None, 1, None) == -3
    lib.fg_release_coverage(None)
    lib.fg_release_edge_coverage(None)
    empty = gpu.CoverageBatch()
    lib.fg_release_coverage(C.byref(empty))
    from flye_amd import config
    p = gpu.CoverageParams.from_config(config.preset("raw"), 24, True)
    assert (p.window, p.max_overhang, p.max_drop_rate, p.overlap_coverage, p.uneven_coverage, p.want_vectors) == (100, 1500, 5.0, 24, 1, 1)


# ---- 3. the two host-only calls (no GPU) ----------------------------------------------------------------------------
def test_windows_and_verdict_on_the_host(built):
    from flye_amd import gpu
    L = gpu.load_library()
    lengths = [0, 1, 99, 100, 101, 199, 200, 201, 1000, 1001, 16777301]
    for window in (100, 1, 7):
        for overhang in (0, 99, 100, 500, 1500):
            got = [gpu.coverage_windows(n, window, overhang) for n in lengths]
            want = [R.windows(n, window) + (R.max_flank(overhang, window),) for n in lengths]
            assert [(g[0], g[2], g[1]) for g in got] == want, (window, overhang)
        # the literal form pins the counts: queries without records
        native = R.native_reads(R.ReadBatch([(n, []) for n in lengths], dict(window=window)))
        assert np.diff(native["win_off"].astype(np.int64)).tolist() == [gpu.coverage_windows(n, window, 0)[0] for n in lengths]
        assert native["degenerate"].tolist() == [int(gpu.coverage_windows(n, window, 0)[2]) for n in lengths]
    assert gpu.coverage_windows(16777301, 100, 0)[0] == 167772 and gpu.coverage_windows(16777300, 100, 0)[0] == 167772
    assert [gpu.coverage_windows(n, 100, 0)[:1] + gpu.coverage_windows(n, 100, 0)[2:] for n in (100, 101)] == [(1, True), (1, False)]
    n, f, d = C.c_int32(), C.c_int32(), C.c_uint8()
    assert L.fg_coverage_windows(-1, 100, 0, C.byref(n), C.byref(f), C.byref(d)) == -3
    assert L.fg_coverage_windows(5, 0, 0, C.byref(n), C.byref(f), C.byref(d)) == -3
    assert L.fg_coverage_windows(5, 100, -1, C.byref(n), C.byref(f), C.byref(d)) == -3
    assert L.fg_coverage_windows(5, 100, 0, None, None, None) == 0

    # thresholds at lround ties and around them, both modes; good_end below, equal to and one above good_start; sum == 0
    cases = []
    for rate, covs in ((2.0, (1, 3, 5)), (5.0, (12, 13)), (4.0, (6, 10)), (2.5, (0, 1, 2, 3, 4, 5, 100))):
        for cov in covs:
            for uneven in (0, 1):
                for overhang in (0, 500, 1500):
                    P = dict(window=100, max_overhang=overhang, max_drop_rate=rate, overlap_coverage=cov, uneven_coverage=uneven)
                    flank = R.max_flank(overhang, 100)
                    rows = [(nw, total, cov, mg) for nw in (max(2 * flank, 1), 2 * flank + 1, 2 * flank + 2, 2 * flank + 30)
                            for total in (0, 7) for mg in (0, 1, 2, 3, 4, R.INT32_MAX)]
                    want = [R.verdict(P, *row) for row in rows]
                    thr, chim = gpu.coverage_verdict(gpu.CoverageParams(want_vectors=0, **P), *zip(*rows))
                    assert thr.tolist() == [w[0] for w in want] and chim.tolist() == [w[1] for w in want], P
                    cases.append((P, want))
    thresholds = {(P["max_drop_rate"], P["overlap_coverage"]): w[-1][0] for P, w in cases}
    assert [thresholds[k] for k in ((2.0, 1), (2.0, 3), (2.0, 5), (5.0, 12), (5.0, 13), (4.0, 6), (4.0, 10))] == [1, 2, 3, 2, 3, 2, 3]
    # the literal form pins the same thresholds (crafted batches whose reads have exactly these coverages)
    for name in THR_NAMES:
        b, want = crafted()[name], expected(name)
        nw = np.diff(want["win_off"].astype(np.int64))
        thr, chim = gpu.coverage_verdict(b.coverage_params(), nw, want["sum"], want["median"], want["min_good"])
        native = R.native_reads(b)
        assert thr.tolist() == native["threshold"].tolist() and chim.tolist() == native["chimeric"].astype(bool).tolist(), name
    ok = gpu.CoverageParams(window=100, max_overhang=0, max_drop_rate=5.0, overlap_coverage=3, uneven_coverage=0, want_vectors=0)
    one = [np.array([5], np.int32), np.array([9], np.int64), np.array([2], np.int32), np.array([1], np.int32)]
    out = [np.zeros(1, np.int32), np.zeros(1, np.uint8)]

    def call(p=ok, n=1, arrays=one, outs=out):
        return L.fg_coverage_verdict(C.byref(p) if p is not None else None, n, *(a.ctypes.data if a is not None else None
                                                                                   for a in list(arrays) + list(outs)))

    assert call() == 0 and out[0][0] == 1 and out[1][0] == 0
    assert call(p=None) == -3
    for field, bad in (("window", 0), ("max_overhang", -1), ("max_drop_rate", 0.0), ("max_drop_rate", float("nan"))):
        p = gpu.CoverageParams(window=100, max_overhang=0, max_drop_rate=5.0)
        setattr(p, field, bad)
        assert call(p=p) == -3, field
    for k in range(4):
        assert call(arrays=[None if i == k else a for i, a in enumerate(one)]) == -3
    assert call(outs=[out[0], None]) == -3 and call(outs=[None, out[1]]) == 0
    assert call(n=0, arrays=[None] * 4, outs=[None, None]) == 0


# ---- the device -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(built):
    from flye_amd import gpu
    c = gpu.Context(17, 0)          # no reads, no index: the step needs a device and a stream
    yield c
    c.close()


def device_reads(ctx, b, want_vectors=True):
    res = ctx.read_coverage(b.recs(), b.query_off, b.query_len, b.coverage_params(want_vectors))
    return {k: getattr(res, k) for k in R.READ_FIELDS}


def device_edges(ctx, b, want_vectors=True):
    got = ctx.edge_coverage(b.window, b.recs(), b.aln, b.aln_off, b.first_ext_id, b.edge_of, b.edge_len, want_vectors)
    return dict(zip(R.EDGE_FIELDS, got))


def assert_same(got, want, fields, what):
    for k in fields:
        g, w = np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert not len(bad), (what, k, bad[:5].tolist(), g[bad[:5]].tolist(), w[bad[:5]].tolist())


SCALARS = tuple(k for k in R.READ_FIELDS if k not in ("full", "junction"))


def check_reads(ctx, b, want, what):
    assert_same(device_reads(ctx, b), want, R.READ_FIELDS, what)
    bare = device_reads(ctx, b, want_vectors=False)
    assert bare["full"] is None and bare["junction"] is None
    assert_same(bare, want, SCALARS, what + ", no vectors")


# ---- 4. crafted read batches ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", CRAFTED_NAMES)
def test_crafted_reads(ctx, name):
    want = expected(name)
    check_crafted_expectations(name, want)
    check_reads(ctx, crafted()[name], want, name)
    kt = ctx.kernel_times()
    assert "k_cov_intervals" in kt and "k_cov_target_wave" in kt, sorted(kt)
    if name == "window_counts":
        # the records' position in the caller's array does not matter: the same queries behind a prefix of records
        b = crafted()[name]
        recs = b.recs()
        res = ctx.read_coverage(np.concatenate([recs[:4], recs]), b.query_off + np.uint64(4), b.query_len, b.coverage_params())
        assert_same({k: getattr(res, k) for k in R.READ_FIELDS}, want, R.READ_FIELDS, "shifted")


@pytest.mark.gpu
def test_empty_read_batches(ctx):
    from flye_amd import gpu
    p = gpu.CoverageParams(window=100, max_overhang=0, max_drop_rate=5.0, want_vectors=1)
    res = ctx.read_coverage(np.zeros(0, gpu.REC_DTYPE), [0], [], p)
    assert res.win_off.tolist() == [0] and len(res.full) == 0 and len(res.chimeric) == 0
    res = ctx.read_coverage(np.zeros(0, gpu.REC_DTYPE), [0, 0, 0], [250, 50], p)
    assert res.win_off.tolist() == [0, 2, 3] and res.full.tolist() == [0, 0, 0] and res.chimeric.tolist() == [True, True]
    assert res.degenerate.tolist() == [False, True] and res.min_good.tolist() == [0, 0] and res.median.tolist() == [0, 0]


# ---- 5. forced classes ----------------------------------------------------------------------------------------------
SETTINGS = [dict(FG_COVERAGE_TILE="64"), dict(FG_COVERAGE_WAVE_MAX="0"), dict(FG_COVERAGE_TILE="64", FG_COVERAGE_WAVE_MAX="0"),
            dict(FG_COVERAGE_BATCH_RECS="1"), dict(FG_COVERAGE_BATCH_RECS="5000")]


@pytest.mark.gpu
@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: ",".join("%s=%s" % kv for kv in s.items()))
def test_forced_classes(ctx, monkeypatch, setting):
    """Tiles of 64 windows (intervals across tile edges, the carry), every target on a workgroup, one query per
    sub-batch and sub-batches of 5000 records: the same results"""
    for k, v in setting.items():
        monkeypatch.setenv(k, v)
    for name in CRAFTED_NAMES:
        check_reads(ctx, crafted()[name], expected(name), name)
        kt = ctx.kernel_times()
        if setting.get("FG_COVERAGE_WAVE_MAX") == "0":
            assert "k_cov_target_wave" not in kt and "k_cov_target_wg" in kt, sorted(kt)
        if setting.get("FG_COVERAGE_BATCH_RECS") == "1":
            assert kt["k_cov_intervals"][1] == int((np.diff(crafted()[name].query_off.astype(np.int64)) > 0).sum())
    for seed in FUZZ_SEEDS[:2]:
        b, native = fuzz(seed)
        check_reads(ctx, b, native, "seed %d" % seed)
        if setting.get("FG_COVERAGE_BATCH_RECS") == "5000":
            assert ctx.kernel_times()["k_cov_intervals"][1] >= 4         # it did run in several sub-batches


# ---- 6. fuzz --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_reads(ctx, seed):
    b, native = fuzz(seed)
    check_reads(ctx, b, native, "seed %d" % seed)
    kt = ctx.kernel_times()
    print("seed", seed, b.params, len(b.table), "records,", int(native["win_off"][-1]), "windows, device call %.4f s" %
          ctx.last_coverage_seconds, {k: "%.1f us" % (v[0] * 1e6) for k, v in kt.items()})
    assert "k_cov_target_wg" in kt and "k_cov_target_wave" in kt


# ---- 7. edge coverage -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE_NAMES)
def test_edge_coverage(ctx, monkeypatch, name):
    b, want = edge_cases()[name]
    if name == "rules":
        check_edge_expectations()
    assert_same(device_edges(ctx, b), want, R.EDGE_FIELDS, name)
    kt = ctx.kernel_times()
    assert "k_cov_bounds" in kt and ("k_cov_intervals" in kt) == (len(b.aln) > 0)
    bare = device_edges(ctx, b, want_vectors=False)
    assert bare["cov"] is None
    assert_same(bare, want, ("win_off", "sum", "max", "median"), name + ", no vectors")
    monkeypatch.setenv("FG_COVERAGE_TILE", "64")
    monkeypatch.setenv("FG_COVERAGE_WAVE_MAX", "3")
    assert_same(device_edges(ctx, b), want, R.EDGE_FIELDS, name + ", tiles of 64")


@pytest.mark.gpu
def test_edge_coverage_of_device_chains(ctx):
    """Chains straight from fg_chain_alignments: its (aln_off, aln) layout is fg_edge_coverage's"""
    import read_chain_restate as RC
    from flye_amd import gpu
    queries = [q for name in ("read_diff", "graph_diff", "equal_best") for q in RC.crafted_cases()[name]]
    cb = RC.from_specs(queries)
    recs = cb.recs()
    _, aln_off, aln, _ = ctx.chain_alignments(recs, cb.query_off, gpu.ChainParams(**cb.params), cb.first_ext_id, cb.node_left,
                                              cb.node_right)
    depth = np.diff(aln_off.astype(np.int64))
    assert (depth > 1).any() and (depth == 1).any()
    n_ext = len(cb.node_left)
    edge_of = np.arange(n_ext) % 5
    edge_len = [300, 640, 90, 1000, 561]
    eb = R.EdgeBatch(100, np.stack([recs["ext_id"], recs["ext_begin"], recs["ext_end"]], 1),
                     [aln[int(aln_off[c]):int(aln_off[c + 1])].tolist() for c in range(len(depth))], cb.first_ext_id, edge_of, edge_len)
    want = R.restate_edges(eb)
    assert R.same(want, R.native_edges(eb), R.EDGE_FIELDS) and want["sum"].sum() > 0
    got = ctx.edge_coverage(100, recs, aln, aln_off, cb.first_ext_id, edge_of, edge_len)
    assert_same(dict(zip(R.EDGE_FIELDS, got)), want, R.EDGE_FIELDS, "device chains")


# ---- 8. argument checks ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_errors(ctx):
    from flye_amd import gpu
    L = ctx.L
    b = crafted()["overhang"]
    recs, off, ln = b.recs(), b.query_off, b.query_len
    P = b.coverage_params()

    def call(p=P, r=recs, o=off, nq=b.n_queries, lens=ln, out=True):
        res = gpu.CoverageBatch()
        rc = L.fg_read_coverage(ctx.h, C.byref(p) if p is not None else None, r.ctypes.data if r is not None else None,
                                o.ctypes.data if o is not None else None, nq, lens.ctypes.data if lens is not None else None,
                                C.byref(res) if out else None)
        if rc == 0:
            L.fg_release_coverage(C.byref(res))
        return rc

    assert call() == 0
    ctx.kernel_times()
    assert call(p=None) == -3 and call(out=False) == -3
    assert call(r=None) == -3 and call(o=None) == -3 and call(lens=None) == -3
    down = off.copy()
    down[2] = down[1] - 1
    assert call(o=down) == -3
    for field, bad in (("window", 0), ("window", -5), ("max_overhang", -1), ("max_drop_rate", 0.0), ("max_drop_rate", -1.0),
                       ("max_drop_rate", float("nan"))):
        p = b.coverage_params()
        setattr(p, field, bad)
        assert call(p=p) == -3, field
    neg = ln.copy()
    neg[5] = -1
    assert call(lens=neg) == -3
    for what, change in (("cur_len != query_len", dict(cur_len=4999)), ("cur_begin < 0", dict(cur_begin=-1)),
                         ("cur_end < cur_begin", dict(cur_begin=700, cur_end=699)), ("cur_end > cur_len", dict(cur_end=5001)),
                         ("ext_begin < 0", dict(ext_begin=-1)), ("ext_end < ext_begin", dict(ext_begin=5, ext_end=4)),
                         ("ext_end > ext_len", dict(ext_end=int(recs["ext_len"][3]) + 1))):
        r = recs.copy()
        for field, value in change.items():
            r[field][3] = value
        assert call(r=r) == -3, what
    assert b"fg_read_coverage" in L.fg_last_error(ctx.h)
    ok = recs.copy()
    ok["cur_end"][2] = ok["cur_begin"][2]           # an empty cur range and cur_end = cur_len are legal
    ok["cur_end"][1] = ok["cur_len"][1]
    assert call(r=ok) == 0
    assert call(r=None, o=None, nq=0, lens=None) == 0
    # every refusal came before device work, and the context still serves
    check_reads(ctx, b, expected("overhang"), "after the refusals")

    e, want = edge_cases()["rules"]
    erecs = e.recs()

    def ecall(window=100, r=erecs, n_recs=None, a=e.aln, o=e.aln_off, first=e.first_ext_id, eo=e.edge_of, n_ext=None, el=e.edge_len,
              n_edges=None, out=True):
        res = gpu.EdgeCoverageBatch()
        ptr = lambda x: x.ctypes.data if x is not None else None
        rc = L.fg_edge_coverage(ctx.h, window, ptr(r), len(erecs) if n_recs is None else n_recs, ptr(a), ptr(o), len(e.aln_off) - 1,
                                first, len(e.edge_of) if n_ext is None else n_ext, ptr(eo), len(e.edge_len) if n_edges is None else n_edges,
                                ptr(el), 1, C.byref(res) if out else None)
        if rc == 0:
            L.fg_release_edge_coverage(C.byref(res))
        return rc

    assert ecall() == 0
    assert ecall(window=0) == -3 and ecall(window=-1) == -3 and ecall(out=False) == -3
    assert ecall(n_recs=len(erecs) - 1) == -3                           # an aln index out of recs
    assert ecall(first=e.first_ext_id + 1) == -3 and ecall(n_ext=len(e.edge_of) - 1) == -3
    assert ecall(n_edges=6) == -3                                       # edge_of names edge 6
    bad_len = e.edge_len.copy()
    bad_len[2] = -1
    assert ecall(el=bad_len) == -3
    down = e.aln_off.copy()
    down[3] = down[2] - 1
    assert ecall(o=down) == -3
    assert ecall(r=None) == -3 and ecall(a=None) == -3 and ecall(o=None) == -3 and ecall(eo=None) == -3 and ecall(el=None) == -3
    assert b"fg_edge_coverage" in L.fg_last_error(ctx.h)
    assert_same(device_edges(ctx, e), want, R.EDGE_FIELDS, "after the refusals")
    got = ctx.edge_coverage(100, erecs[:0], [], [0], 0, [], [])
    assert got[0].tolist() == [0] and len(got[2]) == 0


# ---- 9. end to end, against real overlaps ---------------------------------------------------------------------------
def batch_of(lists, lens, params):
    return R.ReadBatch([(int(n), np.stack([x[f].astype(np.int64) for f in R.COLS], 1).tolist() if len(x) else [])
                        for x, n in zip(lists, lens)], params)


@pytest.mark.gpu
def test_chimera_detector_end_to_end(built):
    from flye_amd import config, gpu, synth
    rs = synth.simulate(seed=2024, genome_len=40_000, coverage=25, kind="pb_raw").filter_min_len(1000)
    cfg = config.preset("raw")
    c = gpu.Context(int(cfg["kmer_size"]), 0)
    c.set_reads(rs, 0)
    vi = gpu.VertexIndex(c, float(int(cfg["assemble_kmer_sample"])))
    vi.build(cfg)
    det = gpu.OverlapDetector.for_assemble(c, vi, cfg)
    oc = gpu.OverlapContainer(det)
    fwd = list(range(0, 2 * rs.n, 2))
    assert rs.n == 113
    base = dict(window=100, max_overhang=int(cfg["maximum_overhang"]), max_drop_rate=5.0)      # asm_defaults.cfg:8, :10
    assert config.assemble_stage("raw")["chimera_window"] == 100 and config.assemble_stage("raw")["max_coverage_drop_rate"] == 5

    # estimateGlobalCoverage with a recorded rand() sequence: the same picks, the pooled median on the host
    draws = np.random.default_rng(5).integers(0, 2 ** 31 - 1, 2 * rs.n).tolist()
    chim = gpu.ChimeraDetector(c, oc, cfg, False)
    feed = iter(draws)
    cov = chim.estimateGlobalCoverage(lambda: next(feed))
    n_seqs = 2 * rs.n
    rate = n_seqs // min(1000, n_seqs)
    picks = [i for i in range(n_seqs) if draws[i] % rate == 0]
    lists = [oc.lazySeqOverlaps(i) for i in picks]
    lens = [int(rs.length[i >> 1]) for i in picks]
    want = R.restate_reads(batch_of(lists, lens, dict(base, overlap_coverage=0, uneven_coverage=0)))
    pooled = [want["full"][int(want["win_off"][q]):int(want["win_off"][q + 1])] for q in range(len(picks)) if want["max"][q]]
    v = np.sort(np.concatenate(pooled))
    assert cov == int(v[min(len(v) * 50 // 100, len(v) - 1)]) == 24
    assert sum(len(oc.lazySeqOverlaps(i)) for i in fwd) == 5444

    for uneven in (False, True):
        chim = gpu.ChimeraDetector(c, oc, cfg, uneven)
        chim._overlapCoverage = cov
        got = chim.classify(fwd)
        b = batch_of([oc.lazySeqOverlaps(i) for i in fwd], rs.length, dict(base, overlap_coverage=cov, uneven_coverage=int(uneven)))
        want = R.restate_reads(b)
        assert R.same(want, R.native_reads(b), R.READ_FIELDS)
        print("uneven", uneven, "chimeric", int(got.sum()), "of", len(fwd))
        assert np.array_equal(got, want["chimeric"]) and int(got.sum()) == 2
        for i in (0, 10, int(np.flatnonzero(got)[0]) * 2):
            assert chim.isChimeric(i + 1) == bool(got[i >> 1]) == chim.testReadByCoverage(i)
            assert np.array_equal(chim.getReadCoverage(i), want["full"][int(want["win_off"][i >> 1]):int(want["win_off"][(i >> 1) + 1])])
        # a reverse-complement id asked first: its own records decide, and the forward id inherits
        fresh = gpu.ChimeraDetector(c, oc, cfg, uneven)
        fresh._overlapCoverage = cov
        rc_want = R.restate_reads(batch_of([oc.lazySeqOverlaps(5)], [rs.length[2]], dict(base, overlap_coverage=cov,
                                                                                          uneven_coverage=int(uneven))))
        assert fresh.isChimeric(5) == bool(rc_want["chimeric"][0]) == fresh.isChimeric(4)

    # getCachedCoverage / isRepetitiveRegion on force-local records of ten reads
    chim = gpu.ChimeraDetector(c, oc, cfg, False)
    for i in fwd[:20:2]:
        local = oc.quickSeqOverlaps(i, 0, True)
        want = R.restate_reads(batch_of([local], [rs.length[i >> 1]], dict(base, overlap_coverage=0, uneven_coverage=0)))
        full, junction = chim.getCachedCoverage(i)
        assert np.array_equal(full, want["full"]) and np.array_equal(junction, want["junction"])
        n = int(rs.length[i >> 1])
        for start, end in ((0, n), (0, 1500), (n - 1500, n), (n // 3, 2 * n // 3), (500, 500), (-300, 250)):
            lo, hi = max(0, int(start / 100)), min(len(full), int(end / 100))
            sus = sum(1 for pos in range(lo, hi) if np.float32(0.75) * np.float32(full[pos]) <= np.float32(junction[pos]))
            rep = hi > lo and bool(np.float32(sus) / np.float32(hi - lo) > np.float32(0.75))
            assert chim.isRepetitiveRegion(i, start, end) == rep, (i, start, end)
    c.close()
