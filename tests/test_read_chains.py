"""fg_chain_alignments: the edge-chain step of ReadAligner::alignReads (reference src/repeat_graph/read_aligner.cpp:
212-262: the lambda's filter, its std::sort, chainReadAlignments, before the divergence gate) on the device, and
Context.align_reads, the whole per-read body of alignReads on top of it.

No program of the reference that is built here prints chains, so the yardstick is a restatement pinned in two
independent forms (tests/read_chain_restate.py: numpy / Python on predecessor arrays with oracle.std_sort_perm, and
tests/native/read_chain_driver.cpp: chain objects in two std::deques under the real std::sort).  The first test pins
that they agree on every case the device tests use; it needs no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import read_chain_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ_SEEDS = list(range(100, 112))

_CACHE = {}


def crafted_batches():
    """name -> Batch: every crafted group as one batch of queries (built once)"""
    if "crafted" not in _CACHE:
        b = {name: R.from_specs(qs) for name, qs in R.crafted_cases().items()}
        b["tied_begin"] = R.from_specs(R.tied_begin_queries())
        b["tied_score"] = R.from_specs(R.tied_score_queries())
        b["wave_edges"] = R.from_specs(R.wave_edge_queries())
        _CACHE["crafted"] = b
    return _CACHE["crafted"]


CRAFTED_NAMES = ["filter", "read_diff", "graph_diff", "jump_div", "can_extend", "can_be_extended", "node_mismatch", "score_edges",
                 "equal_best", "cleanup", "empty_shapes", "tied_begin", "tied_score", "wave_edges"]


def expected(name):
    """The restatement's result for a crafted batch (computed once, never changed)"""
    key = ("want", name)
    if key not in _CACHE:
        _CACHE[key] = R.restate(crafted_batches()[name])
    return _CACHE[key]


def fuzz(seed):
    """(batch, the native form's result) of a fuzz seed, computed once"""
    key = ("fuzz", seed)
    if key not in _CACHE:
        b = R.fuzz_batch(seed)
        _CACHE[key] = (b, R.run_native(b))
    return _CACHE[key]


def chains_of(res, q):
    off, aoff, aln, score = (np.asarray(x).astype(np.int64) for x in res[:4])
    return [(int(score[c]), aln[aoff[c]:aoff[c + 1]].tolist()) for c in range(off[q], off[q + 1])]


def stable_differs(batch):
    """the queries on which a stable sort in place of std::sort's permutation changes the result"""
    return [q for q in range(batch.n_queries)
            if not R.same(R.restate(batch, queries={q}), R.restate(batch, perm=R.stable_perm, queries={q}))]


def check_crafted_expectations(name, want):
    """What each crafted group is there to show, read off the restatement's result"""
    b = crafted_batches()[name]
    n_chains = np.diff(want[0].astype(np.int64)).tolist()
    depth = np.diff(want[1].astype(np.int64)).tolist()
    score = want[3].tolist()
    if name == "filter":                # ext_len 899 / 900; min(range) 500 / 500 / 501 / 501
        assert n_chains == [1, 0, 0, 1, 0, 1]
    elif name == "read_diff":           # max_jump - 1 joins, max_jump does not; -max_read_overlap does not, one more does
        assert [len(chains_of(want, q)[0][1]) for q in range(5)] == [2, 1, 1, 2, 2] and n_chains == [1, 2, 1, 1, 1]
        assert score[0] == 200 - 299 // 50
    elif name == "graph_diff":
        assert n_chains == [1, 2, 1, 1, 2]
    elif name == "jump_div":            # 100 -> 0, 101 / 149 -> 2, 150 -> 3
        assert score == [200, 198, 198, 197, 198, 197, 200]
    elif name == "can_extend":
        assert n_chains == [1, 2]
    elif name == "can_be_extended":     # the first alignment active: it wins; frozen: it comes second and loses
        assert chains_of(want, 0) == [(100, [0])] and chains_of(want, 1) == [(100, [3])]
    elif name == "node_mismatch":
        assert n_chains == [2, 1]
    elif name == "score_edges":         # totals 1 / 0 / -1 / 1 / 0 / 1: only a total > 0 extends
        assert [max(len(a) for _, a in chains_of(want, q)) for q in range(6)] == [1, 1, 1, 1, 1, 2]
        assert n_chains == [1, 2, 2, 1, 2, 1]
    elif name == "equal_best":          # the earlier of two equal candidates in active order
        assert [chains_of(want, q)[0][1] for q in range(3)] == [[0, 3], [4, 7], [9, 11]]
    elif name == "cleanup":
        assert want[4]["cleanups"] == 4      # (4, 1), (3, 1), (2, 0), (8, 6): numOutdated = size / 2 + 1; the others size / 2
        off = b.query_off.astype(np.int64)
        for q, n_out, fires in ((0, 3, False), (1, 4, True), (2, 2, False), (3, 3, True), (4, 1, False), (7, 7, False), (8, 8, True)):
            first = chains_of(want, q)[0][1][0] - off[q]
            assert first == (n_out if fires else 0), (q, first)      # a live chain wins only after a cleanup
            assert off[q + 1] - off[q] <= 16
    elif name == "empty_shapes":
        assert n_chains == [0, 1, 0, 0, 0, 1, 0, 0, 0]
    elif name == "tied_begin":
        assert np.diff(b.query_off.astype(np.int64)).tolist() == [16, 17, 17, 23, 100, 101]
        assert want[4]["tied_first"] == 5 and stable_differs(b)
        assert 0 not in stable_differs(b)           # up to 16 elements std::sort is an insertion sort
    elif name == "tied_score":
        assert np.diff(b.query_off.astype(np.int64)).tolist() == [16, 17, 20, 33, 100]
        assert want[4]["tied_second"] == 4 and stable_differs(b) and 0 not in stable_differs(b)
    elif name == "wave_edges":
        assert n_chains[5:7] == [70, 70] and want[4]["cleanups"] > 60 and max(depth) == 150


# ---- 1. the two forms of the yardstick agree (no GPU) ---------------------------------------------------------------
def test_restatements_agree_on_every_case(built):
    for name in CRAFTED_NAMES:
        b = crafted_batches()[name]
        want = expected(name)
        native = R.run_native(b)
        assert R.same(want, native), name
        assert want[4] == native[4], name
        check_crafted_expectations(name, want)
    total = R.new_stats()
    for seed in FUZZ_SEEDS:
        b, native = fuzz(seed)
        py = R.restate(b)
        assert R.same(py, native), seed
        assert py[4] == native[4], seed
        for k in total:
            total[k] += py[4][k]
        assert all(v > 0 for v in py[4].values()), (seed, py[4])
        sizes = np.diff(b.query_off.astype(np.int64))
        assert b.n_queries == 3000 and sizes.min() == 0 and 200 <= sizes.max() < 400
    assert total["cleanups"] > 1000 and total["tied_first"] > 1000 and total["tied_second"] > 1000 and total["rejected"] > 1000
    # threads change nothing in the native form (tools/read_chain_bench.py times it on 1 and on 16)
    b, native = fuzz(FUZZ_SEEDS[0])
    assert R.same(R.run_native(b, threads=5), native)


# ---- 2. exported and declared (no GPU; fails without the feature) ---------------------------------------------------
def _header_struct(name):
    text = open(os.path.join(ROOT, "include", "flye_gpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"struct " + name + r"\s*\{(.*?)\};", text, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = decl.split(None, 1)
        fields += [(n.strip(), ctype) for n in names.split(",")]
    return fields


def test_symbols_and_struct_layouts(built):
    from flye_amd import gpu
    lib = gpu.load_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flye_gpu.h")).read(), flags=re.S)
    for sym in ("fg_chain_alignments", "fg_release_chains"):
        assert re.search(r"\b" + sym + r"\s*\(", header), sym + " is not declared in include/flye_gpu.h"
        assert hasattr(lib, sym) and sym in gpu.ABI_SYMBOLS
    assert lib.fg_abi_version() == 4 and "#define FG_ABI_VERSION 4" in header
    assert int(re.search(r"#define FG_CHAIN_MAX_RECS (\d+)", header).group(1)) >= 65536
    ctypes_of = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "uint64_t*": C.POINTER(C.c_uint64),
                 "int32_t*": C.POINTER(C.c_int32), "void*": C.c_void_p}
    for cname, cls in (("fg_chain_params", gpu.ChainParams), ("fg_chain_batch", gpu.ChainBatch)):
        declared = [(n, ctypes_of[re.sub(r"\s+", "", t)]) for n, t in _header_struct(cname)]
        assert declared == list(cls._fields_), cname
    assert C.sizeof(gpu.ChainParams) == 24 and C.sizeof(gpu.ChainBatch) == 64
    assert [n for n, _ in gpu.ChainParams._fields_] == ["max_jump", "max_read_overlap", "min_alignment", "max_separation", "long_edge",
                                                       "big_alignment"]
    # no context, no call; releasing nothing is harmless
    assert lib.fg_chain_alignments(None, None, None, None, 0, 0, 0, None, None, None) == -3
    lib.fg_release_chains(None)
    empty = gpu.ChainBatch()
    lib.fg_release_chains(C.byref(empty))
    from flye_amd import config
    p = gpu.ChainParams.from_config(config.preset("subasm"), 1000)
    assert (p.max_jump, p.max_read_overlap, p.min_alignment, p.max_separation, p.long_edge, p.big_alignment) == (500, 50, 1000, 500, 900, 500)
    assert gpu.ChainParams.from_config(config.preset("raw"), 3000).max_jump == 1500


# ---- the device -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(built):
    from flye_amd import gpu
    c = gpu.Context(17, 0)          # no reads, no index: the step needs a device and a stream
    yield c
    c.close()


def device(ctx, batch):
    from flye_amd import gpu
    return ctx.chain_alignments(batch.recs(), batch.query_off, gpu.ChainParams(**batch.params), batch.first_ext_id, batch.node_left,
                                batch.node_right)


def assert_same(got, want, what):
    for field, g, w in zip(("chain_off", "aln_off", "aln", "score"), got, want):
        assert np.array_equal(np.asarray(g).astype(np.int64), np.asarray(w).astype(np.int64)), (what, field)


@pytest.mark.gpu
def test_argument_errors(ctx):
    from flye_amd import gpu
    b = crafted_batches()["read_diff"]
    recs, off = b.recs(), b.query_off
    P = gpu.ChainParams(**b.params)
    L = ctx.L

    def call(p=P, r=recs, o=off, nq=b.n_queries, first=b.first_ext_id, nl=b.node_left, nr=b.node_right, n_ext=None, out=True):
        res = gpu.ChainBatch()
        rc = L.fg_chain_alignments(ctx.h, C.byref(p) if p is not None else None, r.ctypes.data if r is not None else None,
                                   o.ctypes.data if o is not None else None, nq, first, len(b.node_left) if n_ext is None else n_ext,
                                   nl.ctypes.data if nl is not None else None, nr.ctypes.data if nr is not None else None,
                                   C.byref(res) if out else None)
        if rc == 0:
            L.fg_release_chains(C.byref(res))
        return rc

    assert call() == 0
    assert call(p=None) == -3 and call(out=False) == -3
    assert call(r=None) == -3 and call(o=None) == -3 and call(nl=None) == -3 and call(nr=None) == -3
    down = off.copy()
    down[2] = down[1] - 1
    assert call(o=down) == -3
    for field, bad in (("max_jump", 0), ("max_jump", -1), ("max_read_overlap", -1), ("min_alignment", -1), ("max_separation", -1),
                       ("long_edge", -1), ("big_alignment", -1)):
        p = gpu.ChainParams(**dict(b.params, **{field: bad}))
        assert call(p=p) == -3, field
    assert call(p=gpu.ChainParams(**dict(b.params, min_alignment=0, max_separation=0, max_read_overlap=0))) == 0
    assert call(first=b.first_ext_id + 1) == -3 and call(n_ext=len(b.node_left) - 1) == -3     # an ext_id below / above the tables
    for what, change in (("cur_begin < 0", dict(cur_begin=-1)), ("cur_end < cur_begin", dict(cur_begin=700, cur_end=699)),
                         ("ext_begin < 0", dict(ext_begin=-1)), ("ext_end < ext_begin", dict(ext_begin=5, ext_end=4)),
                         ("ext_end > ext_len", dict(ext_end=int(recs["ext_len"][3]) + 1))):
        r = recs.copy()
        for field, value in change.items():
            r[field][3] = value
        assert call(r=r) == -3, what
    ok = recs.copy()
    ok["ext_end"][3] = ok["ext_len"][3]          # ext_end = ext_len and an empty cur range are legal
    ok["cur_end"][2] = ok["cur_begin"][2]
    assert call(r=ok) == 0
    assert b"fg_chain_alignments" in L.fg_last_error(ctx.h)
    # a query beyond the documented limit
    big = np.array([0, 65537], np.uint64)
    assert call(o=big, nq=1, r=np.zeros(65537, gpu.REC_DTYPE)) == -3
    # nothing to do: an empty batch, with or without arrays
    got = ctx.chain_alignments(recs[:0], np.zeros(1, np.uint64), P, 0, [], [])
    assert [x.tolist() for x in got] == [[0], [0], [], []]
    assert call(r=None, o=None, nq=0, nl=None, nr=None, n_ext=0) == 0
    got = ctx.chain_alignments(recs[:0], np.zeros(4, np.uint64), P, 0, [], [])
    assert [x.tolist() for x in got] == [[0, 0, 0, 0], [0], [], []]


@pytest.mark.gpu
@pytest.mark.parametrize("name", CRAFTED_NAMES)
def test_crafted_queries(ctx, name):
    """Every boundary of the step one step on either side, field for field against the restatement"""
    b = crafted_batches()[name]
    want = expected(name)
    check_crafted_expectations(name, want)
    got = device(ctx, b)
    print(name, "chains per query", np.diff(got[0].astype(np.int64)).tolist())
    assert_same(got, want, name)
    kt = ctx.kernel_times()
    if len(want[3]):
        for k in ("k_rc_filter", "k_rc_gather", "k_rc_chain", "k_rc_select", "k_rc_write"):
            assert k in kt, (k, sorted(kt))
    # the records' position in the caller's array is what comes back: the same queries behind a prefix of other records
    if name == "equal_best":
        recs = b.recs()
        from flye_amd import gpu
        shifted = ctx.chain_alignments(np.concatenate([recs[:5], recs]), b.query_off + np.uint64(5), gpu.ChainParams(**b.params),
                                       b.first_ext_id, b.node_left, b.node_right)
        assert_same((shifted[0], shifted[1], shifted[2] - np.uint64(5), shifted[3]), want, "shifted")


@pytest.mark.gpu
@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz(ctx, monkeypatch, seed):
    """About 3000 queries of 0 - 40 records (a few of several hundred) from ranges small enough that ties and every
    threshold occur often; the default sub-batch size and one small enough for a dozen sub-batches give the literal
    form's result.  (The step has one path: all state in global scratch, no switch to force.)"""
    b, native = fuzz(seed)
    st = native[4]
    assert st["cleanups"] > 0 and st["tied_first"] > 0 and st["tied_second"] > 0 and st["rejected"] > 0, st
    got = device(ctx, b)
    print("seed", seed, len(b.table), "records,", len(native[3]), "chains,", st, "device call %.3f s" % ctx.last_chain_seconds)
    assert_same(got, native, "default sub-batches")
    monkeypatch.setenv("FG_READCHAIN_BATCH_RECS", "5000")
    small = device(ctx, b)
    assert_same(small, native, "sub-batches of 5000 records")
    assert ctx.kernel_times()["k_rc_chain"][1] >= 10          # it did run in several sub-batches
    monkeypatch.setenv("FG_READCHAIN_BATCH_RECS", "1")        # every query alone
    few = R.Batch([b.table[int(b.query_off[q]):int(b.query_off[q + 1])].tolist() for q in range(40)], b.node_left, b.node_right,
                  b.first_ext_id, b.params)
    alone = device(ctx, few)
    n = int(native[0][40])
    assert_same(alone, (native[0][:41], native[1][:n + 1], native[2][:int(native[1][n])], native[3][:n]), "one query per sub-batch")


E2E = [("edges_raw", False, False), ("edges_raw", True, False), ("edges_hifi", False, False), ("edges_hifi", True, False),
       ("edges_hifi", False, True), ("edges_hifi", True, True)]
MAX_DIVERGENCE = {"edges_raw": 0.125, "edges_hifi": 0.0078}     # near the median chain divergence of the case


@pytest.mark.gpu
@pytest.mark.parametrize("name,realign,use_hpc", E2E)
def test_align_reads_end_to_end(built, golden_cases, name, realign, use_hpc):
    """Context.align_reads on the inputs of the edges_* golden cases = the same composition with the restatement in the
    middle: chains, complements, node tables at the complement ids, the divergence bits of every chain and the gate."""
    from flye_amd import config, gpu
    case = golden_cases[name]
    cfg = config.preset(case["preset"])
    c, det, fwd, n_edges = R.edges_context(case, cfg)
    node_left, node_right = R.synthetic_nodes(n_edges)
    cp = gpu.ChainParams.from_config(cfg, case["min_overlap"])
    max_div = MAX_DIVERGENCE[name]
    res = c.align_reads(det.p, fwd, cp, node_left, node_right, max_div, realign=realign, use_hpc=use_hpc)

    # the composition in the test
    ov = det.getSeqOverlapsBatch(fwd)
    recs = np.asarray(ov.recs)
    off = np.asarray(ov.query_off).astype(np.int64)
    tab = np.stack([recs[f].astype(np.int64) for f in R.REC_FIELDS], 1)
    params = {k: getattr(cp, k) for k, _ in gpu.ChainParams._fields_}
    batch = R.Batch([tab[off[i]:off[i + 1]].tolist() for i in range(len(fwd))], node_left, node_right, 0, params)
    chain_off, aln_off, aln, _, stats = R.restate(batch)
    alns = recs[aln.astype(np.int64)]
    div = c.edit_ranges(alns, use_hpc)[3] if realign else alns["seq_divergence"]
    chain_div = gpu.chain_divergence(alns["cur_end"] - alns["cur_begin"], div, aln_off)
    good = chain_div < np.float32(max_div)
    depth = np.diff(aln_off.astype(np.int64))
    print(name, "realign", realign, "hpc", use_hpc, len(recs), "records,", len(depth), "chains,", int((depth > 1).sum()), "of two or more,",
          int((~good).sum()), "fail the gate; divergence quantiles", np.quantile(chain_div, [0, 0.25, 0.5, 0.75, 1]), stats)
    assert (depth > 1).any(), "no read yields a chain of two or more alignments"
    assert (~good).any() and good.any(), "the gate must reject some chains and keep some"
    assert np.array_equal(res.all_chain_off.astype(np.int64), chain_off.astype(np.int64))
    assert np.array_equal(res.divergence.view(np.uint32), chain_div.view(np.uint32))
    assert len(res.chain_off) == len(fwd) + 1
    for i in range(len(fwd)):
        mine = [alns[int(aln_off[k]):int(aln_off[k + 1])] for k in range(int(chain_off[i]), int(chain_off[i + 1])) if good[k]]
        want = mine + [gpu.complement(ch)[::-1] for ch in mine]
        got = res.chains_of(i)
        assert len(got) == len(want), i
        for g, w in zip(got, want):
            assert g.tobytes() == w.tobytes(), i
        for k in range(int(res.chain_off[i]), int(res.chain_off[i + 1])):
            a, b = int(res.aln_off[k]), int(res.aln_off[k + 1])
            ids = res.recs["ext_id"][a:b].astype(np.int64)
            assert np.array_equal(res.node_left[a:b], node_left[ids]) and np.array_equal(res.node_right[a:b], node_right[ids])
            if k - int(res.chain_off[i]) >= len(mine):      # a complement chain: the read's other strand, the complement edges
                assert (res.recs["cur_id"][a:b] == (int(fwd[i]) ^ 1)).all()
                assert np.array_equal(ids[::-1] ^ 1, mine[k - int(res.chain_off[i]) - len(mine)]["ext_id"].astype(np.int64))
    c.close()
