"""fg_confirm_positions / fg_classify_reads / gpu.ReadPartitioner: Trestle's partition_reads (flye/trestle/trestle.py) on the
device.

Yardsticks: the records of the reference's own Python (tests/golden/partition_*.gz and partition_cases.json, made by
make_partition_golden.py) and the restatement tests/partition_restate.py.  Without a GPU the restatement is pinned on every
golden run, the mirror's host parts (collapsing, writers) with the restated SAM reader on the files the reference's own
partition_reads left, and the host-only parts of the ABI are checked; with one, both calls on every golden run and on fuzz
seeds, every output array against the restatement, the mirror's two files against the golden text byte for byte, the
sub-batch and tile cuts, windows into larger arrays, empty batches and the argument errors.  Parity is exact everywhere:
there is no tolerance."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import bubbles_restate as R
import partition_restate as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fg_confirm_positions", "fg_release_confirm", "fg_classify_reads", "fg_release_classify")
CASES = json.load(open(os.path.join(R.GOLDEN, "partition_cases.json")))
_CACHE = {}


def restated(name, run=None):
    """one run through the restatement, computed once"""
    if name not in _CACHE:
        run = run or dict(P.CONFIRM_RUNS, **P.CLASSIFY_RUNS)[name]()
        if "buffer_count" in run:
            res = [P.classify(j, run["buffer_count"]) for j in run["jobs"]]
        else:
            res = [P.confirm(j) for j in run["jobs"]]
        _CACHE[name] = dict(run=run, res=res)
    return _CACHE[name]


# ---- 1. the restatement against the reference's records (no GPU) -----------------------------------------------------
@pytest.mark.parametrize("name", sorted(P.CONFIRM_RUNS))
def test_confirm_restatement_equals_the_reference(name):
    g, meta = restated(name), CASES["confirm"][name]
    assert P.confirm_digest(g["run"]) == meta["input_sha256"], "the generator no longer makes the stored input"
    assert len(g["res"]) == len(meta["jobs"])
    for j, (r, m) in enumerate(zip(g["res"], meta["jobs"])):
        assert P.digests(r, P.CONFIRM_KEYS) == m["lists_sha256"], j
        assert P.cons_digest(r["cons"]) == m["cons_sha256"], j
        assert [len(r[k]) for k in P.CONFIRM_KEYS] + [sum(len(c) for c in r["cons"])] == m["n"], j


@pytest.mark.parametrize("name", sorted(P.CLASSIFY_RUNS))
def test_classify_restatement_equals_the_reference(name):
    g, meta = restated(name), CASES["classify"][name]
    assert P.classify_digest(g["run"]) == meta["input_sha256"], "the generator no longer makes the stored input"
    assert g["run"]["buffer_count"] == meta["buffer_count"] and len(g["res"]) == len(meta["jobs"])
    for j, (r, m) in enumerate(zip(g["res"], meta["jobs"])):
        assert P.digests(r, P.READ_KEYS + ("aln_score",)) == m["arrays_sha256"], j
        assert [r["status"].count(k) for k in range(3)] == m["statuses"], j


def sam_texts(name):
    return {k: R.read_gz("partition_%s.%s.gz" % (name, k)) for k in ("confirmed", "part")}


@pytest.mark.parametrize("name", sorted(P.SAMS))
def test_sam_inputs_are_the_stored_ones(name):
    run, meta = P.SAMS[name](), CASES["sams"][name]
    assert P.sam_digest(run) == meta["input_sha256"]
    texts = sam_texts(name)
    assert [texts["confirmed"].count("\n"), texts["part"].count("\n")] == meta["lines"] == [24, len(run["headers_to_id"]) + 1]


@pytest.mark.parametrize("name", ["sam_first", "sam_out"])
def test_restated_reader_collapse_and_partition_equal_partition_reads(name, built, tmp_path):
    """the restated SAM reader (tests/cigar_restate.py), the mirror's host-side collapse, then the restatement: the two
    files the reference's own partition_reads left"""
    import cigar_restate as G
    from flye_amd import gpu
    run = P.SAMS[name]()
    fasta = lambda text: {text.split("\n")[0][1:]: text.split("\n")[1].encode().translate(R.TO_ACGT).decode()}
    first = lambda sam, target: G.chunks(dict(sam=run["files"][sam].encode(), contigs=fasta(run["files"][target]), max_coverage=1000,
                                              use_secondary=False))[0][1]
    with open(str(tmp_path / "positions.txt"), "w") as f:
        f.write(run["files"]["positions.txt"])
    pos = gpu.ReadPartitioner.read_positions(str(tmp_path / "positions.txt"))
    raw = [first("cons_aln_%d.sam" % e, "template.fasta") for e in run["edges"]]
    assert [len(x) for x in raw] == ([2, 1, 1] if name == "sam_out" else [1, 1])
    edges = [gpu.ReadPartitioner._collapse_cons_aln([x]) for x in raw]
    if name == "sam_out":                                         # the two records became one, 7 'N' between them
        a, b = sorted(raw[0], key=lambda x: x.trg_start)
        assert edges[0].trg_end == b.trg_end and edges[0].trg_seq.count("N") == 7 == b.trg_start - a.trg_end
    res = P.confirm(dict(side=("in", "out").index(run["side"]), edges=edges, pos=pos))
    assert P.confirmed_text(res, pos) == sam_texts(name)["confirmed"]
    number = {h: i for i, h in enumerate(run["headers_to_id"])}
    job = dict(n_reads=len(number), edges=[
        dict(pos=res["cons"][i], alns=[a._replace(qry_id="read_%d" % number[a.qry_id]) for a in first("read_aln_%d.sam" % e, "cons_%d.fasta" % e)])
        for i, e in enumerate(run["edges"])])
    got = P.classify(job, 3)
    assert P.partitioning_text(got, run["edges"], run["headers_to_id"]) == sam_texts(name)["part"]
    # the file holds a read with four alignments on an edge (0 from it) and reads with two
    per_read = np.bincount([P.read_number(a) for a in job["edges"][0]["alns"]], minlength=len(number))
    assert per_read[0] == 4 and 2 in per_read and 0 in per_read and {0, 1, 2} <= set(got["status"])


def test_classify_c_contains_what_it_is_for():
    g = restated("classify_c")
    tiles, votes = g["run"]["jobs"]
    rt, rv = g["res"]
    edge, = tiles["edges"]
    alns, pos = edge["alns"], edge["pos"]
    assert [len(a.trg_seq) for a in alns[:len(P.COLUMNS)]] == list(P.COLUMNS) == [63, 64, 65, 1023, 1024, 1025, 2049]
    gap = alns[-1]
    t = np.frombuffer(gap.trg_seq.encode(), np.uint8)
    # a whole tile of target gaps in front of a scored column; scored columns as the last and the first of a tile
    assert (t[1024:2048] == 45).all() and (t[:1024] != 45).all() and t[2048] != 45
    assert (gap.trg_start, gap.trg_end) == (100, 1140) and {1123, 1124} <= set(pos)            # columns 1023 and 2048
    assert gap.trg_seq[1023] == gap.qry_seq[1023] and gap.trg_seq[2048] == gap.qry_seq[2048]
    # trg_start, trg_end - 1, trg_end (not counted), -1, one beyond every alignment, a position twice and three times
    assert {100, 1139, 1140, -1} <= set(pos) and max(pos) >= max(a.trg_end for a in alns) and pos.count(500) == 2 and pos.count(600) == 3
    only = lambda lst: P.aln_score(gap, lst)
    assert only([100]) == only([1139]) == only([1123]) == only([1124]) == 1 and only([1140]) == only([-1]) == only([99]) == 0
    assert only([500]) == 1 and only([500, 500]) == 2 and only([600] * 3) == 3
    # equal letters, lower case on one side only: no match
    col = 1130 - 100 + 1024
    assert 1130 in pos and gap.qry_seq[col] == gap.trg_seq[col].lower() != gap.trg_seq[col] and only([1130]) == 0 and only([1131]) == 1
    assert rt["status"][-1] == 0 and rt["aln_counted"] == [1] * len(alns)                      # a read without alignments
    # the votes job, buffer 3: Partitioned (first edge, and a later edge that resets a tie), Tied by the second and by the
    # third branch, the reset rule, one edge of three, no alignment, None with alignments
    rows = list(zip(*[rv[k] for k in P.READ_KEYS]))
    assert g["run"]["buffer_count"] == 3 and len(votes["edges"]) == 3
    assert rows[0] == (2, 0, 9, 12) and rows[1] == (2, 1, 9, 12) and rows[2] == (1, -1, 7, 12) and rows[3] == (1, -1, 7, 12)
    on = lambda read, e: [i for i, a in enumerate(votes["edges"][e]["alns"]) if P.read_number(a) == read]
    assert [len(on(4, e)) for e in range(3)] == [1, 2, 3]
    first = [0, len(votes["edges"][0]["alns"]), len(votes["edges"][0]["alns"]) + len(votes["edges"][1]["alns"])]
    score = lambda e, i: rv["aln_score"][first[e] + i]
    kept = lambda e, i: rv["aln_counted"][first[e] + i]
    assert [score(1, i) for i in on(4, 1)] == [11, 4] and [kept(1, i) for i in on(4, 1)] == [0, 1]
    assert [score(2, i) for i in on(4, 2)] == [12, 13, 14] and [kept(2, i) for i in on(4, 2)] == [0, 0, 0]
    assert rows[4] == (1, -1, 6, 6 + 4 + 0)
    assert [len(on(5, e)) for e in range(3)] == [0, 1, 0] and rows[5] == (2, 1, 8, 8)
    assert rows[6] == rows[11] == (0, -1, 0, 0) and not any(on(6, e) for e in range(3))
    assert rows[7] == (0, -1, 0, 0) and len(on(7, 0)) == len(on(7, 1)) == 1
    # the same two scores in either edge order: top_score is a running maximum, so no order changes it; what the order
    # changes is the way there (a tie that a later edge resets), and the buffer decides between Tied and Partitioned
    assert rows[8] == rows[9] == (1, -1, 3, 3)
    zero = restated("classify_c0")
    assert zero["run"]["buffer_count"] == 0
    rows0 = list(zip(*[zero["res"][0][k] for k in P.READ_KEYS]))
    assert rows0[8] == (2, 0, 3, 3) and rows0[9] == (2, 1, 3, 3) and rows0[2] == (2, 1, 7, 12) and rows0[3] == (2, 0, 7, 12)
    # lower case in the target only, at a listed position: 19 of 20
    low = votes["edges"][2]["alns"][on(10, 2)[0]]
    assert low.trg_seq[30] == low.qry_seq[30].lower() != low.qry_seq[30] and rows[10] == (2, 2, 19, 19)


def test_confirm_c_contains_what_it_is_for():
    g = restated("confirm_c")
    jobs, res = g["run"]["jobs"], g["res"]
    seq = P.confirm_c_template()
    e0, e1, e2 = jobs[0]["edges"]
    assert jobs[0]["side"] == 0 and jobs[1]["side"] == 1 and jobs[1]["edges"] == jobs[0]["edges"]
    assert [(a.trg_start, a.trg_end) for a in (e0, e1, e2)] == [(0, 30), (5, 40), (2, 35)]          # min_end 30, max_start 5
    total = set(jobs[0]["pos"]["total"])
    judged = lambda r: set(r["conf_total"]) | set(r["rej_total"])
    assert {1, 3, 31, 33, 36} <= total and {1, 3} <= judged(res[0]) and not {31, 33, 36} & judged(res[0])
    assert {31, 33, 36} <= judged(res[1]) and not {1, 3} & judged(res[1]) and not {-1, 44, 48} & (judged(res[0]) | judged(res[1]))
    # an insertion before the first target column of e1, on that edge only: qry_ind - 1 with qry_start 0
    assert e1.trg_seq.startswith("--") and e1.qry_seq.startswith("AC") and e1.qry_start == 0
    assert 5 in res[0]["conf_ins"] and res[0]["cons"][1][0] == 1 and 1 not in res[0]["cons"][0][:1]
    # first edge '-' against a base: a deletion; a base against '-': a substitution, here of a position only `del` holds
    col = lambda a, p: [i for i, ch in enumerate(a.trg_seq) if ch != "-"][p - a.trg_start]
    assert e0.qry_seq[col(e0, 8)] == "-" and e1.qry_seq[col(e1, 8)] == seq[8] and 8 in res[0]["conf_del"]
    assert e0.qry_seq[col(e0, 10)] == seq[10] and e1.qry_seq[col(e1, 10)] == "-"
    assert 10 in res[0]["conf_total"] and 10 in res[0]["rej_del"] and 10 not in jobs[0]["pos"]["sub"]
    # 'N' on either side: nothing; the same substitution on every edge: nothing
    assert e0.qry_seq[col(e0, 12)] == "N" and e1.qry_seq[col(e1, 13)] == "N" and {12, 13, 16} <= set(res[0]["rej_total"])
    # a both-gap column, and a gap run shift_gaps moves (the deletion of 22 goes to 21)
    assert any(a == b == "-" for a, b in zip(e2.trg_seq, e2.qry_seq))
    moved = R.shift_gaps(e0.trg_seq, e0.qry_seq)
    assert moved != e0.qry_seq and e0.qry_seq[col(e0, 22)] == "-" and moved[col(e0, 21)] == "-" and moved[col(e0, 22)] == "T"
    # both entries of one position: the insertion entry before the other one
    assert 14 in res[0]["conf_sub"] and 26 in res[0]["conf_ins"]
    # positions no edge covers go nowhere; -1 in consensus_pos from a negative qry_start
    a0, a1 = jobs[2]["edges"]
    assert (a0.trg_end, a1.trg_start) == (10, 20) and 15 in jobs[2]["pos"]["total"]
    assert all(15 not in judged(res[j]) for j in (2, 3)) and res[3]["cons"] == [[], [-1]] and a1.qry_start == -7
    assert len(jobs[4]["edges"]) == 1 and res[4]["conf_ins"] == [7] and res[4]["rej_del"] == [9]      # one edge: insertions only
    assert not jobs[5]["pos"]["total"] and not judged(res[5])


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
    raw = open(os.path.join(ROOT, "include", "flye_gpu.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b" + sym + r"\s*\(", header), sym + " is not declared in include/flye_gpu.h"
        assert hasattr(lib, sym) and sym in gpu.ABI_SYMBOLS
    assert lib.fg_abi_version() == 4 and "#define FG_ABI_VERSION 4" in header
    assert _header_fields(header, "fg_confirm_batch") == [n for n, _ in gpu.ConfirmBatch._fields_]
    assert _header_fields(header, "fg_classify_batch") == [n for n, _ in gpu.ClassifyBatch._fields_]
    assert C.sizeof(gpu.ConfirmBatch) == 16 + 19 * 8 and C.sizeof(gpu.ClassifyBatch) == 16 + 8 * 8
    assert "fg_partition.hip" in re.search(r"^HIP_SRC := (.*)$", open(os.path.join(ROOT, "flye_amd", "csrc", "Makefile")).read(), re.M).group(1)
    for k in ("FG_PARTITION_BATCH_COLS", "FG_PARTITION_BATCH_JOBS", "FG_PARTITION_TILE"):
        assert k in raw and k in open(os.path.join(ROOT, "README.md")).read(), k
    assert hasattr(gpu.Context, "confirm_positions") and hasattr(gpu.Context, "classify_reads")
    assert hasattr(gpu.ReadPartitioner, "partition_reads")


def test_host_side_argument_errors_without_a_context(built):
    """what the library refuses before it needs a device: a NULL context; release of NULL and of an empty batch"""
    from flye_amd import gpu
    lib = gpu.load_library()
    b, cb = gpu.ConfirmBatch(), gpu.ClassifyBatch()
    assert lib.fg_confirm_positions(None, 0, *[None] * 16, C.byref(b)) == -3
    assert lib.fg_classify_reads(None, 3, 0, *[None] * 11, 0, C.byref(cb)) == -3
    lib.fg_release_confirm(None)
    lib.fg_release_classify(None)
    lib.fg_release_confirm(C.byref(b))
    lib.fg_release_classify(C.byref(cb))
    # the binding refuses offsets outside their arrays before it calls the library
    f = P.classify_arrays(restated("classify_d")["run"]["jobs"])
    ctx = gpu.Context.__new__(gpu.Context)
    with pytest.raises(ValueError):
        gpu.Context.classify_reads(ctx, 3, **dict(f, col_off=f["col_off"] + 1))
    f = P.confirm_arrays(restated("confirm_c")["run"]["jobs"])
    with pytest.raises(ValueError):
        gpu.Context.confirm_positions(ctx, **dict(f, total_off=f["total_off"] + 1))


# ---- 2. the device ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(built):
    from flye_amd import gpu
    c = gpu.Context(17, 0)          # no reads, no index: the calls need a device and a stream
    yield c
    c.close()


def check_confirm(res, want, first_job=0):
    e = 0
    for j, r in enumerate(want):
        confirmed, rejected = res.positions(first_job + j)
        for pre, d in (("conf_", confirmed), ("rej_", rejected)):
            for k in P.LIST_KEYS:
                assert d[k] == r[pre + k], (j, pre + k)
        for i, lst in enumerate(r["cons"]):
            assert res.consensus_pos(e + i) == lst, (j, i)
        e += len(r["cons"])
    assert len(res.cons_off) == e + 1 and all(len(getattr(res, k + "_off")) == len(want) + 1 for k in P.CONFIRM_KEYS)


def check_classify(res, want, scores=True):
    a = 0
    for j, r in enumerate(want):
        lo, hi = int(res.read_off[j]), int(res.read_off[j + 1])
        for k in P.READ_KEYS:
            assert np.array_equal(getattr(res, k)[lo:hi], r[k]), (j, k)
        if scores:
            n = len(r["aln_score"])
            assert np.array_equal(res.aln_score[a:a + n], r["aln_score"]) and np.array_equal(res.aln_counted[a:a + n], r["aln_counted"]), j
            a += n
    assert len(res.read_off) == len(want) + 1
    if scores:
        assert len(res.aln_score) == a == len(res.aln_counted)
    else:
        assert res.aln_score is None and res.aln_counted is None


def call_confirm(ctx, g, **changes):
    return ctx.confirm_positions(**dict(P.confirm_arrays(g["run"]["jobs"]), **changes))


def call_classify(ctx, g, want_scores=True, **changes):
    return ctx.classify_reads(g["run"]["buffer_count"], want_scores=want_scores, **dict(P.classify_arrays(g["run"]["jobs"]), **changes))


CONFIRM_FUZZ = {"confirm_fuzz_%d" % s: (lambda s=s: P.confirm_fuzz(s)) for s in (1, 2, 3)}
CLASSIFY_FUZZ = {"classify_fuzz_%d" % s: (lambda s=s: P.classify_fuzz(s)) for s in (1, 2, 3)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(P.CONFIRM_RUNS) + sorted(CONFIRM_FUZZ))
def test_confirm_on_the_device(ctx, name):
    g = restated(name, CONFIRM_FUZZ[name]() if name in CONFIRM_FUZZ else None)
    res = call_confirm(ctx, g)
    check_confirm(res, g["res"])
    assert {"k_bub_shift", "k_pt_tiles", "k_pt_scan", "k_cf_edge", "k_cf_mark", "k_cf_judge"} <= set(ctx.kernel_times())
    assert res.same_as(call_confirm(ctx, g))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(P.CLASSIFY_RUNS) + sorted(CLASSIFY_FUZZ))
def test_classify_on_the_device(ctx, name):
    g = restated(name, CLASSIFY_FUZZ[name]() if name in CLASSIFY_FUZZ else None)
    res = call_classify(ctx, g)
    check_classify(res, g["res"])
    if name in P.CLASSIFY_RUNS:
        assert {"k_cl_poscount", "k_pt_tiles", "k_pt_scan", "k_cl_score", "k_cl_sort", "k_cl_vote"} <= set(ctx.kernel_times())
    assert res.same_as(call_classify(ctx, g))
    check_classify(call_classify(ctx, g, want_scores=False), g["res"], scores=False)


@pytest.mark.gpu
def test_results_do_not_depend_on_the_cuts(ctx, monkeypatch):
    from flye_amd import gpu
    runs = [(n, call_confirm, check_confirm, lambda j: sum(len(a.trg_seq) for a in j["edges"]) + max(a.trg_end for a in j["edges"]) -
             min(a.trg_start for a in j["edges"])) for n in sorted(P.CONFIRM_RUNS)]
    span = lambda e: max(a.trg_end for a in e["alns"]) - min(a.trg_start for a in e["alns"]) if e["alns"] else 0
    runs += [(n, call_classify, check_classify, lambda j: sum(len(a.trg_seq) for e in j["edges"] for a in e["alns"]) + sum(span(e) for e in j["edges"]))
             for n in sorted(P.CLASSIFY_RUNS)]
    for name, call, check, cost in runs:
        g = restated(name)
        whole = call(ctx, g)
        largest = max(cost(j) for j in g["run"]["jobs"])
        for env in ({"FG_PARTITION_BATCH_JOBS": "1"}, {"FG_PARTITION_BATCH_JOBS": "2"}, {"FG_PARTITION_BATCH_COLS": str(largest)},
                    {"FG_PARTITION_TILE": "64"}, {"FG_PARTITION_TILE": "4096"}, {"FG_PARTITION_TILE": "64", "FG_PARTITION_BATCH_JOBS": "1"}):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            cut = call(ctx, g)
            check(cut, g["res"])
            assert cut.same_as(whole), (name, env)
            for k in env:
                monkeypatch.delenv(k)
        monkeypatch.setenv("FG_PARTITION_BATCH_COLS", str(largest - 1))
        with pytest.raises(gpu.FlyeGpuError) as e:
            call(ctx, g)
        assert e.value.code == -8 and "FG_PARTITION_BATCH_COLS" in str(e.value)
        monkeypatch.delenv("FG_PARTITION_BATCH_COLS")
        for bad in ("63", "96", "8192", "0"):
            monkeypatch.setenv("FG_PARTITION_TILE", bad)
            with pytest.raises(gpu.FlyeGpuError) as e:
                call(ctx, g)
            assert e.value.code == -3 and "FG_PARTITION_TILE" in str(e.value)
        monkeypatch.delenv("FG_PARTITION_TILE")
        check(call(ctx, g), g["res"])                                       # the context works on afterwards


@pytest.mark.gpu
def test_offsets_need_not_start_at_zero(ctx):
    """some jobs of a run as a window into the arrays of the whole run"""
    g = restated("confirm_d")
    f = P.confirm_arrays(g["run"]["jobs"])
    lo, hi = 1, 4
    assert int(f["job_edge_off"][lo]) > 0 and int(f["total_off"][lo]) > 0 and int(f["col_off"][int(f["job_edge_off"][lo])]) > 0
    windows = {k + "_off": f[k + "_off"][lo:hi + 1] for k in P.LIST_KEYS}
    res = call_confirm(ctx, g, side=f["side"][lo:hi], job_edge_off=f["job_edge_off"][lo:hi + 1], **windows)
    check_confirm(res, g["res"][lo:hi])
    for name, lo, hi in (("classify_d", 1, 3), ("classify_c", 1, 2)):
        g = restated(name)
        f = P.classify_arrays(g["run"]["jobs"])
        e0 = int(f["job_edge_off"][lo])
        assert e0 > 0 and int(f["edge_aln_off"][e0]) > 0 and int(f["edge_pos_off"][e0]) > 0
        res = call_classify(ctx, g, job_edge_off=f["job_edge_off"][lo:hi + 1], job_n_reads=f["job_n_reads"][lo:hi])
        check_classify(res, g["res"][lo:hi])


@pytest.mark.gpu
def test_empty_batches_and_group_member(ctx):
    from flye_amd import gpu
    res = ctx.confirm_positions([], [0], [], [], [], [0], b"", b"", *[x for _ in range(4) for x in ([0], [])])
    assert all(list(getattr(res, k + "_off")) == [0] and len(getattr(res, k + "_pos")) == 0 for k in P.CONFIRM_KEYS + ("cons",))
    res = ctx.classify_reads(3, [0], [], [0], [], [0], [], [], [], [0], b"", b"", want_scores=True)
    assert list(res.read_off) == [0] and len(res.status) == 0 and len(res.aln_score) == 0
    lib = gpu.load_library()
    b, cb = gpu.ConfirmBatch(), gpu.ClassifyBatch()
    assert lib.fg_confirm_positions(ctx.h, 0, *[None] * 16, C.byref(b)) == 0
    assert b.n_jobs == 0 and b.conf_total_off[0] == 0 and b.rej_ins_off[0] == 0 and b.cons_off[0] == 0
    lib.fg_release_confirm(C.byref(b))
    assert not b.owner_ and not b.cons_off
    assert lib.fg_classify_reads(ctx.h, 0, 0, *[None] * 11, 1, C.byref(cb)) == 0
    assert cb.n_jobs == 0 and cb.read_off[0] == 0
    lib.fg_release_classify(C.byref(cb))
    assert not cb.owner_ and not cb.read_off
    # an edge without alignments or positions; reads of a job with no alignment at all; an edge of no columns
    res = ctx.classify_reads(3, [0, 2], [4], [0, 0, 2], [5, 6], [0, 0, 0], [], [], [], [0], b"", b"")
    assert res.reads(0) == [(0, -1, 0, 0)] * 4
    res = ctx.confirm_positions([0], [0, 1], [7], [7], [3], [0, 0], b"", b"", [0, 2], [7, 6], [0, 0], [], [0, 0], [], [0, 0], [])
    assert all(len(getattr(res, k + "_pos")) == 0 for k in P.CONFIRM_KEYS + ("cons",))
    grp = gpu.Group([0, 0])
    try:
        g = restated("classify_c")
        check_classify(call_classify(grp.member(1), g), g["res"])
        g = restated("confirm_c")
        check_confirm(call_confirm(grp.member(1), g), g["res"])
    finally:
        grp.close()


def _raw_caller(lib, ctx, fn, batch_type, release, order, f, head, tail=()):
    def call(out=True, head=head, **kw):
        args = dict(f, **kw)
        b = batch_type()
        b.n_jobs, b.owner_ = 99, 1                                      # an error leaves *out all zero
        rc = fn(ctx.h, *head, *[None if args[k] is None else args[k].ctypes.data for k in order], *tail, C.byref(b) if out else None)
        if rc == 0:
            release(C.byref(b))
        elif out:
            assert bytes(b) == bytes(C.sizeof(b))
        return rc
    return call


def _changed(f, name, at, value):
    bad = f[name].copy()
    bad[at] = value
    return {name: bad}


def _swapped(f, name):
    bad = f[name].copy()
    i = next(i for i in range(1, len(bad) - 1) if bad[i] < bad[i + 1])
    bad[i], bad[i + 1] = f[name][i + 1], f[name][i]
    assert bad[i + 1] < bad[i]
    return {name: bad}


@pytest.mark.gpu
def test_confirm_argument_errors(ctx):
    from flye_amd import gpu
    lib = gpu.load_library()
    g = restated("confirm_c")
    f = P.confirm_arrays(g["run"]["jobs"])
    f["trg_cols"], f["qry_cols"] = np.frombuffer(f["trg_cols"], np.uint8).copy(), np.frombuffer(f["qry_cols"], np.uint8).copy()
    order = ("side", "job_edge_off", "trg_start", "trg_end", "qry_start", "col_off", "trg_cols", "qry_cols") + \
        tuple(k + s for k in P.LIST_KEYS for s in ("_off", "_pos"))
    conf = _raw_caller(lib, ctx, lib.fg_confirm_positions, gpu.ConfirmBatch, lib.fg_release_confirm, order, f, (len(f["side"]),))
    assert conf() == 0
    assert conf(out=False) == -3
    for name in order:
        assert conf(**{name: None}) == (0 if name.endswith("_pos") and not len(f[name]) else -3), name
    for name in ("job_edge_off", "col_off", "total_off", "ins_off"):
        assert conf(**_swapped(f, name)) == -3, name
    for name in ("trg_cols", "qry_cols"):
        for byte in (128, 255):
            assert conf(**_changed(f, name, len(f[name]) // 2, byte)) == -3, (name, byte)
    assert conf(**_changed(f, "side", 1, 2)) == -3
    empty = f["job_edge_off"].copy()
    empty[1] = empty[0]                                                 # a job without edges
    assert conf(job_edge_off=empty) == -3
    assert conf(**_changed(f, "trg_start", 0, -1)) == -3
    # the non-gap target columns of an edge against trg_end - trg_start: off by one either way
    for d in (-1, 1):
        assert conf(**_changed(f, "trg_end", 0, int(f["trg_end"][0]) + d)) == -3, d
    gap = int(np.flatnonzero(f["trg_cols"] == 45)[0])
    assert conf(**_changed(f, "trg_cols", gap, ord("A"))) == -3
    assert conf(**_changed(f, "qry_start", 0, -5)) == 0                 # a negative qry_start is arithmetic only
    with pytest.raises(gpu.FlyeGpuError) as e:
        call_confirm(ctx, g, trg_end=_changed(f, "trg_end", 0, int(f["trg_end"][0]) + 1)["trg_end"])
    assert e.value.code == -3 and "non-gap" in str(e.value)
    check_confirm(call_confirm(ctx, g), g["res"])                       # the context is usable after the errors


@pytest.mark.gpu
def test_classify_argument_errors(ctx):
    from flye_amd import gpu
    lib = gpu.load_library()
    g = restated("classify_d")
    f = P.classify_arrays(g["run"]["jobs"])
    f["trg_cols"], f["qry_cols"] = np.frombuffer(f["trg_cols"], np.uint8).copy(), np.frombuffer(f["qry_cols"], np.uint8).copy()
    order = ("job_edge_off", "job_n_reads", "edge_pos_off", "edge_pos", "edge_aln_off", "read", "trg_start", "trg_end", "col_off",
             "trg_cols", "qry_cols")
    cls = _raw_caller(lib, ctx, lib.fg_classify_reads, gpu.ClassifyBatch, lib.fg_release_classify, order, f, (3, len(f["job_n_reads"])), (1,))
    assert cls() == 0
    assert cls(out=False) == -3
    for name in order:
        assert cls(**{name: None}) == -3, name
    for name in ("job_edge_off", "edge_pos_off", "edge_aln_off", "col_off"):
        assert cls(**_swapped(f, name)) == -3, name
    for name in ("trg_cols", "qry_cols"):
        for byte in (128, 255):
            assert cls(**_changed(f, name, len(f[name]) // 2, byte)) == -3, (name, byte)
    assert cls(head=(-1, len(f["job_n_reads"]))) == -3 and cls(head=(0, len(f["job_n_reads"]))) == 0
    n_reads = int(f["job_n_reads"][0])
    assert cls(**_changed(f, "read", 0, n_reads)) == -3 and cls(**_changed(f, "read", 0, n_reads - 1)) == 0
    empty = f["job_edge_off"].copy()
    empty[1] = empty[0]
    assert cls(job_edge_off=empty) == -3
    assert cls(**_changed(f, "trg_start", 0, -1)) == -3
    for d in (-1, 1):
        assert cls(**_changed(f, "trg_end", 3, int(f["trg_end"][3]) + d)) == -3, d
    with pytest.raises(gpu.FlyeGpuError) as e:
        call_classify(ctx, g, read=_changed(f, "read", 0, n_reads)["read"])
    assert e.value.code == -3 and "n_reads" in str(e.value)
    check_classify(call_classify(ctx, g), g["res"])                     # the context is usable after the errors


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(P.SAMS))
def test_sam_files_through_read_partitioner(ctx, name, tmp_path):
    from flye_amd import gpu
    run = P.SAMS[name]()
    args = P.write_files(run, str(tmp_path))
    part = gpu.ReadPartitioner(ctx)
    part.partition_reads(run["edges"], run["it"], run["side"], **args)
    want = sam_texts(name)
    assert open(args["confirmed_pos_path"].format(run["it"], run["side"]), "rb").read() == want["confirmed"].encode("latin-1")
    assert open(args["part_file"].format(run["it"], run["side"]), "rb").read() == want["part"].encode("latin-1")
    # the readers give back what the writers wrote
    confirmed, rejected, pos = part._read_confirmed_positions(args["confirmed_pos_path"].format(run["it"], run["side"]))
    assert pos == {k: sorted(v) for k, v in part.read_positions(args["position_path"]).items()}
    rows = part._read_partitioning_file(args["part_file"].format(run["it"], run["side"]))
    assert sorted(r[5] for r in rows) == sorted(run["headers_to_id"]) and all(r[0] == run["headers_to_id"][r[5]] for r in rows)


@pytest.mark.gpu
def test_confirm_and_classify_take_several_jobs_in_one_call(ctx):
    from flye_amd import gpu
    part = gpu.ReadPartitioner(ctx, buffer_count=3)
    g = restated("confirm_c")
    jobs = [({k: list(v) for k, v in j["pos"].items()}, {"edge%d" % i: a for i, a in enumerate(j["edges"])}, ("in", "out")[j["side"]])
            for j in g["run"]["jobs"]]
    for (confirmed, rejected, cons), r in zip(part.confirm(jobs), g["res"]):
        assert all(confirmed[k] == r["conf_" + k] and rejected[k] == r["rej_" + k] for k in P.LIST_KEYS)
        assert [cons["edge%d" % i] for i in range(len(r["cons"]))] == r["cons"]
    g = restated("classify_c")
    jobs = []
    for j in g["run"]["jobs"]:
        ids = [10 * e + 7 for e in range(len(j["edges"]))]
        jobs.append(({i: [e["alns"]] for i, e in zip(ids, j["edges"])}, {i: e["pos"] for i, e in zip(ids, j["edges"])},
                     {"read_%d" % r: 1000 - r for r in range(j["n_reads"])}))
    for rows, r, (read_aligns, _, headers) in zip(part.classify(jobs), g["res"], jobs):
        ids = list(read_aligns)
        assert rows == [(1000 - k, P.STATUS[r["status"][k]], str(ids[r["top_edge"][k]]) if r["status"][k] == 2 else "NA", r["top_score"][k],
                         r["total_score"][k], "read_%d" % k) for k in range(len(headers))]
