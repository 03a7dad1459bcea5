"""fg_divergence_profile_cigars / fg_classify_reads_cigars and the gpu.py methods on them: CIGAR runs expanded on the device
straight into the divergence and classify kernels' buffers.

The yardstick everywhere is exact equality with the two-step path (fg_expand_cigars with columns, then
fg_divergence_profile / fg_classify_reads), which tests/test_expand_cigars.py, test_divergence.py and test_partition.py pin
to the reference's golden records.  The two-step result of a set of records is computed once, without any switch, and left
unchanged; the fused calls are compared against it under every switch.  There is no tolerance.

The number of distinct query bytes (nB) that fg_divergence_profile_cigars finds from the records is pinned from outside by
the budget edges: a contig's cost is contig_len * nB + columns, the call succeeds with FG_DIVERGENCE_BATCH_COLS at exactly
the largest cost and returns FG_ERR_NOMEM one below, with the cost in the text."""
import collections
import ctypes as C
import os
import re

import numpy as np
import pytest

import bubbles_restate as R
import cigar_restate as G
import divergence_restate as DR
import partition_restate as P
import test_fused_columns as F          # its record helpers and crafted records; its tests are not collected from here

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fg_divergence_profile_cigars", "fg_classify_reads_cigars")
REC_KEYS = F.REC_KEYS
THRESHOLDS = (0.1, 0.2, 0.3)
BUFFER_COUNT = 3
SWITCHES = ("FG_DIVERGENCE_BATCH_COLS", "FG_DIVERGENCE_BATCH_CONTIGS", "FG_PARTITION_BATCH_COLS", "FG_PARTITION_BATCH_JOBS",
            "FG_PARTITION_TILE", "FG_CIGAR_TILE")
ONE_EACH = {"FG_DIVERGENCE_BATCH_CONTIGS": "1", "FG_PARTITION_BATCH_JOBS": "1", "FG_CIGAR_TILE": "64", "FG_PARTITION_TILE": "64"}
CL_KEYS = ("job_edge_off", "job_n_reads", "edge_pos_off", "edge_pos", "contig_off", "contig_seq", "contig_aln_off", "read") + REC_KEYS[3:]


# ---- the present set, restated ---------------------------------------------------------------------------------------
def present_of_records(recs):
    """the query bytes the columns of these records would show, from the records alone: the SEQ bytes that M and I runs
    consume, upper-cased, and '-' where a D run has a length"""
    out = set()
    for r in recs:
        q = 0
        for op, n in r["runs"]:
            ch = chr(op)
            if ch == "S":
                q += n
            elif ch in "MI":
                out |= set(r["seq"][q:q + n].upper())
                q += n
            elif ch == "D" and n:
                out.add(ord("-"))
    return out


def present_of_columns(recs, contigs):
    return set(b"".join(G.parse_cigar(r["runs"], r["seq"], contigs[r["contig"].decode()].encode(), r["pos"])["qry"] for r in recs))


# ---- records -> arguments --------------------------------------------------------------------------------------------
def no_switch():
    assert not [k for k in SWITCHES if k in os.environ], "the two-step yardstick is computed without any switch"


def classify_arrays(contigs, recs, job_sizes, seed=9):
    """the contigs are the edges (in the order of the dict), cut into jobs of job_sizes edges; a read is a qry_id, numbered
    per job; every edge gets a list of positions with duplicates, -1 and values behind its end"""
    A = F.arrays(contigs, recs)
    names = list(contigs)
    assert sum(job_sizes) == len(names)
    rng = np.random.default_rng(seed)
    job_edge_off = np.cumsum([0] + list(job_sizes)).astype(np.uint64)
    read, n_reads = [], []
    for j in range(len(job_sizes)):
        number = {}
        for k in names[int(job_edge_off[j]):int(job_edge_off[j + 1])]:
            read += [number.setdefault(r["qry_id"], len(number)) for r in recs if r["contig"].decode() == k]
        n_reads.append(len(number) + 1)                                  # one read without any alignment
    pos = []
    for k in names:
        p = [int(x) for x in rng.integers(-1, len(contigs[k]) + 2, max(3, len(contigs[k]) // 3))]
        pos.append(p + p[:2] + [-1])
    A.update(job_edge_off=job_edge_off, job_n_reads=np.array(n_reads, np.uint32),
             edge_pos_off=np.cumsum([0] + [len(p) for p in pos]).astype(np.uint64), edge_pos=np.array([x for p in pos for x in p], np.int32),
             read=np.array(read, np.uint32))
    return A


def div_two_step(ctx, A, thresholds=THRESHOLDS):
    no_switch()
    ex = ctx.expand_cigars(**F.expand_args(A))
    return ex, ctx.divergence_profile(*thresholds, np.diff(A["contig_off"]).astype(np.int32), A["contig_aln_off"], ex.trg_start, ex.col_off,
                                      ex.trg_cols, ex.qry_cols, True)


def div_fused(ctx, A, thresholds=THRESHOLDS, want_profile=True):
    return ctx.divergence_profile_cigars(*thresholds, want_profile=want_profile, **F.fused_args(A))


def cl_columns(ctx, A, ex, want_scores=True):
    return ctx.classify_reads(BUFFER_COUNT, A["job_edge_off"], A["job_n_reads"], A["edge_pos_off"], A["edge_pos"], A["contig_aln_off"], A["read"],
                              ex.trg_start, ex.trg_end, ex.col_off, ex.trg_cols, ex.qry_cols, want_scores)


def cl_two_step(ctx, A):
    no_switch()
    ex = ctx.expand_cigars(**F.expand_args(A))
    return ex, cl_columns(ctx, A, ex)


def cl_fused(ctx, A, want_scores=True):
    return ctx.classify_reads_cigars(BUFFER_COUNT, A["job_edge_off"], A["job_n_reads"], A["edge_pos_off"], A["edge_pos"], A["contig_off"],
                                     A["contig_seq"], A["contig_aln_off"], A["read"], *[A[k] for k in REC_KEYS[3:]], want_scores=want_scores)


def same(got, want):
    for k, v in want.__dict__.items():
        g = got.__dict__[k]
        assert (v is None and g is None) or (g.dtype == v.dtype and g.tobytes() == v.tobytes()), k
    assert got.same_as(want)


def div_need(A, ex, n_bytes):
    """the cost of the contig that needs most: contig_len * nB + columns"""
    off = A["contig_aln_off"]
    return max(int(n) * n_bytes + int(ex.col_off[int(off[i + 1])] - ex.col_off[int(off[i])]) for i, n in enumerate(np.diff(A["contig_off"])))


def cl_need(A, ex):
    """the cost of the job that needs most: per edge the span of its alignments, plus the job's columns"""
    need = 0
    for j in range(len(A["job_n_reads"])):
        e0, e1 = int(A["job_edge_off"][j]), int(A["job_edge_off"][j + 1])
        cells = 0
        for e in range(e0, e1):
            a0, a1 = int(A["contig_aln_off"][e]), int(A["contig_aln_off"][e + 1])
            if a1 > a0:
                cells += int(ex.trg_end[a0:a1].max()) - int(ex.trg_start[a0:a1].min())
        need = max(need, cells + int(ex.col_off[int(A["contig_aln_off"][e1])] - ex.col_off[int(A["contig_aln_off"][e0])]))
    return need


def budget_edges(ctx, monkeypatch, switch, need, fused, two_step, want, names):
    """at exactly the largest need the fused call equals the yardstick; one below both paths refuse with the same text"""
    from flye_amd import gpu
    monkeypatch.setenv(switch, str(need))
    same(fused(), want)
    monkeypatch.setenv(switch, str(need - 1))
    texts = []
    for call in (fused, two_step):
        with pytest.raises(gpu.FlyeGpuError) as e:
            call()
        assert e.value.code == -8
        texts.append(str(e.value))
    monkeypatch.delenv(switch)
    assert names[0] + ":" in texts[0] and texts[0].replace(names[0], names[1]) == texts[1]
    assert " %d " % need in texts[0] and switch + " is %d" % (need - 1) in texts[0]


def both_equal(ctx, monkeypatch, contigs, recs, job_sizes, env=ONE_EACH, budgets=True):
    """both fused calls against their yardsticks: without a switch, under env, and at the budget edges"""
    A = classify_arrays(contigs, recs, job_sizes)
    ex, div = div_two_step(ctx, A)
    cl = cl_columns(ctx, A, ex)
    n_bytes = max(1, len(present_of_records(recs)))
    assert present_of_records(recs) == set(ex.qry_cols.tolist()) == present_of_columns(recs, contigs)
    same(div_fused(ctx, A), div)
    same(cl_fused(ctx, A), cl)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    same(div_fused(ctx, A), div)
    same(cl_fused(ctx, A), cl)
    for k in env:
        monkeypatch.delenv(k)
    if budgets:
        lens = np.diff(A["contig_off"]).astype(np.int32)
        budget_edges(ctx, monkeypatch, "FG_DIVERGENCE_BATCH_COLS", div_need(A, ex, n_bytes), lambda: div_fused(ctx, A),
                     lambda: ctx.divergence_profile(*THRESHOLDS, lens, A["contig_aln_off"], ex.trg_start, ex.col_off, ex.trg_cols,
                                                    ex.qry_cols, True), div, ("fg_divergence_profile_cigars", "fg_divergence_profile"))
        budget_edges(ctx, monkeypatch, "FG_PARTITION_BATCH_COLS", cl_need(A, ex), lambda: cl_fused(ctx, A), lambda: cl_columns(ctx, A, ex), cl,
                     ("fg_classify_reads_cigars", "fg_classify_reads"))
    return A, ex, div, cl


# ---- the golden SAM runs as records ----------------------------------------------------------------------------------
def divergence_sam(name):
    run = DR.SAMS[name]()
    recs = [r for _, rs, _ in G.records(dict(sam=run["sam"], contigs=run["contigs"], max_coverage=1000, use_secondary=False)) for r in rs]
    return dict(run["contigs"]), recs, [1] * len(run["contigs"])


def partition_sam(name):
    """the read alignments of a partition_reads run: an edge's consensus is its contig, the run is one job"""
    run = P.SAMS[name]()
    contigs, recs = {}, []
    for e in run["edges"]:
        cid, seq = run["files"]["cons_%d.fasta" % e].split("\n")[:2]
        contigs[cid[1:]] = seq
        recs += G.records(dict(sam=run["files"]["read_aln_%d.sam" % e].encode(), contigs={cid[1:]: seq}, max_coverage=1000,
                               use_secondary=False))[0][1]
    return contigs, recs, [len(run["edges"])]


GOLDEN_SAMS = {"divergence_" + k: (lambda k=k: divergence_sam(k)) for k in DR.SAMS}
GOLDEN_SAMS.update({"partition_" + k: (lambda k=k: partition_sam(k)) for k in P.SAMS})


# ---- crafted records -------------------------------------------------------------------------------------------------
def own_crafted(case):
    """-> (contigs, records, job sizes): tens of columns on contigs of tens of bases"""
    rng = np.random.default_rng(177)
    ctg = {k: F.contig_of(rng, n) for k, n in (("a", 60), ("b", 48), ("c", 70))}
    rec = lambda *a, **kw: F.rec(ctg, *a, **kw)
    along = lambda k, pos, n: ctg[k][pos - 1:pos - 1 + n]
    if case == "byte_only_in_soft_clip":
        recs = [rec("a", 3, "4S20M3S", "NNRN" + along("a", 3, 20) + "YYK"), rec("a", 10, "30M", along("a", 10, 30)), rec("c", 1, "2S16M", "nn" + along("c", 1, 16))]
        assert not {ord(ch) for ch in "NRYK-"} & present_of_records(recs)
        return ctg, recs, [3]
    if case == "byte_behind_the_consumed_seq":
        recs = [rec("a", 3, "20M", along("a", 3, 20) + "NNRR"), rec("a", 1, "10M2I10M", along("a", 1, 10) + "AC" + along("a", 11, 10) + "y"),
                rec("c", 5, "16M", along("c", 5, 16) + "W" * 9)]
        assert not {ord(ch) for ch in "NRYW-"} & present_of_records(recs)
        return ctg, recs, [1, 2]
    if case == "with_D":
        recs = [rec("a", 3, "10M2D10M", along("a", 3, 10) + along("a", 15, 10)), rec("c", 1, "30M", along("c", 1, 30))]
        assert ord("-") in present_of_records(recs)
        return ctg, recs, [2, 1]
    if case == "zero_length_D_only":
        recs = [rec("a", 3, "10M0D10M", along("a", 3, 20)), rec("c", 1, "0D30M0D", along("c", 1, 30)), rec("c", 4, "8M2I8M", along("c", 4, 8) + "GG" + along("c", 12, 8))]
        assert ord("-") not in present_of_records(recs)
        return ctg, recs, [3]
    if case == "one_two_three_alignments_of_a_read":
        recs = [rec("a", 1, "30M", qid="r1"), rec("a", 5, "25M", qid="r2"), rec("a", 9, "10M1I20M", qid="r2"), rec("a", 2, "40M", qid="r3"),
                rec("a", 20, "12M2D20M", qid="r3"), rec("a", 11, "30M", qid="r3"), rec("c", 1, "50M", qid="r3"), rec("c", 7, "30M", qid="r1"),
                rec("c", 9, "20M1I30M", qid="r1")]
        return ctg, recs, [3]
    if case == "edge_without_alignments_in_its_own_job":
        recs = [rec("a", 1, "30M"), rec("a", 5, "10M2I20M"), rec("c", 2, "40M"), rec("c", 1, "64M")]
        return ctg, recs, [1, 1, 1]
    raise KeyError(case)


OWN_CRAFTED = ["byte_only_in_soft_clip", "byte_behind_the_consumed_seq", "with_D", "zero_length_D_only", "one_two_three_alignments_of_a_read",
               "edge_without_alignments_in_its_own_job"]
# of tests/test_fused_columns.py: word and tile ends of a sub-batch, an empty contig between two others, lower case and
# IUPAC, clips at both ends and an S run inside, a first I and a last D, zero-length runs
THEIR_CRAFTED = ["last_1_mod_8", "last_0_mod_8", "tile_boundary", "empty_contig_between", "lower_case_and_iupac", "clips", "first_I_last_D",
                 "zero_length_runs"]


def inner_soft_clip():
    rng = np.random.default_rng(178)
    ctg = {"a": F.contig_of(rng, 60), "c": F.contig_of(rng, 70)}
    recs = [F.rec(ctg, "a", 2, "2H10M5S12M3S", ctg["a"][1:11] + "NNNNN" + ctg["a"][11:23] + "RRR"), F.rec(ctg, "a", 1, "3S20M1I20M4S5H"),
            F.rec(ctg, "c", 4, "6M0S6M2S7M", ctg["c"][3:15] + "YY" + ctg["c"][15:22])]
    assert not {ord(ch) for ch in "NRY"} & present_of_records(recs)
    return ctg, recs, [1, 1]


# ---- 1. without a GPU ------------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_bound(built):
    from flye_amd import gpu
    lib = gpu.load_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flye_gpu.h")).read(), flags=re.S)
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b" + sym + r"\s*\(", header), sym + " is not declared in include/flye_gpu.h"
        assert hasattr(lib, sym) and sym in gpu.ABI_SYMBOLS
        assert getattr(lib, sym).argtypes is not None
    assert callable(gpu.Context.divergence_profile_cigars) and callable(gpu.Context.classify_reads_cigars)
    for cls, names in ((gpu.DivergenceFinder, ("profile_sam", "find_divergence_sam")), (gpu.ReadPartitioner, ("classify_sam", "partition_reads_sam"))):
        for n in names:
            assert callable(getattr(cls, n))
    # a NULL context is refused before anything is read
    assert lib.fg_divergence_profile_cigars(None, 0.1, 0.1, 0.1, 0, *[None] * 9, 0, None) == -3
    assert lib.fg_classify_reads_cigars(None, 3, 0, *[None] * 14, 0, None) == -3


@pytest.mark.parametrize("name", sorted(GOLDEN_SAMS))
def test_present_rule_on_the_golden_sams(name):
    contigs, recs, _ = GOLDEN_SAMS[name]()
    assert len(recs) > 20 and present_of_records(recs) == present_of_columns(recs, contigs)


@pytest.mark.parametrize("case", OWN_CRAFTED + THEIR_CRAFTED + ["inner_soft_clip", "fuzz_1", "fuzz_2", "fuzz_3"])
def test_present_rule_on_the_crafted_records(case):
    if case in OWN_CRAFTED:
        contigs, recs, _ = own_crafted(case)
    elif case == "inner_soft_clip":
        contigs, recs, _ = inner_soft_clip()
    elif case.startswith("fuzz"):
        contigs, recs = F.fuzz_records(int(case[-1]))
    else:
        contigs, recs = F.crafted(case)[:2]
    assert present_of_records(recs) == present_of_columns(recs, contigs)
    # every alignment on its own too: '-' only where its own D runs have a length
    for r in recs:
        assert present_of_records([r]) == present_of_columns([r], contigs)


# ---- 2. the device ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(built):
    from flye_amd import gpu
    c = gpu.Context(17, 0)          # no reads, no index: the calls need a device and a stream
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GOLDEN_SAMS))
def test_golden_sam_runs(ctx, monkeypatch, name):
    contigs, recs, job_sizes = GOLDEN_SAMS[name]()
    A, ex, div, cl = both_equal(ctx, monkeypatch, contigs, recs, job_sizes)
    assert int(div.total_off[-1]) > 0 and int(cl.aln_score.sum()) > 0
    div_fused(ctx, A)
    assert {"k_seq_present", "k_cig_advance", "k_cig_scan", "k_cig_place", "k_cig_expand", "k_bub_shift", "k_dv_count"} <= set(ctx.kernel_times())
    cl_fused(ctx, A)
    assert {"k_cig_expand", "k_pt_tiles", "k_cl_score", "k_cl_vote"} <= set(ctx.kernel_times())
    # without the profile and the scores the lists and the votes are the same
    d, c = div_fused(ctx, A, want_profile=False), cl_fused(ctx, A, want_scores=False)
    assert d.prof_off is None and c.aln_score is None
    assert all(np.array_equal(getattr(d, k + "_pos"), getattr(div, k + "_pos")) for k in DR.LIST_KEYS) and np.array_equal(c.status, cl.status)


@pytest.mark.gpu
@pytest.mark.parametrize("case", OWN_CRAFTED + THEIR_CRAFTED + ["inner_soft_clip"])
def test_crafted_records(ctx, monkeypatch, case):
    env = dict(ONE_EACH)
    if case in OWN_CRAFTED:
        contigs, recs, job_sizes = own_crafted(case)
    elif case == "inner_soft_clip":
        contigs, recs, job_sizes = inner_soft_clip()
    else:
        contigs, recs, _, theirs = F.crafted(case)
        job_sizes = [1] * len(contigs)
        if "FG_CIGAR_TILE" not in theirs:
            del env["FG_CIGAR_TILE"]                                    # the word ends of a sub-batch at the default tile
    A, ex, div, cl = both_equal(ctx, monkeypatch, contigs, recs, job_sizes, env)
    if case == "one_two_three_alignments_of_a_read":
        per = collections.Counter(zip(A["read"].tolist(), np.repeat(np.arange(3), np.diff(A["contig_aln_off"]).astype(int)).tolist()))
        assert {1, 2, 3} <= set(per.values())
        three = [a for a in range(len(recs)) if per[(int(A["read"][a]), 0 if a < 6 else 2)] == 3]
        assert len(three) == 3 and not cl.aln_counted[three].any() and cl.aln_counted.sum() == len(per) - 1
    if case == "edge_without_alignments_in_its_own_job":
        assert list(np.diff(A["contig_aln_off"])) == [2, 0, 2] and cl.status[int(cl.read_off[1]):int(cl.read_off[2])].tolist() == [0]
    if case == "tile_boundary":
        assert int(ex.col_off[2]) == 128
    if case in ("last_1_mod_8", "last_0_mod_8"):
        assert int(ex.col_off[3] - ex.col_off[2]) % 8 == (1 if case == "last_1_mod_8" else 0) and int(A["contig_aln_off"][1]) == 3
    assert -1 in A["edge_pos"] and len(set(A["edge_pos"].tolist())) < len(A["edge_pos"])


@pytest.mark.gpu
def test_offsets_need_not_start_at_zero(ctx):
    """the contigs (edges, jobs) from the second on, with their alignments, as windows into the arrays of a larger set"""
    contigs, recs, _, _ = F.crafted("clips")
    rng = np.random.default_rng(5)
    first = {"x": F.contig_of(rng, 33)}
    big = classify_arrays(dict(first, **contigs), [F.rec(first, "x", 2, "20M"), F.rec(first, "x", 1, "3S10M1I9M")] + recs, [1, 2, 1])
    A = classify_arrays(contigs, recs, [2, 1])
    _, div = div_two_step(ctx, A)
    win = dict(big, contig_off=big["contig_off"][1:], contig_aln_off=big["contig_aln_off"][1:])
    assert win["contig_off"][0] > 0 and win["contig_aln_off"][0] == 2 and big["run_off"][2] > 0 and big["read_off"][2] > 0
    same(div_fused(ctx, win), div)
    # classify: the jobs from the second on; the edge arrays keep their absolute numbering
    ex = ctx.expand_cigars(**F.expand_args(big))
    want = cl_columns(ctx, dict(big, job_edge_off=big["job_edge_off"][1:], job_n_reads=big["job_n_reads"][1:]), ex)
    lib_args = dict(big, job_edge_off=big["job_edge_off"][1:], job_n_reads=big["job_n_reads"][1:])
    assert lib_args["job_edge_off"][0] == 1 and len(want.aln_score) == len(recs)
    same(cl_fused(ctx, lib_args), want)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuzz(ctx, monkeypatch, seed):
    contigs, recs = F.fuzz_records(seed)
    assert 20 <= len(recs) <= 80 and any(n == 0 for r in recs for _, n in r["runs"])
    env = {"FG_CIGAR_TILE": "64", "FG_PARTITION_TILE": "64", "FG_DIVERGENCE_BATCH_CONTIGS": "2", "FG_PARTITION_BATCH_JOBS": "1"}
    both_equal(ctx, monkeypatch, contigs, recs, [2, 1, 2], env)


@pytest.mark.gpu
def test_empty_batch_and_group_member(ctx, monkeypatch):
    from flye_amd import gpu
    lib = gpu.load_library()
    div = ctx.divergence_profile_cigars(0.1, 0.1, 0.1, [0], b"", [0], [], [0], b"", [], [0], b"", want_profile=True)
    assert all(list(getattr(div, k + "_off")) == [0] and len(getattr(div, k + "_pos")) == 0 for k in DR.LIST_KEYS)
    assert list(div.prof_off) == [0] and len(div.cov) == 0
    cl = ctx.classify_reads_cigars(3, [0], [], [0], [], [0], b"", [0], [], [], [0], b"", [], [0], b"", want_scores=True)
    assert list(cl.read_off) == [0] and len(cl.status) == 0 and len(cl.aln_score) == 0
    db, cb = gpu.DivergenceBatch(), gpu.ClassifyBatch()
    assert lib.fg_divergence_profile_cigars(ctx.h, 0.1, 0.1, 0.1, 0, *[None] * 9, 1, C.byref(db)) == 0
    assert db.n_contigs == 0 and db.total_off[0] == 0 and db.prof_off[0] == 0
    lib.fg_release_divergence(C.byref(db))
    assert lib.fg_classify_reads_cigars(ctx.h, 3, 0, *[None] * 14, 1, C.byref(cb)) == 0
    assert cb.n_jobs == 0 and cb.n_alignments == 0 and cb.read_off[0] == 0
    lib.fg_release_classify(C.byref(cb))
    # contigs without a single alignment: positions and no column, the table of the single '-'
    div = ctx.divergence_profile_cigars(0.0, 0.0, 0.0, [0, 7, 7], b"ACGTACG", [0, 0, 0], [], [0], b"", [], [0], b"", want_profile=True)
    same(div, ctx.divergence_profile(0.0, 0.0, 0.0, [7, 0], [0, 0, 0], [], [0], b"", b"", want_profile=True))
    cl = ctx.classify_reads_cigars(3, [0, 2], [4], [0, 2, 2], [1, 5], [0, 7, 7], b"ACGTACG", [0, 0, 0], [], [], [0], b"", [], [0], b"", want_scores=True)
    same(cl, ctx.classify_reads(3, [0, 2], [4], [0, 2, 2], [1, 5], [0, 0, 0], [], [], [], [0], b"", b"", want_scores=True))
    grp = gpu.Group([0, 0])
    try:
        contigs, recs, job_sizes = own_crafted("one_two_three_alignments_of_a_read")
        A = classify_arrays(contigs, recs, job_sizes)
        ex, div = div_two_step(ctx, A)
        same(div_fused(grp.member(1), A), div)
        same(cl_fused(grp.member(1), A), cl_columns(ctx, A, ex))
    finally:
        grp.close()


@pytest.mark.gpu
def test_argument_errors(ctx):
    """both fused calls return the code fg_expand_cigars returns for the records and the two-step call's code for the rest,
    leave *out zeroed and the context usable"""
    from flye_amd import gpu
    lib = gpu.load_library()
    contigs, recs, _, _ = F.crafted("zero_length_runs")
    A = classify_arrays(contigs, recs, [2, 1])
    ex, div = div_two_step(ctx, A)
    cl = cl_columns(ctx, A, ex)
    f = {k: np.array(v) for k, v in A.items()}
    n_contigs, n, n_jobs = len(f["contig_off"]) - 1, len(f["ctg_pos"]), len(f["job_n_reads"])
    ptr = lambda a, k: None if a[k] is None else a[k].ctypes.data

    def codes(thresholds=THRESHOLDS, buffer_count=BUFFER_COUNT, n_jobs=n_jobs, **kw):
        a = dict(f, **kw)
        eb, db, cb = gpu.ExpandBatch(), gpu.DivergenceBatch(), gpu.ClassifyBatch()
        eb.n_alignments, db.n_contigs, cb.n_jobs = 123, 123, 123            # must be cleared by a call that fails
        rcs = [lib.fg_expand_cigars(ctx.h, n_contigs, ptr(a, "contig_off"), ptr(a, "contig_seq"), n, ptr(a, "aln_contig"),
                                    *[ptr(a, k) for k in REC_KEYS[3:]], 1, C.byref(eb)),
               lib.fg_divergence_profile_cigars(ctx.h, *thresholds, n_contigs, *[ptr(a, k) for k in REC_KEYS], 1, C.byref(db)),
               lib.fg_classify_reads_cigars(ctx.h, buffer_count, n_jobs, *[ptr(a, k) for k in CL_KEYS], 1, C.byref(cb))]
        for rc, b, release in zip(rcs, (eb, db, cb), (lib.fg_release_expand, lib.fg_release_divergence, lib.fg_release_classify)):
            if rc == 0:
                release(C.byref(b))
            else:
                assert bytes(b) == bytes(C.sizeof(type(b))), "the output of a failed call is left empty"
        return rcs

    def changed(name, at, value):
        bad = f[name].copy()
        bad[at] = value
        return {name: bad}

    def swapped(name):
        bad = f[name].copy()
        bad[1], bad[2] = f[name][2], f[name][1]
        assert bad[2] < bad[1]
        return {name: bad}

    assert codes() == [0, 0, 0]
    r0 = int(f["run_off"][1])                                           # 0S10M0D2I0M20M0H on contig a at 5
    for op in b"=NPX":
        assert codes(**changed("run_op", r0, op)) == [-7, -7, -7], chr(op)
    assert codes(**changed("run_op", r0, ord("Z"))) == [-3, -3, -3]
    assert codes(**changed("run_len", r0 + 1, 11)) == [-3, -3, -3]         # one base more than SEQ holds
    assert codes(**changed("run_len", r0 + 5, 60)) == [-3, -3, -3]         # past the contig's end
    zero = f["run_len"].copy()
    zero[r0:int(f["run_off"][2])] = 0
    assert codes(run_len=zero) == [-3, -3, -3]                           # an alignment without columns
    for pos in (0, -3):
        assert codes(**changed("ctg_pos", 2, pos)) == [-3, -3, -3]
    for name in ("contig_seq", "read_seq"):
        assert codes(**changed(name, len(f[name]) // 2, 200)) == [-3, -3, -3], name
    for name in REC_KEYS:
        if name != "contig_aln_off":
            assert codes(**{name: None}) == [-3, -3, -3], name
    assert codes(contig_aln_off=None)[1:] == [-3, -3]
    for name in ("contig_off", "run_off", "read_off"):
        assert codes(**swapped(name)) == [-3, -3, -3], name
    down = f["contig_aln_off"].copy()
    down[1] = down[2] + 1
    assert codes(contig_aln_off=down)[1:] == [-3, -3]
    assert lib.fg_divergence_profile_cigars(ctx.h, *THRESHOLDS, n_contigs, *[ptr(f, k) for k in REC_KEYS], 1, None) == -3
    assert lib.fg_classify_reads_cigars(ctx.h, BUFFER_COUNT, n_jobs, *[ptr(f, k) for k in CL_KEYS], 1, None) == -3
    # the calls' own refusals, with the codes of fg_divergence_profile and fg_classify_reads
    for bad in (float("nan"), -0.5):
        for k in range(3):
            thr = list(THRESHOLDS)
            thr[k] = bad
            assert codes(thresholds=tuple(thr)) == [0, -3, 0], (bad, k)
            with pytest.raises(gpu.FlyeGpuError) as e:
                ctx.divergence_profile(*thr, np.diff(A["contig_off"]).astype(np.int32), A["contig_aln_off"], ex.trg_start, ex.col_off, ex.trg_cols,
                                       ex.qry_cols)
            assert e.value.code == -3
    assert codes(buffer_count=-1) == [0, 0, -3]
    assert codes(job_edge_off=np.array([0, 0, 3], np.uint64)) == [0, 0, -3]      # a job without edges
    assert codes(**changed("read", 1, int(f["job_n_reads"][0]))) == [0, 0, -3]    # read >= n_reads
    assert codes(**changed("read", 1, int(f["job_n_reads"][0]) - 1)) == [0, 0, 0]
    for name in ("job_edge_off", "job_n_reads", "edge_pos_off", "edge_pos", "read"):
        assert codes(**{name: None}) == [0, 0, -3], name
    for name in ("job_edge_off", "edge_pos_off"):
        assert codes(**swapped(name)) == [0, 0, -3], name
    for kw, code in ((dict(buffer_count=-1), -3), (changed("read", 1, 99), -3)):
        with pytest.raises(gpu.FlyeGpuError) as e:
            ctx.classify_reads(kw.get("buffer_count", BUFFER_COUNT), A["job_edge_off"], A["job_n_reads"], A["edge_pos_off"], A["edge_pos"],
                               A["contig_aln_off"], kw.get("read", A["read"]), ex.trg_start, ex.trg_end, ex.col_off, ex.trg_cols, ex.qry_cols)
        assert e.value.code == code
    # the wrappers give the code and the text
    with pytest.raises(gpu.FlyeGpuError) as e:
        div_fused(ctx, dict(A, **changed("run_op", r0, ord("="))))
    assert e.value.code == -7 and "fg_divergence_profile_cigars" in str(e.value) and "CIGAR operation =" in str(e.value)
    with pytest.raises(gpu.FlyeGpuError) as e:
        cl_fused(ctx, dict(A, **changed("read", 1, 99)))
    assert e.value.code == -3 and "fg_classify_reads_cigars" in str(e.value) and "n_reads" in str(e.value)
    same(div_fused(ctx, A), div)                                     # the context is usable after the errors
    same(cl_fused(ctx, A), cl)


@pytest.mark.gpu
def test_insertions_alone_behind_the_last_base(ctx):
    """POS = contig_len + 1 with I runs only passes the expansion with trg_start == contig_len: fg_divergence_profile refuses
    it, fg_classify_reads scores it 0; the fused calls do the same"""
    from flye_amd import gpu
    contigs, recs, _, _ = F.crafted("clips")
    recs = recs + [F.rec(contigs, "c", len(contigs["c"]) + 1, "3I", "ACG", qid="behind")]
    A = classify_arrays(contigs, recs, [3])
    ex = ctx.expand_cigars(**F.expand_args(A))
    assert int(ex.trg_start[-1]) == len(contigs["c"]) == int(ex.trg_end[-1])
    texts = []
    for call in (lambda: div_fused(ctx, A), lambda: ctx.divergence_profile(*THRESHOLDS, np.diff(A["contig_off"]).astype(np.int32), A["contig_aln_off"],
                                                                           ex.trg_start, ex.col_off, ex.trg_cols, ex.qry_cols)):
        with pytest.raises(gpu.FlyeGpuError) as e:
            call()
        assert e.value.code == -3
        texts.append(str(e.value))
    assert texts[0].replace("fg_divergence_profile_cigars", "fg_divergence_profile") == texts[1] and "trg_start outside the contig" in texts[0]
    want = cl_columns(ctx, A, ex)
    same(cl_fused(ctx, A), want)
    assert want.aln_score[-1] == 0


# ---- 3. the SAM files through the mirrors ------------------------------------------------------------------------------
Info = collections.namedtuple("Info", ["length"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(DR.SAMS))
def test_find_divergence_sam_writes_the_golden_files(ctx, name, tmp_path):
    from flye_amd import gpu
    run = DR.SAMS[name]()
    sam, fasta = str(tmp_path / "aln.sam"), str(tmp_path / "template.fasta")
    with open(sam, "wb") as f:
        f.write(run["sam"])
    with open(fasta, "w") as f:
        f.write(DR.fasta_of(run["contigs"]))
    info = {cid: Info(len(seq)) for cid, seq in run["contigs"].items()}
    kinds = ("frequency", "positions", "summary")
    paths = {k: str(tmp_path / (k + ".txt")) for k in kinds}
    one, two = gpu.DivergenceFinder(ctx, 1000), gpu.DivergenceFinder(ctx, 1000)
    mean = two.find_divergence_sam(sam, fasta, info, paths["frequency"], paths["positions"], paths["summary"], *run["thresholds"])
    for kind in kinds:
        assert open(paths[kind], "rb").read() == R.read_gz("divergence_%s.%s.gz" % (name, kind)).encode("latin-1"), kind
    other = {k: str(tmp_path / (k + ".cols")) for k in kinds}
    assert mean == one.find_divergence(sam, fasta, info, other["frequency"], other["positions"], other["summary"], *run["thresholds"])
    same(two.result, one.result)
    assert one.aln_errors == two.aln_errors
    with pytest.raises(ValueError):
        two.find_divergence_sam(str(tmp_path / "missing.sam"), fasta, info, other["frequency"], other["positions"], other["summary"], *run["thresholds"])
    empty = str(tmp_path / "empty.sam")
    with open(empty, "wb") as f:
        f.write(b"@HD\tVN:1.6\n")
    none = {k: str(tmp_path / (k + ".none")) for k in kinds}
    assert two.find_divergence_sam(empty, fasta, info, none["frequency"], none["positions"], none["summary"], *run["thresholds"]) == 0.0
    assert not any(os.path.exists(p) for p in none.values())


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(P.SAMS))
def test_partition_reads_sam_writes_the_golden_files(ctx, name, tmp_path):
    from flye_amd import gpu
    run = P.SAMS[name]()
    args = P.write_files(run, str(tmp_path))
    part = gpu.ReadPartitioner(ctx)
    part.partition_reads_sam(run["edges"], run["it"], run["side"], **args)
    for kind, path in (("confirmed", args["confirmed_pos_path"]), ("part", args["part_file"])):
        assert open(path.format(run["it"], run["side"]), "rb").read() == R.read_gz("partition_%s.%s.gz" % (name, kind)).encode("latin-1"), kind
