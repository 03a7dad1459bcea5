"""fg_contig_consensus_cigars / fg_make_bubbles_cigars and the gpu.py methods on them: CIGAR runs expanded on the device
straight into the consensus and bubble kernels' buffers.

The yardstick everywhere is exact equality with the two-step path (fg_expand_cigars with columns, then fg_contig_consensus
/ fg_make_bubbles), which tests/test_expand_cigars.py, test_contig_consensus.py and test_bubbles.py pin to the
reference's golden records.  The two-step result of a set of records is computed once, without any switch, and left
unchanged; the fused calls are compared against it under every switch.  There is no tolerance."""
import ctypes as C
import inspect
import json
import os
import re
import zlib

import numpy as np
import pytest

import bubbles_restate as R
import cigar_restate as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fg_contig_consensus_cigars", "fg_make_bubbles_cigars")
CASES = json.load(open(os.path.join(R.GOLDEN, "cigar_cases.json")))
REC_KEYS = ("contig_off", "contig_seq", "contig_aln_off", "ctg_pos", "run_off", "run_op", "run_len", "read_off", "read_seq")
SMALL = dict(solid_kmer_length=4, simple_kmer_length=2, max_bubble_length=20, min_polish_aln_len=5)     # contigs of tens of bases
SWITCHES = ("FG_CONSENSUS_BATCH_CONTIGS", "FG_BUBBLE_BATCH_CONTIGS", "FG_CONSENSUS_BATCH_COLS", "FG_BUBBLE_BATCH_COLS", "FG_CIGAR_TILE")


# ---- records -> arguments --------------------------------------------------------------------------------------------
def rec(contigs, contig, pos, cigar, seq=None, qid=None):
    """a record in the form cigar_restate.records gives; without seq the SEQ is the bytes the runs consume along the
    contig, some of them changed or lower-cased (seeded by the record itself)"""
    runs = G.tokens_of(cigar.encode())
    if seq is None:
        rng = np.random.default_rng(zlib.crc32(("%s %d %s" % (contig, pos, cigar)).encode()))
        seq = G.noisy_read(rng, contigs[contig], pos - 1, [(chr(op), n) for op, n in runs])
    return dict(qry_id=qid or "q_%s_%d_%s" % (contig, pos, cigar), contig=contig.encode(), flags=0, pos=pos, runs=runs, seq=seq.encode())


def arrays(contigs, recs):
    """the records grouped by contig (contigs in the order of the dict, records in the order given) as the arguments of the
    fused calls, with what the two-step calls need besides: aln_contig and qry_id numbered per contig"""
    names = list(contigs)
    lists = [[r for r in recs if r["contig"].decode() == k] for k in names]
    flat = [r for lst in lists for r in lst]
    qry_id = []
    for lst in lists:
        number = {}
        qry_id += [number.setdefault(r["qry_id"], len(number)) for r in lst]
    return dict(contig_off=np.cumsum([0] + [len(contigs[k]) for k in names]).astype(np.uint64),
                contig_seq=np.frombuffer("".join(contigs[k] for k in names).encode("latin-1"), np.uint8),
                contig_aln_off=np.cumsum([0] + [len(lst) for lst in lists]).astype(np.uint64),
                ctg_pos=np.array([r["pos"] for r in flat], np.int32),
                run_off=np.cumsum([0] + [len(r["runs"]) for r in flat]).astype(np.uint64),
                run_op=np.array([op for r in flat for op, _ in r["runs"]], np.uint8),
                run_len=np.array([n for r in flat for _, n in r["runs"]], np.uint32),
                read_off=np.cumsum([0] + [len(r["seq"]) for r in flat]).astype(np.uint64),
                read_seq=np.frombuffer(b"".join(r["seq"] for r in flat), np.uint8),
                aln_contig=np.repeat(np.arange(len(names), dtype=np.uint32), [len(lst) for lst in lists]),
                qry_id=np.array(qry_id, np.int32), secondary=np.array([bool(r["flags"] & 0x100) for r in flat], np.uint8))


def expand_args(A):
    return {k: A[k] for k in ("contig_off", "contig_seq", "aln_contig", "ctg_pos", "run_off", "run_op", "run_len", "read_off", "read_seq")}


def fused_args(A):
    return {k: A[k] for k in REC_KEYS}


def no_switch():
    assert not [k for k in SWITCHES if k in os.environ], "the two-step yardstick is computed without any switch"


def two_step(ctx, A, params, use="uniform", circular=None):
    """the yardstick: expand with columns, (the coverage cap,) the consensus and the bubbles, profiles included"""
    no_switch()
    ex = ctx.expand_cigars(**expand_args(A))
    lens = np.diff(A["contig_off"]).astype(np.int32)
    if isinstance(use, str):
        use = ctx.uniform_alignments(lens, A["contig_aln_off"], ex.trg_start, ex.trg_end, ex.err_rate, A["secondary"]).keep
    cons = ctx.contig_consensus(lens, A["contig_aln_off"], ex.trg_start, A["qry_id"], ex.col_off, ex.trg_cols, ex.qry_cols, use, True)
    bub = ctx.make_bubbles(params, lens, circular, A["contig_aln_off"], ex.trg_start, ex.trg_end, ex.err_rate, ex.col_off,
                           ex.trg_cols, ex.qry_cols, True)
    return dict(ex=ex, use=use, cons=cons, bub=bub, params=params, circular=circular)


def same(got, want):
    for k, v in want.__dict__.items():
        g = got.__dict__[k]
        assert (v is None and g is None) or (g.dtype == v.dtype and g.tobytes() == v.tobytes()), k
    assert got.same_as(want)


def fused_equal(ctx, A, ref):
    """both fused calls against the yardstick, array for array, want_profile = 1"""
    cons = ctx.contig_consensus_cigars(qry_id=A["qry_id"], use=ref["use"], want_profile=True, **fused_args(A))
    same(cons, ref["cons"])
    bub = ctx.make_bubbles_cigars(ref["params"], contig_circular=ref["circular"], err_rate=ref["ex"].err_rate, want_profile=True,
                                  **fused_args(A))
    same(bub, ref["bub"])
    assert ref["cons"].nucl is not None and ref["bub"].coverage is not None and ref["bub"].in_profile is not None
    return cons, bub


def largest_need(A, ref):
    """columns plus positions of the contig that needs most: what FG_*_BATCH_COLS is compared with"""
    col_off, aln_off = ref["ex"].col_off, A["contig_aln_off"]
    return max(int(n) + int(col_off[int(aln_off[i + 1])] - col_off[int(aln_off[i])]) for i, n in enumerate(np.diff(A["contig_off"])))


_CACHE = {}


def golden_run(ctx, name):
    """a run of cigar_cases.json: the records in the order get_chunk parses them, their arguments, the yardstick"""
    if name not in _CACHE:
        from flye_amd import gpu
        run = G.RUNS[name]()
        assert G.input_digest(run) == CASES[name]["input_sha256"], "the generator no longer makes the stored input"
        recs = [r for _, rs, _ in G.records(run) for r in rs]
        contigs = {k: run["contigs"][k] for k in sorted(run["contigs"])}
        A = arrays(contigs, recs)
        _CACHE[name] = dict(run=run, A=A, ref=two_step(ctx, A, gpu.BubbleParams.for_mode("pacbio", min_polish_aln_len=50)))
    return _CACHE[name]


# ---- 1. without a GPU ------------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_bound(built):
    from flye_amd import gpu
    lib = gpu.load_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flye_gpu.h")).read(), flags=re.S)
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b" + sym + r"\s*\(", header), sym + " is not declared in include/flye_gpu.h"
        assert hasattr(lib, sym) and sym in gpu.ABI_SYMBOLS
        assert getattr(lib, sym).argtypes is not None
    assert callable(gpu.Context.contig_consensus_cigars) and callable(gpu.Context.make_bubbles_cigars)
    for cls, names in ((gpu.ContigConsensus, ("consensus_sam",)), (gpu.BubbleMaker, ("make_sam", "polish_sam"))):
        for n in names:
            assert callable(getattr(cls, n))
    # a NULL context is refused before anything is read
    assert lib.fg_contig_consensus_cigars(None, 0, *[None] * 11, 0, None) == -3
    assert lib.fg_make_bubbles_cigars(None, None, 0, *[None] * 11, 0, None) == -3
    assert "fg_cigexpand.h" in open(os.path.join(ROOT, "flye_amd", "csrc", "Makefile")).read()


class RestatedContext:
    """expand_cigars by the restatement: what SamAlignments needs of a Context, without a device"""

    def expand_cigars(self, contig_off, contig_seq, aln_contig, ctg_pos, run_off, run_op, run_len, read_off, read_seq, want_cols=True):
        from flye_amd import gpu
        contig_seq, read_seq = bytes(contig_seq), bytes(read_seq)
        ps = []
        for a in range(len(aln_contig)):
            c = int(aln_contig[a])
            runs = [(int(run_op[r]), int(run_len[r])) for r in range(int(run_off[a]), int(run_off[a + 1]))]
            ps.append(G.parse_cigar(runs, read_seq[int(read_off[a]):int(read_off[a + 1])],
                                    contig_seq[int(contig_off[c]):int(contig_off[c + 1])], int(ctg_pos[a])))
        out = dict(col_off=np.cumsum([0] + [len(p["trg"]) for p in ps]).astype(np.uint64), trg_cols=None, qry_cols=None,
                   matches=np.array([p["matches"] for p in ps], np.int64), err_rate=np.array([p["err_rate"] for p in ps], np.float64))
        if want_cols:
            out["trg_cols"] = np.frombuffer(b"".join(p["trg"] for p in ps), np.uint8)
            out["qry_cols"] = np.frombuffer(b"".join(p["qry"] for p in ps), np.uint8)
        for k in ("trg_start", "trg_end", "qry_start", "qry_end", "qry_len"):
            out[k] = np.array([p[k] for p in ps], np.int32)
        return gpu.ExpandResult(**out)


def golden_row(a):
    import hashlib
    sha = lambda text: hashlib.sha256(text.encode("latin-1")).hexdigest()
    return [a.qry_id, a.trg_id, a.qry_start, a.qry_end, a.qry_sign, a.qry_len, a.trg_start, a.trg_end, a.trg_sign, a.trg_len,
            float(a.err_rate).hex(), int(a.is_secondary), len(a.trg_seq), sha(a.trg_seq), len(a.qry_seq), sha(a.qry_seq)]


@pytest.mark.parametrize("name", sorted(G.RUNS))
def test_sam_alignments_keyword(built, tmp_path, name):
    """the default is today's reader, record for record against the reference's golden records; want_cols=False gives the
    same records in the same order with the runs and SEQ in place of the two strings"""
    from flye_amd import gpu
    assert inspect.signature(gpu.SamAlignments.__init__).parameters["want_cols"].default is True
    run, meta = G.RUNS[name](), CASES[name]
    path = tmp_path / "aln.sam"
    path.write_bytes(run["sam"])
    kw = dict(max_coverage=run["max_coverage"], use_secondary=run["use_secondary"])
    chunks = gpu.SamAlignments(RestatedContext(), str(path), run["contigs"], **kw).chunks()
    assert [c for c, _ in chunks] == [c["contig"] for c in meta["chunks"]]
    for (contig, alns), stored in zip(chunks, meta["chunks"]):
        assert [golden_row(a) for a in alns] == stored["alignments"], contig
    assert chunks == gpu.SamAlignments(RestatedContext(), str(path), run["contigs"], want_cols=True, **kw).chunks()
    sam = gpu.SamAlignments(RestatedContext(), str(path), run["contigs"], want_cols=False, **kw)
    assert sam.result.trg_cols is None and [c for c, _ in sam.chunks()] == [c for c, _ in chunks]
    shared = [f for f in gpu.Alignment._fields if f not in ("trg_seq", "qry_seq")]
    for (contig, alns), (_, recs) in zip(chunks, sam.chunks()):
        assert len(alns) == len(recs)
        for a, r in zip(alns, recs):
            assert [getattr(a, f) for f in shared] == [getattr(r, f) for f in shared]
            p = G.parse_cigar(list(zip(r.ops.tolist(), r.lens.tolist())), r.seq, run["contigs"][contig].encode(), r.ctg_pos)
            assert (p["trg"].decode(), p["qry"].decode()) == (a.trg_seq, a.qry_seq)
    with pytest.raises(ValueError):
        gpu.SamAlignments(RestatedContext(), str(path), run["contigs"], **kw).flatten([])


# ---- 2. the device ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(built):
    from flye_amd import gpu
    c = gpu.Context(17, 0)          # no reads, no index: the calls need a device and a stream
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(G.RUNS))
def test_golden_runs(ctx, name):
    g = golden_run(ctx, name)
    fused_equal(ctx, g["A"], g["ref"])
    assert {"k_cig_advance", "k_cig_scan", "k_cig_place", "k_cig_expand", "k_bub_shift"} <= set(ctx.kernel_times())
    ctx.contig_consensus_cigars(qry_id=g["A"]["qry_id"], use=g["ref"]["use"], **fused_args(g["A"]))
    assert {"k_col_present", "k_cig_expand", "k_cc_profile"} <= set(ctx.kernel_times())
    if name == "sam_a":
        assert int(g["ref"]["bub"].bubble_off[-1]) > 0 and 0 < int(g["ref"]["use"].sum()) < len(g["ref"]["use"])
    # without the coverage cap every alignment takes part
    cons = ctx.contig_consensus_cigars(qry_id=g["A"]["qry_id"], use=None, want_profile=True, **fused_args(g["A"]))
    ex = g["ref"]["ex"]
    same(cons, ctx.contig_consensus(np.diff(g["A"]["contig_off"]), g["A"]["contig_aln_off"], ex.trg_start, g["A"]["qry_id"], ex.col_off,
                                    ex.trg_cols, ex.qry_cols, None, True))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(G.RUNS))
def test_the_cut_is_invisible(ctx, monkeypatch, name):
    from flye_amd import gpu
    g = golden_run(ctx, name)
    A, ref = g["A"], g["ref"]
    need = largest_need(A, ref)
    for env in ({"FG_CONSENSUS_BATCH_CONTIGS": "1", "FG_BUBBLE_BATCH_CONTIGS": "1"}, {"FG_CIGAR_TILE": "64"},
                {"FG_CONSENSUS_BATCH_COLS": str(need + 1), "FG_BUBBLE_BATCH_COLS": str(need + 1)},
                {"FG_CONSENSUS_BATCH_CONTIGS": "1", "FG_BUBBLE_BATCH_CONTIGS": "1", "FG_CIGAR_TILE": "64"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        fused_equal(ctx, A, ref)
        for k in env:
            monkeypatch.delenv(k)
    for switch, call in (("FG_CONSENSUS_BATCH_COLS", lambda: ctx.contig_consensus_cigars(qry_id=A["qry_id"], use=ref["use"], **fused_args(A))),
                         ("FG_BUBBLE_BATCH_COLS", lambda: ctx.make_bubbles_cigars(ref["params"], contig_circular=None,
                                                                                  err_rate=ref["ex"].err_rate, **fused_args(A)))):
        monkeypatch.setenv(switch, str(need - 1))
        with pytest.raises(gpu.FlyeGpuError) as e:
            call()
        assert e.value.code == -8 and switch in str(e.value)
        monkeypatch.delenv(switch)
    fused_equal(ctx, A, ref)                                         # the context works on afterwards


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(G.RUNS))
def test_sam_methods_equal_their_counterparts(ctx, tmp_path, name):
    from flye_amd import gpu
    run = G.RUNS[name]()
    path = tmp_path / "aln.sam"
    path.write_bytes(run["sam"])
    kw = dict(max_coverage=run["max_coverage"], use_secondary=run["use_secondary"])
    by_contig = gpu.SamAlignments(ctx, str(path), run["contigs"], **kw).by_contig()
    sam = gpu.SamAlignments(ctx, str(path), run["contigs"], want_cols=False, **kw)
    assert sam.result.trg_cols is None and list(sam.by_contig()) == list(by_contig)
    contigs = [R.Contig(c, len(run["contigs"][c]), "circular" if k == 1 else "linear") for k, c in enumerate(sorted(run["contigs"]))]
    one, two = gpu.ContigConsensus(ctx), gpu.ContigConsensus(ctx)
    for uniform in (True, False):
        assert one.consensus(contigs, by_contig, uniform=uniform, want_profile=True) == \
            two.consensus_sam(contigs, sam, uniform=uniform, want_profile=True)
        same(two.result, one.result)
        assert one.aln_errors == two.aln_errors
    overrides = dict(min_polish_aln_len=50)
    mk1, mk2 = gpu.BubbleMaker(ctx, **overrides), gpu.BubbleMaker(ctx, **overrides)
    capped = {c.id: gpu.BubbleMaker.uniform_alignments_device(ctx, by_contig.get(c.id, []), c.length) for c in contigs}
    for lists, uniform in ((capped, True), (by_contig, False)):
        assert mk1.make(contigs, lists, "pacbio", want_profile=True) == mk2.make_sam(contigs, sam, "pacbio", want_profile=True, uniform=uniform)
        same(mk2.result, mk1.result)
        assert mk1.aln_errors == mk2.aln_errors
    matrix = gpu.SubstitutionMatrix(os.path.join(R.GOLDEN, "bin_cfg", "pacbio_substitutions.mat"))
    b1, p1 = mk1.polish(contigs, capped, "pacbio", matrix, want_steps=True)
    b2, p2 = mk2.polish_sam(contigs, sam, "pacbio", matrix, want_steps=True)
    assert b1 == b2 and p1.candidates == p2.candidates and p1.steps == p2.steps
    assert np.array_equal(p1.n_steps, p2.n_steps) and np.array_equal(p1.status, p2.status)
    if name == "sam_a":
        assert len(b1) > 0


# ---- crafted records: tens of columns on contigs of tens of bases ------------------------------------------------------
def contig_of(rng, n, alphabet="ACGT"):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), n))


def crafted(case):
    """-> (contigs, records, use or None (all), environment)"""
    rng = np.random.default_rng(77)
    two = {"FG_CONSENSUS_BATCH_CONTIGS": "1", "FG_BUBBLE_BATCH_CONTIGS": "1"}
    ctg = {k: contig_of(rng, n) for k, n in (("a", 60), ("b", 48), ("c", 70))}
    rec = lambda *a, **kw: globals()["rec"](ctg, *a, **kw)              # reads along the contigs as they stand when it is called
    body = [rec("a", 1, "30M"), rec("a", 5, "10M2I20M"), rec("a", 11, "12M3D25M"), rec("c", 2, "40M"), rec("c", 9, "20M1I30M"),
            rec("c", 1, "64M")]
    if case in ("last_1_mod_8", "last_0_mod_8"):
        # the last alignment of the first sub-batch ends 1 / 0 columns behind a whole word; a sub-batch follows
        last = "17M" if case == "last_1_mod_8" else "10M2I4M"
        recs = [rec("a", 1, "31M"), rec("a", 4, "8M1D8M"), rec("a", 20, last)] + [r for r in body if r["contig"] == b"c"]
        assert sum(n for op, n in recs[2]["runs"]) % 8 == (1 if case == "last_1_mod_8" else 0)
        return ctg, recs, None, two
    if case == "tile_boundary":
        # the first sub-batch has exactly two tiles of 64 columns
        recs = [rec("a", 1, "50M"), rec("a", 3, "20M38I20M")] + [r for r in body if r["contig"] == b"c"]
        assert sum(n for r in recs[:2] for op, n in r["runs"]) == 128
        return ctg, recs, None, dict(two, FG_CIGAR_TILE="64")
    if case == "empty_contig_between":
        return ctg, body, None, two
    if case == "unused_contig":
        return ctg, body + [rec("b", 3, "30M"), rec("b", 1, "20M")], [1, 1, 1, 0, 0, 1, 1, 1], two
    if case == "nothing_used":
        return ctg, body, [0] * len(body), {}
    if case == "byte_only_in_unused":
        # 'N' and 'y' stand in no alignment that takes part: the match table must not get a rank for them
        recs = body[:3] + [rec("a", 7, "12M", "ACGTNNyyACGT")] + body[3:]
        return ctg, recs, [1, 1, 1, 0, 1, 1, 1], {}
    if case == "lower_case_and_iupac":
        ctg = dict(ctg, a=contig_of(rng, 60, "ACGTacgtNRYKMryn"), c=contig_of(rng, 70, "ACGTacgtSWBDHVswx"))
        recs = [rec("a", 1, "30M", contig_of(rng, 30, "ACGTacgtNnRYrykmSW")), rec("a", 3, "10M4I20M", contig_of(rng, 34, "acgtBDHVbdhvXx")),
                rec("a", 20, "12M3D25M"), rec("c", 2, "40M", contig_of(rng, 40, "ACGTUuNn")), rec("c", 6, "64M")]
        return ctg, recs, None, two
    if case == "clips":
        recs = [rec("a", 1, "3H4S30M"), rec("a", 5, "10M2I20M5S"), rec("a", 11, "6S12M3D25M7H"), rec("a", 2, "2H3S20M1I20M4S5H"),
                rec("c", 2, "9S40M"), rec("c", 9, "20M1I30M2S3H")]
        return ctg, recs, None, {}
    if case == "first_I_last_D":
        recs = [rec("a", 2, "3I30M"), rec("a", 5, "10M2I20M4D"), rec("a", 11, "2I12M25M3D"), rec("c", 1, "1I40M1D"), rec("c", 9, "20M1I30M")]
        return ctg, recs, None, {}
    if case == "zero_length_runs":
        recs = [rec("a", 1, "0M30M0I"), rec("a", 5, "0S10M0D2I0M20M0H"), rec("a", 11, "12M0I3D0S25M"), rec("c", 2, "0H0S0I0D40M"),
                rec("c", 9, "20M1I30M")]
        return ctg, recs, None, {}
    raise KeyError(case)


CRAFTED = ["last_1_mod_8", "last_0_mod_8", "tile_boundary", "empty_contig_between", "unused_contig", "nothing_used", "byte_only_in_unused",
           "lower_case_and_iupac", "clips", "first_I_last_D", "zero_length_runs"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CRAFTED)
def test_crafted_records(ctx, monkeypatch, case):
    from flye_amd import gpu
    contigs, recs, use, env = crafted(case)
    A = arrays(contigs, recs)
    assert A["contig_aln_off"][-1] == len(recs)
    if use is not None:
        use = np.array(use, np.uint8)
        assert len(use) == len(recs)
    ref = two_step(ctx, A, gpu.BubbleParams.for_mode("pacbio", **SMALL), use=use, circular=np.array([0, 1, 0], np.uint8))
    assert int(ref["bub"].in_profile.sum()) > 0
    if case == "nothing_used":
        assert not ref["cons"].match_total.any() and len(ref["cons"].seq) == 0        # the table of the single '-'
    if case == "unused_contig":
        lo, hi = int(ref["cons"].prof_off[1]), int(ref["cons"].prof_off[2])
        assert not ref["cons"].match_total[lo:hi].any() and ref["cons"].match_total[:lo].any()
    if case == "byte_only_in_unused":
        cols = ref["ex"].qry_cols
        lo, hi = int(ref["ex"].col_off[3]), int(ref["ex"].col_off[4])
        others = np.concatenate([cols[:lo], cols[hi:]])
        assert ord("N") in cols[lo:hi] and ord("Y") in cols[lo:hi] and ord("N") not in others and ord("Y") not in others
    if case == "lower_case_and_iupac":
        assert len(set(ref["ex"].qry_cols.tolist())) > 8 and any(chr(b).islower() for b in A["read_seq"])
    fused_equal(ctx, A, ref)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fused_equal(ctx, A, ref)


@pytest.mark.gpu
def test_offsets_need_not_start_at_zero(ctx):
    """the contigs from the second on, with their alignments, as windows into the arrays of a larger set of records"""
    from flye_amd import gpu
    contigs, recs, _, _ = crafted("clips")
    rng = np.random.default_rng(5)
    first = {"x": contig_of(rng, 33)}
    big = arrays(dict(first, **contigs), [rec(first, "x", 2, "20M"), rec(first, "x", 1, "3S10M1I9M")] + recs)
    A = arrays(contigs, recs)
    ref = two_step(ctx, A, gpu.BubbleParams.for_mode("pacbio", **SMALL), use=np.array([1, 0, 1, 1, 1, 1], np.uint8))
    win = dict(big, contig_off=big["contig_off"][1:], contig_aln_off=big["contig_aln_off"][1:])
    assert win["contig_off"][0] > 0 and win["contig_aln_off"][0] == 2 and big["run_off"][2] > 0 and big["read_off"][2] > 0
    use, err = np.concatenate([[1, 1], ref["use"]]).astype(np.uint8), np.concatenate([[0.5, 0.5], ref["ex"].err_rate])
    same(ctx.contig_consensus_cigars(qry_id=big["qry_id"], use=use, want_profile=True, **fused_args(win)), ref["cons"])
    same(ctx.make_bubbles_cigars(ref["params"], contig_circular=None, err_rate=err, want_profile=True, **fused_args(win)), ref["bub"])


# ---- fuzz ------------------------------------------------------------------------------------------------------------
def fuzz_records(seed):
    """tens of alignments on contigs of a few hundred bases: small random CIGARs with clips and zero-length runs"""
    rng = np.random.default_rng(31000 + seed)
    contigs = {"z_%d" % i: G.rand_contig(rng, int(rng.integers(150, 400)), lower=0.3, n_rate=0.03) for i in range(5)}
    recs = []
    for cid in sorted(contigs):
        L = len(contigs[cid])
        for j in range(0 if cid == "z_2" else int(rng.integers(4, 16))):
            start = int(rng.integers(0, L - 40))
            runs = G.noisy_runs(rng, int(rng.integers(30, min(L - start, 200) + 1)), max_run=12)
            runs = [(op, n if rng.random() > 0.05 else 0) for op, n in runs]
            if not any(n for op, n in runs if op in "MD"):
                runs.append(("M", 5))
            if rng.random() < 0.4:
                runs = [("H", 3), ("S", int(rng.integers(0, 6)))] + runs
            if rng.random() < 0.4:
                runs = runs + [("S", int(rng.integers(0, 6))), ("H", 2)]
            r = rec(contigs, cid, start + 1, G.cigar_of(runs), G.noisy_read(rng, contigs[cid], start, runs) + "ACGT"[:j % 3], "fz_%d" % (j % 9))
            r["flags"] = [0, 16, 256][j % 3]
            recs.append(r)
    return contigs, recs


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuzz(ctx, monkeypatch, seed):
    from flye_amd import gpu
    contigs, recs = fuzz_records(seed)
    assert 20 <= len(recs) <= 80 and any(n == 0 for r in recs for _, n in r["runs"])
    A = arrays(contigs, recs)
    ref = two_step(ctx, A, gpu.BubbleParams.for_mode("pacbio", solid_kmer_length=6, simple_kmer_length=4, max_bubble_length=40,
                                                     min_polish_aln_len=40, max_aln_error=0.5))
    assert int(np.diff(ref["ex"].col_off).max()) <= 400 and int(ref["bub"].in_profile.sum()) > 0
    for k, v in (("FG_CIGAR_TILE", "64"), ("FG_CONSENSUS_BATCH_CONTIGS", "2"), ("FG_BUBBLE_BATCH_CONTIGS", "2")):
        monkeypatch.setenv(k, v)
    fused_equal(ctx, A, ref)
    cons = ctx.contig_consensus_cigars(qry_id=A["qry_id"], use=None, want_profile=True, **fused_args(A))
    for k in ("FG_CIGAR_TILE", "FG_CONSENSUS_BATCH_CONTIGS", "FG_BUBBLE_BATCH_CONTIGS"):
        monkeypatch.delenv(k)
    ex = ref["ex"]
    same(cons, ctx.contig_consensus(np.diff(A["contig_off"]), A["contig_aln_off"], ex.trg_start, A["qry_id"], ex.col_off, ex.trg_cols,
                                    ex.qry_cols, None, True))


# ---- errors and the empty batch --------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_argument_errors(ctx):
    """both fused calls return the code fg_expand_cigars returns, leave *out zeroed and the context usable"""
    from flye_amd import gpu
    lib = gpu.load_library()
    contigs, recs, _, _ = crafted("zero_length_runs")
    A = arrays(contigs, recs)
    params = gpu.BubbleParams.for_mode("pacbio", **SMALL)
    ref = two_step(ctx, A, params, use=None)
    f = {k: np.array(v) for k, v in A.items()}
    f["err_rate"] = ref["ex"].err_rate.copy()
    n_contigs, n = len(f["contig_off"]) - 1, len(f["ctg_pos"])
    ptr = lambda a, k: None if a[k] is None else a[k].ctypes.data

    def codes(**kw):
        a = dict(f, **kw)
        eb, cb, bb = gpu.ExpandBatch(), gpu.ConsensusBatch(), gpu.BubbleBatch()
        eb.n_alignments, cb.n_contigs, bb.n_contigs = 123, 123, 123           # must be cleared by a call that fails
        rcs = [lib.fg_expand_cigars(ctx.h, n_contigs, ptr(a, "contig_off"), ptr(a, "contig_seq"), n, ptr(a, "aln_contig"),
                                    *[ptr(a, k) for k in REC_KEYS[3:]], 1, C.byref(eb)),
               lib.fg_contig_consensus_cigars(ctx.h, n_contigs, *[ptr(a, k) for k in REC_KEYS], ptr(a, "qry_id"), None, 1, C.byref(cb)),
               lib.fg_make_bubbles_cigars(ctx.h, C.byref(params), n_contigs, ptr(a, "contig_off"), ptr(a, "contig_seq"), None,
                                          *[ptr(a, k) for k in REC_KEYS[2:]], ptr(a, "err_rate"), 1, C.byref(bb))]
        for rc, b, release in zip(rcs, (eb, cb, bb), (lib.fg_release_expand, lib.fg_release_consensus, lib.fg_release_bubbles)):
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
    assert codes(contig_aln_off=None)[1:] == [-3, -3] and codes(qry_id=None)[1] == -3 and codes(err_rate=None)[2] == -3
    for name in ("contig_off", "run_off", "read_off"):
        assert codes(**swapped(name)) == [-3, -3, -3], name
    down = f["contig_aln_off"].copy()
    down[1] = down[2] + 1
    assert codes(contig_aln_off=down)[1:] == [-3, -3]
    assert lib.fg_contig_consensus_cigars(ctx.h, n_contigs, *[ptr(f, k) for k in REC_KEYS], ptr(f, "qry_id"), None, 1, None) == -3
    assert lib.fg_make_bubbles_cigars(ctx.h, None, n_contigs, ptr(f, "contig_off"), ptr(f, "contig_seq"), None,
                                      *[ptr(f, k) for k in REC_KEYS[2:]], ptr(f, "err_rate"), 1, C.byref(gpu.BubbleBatch())) == -3
    # the wrapper gives the code and the text
    with pytest.raises(gpu.FlyeGpuError) as e:
        ctx.contig_consensus_cigars(qry_id=A["qry_id"], **dict(fused_args(A), **changed("run_op", r0, ord("="))))
    assert e.value.code == -7 and "CIGAR operation =" in str(e.value)
    fused_equal(ctx, A, ref)                                         # the context is usable after the errors


@pytest.mark.gpu
def test_empty_batch(ctx):
    from flye_amd import gpu
    lib = gpu.load_library()
    cons = ctx.contig_consensus_cigars([0], b"", [0], [], [0], b"", [], [0], b"", [], want_profile=True)
    assert list(cons.seq_off) == [0] and len(cons.seq) == 0 and list(cons.prof_off) == [0] and list(cons.ins_off) == [0]
    params = gpu.BubbleParams.for_mode("pacbio")
    bub = ctx.make_bubbles_cigars(params, [0], b"", [], [0], [], [0], b"", [], [0], b"", [], want_profile=True)
    assert list(bub.bubble_off) == [0] and len(bub.position) == 0 and len(bub.in_profile) == 0 and list(bub.prof_off) == [0]
    cb, bb = gpu.ConsensusBatch(), gpu.BubbleBatch()
    assert lib.fg_contig_consensus_cigars(ctx.h, 0, *[None] * 11, 1, C.byref(cb)) == 0
    assert cb.n_contigs == 0 and cb.seq_off[0] == 0
    lib.fg_release_consensus(C.byref(cb))
    assert lib.fg_make_bubbles_cigars(ctx.h, C.byref(params), 0, *[None] * 11, 1, C.byref(bb)) == 0
    assert bb.n_contigs == 0 and bb.n_bubbles == 0 and bb.bubble_off[0] == 0
    lib.fg_release_bubbles(C.byref(bb))
    # contigs without a single alignment: positions and no column
    cons = ctx.contig_consensus_cigars([0, 7, 7], b"ACGTACG", [0, 0, 0], [], [0], b"", [], [0], b"", [], want_profile=True)
    same(cons, ctx.contig_consensus([7, 0], [0, 0, 0], [], [], [0], b"", b"", None, True))
