"""fg_uniform_alignments / fg_contig_consensus / gpu.ContigConsensus: the reference's consensus stage
(flye/polishing/consensus.py) and the coverage cap in front of it (alignment.py: get_uniform_alignments) on the device.

Yardsticks: the records of the reference's own Python (tests/golden/contig_consensus_*.fa.gz and
contig_consensus_cases.json, made by make_contig_consensus_golden.py) and the restatement
tests/contig_consensus_restate.py.  Without a GPU the restatement is pinned on every golden run and the host-only parts of
the ABI are checked; with one, both calls on every golden run and on fuzz seeds, every output array against the
restatement, the mirror against the golden FASTA, the sub-batch cuts, windows into larger arrays and the argument errors.
Parity is exact everywhere: there is no tolerance."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

import bubbles_restate as R
import contig_consensus_restate as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fg_uniform_alignments", "fg_release_uniform", "fg_contig_consensus", "fg_release_consensus")
CASES = json.load(open(os.path.join(R.GOLDEN, "contig_consensus_cases.json")))
_CACHE = {}


def restated(name, run=None):
    """one run through the restatement, computed once: with the uniform step (as get_consensus runs) and without it"""
    if name not in _CACHE:
        run = run or CR.RUNS[name]()
        _CACHE[name] = dict(run=run, res=CR.restate_run(run), res_all=CR.restate_run(run, with_uniform=False))
    return _CACHE[name]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- 1. the restatement against the reference's records (no GPU) -----------------------------------------------------
@pytest.mark.parametrize("name", sorted(CR.RUNS))
def test_restatement_equals_the_reference(name):
    g, meta = restated(name), CASES[name]
    assert CR.input_digest(g["run"]) == meta["input_sha256"], "the generator no longer makes the stored input"
    seqs = {}
    for contig, _ in g["run"]["contigs"]:
        r, m = g["res"][contig.id], meta["contigs"][contig.id]
        assert [k for k, f in enumerate(r["uniform"]["keep"]) if f] == m["uniform_kept"], contig.id
        assert r["uniform"]["cov_threshold"] == m["cov_threshold"], contig.id
        assert sha(np.array(r["uniform"]["thresholds"], np.float64)) == m["thresholds_sha256"], contig.id
        assert [a.err_rate for a, f in zip(g["run"]["alns"][contig.id], r["use"]) if f] == m["aln_errors"], contig.id
        seq = r["consensus"]["seq"]
        assert (len(seq), hashlib.sha256(seq).hexdigest()) == (m["seq_len"], m["seq_sha256"]), contig.id
        assert CR.profile_digests(r["consensus"]) == m["profile_sha256"], contig.id
        assert int(r["consensus"]["accepted"].sum()) == m["n_accepted"]
        if seq:
            seqs[contig.id] = seq.decode("latin-1")
    assert CR.write_fasta(seqs) == R.read_gz("contig_consensus_" + name + ".fa.gz")


def test_consensus_e_contains_what_it_is_for():
    g = restated("consensus_e")
    run, res = g["run"], g["res"]
    alns = run["alns"]
    seqs = {c.id: s for c, s in run["contigs"]}
    assert all(c.length < 3000 and len(alns[c.id]) <= 100 for c, _ in run["contigs"])
    v, use = res["votes"]["consensus"], res["votes"]["use"]
    ids = [a.qry_id for a in alns["votes"]]
    # two alignments of one qry_id insert at position 20: "C" and "G" become the read's "CG", beside two other reads' "CG"
    assert ids[:3] == ["dup", "dup", "other"] and use[:8] == [1] * 8
    per_aln = [CR.consensus(alns["votes"], list(range(9)), [int(k == j) for k in range(9)], 300)["ins"][20] for j in range(8)]
    assert per_aln[:6] == [b"C", b"G", b"CG", b"CG", b"G", b"G"]
    assert (v["ins"][20], v["num_ins"][20], v["match_total"][20], v["accepted"][20]) == (b"CG", 5, 8, 1)
    apart = CR.consensus(alns["votes"], list(range(9)), use, 300)           # every alignment a read of its own: "G" wins
    assert apart["ins"][20] == b"G" and apart["num_ins"][20] == 6
    # the top count is tied: byte order decides ("C" 2, "G" 2, "T" 1), and a proper prefix comes first ("A" 2, "AC" 2)
    assert (v["ins"][40], v["accepted"][40], v["num_ins"][40]) == (b"C", 1, 5)
    assert (v["ins"][60], v["accepted"][60], v["num_ins"][60]) == (b"A", 1, 5)
    # num_ins exactly at match_total // 2 is not enough, one above is
    assert (v["num_ins"][80], v["match_total"][80] // 2, v["accepted"][80]) == (4, 4, 0)
    assert (v["num_ins"][100], v["match_total"][100] // 2, v["accepted"][100]) == (5, 4, 1)
    # four deletions against four bases: the deletion wins, the position gives no base
    assert v["max_match"][120] == ord("-") and v["nucl"][120] == ord("A") and v["match_total"][120] == 8
    # a masked-out alignment would change the vote at 140: without it "C" and "G" tie and "C" wins
    assert use[8] == 0 and ids[8] == "inside" and alns["votes"][8].trg_seq[30] == "G" == seqs["votes"][140]
    assert v["max_match"][140] == ord("C")
    assert res_all_of("consensus_e")["votes"]["consensus"]["max_match"][140] == ord("G")
    # an insertion before position 0 lands on the last position
    assert all(a.trg_seq.startswith("--") and a.trg_start == 0 for a in alns["votes"][3:8])
    assert (v["ins"][299], v["accepted"][299]) == (b"GT", 1) and v["seq"].endswith(b"AGT")
    # a position nobody covers
    h = res["hole"]["consensus"]
    assert (h["nucl"][200:250] == ord("-")).all() and (h["match_total"][200:250] == 0).all() and len(h["seq"]) == 350
    assert (h["max_match"][200:250] == ord("-")).all()
    # the circular contig: alignments wrap (and pass the uniform step with a negative window count); insertions behind the
    # last position and behind position 0, and one before the first column of an alignment that starts at 0
    c = res["circ"]["consensus"]
    assert all(a.trg_end < a.trg_start for a in alns["circ"][:3]) and res["circ"]["use"] == [1, 1, 1, 1]
    assert (c["ins"][299], c["num_ins"][299], c["accepted"][299]) == (b"CT", 4, 1)
    assert (c["ins"][0], c["num_ins"][0], c["accepted"][0]) == (b"GC", 3, 1)
    assert alns["circ"][3].trg_seq.startswith("--") and alns["circ"][3].qry_seq.startswith("TC")
    # strings of 1, 63, 64, 65 and 257 bytes: two reads agree, one differs in the last byte
    lg = res["long"]["consensus"]
    assert sorted(len(lg["ins"][p]) for p in CR.LONG) == [1, 63, 64, 65, 257]
    for p, n in CR.LONG.items():
        other = CR.consensus(alns["long"][1:2], [0], None, 300)["ins"][p]
        assert len(lg["ins"][p]) == n and lg["accepted"][p] == 1 and other[:-1] == lg["ins"][p][:-1] and other != lg["ins"][p]
    # 70 reads insert at one position
    d = res["deep"]["consensus"]
    assert (d["num_ins"][100], d["match_total"][100], d["ins"][100], d["accepted"][100]) == (70, 75, b"C", 1)
    # the uniform step: 11 windows with cov_threshold 10; windows of exactly 10 and of 11 entries; an err_rate equal to
    # the threshold stays; secondaries fill windows without raising the median; an alignment inside one window goes
    u, lst = res["uni_odd"]["uniform"], alns["uni_odd"]
    assert len(u["thresholds"]) == 11 and u["cov_threshold"] == 10
    assert u["counts"][2] == 10 and u["thresholds"][2] == 1.0 and u["counts"][5] == 11 and u["thresholds"][5] < 1.0
    by_id = {a.qry_id: (a, k) for a, k in zip(lst, u["keep"])}
    assert by_id["s5_2"][0].err_rate == u["thresholds"][5] and by_id["s5_2"][1] == 1
    assert u["thresholds"][7] == by_id["p5"][0].err_rate and by_id["p6"][0].err_rate > u["thresholds"][7] and by_id["p6"][1] == 1
    assert by_id["bad"][1] == 0 and by_id["one_window"][1] == 0 and by_id["one_window"][0].err_rate == 0.0
    assert sum(1 for a in lst if a.is_secondary) == 10 and max(u["counts"]) == 14
    # 10 windows: the middle coverages 10 and 11 give m2 = 21 and 13, where 10 alone would give 12
    u, lst = res["uni_even"]["uniform"], alns["uni_even"]
    assert len(u["thresholds"]) == 10 and u["cov_threshold"] == 13 == 5 * 21 // 8 and 5 * 20 // 8 == 12
    assert u["counts"][0] == 13 and u["thresholds"][0] == 1.0 and u["counts"][2] == 14
    assert lst[9].qry_id == "p9" and u["thresholds"][2] == lst[9].err_rate and u["keep"][9] == 1
    # trg_end == len on a contig of 1000 bp
    assert all(a.trg_end == 1000 for a in alns["uni_1000"]) and res["uni_1000"]["use"] == [1] * 6
    assert len(res["uni_1000"]["uniform"]["thresholds"]) == 11 and res["uni_1000"]["uniform"]["counts"][10] == 0


def res_all_of(name):
    return restated(name)["res_all"]


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
    assert _header_fields(header, "fg_uniform_result") == [n for n, _ in gpu.UniformResultStruct._fields_]
    assert _header_fields(header, "fg_consensus_batch") == [n for n, _ in gpu.ConsensusBatch._fields_]
    assert C.sizeof(gpu.UniformResultStruct) == 16 + 5 * 8 and C.sizeof(gpu.ConsensusBatch) == 8 + 11 * 8
    assert lib.fg_uniform_alignments(None, 0, None, None, None, None, None, None, 0, None) == -3
    assert lib.fg_contig_consensus(None, 0, None, None, None, None, None, None, None, None, 0, None) == -3
    lib.fg_release_uniform(None)
    lib.fg_release_consensus(None)
    lib.fg_release_uniform(C.byref(gpu.UniformResultStruct()))
    lib.fg_release_consensus(C.byref(gpu.ConsensusBatch()))


# ---- 2. the device ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(built):
    from flye_amd import gpu
    c = gpu.Context(17, 0)          # no reads, no index: the calls need a device and a stream
    yield c
    c.close()


def flat(run):
    """the arrays of both calls for the contigs of a run in order"""
    contigs = [c for c, _ in run["contigs"]]
    alns = [a for c in contigs for a in run["alns"][c.id]]
    return dict(contig_len=np.array([c.length for c in contigs], np.int32),
                contig_aln_off=np.cumsum([0] + [len(run["alns"][c.id]) for c in contigs]).astype(np.uint64),
                trg_start=np.array([a.trg_start for a in alns], np.int32), trg_end=np.array([a.trg_end for a in alns], np.int32),
                err_rate=np.array([a.err_rate for a in alns], np.float64),
                is_secondary=np.array([a.is_secondary for a in alns], np.uint8),
                qry_id=np.array([q for c in contigs for q in CR.number_reads(run["alns"][c.id])], np.int32),
                col_off=np.cumsum([0] + [len(a.trg_seq) for a in alns]).astype(np.uint64),
                trg_cols="".join(a.trg_seq for a in alns).encode("latin-1"),
                qry_cols="".join(a.qry_seq for a in alns).encode("latin-1"))


UNI_KEYS = ("contig_len", "contig_aln_off", "trg_start", "trg_end", "err_rate", "is_secondary")
CONS_KEYS = ("contig_len", "contig_aln_off", "trg_start", "qry_id", "col_off", "trg_cols", "qry_cols")


def uni_args(f):
    return {k: f[k] for k in UNI_KEYS}


def cons_args(f):
    return {k: f[k] for k in CONS_KEYS}


def check_uniform(res, g, contigs=None):
    contigs = contigs if contigs is not None else [c for c, _ in g["run"]["contigs"]]
    keep, thr = [], []
    for i, contig in enumerate(contigs):
        u = g["res"][contig.id]["uniform"]
        keep += u["keep"]
        thr += u["thresholds"]
        assert int(res.cov_threshold[i]) == u["cov_threshold"], contig.id
        assert int(res.wnd_off[i + 1]) - int(res.wnd_off[i]) == contig.length // 100 + 1
    assert list(res.keep) == keep
    assert res.wnd_threshold.tobytes() == np.array(thr, np.float64).tobytes()
    return np.array(keep, np.uint8)


def check_consensus(res, restated_contigs, contigs, profile=True):
    assert len(res.seq_off) == len(contigs) + 1
    for i, contig in enumerate(contigs):
        r = restated_contigs[contig.id]["consensus"]
        assert res.sequence(i) == r["seq"], contig.id
        if profile:
            a, b = int(res.prof_off[i]), int(res.prof_off[i + 1])
            assert b - a == contig.length
            for k in CR.PROFILE_KEYS:
                assert np.array_equal(getattr(res, k)[a:b], r[k]), (contig.id, k)
            assert [res.insertion(p) for p in range(a, b)] == r["ins"], contig.id


def both_calls(ctx, g, contigs=None):
    f = flat(g["run"])
    contigs = [c for c, _ in g["run"]["contigs"]]
    uni = ctx.uniform_alignments(want_thresholds=True, **uni_args(f))
    keep = check_uniform(uni, g)
    res = ctx.contig_consensus(use=uni.keep, want_profile=True, **cons_args(f))
    check_consensus(res, g["res"], contigs)
    return f, uni, res, keep


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CR.RUNS))
def test_golden_runs_on_the_device(ctx, name):
    from flye_amd import gpu
    g = restated(name)
    contigs = [c for c, _ in g["run"]["contigs"]]
    f, uni, res, keep = both_calls(ctx, g)
    times = ctx.kernel_times()
    assert {"k_bub_shift", "k_cc_count", "k_cc_profile", "k_cc_flatten", "k_cc_write"} <= set(times)
    if int(res.num_ins.sum()):
        assert {"k_cc_sort", "k_cc_heads", "k_cc_vote"} <= set(times)
    assert res.same_as(ctx.contig_consensus(use=uni.keep, want_profile=True, **cons_args(f)))
    ctx.uniform_alignments(**uni_args(f))
    times = ctx.kernel_times()
    assert {"k_uni_scan", "k_uni_median", "k_uni_thresh"} <= set(times)
    if len(f["trg_start"]):
        assert "k_uni_keep" in times
    if any(a.trg_end // 100 > a.trg_start // 100 for c in contigs for a in g["run"]["alns"][c.id]):
        assert {"k_uni_emit", "k_uni_sort"} <= set(times)
    assert uni.same_as(ctx.uniform_alignments(want_thresholds=True, **uni_args(f)))
    plain = ctx.contig_consensus(use=keep, **cons_args(f))
    assert plain.nucl is None and plain.ins_off is None
    check_consensus(plain, g["res"], contigs, profile=False)
    # every alignment takes part: use = NULL, and a mask of ones
    for use in (None, np.ones(len(f["trg_start"]), np.uint8)):
        check_consensus(ctx.contig_consensus(use=use, want_profile=True, **cons_args(f)), g["res_all"], contigs)
    # the mirror: the reference's FASTA of the run, byte for byte, and the mean error
    cc = gpu.ContigConsensus(ctx)
    seqs, mean_err = cc.consensus(contigs, g["run"]["alns"])
    assert CR.write_fasta(seqs).encode("latin-1") == R.read_gz("contig_consensus_" + name + ".fa.gz").encode("latin-1")
    errors = [e for c in contigs for e in CASES[name]["contigs"][c.id]["aln_errors"]]
    assert cc.aln_errors == errors
    total = 0.0
    for e in errors:
        total += e
    assert mean_err == total / (len(errors) + 1)
    for c in contigs:
        kept = gpu.BubbleMaker.uniform_alignments_device(ctx, g["run"]["alns"][c.id], c.length)
        assert [id(a) for a in kept] == [id(g["run"]["alns"][c.id][k]) for k in CASES[name]["contigs"][c.id]["uniform_kept"]], c.id


@pytest.mark.gpu
def test_uniform_alignments_device_equals_the_host_classmethod(ctx):
    from flye_amd import gpu
    stored = json.load(open(os.path.join(R.GOLDEN, "bubbles_cases.json")))["bubbles_a"]["uniform_kept"]
    for name in ("bubbles_a", "consensus_e"):
        run = restated(name)["run"]
        for contig, _ in run["contigs"]:
            lst = run["alns"][contig.id]
            dev = gpu.BubbleMaker.uniform_alignments_device(ctx, lst, contig.length)
            host = gpu.BubbleMaker.uniform_alignments(lst, contig.length)
            assert [id(a) for a in dev] == [id(a) for a in host], contig.id
            if name == "bubbles_a":
                assert [id(a) for a in dev] == [id(lst[k]) for k in stored[contig.id]] and 0 < len(dev)


@pytest.mark.gpu
def test_results_do_not_depend_on_the_cut(ctx, monkeypatch):
    from flye_amd import gpu
    for name in ("bubbles_c", "consensus_e"):
        g = restated(name)
        contigs = [c for c, _ in g["run"]["contigs"]]
        f, uni, whole, keep = both_calls(ctx, g)
        costs = [c.length + sum(len(a.trg_seq) for a in g["run"]["alns"][c.id]) for c in contigs]
        for env in ({"FG_CONSENSUS_BATCH_CONTIGS": "1"}, {"FG_CONSENSUS_BATCH_COLS": str(max(costs))}):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            cut = ctx.contig_consensus(use=keep, want_profile=True, **cons_args(f))
            check_consensus(cut, g["res"], contigs)
            assert cut.same_as(whole)
            for k in env:
                monkeypatch.delenv(k)
        monkeypatch.setenv("FG_CONSENSUS_BATCH_COLS", str(max(costs) - 1))
        with pytest.raises(gpu.FlyeGpuError) as e:
            ctx.contig_consensus(use=keep, **cons_args(f))
        assert e.value.code == -8 and "FG_CONSENSUS_BATCH_COLS" in str(e.value)
        monkeypatch.delenv("FG_CONSENSUS_BATCH_COLS")
        pairs = [sum(max(0, a.trg_end // 100 - a.trg_start // 100) for a in g["run"]["alns"][c.id]) for c in contigs]
        monkeypatch.setenv("FG_UNIFORM_BATCH_PAIRS", str(max(pairs)))
        cut = ctx.uniform_alignments(want_thresholds=True, **uni_args(f))
        check_uniform(cut, g)
        assert cut.same_as(uni)
        if max(pairs):
            monkeypatch.setenv("FG_UNIFORM_BATCH_PAIRS", str(max(pairs) - 1))
            with pytest.raises(gpu.FlyeGpuError) as e:
                ctx.uniform_alignments(**uni_args(f))
            assert e.value.code == -8 and "FG_UNIFORM_BATCH_PAIRS" in str(e.value)
        monkeypatch.delenv("FG_UNIFORM_BATCH_PAIRS")
        both_calls(ctx, g)                                            # the context works on afterwards


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_fuzz(ctx, seed):
    g = restated("fuzz_%d" % seed, CR.fuzz(seed))
    assert any(len(set(a.qry_id for a in lst)) < len(lst) for lst in g["run"]["alns"].values())
    f, _, _, _ = both_calls(ctx, g)
    check_consensus(ctx.contig_consensus(want_profile=True, **cons_args(f)), g["res_all"], [c for c, _ in g["run"]["contigs"]])


@pytest.mark.gpu
@pytest.mark.parametrize("name,lo,hi", [("bubbles_c", 8, 15), ("consensus_e", 1, 6)])
def test_offsets_need_not_start_at_zero(ctx, name, lo, hi):
    """some contigs of a run as a window into the arrays of the whole run"""
    g = restated(name)
    f = flat(g["run"])
    contigs = [c for c, _ in g["run"]["contigs"]][lo:hi]
    f["contig_len"], f["contig_aln_off"] = f["contig_len"][lo:hi], f["contig_aln_off"][lo:hi + 1]
    first, last = int(f["contig_aln_off"][0]), int(f["contig_aln_off"][-1])
    assert first > 0
    uni = ctx.uniform_alignments(want_thresholds=True, **uni_args(f))
    assert len(uni.keep) == last - first
    check_uniform(uni, g, contigs)
    use = np.zeros(len(f["trg_start"]), np.uint8)
    use[first:last] = uni.keep
    check_consensus(ctx.contig_consensus(use=use, want_profile=True, **cons_args(f)), g["res"], contigs)


@pytest.mark.gpu
def test_empty_batch_and_group_member(ctx):
    from flye_amd import gpu
    uni = ctx.uniform_alignments([], [0], [], [], [], want_thresholds=True)
    assert len(uni.keep) == 0 and len(uni.cov_threshold) == 0 and list(uni.wnd_off) == [0]
    res = ctx.contig_consensus([], [0], [], [], [0], b"", b"", want_profile=True)
    assert list(res.seq_off) == [0] and list(res.prof_off) == [0] and list(res.ins_off) == [0] and len(res.seq) == 0
    lib = gpu.load_library()
    r, b = gpu.UniformResultStruct(), gpu.ConsensusBatch()
    assert lib.fg_uniform_alignments(ctx.h, 0, None, None, None, None, None, None, 1, C.byref(r)) == 0
    assert r.n_alignments == 0 and r.wnd_off[0] == 0
    lib.fg_release_uniform(C.byref(r))
    assert lib.fg_contig_consensus(ctx.h, 0, None, None, None, None, None, None, None, None, 1, C.byref(b)) == 0
    assert b.seq_off[0] == 0 and b.ins_off[0] == 0
    lib.fg_release_consensus(C.byref(b))
    # a contig without alignments, and one of length 0
    res = ctx.contig_consensus([7, 0], [0, 0, 0], [], [], [0], b"", b"", want_profile=True)
    assert list(res.seq_off) == [0, 0, 0] and bytes(res.nucl) == b"-" * 7 and list(res.match_total) == [0] * 7
    uni = ctx.uniform_alignments([7, 0], [0, 0, 0], [], [], [], want_thresholds=True)
    assert list(uni.cov_threshold) == [10, 10] and list(uni.wnd_threshold) == [1.0, 1.0]
    grp = gpu.Group([0, 0])
    try:
        both_calls(grp.member(1), restated("consensus_e"))
    finally:
        grp.close()


@pytest.mark.gpu
def test_argument_errors(ctx):
    from flye_amd import gpu
    lib = gpu.load_library()
    g = restated("consensus_e")
    f = flat(g["run"])
    f["trg_cols"] = np.frombuffer(f["trg_cols"], np.uint8).copy()
    f["qry_cols"] = np.frombuffer(f["qry_cols"], np.uint8).copy()
    f["use"] = np.array([k for c, _ in g["run"]["contigs"] for k in g["res"][c.id]["use"]], np.uint8)
    n = len(f["contig_len"])
    uni_order = UNI_KEYS
    cons_order = ("contig_len", "contig_aln_off", "trg_start", "qry_id", "use", "col_off", "trg_cols", "qry_cols")

    def uni(out=True, **kw):
        args = dict(f, **kw)
        r = gpu.UniformResultStruct()
        rc = lib.fg_uniform_alignments(ctx.h, n, *[None if args[k] is None else args[k].ctypes.data for k in uni_order], 0,
                                       C.byref(r) if out else None)
        if rc == 0:
            lib.fg_release_uniform(C.byref(r))
        return rc

    def cons(out=True, **kw):
        args = dict(f, **kw)
        b = gpu.ConsensusBatch()
        rc = lib.fg_contig_consensus(ctx.h, n, *[None if args[k] is None else args[k].ctypes.data for k in cons_order], 0,
                                     C.byref(b) if out else None)
        if rc == 0:
            lib.fg_release_consensus(C.byref(b))
        return rc

    def changed(name, at, value):
        bad = f[name].copy()
        bad[at] = value
        return {name: bad}

    def swapped(name):
        bad = f[name].copy()
        bad[1], bad[2] = f[name][2], f[name][1]
        assert bad[2] < bad[1]
        return {name: bad}

    assert uni() == 0 and cons() == 0
    assert uni(out=False) == -3 and cons(out=False) == -3
    for name in uni_order:
        if name != "is_secondary":                                   # NULL there means: no alignment is secondary
            assert uni(**{name: None}) == -3, name
    assert uni(is_secondary=None) == 0
    for name in cons_order:
        if name != "use":                                            # NULL there means: every alignment takes part
            assert cons(**{name: None}) == -3, name
    assert cons(use=None) == 0
    assert uni(**swapped("contig_aln_off")) == -3
    assert cons(**swapped("contig_aln_off")) == -3 and cons(**swapped("col_off")) == -3
    assert uni(**changed("contig_len", 1, -1)) == -3 and cons(**changed("contig_len", 1, -1)) == -3
    # the uniform step: negative ends, an alignment beyond the last window, err_rate NaN or negative
    assert uni(**changed("trg_start", 0, -1)) == -3 and uni(**changed("trg_end", 0, -1)) == -3
    assert f["contig_len"][0] == 300 and uni(**changed("trg_end", 0, 399)) == 0
    assert uni(**changed("trg_end", 0, 400)) == -3 and uni(**changed("trg_start", 0, 400)) == -3
    for v in (float("nan"), -0.5):
        assert uni(**changed("err_rate", 3, v)) == -3, v
    # the consensus: bytes, trg_start outside the contig, more target bases than positions, a contig of length 0
    for name in ("trg_cols", "qry_cols"):
        for byte in (128, 255):
            assert cons(**changed(name, len(f[name]) // 2, byte)) == -3, (name, byte)
    for value in (-1, 300):
        assert cons(**changed("trg_start", 0, value)) == -3, value
    assert cons(**changed("contig_len", 0, 299)) == -3
    assert f["use"][8] == 0 and cons(**changed("trg_start", 8, 300)) == 0          # not looked at: the alignment takes no part
    assert cons(use=None, **changed("trg_start", 8, 300)) == -3
    one = dict(contig_len=np.array([0], np.int32), contig_aln_off=np.array([0, 1], np.uint64), trg_start=np.array([0], np.int32),
               qry_id=np.array([0], np.int32), col_off=np.array([0, 0], np.uint64), trg_cols=b"", qry_cols=b"")
    with pytest.raises(gpu.FlyeGpuError) as e:
        ctx.contig_consensus(**one)
    assert e.value.code == -3 and "length 0" in str(e.value)
    assert ctx.contig_consensus(use=[0], **one).sequence(0) == b""
    both_calls(ctx, g)                                                # the context is usable after the errors
