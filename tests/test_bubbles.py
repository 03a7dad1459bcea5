"""fg_make_bubbles / gpu.BubbleMaker: the bubble partition of the reference's polisher (flye/polishing/bubbles.py) on the
device.

Yardsticks: the records of the reference's own Python (tests/golden/bubbles_*.fa.gz and bubbles_cases.json, made by
make_bubbles_golden.py) and the restatement tests/bubbles_restate.py.  Without a GPU the restatement is pinned on every
golden run (every bubble, counter and profile array) and the host-only parts of the ABI are checked; with one, every
golden run, the file form, the sub-batch cuts, fuzz seeds, windows into larger arrays and the argument errors."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import bubbles_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fg_make_bubbles", "fg_release_bubbles")
CASES = json.load(open(os.path.join(R.GOLDEN, "bubbles_cases.json")))
_CACHE = {}


def restated(name, run=None):
    """one run through the restatement, computed once: the run, its parameters, the alignments that take part per contig
    (run (a): the reference's selection) and make_contig's result per contig"""
    if name not in _CACHE:
        run = run or R.RUNS[name]()
        p = R.params_for(run["err_mode"], run["overrides"])
        alns, res = {}, {}
        for contig, _ in run["contigs"]:
            lst = run["alns"][contig.id]
            if run["uniform"]:
                lst = [lst[k] for k in CASES[name]["uniform_kept"][contig.id]]
            alns[contig.id] = lst
            res[contig.id] = R.make_contig(contig, lst, p)
        _CACHE[name] = dict(run=run, p=p, alns=alns, res=res)
    return _CACHE[name]


# ---- 1. the restatement against the reference's records (no GPU) -----------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.RUNS))
def test_restatement_equals_the_reference(name):
    g, meta = restated(name), CASES[name]
    assert R.input_digest(g["run"]) == meta["input_sha256"], "the generator no longer makes the stored input"
    assert meta["overrides"] == g["run"]["overrides"] and meta["err_mode"] == g["run"]["err_mode"]
    text = []
    for contig, _ in g["run"]["contigs"]:
        r, m = g["res"][contig.id], meta["contigs"][contig.id]
        assert r["partition"] == m["partition"], contig.id
        for k in ("n_long_bubbles", "n_empty", "n_long_branch", "mean_cov"):
            assert r[k] == m[k], (contig.id, k)
        assert len(r["bubbles"]) == m["n_bubbles"]
        assert r["profile"]["aln_errors"] == m["aln_errors"], contig.id
        assert R.profile_digests(r["profile"]) == m["profile_sha256"], contig.id
        text.append(R.write_bubbles(contig.id, r["bubbles"]))
    assert "".join(text) == R.read_gz(name + ".fa.gz")


def test_solid_flags_closed_form_against_the_greedy_loop():
    """the first loop of _get_partition as the reference walks it, against the closed form"""
    rng = np.random.default_rng(7)
    for n in list(range(0, 45)) + [200, 777]:
        for solid_len in (1, 3, 6, 10):
            for density in (0.5, 0.9, 0.99, 1.0):
                good = rng.random(n) < density
                want = np.zeros(n, bool)
                pos = 0
                while pos < n - solid_len:
                    if good[pos:pos + solid_len].all():
                        want[pos:pos + solid_len] = True
                        pos += solid_len
                    else:
                        pos += 1
                assert np.array_equal(R.solid_flags(good, solid_len), want), (n, solid_len, density)


def test_crafted_cases_show_what_they_are_for():
    c, d = restated("bubbles_c"), restated("bubbles_d")
    res, alns, p = c["res"], c["alns"], c["p"]
    # lengths around 2 * SOLID: the first partition point becomes possible at 21
    assert [len(res["len_%d" % n]["partition"]) for n in (0, 1, 19, 20, 21, 22, 25)] == [0, 0, 0, 0, 1, 1, 1]
    assert res["len_21"]["partition"] == [12] and len(res["len_21"]["bubbles"]) == 2
    # an insertion before position 0 counts at the last position; trg_start 0 on a linear contig gives an empty first
    # branch to bubble 0; chromosome_end gives the last bubble its branches
    r = res["ins_first"]
    assert r["profile"]["num_inserts"][119] == 2 and alns["ins_first"][4].trg_seq.startswith("--")
    first = r["raw"][0][2]                   # per alignment: the empty branch of the cut at position 0, then the bubble's own
    assert first[0:8:2] == [""] * 4 and all(first[1:8:2]) and first[8] == "GT"
    assert len(r["raw"][-1][2]) == 6 and all(w for w in r["raw"][-1][2])
    # nobody covers 80 .. 110: one consensus is shorter than its span, and the bubble in the hole is empty
    r = res["uncovered"]
    ext = [0] + r["partition"] + [200]
    short = [i for i, b in enumerate(r["raw"]) if len(b[1]) < ext[i + 1] - ext[i]]
    assert short and not r["profile"]["has"][80:110].any() and r["n_empty"] == 1
    # no landmark: forced cuts
    for cid in ("homopolymer", "dinucleotide"):
        assert res[cid]["n_long_bubbles"] > 0 and res[cid]["partition"] == [513]
    # the median of a bubble is empty: dropped, not counted
    r = res["median_empty"]
    dropped = [b for b in r["raw"] if b[2] and sorted(map(len, b[2]))[len(b[2]) // 2] == 0]
    assert dropped and r["n_empty"] == 0 and len(r["bubbles"]) == len(r["raw"]) - len(dropped)
    # the consensus is replaced by the median
    r = res["cons_replaced"]
    raw_cons = {b[0]: b[1] for b in r["raw"]}
    assert any(cons != raw_cons[pos] and len(cons) > 2 * len(raw_cons[pos]) for pos, cons, _ in r["bubbles"])
    # a zero-length branch next to a median > 0 has incons_rate 1: it never stays, so '"A"' is never written
    for g in (c, d):
        for r in g["res"].values():
            kept = {b[0]: b[2] for b in r["bubbles"]}
            assert all(w for ws in kept.values() for w in ws)
    assert any("" in b[2] and b[0] in {k[0] for k in r["bubbles"]} for r in res.values() for b in r["raw"])
    # alignments shorter than min_polish_aln_len give branches but no profile
    r, a = d["res"]["short_alns"], d["alns"]["short_alns"]
    assert r["profile"]["in_profile"] == [1, 1, 0, 0, 0, 0, 0] and all(len(x.qry_seq) == 40 for x in a[2:])
    assert int(r["profile"]["coverage"].max()) == 2 and max(len(b[2]) for b in r["raw"]) > 2
    # err_rate exactly at the limit is in, just above it is out
    assert res["err_limit"]["profile"]["in_profile"] == [1, 1, 0] and alns["err_limit"][2].err_rate > 0.25
    assert res["err_limit"]["profile"]["aln_errors"] == [0.25, 0.25]
    # 1/5 is good under 0.2, 2/5 is not
    prof = res["one_fifth"]["profile"]
    good = R.good_positions(prof, p)
    assert (prof["num_missmatch"][50], prof["coverage"][50]) == (1, 5) and good[50]
    assert prof["num_missmatch"][60] + prof["num_deletions"][60] == 2 and not good[60]
    assert prof["num_deletions"][61:71].sum() == 1 and good[61:71].all()        # shift_gaps may have moved it left of 70
    assert R.max_numerator(0.2, 5) == 1 and R.max_numerator(0.3, 10) == 3 and R.max_numerator(0.2, 4) == 0
    # two alignments disagree on a target byte: the last one in list order names the base
    a = alns["disagree"]
    assert a[0].trg_seq[40] == a[1].trg_seq[40] != a[2].trg_seq[40] == chr(res["disagree"]["profile"]["nucl"][40])
    assert a[1].trg_seq[70] == a[1].qry_seq[70] == "-" and res["disagree"]["profile"]["num_inserts"][69] == 1
    # shift_gaps: runs at both ends, adjacent runs, and a later run that walks over bytes an earlier run moved
    events = {}
    for x in alns["shifts"]:
        ev = []
        q = R.shift_gaps(x.trg_seq, x.qry_seq, ev)
        R.shift_gaps(q, x.trg_seq, ev)
        events[x.qry_id] = ev
    n = len(alns["shifts"][3].qry_seq)
    assert events["ends"][0][:2] == (0, 2) and any(e[1] == n for e in events["ends"])
    assert any(e[2] > 0 for e in events["ends"]) and any(e[2] > 0 for e in events["adjacent"])
    assert any(e[3] and e[2] > 0 for ev in events.values() for e in ev), "no walk reached moved bytes"
    # walks longer than a wave: 80 bases moved at once, and a walk that stops at the first mismatch after 70
    wide = {x.qry_id: x for x in alns["wide"]}
    for qid, m in (("moves_80", 80), ("stops_at_70", 70)):
        ev = []
        R.shift_gaps(wide[qid].trg_seq, wide[qid].qry_seq, ev)
        assert [e[2] for e in ev] == [m], (qid, ev)
    # more than 64 branches in a bubble, and more than the cap
    counts = [len(b[2]) for b in res["wide"]["raw"]]          # bubble 0 also takes the empty branches of the cuts at position 0
    assert counts[0] == 142 and 71 in counts and max(len(b[2]) for b in res["wide"]["bubbles"]) == 50
    # column counts around the wave width; other letters and lower case in the query
    assert {1, 63, 64, 65, 255, 256, 257, 1025} <= {len(x.trg_seq) for x in alns["columns"]}
    odd = alns["letters"][3].qry_seq
    assert set("NRYKMSWBVDHXUnacgtryk") <= set(odd)
    kept = [w for b in res["letters"]["raw"] for w in b[2]]
    assert any(ch.islower() for w in kept for ch in w) and all(ch in "ACGTacgt" for w in kept for ch in w)
    # run (d): long bubbles, a long branch and the cap at small size
    assert d["res"]["forced"]["n_long_bubbles"] == 4 and d["res"]["long_branch"]["n_long_branch"] == 1
    assert any(len(b[2]) > 5 for b in d["res"]["forced"]["raw"]) and all(len(b[2]) <= 5 for b in d["res"]["forced"]["bubbles"])
    assert any(len(b[2]) == 1 and len(b[2][0]) > 90 for b in d["res"]["long_branch"]["bubbles"])
    # run (b): alignments wrap past the end of a circular contig
    b = restated("bubbles_b")
    assert any(x.trg_end < x.trg_start for x in b["alns"]["circular_1"])


def test_uniform_alignments_equal_the_reference(built):
    from flye_amd import gpu
    run = restated("bubbles_a")["run"]
    for contig, _ in run["contigs"]:
        lst = run["alns"][contig.id]
        kept = gpu.BubbleMaker.uniform_alignments(lst, contig.length)
        want = CASES["bubbles_a"]["uniform_kept"][contig.id]
        assert [id(a) for a in kept] == [id(lst[k]) for k in want] and 0 < len(want)
    assert len(CASES["bubbles_a"]["uniform_kept"]["contig_2"]) < len(run["alns"]["contig_2"])
    with pytest.raises(ValueError):
        gpu.BubbleMaker.uniform_alignments([R.perfect("x", "ACGT" * 100, 0, 400, "r")._replace(trg_end=900)], 400)


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
    assert _header_fields(header, "fg_bubble_batch") == [n for n, _ in gpu.BubbleBatch._fields_]
    assert _header_fields(header, "fg_bubble_params") == [n for n, _ in gpu.BubbleParams._fields_]
    assert C.sizeof(gpu.BubbleParams) == 48 and C.sizeof(gpu.BubbleBatch) == 16 + 22 * 8
    p = gpu.BubbleParams.for_mode("nano", max_bubble_length=60)
    assert (p.solid_kmer_length, p.simple_kmer_length, p.max_bubble_length, p.solid_indel) == (10, 4, 60, 0.3)
    assert lib.fg_make_bubbles(None, None, 0, None, None, None, None, None, None, None, None, None, 0, None) == -3
    lib.fg_release_bubbles(None)
    empty = gpu.BubbleBatch()
    lib.fg_release_bubbles(C.byref(empty))


# ---- 2. the device ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(built):
    from flye_amd import gpu
    c = gpu.Context(17, 0)          # no reads, no index: the call needs a device and a stream
    yield c
    c.close()


def flat(g):
    """the arguments of Context.make_bubbles after params, for the contigs of a restated run in order"""
    contigs = [c for c, _ in g["run"]["contigs"]]
    alns = [a for c in contigs for a in g["alns"][c.id]]
    return dict(contig_len=np.array([c.length for c in contigs], np.int32),
                contig_circular=np.array([c.type == "circular" for c in contigs], np.uint8),
                contig_aln_off=np.cumsum([0] + [len(g["alns"][c.id]) for c in contigs]).astype(np.uint64),
                trg_start=np.array([a.trg_start for a in alns], np.int32), trg_end=np.array([a.trg_end for a in alns], np.int32),
                err_rate=np.array([a.err_rate for a in alns], np.float64),
                col_off=np.cumsum([0] + [len(a.trg_seq) for a in alns]).astype(np.uint64),
                trg_cols="".join(a.trg_seq for a in alns).encode("latin-1"),
                qry_cols="".join(a.qry_seq for a in alns).encode("latin-1"))


def params(g):
    from flye_amd import gpu
    return gpu.BubbleParams.for_mode(g["run"]["err_mode"], **g["run"]["overrides"])


def check_against(res, g, contigs=None, profile=True):
    """every bubble, counter, partition point and profile value of every contig against the restatement"""
    contigs = contigs if contigs is not None else [c for c, _ in g["run"]["contigs"]]
    assert len(res.bubble_off) == len(contigs) + 1
    flags = []
    for i, contig in enumerate(contigs):
        r = g["res"][contig.id]
        want = [(pos, cons.encode("latin-1"), [w.encode("latin-1") for w in ws]) for pos, cons, ws in r["bubbles"]]
        assert res.bubbles(i) == want, contig.id
        got = (int(res.n_long_bubbles[i]), int(res.n_empty[i]), int(res.n_long_branch[i]), int(res.mean_cov[i]), int(res.n_partition[i]))
        assert got == (r["n_long_bubbles"], r["n_empty"], r["n_long_branch"], r["mean_cov"], len(r["partition"])), contig.id
        flags += r["profile"]["in_profile"]
        if profile:
            assert list(res.partition[int(res.part_off[i]):int(res.part_off[i + 1])]) == r["partition"], contig.id
            a, b = int(res.prof_off[i]), int(res.prof_off[i + 1])
            assert b - a == contig.length
            for k in ("coverage", "num_inserts", "num_deletions", "num_missmatch", "nucl"):
                assert np.array_equal(getattr(res, k)[a:b], r["profile"][k]), (contig.id, k)
    assert list(res.in_profile) == flags


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(R.RUNS))
def test_golden_runs_on_the_device(ctx, name, tmp_path):
    from flye_amd import gpu
    g = restated(name)
    res = ctx.make_bubbles(params(g), want_profile=True, **flat(g))
    check_against(res, g)
    times = ctx.kernel_times()
    assert {"k_bub_shift", "k_bub_profile", "k_bub_good", "k_bub_solid", "k_bub_landmark", "k_bub_walk", "k_bub_cuts",
            "k_bub_post", "k_bub_fill"} <= set(times)
    again = ctx.make_bubbles(params(g), want_profile=True, **flat(g))
    assert res.same_as(again)
    plain = ctx.make_bubbles(params(g), **flat(g))
    assert plain.partition is None and plain.coverage is None
    check_against(plain, g, profile=False)
    # the mirror: the reference's record of the run, byte for byte, and its two return values
    maker = gpu.BubbleMaker(ctx, **g["run"]["overrides"])
    contigs = [c for c, _ in g["run"]["contigs"]]
    bubbles, coverage_stats, mean_err = maker.make(contigs, g["alns"], g["run"]["err_mode"])
    maker.write_bubbles(str(tmp_path / "bubbles.fa"))
    assert (tmp_path / "bubbles.fa").read_bytes() == R.read_gz(name + ".fa.gz").encode("latin-1")
    assert coverage_stats == {c.id: CASES[name]["contigs"][c.id]["mean_cov"] for c in contigs}
    errors = [e for c in contigs for e in CASES[name]["contigs"][c.id]["aln_errors"]]
    assert maker.aln_errors == errors
    total = 0.0
    for e in errors:
        total += e
    assert mean_err == total / (len(errors) + 1)


@pytest.mark.gpu
def test_results_do_not_depend_on_the_cut(ctx, monkeypatch):
    from flye_amd import gpu
    for name in ("bubbles_c", "bubbles_d"):
        g = restated(name)
        whole = ctx.make_bubbles(params(g), want_profile=True, **flat(g))
        costs = [c.length + sum(len(a.trg_seq) for a in g["alns"][c.id]) for c, _ in g["run"]["contigs"]]
        # every contig a sub-batch of its own (a contig of length 0 fits into any budget, so a switch does that); then
        # the smallest budget that still takes the largest contig
        for env in ({"FG_BUBBLE_BATCH_CONTIGS": "1"}, {"FG_BUBBLE_BATCH_COLS": str(max(costs))}):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            cut = ctx.make_bubbles(params(g), want_profile=True, **flat(g))
            check_against(cut, g)
            assert cut.same_as(whole)
            for k in env:
                monkeypatch.delenv(k)
        monkeypatch.setenv("FG_BUBBLE_BATCH_COLS", str(max(costs) - 1))
        with pytest.raises(gpu.FlyeGpuError) as e:
            ctx.make_bubbles(params(g), **flat(g))
        assert e.value.code == -8 and "FG_BUBBLE_BATCH_COLS" in str(e.value)
        monkeypatch.delenv("FG_BUBBLE_BATCH_COLS")
        check_against(ctx.make_bubbles(params(g), want_profile=True, **flat(g)), g)     # the context works on afterwards


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_fuzz(ctx, seed):
    g = restated("fuzz_%d" % seed, R.fuzz(seed))
    assert R.supported(g["p"])
    check_against(ctx.make_bubbles(params(g), want_profile=True, **flat(g)), g)


@pytest.mark.gpu
def test_offsets_need_not_start_at_zero(ctx):
    """contigs 8 .. 14 of run (c) as a window into the arrays of the whole run"""
    g = restated("bubbles_c")
    f = flat(g)
    contigs = [c for c, _ in g["run"]["contigs"]][8:15]
    f["contig_len"], f["contig_circular"], f["contig_aln_off"] = f["contig_len"][8:15], f["contig_circular"][8:15], f["contig_aln_off"][8:16]
    assert f["contig_aln_off"][0] > 0
    res = ctx.make_bubbles(params(g), want_profile=True, **f)
    check_against(res, g, contigs=contigs)


@pytest.mark.gpu
def test_empty_batch_and_group_member(ctx):
    from flye_amd import gpu
    p = gpu.BubbleParams.for_mode("pacbio")
    res = ctx.make_bubbles(p, [], None, [0], [], [], [], [0], b"", b"", want_profile=True)
    assert len(res.position) == 0 and list(res.bubble_off) == [0] and list(res.cand_off) == [0] and list(res.branch_off) == [0]
    assert list(res.part_off) == [0] and list(res.prof_off) == [0]
    lib = gpu.load_library()
    b = gpu.BubbleBatch()
    assert lib.fg_make_bubbles(ctx.h, C.byref(p), 0, None, None, None, None, None, None, None, None, None, 1, C.byref(b)) == 0
    assert b.n_bubbles == 0 and b.bubble_off[0] == 0 and b.bubble_branch_off[0] == 0
    lib.fg_release_bubbles(C.byref(b))
    grp = gpu.Group([0, 0])
    try:
        g = restated("bubbles_d")
        check_against(grp.member(1).make_bubbles(params(g), want_profile=True, **flat(g)), g)
    finally:
        grp.close()


@pytest.mark.gpu
def test_argument_errors(ctx):
    from flye_amd import gpu
    lib = gpu.load_library()
    g = restated("bubbles_d")
    f = flat(g)
    f["trg_cols"] = np.frombuffer(f["trg_cols"], np.uint8).copy()
    f["qry_cols"] = np.frombuffer(f["qry_cols"], np.uint8).copy()
    order = ("contig_len", "contig_circular", "contig_aln_off", "trg_start", "trg_end", "err_rate", "col_off", "trg_cols", "qry_cols")
    n = len(f["contig_len"])

    def call(p=None, out=True, null_params=False, **kw):
        args = dict(f, **kw)
        p = p or params(g)
        b = gpu.BubbleBatch()
        ptr = [None if args[k] is None else args[k].ctypes.data for k in order]
        rc = lib.fg_make_bubbles(ctx.h, None if null_params else C.byref(p), n, *ptr, 0, C.byref(b) if out else None)
        if rc == 0:
            lib.fg_release_bubbles(C.byref(b))
        return rc

    def with_param(**kw):
        p = params(g)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    assert call() == 0
    assert call(null_params=True) == -3 and call(out=False) == -3
    for name in order:
        if name != "contig_circular":                                # NULL there means: no contig is circular
            assert call(**{name: None}) == -3, name
    for name in ("contig_aln_off", "col_off"):
        bad = f[name].copy()
        bad[1], bad[2] = f[name][2], f[name][1]
        assert bad[2] < bad[1]
        assert call(**{name: bad}) == -3, name
    for name in ("trg_cols", "qry_cols"):
        for byte in (128, 255):
            bad = f[name].copy()
            bad[len(bad) // 2] = byte
            assert call(**{name: bad}) == -3, (name, byte)
    bad = f["contig_len"].copy()
    bad[1] = -1
    assert call(contig_len=bad) == -3
    for value in (-1, int(f["contig_len"][0])):
        bad = f["trg_start"].copy()
        bad[0] = value
        assert call(trg_start=bad) == -3, value
    # more non-gap target columns than the contig has positions
    bad = f["contig_len"].copy()
    bad[1] = 299
    assert call(contig_len=bad) == -3
    for k in ("solid_kmer_length", "simple_kmer_length", "max_bubble_length", "max_bubble_branches", "min_polish_aln_len"):
        for v in (0, -5):
            assert call(p=with_param(**{k: v})) == -3, (k, v)
    for k in ("solid_missmatch", "solid_indel", "max_aln_error"):
        for v in (float("nan"), -0.1):
            assert call(p=with_param(**{k: v})) == -3, (k, v)
    for v in (float("nan"), -0.5):
        bad = f["err_rate"].copy()
        bad[3] = v
        assert call(err_rate=bad) == -3, v
    # slices of _is_simple_kmer that would leave the profile
    for solid, simple in ((10, 3), (10, 8), (2, 6), (6, 6)):
        assert call(p=with_param(solid_kmer_length=solid, simple_kmer_length=simple)) == -7, (solid, simple)
    assert call(p=with_param(solid_kmer_length=10, simple_kmer_length=6)) == 0
    check_against(ctx.make_bubbles(params(g), want_profile=True, **flat(g)), g)      # the context is usable after the errors


@pytest.mark.gpu
def test_polish_is_make_then_polish(ctx):
    """BubbleMaker.polish on run (a) against the polishing restatement applied to the reference's bubbles"""
    import polish_restate as PR
    from flye_amd import gpu
    g = restated("bubbles_a")
    path = os.path.join(PR.GOLDEN, "bin_cfg", "pacbio_substitutions.mat")
    s = PR.load_matrix(path)
    ref_bubbles = PR.parse_bubbles(R.read_gz("bubbles_a.fa.gz"))          # the reader upper-cases, as the polisher's does
    want = [PR.polish_bubble(b.cand, b.branches, s) for b in ref_bubbles]
    maker = gpu.BubbleMaker(ctx)
    bubbles, res = maker.polish([c for c, _ in g["run"]["contigs"]], g["alns"], "pacbio", gpu.SubstitutionMatrix(path))
    assert len(bubbles) == len(want) == len(res.candidates)
    for i, (cand, steps, status) in enumerate(want):
        assert res.candidates[i].decode("latin-1") == cand and int(res.status[i]) == status and int(res.n_steps[i]) == len(steps), i
