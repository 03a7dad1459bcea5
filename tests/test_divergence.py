"""fg_divergence_profile / gpu.DivergenceFinder: Trestle's divergent positions (flye/trestle/divergence.py) on the device.

Yardsticks: the records of the reference's own Python (tests/golden/divergence_*.gz and divergence_cases.json, made by
make_divergence_golden.py) and the restatement tests/divergence_restate.py.  Without a GPU the restatement is pinned on
every golden run and the host-only parts of the ABI are checked; with one, the call on every golden run and on fuzz seeds,
every output array against the restatement, the mirror's three files against the golden text byte for byte, the sub-batch
cuts, windows into larger arrays, the argument errors, and SAM files through DivergenceFinder against the files the
reference's own find_divergence left.  Parity is exact everywhere: there is no tolerance."""
import collections
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import bubbles_restate as R
import divergence_restate as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fg_divergence_profile", "fg_release_divergence")
CASES = json.load(open(os.path.join(R.GOLDEN, "divergence_cases.json")))
KINDS = ("frequency", "positions", "summary")
_CACHE = {}


def restated(name, run=None):
    """one run through the restatement, computed once"""
    if name not in _CACHE:
        run = run or DR.RUNS[name]()
        _CACHE[name] = dict(run=run, res=DR.restate_run(run))
    return _CACHE[name]


# ---- 1. the restatement against the reference's records (no GPU) -----------------------------------------------------
@pytest.mark.parametrize("name", sorted(DR.RUNS))
def test_restatement_equals_the_reference(name):
    g, meta = restated(name), CASES["runs"][name]
    run = g["run"]
    assert DR.input_digest(run) == meta["input_sha256"], "the generator no longer makes the stored input"
    assert list(run["thresholds"]) == meta["thresholds"]
    for contig, _ in run["contigs"]:
        r, m = g["res"][contig.id], meta["contigs"][contig.id]
        assert DR.digests(r) == m["arrays_sha256"], contig.id
        assert [len(r[k]) for k in DR.LIST_KEYS] == m["n_called"], contig.id
        assert DR.text_digests(DR.texts(r, contig.length, run["thresholds"])) == m["texts_sha256"], contig.id
        assert [a.err_rate for a in run["alns"][contig.id]] == m["aln_errors"], contig.id
    last = run["contigs"][-1][0]
    for kind, text in DR.texts(g["res"][last.id], last.length, run["thresholds"]).items():
        assert text == R.read_gz("%s.%s.gz" % (name, kind)), kind


@pytest.mark.parametrize("name", sorted(DR.SAMS))
def test_sam_inputs_are_the_stored_ones(name):
    run, meta = DR.SAMS[name](), CASES["sams"][name]
    assert DR.sam_digest(run) == meta["input_sha256"] and list(run["thresholds"]) == meta["thresholds"]
    with_records = [cid for cid in run["contigs"] if ("\t%s\t" % cid).encode() in run["sam"]]
    assert meta["chunks"] == with_records
    assert len(run["contigs"]) == (1 if name == "sam_one" else 3) and len(with_records) == (1 if name == "sam_one" else 2)


@pytest.mark.parametrize("name", sorted(DR.SAMS))
def test_restated_reader_and_profile_equal_find_divergence(name):
    """the restated reader (tests/cigar_restate.py) on the contigs as read_sequence_dict hands them over, then the restated
    profile of the last chunk: the three files the reference's own find_divergence left"""
    import cigar_restate as G
    run, meta = DR.SAMS[name](), CASES["sams"][name]
    contigs = {cid: seq.encode().translate(R.TO_ACGT).decode() for cid, seq in run["contigs"].items()}
    assert any(seq != run["contigs"][cid] for cid, seq in contigs.items())                       # the files hold N
    chunks = G.chunks(dict(sam=run["sam"], contigs=contigs, max_coverage=meta["max_read_coverage"], use_secondary=False))
    assert [cid for cid, _ in chunks] == meta["chunks"]
    assert [float(a.err_rate).hex() for _, alns in chunks for a in alns] == meta["aln_errors"]
    cid, alns = chunks[-1]
    res = DR.divergence(alns, len(contigs[cid]), run["thresholds"])
    for kind, text in DR.texts(res, len(contigs[cid]), run["thresholds"]).items():
        assert text == R.read_gz("divergence_%s.%s.gz" % (name, kind)), kind


def test_divergence_e_contains_what_it_is_for():
    g = restated("divergence_e")
    run, res = g["run"], g["res"]
    alns = run["alns"]
    seqs = {c.id: s for c, s in run["contigs"]}
    assert all(c.length < 3000 for c, _ in run["contigs"]) and run["thresholds"] == (0.1, 0.2, 0.3)
    row = lambda cid, p: tuple(int(res[cid][k][p]) for k in DR.VALUE_KEYS)
    # alignments of every edge length, in columns
    assert [len(a.trg_seq) for a in alns["edges"]] == list(DR.EDGE_COLUMNS + DR.TILE_COLUMNS)
    t = res["ties"]
    # a substitution tie across two alignments: first arrival 'T', byte order would say 'C'; 1/10 passes 0.1
    assert alns["ties"][0].qry_seq.count("T") and (t["cov"][20], chr(t["sub_base"][20]), t["sub_ct"][20], t["flags"][20] & 1) == (10, "T", 1, 1)
    assert alns["ties"][0].qry_seq[2 + 20] == "T" and alns["ties"][1].qry_seq[2 + 20] == "C"
    # the earlier alignment reaches position 40 at a later column than the later alignment does, and still wins
    a4, a10 = alns["ties"][4], alns["ties"][10]
    assert (a4.trg_start, a4.qry_seq[40], a10.trg_start, a10.qry_seq[0]) == (0, "T", 40, "C")
    assert (chr(t["sub_base"][40]), t["sub_ct"][40], t["cov"][40], t["mat_ct"][40]) == ("T", 1, 11, 9)
    # an insertion tie inside one alignment: "GA" against "AG" give G 2 and A 2, 'G' entered first
    assert (chr(t["ins_base"][60]), t["ins_ct"][60]) == ("G", 2) and t["ins_table"][60, ord("A")] == 2
    # the same before column 0 of alignments that start at 0: it lands on the last position
    assert all(a.trg_start == 0 and a.trg_seq.startswith("--") for a in alns["ties"][:2])
    assert (alns["ties"][0].qry_seq[:2], alns["ties"][1].qry_seq[:2]) == ("GA", "AG")
    assert (chr(t["ins_base"][119]), t["ins_ct"][119], t["ins_table"][119, ord("A")]) == ("G", 2, 2)
    # N and lower case: 'N' (alignment 0) against 'c', two each; 'g' before 'G', one each
    assert (chr(t["sub_base"][80]), t["sub_ct"][80]) == ("N", 2) and (chr(t["sub_base"][100]), t["sub_ct"][100]) == ("g", 1)
    o = res["odd"]
    # a '-' against a '-' counts insertions['-']
    assert alns["odd"][0].trg_seq[11] == "-" == alns["odd"][0].qry_seq[11] and (chr(o["ins_base"][10]), o["ins_ct"][10]) == ("-", 1)
    # a position everybody deletes; a stretch nobody covers
    assert row("odd", 30) == (3, ord("A"), 0, 0, 0, 3, 0, 0, 2)
    assert all(row("odd", p) == (0, ord("-"), 0, 0, 0, 0, 0, 0, 0) for p in range(90, 120))
    # nucl from the last alignment that covers the position, whose target byte differs from the contig's
    assert seqs["odd"][50] != "G" and alns["odd"][2].trg_seq[50] == "G" and chr(o["nucl"][50]) == "G"
    assert o["mat_ct"][50] == 0 and o["sub_ct"][50] == 3 and chr(o["sub_base"][50]) == seqs["odd"][50]
    # a target byte in lower case is no query byte's key: 't' counts as a substitution of 'A'
    assert (chr(o["nucl"][150]), chr(o["sub_base"][150]), o["sub_ct"][150], o["mat_ct"][150]) == ("A", "t", 2, 1)
    c = res["circ"]
    # the circular contig: an insertion behind the last position, one behind position 0 after the wrap, one before the
    # first column of the alignment that starts at 0
    assert all(a.trg_end < a.trg_start for a in alns["circ"][:3])
    assert alns["circ"][3].qry_seq[:2] == "TC"                            # with the three "CT": C 4 and T 4, 'C' entered first
    assert (chr(c["ins_base"][299]), c["ins_ct"][299], c["ins_table"][299, ord("T")]) == ("C", 4, 4)
    assert (chr(c["ins_base"][0]), c["ins_ct"][0]) == ("G", 3)
    # thresholds hit exactly pass; one count below does not
    c30 = res["c30"]
    assert set(c30["cov"]) == {30}
    assert [(int(c30[k][p]), int(c30["flags"][p])) for k, p in (("sub_ct", 10), ("sub_ct", 20), ("del_ct", 30), ("del_ct", 40),
                                                                 ("ins_ct", 50), ("ins_ct", 60))] == [(3, 1), (2, 0), (6, 2), (5, 0), (9, 4), (8, 0)]
    assert (c30["total"], c30["sub"], c30["del"], c30["ins"]) == ([10, 30, 50], [10], [30], [50])
    # 70 alignments over one position: 7/70 passes 0.1; 2/21 does not
    assert row("c70", 45)[:5] == (70, ord("A"), 63, ord("G"), 7) and res["c70"]["sub"] == [45]
    assert row("c21", 45)[:5] == (21, ord("A"), 19, ord("G"), 2) and res["c21"]["total"] == []
    assert 2 / float(21) < 0.1 <= 7 / float(70) and DR.min_count(0.1, 21) == 3 and DR.min_count(0.1, 70) == 7
    assert res["bare"]["total"] == [] and set(res["bare"]["cov"]) == {0}


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
    assert "entered the reference's dict first" in raw and "index -1" in raw          # the tie rule and the index -1 rule
    assert _header_fields(header, "fg_divergence_batch") == [n for n, _ in gpu.DivergenceBatch._fields_]
    assert C.sizeof(gpu.DivergenceBatch) == 8 + 19 * 8
    assert "fg_divergence.hip" in re.search(r"^HIP_SRC := (.*)$", open(os.path.join(ROOT, "flye_amd", "csrc", "Makefile")).read(), re.M).group(1)
    assert lib.fg_divergence_profile(None, 0.1, 0.1, 0.1, 0, None, None, None, None, None, None, 0, None) == -3
    lib.fg_release_divergence(None)
    lib.fg_release_divergence(C.byref(gpu.DivergenceBatch()))
    assert hasattr(gpu.Context, "divergence_profile") and hasattr(gpu.DivergenceFinder, "find_divergence")


# ---- 2. the device ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(built):
    from flye_amd import gpu
    c = gpu.Context(17, 0)          # no reads, no index: the call needs a device and a stream
    yield c
    c.close()


def flat(run):
    """the arrays of the call for the contigs of a run in order"""
    contigs = [c for c, _ in run["contigs"]]
    alns = [a for c in contigs for a in run["alns"][c.id]]
    return dict(contig_len=np.array([c.length for c in contigs], np.int32),
                contig_aln_off=np.cumsum([0] + [len(run["alns"][c.id]) for c in contigs]).astype(np.uint64),
                trg_start=np.array([a.trg_start for a in alns], np.int32),
                col_off=np.cumsum([0] + [len(a.trg_seq) for a in alns]).astype(np.uint64),
                trg_cols="".join(a.trg_seq for a in alns).encode("latin-1"),
                qry_cols="".join(a.qry_seq for a in alns).encode("latin-1"))


def check(res, restated_contigs, contigs, profile=True):
    for k in DR.LIST_KEYS:
        assert len(getattr(res, k + "_off")) == len(contigs) + 1
    for i, contig in enumerate(contigs):
        r = restated_contigs[contig.id]
        assert res.positions(i) == {k: r[k] for k in DR.LIST_KEYS}, contig.id
        if profile:
            a, b = int(res.prof_off[i]), int(res.prof_off[i + 1])
            assert b - a == contig.length
            for k in DR.VALUE_KEYS:
                assert np.array_equal(getattr(res, k)[a:b], r[k]), (contig.id, k)
    if not profile:
        assert res.prof_off is None and all(getattr(res, k) is None for k in DR.VALUE_KEYS)


def call(ctx, g, want_profile=True, **changes):
    f = dict(flat(g["run"]), **changes)
    return ctx.divergence_profile(*g["run"]["thresholds"], want_profile=want_profile, **f)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(DR.RUNS))
def test_golden_runs_on_the_device(ctx, name):
    from flye_amd import gpu
    g = restated(name)
    run = g["run"]
    contigs = [c for c, _ in run["contigs"]]
    res = call(ctx, g)
    check(res, g["res"], contigs)
    assert {"k_bub_shift", "k_dv_tiles", "k_dv_scan", "k_dv_count", "k_dv_finish", "k_dv_compact"} <= set(ctx.kernel_times())
    assert res.same_as(call(ctx, g))
    check(call(ctx, g, want_profile=False), g["res"], contigs, profile=False)
    # the mirror: per contig the three texts, the last contig's against the golden files byte for byte
    finder = gpu.DivergenceFinder(ctx)
    got = finder.profile(run["alns"], contigs, *run["thresholds"])
    assert got.same_as(res)
    assert finder.aln_errors == [e for c in contigs for e in CASES["runs"][name]["contigs"][c.id]["aln_errors"]]
    for i, c in enumerate(contigs):
        pos = got.positions(i)
        texts = dict(frequency=finder.frequency_text(got, i), positions=finder.positions_text(pos, *run["thresholds"]),
                     summary=finder.summary_text(pos, c.length))
        assert DR.text_digests(texts) == CASES["runs"][name]["contigs"][c.id]["texts_sha256"], c.id
    for kind in KINDS:
        assert texts[kind].encode("latin-1") == R.read_gz("%s.%s.gz" % (name, kind)).encode("latin-1"), kind


@pytest.mark.gpu
def test_results_do_not_depend_on_the_cut(ctx, monkeypatch):
    from flye_amd import gpu
    for name in sorted(DR.RUNS):
        g = restated(name)
        contigs = [c for c, _ in g["run"]["contigs"]]
        whole = call(ctx, g)
        width = len(set(flat(g["run"])["qry_cols"]))
        costs = [c.length * width + sum(len(a.trg_seq) for a in g["run"]["alns"][c.id]) for c in contigs]
        for env in ({"FG_DIVERGENCE_BATCH_CONTIGS": "1"}, {"FG_DIVERGENCE_BATCH_CONTIGS": "2"},
                    {"FG_DIVERGENCE_BATCH_COLS": str(max(costs))}):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            cut = call(ctx, g)
            check(cut, g["res"], contigs)
            assert cut.same_as(whole)
            for k in env:
                monkeypatch.delenv(k)
        monkeypatch.setenv("FG_DIVERGENCE_BATCH_COLS", str(max(costs) - 1))
        with pytest.raises(gpu.FlyeGpuError) as e:
            call(ctx, g)
        assert e.value.code == -8 and "FG_DIVERGENCE_BATCH_COLS" in str(e.value)
        monkeypatch.delenv("FG_DIVERGENCE_BATCH_COLS")
        check(call(ctx, g), g["res"], contigs)                           # the context works on afterwards


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuzz(ctx, seed):
    g = restated("fuzz_%d" % seed, DR.fuzz(seed))
    check(call(ctx, g), g["res"], [c for c, _ in g["run"]["contigs"]])


@pytest.mark.gpu
@pytest.mark.parametrize("name,lo,hi", [("divergence_e", 2, 7), ("divergence_f", 1, 3)])
def test_offsets_need_not_start_at_zero(ctx, name, lo, hi):
    """some contigs of a run as a window into the arrays of the whole run"""
    g = restated(name)
    f = flat(g["run"])
    contigs = [c for c, _ in g["run"]["contigs"]][lo:hi]
    assert int(f["contig_aln_off"][lo]) > 0 and int(f["col_off"][int(f["contig_aln_off"][lo])]) > 0
    res = call(ctx, g, contig_len=f["contig_len"][lo:hi], contig_aln_off=f["contig_aln_off"][lo:hi + 1])
    check(res, g["res"], contigs)


@pytest.mark.gpu
def test_empty_batch_and_group_member(ctx):
    from flye_amd import gpu
    res = ctx.divergence_profile(0.1, 0.1, 0.1, [], [0], [], [0], b"", b"", want_profile=True)
    assert all(list(getattr(res, k + "_off")) == [0] and len(getattr(res, k + "_pos")) == 0 for k in DR.LIST_KEYS)
    assert list(res.prof_off) == [0] and len(res.cov) == 0
    lib = gpu.load_library()
    b = gpu.DivergenceBatch()
    assert lib.fg_divergence_profile(ctx.h, 0.1, 0.1, 0.1, 0, None, None, None, None, None, None, 1, C.byref(b)) == 0
    assert b.n_contigs == 0 and b.total_off[0] == 0 and b.ins_off[0] == 0 and b.prof_off[0] == 0
    lib.fg_release_divergence(C.byref(b))
    assert not b.owner_ and not b.total_off
    # a contig without alignments, and one of length 0
    res = ctx.divergence_profile(0.0, 0.0, 0.0, [7, 0], [0, 0, 0], [], [0], b"", b"", want_profile=True)
    assert list(res.total_off) == [0, 0, 0] and bytes(res.nucl) == b"-" * 7 and list(res.cov) == [0] * 7 and list(res.flags) == [0] * 7
    grp = gpu.Group([0, 0])
    try:
        g = restated("divergence_e")
        check(call(grp.member(1), g), g["res"], [c for c, _ in g["run"]["contigs"]])
    finally:
        grp.close()


@pytest.mark.gpu
def test_argument_errors(ctx):
    from flye_amd import gpu
    lib = gpu.load_library()
    g = restated("divergence_e")
    f = flat(g["run"])
    f["trg_cols"] = np.frombuffer(f["trg_cols"], np.uint8).copy()
    f["qry_cols"] = np.frombuffer(f["qry_cols"], np.uint8).copy()
    n = len(f["contig_len"])
    order = ("contig_len", "contig_aln_off", "trg_start", "col_off", "trg_cols", "qry_cols")

    def div(out=True, thresholds=(0.1, 0.2, 0.3), **kw):
        args = dict(f, **kw)
        b = gpu.DivergenceBatch()
        b.n_contigs, b.owner_ = 99, 1                                   # an error leaves *out all zero
        rc = lib.fg_divergence_profile(ctx.h, *thresholds, n, *[None if args[k] is None else args[k].ctypes.data for k in order], 0,
                                       C.byref(b) if out else None)
        if rc == 0:
            lib.fg_release_divergence(C.byref(b))
        elif out:
            assert bytes(b) == bytes(C.sizeof(b))
        return rc

    def changed(name, at, value):
        bad = f[name].copy()
        bad[at] = value
        return {name: bad}

    def swapped(name):
        bad = f[name].copy()
        i = next(i for i in range(1, len(bad) - 1) if bad[i] < bad[i + 1])
        bad[i], bad[i + 1] = f[name][i + 1], f[name][i]
        assert bad[i + 1] < bad[i]
        return {name: bad}

    assert div() == 0
    assert div(out=False) == -3
    for name in order:
        assert div(**{name: None}) == -3, name
    assert div(**swapped("contig_aln_off")) == -3 and div(**swapped("col_off")) == -3
    assert div(**changed("contig_len", 1, -1)) == -3
    for name in ("trg_cols", "qry_cols"):
        for byte in (128, 255):
            assert div(**changed(name, len(f[name]) // 2, byte)) == -3, (name, byte)
    length = int(f["contig_len"][0])
    for value in (-1, length):
        assert div(**changed("trg_start", 0, value)) == -3, value
    assert div(**changed("trg_start", 0, length - 1)) == 0             # the alignment wraps: legal
    # more non-gap target columns than positions
    first = g["run"]["contigs"][0][0]
    longest = max(sum(1 for ch in a.trg_seq if ch != "-") for a in g["run"]["alns"][first.id])
    assert div(**changed("contig_len", 0, longest)) == 0 and div(**changed("contig_len", 0, longest - 1)) == -3
    for bad in (float("nan"), -0.5, -float("inf")):
        for k in range(3):
            thr = [0.1, 0.2, 0.3]
            thr[k] = bad
            assert div(thresholds=tuple(thr)) == -3, (bad, k)
    assert div(thresholds=(0.0, float("inf"), 2.5)) == 0
    with pytest.raises(gpu.FlyeGpuError) as e:
        call(ctx, g, trg_start=changed("trg_start", 0, -1)["trg_start"])
    assert e.value.code == -3 and "trg_start" in str(e.value)
    check(call(ctx, g), g["res"], [c for c, _ in g["run"]["contigs"]])  # the context is usable after the errors


@pytest.mark.gpu
def test_thresholds_beyond_one_and_zero(ctx):
    """ins_ct may exceed cov, so a threshold above 1 can pass; 0 calls every covered position; infinity none"""
    g = restated("divergence_e")
    run = dict(g["run"], thresholds=(0.0, float("inf"), 1.5))
    contigs = [c for c, _ in run["contigs"]]
    want = DR.restate_run(run)
    assert any(want[c.id]["ins"] for c in contigs) and not any(want[c.id]["del"] for c in contigs)
    assert all(want[c.id]["sub"] == [int(p) for p in np.flatnonzero(want[c.id]["cov"])] for c in contigs)
    check(call(ctx, dict(run=run)), want, contigs)


Info = collections.namedtuple("Info", ["length"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(DR.SAMS))
def test_sam_to_divergence_finder(ctx, name, tmp_path):
    from flye_amd import gpu
    run, meta = DR.SAMS[name](), CASES["sams"][name]
    sam, fasta = str(tmp_path / "aln.sam"), str(tmp_path / "template.fasta")
    with open(sam, "wb") as f:
        f.write(run["sam"])
    with open(fasta, "w") as f:
        f.write(DR.fasta_of(run["contigs"]))
    info = {cid: Info(len(seq)) for cid, seq in run["contigs"].items()}
    paths = {k: str(tmp_path / (k + ".txt")) for k in KINDS}
    finder = gpu.DivergenceFinder(ctx, meta["max_read_coverage"])
    mean = finder.find_divergence(sam, fasta, info, paths["frequency"], paths["positions"], paths["summary"], *run["thresholds"])
    for kind in KINDS:
        assert open(paths[kind], "rb").read() == R.read_gz("divergence_%s.%s.gz" % (name, kind)).encode("latin-1"), kind
    errors = [float.fromhex(e) for e in meta["aln_errors"]]
    assert finder.aln_errors == errors and mean == sum(errors) / (len(errors) + 1)
    assert len(finder.result.total_off) == len(meta["chunks"]) + 1                   # one device call for all contigs
    # a missing file: ValueError, and nothing is written; a file without an aligned record writes nothing
    other = {k: str(tmp_path / (k + ".none")) for k in KINDS}
    with pytest.raises(ValueError):
        finder.find_divergence(str(tmp_path / "missing.sam"), fasta, info, other["frequency"], other["positions"], other["summary"],
                               *run["thresholds"])
    empty = str(tmp_path / "empty.sam")
    with open(empty, "wb") as f:
        f.write(b"@HD\tVN:1.6\n")
    assert finder.find_divergence(empty, fasta, info, other["frequency"], other["positions"], other["summary"], *run["thresholds"]) == 0.0
    assert not any(os.path.exists(p) for p in other.values())
