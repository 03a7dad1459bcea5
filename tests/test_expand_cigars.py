"""fg_expand_cigars / fg_cigar_parse / gpu.SamAlignments: the reference's SAM reader (flye/utils/sam_parser.py:
SynchronizedSamReader.get_chunk and _parse_cigar) with the CIGAR expansion and the match count on the device.

Yardsticks: the records of the reference's own class (tests/golden/cigar_cases.json, made by make_cigar_golden.py) and the
restatement tests/cigar_restate.py.  Without a GPU the restatement is pinned on every golden run and the host-only parts of
the ABI are checked; with one, the call on every golden run and on fuzz seeds, every output array against the restatement,
the mirror against the golden records, tiles, sub-batch cuts, windows into larger arrays, the argument errors and the two
stages behind it end to end.  Parity is exact everywhere: there is no tolerance."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

import bubbles_restate as R
import cigar_restate as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fg_expand_cigars", "fg_release_expand", "fg_cigar_parse")
CASES = json.load(open(os.path.join(R.GOLDEN, "cigar_cases.json")))
OUT_KEYS = ("col_off", "trg_cols", "qry_cols", "trg_start", "trg_end", "qry_start", "qry_end", "qry_len", "matches", "err_rate")
_CACHE = {}


def restated(name, run=None):
    """one run through the restatement, computed once and left unchanged: the chunks, the records in the order get_chunk
    parses them, the arguments of the device call for them and what it must return"""
    if name not in _CACHE:
        run = run or G.RUNS[name]()
        per_chunk = G.records(run)
        recs = [r for _, rs, _ in per_chunk for r in rs]
        _CACHE[name] = dict(run=run, per_chunk=per_chunk, chunks=G.chunks(run), recs=recs, args=G.call_arrays(recs, run["contigs"]),
                            want=G.expand(recs, run["contigs"]))
    return _CACHE[name]


def sha(text):
    return hashlib.sha256(text.encode("latin-1")).hexdigest()


def row(a):
    return [a.qry_id, a.trg_id, a.qry_start, a.qry_end, a.qry_sign, a.qry_len, a.trg_start, a.trg_end, a.trg_sign, a.trg_len,
            float(a.err_rate).hex(), int(a.is_secondary), len(a.trg_seq), sha(a.trg_seq), len(a.qry_seq), sha(a.qry_seq)]


# ---- 1. without a GPU ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(G.RUNS))
def test_restatement_equals_the_reference(name):
    g, meta = restated(name), CASES[name]
    assert G.input_digest(g["run"]) == meta["input_sha256"], "the generator no longer makes the stored input"
    assert [c for c, _ in g["chunks"]] == [c["contig"] for c in meta["chunks"]]
    for (contig, alns), stored in zip(g["chunks"], meta["chunks"]):
        assert [row(a) for a in alns] == stored["alignments"], contig
    # err_rate is what the host makes of the match count, to the bit
    for r, m, e, c0, c1 in zip(g["recs"], g["want"]["matches"], g["want"]["err_rate"], g["want"]["col_off"], g["want"]["col_off"][1:]):
        assert e == 1 - int(m) / int(c1 - c0)


def test_sam_a_contains_what_it_is_for():
    for name in ("sam_a", "sam_a_primary"):
        g = restated(name)
        run = g["run"]
        assert sorted(len(s) for s in run["contigs"].values()) == [300, 700, 1500]
        assert [cut for _, _, cut in g["per_chunk"]] == [False, False, True], "the coverage cut on exactly one contig"
        lines = [ln for ln in run["sam"].split(b"\n") if ln and not ln.startswith(b"@")]
        assert 110 <= len(lines) <= 130 and sum(1 for ln in run["sam"].split(b"\n") if ln[:3] in G.HEADERS) >= 4
        assert {0, 16, 256, 272, 2048, 4} <= set(int(ln.split(b"\t")[1]) for ln in lines)
        assert sum(1 for ln in lines if len(ln.split()) == 8) == 1
        assert any(ch.islower() for s in run["contigs"].values() for ch in s) and any("N" in s for s in run["contigs"].values())
        assert any(any(chr(b).islower() for b in r["seq"]) for r in g["recs"])
        ops = [[chr(op) for op, _ in r["runs"]] for r in g["recs"]]
        assert any(o[0] == "H" and o[1] == "S" for o in ops) and any(o[-1] == "H" and o[-2] == "S" for o in ops)
        assert any(o[0] == "S" for o in ops) and any(o[-1] == "S" for o in ops)
        assert all(1 <= n <= 20 for r in g["recs"] if r["qry_id"] != "read_twice" for op, n in r["runs"] if chr(op) in "MID")
        twice = [a for a in dict(g["chunks"])["ctg_1"] if a.qry_id == "read_twice"]
        assert len(twice) == 2 and twice[0].qry_end - twice[0].qry_start == twice[1].qry_end - twice[1].qry_start
        order = [r["pos"] - 1 for r in g["recs"] if r["qry_id"] == "read_twice"]
        assert [a.trg_start for a in twice] == order, "the tie keeps the shuffled order"
        secondary = sum(1 for a in g["chunks"][0][1] if a.is_secondary)
        assert (secondary > 0) == (name == "sam_a")


def test_sam_edges_contains_what_it_is_for():
    g = restated("sam_edges")
    cols = [int(n) for n in np.diff(g["want"]["col_off"])]
    cigars = [G.cigar_of([(chr(op), n) for op, n in r["runs"]]) for r in g["recs"]]
    assert {1, 63, 64, 65, 128, 129} <= set(cols)
    for single in ("64M", "10M65I10M", "10M1000D10M"):
        assert single in cigars
    assert "1M1I1M1D" * 75 in cigars and cols[cigars.index("1M1I1M1D" * 75)] == 300
    assert {"5M2H3M", "3M2S3M", "4M0M4M", "30I", "40D"} <= set(cigars)
    by_cigar = {c: k for k, c in enumerate(cigars)}
    want = g["want"]
    # H and S in the middle count on the right
    k = by_cigar["5M2H3M"]
    assert (want["qry_start"][k], want["qry_end"][k], want["qry_len"][k]) == (0, 8, 10)
    k = by_cigar["3M2S3M"]
    assert (want["qry_start"][k], want["qry_end"][k], want["qry_len"][k]) == (0, 6, 8)
    k = by_cigar["2H3S20M1I20M4S5H"]
    assert (want["qry_start"][k], want["qry_end"][k], want["qry_len"][k]) == (5, 46, 55)
    k = by_cigar["30I"]
    assert bytes(want["trg_cols"][int(want["col_off"][k]):int(want["col_off"][k + 1])]) == b"-" * 30 and want["trg_start"][k] == want["trg_end"][k]
    k = by_cigar["40D"]
    assert bytes(want["qry_cols"][int(want["col_off"][k]):int(want["col_off"][k + 1])]) == b"-" * 40 and want["err_rate"][k] == 1.0
    assert any(r["qry_id"] == "last_base" and want["trg_end"][k] == 1400 == len(g["run"]["contigs"]["edge_1"]) for k, r in enumerate(g["recs"]))
    # two adjacent one-column alignments and then a long one, in the order of the call
    assert any(cols[k] == 1 and cols[k + 1] == 1 and cols[k + 2] >= 129 for k in range(len(cols) - 2))
    assert sum(1 for c in cols if c == 1) >= 12


def findall(cigar):
    return [(t[-1], int(t[:-1])) for t in re.findall(b"[0-9]+[MIDNSHP=X]", cigar)]


def test_cigar_parse_equals_findall(built):
    from flye_amd import gpu
    lib = gpu.load_library()
    crafted = [b"", b"10M", b"10M2I3D4N5S6H7P8=9X", b"xx12M,,0I", b"5 7M=3X9", b"12", b"M", b"3M4", b"007S1H", b"1M\n", b"*",
               b"4294967295M", b"12m3M", b"1M2", b"--3D--", b"9Z8M", b"1M" * 500, b"\x0012M\xff3I", b"1 M2 I33D"]
    for cigar in crafted:
        ops, lens = gpu.cigar_parse(cigar)
        assert [(int(o), int(n)) for o, n in zip(ops, lens)] == findall(cigar), cigar
    # a capacity that is too small: FG_ERR_ARG, n_runs says what is needed, the first cap tokens are written
    ops, lens, n = np.zeros(2, np.uint8), np.full(3, 77, np.uint32), C.c_uint64(99)
    assert lib.fg_cigar_parse(b"1M2I3D4M", 8, ops.ctypes.data, lens.ctypes.data, 2, C.byref(n)) == -3
    assert n.value == 4 and list(ops) == [ord("M"), ord("I")] and list(lens) == [1, 2, 77]
    assert lib.fg_cigar_parse(b"1M2I3D4M", 8, None, None, 0, C.byref(n)) == -3 and n.value == 4
    assert lib.fg_cigar_parse(b"", 0, None, None, 0, C.byref(n)) == 0 and n.value == 0
    assert lib.fg_cigar_parse(None, 0, None, None, 0, C.byref(n)) == 0 and n.value == 0
    assert lib.fg_cigar_parse(b"1M2I", 2, ops.ctypes.data, lens.ctypes.data, 2, C.byref(n)) == 0 and n.value == 1     # n_bytes, not NUL
    assert lib.fg_cigar_parse(b"1M", 2, ops.ctypes.data, lens.ctypes.data, 2, None) == -3
    assert lib.fg_cigar_parse(None, 2, ops.ctypes.data, lens.ctypes.data, 2, C.byref(n)) == -3
    assert lib.fg_cigar_parse(b"4294967296M", 11, ops.ctypes.data, lens.ctypes.data, 2, C.byref(n)) == -3       # beyond uint32


def _header_fields(text, name):
    body = re.search(r"struct " + name + r"\s*\{(.*?)\};", text, re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"[*\s]|\[\d+\]", "", n) for n in decl.split(None, 1)[1].split(",")]
    return names


def test_symbols_and_struct_layout(built):
    from flye_amd import gpu
    lib = gpu.load_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flye_gpu.h")).read(), flags=re.S)
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b" + sym + r"\s*\(", header), sym + " is not declared in include/flye_gpu.h"
        assert hasattr(lib, sym) and sym in gpu.ABI_SYMBOLS
    assert lib.fg_abi_version() == 4 and "#define FG_ABI_VERSION 4" in header
    assert _header_fields(header, "fg_expand_batch") == [n for n, _ in gpu.ExpandBatch._fields_]
    assert C.sizeof(gpu.ExpandBatch) == 12 * 8
    assert lib.fg_expand_cigars(None, 0, None, None, 0, None, None, None, None, None, None, None, 1, None) == -3
    lib.fg_release_expand(None)
    lib.fg_release_expand(C.byref(gpu.ExpandBatch()))
    assert "fg_cigar.hip" in open(os.path.join(ROOT, "flye_amd", "csrc", "Makefile")).read()
    assert gpu.Alignment._fields == G.Alignment._fields and len(gpu.Alignment._fields) == 14


# ---- 2. the device ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(built):
    from flye_amd import gpu
    c = gpu.Context(17, 0)          # no reads, no index: the call needs a device and a stream
    yield c
    c.close()


def check(res, want, cols=True):
    for k in OUT_KEYS:
        if k in ("trg_cols", "qry_cols") and not cols:
            assert getattr(res, k) is None
            continue
        got = getattr(res, k)
        assert got.dtype == want[k].dtype and got.tobytes() == want[k].tobytes(), k


TILES = [("sam_a", "64"), ("sam_a", "256"), ("sam_a", None), ("sam_a_primary", None), ("sam_edges", "64"), ("sam_edges", None)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,tile", TILES)
def test_golden_runs_on_the_device(ctx, monkeypatch, name, tile):
    g = restated(name)
    if tile is not None:
        monkeypatch.setenv("FG_CIGAR_TILE", tile)
    res = ctx.expand_cigars(**g["args"])
    check(res, g["want"])
    assert {"k_cig_advance", "k_cig_scan", "k_cig_place", "k_cig_expand"} <= set(ctx.kernel_times())
    assert res.same_as(ctx.expand_cigars(**g["args"]))
    # want_cols = 0: the same integers and err_rate, no columns
    check(ctx.expand_cigars(want_cols=False, **g["args"]), g["want"], cols=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sam_a", "sam_edges"])
def test_results_do_not_depend_on_the_cut(ctx, monkeypatch, name):
    from flye_amd import gpu
    g = restated(name)
    whole = ctx.expand_cigars(**g["args"])
    longest = int(np.diff(g["want"]["col_off"]).max())
    for env in ({"FG_CIGAR_BATCH_ALNS": "1"}, {"FG_CIGAR_BATCH_ALNS": "7"}, {"FG_CIGAR_BATCH_COLS": str(longest + 1)},
                {"FG_CIGAR_BATCH_ALNS": "7", "FG_CIGAR_TILE": "64"}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        cut = ctx.expand_cigars(**g["args"])
        check(cut, g["want"])
        assert cut.same_as(whole)
        check(ctx.expand_cigars(want_cols=False, **g["args"]), g["want"], cols=False)
        for k in env:
            monkeypatch.delenv(k)
    monkeypatch.setenv("FG_CIGAR_BATCH_COLS", str(longest - 1))
    with pytest.raises(gpu.FlyeGpuError) as e:
        ctx.expand_cigars(**g["args"])
    assert e.value.code == -8 and "FG_CIGAR_BATCH_COLS" in str(e.value)
    monkeypatch.delenv("FG_CIGAR_BATCH_COLS")
    check(ctx.expand_cigars(**g["args"]), g["want"])                 # the context works on afterwards


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sam_a", "sam_edges"])
def test_offsets_need_not_start_at_zero(ctx, name):
    """the alignments of the second chunk on, and the contigs from the second on, as windows into the arrays of the run"""
    g = restated(name)
    lo, hi = len(g["per_chunk"][0][1]), len(g["recs"])
    a = dict(g["args"])
    assert lo > 0 and int(a["aln_contig"][lo:].min()) >= 1
    a["contig_off"] = a["contig_off"][1:]
    a["aln_contig"] = a["aln_contig"][lo:hi] - 1
    a["ctg_pos"] = a["ctg_pos"][lo:hi]
    a["run_off"], a["read_off"] = a["run_off"][lo:hi + 1], a["read_off"][lo:hi + 1]
    assert a["contig_off"][0] > 0 and a["run_off"][0] > 0 and a["read_off"][0] > 0
    check(ctx.expand_cigars(**a), G.expand(g["recs"][lo:hi], g["run"]["contigs"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(G.RUNS))
def test_sam_alignments_equal_the_reference(ctx, tmp_path, name):
    from flye_amd import gpu
    g, meta = restated(name), CASES[name]
    run = g["run"]
    path = tmp_path / "aln.sam"
    path.write_bytes(run["sam"])
    sam = gpu.SamAlignments(ctx, str(path), run["contigs"], max_coverage=run["max_coverage"], use_secondary=run["use_secondary"])
    chunks = sam.chunks()
    assert [c for c, _ in chunks] == [c["contig"] for c in meta["chunks"]]
    for (contig, alns), stored, (_, mine) in zip(chunks, meta["chunks"], g["chunks"]):
        assert [row(a) for a in alns] == stored["alignments"], contig
        assert [tuple(a) for a in alns] == [tuple(a) for a in mine], contig
    assert "k_cig_expand" in ctx.kernel_times() and len(sam.result.col_off) == len(g["recs"]) + 1     # one call for the file
    by_contig = sam.by_contig()
    assert list(by_contig) == [c for c, _ in chunks]
    # SAM file -> consensus: the sequences the reference's consensus stage makes of its own reader's alignments
    contigs = [R.Contig(c, len(run["contigs"][c]), "linear") for c, _ in chunks]
    seqs, _ = gpu.ContigConsensus(ctx).consensus(contigs, by_contig)
    for c, stored in zip(contigs, meta["chunks"]):
        seq = seqs.get(c.id, "")
        assert (len(seq), sha(seq)) == (stored["consensus_len"], stored["consensus_sha256"]), c.id
    # SAM file -> bubbles: the restatement of the bubble stage on the restated alignments
    overrides = dict(min_polish_aln_len=50)
    bubbles, _, _ = gpu.BubbleMaker(ctx, **overrides).make(contigs, by_contig, "pacbio")
    want = []
    for c in contigs:
        r = R.make_contig(c, dict(g["chunks"])[c.id], R.params_for("pacbio", overrides))
        want += [(c.id, pos, cons.encode("latin-1"), [w.encode("latin-1") for w in ws]) for pos, cons, ws in r["bubbles"]]
    assert bubbles == want
    if name == "sam_a":
        assert len(bubbles) > 0
        gz = tmp_path / "aln2.sam.gz"
        import gzip
        with gzip.open(str(gz), "wb") as f:
            f.write(run["sam"])
        again = gpu.SamAlignments(ctx, str(gz), run["contigs"], max_coverage=run["max_coverage"], use_secondary=run["use_secondary"])
        assert again.chunks() == chunks


@pytest.mark.gpu
def test_sam_alignments_refuse_what_the_reference_refuses(ctx, tmp_path):
    from flye_amd import gpu
    contigs = {"a": "ACGTACGTAC", "b": "GGGGGCCCCC"}
    line = lambda q, c, cigar="4M", seq="ACGT": G.sam_line(q, 0, c, 1, cigar, seq)
    path = tmp_path / "unsorted.sam"
    path.write_text(line("r1", "a") + line("r2", "b") + line("r3", "a"))
    with pytest.raises(ValueError, match="Alignment file is not sorted"):
        gpu.SamAlignments(ctx, str(path), contigs)
    path.write_text(line("r1", "a", seq="*"))
    with pytest.raises(Exception, match="without read sequence"):
        gpu.SamAlignments(ctx, str(path), contigs)
    path.write_text(line("r1", "a", cigar="2M2X"))
    with pytest.raises(gpu.FlyeGpuError) as e:
        gpu.SamAlignments(ctx, str(path), contigs)
    assert e.value.code == -7
    path.write_text("@HD\tVN:1\n")
    assert gpu.SamAlignments(ctx, str(path), contigs).chunks() == []


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuzz(ctx, monkeypatch, seed):
    g = restated("fuzz_%d" % seed, G.fuzz(seed))
    cols = np.diff(g["want"]["col_off"])
    assert 0 < len(g["recs"]) <= 200 and int(cols.max()) <= 400 and int(cols.min()) >= 1
    assert any(n == 0 for r in g["recs"] for _, n in r["runs"])
    check(ctx.expand_cigars(**g["args"]), g["want"])
    monkeypatch.setenv("FG_CIGAR_TILE", "64")
    monkeypatch.setenv("FG_CIGAR_BATCH_ALNS", "5")
    check(ctx.expand_cigars(**g["args"]), g["want"])
    check(ctx.expand_cigars(want_cols=False, **g["args"]), g["want"], cols=False)


@pytest.mark.gpu
def test_empty_batch_and_group_member(ctx):
    from flye_amd import gpu
    res = ctx.expand_cigars([0], b"", [], [], [0], b"", [], [0], b"")
    assert list(res.col_off) == [0] and len(res.trg_cols) == 0 and len(res.matches) == 0 and len(res.err_rate) == 0
    lib = gpu.load_library()
    b = gpu.ExpandBatch()
    assert lib.fg_expand_cigars(ctx.h, 0, None, None, 0, None, None, None, None, None, None, None, 1, C.byref(b)) == 0
    assert b.n_alignments == 0 and b.col_off[0] == 0
    lib.fg_release_expand(C.byref(b))
    assert b.col_off is None or not b.col_off
    g = restated("sam_edges")
    grp = gpu.Group([0, 0])
    try:
        check(grp.member(1).expand_cigars(**g["args"]), g["want"])
    finally:
        grp.close()


@pytest.mark.gpu
def test_argument_errors(ctx, monkeypatch):
    from flye_amd import gpu
    lib = gpu.load_library()
    g = restated("sam_edges")
    f = {k: v.copy() for k, v in g["args"].items()}
    order = ("contig_off", "contig_seq", "aln_contig", "ctg_pos", "run_off", "run_op", "run_len", "read_off", "read_seq")
    n_contigs, n = len(f["contig_off"]) - 1, len(f["aln_contig"])

    def call(out=True, want_cols=1, **kw):
        a = dict(f, **kw)
        p = [None if a[k] is None else a[k].ctypes.data for k in order]
        b = gpu.ExpandBatch()
        b.n_alignments = 123                                           # must be cleared by a call that fails
        rc = lib.fg_expand_cigars(ctx.h, n_contigs, p[0], p[1], n, *p[2:], want_cols, C.byref(b) if out else None)
        if rc == 0:
            assert b.n_alignments == n
            lib.fg_release_expand(C.byref(b))
        elif out:
            assert bytes(b) == bytes(C.sizeof(gpu.ExpandBatch)), "the output of a failed call is left empty"
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

    assert call() == 0
    assert call(out=False) == -3
    for name in order:
        assert call(**{name: None}) == -3, name
    for name in ("contig_off", "run_off", "read_off"):
        assert call(**swapped(name)) == -3, name
    k = [G.cigar_of([(chr(op), c) for op, c in r["runs"]]) for r in g["recs"]].index("4M0M4M")
    r0 = int(f["run_off"][k])
    for op in b"NP=X":
        assert call(**changed("run_op", r0 + 1, op)) == -7, chr(op)
    for op in (ord("Z"), ord("m"), 0, 200):
        assert call(**changed("run_op", r0 + 1, op)) == -3, op
    assert call(**changed("aln_contig", 3, n_contigs)) == -3
    for pos in (0, -5):
        assert call(**changed("ctg_pos", 3, pos)) == -3, pos
    for name in ("contig_seq", "read_seq"):
        for byte in (128, 255):
            assert call(**changed(name, len(f[name]) // 2, byte)) == -3, (name, byte)
    # one run more than SEQ holds / than the contig holds
    need = sum(c for op, c in g["recs"][k]["runs"] if chr(op) in "MIS")
    assert call(**changed("run_len", r0, 4 + len(g["recs"][k]["seq"]) - need)) == 0
    assert call(**changed("run_len", r0, 4 + len(g["recs"][k]["seq"]) - need + 1)) == -3
    last = [r["qry_id"] for r in g["recs"]].index("last_base")
    assert call(**changed("ctg_pos", last, int(f["ctg_pos"][last]) + 1)) == -3
    assert call(**changed("ctg_pos", last, int(f["ctg_pos"][last]) - 1)) == 0
    # no columns; totals beyond int32
    zero = f["run_len"].copy()
    zero[r0:int(f["run_off"][k + 1])] = 0
    assert call(run_len=zero) == -3
    big = dict(changed("run_op", r0 + 1, ord("H")), **changed("run_len", r0 + 1, 3000000000))
    assert call(**big) == -3
    big["run_len"][r0 + 1] = 2000000000
    assert call(**big) == 0
    # the wrapper gives the code and the text
    with pytest.raises(gpu.FlyeGpuError) as e:
        ctx.expand_cigars(**dict(f, **changed("run_op", r0 + 1, ord("N"))))
    assert e.value.code == -7 and "CIGAR operation N" in str(e.value)
    assert call(want_cols=0) == 0
    check(ctx.expand_cigars(**g["args"]), g["want"])                 # the context is usable after the errors
