"""fg_sam_parse / gpu.Context.sam_parse / gpu.SamAlignments(device_text=True): the SAM text cut into lines, records, chunks,
tokens, integers, CIGAR runs and spans on the device.

Yardsticks: tests/sam_text_restate.py (the contract of include/flye_gpu.h in plain Python, bytes to arrays), itself pinned on
the runs of tests/cigar_restate.py against that module's reader, against gpu.cigar_parse and against the reference's golden
records (tests/golden/cigar_cases.json), and on crafted texts against Python's own bytes.find, bytes.split, re.findall and
int.  With a GPU: every output array of the call against the restatement, under both tile sizes and every kind of sub-batch
cut, and the mirror with device_text=True against the host tokeniser.  Parity is exact everywhere: there is no tolerance."""
import collections
import ctypes as C
import gzip
import inspect
import json
import os
import random
import re

import numpy as np
import pytest

import bubbles_restate as R
import cigar_restate as G
import divergence_restate as DR
import partition_restate as P
import sam_text_craft as K
import sam_text_restate as T
import test_fused_columns as F          # RestatedContext and golden_row; its tests are not collected from here

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("fg_sam_parse", "fg_release_sam_text")
CASES = json.load(open(os.path.join(R.GOLDEN, "cigar_cases.json")))
RUNS = dict(G.RUNS)
RUNS.update({"fuzz_%d" % s: (lambda s=s: G.fuzz(s)) for s in (1, 2, 3)})
_CACHE = {}


def run_of(name):
    if name not in _CACHE:
        _CACHE[name] = RUNS[name]()
    return _CACHE[name]


def all_texts():
    """name -> text: the crafted set, the texts around byte 256 and the runs of cigar_restate"""
    out = dict(K.TEXTS)
    out.update({"boundary_%d" % i: t for i, t in enumerate(K.boundary_texts())})
    out.update({name: run_of(name)["sam"] for name in RUNS})
    return out


def restated(name):
    key = ("restated", name)
    if key not in _CACHE:
        _CACHE[key] = T.parse(all_texts()[name])
    return _CACHE[key]


# ---- 1. without a GPU ------------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_bound(built):
    from flye_amd import gpu
    lib = gpu.load_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flye_gpu.h")).read(), flags=re.S)
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b" + sym + r"\s*\(", header), sym + " is not declared in include/flye_gpu.h"
        assert hasattr(lib, sym) and sym in gpu.ABI_SYMBOLS
        assert getattr(lib, sym).argtypes is not None
    assert "struct fg_sam_text" in header and lib.fg_abi_version() == 4
    assert callable(gpu.Context.sam_parse)
    assert inspect.signature(gpu.SamAlignments.__init__).parameters["device_text"].default is False
    for fn in (gpu.DivergenceFinder.find_divergence, gpu.DivergenceFinder.find_divergence_sam, gpu.ReadPartitioner.partition_reads,
               gpu.ReadPartitioner.partition_reads_sam, gpu.ReadPartitioner._read_records, gpu.ReadPartitioner._read_alignment):
        assert inspect.signature(fn).parameters["device_text"].default is False
    assert lib.fg_sam_parse(None, None, 0, None) == -3         # a NULL context is refused before anything is read
    assert "fg_samtext.hip" in open(os.path.join(ROOT, "flye_amd", "csrc", "Makefile")).read()
    # the struct of the binding has the header's fields in the header's order
    body = re.search(r"struct fg_sam_text \{(.*?)\};", header, re.S).group(1)
    assert re.findall(r"(\w+);", body) == [name for name, _ in gpu.SamText._fields_]


@pytest.mark.parametrize("name", sorted(RUNS))
def test_restatement_equals_the_reader_restated_before(built, name):
    """records, chunk names and sizes, tokens, flag, pos, runs and spans against cigar_restate and gpu.cigar_parse"""
    from flye_amd import gpu
    run, res = run_of(name), restated(name)
    text = run["sam"]
    chunks = G.file_chunks(text)
    lines = [ln for _, lns in chunks for ln in lns]
    assert res["n_records"] == len(lines) and res["n_chunks"] == len(chunks)
    assert np.diff(res["chunk_off"]).tolist() == [len(lns) for _, lns in chunks]
    assert [T.token(text, res, int(r), "tab_rname") for r in res["chunk_off"][:-1]] == [c for c, _ in chunks]
    by_line = {}
    for r, line in enumerate(lines):
        assert T.token(text, res, r, "line") + b"\n" == line
        assert text.split(b"\n")[int(res["line_no"][r]) - 1] + b"\n" == line
        tok = line.strip().split()
        assert bool(res["status"][r] & 1) == (len(tok) < 11)
        if len(tok) < 11:
            continue
        by_line[line] = r
        assert [T.token(text, res, r, k) for k in ("qname", "rname", "cigar", "seq")] == [tok[0], tok[2], tok[5], tok[9]]
        assert res["status"][r] == 0 and (res["flag"][r], res["pos"][r]) == (int(tok[1]), int(tok[3]))
        ops, lens = gpu.cigar_parse(tok[5])
        a, b = int(res["run_off"][r]), int(res["run_off"][r + 1])
        assert res["run_op"][a:b].tolist() == ops.tolist() and res["run_len"][a:b].tolist() == lens.tolist()
        assert (res["qry_start"][r], res["qry_end"][r]) == gpu.SamAlignments._span(ops, lens)
    # the records the reader restated before selects, in its order, are these records
    for (_, recs, _), (_, lns) in zip(G.records(run), chunks):
        shuffled = list(lns)
        random.Random(42).shuffle(shuffled)
        order = list(range(len(lns)))
        random.Random(42).shuffle(order)
        assert shuffled == [lns[i] for i in order], "the shuffle is a permutation of the count alone"
        picked = iter(shuffled)
        for rec in recs:
            line = next(ln for ln in picked if ln.split()[0].decode() == rec["qry_id"] and len(ln.split()) >= 11 and
                        int(ln.split()[3]) == rec["pos"])
            r = by_line[line]
            a, b = int(res["run_off"][r]), int(res["run_off"][r + 1])
            assert (res["flag"][r], res["pos"][r]) == (rec["flags"], rec["pos"])
            assert list(zip(res["run_op"][a:b].tolist(), res["run_len"][a:b].tolist())) == rec["runs"]
            assert T.token(text, res, r, "seq") == rec["seq"]


class RestatedSamContext(F.RestatedContext):
    """sam_parse by the restatement, expand_cigars by the restatement: the mirror's own logic, without a device"""

    def sam_parse(self, data):
        from flye_amd import gpu
        res = T.parse(bytes(data))
        return gpu.SamTextResult(np.frombuffer(bytes(data), np.uint8), **res)


def same_chunks(got, want):
    assert [c for c, _ in got] == [c for c, _ in want]
    for (contig, a), (_, b) in zip(got, want):
        assert len(a) == len(b), contig
        for x, y in zip(a, b):
            assert type(x) is type(y) and x._fields == y._fields
            for f in x._fields:
                u, v = getattr(x, f), getattr(y, f)
                if isinstance(u, np.ndarray):
                    assert u.dtype == v.dtype and np.array_equal(u, v), (contig, f)
                else:
                    assert type(u) is type(v) and u == v, (contig, f)


@pytest.mark.parametrize("name", sorted(G.RUNS))
def test_selection_from_the_arrays_gives_the_golden_rows(built, tmp_path, name):
    from flye_amd import gpu
    run, meta = run_of(name), CASES[name]
    path = tmp_path / "aln.sam"
    path.write_bytes(run["sam"])
    kw = dict(max_coverage=run["max_coverage"], use_secondary=run["use_secondary"])
    chunks = gpu.SamAlignments(RestatedSamContext(), str(path), run["contigs"], device_text=True, **kw).chunks()
    assert [c for c, _ in chunks] == [c["contig"] for c in meta["chunks"]]
    for (contig, alns), stored in zip(chunks, meta["chunks"]):
        assert [F.golden_row(a) for a in alns] == stored["alignments"], contig
    same_chunks(chunks, gpu.SamAlignments(F.RestatedContext(), str(path), run["contigs"], **kw).chunks())
    same_chunks(gpu.SamAlignments(RestatedSamContext(), str(path), run["contigs"], want_cols=False, device_text=True, **kw).chunks(),
                gpu.SamAlignments(F.RestatedContext(), str(path), run["contigs"], want_cols=False, **kw).chunks())


def reader_lines(text):
    """the lines a Python file object gives, newline included"""
    parts = text.split(b"\n")
    return [ln + b"\n" for ln in parts[:-1]] + ([parts[-1]] if parts[-1] else [])


@pytest.mark.parametrize("name", sorted(K.TEXTS) + ["boundary_0", "boundary_30"])
def test_restatement_equals_python_on_the_crafted_texts(name):
    """the reference's own statements, line by line: find for the tabs, strip().split() for the tokens, findall for the runs,
    int for FLAG and POS"""
    text, res = all_texts()[name], restated(name)
    lines = reader_lines(text)
    assert b"".join(lines) == text and res["n_lines"] == len(lines)
    r, names = 0, []
    for no, line in enumerate(lines, 1):
        if line[:3] in G.HEADERS:
            continue
        tab_1 = line.find(b"\t")
        tab_2 = line.find(b"\t", tab_1 + 1)
        tab_3 = line.find(b"\t", tab_2 + 1)
        if tab_2 == -1 or tab_3 == -1:
            continue
        assert r < res["n_records"] and res["line_no"][r] == no and T.token(text, res, r, "line") == line.rstrip(b"\n")
        assert T.token(text, res, r, "tab_rname") == line[tab_2 + 1:tab_3]
        if not names or names[-1][0] != line[tab_2 + 1:tab_3]:
            names.append([line[tab_2 + 1:tab_3], 0])
        names[-1][1] += 1
        tok = line.strip().split()
        st = int(res["status"][r])
        assert bool(st & 1) == (len(tok) < 11)
        a, b = int(res["run_off"][r]), int(res["run_off"][r + 1])
        if st & 1:
            assert a == b and st == 1
        else:
            assert [T.token(text, res, r, k) for k in ("qname", "rname", "cigar", "seq")] == [tok[0], tok[2], tok[5], tok[9]]
            for bit, k, field in ((2, 1, "flag"), (4, 3, "pos")):
                plain = re.fullmatch(b"[+-]?[0-9]+", tok[k]) is not None
                if st & bit:
                    assert res[field][r] == 0 and (not plain or not -2 ** 31 <= int(tok[k]) < 2 ** 31)
                else:
                    assert plain and res[field][r] == int(tok[k])
            assert bool(st & 8) == (tok[9] == b"*")
            found = [(t[-1], int(t[:-1])) for t in re.findall(b"[0-9]+[MIDNSHP=X]", tok[5])]
            assert res["run_op"][a:b].tolist() == [op for op, _ in found]
            assert res["run_len"][a:b].tolist() == [n if n < 2 ** 32 else 0 for _, n in found]
            assert bool(st & 16) == any(n >= 2 ** 32 for _, n in found)
            if not st & 16:
                hard_left, _, soft_left, soft_right = G.clips(found) if found else (0, 0, 0, 0)
                q = sum(n for op, n in found if chr(op) in "MIS")
                assert (res["qry_start"][r], res["qry_end"][r]) == (hard_left + soft_left, q + hard_left - soft_right), tok[5]
        r += 1
    assert r == res["n_records"] and res["n_chunks"] == len(names)
    assert np.diff(res["chunk_off"]).tolist() == [n for _, n in names]


def test_crafted_texts_contain_what_they_are_for():
    X = K.TEXTS
    rec_lines = lambda t: [ln for ln in t.split(b"\n") if ln[:3] not in G.HEADERS and ln.count(b"\t") >= 3]
    assert X["empty"] == b"" and rec_lines(X["headers_only"]) == [] and {ln[:3] for ln in X["headers_only"].split(b"\n") if ln} == set(G.HEADERS)
    assert all(ln.count(b"\t") >= 3 for ln in X["headers_only"].split(b"\n")[2:5]), "headers that only the prefix test drops"
    assert not X["no_final_newline"].endswith(b"\n") and X["final_blank_line"].endswith(b"\n\n")
    assert X["crlf"].count(b"\r\n") == X["crlf"].count(b"\n") == 2
    assert b"\nx\n" in X["short_lines"] and b"\n@P\n" in X["short_lines"] and b"\n\n" in X["short_lines"]
    hp = X["header_prefix"].split(b"\n")
    assert hp[0].startswith(b"@PGx") and hp[0].count(b"\t") >= 3 and hp[1].startswith(b"@XX") and hp[1].count(b"\t") == 3
    for k in range(4):
        with_11, without = X["tabs_%d" % k].split(b"\n")[:2]
        assert with_11.count(b"\t") == without.count(b"\t") == k and len(with_11.split()) == 11 and len(without.split()) < 11
    mid = rec_lines(X["ten_tokens_mid_chunk"])
    assert len(mid) == 7 and len(mid[3].split()) == 10 and len({ln.split(b"\t")[2] for ln in mid}) == 1
    a, b = list(range(7)), list(range(6))
    random.Random(42).shuffle(a); random.Random(42).shuffle(b)
    assert [i for i in a if i != 3] != [i if i < 3 else i + 1 for i in b], "leaving the short record out of the count changes the order"
    e = X["empty_tab_rname"]
    assert b"\t\t" in e and e.split(b"\t")[2] == b"" and len(e.split()) >= 11 and e.split()[2] != e.split(b"\t")[3 - 1]
    s = X["space_in_field"]
    assert s.split(b"\t")[2] == b"c 1" and s.split()[2] == b"c" and len(s.split()) >= 11
    assert b"\x0b" in X["vt_ff"] and b"\x0c" in X["vt_ff"] and len(X["vt_ff"].split()) == 11 and X["vt_ff"].count(b"\t") >= 3
    assert len(X["exactly_11"].split()) == 11 and len(X["more_than_11"].split()) > 11
    for form in ("+4", "-1", "007", "4x", "1_0", "2147483648", "-2147483649"):
        assert form in K.INT_FORMS
    assert [ln.split()[1].decode() for ln in rec_lines(X["flag_forms"])] == K.INT_FORMS
    assert [ln.split()[3].decode() for ln in rec_lines(X["pos_forms"])] == K.INT_FORMS
    assert int(b"1_0") == 10 and int(b"+4") == 4 and int(b"007") == 7, "what Python's int makes of them"
    assert rec_lines(X["seq_star"])[0].split()[9] == b"*"
    for form in ("*", "5MM", "12AB3M", "0012M", "3m", "4294967295M", "4294967296M", "7N2P1=1X"):
        assert form in K.CIGAR_FORMS
    runs = [re.findall(b"[0-9]+[MIDNSHP=X]", c.encode()) for c in K.CIGAR_FORMS]
    assert any([t[-1:] for t in r[:3]] == [b"H", b"H", b"S"] for r in runs) and any([t[-1:] for t in r[-2:]] == [b"S", b"H"] for r in runs)
    assert max(len(r) for r in runs) > 256, "more runs than the smallest tile has bytes"
    assert {32, 33} <= {len(r) for r in runs}, "either side of the cut between a lane and a wave"
    assert any(len(r) > 33 and r[0][-1:] == b"H" and r[1][-1:] == b"S" for r in runs)
    ch = [ln.split(b"\t")[2] for ln in rec_lines(X["chunks"])]
    assert ch == [b"c1", b"c1", b"c2", b"c3", b"c3", b"c33", b"c3"]
    at = X["chunks"].index(b"q2\t")
    assert b"@CO" in X["chunks"][:at] and b"junk\n" in X["chunks"][:at], "dropped lines inside the chunk of c1"


def test_boundary_texts_put_every_feature_on_both_sides():
    feats = [K.features(t) for t in K.boundary_texts()]
    B = K.BOUNDARY
    for pick in (lambda f: f["line_start"], lambda f: f["token_starts"][5], lambda f: f["token_ends"][5], lambda f: f["token_starts"][9],
                 lambda f: f["token_ends"][10], lambda f: f["third_tab"], lambda f: f["runs"][0][1], lambda f: f["runs"][1][0]):
        at = sorted(pick(f) for f in feats)
        assert {B - 1, B, B + 1} <= set(at)
    for k in range(3):
        assert any(f["runs"][k][0] < B <= f["runs"][k][1] for f in feats), "a digit run on one side, its op byte on the other"
    assert any(f["runs"][0][0] < B < f["runs"][0][1] for f in feats), "a digit run cut in two"
    assert any(f["token_starts"][5] < B <= f["token_ends"][5] for f in feats)


# ---- 2. the device ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(built):
    from flye_amd import gpu
    c = gpu.Context(17, 0)          # no reads, no index: the call needs a device and a stream
    yield c
    c.close()


def equal(got, want, what=""):
    for k in T.COUNTS:
        assert getattr(got, k) == want[k], (what, k)
    for k, dt in T.FIELDS:
        a = getattr(got, k)
        assert a.dtype == dt and a.shape == want[k].shape and np.array_equal(a, want[k]), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", ["256", None, "16384"])
def test_every_text_equals_the_restatement(ctx, monkeypatch, tile):
    if tile:
        monkeypatch.setenv("FG_SAM_TILE", tile)
    for name, text in all_texts().items():
        equal(ctx.sam_parse(text), restated(name), name)
    assert {"k_sam_classify", "k_sam_lines", "k_sam_scatter", "k_sam_record", "k_sam_runs", "k_sam_span"} <= set(ctx.kernel_times())


def cuts(text, budget):
    """where the sub-batches end: whole lines of at most budget bytes, the last newline inside the budget"""
    out, at = [], 0
    while len(text) - at > budget:
        nl = text.rfind(b"\n", at, at + budget)
        assert nl >= 0
        at = nl + 1
        out.append(at)
    return out


CUT_TEXT = b"".join(K.rec(qname="r%d" % i, rname=c) for i, c in enumerate(["c1", "c1", "c2", "c2", "c2", "c3", "c4", "c4"]))


@pytest.mark.gpu
@pytest.mark.parametrize("tile", ["256", None])
def test_sub_batch_cuts_are_invisible(ctx, monkeypatch, tile):
    from flye_amd import gpu
    if tile:
        monkeypatch.setenv("FG_SAM_TILE", tile)
    want = T.parse(CUT_TEXT)
    L = len(K.rec(qname="r0"))
    starts = [int(x) for x in want["line_off"]]
    assert starts == [i * L for i in range(8)] and want["chunk_off"].tolist() == [0, 2, 5, 6, 8]
    inside = {starts[r] for r in range(8)} - {starts[int(r)] for r in want["chunk_off"][:-1]}
    between = {starts[int(r)] for r in want["chunk_off"][1:-1]}
    seen = set()
    for budget in (L, 2 * L, 3 * L, 3 * L + 1, 4 * L - 1, 5 * L, 8 * L - 1, 8 * L):
        monkeypatch.setenv("FG_SAM_BATCH_BYTES", str(budget))
        equal(ctx.sam_parse(CUT_TEXT), want, budget)
        seen |= set(cuts(CUT_TEXT, budget))
    assert cuts(CUT_TEXT, L) == starts[1:], "a cut after every line"
    assert seen & inside and seen & between and set(cuts(CUT_TEXT, 3 * L)) & inside and set(cuts(CUT_TEXT, 2 * L)) <= between | inside
    # every text with a cut after as many lines as fit its longest line, which is a cut after every line for most
    for name, text in all_texts().items():
        longest = max(len(ln) + 1 for ln in text.split(b"\n"))
        monkeypatch.setenv("FG_SAM_BATCH_BYTES", str(longest))
        equal(ctx.sam_parse(text), restated(name), name)
        if text.endswith(b"\n") and len(text) > longest:
            monkeypatch.setenv("FG_SAM_BATCH_BYTES", str(longest - 1))
            with pytest.raises(gpu.FlyeGpuError) as e:
                ctx.sam_parse(text)
            assert e.value.code == -8 and "FG_SAM_BATCH_BYTES" in str(e.value)
    monkeypatch.setenv("FG_SAM_BATCH_BYTES", str(L))
    equal(ctx.sam_parse(CUT_TEXT), want, "the context works on afterwards")


@pytest.mark.gpu
def test_a_window_inside_a_larger_buffer(ctx, monkeypatch):
    for name in ("chunks", "cigar_forms", "sam_a", "no_final_newline"):
        text = all_texts()[name]
        for before, after in ((b"zz\tzz\tzz\tzz\n", b"tail\t1\t2\t3\n"), (b"x" * 301, b"\ty" * 77)):
            buf = before + text + after
            equal(ctx.sam_parse(buf, len(before), len(text)), restated(name), name)
            equal(ctx.sam_parse(np.frombuffer(buf, np.uint8), len(before), len(text)), restated(name), name)
    text = all_texts()["sam_edges"]
    longest = max(len(ln) + 1 for ln in text.split(b"\n"))
    monkeypatch.setenv("FG_SAM_BATCH_BYTES", str(longest + 5))
    equal(ctx.sam_parse(b"@" * 13 + text + b"\n\n", 13, len(text)), restated("sam_edges"))


@pytest.mark.gpu
def test_argument_errors_and_the_empty_batch(ctx):
    from flye_amd import gpu
    lib = gpu.load_library()
    text = all_texts()["chunks"]
    b = gpu.SamText()
    assert lib.fg_sam_parse(ctx.h, text, len(text), None) == -3 and b"fg_sam_parse" in lib.fg_last_error(ctx.h)
    C.memset(C.byref(b), 0xFF, C.sizeof(b))
    assert lib.fg_sam_parse(ctx.h, None, 5, C.byref(b)) == -3 and bytes(b) == bytes(C.sizeof(b))
    assert b"null text" in lib.fg_last_error(ctx.h)
    for empty in (b"", all_texts()["headers_only"], b"\n\n\n", b"no tabs at all"):
        res = ctx.sam_parse(empty)
        assert (res.n_records, res.n_chunks, res.n_runs) == (0, 0, 0) and res.chunk_off.tolist() == [0] and res.run_off.tolist() == [0]
        assert res.n_lines == T.parse(empty)["n_lines"]
    assert lib.fg_sam_parse(ctx.h, None, 0, C.byref(b)) == 0 and b.n_records == 0 and b.chunk_off[0] == 0 and b.run_off[0] == 0
    lib.fg_release_sam_text(C.byref(b))
    assert bytes(b) == bytes(C.sizeof(b))
    lib.fg_release_sam_text(C.byref(b))                         # releasing twice is harmless
    lib.fg_release_sam_text(None)
    equal(ctx.sam_parse(text), restated("chunks"), "the context works on afterwards")
    with pytest.raises(ValueError):
        ctx.sam_parse(text, 5, len(text))
    res = ctx.sam_parse(text)
    assert res.token(2, "qname") == b"q3" and res.token(2, "tab_rname") == b"c2" and res.token(0, "line") == K.rec(rname="c1")[:-1]
    assert [bytes(x).decode() for x in res.runs(0)[0:1]] == ["M"] and res.runs(0)[1].tolist() == [3]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(G.RUNS))
def test_the_mirror_with_device_text_equals_the_host_tokeniser(ctx, tmp_path, name):
    from flye_amd import gpu
    run, meta = run_of(name), CASES[name]
    path, gz = tmp_path / "aln.sam", tmp_path / "aln.sam.gz"
    path.write_bytes(run["sam"])
    with gzip.open(str(gz), "wb") as f:
        f.write(run["sam"])
    kw = dict(max_coverage=run["max_coverage"], use_secondary=run["use_secondary"])
    host = gpu.SamAlignments(ctx, str(path), run["contigs"], **kw)
    calls = getattr(ctx, "sam_parse_calls", 0)
    dev = gpu.SamAlignments(ctx, str(path), run["contigs"], device_text=True, **kw)
    assert ctx.sam_parse_calls == calls + 1, "one fg_sam_parse per file"
    same_chunks(dev.chunks(), host.chunks())
    assert dev.chunks() == host.chunks() and list(dev.by_contig()) == list(host.by_contig())
    for (contig, alns), stored in zip(dev.chunks(), meta["chunks"]):
        assert [F.golden_row(a) for a in alns] == stored["alignments"], contig
    same_chunks(gpu.SamAlignments(ctx, str(gz), run["contigs"], device_text=True, **kw).chunks(), host.chunks())
    host_r = gpu.SamAlignments(ctx, str(path), run["contigs"], want_cols=False, **kw)
    dev_r = gpu.SamAlignments(ctx, str(gz), run["contigs"], want_cols=False, device_text=True, **kw)
    same_chunks(dev_r.chunks(), host_r.chunks())
    contigs = [R.Contig(c, len(run["contigs"][c]), "linear") for c in sorted(run["contigs"])]
    for keep in (None, [k % 3 != 0 for k in range(sum(len(a) for _, a in host_r.chunks()))]):
        (ra, a), (rb, b) = dev_r.flatten(contigs, keep), host_r.flatten(contigs, keep)
        same_chunks([("all", ra)], [("all", rb)])
        assert sorted(a) == sorted(b)
        for k in a:
            assert np.array_equal(np.frombuffer(a[k], np.uint8) if isinstance(a[k], bytes) else np.asarray(a[k]),
                                  np.frombuffer(b[k], np.uint8) if isinstance(b[k], bytes) else np.asarray(b[k])), k
    ctx.sam_parse(run["sam"])
    assert "k_sam_classify" in ctx.kernel_times()


@pytest.mark.gpu
def test_device_text_refuses_what_the_reference_refuses(ctx, tmp_path):
    from flye_amd import gpu
    contigs = {"a": "ACGTACGTAC", "b": "GGGGGCCCCC"}
    line = lambda q, c, cigar="4M", seq="ACGT", flag=0, pos=1: G.sam_line(q, flag, c, pos, cigar, seq)
    path = tmp_path / "text.sam"

    def both(text, **kw):
        """the exception of either tokeniser, or its chunks"""
        path.write_text(text)
        out = []
        for device_text in (False, True):
            try:
                out.append(gpu.SamAlignments(ctx, str(path), contigs, device_text=device_text, **kw).chunks())
            except Exception as e:      # noqa: the two are compared below, whatever they are
                out.append((type(e), str(e), getattr(e, "code", None)))
        return out

    h, d = both(line("r1", "a") + line("r2", "b") + line("r3", "a"))
    assert h == d and h[0] is ValueError and "Alignment file is not sorted" in h[1]
    h, d = both(line("r1", "a", seq="*"))
    assert h == d and "without read sequence" in h[1]
    h, d = both(line("r1", "a", cigar="2M2X"))
    assert h == d and h[0] is gpu.FlyeGpuError and h[2] == -7
    h, d = both("@HD\tVN:1\n")
    assert h == d == []
    h, d = both(line("r1", "a", flag="4x"))
    assert h == d and h[0] is ValueError and "4x" in h[1]
    h, d = both(line("r1", "a", pos="1x"))
    assert h == d and h[0] is ValueError and "1x" in h[1]
    h, d = both(line("r1", "a", cigar="4294967296M"))
    assert h == d and h[0] is gpu.FlyeGpuError
    h, d = both(line("r1", "nowhere"))
    assert h == d and h[0] is KeyError
    h, d = both(line("r0", "a", flag=4, seq="*") + line("r1", "a", flag="1_6") + line("r2", "a", pos="+2") + line("r3", "a", flag="0_0", pos="0_3"))
    assert isinstance(h, list) and len(h[0][1]) == 3
    same_chunks(d, h)
    assert [a.qry_sign for a in h[0][1]] == ["-", "+", "+"] and sorted(a.trg_start for a in h[0][1]) == [0, 1, 2]
    # a record the reference never evaluates raises nothing: the cut ends the chunk before it
    many = "".join(line("r%d" % i, "a", cigar="10M", seq="ACGTACGTAC") for i in range(30)) + line("bad", "a", flag="x")
    order = list(range(31))
    random.Random(42).shuffle(order)
    h, d = both(many, max_coverage=order.index(30) - 1)
    assert isinstance(h, list) and len(h[0][1]) == order.index(30)
    same_chunks(d, h)
    h, d = both(many, max_coverage=order.index(30))
    assert h == d and h[0] is ValueError


@pytest.mark.gpu
def test_sam_a_end_to_end_over_either_reader(ctx, tmp_path):
    from flye_amd import gpu
    run = run_of("sam_a")
    path = tmp_path / "aln.sam"
    path.write_bytes(run["sam"])
    kw = dict(max_coverage=run["max_coverage"], use_secondary=run["use_secondary"], want_cols=False)
    host, dev = gpu.SamAlignments(ctx, str(path), run["contigs"], **kw), gpu.SamAlignments(ctx, str(path), run["contigs"], device_text=True, **kw)
    contigs = [R.Contig(c, len(run["contigs"][c]), "circular" if k == 1 else "linear") for k, c in enumerate(sorted(run["contigs"]))]
    one, two = gpu.ContigConsensus(ctx), gpu.ContigConsensus(ctx)
    assert one.consensus_sam(contigs, host, want_profile=True) == two.consensus_sam(contigs, dev, want_profile=True)
    F.same(two.result, one.result)
    assert one.aln_errors == two.aln_errors and len(one.aln_errors) > 0
    mk1, mk2 = gpu.BubbleMaker(ctx, min_polish_aln_len=50), gpu.BubbleMaker(ctx, min_polish_aln_len=50)
    made = mk1.make_sam(contigs, host, "pacbio", want_profile=True)
    assert made == mk2.make_sam(contigs, dev, "pacbio", want_profile=True) and len(made) > 0
    F.same(mk2.result, mk1.result)


Info = collections.namedtuple("Info", ["length"])


@pytest.mark.gpu
def test_find_divergence_sam_writes_the_same_files(ctx, tmp_path):
    from flye_amd import gpu
    name = sorted(DR.SAMS)[0]
    run = DR.SAMS[name]()
    sam, fasta = str(tmp_path / "aln.sam"), str(tmp_path / "template.fasta")
    with open(sam, "wb") as f:
        f.write(run["sam"])
    with open(fasta, "w") as f:
        f.write(DR.fasta_of(run["contigs"]))
    info = {cid: Info(len(seq)) for cid, seq in run["contigs"].items()}
    kinds = ("frequency", "positions", "summary")
    means = {}
    for tag, kw in (("host", {}), ("device", dict(device_text=True))):
        paths = [str(tmp_path / (k + "." + tag)) for k in kinds]
        means[tag] = gpu.DivergenceFinder(ctx, 1000).find_divergence_sam(sam, fasta, info, *paths, *run["thresholds"], **kw)
        cols = [str(tmp_path / (k + ".cols." + tag)) for k in kinds]
        assert gpu.DivergenceFinder(ctx, 1000).find_divergence(sam, fasta, info, *cols, *run["thresholds"], **kw) == means[tag]
    assert means["host"] == means["device"]
    for k in kinds:
        stored = R.read_gz("divergence_%s.%s.gz" % (name, k)).encode("latin-1")
        for ext in (".host", ".device"):
            assert open(str(tmp_path / (k + ext)), "rb").read() == stored, (k, ext)
        assert open(str(tmp_path / (k + ".cols.device")), "rb").read() == open(str(tmp_path / (k + ".cols.host")), "rb").read(), k


@pytest.mark.gpu
def test_partition_reads_sam_writes_the_same_files(ctx, tmp_path):
    from flye_amd import gpu
    name = sorted(P.SAMS)[0]
    run = P.SAMS[name]()
    wrote = {}
    for tag, method, kw in (("host", "partition_reads_sam", {}), ("device", "partition_reads_sam", dict(device_text=True)),
                            ("cols_host", "partition_reads", {}), ("cols_device", "partition_reads", dict(device_text=True))):
        os.mkdir(str(tmp_path / tag))
        args = P.write_files(run, str(tmp_path / tag))
        calls = getattr(ctx, "sam_parse_calls", 0)
        getattr(gpu.ReadPartitioner(ctx), method)(run["edges"], run["it"], run["side"], **args, **kw)
        assert (getattr(ctx, "sam_parse_calls", 0) > calls) == bool(kw)
        wrote[tag] = [open(p.format(run["it"], run["side"]), "rb").read() for p in (args["confirmed_pos_path"], args["part_file"])]
    stored = [R.read_gz("partition_%s.%s.gz" % (name, kind)).encode("latin-1") for kind in ("confirmed", "part")]
    assert wrote["host"] == stored and wrote["device"] == stored and wrote["cols_device"] == wrote["cols_host"]
