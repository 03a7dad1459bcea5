"""fg_polish_bubbles / gpu.BubbleProcessor: the bubble polishing of flye-modules polisher on the device.

Yardsticks: the records of the reference program itself (tests/golden/polish_*.gz, made by make_polish_golden.py: bubble
files, consensus files, --debug step logs) and the numpy restatement tests/polish_restate.py.  Without a GPU the
restatement is pinned on every golden run and the host-only parts of the ABI are checked; with one, every golden run,
the file forms, the scratch cuts, the switches, fuzz seeds and the argument errors.  No bubble is left out of any
comparison."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import polish_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(R.GOLDEN, "bin_cfg")
MATRICES = ("pacbio_substitutions.mat", "nano_r94_substitutions.mat", "tie.mat", "pos.mat")
NEW_SYMBOLS = ("fg_subs_matrix_load", "fg_polish_bubbles", "fg_release_polish")
_CACHE = {}


def golden(name):
    """one golden run, computed once: the bubbles as the reference's reader sees them, the reference's steps and final
    candidates per bubble (input order), the raw consensus and log texts, and the restatement's results"""
    if name not in _CACHE:
        matrix = R.RUNS[name][0]
        bubbles = R.parse_bubbles(R.read_gz(name + ".fa.gz"))
        cons, log = R.read_gz(name + ".cons.gz"), R.read_gz(name + ".log.gz")
        order = R.consensus_order(len(bubbles))
        steps_in_file_order = R.parse_log(log)
        cons_lines = cons.split("\n")
        assert len(steps_in_file_order) == len(bubbles) and len(cons_lines) == 2 * len(bubbles) + 1
        steps, cands = [None] * len(bubbles), [None] * len(bubbles)
        for k, i in enumerate(order):
            steps[i] = steps_in_file_order[k]
            cands[i] = cons_lines[2 * k + 1]
        s = R.load_matrix(os.path.join(CFG, matrix))
        details = [[] for _ in bubbles]
        restated = [R.polish_bubble(b.cand, b.branches, s, details=details[i]) for i, b in enumerate(bubbles)]
        _CACHE[name] = dict(matrix=matrix, bubbles=bubbles, cons=cons, log=log, steps=steps, cands=cands, restated=restated,
                            details=details, s=s)
    return _CACHE[name]


def by_name(run, header):
    g = golden(run)
    (i,) = [k for k, b in enumerate(g["bubbles"]) if b.header == header]
    return g["bubbles"][i], g["restated"][i], g["details"][i]


# ---- 1. the restatement against the reference's records (no GPU) -----------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.RUNS))
def test_restatement_is_pinned_on_the_reference(name):
    g = golden(name)
    meta = json.load(open(os.path.join(R.GOLDEN, "polish_cases.json")))[name]
    assert meta["n_bubbles"] == len(g["bubbles"]) and meta["matrix"] == g["matrix"]
    # the stored bubble file is what the generator makes today
    assert R.read_gz(name + ".fa.gz") == R.write_bubbles(R.RUNS[name][1]())
    for i, (cand, steps, status) in enumerate(g["restated"]):
        assert cand == g["cands"][i], (name, i)
        assert steps == g["steps"][i], (name, i)
    assert R.write_consensus(g["bubbles"], [r[0] for r in g["restated"]]) == g["cons"]
    assert R.write_log([r[1] for r in g["restated"]]) == g["log"]
    assert sum(len(r[1]) for r in g["restated"]) == meta["n_steps"]
    assert sum(1 for r in g["restated"] if r[2] & R.OVERFLOW) == meta["overflow_messages"]
    assert sum(1 for r in g["restated"] if r[2] & R.ITER_LIMIT) == meta["iteration_limit_messages"]


def test_crafted_cases_show_what_they_are_for():
    # the empty candidate stays empty: one step of score 0
    b, (cand, steps, status), _ = by_name("polish_a", "empty_candidate")
    assert cand == "" and steps == [("", 0)] and status == 0
    # the empty last branch counts 0: ACGT against ACGT and nothing scores what ACGT against ACGT alone scores
    b, (cand, steps, status), _ = by_name("polish_a", "empty_branch")
    s = golden("polish_a")["s"]
    assert b.branches[-1] == "" and R.alignment_score("ACGT", ["ACGT", ""], s) == -25808
    assert R.alignment_score("ACGT", ["ACGT", ""], s) == int(s[0, 0] + s[1, 1] + s[2, 2] + s[3, 3])
    # byte classes: other letters, lower case in the file (upper-cased by the reader), the gap byte
    assert "N" in by_name("polish_a", "classes_n")[0].cand and "-" in by_name("polish_a", "classes_gap")[0].cand
    assert ">classes_lower 2 3\nacgtacgt\n" in R.read_gz("polish_a.fa.gz")
    assert by_name("polish_a", "classes_lower")[0].cand == "ACGTACGT"
    # the iteration limit: 12 optimize steps, the candidate of the step before the last one; once with a fixer step
    b, (cand, steps, status), _ = by_name("polish_a", "iteration_limit")
    assert status == R.ITER_LIMIT and len(steps) == 12 and cand == steps[10][0] != steps[11][0]
    b, (cand, steps, status), _ = by_name("polish_a", "iteration_limit_fixer")
    assert status == R.ITER_LIMIT | R.FIXED and len(steps) == 13 and steps[12] == (cand, 0) and len(cand) == len(steps[10][0]) + 2
    # overflow: one step with a positive score is recorded, the candidate stays
    b, (cand, steps, status), _ = by_name("polish_d", "overflow")
    assert status == R.OVERFLOW and cand == "AAC" and len(steps) == 1 and steps[0][0] == "AAAC" and steps[0][1] > 0
    # the skip rule
    for header in ("skip_one_branch", "skip_5000"):
        b, (cand, steps, status), _ = by_name("polish_a", header)
        assert status == R.SKIPPED and steps == [] and cand == b.cand
    assert len(by_name("polish_a", "skip_5000")[0].cand) == 5000 and len(by_name("polish_a", "skip_one_branch")[0].branches) == 1
    # the dinucleotide fixer: grows, shrinks, and the run searches that change nothing
    b, (cand, steps, status), _ = by_name("polish_d", "dinuc_grow")
    assert status & R.FIXED and len(cand) == len(b.cand) + 2 and steps[-1] == (cand, 0)
    b, (cand, steps, status), _ = by_name("polish_d", "dinuc_shrink")
    assert status & R.FIXED and len(cand) == len(b.cand) - 2 and steps[-1] == (cand, 0)
    assert R.dinucleotide_run("GGCATATATATCCGA") == (3, 4) and R.dinucleotide_run("GGCATATCCGA") == (3, 2)
    assert R.dinucleotide_run("GGACACACCTGTGTGTG") == (2, 3)               # the run of 4 TG touches the end: never counted
    assert R.dinucleotide_run("CACACACTTGAGAGAGC") == (0, 3)               # shift 0 first; the equal run at shift 1 loses
    assert R.dinucleotide_run("CCACACACTTGAGAGAGC") == (2, 3)              # CC AC AC AC TT: the pairs of shift 0
    for header in ("dinuc_grow", "dinuc_shrink", "dinuc_run2", "dinuc_at_end", "dinuc_both_shifts"):
        assert not by_name("polish_a", header)[1][2] & R.FIXED
    # sizes around a piece of 64 columns; branch counts around 10 / 11 and 16 / 17
    g = golden("polish_a")
    lens = {len(b.cand) for b in g["bubbles"]} | {len(w) for b in g["bubbles"] for w in b.branches}
    assert {1, 2, 63, 64, 65, 127, 128, 129} <= lens
    counts = {len(b.branches) for b in g["bubbles"]}
    assert {2, 10, 11, 16, 17, 50} <= counts
    # more than 16 branches: std::sort is not stable there, and the stable order would pick another middle five
    for header in ("count_17", "count_23", "count_37", "count_50"):
        b = by_name("polish_a", header)[0]
        keys = [len(w) for w in b.branches]
        left = len(keys) // 2 - 2
        stable = sorted(range(len(keys)), key=lambda k: keys[k])[left:left + 5]
        assert sorted(b.branches[k] for k in stable) != sorted(R.middle_five(b.branches)), header
    # at 11 .. 16 branches std::sort is one insertion pass, which is stable
    b = by_name("polish_a", "count_16")[0]
    assert R.std_sort_perm([len(w) for w in b.branches]) == sorted(range(16), key=lambda k: len(b.branches[k]))
    # ties under tie.mat: two edits reach the best score of the first step, and the first in the reference's order wins
    for header, stage, first in (("tie_insert", "ins", "ACT"), ("tie_delete", "del", "AGT"), ("tie_substitute", "sub", "ACA"),
                                 ("tie_insert_t", "ins", "CAC")):
        b, (cand, steps, status), details = by_name("polish_c", header)
        assert details[0]["stage"] == stage and details[0]["ties"] >= 2, (header, details[0])
        assert steps[0][0] == first, (header, steps[0])


def test_std_sort_restatement_against_libstdcxx(built):
    """the second writing of std::sort's permutation agrees with the real one (the oracle library calls std::sort)"""
    from oracle import oracle as O
    rng = np.random.default_rng(5)
    for n in list(range(0, 70)) + [200, 1000]:
        for rep in range(4):
            keys = rng.integers(0, max(2, n // (rep + 1)), size=n)
            assert list(O.std_sort_perm(keys)) == R.std_sort_perm(keys.tolist()), n


# ---- 2. the host-only parts of the ABI (no GPU; fail without the feature) ------------------------------------------------
@pytest.mark.parametrize("matrix", MATRICES)
def test_subs_matrix_load(built, matrix):
    from flye_amd import gpu
    path = os.path.join(CFG, matrix)
    want = R.load_matrix(path)
    got = gpu.SubstitutionMatrix(path).table
    assert got.dtype == np.int64 and got.shape == (6, 6) and np.array_equal(got, want)
    assert not got[4].any() and not got[:, 4].any() and got[5, 5] == 0
    if matrix == "pos.mat":
        assert got[0, 0] == 53145                       # round(log(1.5) * 131072)


def test_subs_matrix_load_errors(built, tmp_path):
    from flye_amd import gpu
    lib = gpu.load_library()
    m = gpu.SubsMatrixStruct()
    assert lib.fg_subs_matrix_load(None, C.byref(m)) == -3
    assert lib.fg_subs_matrix_load(b"x", None) == -3
    assert lib.fg_subs_matrix_load(os.fsencode(tmp_path / "missing.mat"), C.byref(m)) == -3
    good = open(os.path.join(CFG, "pacbio_substitutions.mat")).read()

    def load(text):
        p = tmp_path / "m.mat"
        p.write_bytes(text.encode())
        return lib.fg_subs_matrix_load(os.fsencode(p), C.byref(m))

    assert load(good) == 0
    want = R.load_matrix(os.path.join(CFG, "pacbio_substitutions.mat"))
    # a trailing \r is tolerated, other lines are ignored
    assert load(good.replace("\n", "\r\n") + "comment\nnoins\t\t0.5\n\n") == 0
    assert np.array_equal(np.ctypeslib.as_array(m.score), want)
    for bad in ("mat\tN\t0.9\n", "mis\tA->N\t0.1\n", "mis\tN->A\t0.1\n", "del\tn\t0.1\n", "ins\t-\t0.1\n", "mat\ta\t0.9\n",
                "mat\tA\n", "del\tA\tx\n", "ins\t\t0.1\n"):
        assert load(good + bad) == -3, bad
    with pytest.raises(gpu.FlyeGpuError):
        gpu.SubstitutionMatrix(str(tmp_path / "missing.mat"))


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
    assert _header_fields(header, "fg_polish_batch") == [n for n, _ in gpu.PolishBatch._fields_]
    assert C.sizeof(gpu.PolishBatch) == 80 and C.sizeof(gpu.SubsMatrixStruct) == 288
    assert lib.fg_polish_bubbles(None, None, None, None, None, None, None, 0, 1, 1, None) == -3
    lib.fg_release_polish(None)
    empty = gpu.PolishBatch()
    lib.fg_release_polish(C.byref(empty))


def test_reader_and_writers_of_the_file_forms(built, tmp_path):
    """gpu.BubbleProcessor.read_bubbles reads what the restatement's reader reads (no device needed)"""
    from flye_amd import gpu
    for name in sorted(R.RUNS):
        p = tmp_path / (name + ".fa")
        p.write_bytes(R.read_gz(name + ".fa.gz").encode("latin-1"))
        got = gpu.BubbleProcessor.read_bubbles(str(p))
        want = golden(name)["bubbles"]
        assert [(b.header, b.position, b.cand, b.branches) for b in want] == [tuple(x) for x in got]
    bad = tmp_path / "bad.fa"
    bad.write_bytes(b">a 0 2\nACGT\n>0\n\n>1\nACGT\n")           # an empty branch that is not the last line
    with pytest.raises(RuntimeError):
        gpu.BubbleProcessor.read_bubbles(str(bad))
    with pytest.raises(ValueError):
        R.parse_bubbles(bad.read_text())


# ---- 3. the device -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(built):
    from flye_amd import gpu
    c = gpu.Context(17, 0)          # no reads, no index: the call needs a device and a stream
    yield c
    c.close()


def device(ctx, matrix, bubbles, **kw):
    from flye_amd import gpu
    m = matrix if isinstance(matrix, gpu.SubstitutionMatrix) else gpu.SubstitutionMatrix(os.path.join(CFG, matrix))
    return ctx.polish_bubbles(m, *R.flatten(bubbles), **kw)


def check_against(res, want, steps=True):
    """want[i] = (candidate, [(sequence, score)], status); every bubble is compared"""
    assert len(res.candidates) == len(want)
    for i, (cand, st, status) in enumerate(want):
        assert res.candidates[i].decode("latin-1") == cand, i
        assert int(res.n_steps[i]) == len(st), i
        assert int(res.status[i]) == status, i
        if steps:
            assert [(q.decode("latin-1"), sc) for q, sc in res.steps[i]] == st, i


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(R.RUNS))
def test_golden_runs_on_the_device(ctx, name):
    g = golden(name)
    res = device(ctx, g["matrix"], g["bubbles"])
    # the reference's record: candidates and steps from its files, the status bits as the restatement derives them
    # (pinned above on the reference's messages)
    check_against(res, [(g["cands"][i], g["steps"][i], g["restated"][i][2]) for i in range(len(g["bubbles"]))])
    times = ctx.kernel_times()
    assert {"k_pol_fill", "k_pol_edits", "k_pol_select"} <= set(times)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(R.RUNS))
def test_bubble_processor_files(ctx, name, tmp_path):
    from flye_amd import gpu
    g = golden(name)
    src = tmp_path / "bubbles.fa"
    src.write_bytes(R.read_gz(name + ".fa.gz").encode("latin-1"))
    bp = gpu.BubbleProcessor(ctx, os.path.join(CFG, g["matrix"]))
    bp.polishAll(str(src), str(tmp_path / "cons.fa"), str(tmp_path / "log.txt"))
    assert (tmp_path / "cons.fa").read_bytes() == g["cons"].encode("latin-1")
    assert (tmp_path / "log.txt").read_bytes() == g["log"].encode("latin-1")
    bp.polishAll(str(src), str(tmp_path / "cons2.fa"))                      # without the log: no steps are asked for
    assert (tmp_path / "cons2.fa").read_bytes() == g["cons"].encode("latin-1")


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"FG_POLISH_BATCH_BUBBLES": "1"}, {"FG_POLISH_BATCH_BUBBLES": "2"},
                                 {"FG_POLISH_SCRATCH_BYTES": str(24 << 20)}, {"FG_POLISH_SCRATCH_BYTES": str(64 << 20)}],
                         ids=["one_bubble", "two_bubbles", "24MiB", "64MiB"])
def test_results_do_not_depend_on_the_cut(ctx, monkeypatch, env):
    """Run (a) with every bubble a chunk of its own, with two bubbles per chunk, and under two small scratch budgets (its
    largest bubble, 50 branches of up to 130 bases against a candidate that grows to about 130, needs about 14 MB, the
    smallest a few hundred bytes: no budget makes every bubble its own chunk, so FG_POLISH_BATCH_BUBBLES does that)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    g = golden("polish_a")
    res = device(ctx, g["matrix"], g["bubbles"])
    check_against(res, [(g["cands"][i], g["steps"][i], g["restated"][i][2]) for i in range(len(g["bubbles"]))])


@pytest.mark.gpu
def test_scratch_budget_too_small_for_one_bubble(ctx, monkeypatch):
    from flye_amd import gpu
    monkeypatch.setenv("FG_POLISH_SCRATCH_BYTES", "1000")
    g = golden("polish_c")
    with pytest.raises(gpu.FlyeGpuError) as e:
        device(ctx, g["matrix"], [R.Bubble("big", 0, "ACGT" * 10, ["ACGT" * 10] * 4)])
    assert e.value.code == -8 and "FG_POLISH_SCRATCH_BYTES" in str(e.value)
    monkeypatch.delenv("FG_POLISH_SCRATCH_BYTES")
    res = device(ctx, g["matrix"], g["bubbles"])                            # the context works on afterwards
    check_against(res, g["restated"])


@pytest.mark.gpu
def test_switches(ctx):
    g = golden("polish_a")
    want = g["restated"]
    res = device(ctx, g["matrix"], g["bubbles"], want_steps=False)
    assert res.steps is None
    check_against(res, want, steps=False)
    # without the fixer: the restatement without it; the bubbles the fixer changed differ, and only those
    for name in ("polish_a", "polish_d"):
        g = golden(name)
        plain = [R.polish_bubble(b.cand, b.branches, g["s"], fix=False) for b in g["bubbles"]]
        res = device(ctx, g["matrix"], g["bubbles"], fix_dinucleotides=False)
        check_against(res, plain)
        changed = [i for i, r in enumerate(g["restated"]) if r[2] & R.FIXED]
        assert changed and [i for i in range(len(plain)) if plain[i] != g["restated"][i]] == changed


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [11, 12, 13, 14])
def test_fuzz(ctx, seed):
    matrix = MATRICES[seed % 2]
    s = R.load_matrix(os.path.join(CFG, matrix))
    bubbles = R.generate(seed, 40, cand_len=(1, 40), n_branches=(2, 24), rate=0.1 + 0.05 * (seed % 3))
    want = [R.polish_bubble(b.cand, b.branches, s) for b in bubbles]
    check_against(device(ctx, matrix, bubbles), want)


@pytest.mark.gpu
def test_offsets_need_not_start_at_zero(ctx):
    """a window into larger arrays: the call reads only what the offsets name"""
    g = golden("polish_b")
    cand, cand_off, br, br_off, bb_off = R.flatten(g["bubbles"])
    from flye_amd import gpu
    m = gpu.SubstitutionMatrix(os.path.join(CFG, g["matrix"]))
    res = ctx.polish_bubbles(m, cand, cand_off[5:21], br, br_off, bb_off[5:21])
    check_against(res, g["restated"][5:20])


@pytest.mark.gpu
def test_empty_batch_and_group_member(ctx):
    from flye_amd import gpu
    m = gpu.SubstitutionMatrix(os.path.join(CFG, "tie.mat"))
    res = ctx.polish_bubbles(m, b"", [0], b"", [0], [0])
    assert res.candidates == [] and len(res.n_steps) == 0 and res.steps == []
    lib = gpu.load_library()
    b = gpu.PolishBatch()
    assert lib.fg_polish_bubbles(ctx.h, C.byref(m.c), None, None, None, None, None, 0, 1, 1, C.byref(b)) == 0
    assert b.n_bubbles == 0 and b.cand_off[0] == 0 and b.step_off[0] == 0 and b.step_seq_off[0] == 0
    lib.fg_release_polish(C.byref(b))
    g = gpu.Group([0, 0])
    try:
        gold = golden("polish_c")
        check_against(device(g.member(1), m, gold["bubbles"]), gold["restated"])
    finally:
        g.close()


@pytest.mark.gpu
def test_argument_errors(ctx):
    from flye_amd import gpu
    lib = gpu.load_library()
    m = gpu.SubstitutionMatrix(os.path.join(CFG, "tie.mat"))
    bubbles = golden("polish_c")["bubbles"]
    cand, cand_off, br, br_off, bb_off = R.flatten(bubbles)
    n = len(bubbles)
    cb, bb = np.frombuffer(cand, np.uint8).copy(), np.frombuffer(br, np.uint8).copy()

    def call(matrix=m, cand=cb, cand_off=cand_off, br=bb, br_off=br_off, bb_off=bb_off, n=n, out=True):
        b = gpu.PolishBatch()
        ptr = [None if a is None else a.ctypes.data for a in (cand, cand_off, br, br_off, bb_off)]
        rc = lib.fg_polish_bubbles(ctx.h, C.byref(matrix.c) if matrix is not None else None, *ptr, n, 1, 1,
                                   C.byref(b) if out else None)
        if rc == 0:
            lib.fg_release_polish(C.byref(b))
        return rc

    assert call() == 0
    assert call(matrix=None) == -3 and call(out=False) == -3
    for name in ("cand", "cand_off", "br", "br_off", "bb_off"):
        assert call(**{name: None}) == -3, name
    for name, arr in (("cand_off", cand_off), ("br_off", br_off), ("bb_off", bb_off)):
        bad = arr.copy()
        bad[1], bad[2] = arr[2], arr[1]
        assert bad[2] < bad[1]
        assert call(**{name: bad}) == -3, name
    for arr, name in ((cb, "cand"), (bb, "br")):
        for byte in (128, 255):
            bad = arr.copy()
            bad[len(bad) // 2] = byte
            assert call(**{name: bad}) == -3, (name, byte)
        ok = arr.copy()
        ok[len(ok) // 2] = 127
        assert call(**{name: ok}) == 0
    assert call() == 0                                              # the context is usable after the errors
