"""The three forms of the ksw_extz2 recurrence in fg_ksw.hip -- state in memory (k_ksw_extz2), in LDS rings
(k_ksw_extz2_lds, FG_KSW_REG=0), in a register window (k_ksw_extz2_reg, the default) -- on the crafted pairs of
tests/ksw_craft.py: every class edge of the dispatcher, ring wraps, stage flushes, look-ahead and tile edges, tie rules,
band-edge paths; batches that give a block a second job; one pair per scratch sub-batch; the range callers.

Everything is integer and bit-exact: CIGAR arrays and error-rate bit patterns are compared for equality.  The oracle
(O.ksw_cigar) is pinned on what the compiled reference returned for the same pairs (tests/golden/ksw_edge_pairs.json,
tests/golden/make_ksw_edge_golden.py)."""
import hashlib
import json
import os

import numpy as np
import pytest

import ksw_craft
from helpers import GOLDEN

KSW_KERNELS = ("k_ksw_extz2", "k_ksw_extz2_lds", "k_ksw_extz2_reg")
FORMS = {"reg": ({}, "k_ksw_extz2_reg"), "lds": ({"FG_KSW_REG": "0"}, "k_ksw_extz2_lds"),
         "literal": ({"FG_KSW_LITERAL": "1"}, None)}


@pytest.fixture(scope="module")
def crafted():
    return ksw_craft.cases()


@pytest.fixture(scope="module")
def fixture_rows():
    with open(os.path.join(GOLDEN, "ksw_edge_pairs.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def oracle_text(built, crafted):
    """O.ksw_cigar of every crafted case, computed once: [(error-rate bits as hex, CIGAR text)]."""
    from oracle import oracle as O
    return [O.ksw_cigar(t, q) for _, t, q in crafted]


def to_arrays(text):
    """The arrays fg_align_cigar_ksw returns for pairs whose results are ``text``: (run_off, ops, lens, bits)."""
    run_off = np.zeros(len(text) + 1, np.uint64)
    ops, lens = [], []
    for i, (_, cig) in enumerate(text):
        for run in cig.split():
            ops.append(ord(run[-1]))
            lens.append(int(run[:-1]))
        run_off[i + 1] = len(ops)
    return run_off, np.array(ops, np.uint8), np.array(lens, np.int32), np.array([int(b, 16) for b, _ in text], np.uint32)


def assert_arrays_equal(got, want):
    for g, w, field in zip(got, want, ("run_off", "ops", "lens", "err_rate bits")):
        assert g.dtype == w.dtype and np.array_equal(g, w), field


def assert_equals_fixture(got, rows, crafted):
    """(run_off, ops, lens, bits) against the reference's recorded results."""
    run_off, ops, lens, bits = got
    assert len(rows) == len(crafted) == len(bits)
    for i, ((name, tlen, qlen, err_bits, sha), (cname, t, q)) in enumerate(zip(rows, crafted)):
        assert (name, tlen, qlen) == (cname, len(t), len(q))
        assert f"{int(bits[i]):08x}" == err_bits, name
        a, b = int(run_off[i]), int(run_off[i + 1])
        cig = " ".join(f"{lens[k]}{chr(ops[k])}" for k in range(a, b))
        assert hashlib.sha256(cig.encode()).hexdigest() == sha, name


def ksw_launches(ctx):
    """{kernel: launches} of the ksw kernels in the last call."""
    return {k: v[1] for k, v in ctx.kernel_times().items() if k in KSW_KERNELS}


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_crafted_cases_are_what_they_claim(crafted):
    ksw_craft.assert_claims(crafted)


def test_class_batches_are_in_their_class():
    for c in range(5):
        batch = ksw_craft.class_batch(c)
        assert len(batch) == 61 and len({(t.tobytes(), q.tobytes()) for t, q in batch}) == 61
        assert all(ksw_craft.kernel_class(len(t), len(q)) == c for t, q in batch)
    # the largest batch of the second-job test stays in one scratch sub-batch: direction matrix + state per pair
    # (fg_ksw.hip, kswAlignDevice), 8192 + 256 pairs, under the default 8 GiB
    need = 0
    for k in range(8192 + 256):
        tlen, qlen = ksw_craft.class_lengths(4, k % 61)
        t16, q16 = (tlen + 15) // 16 * 16, (qlen + 15) // 16 * 16
        need += (qlen + tlen) * ksw_craft.row_bytes(tlen, qlen) + 64 + t16 * 6 + q16 + 64
    assert need < 8 << 30


def test_oracle_ksw_cigar_equals_reference_on_crafted_cases(crafted, fixture_rows, oracle_text):
    assert_equals_fixture(to_arrays(oracle_text), fixture_rows, crafted)
    # what the look-ahead and decode cases rely on
    by_name = {name: text for (name, _, _), text in zip(crafted, oracle_text)}
    for n in (64, 128, 129):
        assert by_name[f"ident/{n}"] == ("00000000", f"{n}=")
    assert by_name["look/sub/1500/p63"][1] == "63= 1X 1436="
    assert by_name["look/sub/1500/p64"][1] == "64= 1X 1435="


@pytest.mark.skipif(not os.path.exists(os.path.join(os.path.dirname(GOLDEN), "..", "oracle", "_ref", "ref_dumper")),
                    reason="oracle/_ref/ref_dumper not built")
def test_oracle_ksw_cigar_live_against_reference_on_crafted_cases(crafted, oracle_text):
    from oracle import oracle as O
    assert oracle_text == O.ref_ksw_cigars([(t, q) for _, t, q in crafted])


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(built):
    from flye_amd import gpu
    c = gpu.Context(17, 0)
    yield c
    c.close()


def set_form(monkeypatch, form):
    monkeypatch.delenv("FG_KSW_REG", raising=False)
    monkeypatch.delenv("FG_KSW_LITERAL", raising=False)
    monkeypatch.delenv("FG_KSW_DEBUG", raising=False)
    for k, v in FORMS[form][0].items():
        monkeypatch.setenv(k, v)
    return FORMS[form][1]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["reg", "lds", "literal"])
def test_three_forms_one_truth(ctx, monkeypatch, crafted, fixture_rows, oracle_text, form):
    """Every crafted case through each form: equal to the oracle field for field and to the reference's recorded
    results; the kernels that ran are the form's, the windowed one launched once per class."""
    windowed = set_form(monkeypatch, form)
    monkeypatch.delenv("FG_KSW_SCRATCH_BYTES", raising=False)
    got = ctx.align_cigar_ksw([(t, q) for _, t, q in crafted], arrays=True)
    launches = ksw_launches(ctx)
    assert_arrays_equal(got, to_arrays(oracle_text))
    assert_equals_fixture(got, fixture_rows, crafted)
    assert launches == ({"k_ksw_extz2": 1, windowed: 4} if windowed else {"k_ksw_extz2": 1})


@pytest.mark.gpu
@pytest.mark.parametrize("form,cls", [("reg", 0), ("reg", 1), ("reg", 2), ("reg", 3), ("reg", 4), ("lds", 1), ("lds", 4)])
def test_second_job_on_a_block(ctx, monkeypatch, form, cls):
    """8192 + 256 pairs of one class: the kernels run min(count, 8192) blocks that stride over the jobs, so 256 blocks
    take a second job after their first -- the rings, the window and the tile are set up again behind a finished walk.
    61 distinct pairs tiled (61 is coprime to 8192: a block's two jobs differ), against the oracle on the 61."""
    from oracle import oracle as O
    windowed = set_form(monkeypatch, form)
    monkeypatch.delenv("FG_KSW_SCRATCH_BYTES", raising=False)
    base = ksw_craft.class_batch(cls)
    n = 8192 + 256
    pairs = [base[i % 61] for i in range(n)]
    assert not np.array_equal(pairs[0][0], pairs[8192][0])
    text = [O.ksw_cigar(t, q) for t, q in base]
    got = ctx.align_cigar_ksw(pairs, arrays=True)
    launches = ksw_launches(ctx)
    assert_arrays_equal(got, to_arrays([text[i % 61] for i in range(n)]))
    assert launches == {("k_ksw_extz2" if cls == 0 else windowed): 1}        # one class, no sub-batch split


@pytest.mark.gpu
def test_one_pair_per_scratch_sub_batch(ctx, monkeypatch, crafted, oracle_text):
    """A scratch budget below any pair's need: every pair is its own sub-batch, the run list and its counter are
    reused 60 times."""
    set_form(monkeypatch, "reg")
    cls_of = [ksw_craft.kernel_class(len(t), len(q)) for _, t, q in crafted]
    pick = []
    for c in range(5):                  # twelve of every class, spread over the class's cases
        mine = [i for i, x in enumerate(cls_of) if x == c]
        pick += mine[::len(mine) // 12][:12]
    pick.sort()
    classes = [cls_of[i] for i in pick]
    assert len(pick) == 60 and set(classes) == {0, 1, 2, 3, 4}
    monkeypatch.setenv("FG_KSW_SCRATCH_BYTES", "1")
    got = ctx.align_cigar_ksw([crafted[i][1:] for i in pick], arrays=True)
    launches = ksw_launches(ctx)
    assert_arrays_equal(got, to_arrays([oracle_text[i] for i in pick]))
    assert launches == {"k_ksw_extz2": classes.count(0), "k_ksw_extz2_reg": 60 - classes.count(0)}


@pytest.mark.gpu
def test_range_callers_on_crafted_cases(built, monkeypatch, crafted, oracle_text):
    """The class-edge, ring-wrap and look-ahead cases as resident reads through fg_align_ranges (whole-read ranges, HPC
    off): equal to fg_align_cigar_ksw on the same strings -- k_ksw_decode on M runs of exactly 64, 128 and 129 columns
    and on a mismatch in column 63 and in column 64 of a step."""
    from flye_amd import gpu, synth
    set_form(monkeypatch, "reg")
    monkeypatch.delenv("FG_KSW_SCRATCH_BYTES", raising=False)
    pick = [i for i, (name, _, _) in enumerate(crafted) if name.split("/")[0] in ("edge", "ring", "ident", "look")]
    strings = [crafted[i][1:] for i in pick]
    reads = [s for pair in strings for s in pair]
    c = gpu.Context(17, 0)
    c.set_reads(synth.ReadSet.from_arrays(reads), 0)
    table = np.array([(4 * k, 4 * k + 2, 0, len(t), 0, len(q)) for k, (t, q) in enumerate(strings)], np.int64)
    want = c.align_cigar_ksw(strings, arrays=True)
    assert_arrays_equal(want, to_arrays([oracle_text[i] for i in pick]))
    (run_off, ops, lens, bits), len_cur, len_ext = c.align_ranges(table, use_hpc=False, arrays=True)
    kt = c.kernel_times()
    c.close()
    assert np.array_equal(len_cur, [len(t) for t, _ in strings]) and np.array_equal(len_ext, [len(q) for _, q in strings])
    assert_arrays_equal((run_off, ops, lens, bits), want)
    assert {"k_range_extract", "k_ksw_decode", "k_ksw_extz2", "k_ksw_extz2_reg"} <= set(kt)
    assert kt["k_ksw_extz2_reg"][1] == 4
