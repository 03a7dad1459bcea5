"""fg_align_ranges: the ksw2 alignment of checkIdyAndTrim's first half (alignment.cpp:306-321) for ranges of the reads
that are resident on the device -- cut out of the 2-bit words, homopolymer-compressed, aligned and decoded there.

The oracle of every device test is Context.align_cigar_ksw (pinned to the reference by tests/golden/ksw_pairs.json and
consensus_pairs.json) on strings cut and compressed in numpy from the same reads: run offsets, ops, lens and the
err_rate bit patterns must be equal, and the returned lengths must be numpy's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from helpers import golden_reads, hpc, repeat_stage_setup
from ksw_craft import band as ksw_band

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_align_ranges_is_exported_and_declared(built):
    from flye_amd import gpu
    lib = gpu.load_library()
    assert hasattr(lib, "fg_align_ranges")
    assert "fg_align_ranges" in gpu.ABI_SYMBOLS
    text = open(os.path.join(ROOT, "include", "flye_gpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+fg_align_ranges\s*\(\s*fg_ctx\s*\*", text)
    assert re.search(r"struct\s+fg_range_pair\s*\{\s*uint32_t\s+cur_id\s*,\s*ext_id\s*;\s*int32_t\s+cur_begin\s*,\s*cur_end\s*,"
                     r"\s*ext_begin\s*,\s*ext_end\s*;\s*\}", text)
    assert re.search(r"#define\s+FG_ABI_VERSION\s+4\b", text)
    assert lib.fg_abi_version() == 4
    assert lib.fg_align_ranges(None, None, 0, 0, None, None, None) == -3


# ---- numpy side -------------------------------------------------------------------------------------------------------
def read_bases(rs, i):
    w = rs.words[int(rs.word_off[i]):int(rs.word_off[i + 1])]
    sh = np.arange(32, dtype=np.uint64) * np.uint64(2)
    return ((w[:, None] >> sh[None, :]) & np.uint64(3)).reshape(-1)[:int(rs.length[i])].astype(np.uint8)


class Strands:
    """The sequences of a container by FastaRecord id (odd = reverse complement), decoded once."""

    def __init__(self, rs, first_id):
        self.first = first_id
        self.fwd = [read_bases(rs, i) for i in range(rs.n)]
        self.rev = [None] * rs.n

    def seq(self, seq_id):
        i, rc = (int(seq_id) - self.first) >> 1, (int(seq_id) - self.first) & 1
        if not rc:
            return self.fwd[i]
        if self.rev[i] is None:
            self.rev[i] = (3 - self.fwd[i])[::-1].copy()
        return self.rev[i]


def cut_pairs(cur, ext, pairs, use_hpc):
    """(target, query) strings of fg_range_pair rows: target = the cur range, query = the ext range."""
    out = []
    for cid, eid, cb, ce, eb, ee in pairs:
        t, q = cur.seq(cid)[cb:ce], ext.seq(eid)[eb:ee]
        out.append((hpc(t), hpc(q)) if use_hpc else (t, q))
    return out


def check_against_oracle(ctx, pairs, strings, use_hpc, oracle=None):
    """align_ranges on `pairs` == align_cigar_ksw on `strings`, field for field; lengths == numpy's."""
    want = oracle if oracle is not None else ctx.align_cigar_ksw(strings, arrays=True)
    (run_off, ops, lens, bits), len_cur, len_ext = ctx.align_ranges(pairs, use_hpc=use_hpc, arrays=True)
    assert np.array_equal(len_cur, [len(t) for t, _ in strings])
    assert np.array_equal(len_ext, [len(q) for _, q in strings])
    assert np.array_equal(run_off, want[0])
    assert np.array_equal(bits, want[3])
    assert np.array_equal(ops, want[1])
    assert np.array_equal(lens, want[2])
    return want


# ---- 1. crafted reads -------------------------------------------------------------------------------------------------
def crafted():
    """Reads of 300..600 bases and the pair table of test 1 (ids from 0).
    read 0: random, with homopolymer runs planted at [28, 37) (crosses the 32-base word boundary), [60, 70) (crosses
            the 64-base step boundary of a range that begins at 0) and [100, 250) (longer than 64: the step [128, 192)
            of a range from 0 keeps nothing)
    read 1: read 0 with substitutions and small indels      read 2: a copy of read 0
    read 3: read 0 with 40 bases inserted at 400            read 4: read 0 with 120 bases inserted at 400
    read 5 / 6: "ACAC.." / "GTGT.." over the first 70 bases, then the same random bases"""
    rng = np.random.default_rng(20261018)
    r0 = rng.integers(0, 4, size=600, dtype=np.uint8)
    # neighbours of the planted runs differ from them, so that the runs are exactly these
    for a, b in ((28, 37), (60, 70), (100, 250)):
        r0[a:b] = r0[a]
        r0[a - 1] = (r0[a] + 1) & 3
        r0[b] = (r0[a] + 2) & 3
    r1 = []
    for i, x in enumerate(r0):
        u = rng.random()
        if u < 0.02:
            r1.append((x + 1 + rng.integers(0, 3)) & 3)
        elif u < 0.03:
            r1 += [x, rng.integers(0, 4)]
        elif u >= 0.04:
            r1.append(x)
    r1 = np.array(r1, np.uint8)
    r3 = np.concatenate([r0[:400], rng.integers(0, 4, size=40, dtype=np.uint8), r0[400:]])[:600]
    r4 = np.concatenate([r0[:400], rng.integers(0, 4, size=120, dtype=np.uint8), r0[400:]])[:600]
    body = rng.integers(0, 4, size=300, dtype=np.uint8)
    r5 = np.concatenate([np.tile(np.array([0, 1], np.uint8), 35), body])
    r6 = np.concatenate([np.tile(np.array([2, 3], np.uint8), 35), body])
    reads = [r0, r1, r0.copy(), r3, r4, r5, r6]
    L = [len(r) for r in reads]
    assert all(300 <= n <= 600 for n in L)
    P = []
    # lengths x begins on the 32-base word and 64-base step edges; the ext side a little longer or shorter
    for n in (0, 1, 2, 63, 64, 65, 127, 128, 129):
        for b in (0, 31, 32, 33):
            P.append((0, 2, b, b + n, b, min(b + n + (n % 3), L[1])))
    P.append((0, 2, 0, 0, 10, 15))                          # empty target, query of 5
    P.append((0, 2, 10, 15, 7, 7))                          # target of 5, empty query
    P.append((0, 2, L[0] - 129, L[0], L[1] - 131, L[1]))    # ranges ending on the reads' last base
    P.append((1, 3, 0, L[0], 0, L[1]))                      # whole reads, both reverse complements
    for n, b in ((65, 31), (129, 33), (200, 0)):
        P.append((1, 2, b, b + n, b, b + n))                # odd id on the cur side
        P.append((0, 3, b, b + n, b, b + n))                # ... on the ext side
        P.append((1, 3, b, b + n, b + 1, b + n))            # ... on both
    P.append((1, 3, L[0] - 64, L[0], L[1] - 64, L[1]))      # the last bases of a reverse strand = the read's first
    P.append((0, 2, 1, 91, 1, 91))                          # runs across the word and (at 65) the step boundary
    P.append((0, 2, 0, 300, 0, 300))                        # a step that keeps nothing
    P.append((0, 4, 110, 200, 110, 200))                    # one single run: compressed length 1
    P.append((0, 4, 105, 260, 104, 260))                    # first base equals the base in front of the range
    P.append((0, 6, 300, 560, 300, 600))                    # 40-base insertion
    P.append((0, 8, 300, 480, 300, 600))                    # 120-base insertion: lengths 180 / 300
    P.append((0, 4, 250, 600, 250, 600))                    # identical strings
    P.append((4, 4, 0, 333, 0, 333))                        # the same range of one record on both sides
    P.append((10, 12, 0, L[5], 0, L[6]))                    # no base in common in the first 70 columns
    return reads, np.array(P, np.int64)


@pytest.fixture(scope="module")
def crafted_ctx(built):
    from flye_amd import gpu, synth
    reads, pairs = crafted()
    rs = synth.ReadSet.from_arrays(reads)
    ctx = gpu.Context(17, 0)
    ctx.set_reads(rs, 0)
    return ctx, Strands(rs, 0), pairs


@pytest.mark.gpu
@pytest.mark.parametrize("use_hpc", [False, True])
def test_crafted_ranges(crafted_ctx, use_hpc):
    """Word / step edges, strands, homopolymer runs across the edges, the band classes, an 'X' run across a step: one
    batch, HPC off and on.

    A 40-base insertion alone does not make ksw_extz2 refuse band 64 (it gives up only when the lengths are more than
    the band apart), so next to that pair the batch holds one with 120 bases inserted: its band is 128, compressed or not."""
    ctx, st, pairs = crafted_ctx
    strings = cut_pairs(st, st, pairs, use_hpc)
    want = check_against_oracle(ctx, pairs, strings, use_hpc)
    kt = ctx.kernel_times()
    assert "k_range_extract" in kt and "k_ksw_decode" in kt
    assert ("k_range_lengths" in kt) == use_hpc
    # the cases are what they claim to be
    bands = {ksw_band(len(t), len(q)) for t, q in strings}
    assert {0, 64, 128} <= bands
    run_off, ops, lens, _ = want
    if use_hpc:
        lt = [len(t) for t, _ in strings]
        assert 1 in lt and min(len(t) for (t, _), p in zip(strings, pairs) if p[3] - p[2] == 300) < 300 - 140
    else:
        a, b = int(run_off[-2]), int(run_off[-1])                   # the last pair: 70 columns without a common base
        assert chr(ops[a]) == "X" and lens[a] >= 65
        ident = [i for i, (t, q) in enumerate(strings) if len(t) > 300 and np.array_equal(t, q)]
        assert ident and all(run_off[i + 1] - run_off[i] == 1 for i in ident)


@pytest.mark.gpu
def test_ksw_call_unchanged_around_align_ranges(crafted_ctx):
    """The existing call on one context before and after the new one: same bytes."""
    ctx, st, pairs = crafted_ctx
    strings = cut_pairs(st, st, pairs, False)
    before = ctx.align_cigar_ksw(strings, arrays=True)
    text = ctx.align_cigar_ksw(strings[-3:])
    ctx.align_ranges(pairs, use_hpc=True)
    after = ctx.align_cigar_ksw(strings, arrays=True)
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    assert text == ctx.align_cigar_ksw(strings[-3:])
    assert ctx.align_ranges(pairs[-3:], use_hpc=False)[0] == text       # the text form of both calls


@pytest.mark.gpu
def test_argument_errors(crafted_ctx):
    """Each bad argument: its code, a text in fg_last_error, and a context that still works."""
    from flye_amd import gpu
    ctx, st, pairs = crafted_ctx
    L = ctx.L
    n_ids = 2 * ctx.n_reads
    good = (0, 2, 0, 100, 0, 100)
    bad = [(n_ids, 2, 0, 10, 0, 10), (0, n_ids, 0, 10, 0, 10), (0, 2, -1, 10, 0, 10), (0, 2, 0, 10, -1, 10),
           (0, 2, 11, 10, 0, 10), (0, 2, 0, 10, 11, 10), (0, 2, 0, len(st.seq(0)) + 1, 0, 10),
           (0, 2, 0, 10, 0, len(st.seq(2)) + 1)]
    for row in bad:
        with pytest.raises(gpu.FlyeGpuError) as e:
            ctx.align_ranges(np.array([good, row], np.int64))
        assert e.value.code == -3 and "fg_align_ranges" in str(e.value)
    tab = np.zeros(1, gpu.RANGE_PAIR_DTYPE)
    tab[0] = good
    b = gpu.CigarBatch()
    assert L.fg_align_ranges(ctx.h, None, 1, 0, C.byref(b), None, None) == -3
    assert L.fg_last_error(ctx.h)
    assert L.fg_align_ranges(ctx.h, tab.ctypes.data, 1, 0, None, None, None) == -3
    assert L.fg_last_error(ctx.h)
    # no pairs: an empty batch, lengths may be NULL
    assert L.fg_align_ranges(ctx.h, None, 0, 0, C.byref(b), None, None) == 0
    assert b.n_pairs == 0 and b.run_off[0] == 0
    L.fg_release_cigars(C.byref(b))
    empty = gpu.Context(17, 0)
    with pytest.raises(gpu.FlyeGpuError) as e:
        empty.align_ranges(np.array([good], np.int64))
    assert e.value.code == -4 and "reads" in str(e.value)
    # still usable
    strings = cut_pairs(st, st, pairs, True)
    check_against_oracle(ctx, pairs, strings, True)


# ---- 2., 3. the records of a golden overlap case ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def repeat_records(built, golden_cases):
    """repeat_raw_all: index, fg_overlaps with nucl_alignment (use_hpc off and on), every record's strings and the
    oracle's alignment of them, computed once."""
    from flye_amd import config, gpu
    case = golden_cases["repeat_raw_all"]
    seqs = golden_reads(case)
    cfg = config.preset(case["preset"])
    wnd, dk = repeat_stage_setup(case, cfg)
    assert dk["nucl_alignment"] and dk["max_divergence"] == 1.0
    ctx = gpu.Context(int(cfg["kmer_size"]), 0)
    ctx.set_reads(seqs, 0)
    vi = gpu.VertexIndex(ctx, float(int(cfg["assemble_kmer_sample"])))
    vi.buildIndexMinimizers(1, wnd, cfg["repeat_kmer_rate"])
    st = Strands(seqs, 0)
    q = np.arange(0, 2 * seqs.n, 2, dtype=np.uint32)
    out = {}
    for use_hpc in (False, True):
        det = gpu.OverlapDetector(ctx, vi, int(cfg["maximum_jump"]), dk["min_overlap"], dk["max_overhang"], True,
                                  dk["only_max_ext"], dk["max_divergence"], True, True, use_hpc)
        recs = det.getSeqOverlapsBatch(q).recs.copy()
        pairs = np.stack([recs[f].astype(np.int64) for f in gpu.RANGE_PAIR_DTYPE.names], axis=1)
        strings = cut_pairs(st, st, pairs, use_hpc)
        out[use_hpc] = (recs, pairs, strings, ctx.align_cigar_ksw(strings, arrays=True))
    return ctx, seqs, out


@pytest.mark.gpu
@pytest.mark.parametrize("use_hpc", [False, True])
def test_golden_records(repeat_records, use_hpc):
    """Every record fg_overlaps returns for repeat_raw_all (17 reads, 1054 records), as the record array itself."""
    ctx, seqs, out = repeat_records
    recs, pairs, strings, want = out[use_hpc]
    assert seqs.n == 17 and len(recs) == 1054
    (run_off, ops, lens, bits), len_cur, len_ext = ctx.align_ranges(recs, use_hpc=use_hpc, arrays=True)
    # what the edit-distance step of fg_overlaps measured on the same ranges
    assert np.array_equal(len_cur, recs["hpc_len_cur"]) and np.array_equal(len_ext, recs["hpc_len_ext"])
    assert np.array_equal(len_cur, [len(t) for t, _ in strings]) and np.array_equal(len_ext, [len(x) for _, x in strings])
    assert np.array_equal(run_off, want[0]) and np.array_equal(bits, want[3])
    assert np.array_equal(ops, want[1]) and np.array_equal(lens, want[2])
    assert len({ksw_band(len(t), len(x)) for t, x in strings} - {0}) > 1        # more than one band class
    kt = ctx.kernel_times()
    assert kt["k_ksw_extz2_reg"][1] > 1 and "k_ksw_extz2_lds" not in kt
    print({k: round(v[0] * 1e3, 3) for k, v in kt.items()})


@pytest.mark.gpu
@pytest.mark.parametrize("use_hpc", [False, True])
def test_cur_side_in_its_own_container(repeat_records, use_hpc):
    """The same sequences once more as an fg_set_queries container under other ids: cur ids name that container, ext
    ids the indexed one; same result."""
    from flye_amd import gpu
    _, seqs, out = repeat_records
    _, pairs, strings, want = out[use_hpc]
    first = 2 * seqs.n + 4
    ctx = gpu.Context(17, 0)
    ctx.set_reads(seqs, 0)
    ctx.set_queries(seqs, first)
    moved = pairs.copy()
    moved[:, 0] += first
    check_against_oracle(ctx, moved, strings, use_hpc, oracle=want)
    # with a query container set, a cur id of the indexed container is unknown
    with pytest.raises(gpu.FlyeGpuError) as e:
        ctx.align_ranges(pairs[:1])
    assert e.value.code == -3
