"""fg_edit_ranges: getAlignmentErrEdlib (alignment.cpp:218-247) for (id, begin, end) ranges of the sequences that are
resident on the device, and fg_chain_divergence: ReadAligner::getChainBaseDivergence (read_aligner.cpp:410-434) from
the per-alignment values.

The expected distances come from oracle.edit_distance (pinned to the reference's edlib by tests/golden/edlib_pairs.json)
on strings cut with numpy from the same ReadSet; reverse complement and homopolymer compression are applied here in
Python.  Lengths are numpy's, the divergence is float32(dist) / float32(max(lengths)) compared as bit patterns."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from edit_craft import ED_BIG_MIN, ED_EMAX        # mirrored from fg_editdist.hip
from helpers import GOLDEN, golden_lines, golden_queries, golden_reads, hpc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- without a GPU ----------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_declared(built):
    from flye_amd import gpu
    lib = gpu.load_library()
    text = open(os.path.join(ROOT, "include", "flye_gpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym in ("fg_edit_ranges", "fg_chain_divergence"):
        assert hasattr(lib, sym)
        assert sym in gpu.ABI_SYMBOLS
    assert re.search(r"\bint\s+fg_edit_ranges\s*\(\s*fg_ctx\s*\*\s*\w+\s*,\s*const\s+struct\s+fg_range_pair\s*\*\s*\w+\s*,"
                     r"\s*uint32_t\s+\w+\s*,\s*uint8_t\s+\w+\s*,\s*int32_t\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*,"
                     r"\s*int32_t\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*\)", text)
    assert re.search(r"\bint\s+fg_chain_divergence\s*\(\s*const\s+int32_t\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*\w+\s*,"
                     r"\s*const\s+uint64_t\s*\*\s*\w+\s*,\s*uint32_t\s+\w+\s*,\s*float\s*\*\s*\w+\s*\)", text)
    assert re.search(r"#define\s+FG_ABI_VERSION\s+4\b", text)
    assert lib.fg_abi_version() == 4
    assert lib.fg_edit_ranges(None, None, 0, 0, None, None, None, None) == -3


def chain_restate(cur_range, divergence):
    """read_aligner.cpp:428-431 on numpy.float32 scalars: every operation rounds to single precision."""
    one = np.float32(1)
    s, ln = np.float32(0), 0
    for r, d in zip(cur_range, divergence):
        s = s + np.float32(int(r)) * (one - np.float32(d))
        assert s.dtype == np.float32
        ln += int(r)
    with np.errstate(divide="ignore", invalid="ignore"):
        return one - s / np.float32(ln)


def exactly_f32(x):
    """A Fraction rounded to the nearest float32 (ties to even), through exact arithmetic only."""
    if x == 0:
        return np.float32(0)
    e = math.floor(math.log2(abs(x)))
    while Fraction(2) ** e > abs(x):
        e -= 1
    while Fraction(2) ** (e + 1) <= abs(x):
        e += 1
    ulp = Fraction(2) ** (e - 23)
    q = x / ulp
    n = math.floor(q)
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
        n += 1
    return np.float32(float(n * ulp))


def fma_sensitive_chain(rng):
    """A two-entry chain whose second step gives other bits when the multiply-add is fused (one rounding of the exact
    r * (1 - d) + sum) than with the product rounded first, found by search."""
    one = np.float32(1)
    for _ in range(200000):
        r1, r2 = int(rng.integers(500, 30000)), int(rng.integers(500, 30000))
        d1, d2 = np.float32(rng.random() * 0.2), np.float32(rng.random() * 0.2)
        s1 = np.float32(r1) * (one - d1)
        keep2 = one - d2
        two = s1 + np.float32(r2) * keep2
        fused = exactly_f32(Fraction(float(r2)) * Fraction(float(keep2)) + Fraction(float(s1)))
        if two.view(np.uint32) != fused.view(np.uint32):
            # ... and the chain's value differs too, not only the running sum
            ln = np.float32(r1 + r2)
            if (one - two / ln).view(np.uint32) != (one - fused / ln).view(np.uint32):
                return [r1, r2], [d1, d2], one - fused / ln
    return None


def test_chain_divergence_equals_float32_restatement(built):
    """fg_chain_divergence against chain_restate, bit for bit.  No program of the reference prints a chain's
    divergence (getChainBaseDivergence only feeds a comparison inside alignReads), so the yardstick is the restatement
    of its three lines in numpy.float32, whose scalars round every operation on its own as the reference's build
    (plain -O3, no -march: no fused multiply-add) does."""
    from flye_amd import gpu
    rng = np.random.default_rng(410434)
    chains = []
    for _ in range(10000):
        n = int(rng.integers(1, 13))
        chains.append((rng.integers(1, 40000, size=n).astype(np.int32), (rng.random(n) * rng.choice([0.01, 0.2, 1.0])).astype(np.float32)))
    found = fma_sensitive_chain(rng)
    assert found is not None, "no chain found on which a fused multiply-add shows"
    chains.append((np.array(found[0], np.int32), np.array(found[1], np.float32)))
    i_fma = len(chains) - 1
    chains.append((np.array([1234], np.int32), np.array([0.0625], np.float32)))         # a single entry
    chains.append((np.empty(0, np.int32), np.empty(0, np.float32)))                    # empty: 0 / 0
    chains.append((np.zeros(3, np.int32), np.array([0.1, 0.2, 0.3], np.float32)))      # total length 0
    off = np.zeros(len(chains) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r, _ in chains])
    cr = np.concatenate([r for r, _ in chains])
    dv = np.concatenate([d for _, d in chains])
    got = gpu.chain_divergence(cr, dv, off)
    want = np.array([chain_restate(r, d) for r, d in chains], np.float32)
    assert got.dtype == np.float32 and len(got) == len(chains)
    nan = np.isnan(want)                # a NaN's sign and payload carry nothing: NaN where the restatement has one
    assert np.array_equal(np.isnan(got), nan) and nan.sum() == 2
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    assert got[i_fma].view(np.uint32) != np.float32(found[2]).view(np.uint32)          # not the fused value
    assert got[-3] == np.float32(1) - np.float32(1234) * (np.float32(1) - np.float32(0.0625)) / np.float32(1234)
    assert np.isnan(got[-2]) and np.isnan(got[-1])
    assert not np.isnan(got[:-2]).any()
    # argument errors
    L = gpu.load_library()
    out = np.zeros(2, np.float32)
    ok_off = np.array([0, 1, 2], np.uint64)
    assert L.fg_chain_divergence(None, None, None, 0, None) == 0
    assert L.fg_chain_divergence(cr.ctypes.data, dv.ctypes.data, ok_off.ctypes.data, 2, out.ctypes.data) == 0
    assert L.fg_chain_divergence(None, dv.ctypes.data, ok_off.ctypes.data, 2, out.ctypes.data) == -3
    assert L.fg_chain_divergence(cr.ctypes.data, None, ok_off.ctypes.data, 2, out.ctypes.data) == -3
    assert L.fg_chain_divergence(cr.ctypes.data, dv.ctypes.data, None, 2, out.ctypes.data) == -3
    assert L.fg_chain_divergence(cr.ctypes.data, dv.ctypes.data, ok_off.ctypes.data, 2, None) == -3
    bad_off = np.array([0, 2, 1], np.uint64)
    assert L.fg_chain_divergence(cr.ctypes.data, dv.ctypes.data, bad_off.ctypes.data, 2, out.ctypes.data) == -3


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
    out = []
    for cid, eid, cb, ce, eb, ee in pairs:
        a, b = cur.seq(cid)[cb:ce], ext.seq(eid)[eb:ee]
        out.append((hpc(a), hpc(b)) if use_hpc else (a, b))
    return out


def expected(strings):
    """(dist, len_cur, len_ext, divergence bits) of string pairs: the oracle's distance (max(n, m) for an empty side is
    what it returns too, edlib.cpp:160-164), the float as alignment.cpp:244 forms it."""
    from oracle import oracle as O
    d = np.array([O.edit_distance(a, b) for a, b in strings], np.int32)
    la = np.array([len(a) for a, _ in strings], np.int32)
    lb = np.array([len(b) for _, b in strings], np.int32)
    with np.errstate(divide="ignore", invalid="ignore"):
        div = d.astype(np.float32) / np.maximum(la, lb).astype(np.float32)
    return d, la, lb, div


def assert_same(got, want):
    """Distances, lengths and divergence bit patterns; NaN where and only where both strings are empty."""
    d, la, lb, div = got
    assert div.dtype == np.float32
    assert np.array_equal(la, want[1]) and np.array_equal(lb, want[2])
    assert np.array_equal(d, want[0])
    both_empty = (want[1] == 0) & (want[2] == 0)
    assert np.array_equal(np.isnan(div), both_empty)
    assert np.array_equal(div.view(np.uint32)[~both_empty], want[3].view(np.uint32)[~both_empty])


def with_env(monkeypatch, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


# ---- 1. crafted ranges ------------------------------------------------------------------------------------------------
def mutate(rng, x, rate):
    out = []
    for b in x:
        u = rng.random()
        if u < rate / 3:
            out.append((b + 1 + rng.integers(0, 3)) & 3)
        elif u < 2 * rate / 3:
            out += [b, rng.integers(0, 4)]
        elif u >= rate:
            out.append(b)
    return np.array(out, np.uint8)


def crafted():
    """Reads 0..7 of 1, 31, 32, 33, 64, 65, 200 and 5000 bases; reads 8 and 9: 50 000 bases, the second the first with
    2 % errors.  Read 6 holds one homopolymer run at [50, 120) with other bases on both sides of it.  Pairs by id
    (2 * read + strand); `big` = index of the 50 kb pair."""
    rng = np.random.default_rng(218247)
    reads = [rng.integers(0, 4, size=n, dtype=np.uint8) for n in (1, 31, 32, 33, 64, 65, 200, 5000)]
    r6 = reads[6]
    r6[50:120] = r6[50]
    r6[49] = (r6[50] + 1) & 3
    r6[120] = (r6[50] + 2) & 3
    a = rng.integers(0, 4, size=50000, dtype=np.uint8)
    b = mutate(rng, a, 0.02)
    b = np.concatenate([b, rng.integers(0, 4, size=max(0, 50000 - len(b)), dtype=np.uint8)])[:50000]
    reads += [a, b]
    assert [len(r) for r in reads] == [1, 31, 32, 33, 64, 65, 200, 5000, 50000, 50000]
    P = [(14, 12, 10, 10, 0, 200),          # cur empty
         (14, 12, 0, 100, 5, 5),            # ext empty
         (14, 12, 7, 7, 9, 9)]              # both empty: NaN
    # begins and ends on the 32-base word and 64-base chunk edges, the ext side a little longer
    for beg in (0, 31, 32, 33, 63, 64, 65):
        for end in (31, 32, 33, 63, 64, 65, 300):
            if end > beg:
                P.append((16, 18, beg, end, beg, end + end % 3))
    for i in range(7):                      # whole reads, the short ones against their neighbours
        P.append((2 * i, 2 * i + 2, 0, len(reads[i]), 0, len(reads[i + 1])))
    P.append((14, 14, 0, 5000, 0, 5000))    # a read against itself
    P.append((15, 15, 0, 5000, 0, 5000))
    for s1 in (0, 1):                       # the four strand combinations
        for s2 in (0, 1):
            P.append((16 + s1, 18 + s2, 1000, 3000, 1000, 3000))
    P.append((17, 19, 49936, 50000, 49937, 50000))      # the last bases of a reverse strand = the read's first
    P.append((12, 12, 60, 150, 40, 150))    # the first base equals the base before begin: kept under HPC
    P.append((12, 12, 55, 110, 60, 100))    # inside one homopolymer run: compressed length 1
    P.append((12, 14, 55, 110, 0, 100))
    P.append((14, 14, 0, 100, 0, 1000))     # lengths further apart than ED_EMAX
    P.append((16, 18, 0, 50000, 0, 50000))  # the 8-wave kernel
    return reads, np.array(P, np.int64), len(P) - 1


@pytest.fixture(scope="module")
def crafted_expected(built):
    """Reads, pairs and, per use_hpc, the strings and what the oracle says of them; computed once."""
    from flye_amd import synth
    reads, pairs, big = crafted()
    rs = synth.ReadSet.from_arrays(reads)
    st = Strands(rs, 0)
    assert all(np.array_equal(st.seq(2 * i), r) for i, r in enumerate(reads))
    want, strings = {}, {}
    for use_hpc in (False, True):
        strings[use_hpc] = cut_pairs(st, st, pairs, use_hpc)
        want[use_hpc] = expected(strings[use_hpc])
    # the cases are what they claim to be
    d, la, lb, _ = want[False]
    assert d[0] == 200 and d[1] == 100 and d[2] == 0
    assert max(la[big], lb[big]) > ED_BIG_MIN and (np.maximum(la, lb)[:big] <= ED_BIG_MIN).all()
    assert (abs(la - lb) > ED_EMAX).any()
    assert ((d == 0) & (la == 5000)).sum() == 2
    hd, hla, hlb, _ = want[True]
    assert ((hla == 1) & (hlb == 1) & (hd == 0)).any()
    i_kept = next(i for i, p in enumerate(pairs) if tuple(p) == (12, 12, 60, 150, 40, 150))
    assert reads[6][59] == reads[6][60] == strings[True][i_kept][0][0] != strings[True][i_kept][0][1]
    return rs, st, pairs, big, strings, want


@pytest.fixture(scope="module")
def crafted_ctx(crafted_expected):
    from flye_amd import gpu
    ctx = gpu.Context(17, 0)
    ctx.set_reads(crafted_expected[0], 0)
    return ctx


@pytest.mark.gpu
@pytest.mark.parametrize("use_hpc", [False, True])
def test_crafted_ranges(crafted_expected, crafted_ctx, use_hpc):
    """Empty sides, word and chunk edges, whole reads, strands, homopolymer edge cases, a pair beyond the O(ND) limit
    and one for the 8-wave kernel: all four outputs."""
    _, _, pairs, _, _, want = crafted_expected
    assert_same(crafted_ctx.edit_ranges(pairs, use_hpc=use_hpc), want[use_hpc])
    kt = crafted_ctx.kernel_times()
    assert {"k_edit_range_prims", "k_edit_range_collect", "k_edit_myers_wide"} <= set(kt)
    assert kt["k_edit_range_prims"][1] == 1 and kt["k_edit_range_collect"][1] == 1


# ---- 2. forced kernel paths -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("use_hpc", [False, True])
def test_forced_kernel_paths(crafted_expected, crafted_ctx, use_hpc, monkeypatch):
    """FG_ED_EMAX = 3 sends nearly every pair to the bit-vector kernel, FG_ED_LDS_BASES = 2048 the longer ones without
    an O(ND) attempt: same results."""
    _, _, pairs, big, _, want = crafted_expected
    with_env(monkeypatch, FG_ED_EMAX=3, FG_ED_LDS_BASES=2048)
    assert big == len(pairs) - 1
    assert_same(crafted_ctx.edit_ranges(pairs[:big], use_hpc=use_hpc), [w[:big] for w in want[use_hpc]])
    kt = crafted_ctx.kernel_times()
    assert "k_edit_myers" in kt and "k_edit_myers_wide" not in kt


# ---- 3. sub-batching --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sub_batches(crafted_expected, crafted_ctx, monkeypatch):
    """FG_EDIT_BATCH_PAIRS = 7: 23 pairs in 4 sub-batches (the last of 2), 7 in one, 8 in two (the last of 1), 14 in
    two full ones -- each equal to the unsplit call, kernel times summed over the sub-batches."""
    _, _, pairs, _, _, want = crafted_expected
    sel = np.r_[0:3, 25:45]                             # empty sides, edges, whole reads, self, strands
    assert len(sel) == 23
    whole = crafted_ctx.edit_ranges(pairs[sel], use_hpc=True)
    assert_same(whole, [w[sel] for w in want[True]])
    assert crafted_ctx.kernel_times()["k_edit_range_prims"][1] == 1
    with_env(monkeypatch, FG_EDIT_BATCH_PAIRS=7)
    for n in (23, 7, 8, 14):
        got = crafted_ctx.edit_ranges(pairs[sel[:n]], use_hpc=True)
        assert_same(got, [w[sel[:n]] for w in want[True]])
        assert all(np.array_equal(g.view(np.uint32), w[:n].view(np.uint32)) for g, w in zip(got, whole))
        kt = crafted_ctx.kernel_times()
        assert kt["k_edit_range_prims"][1] == kt["k_edit_range_collect"][1] == (n + 6) // 7


# ---- 4. the reference's own numbers -----------------------------------------------------------------------------------
def golden_records(name):
    """(pairs, divergence bit patterns) of the lines the compiled reference wrote for a golden case."""
    rows = [l.split() for l in golden_lines(name)]
    pairs = np.array([[int(f[0]), int(f[4]), int(f[1]), int(f[2]), int(f[5]), int(f[6])] for f in rows], np.int64)
    bits = np.array([int(f[9], 16) for f in rows], np.uint32)
    return pairs, bits


@pytest.mark.gpu
@pytest.mark.parametrize("name,n_records", [("repeat_raw_all", 1054), ("repeat_hifi", 89)])
def test_reference_divergences(built, golden_cases, name, n_records):
    """Every record the compiled reference wrote for the case with nuclAlignment on (its seqDivergence is
    getAlignmentErrEdlib's value, overlap.cpp:474-485 with partitionBadMappings off): the call's divergence has the same bits."""
    from flye_amd import config, gpu
    case = golden_cases[name]
    assert case["nucl_aln"]
    cfg = config.preset(case["preset"])
    seqs = golden_reads(case)
    pairs, bits = golden_records(name)
    assert len(pairs) == n_records == case["n_overlaps"]
    ctx = gpu.Context(int(cfg["kmer_size"]), 0)
    ctx.set_reads(seqs, 0)
    d, la, lb, div = ctx.edit_ranges(pairs, use_hpc=bool(cfg["hpc_scoring_on"]))
    assert np.array_equal(div.view(np.uint32), bits)
    assert (d > 0).any() and (la > 0).all() and (lb > 0).all()
    print({k: round(v[0] * 1e3, 3) for k, v in ctx.kernel_times().items()})


# ---- 5. cur side in its own container ---------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cur_side_in_its_own_container(built, golden_cases):
    """edges_hifi: reads (fg_set_queries) against edges (indexed); the coordinates of all the reference's records."""
    from flye_amd import config, gpu
    case = golden_cases["edges_hifi"]
    cfg = config.preset(case["preset"])
    edges, reads = golden_reads(case), golden_queries(case)
    first_q = 2 * edges.n
    pairs, _ = golden_records("edges_hifi")
    assert len(pairs) == case["n_overlaps"] and (pairs[:, 0] >= first_q).all() and (pairs[:, 1] < first_q).all()
    # the reference's records all have a forward cur id: the same overlaps seen from the other strands as well
    lc, le = reads.length[(pairs[:200, 0] - first_q) >> 1], edges.length[pairs[:200, 1] >> 1]
    mirrored = np.stack([pairs[:200, 0] ^ 1, pairs[:200, 1] ^ 1, lc - pairs[:200, 3], lc - pairs[:200, 2],
                         le - pairs[:200, 5], le - pairs[:200, 4]], axis=1)
    pairs = np.concatenate([pairs, mirrored])
    assert (pairs[:, 0] & 1).any() and (pairs[:, 1] & 1).any()
    ctx = gpu.Context(int(cfg["kmer_size"]), 0)
    ctx.set_reads(edges, 0)
    ctx.set_queries(reads, first_q)
    use_hpc = bool(cfg["hpc_scoring_on"])
    strings = cut_pairs(Strands(reads, first_q), Strands(edges, 0), pairs, use_hpc)
    assert_same(ctx.edit_ranges(pairs, use_hpc=use_hpc), expected(strings))
    # with a query container set, a cur id of the indexed container is unknown
    with pytest.raises(gpu.FlyeGpuError) as e:
        ctx.edit_ranges(np.array([(0, 0, 0, 10, 0, 10)], np.int64))
    assert e.value.code == -3 and "fg_edit_ranges" in str(e.value)


# ---- 6., 7. next to fg_overlaps ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hifi_ctx(built, golden_cases):
    from flye_amd import config, gpu
    case = golden_cases["hifi"]
    cfg = config.preset(case["preset"])
    seqs = golden_reads(case)
    ctx = gpu.Context(int(cfg["kmer_size"]), 0)
    ctx.set_reads(seqs, 0)
    vi = gpu.VertexIndex(ctx, float(int(cfg["assemble_kmer_sample"])))
    vi.build(cfg)
    use_hpc = bool(cfg["hpc_scoring_on"])
    det = gpu.OverlapDetector(ctx, vi, int(cfg["maximum_jump"]), 1000, int(cfg["maximum_overhang"]), False, True, 1.0,
                              True, False, use_hpc)
    return ctx, seqs, det, use_hpc


@pytest.mark.gpu
def test_same_answer_as_nucl_alignment(hifi_ctx):
    """Every record of the detector with nucl_alignment = 1: the call on its coordinates gives the record's
    edit_distance, hpc_len_cur, hpc_len_ext and seq_divergence."""
    ctx, seqs, det, use_hpc = hifi_ctx
    recs = det.getSeqOverlapsBatch(np.arange(0, 2 * seqs.n, 2, dtype=np.uint32)).recs.copy()
    assert len(recs) > 1000
    d, la, lb, div = ctx.edit_ranges(recs, use_hpc=use_hpc)
    assert np.array_equal(d, recs["edit_distance"])
    assert np.array_equal(la, recs["hpc_len_cur"]) and np.array_equal(lb, recs["hpc_len_ext"])
    assert np.array_equal(div.view(np.uint32), recs["seq_divergence"].view(np.uint32))


@pytest.mark.gpu
def test_arguments_and_state(hifi_ctx):
    """Each bad argument: its code, a text in fg_last_error, nothing launched; fg_overlaps before and after a call."""
    from flye_amd import gpu
    ctx, seqs, det, use_hpc = hifi_ctx
    L = ctx.L
    q = np.arange(0, 40, 2, dtype=np.uint32)
    before = det.getSeqOverlapsBatch(q)
    lines, recs = before.lines(), before.recs.copy()
    assert len(recs) > 100
    good = (0, 2, 0, 100, 0, 100)
    ctx.edit_ranges(np.array([good], np.int64))
    kt = ctx.kernel_times()
    assert "k_edit_range_prims" in kt
    n_ids = 2 * seqs.n
    len0, len1 = int(seqs.length[0]), int(seqs.length[1])
    bad = [(n_ids, 2, 0, 10, 0, 10), (0, n_ids, 0, 10, 0, 10), (0, 2, -1, 10, 0, 10), (0, 2, 0, 10, -1, 10),
           (0, 2, 11, 10, 0, 10), (0, 2, 0, 10, 11, 10), (0, 2, 0, len0 + 1, 0, 10), (0, 2, 0, 10, 0, len1 + 1)]
    for row in bad:
        with pytest.raises(gpu.FlyeGpuError) as e:
            ctx.edit_ranges(np.array([good, row], np.int64))
        assert e.value.code == -3 and "fg_edit_ranges" in str(e.value)
        assert ctx.kernel_times() == kt                 # the timer was neither reset nor collected: nothing ran
    tab = np.zeros(1, gpu.RANGE_PAIR_DTYPE)
    tab[0] = good
    dist = np.full(1, -7, np.int32)
    assert L.fg_edit_ranges(ctx.h, None, 1, 0, dist.ctypes.data, None, None, None) == -3
    assert L.fg_last_error(ctx.h)
    assert L.fg_edit_ranges(ctx.h, tab.ctypes.data, 1, 0, None, None, None, None) == -3
    assert L.fg_last_error(ctx.h)
    assert ctx.kernel_times() == kt and dist[0] == -7
    # no pairs: nothing to do, every pointer may be NULL
    assert L.fg_edit_ranges(ctx.h, None, 0, 0, None, None, None, None) == 0
    assert ctx.kernel_times() == kt
    # only the distances asked for, then only the divergence besides them
    assert L.fg_edit_ranges(ctx.h, tab.ctypes.data, 1, 0, dist.ctypes.data, None, None, None) == 0
    div = np.zeros(1, np.float32)
    d0 = int(dist[0])
    assert L.fg_edit_ranges(ctx.h, tab.ctypes.data, 1, 0, dist.ctypes.data, None, None, div.ctypes.data) == 0
    assert dist[0] == d0 >= 0 and div[0] == np.float32(d0) / np.float32(100)
    empty = gpu.Context(17, 0)
    with pytest.raises(gpu.FlyeGpuError) as e:
        empty.edit_ranges(np.array([good], np.int64))
    assert e.value.code == -4 and "reads" in str(e.value)
    # the overlap call is where it was
    ctx.edit_ranges(recs, use_hpc=use_hpc)
    after = det.getSeqOverlapsBatch(q)
    assert after.lines() == lines
    assert after.recs.tobytes() == recs.tobytes()


# ---- 8. live reference ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(os.path.join(os.path.dirname(GOLDEN), "..", "oracle", "_ref", "ref_dumper")),
                    reason="oracle/_ref/ref_dumper not built")
@pytest.mark.parametrize("use_hpc", [False, True])
def test_live_against_reference_edlib(crafted_expected, crafted_ctx, use_hpc):
    """The reference's own edlibAlign on the crafted strings against the device's distances."""
    from oracle import oracle as O
    _, _, pairs, _, strings, _ = crafted_expected
    d = crafted_ctx.edit_ranges(pairs, use_hpc=use_hpc)[0]
    assert O.ref_edlib_distances(strings[use_hpc]) == d.tolist()
