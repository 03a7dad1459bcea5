"""fg_trim_ranges: checkIdyAndTrim (alignment.cpp:306-495) on the device -- the alignment of fg_align_ranges, then the
interval search, std::sort, greedy selection, offset-table mapping and minOverlap filter on the runs where they are.

The yardstick is a restatement of :330-457 in this file (numpy prefix sums, the oracle's std::sort permutation on
2^32 - realLen, float32 division).  Test 2 pins it on what the compiled reference's own checkIdyAndTrim returned
(tests/golden/trim_repeat_raw*.ovlp.gz, made by tests/golden/make_trim_golden.py); tests 3 hold the device to it field
for field on crafted reads, test 4 holds the device to the reference's lines end to end."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from helpers import GOLDEN, golden_lines, golden_reads, repeat_stage_setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = {False: "trim_repeat_raw", True: "trim_repeat_raw_hpc"}


# ---- 1. declared and exported -----------------------------------------------------------------------------------------
def test_trim_ranges_is_exported_and_declared(built):
    from flye_amd import gpu
    lib = gpu.load_library()
    for sym in ("fg_trim_ranges", "fg_release_trims"):
        assert hasattr(lib, sym) and sym in gpu.ABI_SYMBOLS
    text = open(os.path.join(ROOT, "include", "flye_gpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"struct\s+fg_trim_rec\s*\{\s*int32_t\s+cur_begin\s*,\s*cur_end\s*,\s*ext_begin\s*,\s*ext_end\s*;\s*"
                     r"int32_t\s+run_start\s*,\s*run_end\s*;\s*int32_t\s+range_err\s*,\s*range_len\s*;\s*"
                     r"float\s+seq_divergence\s*;\s*\}", text)
    assert re.search(r"struct\s+fg_trim_batch\s*\{\s*uint32_t\s+n_pairs\s*;\s*uint64_t\s*\*\s*rec_off\s*;\s*"
                     r"struct\s+fg_trim_rec\s*\*\s*recs\s*;\s*void\s*\*\s*owner_\s*;\s*\}", text)
    assert re.search(r"\bint\s+fg_trim_ranges\s*\(\s*fg_ctx\s*\*[^)]*uint8_t\s+use_hpc\s*,\s*float\s+max_divergence\s*,"
                     r"\s*int32_t\s+min_overlap\s*,\s*struct\s+fg_trim_batch\s*\*", text)
    assert re.search(r"\bvoid\s+fg_release_trims\s*\(\s*struct\s+fg_trim_batch\s*\*", text)
    assert re.search(r"#define\s+FG_ABI_VERSION\s+4\b", text)
    assert lib.fg_abi_version() == 4
    assert gpu.TRIM_REC_DTYPE.itemsize == 36
    assert lib.fg_trim_ranges(None, None, 0, 0, 0.0, 0, None) == -3


# ---- the restatement of alignment.cpp:330-457 -------------------------------------------------------------------------
def parse_cigar(text):
    toks = text.split()
    return np.array([ord(t[-1]) for t in toks], np.uint8), np.array([int(t[:-1]) for t in toks], np.int64)


def offset_table(x, use_hpc):
    """homopolymerCompression's offsetTable (alignment.cpp:52-70) of a 0..3 array."""
    x = np.asarray(x, np.uint8)
    if not use_hpc or len(x) == 0:
        return np.arange(len(x), dtype=np.int64)
    keep = np.ones(len(x), bool)
    keep[1:] = x[1:] != x[:-1]
    return np.flatnonzero(keep).astype(np.int64)


def good_intervals(ops, lens, max_div):
    """:330-385: (start, end, realLen, err) of the good intervals in the enumeration order (interval length in runs
    descending, then start ascending), and the three prefix sums."""
    n = len(ops)
    z = np.zeros(1, np.int64)
    s_cur = np.concatenate([z, np.cumsum(np.where(ops == ord("I"), 0, lens))])
    s_ext = np.concatenate([z, np.cumsum(np.where(ops == ord("D"), 0, lens))])
    s_err = np.concatenate([z, np.cumsum(np.where(ops != ord("="), lens, 0))])
    eq = np.flatnonzero(ops == ord("="))
    a, b = np.triu_indices(len(eq))
    i, j = eq[a], eq[b]
    order = np.lexsort((i, -(j - i + 1)))
    i, j = i[order], j[order]
    real = np.maximum(s_cur[j + 1] - s_cur[i], s_ext[j + 1] - s_ext[i])
    err = s_err[j + 1] - s_err[i]
    div = err.astype(np.float32) / real.astype(np.float32)          # float(rangeErr) / rangeLen
    ok = div < np.float32(max_div)
    return i[ok], j[ok], real[ok], err[ok], (s_cur, s_ext, s_err), n


def std_perm(keys):
    from oracle import oracle as O
    return O.std_sort_perm(keys).astype(np.int64)


def stable_perm(keys):
    return np.argsort(keys, kind="stable")


def trim_restate(ops, lens, cur_begin, ext_begin, off_cur, off_ext, max_div, min_overlap, perm=std_perm):
    """checkIdyAndTrim behind its alignment: rows (cur_begin, cur_end, ext_begin, ext_end, run_start, run_end, range_err,
    range_len) in the order the function returns them."""
    i, j, real, err, (s_cur, s_ext, _), _ = good_intervals(ops, lens, max_div)
    if len(i) == 0:
        return np.zeros((0, 8), np.int64), 0
    p = perm((np.int64(1) << 32) - real)                           # realLen descending, nothing else
    out = []
    taken = []
    for k in p:
        s, e = int(i[k]), int(j[k])
        if any(min(e + 1, oe + 1) - max(s, os_) > 0 for os_, oe in taken):
            continue
        taken.append((s, e))
        cb = cur_begin + int(off_cur[s_cur[s]])
        eb = ext_begin + int(off_ext[s_ext[s]])
        ce = cur_begin + int(off_cur[s_cur[e + 1] - 1])             # the offset of the LAST aligned base (:444-445)
        ee = ext_begin + int(off_ext[s_ext[e + 1] - 1])
        if ce - cb > min_overlap and ee - eb > min_overlap:
            out.append((cb, ce, eb, ee, s, e, int(err[k]), int(real[k])))
    return np.array(out, np.int64).reshape(-1, 8), len(i)


def restate_pairs(cur, ext, pairs, use_hpc, max_div, min_overlap, perm=std_perm):
    """(rec_off, rows, good-list sizes) of fg_range_pair rows, aligned by the oracle's ksw2 on numpy-cut strings."""
    from oracle import oracle as O
    off = [0]
    rows = []
    good = []
    for cid, eid, cb, ce, eb, ee in pairs:
        t, q = cur.seq(cid)[cb:ce], ext.seq(eid)[eb:ee]
        ot, oq = offset_table(t, use_hpc), offset_table(q, use_hpc)
        ops, lens = parse_cigar(O.ksw_cigar(t[ot], q[oq])[1])
        r, g = trim_restate(ops, lens, int(cb), int(eb), ot, oq, max_div, min_overlap, perm)
        rows.append(r)
        good.append(g)
        off.append(off[-1] + len(r))
    return np.array(off, np.uint64), np.concatenate(rows) if rows else np.zeros((0, 8), np.int64), good


FIELDS = ("cur_begin", "cur_end", "ext_begin", "ext_end", "run_start", "run_end", "range_err", "range_len")


def assert_same(got, want):
    rec_off, recs = got
    want_off, rows, _ = want
    assert np.array_equal(rec_off, want_off)
    for k, f in enumerate(FIELDS):
        assert np.array_equal(recs[f].astype(np.int64), rows[:, k]), f
    bits = (rows[:, 6].astype(np.float32) / rows[:, 7].astype(np.float32)).view(np.uint32)
    assert np.array_equal(recs["seq_divergence"].view(np.uint32), bits)


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


def splice_lines(res, marked_rows, rec_off):
    """lines() of an oracle result with each marked record replaced by its pieces (rows of the restatement)."""
    lines = res.lines()
    out = []
    m = 0
    for i, line in enumerate(lines):
        if not res.needs_trim[i]:
            out.append(line)
            continue
        f = line.split()
        for cb, ce, eb, ee, _, _, err, real in marked_rows[int(rec_off[m]):int(rec_off[m + 1])]:
            bits = int(np.array([np.float32(err) / np.float32(real)], np.float32).view(np.uint32)[0])
            out.append(" ".join([f[0], str(cb), str(ce), f[3], f[4], str(eb), str(ee), f[7], f[8], f"{bits:08x}"] + f[10:]))
        m += 1
    return out


# ---- 2. the restatement is pinned on the reference --------------------------------------------------------------------
QUERY_STEP = 6      # every 6th query read whole (reads 0, 6, 12): the oracle's ksw2 on all 972 marked records of the
#                     case takes minutes on one core; the golden lines of those reads are compared


@pytest.mark.parametrize("use_hpc", [False, True])
def test_restatement_equals_reference(built, golden_cases, use_hpc):
    from flye_amd import config
    from oracle import oracle as O
    meta = json.load(open(os.path.join(GOLDEN, "trim_cases.json")))[FIXTURES[use_hpc]]
    case = golden_cases["repeat_raw"]
    seqs = golden_reads(case)
    cfg = config.preset(case["preset"])
    wnd, dk = repeat_stage_setup(case, cfg)
    assert dk["max_divergence"] == float(np.float32(meta["max_div"])) and dk["min_overlap"] == meta["min_overlap"]
    o = O.Oracle(int(cfg["kmer_size"]))
    o.set_reads(seqs, 0)
    o.build_index_minimizers(1, wnd, cfg["repeat_kmer_rate"])
    p = O.detector_params(cfg, **dk)
    p.use_hpc = int(use_hpc)
    q = np.arange(0, 2 * seqs.n, 2 * QUERY_STEP, dtype=np.uint32)
    res = o.overlaps(p, q)
    marked = res.recs[res.needs_trim != 0]
    assert len(marked) > 100
    st = Strands(seqs, 0)
    pairs = np.stack([marked[f].astype(np.int64) for f in ("cur_id", "ext_id", "cur_begin", "cur_end", "ext_begin", "ext_end")], axis=1)
    rec_off, rows, good = restate_pairs(st, st, pairs, use_hpc, np.float32(meta["max_div"]), meta["min_overlap"])
    want = [l for l in golden_lines(FIXTURES[use_hpc]) if int(l.split()[0]) in set(int(x) for x in q)]
    assert len(want) > 0 and len(rows) > 0
    assert splice_lines(res, rows, rec_off) == want
    print("marked", len(marked), "pieces", len(rows), "good intervals", sum(good))


# ---- 3. crafted reads -------------------------------------------------------------------------------------------------
def mutate(rng, x, sub, indel, keep_clear=()):
    """x with substitutions (rate sub) and single-base insertions / deletions (rate indel); positions in keep_clear stay."""
    out = []
    for i, b in enumerate(x):
        u = rng.random()
        if i in keep_clear or u >= sub + 2 * indel:
            out.append(b)
        elif u < sub:
            out.append((b + 1 + rng.integers(0, 3)) & 3)
        elif u < sub + indel:
            out += [b, rng.integers(0, 4)]
    return np.array(out, np.uint8)


SUBS = (99, 163, 227, 291, 300, 364, 396, 460)      # substitutions of read 1 against read 0: a '=' run begins behind each


def crafted():
    """Reads (ids from 0) and the pair table.
    read 0: random, 600 bases, homopolymer runs planted across the 32-base word edges and the 64-base step edges of
            ranges that begin at 0, 36 and 37
    read 1: read 0 with substitutions at SUBS only (no indels): with ranges that begin at 36 / 37 a '=' run's first base
            is base 64 / 63 of the range and another one's last base is base 63 / 62 .. -- the rank-select edges
    read 2: read 0 with 4 % substitutions and 3 % indels        read 3: the same at 8 % and 6 %
    read 4: a copy of read 0        read 5 / 6: "ACAC.." / "GTGT..": not one base in common
    read 7 / 8: the tie case (see tie_reads)"""
    rng = np.random.default_rng(20261019)
    r0 = rng.integers(0, 4, size=600, dtype=np.uint8)
    for a, b in ((28, 37), (60, 70), (92, 99), (100, 104), (120, 135), (155, 163), (164, 170), (222, 227), (228, 232),
                 (286, 291), (292, 296), (301, 306), (350, 364), (365, 372), (390, 396), (397, 420), (455, 460), (461, 470)):
        r0[a:b] = r0[a]
        r0[a - 1] = (r0[a] + 1) & 3
        r0[b] = (r0[a] + 2) & 3
    r1 = r0.copy()
    for p in SUBS:
        r1[p] = (r0[p] + 2) & 3 if (r0[p] + 2) & 3 not in (r0[p - 1], r0[p + 1]) else (r0[p] + 3) & 3
    r2 = mutate(rng, r0, 0.04, 0.015)[:600]
    r3 = mutate(rng, r0, 0.08, 0.03)[:600]
    r5 = np.tile(np.array([0, 1], np.uint8), 150)
    r6 = np.tile(np.array([2, 3], np.uint8), 150)
    t7, t8 = tie_reads()
    reads = [r0, r1, r2, r3, r0.copy(), r5, r6, t7, t8]
    L = [len(r) for r in reads]
    assert all(300 <= n <= 600 for n in L)
    P = []
    for b in (0, 36, 37, 35, 34, 28, 100, 101):              # read 0 against read 1: the edges
        P.append((0, 2, b, 600, b, 600))
        P.append((2, 0, b, 590, b, 590))
    for e in (164, 228, 292, 365, 397):                      # ... ranges that END behind a substitution / in a run
        P.append((0, 2, 36, e, 36, e))
        P.append((0, 2, 0, e + 1, 0, e + 1))
    P.append((0, 4, 0, 600, 0, L[2]))                        # noisy pairs, whole reads
    P.append((0, 6, 0, 600, 0, L[3]))
    P.append((4, 6, 10, 500, 5, 520))
    P.append((1, 5, 0, 600, 0, L[2]))                        # reverse strand on both sides
    P.append((1, 4, 0, 600, 0, L[2]))                        # ... on the cur side only: nothing aligns well
    P.append((0, 5, 0, 600, 0, L[2]))                        # ... on the ext side only
    P.append((3, 1, 33, 577, 31, 580))                       # reverse strands of reads 1 and 0
    P.append((5, 7, 64, 512, 60, 500))
    P.append((0, 8, 0, 600, 0, 600))                         # identical strings: one run, one record
    P.append((0, 8, 250, 600, 250, 600))
    P.append((10, 12, 0, 300, 0, 300))                       # no '=' run: no record
    P.append((0, 2, 0, 0, 10, 15))                           # empty ranges
    P.append((0, 2, 10, 15, 7, 7))
    P.append((0, 2, 5, 5, 7, 7))
    P.append((14, 16, 0, L[7], 0, L[8]))                     # the tie case
    P.append((0, 2, 37, 420, 37, 420))
    return reads, np.array(P, np.int64)


TIE_SEED, TIE_DIV, MIN_OVERLAP = 42, 0.05, 10


def tie_reads():
    """Two reads of 500 bases, 6 % substitutions and 4 % indels apart: at gate TIE_DIV the pair has hundreds of good
    intervals with many equal realLen, and the unstable std::sort decides between two intersecting ones (asserted in
    test_tie_case_is_a_tie_case)."""
    rng = np.random.default_rng(TIE_SEED)
    a = rng.integers(0, 4, size=500, dtype=np.uint8)
    return a, mutate(rng, a, 0.06, 0.02)[:600]


GATES = (np.float32(0.02), np.float32(TIE_DIV), np.float32(0.3), np.float32(1e-9))


@pytest.fixture(scope="module")
def crafted_expected(built):
    """The restatement's records of the crafted pairs per (use_hpc, gate), computed once on the CPU."""
    from flye_amd import synth
    reads, pairs = crafted()
    rs = synth.ReadSet.from_arrays(reads)
    st = Strands(rs, 0)
    want = {(h, float(g)): restate_pairs(st, st, pairs, h, g, MIN_OVERLAP) for h in (False, True) for g in GATES}
    return rs, st, pairs, want


def test_tie_case_is_a_tie_case(crafted_expected):
    """The last but one pair: more than 16 good intervals, two intersecting ones of equal realLen that both pass
    min_overlap, and std::sort's permutation gives other records than a stable sort's."""
    rs, st, pairs, want = crafted_expected
    k = len(pairs) - 2
    assert tuple(pairs[k][:2]) == (14, 16)
    from oracle import oracle as O
    for use_hpc in (False, True):
        cid, eid, cb, ce, eb, ee = pairs[k]
        t, q = st.seq(cid)[cb:ce], st.seq(eid)[eb:ee]
        ot, oq = offset_table(t, use_hpc), offset_table(q, use_hpc)
        ops, lens = parse_cigar(O.ksw_cigar(t[ot], q[oq])[1])
        i, j, real, err, (s_cur, s_ext, _), _ = good_intervals(ops, lens, np.float32(TIE_DIV))
        assert len(i) > 16
        a, _ = trim_restate(ops, lens, int(cb), int(eb), ot, oq, np.float32(TIE_DIV), MIN_OVERLAP, std_perm)
        b, _ = trim_restate(ops, lens, int(cb), int(eb), ot, oq, np.float32(TIE_DIV), MIN_OVERLAP, stable_perm)
        # the first record the two outcomes differ in: intersecting intervals of equal realLen, both above min_overlap
        # (they are records), one chosen by std::sort's permutation and the other by a stable sort's
        d = [m for m in range(min(len(a), len(b))) if not np.array_equal(a[m], b[m])]
        assert d, "std::sort and a stable sort agree on the tie pair"
        x, y = a[d[0]], b[d[0]]
        assert x[7] == y[7] and tuple(x[4:6]) != tuple(y[4:6]) and min(x[5], y[5]) - max(x[4], y[4]) >= 0


@pytest.fixture(scope="module")
def crafted_ctx(crafted_expected):
    from flye_amd import gpu
    rs, st, pairs, want = crafted_expected
    ctx = gpu.Context(17, 0)
    ctx.set_reads(rs, 0)
    return ctx


@pytest.mark.gpu
@pytest.mark.parametrize("use_hpc", [False, True])
def test_crafted_pairs(crafted_expected, crafted_ctx, use_hpc):
    """Every crafted pair at every gate, field for field; the cases are what they claim to be."""
    rs, st, pairs, want = crafted_expected
    ctx = crafted_ctx
    for g in GATES:
        w = want[(use_hpc, float(g))]
        assert_same(ctx.trim_ranges(pairs, use_hpc, g, MIN_OVERLAP), w)
    kt = ctx.kernel_times()
    for k in ("k_trim_prefix", "k_trim_count", "k_trim_emit", "k_trim_select", "k_trim_map", "k_ksw_decode"):
        assert k in kt, k
    off, rows, good = want[(use_hpc, float(GATES[1]))]
    n_of = np.diff(off.astype(np.int64))
    ident = [k for k, p in enumerate(pairs) if tuple(p[:2]) == (0, 8)]
    assert all(n_of[k] == 1 and good[k] == 1 for k in ident)                        # one run, one record
    none = [k for k, p in enumerate(pairs) if tuple(p[:2]) == (10, 12) or p[3] == p[2] or p[5] == p[4]]
    assert len(none) == 4 and all(n_of[k] == 0 and good[k] == 0 for k in none)      # no '=' run / empty ranges
    assert max(good) > 16 and n_of.max() > 3
    assert any(n_of[k] > 0 for k, p in enumerate(pairs) if p[0] & 1) and any(n_of[k] > 0 for k, p in enumerate(pairs) if p[1] & 1)
    # the rank-select edges, over all gates: pieces whose first / last base is base 0 or 63 of a 64-base step of the
    # range, and 0 or 31 of a 32-base word
    for col, beg in ((0, 2), (1, 2), (2, 4), (3, 4)):
        rel = np.concatenate([want[(use_hpc, float(g))][1][:, col] -
                              pairs[np.repeat(np.arange(len(pairs)), np.diff(want[(use_hpc, float(g))][0].astype(np.int64))), beg]
                              for g in GATES])
        assert {0, 63} <= set(int(x) for x in rel % 64), (col, sorted(set(int(x) for x in rel % 64)))
        assert {0, 31} <= set(int(x) for x in rel % 32)
    if use_hpc:     # compression moved them: the offset tables are not the identity
        rows0 = want[(False, float(GATES[1]))][1]
        assert rows0.shape != rows.shape or not np.array_equal(rows0[:, :4], rows[:, :4])


@pytest.mark.gpu
def test_gate_exactly_on_a_quotient(crafted_expected, crafted_ctx):
    """max_divergence = float32(e) / float32(l) of an interval that occurs: the test is strictly less, so that interval
    is not kept, and is kept at the next float above."""
    rs, st, pairs, want = crafted_expected
    ctx = crafted_ctx
    from oracle import oracle as O
    k = [k for k, p in enumerate(pairs) if tuple(p) == (0, 4, 0, 600, 0, len(st.seq(4)))][0]
    cid, eid, cb, ce, eb, ee = pairs[k]
    ops, lens = parse_cigar(O.ksw_cigar(st.seq(cid)[cb:ce], st.seq(eid)[eb:ee])[1])
    i, j, real, err, _, _ = good_intervals(ops, lens, np.float32(2.0))
    # the first interval of the enumeration spans every other one: the longest realLen, so it is the first record
    # wherever it is good
    cand = 0
    assert err[cand] > 0 and real[cand] == real.max()
    thr = np.float32(err[cand]) / np.float32(real[cand])
    up = np.nextafter(thr, np.float32(1))
    sel = pairs[k:k + 1]
    at = restate_pairs(st, st, sel, False, thr, MIN_OVERLAP)
    above = restate_pairs(st, st, sel, False, up, MIN_OVERLAP)
    key = (int(i[cand]), int(j[cand]))
    in_at = key in {(int(r[4]), int(r[5])) for r in at[1]}
    in_up = key in {(int(r[4]), int(r[5])) for r in above[1]}
    assert above[2][0] > at[2][0]                       # the good list grows by the intervals on the quotient
    assert not in_at
    got_at, got_up = ctx.trim_ranges(sel, False, thr, MIN_OVERLAP), ctx.trim_ranges(sel, False, up, MIN_OVERLAP)
    assert_same(got_at, at)
    assert_same(got_up, above)
    assert key not in set(zip(got_at[1]["run_start"].tolist(), got_at[1]["run_end"].tolist()))
    assert in_up and key in set(zip(got_up[1]["run_start"].tolist(), got_up[1]["run_end"].tolist()))


@pytest.mark.gpu
@pytest.mark.parametrize("use_hpc", [False, True])
def test_cur_side_in_its_own_container(crafted_expected, use_hpc):
    from flye_amd import gpu
    rs, st, pairs, want = crafted_expected
    first = 2 * rs.n + 4
    ctx = gpu.Context(17, 0)
    ctx.set_reads(rs, 0)
    ctx.set_queries(rs, first)
    moved = pairs.copy()
    moved[:, 0] += first
    assert_same(ctx.trim_ranges(moved, use_hpc, GATES[1], MIN_OVERLAP), want[(use_hpc, float(GATES[1]))])
    with pytest.raises(gpu.FlyeGpuError) as e:
        ctx.trim_ranges(pairs[:1], use_hpc, GATES[1], MIN_OVERLAP)
    assert e.value.code == -3


@pytest.mark.gpu
def test_argument_errors_and_align_ranges_unchanged(crafted_expected, crafted_ctx):
    """fg_align_ranges' argument errors with their codes, a context that still works, and fg_align_ranges' bytes on the
    same context before and after the new call."""
    from flye_amd import gpu
    rs, st, pairs, want = crafted_expected
    ctx = crafted_ctx
    L = ctx.L
    before = [ctx.align_ranges(pairs, use_hpc=h, arrays=True) for h in (False, True)]
    n_ids = 2 * ctx.n_reads
    good = (0, 2, 0, 100, 0, 100)
    bad = [(n_ids, 2, 0, 10, 0, 10), (0, n_ids, 0, 10, 0, 10), (0, 2, -1, 10, 0, 10), (0, 2, 0, 10, -1, 10),
           (0, 2, 11, 10, 0, 10), (0, 2, 0, 10, 11, 10), (0, 2, 0, len(st.seq(0)) + 1, 0, 10),
           (0, 2, 0, 10, 0, len(st.seq(2)) + 1)]
    for row in bad:
        with pytest.raises(gpu.FlyeGpuError) as e:
            ctx.trim_ranges(np.array([good, row], np.int64), False, 0.1, MIN_OVERLAP)
        assert e.value.code == -3 and "fg_trim_ranges" in str(e.value)
    tab = np.zeros(1, gpu.RANGE_PAIR_DTYPE)
    tab[0] = good
    b = gpu.TrimBatch()
    assert L.fg_trim_ranges(ctx.h, None, 1, 0, 0.1, 10, C.byref(b)) == -3
    assert L.fg_last_error(ctx.h)
    assert L.fg_trim_ranges(ctx.h, tab.ctypes.data, 1, 0, 0.1, 10, None) == -3
    assert L.fg_trim_ranges(ctx.h, None, 0, 0, 0.1, 10, C.byref(b)) == 0          # no pairs: an empty batch
    assert b.n_pairs == 0 and b.rec_off[0] == 0
    L.fg_release_trims(C.byref(b))
    empty = gpu.Context(17, 0)
    with pytest.raises(gpu.FlyeGpuError) as e:
        empty.trim_ranges(np.array([good], np.int64), False, 0.1, MIN_OVERLAP)
    assert e.value.code == -4
    assert_same(ctx.trim_ranges(pairs, True, GATES[1], MIN_OVERLAP), want[(True, float(GATES[1]))])
    after = [ctx.align_ranges(pairs, use_hpc=h, arrays=True) for h in (False, True)]
    for x, y in zip(before, after):
        assert all(np.array_equal(u, v) for u, v in zip(x[0], y[0]))
        assert np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2])


# ---- 4. the reference end to end --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def repeat_ctx(built, golden_cases):
    from flye_amd import config, gpu
    case = golden_cases["repeat_raw"]
    seqs = golden_reads(case)
    cfg = config.preset(case["preset"])
    wnd, dk = repeat_stage_setup(case, cfg)
    ctx = gpu.Context(int(cfg["kmer_size"]), 0)
    ctx.set_reads(seqs, 0)
    vi = gpu.VertexIndex(ctx, float(int(cfg["assemble_kmer_sample"])))
    vi.buildIndexMinimizers(1, wnd, cfg["repeat_kmer_rate"])
    return ctx, vi, seqs, cfg, dk


@pytest.mark.gpu
@pytest.mark.parametrize("use_hpc", [False, True])
def test_reference_end_to_end(repeat_ctx, use_hpc, monkeypatch):
    """fg_overlaps with partition_bad_mappings, fg_trim_ranges on the marked records, spliced(): the lines the
    reference's getSeqOverlaps wrote with its own checkIdyAndTrim.  Once more with a scratch budget that cuts the marked
    pairs into several sub-batches: identical records."""
    from flye_amd import gpu
    ctx, vi, seqs, cfg, dk = repeat_ctx
    meta = json.load(open(os.path.join(GOLDEN, "trim_cases.json")))[FIXTURES[use_hpc]]
    det = gpu.OverlapDetector(ctx, vi, int(cfg["maximum_jump"]), dk["min_overlap"], dk["max_overhang"], True,
                              dk["only_max_ext"], dk["max_divergence"], True, True, use_hpc)
    det.p.partition_bad_mappings = 1
    res = det.getSeqOverlapsBatch(np.arange(0, 2 * seqs.n, 2, dtype=np.uint32))
    marked = res.recs[res.needs_trim != 0].copy()
    assert len(marked) > 900 if not use_hpc else len(marked) > 0
    trims = ctx.trim_ranges(marked, use_hpc, det.p.max_divergence, dk["min_overlap"])
    kt = ctx.kernel_times()
    print(len(marked), "marked,", len(trims[1]), "pieces,", round(ctx.last_trim_seconds * 1e3, 2), "ms",
          {k: round(v[0] * 1e3, 3) for k, v in kt.items()})
    assert "k_trim_select" in kt and "k_trim_map" in kt
    sp = res.spliced(trims)
    lines = sp.lines()
    assert lines == golden_lines(FIXTURES[use_hpc])
    assert len(lines) == meta["n_records"] and int(sp.query_off[-1]) == len(lines)
    monkeypatch.setenv("FG_TRIM_SCRATCH_BYTES", str(1 << 18))      # ~ 100k intervals x 32 bytes: ten or more sub-batches
    small = ctx.trim_ranges(marked, use_hpc, det.p.max_divergence, dk["min_overlap"])
    monkeypatch.delenv("FG_TRIM_SCRATCH_BYTES")
    assert np.array_equal(small[0], trims[0]) and small[1].tobytes() == trims[1].tobytes()
