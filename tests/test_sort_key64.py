"""The hit sort in its two 64-bit forms, each on its own (the overlap stage reaches them only with more than 32 key bits):

* packed records (fg_debug_sort_packed): ``key << 24 | value`` in one word with ``key = record << cur_bits | cur``, no
  value array, ordered on the 40 key bits alone;
* 64-bit keys ``ext_id << 32 | cur`` beside 32-bit values (fg_debug_sort_pairs64), told ``cur_bits`` as the stage tells
  it, so that the LDS kernel's remap to ``ext_id << cur_bits | cur`` and back runs.

``cur_bits`` = 17 throughout; the same (record, cur) pairs serve both forms.  One call sorts segments laid back to back,
with empty and one-hit segments between them; every segment is held against ``oracle.std_sort_perm`` of its keys, the
permutation through the values, then the keys.

Sizes, one per route of sortSegments at its edges: 2, 16, 17, 63, 64, 65 (the register sort inside k_sort_lds); 447, 448
(the LDS piece), 449 (one streamed level first); 8191, 8192 (streamed partition), 8193 (one-wave closed form); 16384
(closed form), 16385 and 40001 (a workgroup per piece, k_sort_wide).

Key families:

* straddle: all sizes, records {2^15 - 1, 2^15, 2^15 + 1, 2^23 - 1}, cur from a small set (most keys several times):
  packed keys on both sides of 2^32 and up to 40 bits;
* uniform40: all sizes, keys uniform in [0, 2^40): the LDS pieces of the larger segments span more than 2^32 keys or
  fewer, so one call takes both branches of the narrowing decision with no switch set (the CPU replay below says which
  pieces of the 40001-hit segment do what);
* narrow edge: 300 and 448 hits (one LDS piece each) with minimum key m and maximum m + 0xFFFFFFFF (the last span that
  is narrowed) or m + 0x100000000 (the first that is not), m = 0 and 2^39, ties inside;
* killer: Musser's median-of-3 killer at n = 1000 and 20000 and each ``// 3``, shifted so that 2^32 lies in the middle of the
  key range (the shift keeps the order, hence the trajectory).  Replayed on the CPU (polish_restate.std_sort_perm with
  its trace), the plain killers run out of depth budget on a 468-hit piece (n = 1000: just above SORT_CAP, heap sorted
  by one lane of a k_sort_level wave under every setting) and on pieces of 516 .. 9948 hits (n = 20000: the 9948-hit
  one is a k_sort_level task by default and a k_sort_wide task under FG_SORT_WIDE_MIN=4096); the ``// 3`` forms on
  571 .. 1294 hits (n = 20000) and only inside LDS pieces (n = 1000).

Two value runs: the index inside the segment (the value array is the permutation), then 0xFFFFFF - index: the keys must
come out identical and the values in the same permutation, so the 24 value bits of a packed record take no part in a
compare.  Every setting of SETTINGS is run with both forms; the arrays must equal the oracle's and, byte for byte, those
of the run with no setting.

The tests without a ``gpu`` mark show that these inputs can tell a wrong kernel from a right one without running a wrong
one: what a compare truncated to 32 bits or a compare on the whole packed word would give differs from the oracle's.

One check departs from its first wording, "a 448-hit window of a uniform40 segment's sorted keys spans less than 2^32
and another more": 448 of 40001 uniform keys span 2^33.5 on average and never less than 2^32, so no segment of these
sizes has such a window.  What decides the branch is the span of an LDS piece, and pieces have 2 .. 448 hits; the test
replays the partitions of the 40001-hit segment and asserts that its real pieces fall on both sides."""
import functools
import os
import time

import numpy as np
import pytest

import polish_restate as R

SORT_CAP = 448
WIDE_MIN = 16384                      # FG_SORT_WIDE_MIN's default
CUR_BITS = 17
CUR_MASK = (1 << CUR_BITS) - 1
VAL_MAX = 0xFFFFFF
B32 = 1 << 32

SIZES = [2, 16, 17, 63, 64, 65, 447, 448, 449, 8191, 8192, 8193, 16384, 16385, 40001]
STRADDLE_RECS = [(1 << 15) - 1, 1 << 15, (1 << 15) + 1, (1 << 23) - 1]
EDGE_SIZES = [300, 448]
EDGE_SPANS = [0xFFFFFFFF, 0x100000000]
EDGE_MINS = [0, 1 << 39]
KILLERS = [(1000, 1), (1000, 3), (20000, 1), (20000, 3)]

FORMS = ["packed", "pairs64"]
SETTINGS = [{},
            {"FG_SORT_STREAM_MAX": "600"},
            {"FG_SORT_STREAM_MAX": "1000000000"},
            {"FG_SORT_MANY_MIN": "2", "FG_SORT_STREAM_MANY": "50000"},
            {"FG_NARROW_MAX": "0"},
            {"FG_SORT_WIDE_MIN": "4096"},
            {"FG_SORT_LEVEL_BATCH": "1"},
            {"FG_SORT_LEVEL_BATCH": "16"}]
SWITCHES = ["FG_SORT_STREAM_MAX", "FG_SORT_MANY_MIN", "FG_SORT_STREAM_MANY", "FG_NARROW_MAX", "FG_SORT_WIDE_MIN",
            "FG_SORT_LEVEL_BATCH", "FG_SORT_TIEFREE", "FG_SORT_RADIX_MAX", "FG_SORT_TRACE"]


def _setting_id(s):
    return ",".join(f"{k}={v}" for k, v in s.items()) or "none"


def _median3_killer(n):
    k = n // 2
    a = np.zeros(n, np.uint64)
    for i in range(1, k + 1):
        if i % 2 == 1:
            a[i - 1] = i
            a[i] = k + i
        a[k + i - 1] = 2 * i
    return a


def _straddle(rng, n):
    rec = rng.choice(np.asarray(STRADDLE_RECS, np.uint64), size=n)
    cur = rng.integers(0, max(2, n // 24), size=n).astype(np.uint64)
    # in front: a pair that the full key swaps and its low 32 bits (0 and 0xFFFE0001) leave in place
    rec[0], cur[0], rec[1], cur[1] = 1 << 15, 0, (1 << 15) - 1, 1
    return (rec << np.uint64(CUR_BITS)) | cur


def _edge(rng, n, m, span):
    offs = np.unique(np.concatenate([[0, span], rng.integers(0, span + 1, size=n // 6)])).astype(np.uint64)
    keys = np.uint64(m) + rng.choice(offs, size=n)
    lo, hi = rng.choice(n, size=2, replace=False)
    keys[lo], keys[hi] = m, m + span
    return keys


@functools.lru_cache(maxsize=None)
def _input():
    """(packed keys of all segments, segment offsets, [(family, what)] per segment)"""
    rng = np.random.default_rng(20264)
    segs, fam = [], []

    def add(family, what, keys):
        # an empty and a one-hit segment in turn between the real ones
        if len(segs) % 4 == 2:
            segs.append(np.empty(0, np.uint64))
        else:
            segs.append(rng.integers(0, 1 << 40, size=1, dtype=np.uint64))
        fam.append(("between", len(segs[-1])))
        segs.append(np.ascontiguousarray(keys, np.uint64))
        fam.append((family, what))

    for n in SIZES:
        add("straddle", n, _straddle(rng, n))
    for n in SIZES:
        add("uniform40", n, rng.integers(0, 1 << 40, size=n, dtype=np.uint64))
    for n in EDGE_SIZES:
        for m in EDGE_MINS:
            for span in EDGE_SPANS:
                add("edge", (n, m, span), _edge(rng, n, m, span))
    for n, div in KILLERS:
        add("killer", (n, div), _median3_killer(n) // np.uint64(div) + np.uint64(B32 - n // div // 2))
    off = np.zeros(len(segs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in segs])
    keys = np.concatenate(segs)
    assert int(keys.max()) < 1 << 40
    return keys, off, fam


def _form_keys(form, keys):
    """the packed keys as the form's own keys (an order-preserving map: record and cur change places with nothing)"""
    if form == "packed":
        return keys
    return ((keys >> np.uint64(CUR_BITS)) << np.uint64(32)) | (keys & np.uint64(CUR_MASK))


def _index_vals(off):
    n = np.diff(off.astype(np.int64))
    return (np.arange(int(off[-1]), dtype=np.int64) - np.repeat(off[:-1].astype(np.int64), n)).astype(np.uint32)


def _segments():
    keys, off, fam = _input()
    for i, f in enumerate(fam):
        yield f, keys[int(off[i]):int(off[i + 1])]


def _sort(ctx, form, vals):
    keys, off, _ = _input()
    if form == "packed":
        return ctx.debug_sort_packed(keys, vals, off, CUR_BITS)
    return ctx.debug_sort_pairs64(_form_keys(form, keys), vals, off, CUR_BITS)


def _clean_env():
    return {sw: os.environ.pop(sw) for sw in SWITCHES if sw in os.environ}


# ---- fixtures: one oracle pass, one context, one run without settings -----------------------------------------------------
@pytest.fixture(scope="module")
def gather(built):
    """index array g with sorted = input[g]: oracle.std_sort_perm per segment; the same for both forms"""
    from oracle import oracle as O
    keys, off, _ = _input()
    out = {}
    for form in FORMS:
        fk = _form_keys(form, keys)
        out[form] = np.concatenate([int(off[i]) + O.std_sort_perm(fk[int(off[i]):int(off[i + 1])]).astype(np.int64)
                                    for i in range(len(off) - 1)])
    assert np.array_equal(out["packed"], out["pairs64"])
    return out["packed"]


@pytest.fixture(scope="module")
def ctx(built):
    from flye_amd import gpu
    c = gpu.Context(17, 0)
    yield c
    c.close()


def _both_runs(ctx, form):
    """((keys, values) with value = index, (keys, values) with value = 0xFFFFFF - index)"""
    _, off, _ = _input()
    idx = _index_vals(off)
    return _sort(ctx, form, idx), _sort(ctx, form, np.uint32(VAL_MAX) - idx)


@pytest.fixture(scope="module")
def baseline(ctx):
    saved = _clean_env()
    out = {form: _both_runs(ctx, form) for form in FORMS}
    os.environ.update(saved)
    return out


def _assert_is_std_sort(form, runs, gather):
    keys, off, fam = _input()
    fk = _form_keys(form, keys)
    idx = _index_vals(off)
    (k1, v1), (k2, v2) = runs
    want_k = fk[gather]
    for (k, v), vals in (((k1, v1), idx), ((k2, v2), np.uint32(VAL_MAX) - idx)):
        assert k.dtype == np.uint64 and v.dtype == np.uint32 and len(k) == len(v) == len(keys)
        if not (np.array_equal(k, want_k) and np.array_equal(v, vals[gather])):      # name the first segment that differs
            for i in range(len(off) - 1):
                a, b = int(off[i]), int(off[i + 1])
                assert np.array_equal(v[a:b], vals[gather[a:b]]), (form, i, fam[i], "values")
                assert np.array_equal(k[a:b], want_k[a:b]), (form, i, fam[i], "keys")
    # the value bits took no part: same keys, same permutation
    assert k1.tobytes() == k2.tobytes()
    assert np.array_equal(np.uint32(VAL_MAX) - v2, v1)


# ---- CPU: the inputs are what the docstring says, and they can tell a wrong compare from a right one ------------------------
def test_input_is_what_the_docstring_says():
    keys, off, fam = _input()
    size = np.diff(off.astype(np.int64))
    real = [i for i, f in enumerate(fam) if f[0] != "between"]
    assert [int(size[i]) for i in real if fam[i][0] in ("straddle", "uniform40")] == SIZES + SIZES
    between = [int(size[i]) for i, f in enumerate(fam) if f[0] == "between"]
    assert set(between) == {0, 1} and len(between) == len(real)
    assert real == list(range(1, len(fam), 2))                                         # one in front of every real one
    assert int(size.max()) <= VAL_MAX                                                  # the index fits the 24 value bits
    for f, seg in _segments():
        if f[0] == "straddle":
            assert set(int(x) for x in np.unique(seg >> np.uint64(CUR_BITS))) <= set(STRADDLE_RECS)
            if len(seg) > 64:
                assert len(np.unique(seg)) < len(seg) // 2                             # most keys several times
                assert int(seg.max()) >> 39 == 1 and int(seg.min()) < B32              # 40 bits, and below 2^32
        elif f[0] == "killer":
            n, div = f[1]
            assert len(seg) == n and int(seg.min()) < B32 <= int(seg.max())
    # the pair form's keys are an order-preserving image of the packed keys
    o = np.argsort(keys, kind="stable")
    assert np.array_equal(o, np.argsort(_form_keys("pairs64", keys), kind="stable"))
    assert int((_form_keys("pairs64", keys) & np.uint64(0xFFFFFFFF)).max()) <= CUR_MASK


def test_a_segment_straddles_2_to_the_32():
    n = sum(1 for f, seg in _segments() if len(seg) and int(seg.min()) < B32 <= int(seg.max()))
    assert n >= len(SIZES) + len(KILLERS)                # every straddle and killer segment, and most uniform40 ones


def test_narrow_edge_spans_are_exact():
    seen = []
    for f, seg in _segments():
        if f[0] != "edge":
            continue
        n, m, span = f[1]
        assert len(seg) == n <= SORT_CAP                 # one LDS piece: its span is the segment's
        assert int(seg.min()) == m and int(seg.max()) - int(seg.min()) == span
        assert len(np.unique(seg)) < n                   # ties inside
        seen.append((n, m, span))
    assert sorted(seen) == sorted((n, m, s) for n in EDGE_SIZES for m in EDGE_MINS for s in EDGE_SPANS)
    assert EDGE_SPANS == [(1 << 32) - 1, 1 << 32]


def test_a_compare_on_the_low_32_bits_would_be_caught(built):
    from oracle import oracle as O
    checked = 0
    for f, seg in _segments():
        if f[0] not in ("straddle", "killer"):
            continue
        want = seg[O.std_sort_perm(seg)]
        assert not np.array_equal(seg[O.std_sort_perm(seg & np.uint64(0xFFFFFFFF))], want), f
        # the pair form: the low word of ext_id << 32 | cur is cur alone
        pk = _form_keys("pairs64", seg)
        assert not np.array_equal(pk[O.std_sort_perm(pk & np.uint64(0xFFFFFFFF))], pk[O.std_sort_perm(pk)]), f
        checked += 1
    assert checked == len(SIZES) + len(KILLERS)


def test_a_compare_on_the_whole_packed_word_would_be_caught(built):
    """with ties in a segment, ordering the words ``key << 24 | value`` cannot agree with the order by key in both value
    runs: the first run's values ascend among equal keys where the second's descend"""
    from oracle import oracle as O
    checked = 0
    for f, seg in _segments():
        if len(np.unique(seg)) == len(seg):
            continue
        idx = np.arange(len(seg), dtype=np.uint64)
        perm = O.std_sort_perm(seg)
        differs = [not np.array_equal(O.std_sort_perm((seg << np.uint64(24)) | v), perm)
                   for v in (idx, np.uint64(VAL_MAX) - idx)]
        assert any(differs), f
        checked += 1
    # the straddle segments from 63 hits on, the narrow-edge segments and the killers // 3 at the least
    assert checked >= (len(SIZES) - 3) + len(EDGE_SIZES) * len(EDGE_MINS) * len(EDGE_SPANS) + 2


def _pieces(keys):
    """the ranges the level loop hands on: [(first, last, depth)] of the LDS pieces (2 .. SORT_CAP hits) and the sizes of
    the larger pieces it heap sorts at depth 0, with the final arrangement of the indices"""
    lds, heaps = [], []

    def trace(first, last, depth, heap):
        if heap:
            heaps.append(last - first)
        elif 2 <= last - first <= SORT_CAP:
            lds.append((first, last, depth))
    perm = R.std_sort_perm([int(x) for x in keys], trace=trace, leaf=SORT_CAP)
    return lds, heaps, np.asarray(perm, np.int64)


def test_uniform40_pieces_take_both_narrowing_branches():
    seg = next(s for f, s in _segments() if f == ("uniform40", 40001))
    lds, heaps, perm = _pieces(seg)
    assert not heaps and sum(b - a for a, b, _ in lds) > 39000
    spans = [int(seg[perm[a:b]].max()) - int(seg[perm[a:b]].min()) for a, b, _ in lds]
    narrow = sum(1 for s in spans if s <= 0xFFFFFFFF)
    assert narrow >= 10 and len(spans) - narrow >= 10, (narrow, len(spans))
    # a window of SORT_CAP sorted keys, the largest piece there can be, spans more than 2^32 wherever it lies
    s = np.sort(seg)
    assert int((s[SORT_CAP - 1:] - s[:len(s) - SORT_CAP + 1]).min()) > 0xFFFFFFFF


def _route(n, wide_min=WIDE_MIN):
    """sort_route's choice for a piece above SORT_CAP"""
    assert n > SORT_CAP
    return "k_sort_wide" if n > wide_min else "k_sort_level"


def test_killers_reach_the_depth_limit_heapsort_on_both_kernels():
    heaps = {}
    for f, seg in _segments():
        if f[0] == "killer":
            heaps[f[1]] = _pieces(seg)[1]
            # the shift changed nothing: the plain killer walks the same way
            n, div = f[1]
            assert _pieces(_median3_killer(n) // np.uint64(div))[1] == heaps[f[1]]
    assert heaps[(1000, 1)] == [468]
    assert heaps[(1000, 3)] == []                         # out of budget only inside LDS pieces (wave_sort's own heap sort)
    assert sorted(heaps[(20000, 1)]) == [516, 547, 1175, 1443, 9948]
    assert sorted(heaps[(20000, 3)]) == [571, 616, 690, 1294]
    # one lane of a k_sort_level wave by default; the 9948-hit piece alone goes to a workgroup task under
    # FG_SORT_WIDE_MIN=4096 (thread 0 of k_sort_wide heap sorts it)
    every = [n for h in heaps.values() for n in h]
    assert {_route(n) for n in every} == {"k_sort_level"}
    assert [n for n in every if _route(n, 4096) == "k_sort_wide"] == [9948]
    # FG_SORT_MANY_MIN=2 / FG_SORT_STREAM_MANY=50000 raises the workgroup threshold to 50000 (sort_level_mode)
    assert {_route(n, max(50000, WIDE_MIN)) for n in every} == {"k_sort_level"}


def test_hooks_check_their_arguments(built):
    """refused on the arguments alone: the stand-in context is never looked at"""
    import ctypes as C
    from flye_amd import gpu
    L = gpu.load_library()
    FG_ERR_ARG = -3
    k = np.arange(4, dtype=np.uint64)
    v = np.arange(4, dtype=np.uint32)
    off = np.asarray([0, 4], np.uint64)
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    assert L.fg_debug_sort_packed(None, k.ctypes.data, off.ctypes.data, 1, CUR_BITS) == FG_ERR_ARG
    assert L.fg_debug_sort_packed(h, None, off.ctypes.data, 1, CUR_BITS) == FG_ERR_ARG
    assert L.fg_debug_sort_packed(h, k.ctypes.data, None, 1, CUR_BITS) == FG_ERR_ARG
    for bits in (-1, 40, 41, 64, 1 << 30):               # cur_bits + 24 value bits must stay below 64
        assert L.fg_debug_sort_packed(h, k.ctypes.data, off.ctypes.data, 1, bits) == FG_ERR_ARG, bits
    assert L.fg_debug_sort_pairs64(None, k.ctypes.data, v.ctypes.data, off.ctypes.data, 1, CUR_BITS) == FG_ERR_ARG
    assert L.fg_debug_sort_pairs64(h, None, v.ctypes.data, off.ctypes.data, 1, CUR_BITS) == FG_ERR_ARG
    assert L.fg_debug_sort_pairs64(h, k.ctypes.data, None, off.ctypes.data, 1, CUR_BITS) == FG_ERR_ARG
    assert L.fg_debug_sort_pairs64(h, k.ctypes.data, v.ctypes.data, None, 1, CUR_BITS) == FG_ERR_ARG
    for bits in (-1, 33, 64):
        assert L.fg_debug_sort_pairs64(h, k.ctypes.data, v.ctypes.data, off.ctypes.data, 1, bits) == FG_ERR_ARG, bits
    assert k.tolist() == [0, 1, 2, 3] and v.tolist() == [0, 1, 2, 3]


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("setting", SETTINGS, ids=_setting_id)
def test_order_is_std_sort_s_under_every_setting(ctx, gather, baseline, monkeypatch, form, setting):
    for sw in SWITCHES:
        monkeypatch.delenv(sw, raising=False)
    for sw, value in setting.items():
        monkeypatch.setenv(sw, value)
    t0 = time.perf_counter()
    runs = _both_runs(ctx, form) if setting else baseline[form]
    print(f"{form} {_setting_id(setting)}: two sorts of {len(_input()[0])} hits in {time.perf_counter() - t0:.2f} s")
    _assert_is_std_sort(form, runs, gather)
    for (k, v), (bk, bv) in zip(runs, baseline[form]):
        assert k.tobytes() == bk.tobytes() and v.tobytes() == bv.tobytes()


@pytest.mark.gpu
def test_both_forms_agree(baseline):
    """the same (record, cur) pairs in the same order, whichever form carried them"""
    (pk, pv), _ = baseline["packed"]
    (qk, qv), _ = baseline["pairs64"]
    assert np.array_equal(_form_keys("pairs64", pk), qk) and np.array_equal(pv, qv)
