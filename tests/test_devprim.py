"""The device-wide primitives of fg_devprim.h on their own, through fg_debug_scan / fg_debug_radix_sort_pairs:

* fgprim::scan against np.cumsum in uint64 reduced to the element width (sums are modulo 2^width), at every size where
  the number of levels or of tiles changes -- one tile (n <= 2048), two levels, three levels (n > 2048^2);
* fgprim::radixSortPairs against a stable np.argsort of the bits [begin, end) alone: keys whose other bits are not
  zero, ranges that are no multiple of 8 bits, skipped passes (which decide the buffer the result is in), heavy ties
  (the value permutation proves stability), tiles with one digit each (long look-back runs over empty aggregates) and
  more tiles than can be resident at once.

The hooks give every device buffer exactly the promised size with a guard behind it: a write past a buffer, or a
scratch size function that promises too little, fails the call.  Nothing here is compared with the library's own
output: the references are numpy's."""
import ctypes as C

import numpy as np
import pytest

SEED = 20240607
FG_ERR_ARG = -3
SCAN_TILE = 2048
RS_TILE = 2048
SQ = SCAN_TILE * SCAN_TILE

SCAN_N = [0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 2048 + 5, SQ - 1, SQ, SQ + 1,
          SQ + 2049]
SORT_N = [0, 1, 2, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 4096, 4097, 20 * 2048 + 1, 300_000]
SORT_N_LARGE = 3_000_001        # 1465 tiles
BIT_RANGES = [(0, 64), (0, 8), (0, 1), (0, 30), (0, 34), (34, 42), (5, 13), (3, 20), (7, 64), (60, 64)]
BIT_RANGES_LARGE = [(0, 64), (3, 20), (34, 42)]


@pytest.fixture(scope="module")
def ctx(built):
    from flye_amd import gpu
    c = gpu.Context(17, 0)
    yield c
    c.close()


# ---- scan ---------------------------------------------------------------------------------------------------------------
def _scan_inputs(rng, dtype, n):
    """(family, values) of n elements"""
    full = np.iinfo(dtype).max
    yield "ones", np.ones(n, dtype)
    yield "zeros", np.zeros(n, dtype)
    for at in (2047, 2048, SQ):
        if at < n:
            x = np.zeros(n, dtype)
            x[at] = 0x9E3779B1 if dtype == np.uint32 else 0x9E3779B97F4A7C15
            yield f"single@{at}", x
    if dtype == np.uint64:
        yield "random<2^40", rng.integers(0, 1 << 40, n, dtype=np.uint64)
    else:
        yield "random full width", rng.integers(0, full, n, dtype=np.uint32, endpoint=True)


def _scan_reference(x, inclusive):
    """np.cumsum in uint64 (itself modulo 2^64), reduced to the element width; exclusive = shifted by one"""
    inc = np.cumsum(x.astype(np.uint64), dtype=np.uint64)
    if not inclusive:
        inc = np.concatenate([np.zeros(1, np.uint64), inc[:-1]]) if len(x) else inc
    return inc.astype(x.dtype)          # uint64 -> uint32 keeps the low 32 bits


def _assert_same(got, want, tile, what):
    if np.array_equal(got, want):
        return
    assert len(got) == len(want), what
    bad = np.nonzero(got != want)[0]
    i = int(bad[0])
    raise AssertionError(f"{what}: {len(bad)} of {len(want)} wrong, first at index {i} (tile {i // tile}, offset "
                         f"{i % tile}): got {int(got[i]):#x}, want {int(want[i]):#x}")


@pytest.mark.gpu
@pytest.mark.parametrize("in_place", [True, False], ids=["in_place", "out_of_place"])
@pytest.mark.parametrize("inclusive", [True, False], ids=["inclusive", "exclusive"])
@pytest.mark.parametrize("dtype", [np.uint32, np.uint64], ids=["u32", "u64"])
def test_scan_equals_cumsum(ctx, dtype, inclusive, in_place):
    rng = np.random.default_rng(SEED)
    for n in SCAN_N:
        for family, x in _scan_inputs(rng, dtype, n):
            got = ctx.debug_scan(x, inclusive=inclusive, in_place=in_place)
            assert got.dtype == x.dtype
            _assert_same(got, _scan_reference(x, inclusive), SCAN_TILE, f"scan n={n} {family}")


@pytest.mark.gpu
def test_scan_u32_wraps_as_the_reference_does(ctx):
    """the sum passes 2^32 inside a tile, between tiles and between second-level tiles"""
    x = np.full(SQ + 2049, 0xFFFFFFF1, np.uint32)
    want = _scan_reference(x, True)
    assert int(np.cumsum(x[:3].astype(np.uint64))[-1]) >> 32 and want[1] < want[0]
    _assert_same(ctx.debug_scan(x, inclusive=True, in_place=True), want, SCAN_TILE, "scan of 0xFFFFFFF1")


# ---- radix sort -----------------------------------------------------------------------------------------------------------
def _shl(x, b):
    return x << np.uint64(b)


def _junk_below(rng, n, b):
    """random bits below bit b: outside the range, never to be looked at"""
    return rng.integers(0, 1 << b, n, dtype=np.uint64) if b else np.zeros(n, np.uint64)


def _from_pool(m):
    def make(rng, n, b, e):
        pool = rng.integers(0, 1 << 64, m, dtype=np.uint64)
        return pool[rng.integers(0, m, n)]
    return make


def _byte2_const(rng, n, b, e):
    k = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    mask = np.uint64(0xFF << (b + 16) & (1 << 64) - 1)
    return (k & ~mask) | (np.uint64(0xA7 << (b + 16) & (1 << 64) - 1) & mask)


def _index(n):
    return np.arange(n, dtype=np.uint64)


KEY_FAMILIES = {
    # bits outside [begin, end) are not zero
    "random": lambda rng, n, b, e: rng.integers(0, 1 << 64, n, dtype=np.uint64),
    "distinct2": _from_pool(2),
    "distinct5": _from_pool(5),
    "distinct300": _from_pool(300),
    "all_equal": lambda rng, n, b, e: np.full(n, rng.integers(0, 1 << 64, dtype=np.uint64), np.uint64),
    "byte2_const": _byte2_const,
    "ascending": lambda rng, n, b, e: _shl(_index(n), b) | _junk_below(rng, n, b),
    "descending": lambda rng, n, b, e: _shl(_index(n)[::-1].copy(), b) | _junk_below(rng, n, b),
    # one digit per tile: most (tile, digit) counts are zero
    "index//2048": lambda rng, n, b, e: _shl(_index(n) // np.uint64(2048), b) | _junk_below(rng, n, b),
    "index//5000": lambda rng, n, b, e: _shl(_index(n) // np.uint64(5000), b) | _junk_below(rng, n, b),
    "255-index%256": lambda rng, n, b, e: _shl(np.uint64(255) - _index(n) % np.uint64(256), b) | _junk_below(rng, n, b),
}


def _field(keys, b, e):
    return (keys >> np.uint64(b)) & np.uint64((1 << (e - b)) - 1)


def _expected_passes(keys, b, e):
    """8-bit passes from begin upwards, the last one as wide as is left; a pass in which all keys agree is skipped"""
    if len(keys) <= 1:
        return 0, 0
    total = (e - b + 7) // 8
    f = _field(keys, b, e)
    run = 0
    for p in range(total):
        d = (f >> np.uint64(8 * p)) & np.uint64(255)
        run += bool((d != d[0]).any())
    return run, total


def _check_sort(ctx, rng, family, n, b, e):
    keys = KEY_FAMILIES[family](rng, n, b, e)
    vals = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    assert keys.dtype == np.uint64 and len(keys) == n
    what = f"radix sort n={n} bits [{b}, {e}) {family}"
    order = np.argsort(_field(keys, b, e), kind="stable")
    gk, gv, passes = ctx.debug_radix_sort_pairs(keys, vals, b, e)
    print(f"{what}: {passes} passes")
    _assert_same(gk, keys[order], RS_TILE, what + " keys")
    _assert_same(gv, vals[order], RS_TILE, what + " values")
    run, total = _expected_passes(keys, b, e)
    assert passes == run, (what, passes, run, total)
    if family == "all_equal":
        assert passes == 0 and np.array_equal(gk, keys) and np.array_equal(gv, vals), what
    if n >= 63 and family == "random":
        assert passes == total, what
    if n >= 63 and family == "byte2_const" and e - b > 16:
        assert passes == total - 1, what            # the skipped pass lies in the middle wherever e - b > 24
    return passes


@pytest.mark.gpu
@pytest.mark.parametrize("bits", BIT_RANGES, ids=lambda r: f"{r[0]}_{r[1]}")
def test_radix_sort_equals_stable_argsort(ctx, bits):
    b, e = bits
    rng = np.random.default_rng(SEED + 64 * b + e)
    for n in SORT_N:
        for family in KEY_FAMILIES:
            _check_sort(ctx, rng, family, n, b, e)


@pytest.mark.gpu
@pytest.mark.parametrize("family", list(KEY_FAMILIES))
@pytest.mark.parametrize("bits", BIT_RANGES_LARGE, ids=lambda r: f"{r[0]}_{r[1]}")
def test_radix_sort_more_tiles_than_resident(ctx, bits, family):
    """1465 tiles of 39 KB of LDS each: late tiles take their tickets after early ones have retired"""
    b, e = bits
    _check_sort(ctx, np.random.default_rng(SEED + 64 * b + e), family, SORT_N_LARGE, b, e)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [(8, 8), (0, 0), (64, 64)], ids=lambda r: f"{r[0]}_{r[1]}")
def test_radix_sort_empty_bit_range_changes_nothing(ctx, bits):
    rng = np.random.default_rng(SEED)
    for n in (0, 1, 513, 20 * 2048 + 1):
        keys = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        vals = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        gk, gv, passes = ctx.debug_radix_sort_pairs(keys, vals, *bits)
        assert passes == 0 and np.array_equal(gk, keys) and np.array_equal(gv, vals), (n, bits)


@pytest.mark.gpu
def test_radix_sort_skipped_first_middle_and_last_pass(ctx):
    """bits [0, 24) with byte 0, 1 or 2 constant: two of the three passes run, whichever is left out, and the pass
    behind a skipped one reads the buffer pair the last pass that ran wrote"""
    rng = np.random.default_rng(SEED + 1)
    n = 20 * 2048 + 1
    vals = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    for const_byte, runs in ((1, 2), (2, 2), (0, 2)):
        keys = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        keys = (keys & ~np.uint64(0xFF << (8 * const_byte))) | np.uint64(0x5A << (8 * const_byte))
        order = np.argsort(_field(keys, 0, 24), kind="stable")
        gk, gv, passes = ctx.debug_radix_sort_pairs(keys, vals, 0, 24)
        assert passes == runs, const_byte
        _assert_same(gk, keys[order], RS_TILE, f"constant byte {const_byte} keys")
        _assert_same(gv, vals[order], RS_TILE, f"constant byte {const_byte} values")


# ---- host only: the argument checks come before any device call ---------------------------------------------------------
def test_primitive_hooks_check_their_arguments(built):
    from flye_amd import gpu
    L = gpu.load_library()
    a = np.arange(16, dtype=np.uint64)
    v = np.arange(16, dtype=np.uint64)
    p = C.c_int(-7)
    # a null context, everything else in order
    assert L.fg_debug_scan(None, a.ctypes.data, 16, 8, 0, 1) == FG_ERR_ARG
    assert L.fg_debug_radix_sort_pairs(None, a.ctypes.data, v.ctypes.data, 16, 0, 64, C.byref(p)) == FG_ERR_ARG
    # the calls below are refused on their other arguments: the stand-in context is never looked at
    fake = C.create_string_buffer(1 << 16)
    h = C.cast(fake, C.c_void_p)
    assert L.fg_debug_scan(h, None, 1, 8, 0, 1) == FG_ERR_ARG
    for eb in (0, 1, 2, 3, 5, 7, 16, -4):
        assert L.fg_debug_scan(h, a.ctypes.data, 4, eb, 0, 1) == FG_ERR_ARG, eb
    assert L.fg_debug_radix_sort_pairs(h, None, v.ctypes.data, 16, 0, 64, C.byref(p)) == FG_ERR_ARG
    assert L.fg_debug_radix_sort_pairs(h, a.ctypes.data, None, 16, 0, 64, C.byref(p)) == FG_ERR_ARG
    for b, e in ((-1, 8), (0, 65), (9, 8), (64, 0), (-8, -1), (65, 66)):
        assert L.fg_debug_radix_sort_pairs(h, a.ctypes.data, v.ctypes.data, 16, b, e, C.byref(p)) == FG_ERR_ARG, (b, e)
    assert L.fg_debug_radix_sort_pairs(h, a.ctypes.data, v.ctypes.data, 1 << 30, 0, 64, C.byref(p)) == FG_ERR_ARG
    assert L.fg_debug_radix_sort_pairs(h, a.ctypes.data, v.ctypes.data, 1 << 40, 0, 64, None) == FG_ERR_ARG
    assert a.tolist() == list(range(16)) and v.tolist() == list(range(16)) and p.value == -7
