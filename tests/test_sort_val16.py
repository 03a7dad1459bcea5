"""The hit sort with 16-bit values (fg_debug_sort_pairs32_val16): 32-bit keys ``rec << cur_bits | cur`` beside a
uint16 value array, the form the overlap stage takes when every target position fits 16 bits.

One call sorts segments laid back to back, one per route of sortSegments at its edges:

* 2, 16, 17, 63, 64, 65 hits: the register sort of at most one wave (sort_small, inside k_sort_lds);
* 447, 448 (the LDS piece), 449 (one streamed level first);
* 8191, 8192 (streamed partition), 8193 (one-wave closed form);
* 16384 (closed form), 16385 and 40001 (a workgroup per piece, k_sort_wide);
* flagged tie-free: 449 and 65536 (k_sort_radix), 65537 (back in the level loop).

The unflagged segments hold many duplicate keys, the values are random with 0 and 65535 planted, and every one of
these segments starts at an odd index (a one-hit segment stands in front where the sum of the lengths would be even):
its first value shares a 32-bit word with the last value of the segment in front, which another wave (or workgroup)
owns, and so does the last value of every segment of even length.  A store that wrote a whole word there would damage
the neighbour: the test asks that every segment keeps its multiset of (key, value) pairs, that the arrays equal
``oracle.std_sort_perm`` applied per segment, and that they equal what the 32-bit value path (fg_debug_sort_pairs32)
gives on the same input."""
import numpy as np
import pytest

SORT_CAP = 448
RADIX_MAX = 65536
CUR_BITS = REC_BITS = 16

# (hits, flagged tie-free)
SEGMENTS = [(2, False), (16, False), (17, False), (63, False), (64, False), (65, False),
            (447, False), (448, False), (449, False),
            (8191, False), (8192, False), (8193, False),
            (16384, False), (16385, False), (40001, False),
            (449, True), (65536, True), (65537, True)]


def _distinct_keys(rng, n):
    """n distinct keys in emission order: cur ascending, the records of one cur ascending"""
    codes = np.empty(0, np.int64)
    while len(codes) < n:
        codes = np.unique(np.concatenate([codes, rng.integers(0, 1 << 32, size=n + n // 4 + 16)]))
    codes = np.sort(rng.permutation(codes)[:n])          # cur << 16 | rec
    return (((codes & 0xFFFF) << CUR_BITS) | (codes >> 16)).astype(np.uint32)


def _duplicate_keys(rng, n):
    """keys over 4 records and about n / 6 positions, any order: most keys several times"""
    rec = rng.integers(0, 4, size=n)
    cur = rng.integers(0, max(2, n // 24), size=n)
    return ((rec << CUR_BITS) | cur).astype(np.uint32)


def _input():
    rng = np.random.default_rng(20261)
    keys, flags, off = [], [], [0]
    for n, flagged in SEGMENTS:
        if off[-1] % 2 == 0:                             # a one-hit segment: nothing to sort, a value to keep
            keys.append(rng.integers(0, 1 << 32, size=1).astype(np.uint32))
            flags.append(0)
            off.append(off[-1] + 1)
        keys.append(_distinct_keys(rng, n) if flagged else _duplicate_keys(rng, n))
        flags.append(1 if flagged else 0)
        off.append(off[-1] + n)
    keys = np.concatenate(keys)
    vals = rng.integers(0, 1 << 16, size=len(keys)).astype(np.uint16)
    for a, b in zip(off[:-1], off[1:]):                  # both ends of the range in every segment, at its edges too
        if b - a < 2:
            continue
        vals[a], vals[b - 1] = 0xFFFF, 0
        if b - a > 4:
            vals[a + 1], vals[b - 2] = 0, 0xFFFF
    return keys, vals, np.asarray(off, np.uint64), np.asarray(flags, np.uint32)


@pytest.fixture(scope="module")
def sorted16(built):
    """(input, output of the 16-bit call, output of the 32-bit call) -- one call each, shared by the tests"""
    import os
    from flye_amd import gpu
    saved = {sw: os.environ.pop(sw) for sw in ("FG_SORT_TIEFREE", "FG_SORT_RADIX_MAX", "FG_SORT_STREAM_MAX", "FG_SORT_WIDE_MIN",
                                               "FG_SORT_MANY_MIN", "FG_SORT_STREAM_MANY") if sw in os.environ}
    keys, vals, off, flags = _input()
    ctx = gpu.Context(17, 0)
    got16 = ctx.debug_sort_pairs32_val16(keys, vals, off, CUR_BITS, REC_BITS, flags)
    got32 = ctx.debug_sort_pairs32(keys, off, CUR_BITS, REC_BITS, flags)
    ctx.close()
    os.environ.update(saved)
    return (keys, vals, off, flags), got16, got32


def test_input_is_what_the_docstring_says():
    keys, vals, off, flags = _input()
    size = np.diff(off.astype(np.int64))
    assert [int(n) for n in size[size > 1]] == [n for n, _ in SEGMENTS]
    assert np.all(off[:-1][size > 1] % 2 == 1)                # neighbouring segments share a 32-bit word of values
    assert vals.min() == 0 and vals.max() == 0xFFFF
    for i in np.nonzero(size > 1)[0]:
        seg, n, flagged = keys[int(off[i]):int(off[i + 1])], int(size[i]), flags[i] != 0
        if flagged:
            assert len(np.unique(seg)) == n and np.all(np.diff((seg & 0xFFFF).astype(np.int64)) >= 0)
        elif n > 64:
            assert len(np.unique(seg)) < n // 2


@pytest.mark.gpu
def test_every_segment_keeps_its_pairs(sorted16):
    (keys, vals, off, flags), (k, v, segs, hits), _ = sorted16
    assert v.dtype == np.uint16 and len(v) == len(vals)
    before = (keys.astype(np.uint64) << np.uint64(16)) | vals.astype(np.uint64)
    after = (k.astype(np.uint64) << np.uint64(16)) | v.astype(np.uint64)
    for i in range(len(off) - 1):
        a, b = int(off[i]), int(off[i + 1])
        assert np.array_equal(np.sort(before[a:b]), np.sort(after[a:b])), (i, b - a)
        assert np.all(np.diff(k[a:b].astype(np.int64)) >= 0), (i, b - a)
    # the flagged segments of a size the radix path takes went there
    n = np.diff(off.astype(np.int64))
    took = (flags != 0) & (n > SORT_CAP) & (n <= RADIX_MAX)
    assert (segs, hits) == (int(took.sum()), int(n[took].sum())) == (2, 449 + 65536)


@pytest.mark.gpu
def test_order_is_std_sort_s(sorted16):
    from oracle import oracle as O
    (keys, vals, off, flags), (k, v, _, _), _ = sorted16
    for i in range(len(off) - 1):
        a, b = int(off[i]), int(off[i + 1])
        perm = O.std_sort_perm(keys[a:b].astype(np.uint64))
        assert np.array_equal(k[a:b], keys[a:b][perm]), (i, b - a)
        assert np.array_equal(v[a:b], vals[a:b][perm]), (i, b - a)


@pytest.mark.gpu
def test_equal_to_the_32_bit_value_path(sorted16):
    (keys, vals, off, flags), (k, v, segs, hits), (k32, perm32, segs32, hits32) = sorted16
    assert k.tobytes() == k32.tobytes()
    base = np.repeat(off[:-1].astype(np.int64), np.diff(off.astype(np.int64)))
    assert np.array_equal(v, vals[base + perm32.astype(np.int64)])
    assert (segs, hits) == (segs32, hits32)
