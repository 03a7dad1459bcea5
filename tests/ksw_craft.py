"""Crafted (target, query) pairs for the three forms of the ksw_extz2 recurrence in fg_ksw.hip, and the dispatcher's
class rule restated (tests only).

The rule (fg_ksw.hip, kswAlignDevice): the band of a pair is the smallest of 64, 128, 256, ... that holds the length
difference; a pair takes a windowed kernel (state in registers, or in LDS rings under FG_KSW_REG=0) iff the target
rounded up to 16 is longer than band + 32 and the band is at most 512, else the literal kernel (state in memory).
Windowed classes 1..4 = bands 64..512, instantiated with RING = 256, 256, 512, 1024 bytes of target / query ring
and direction rows staged G = 8, 8, 4, 2 at a time.

cases() places pairs on both sides of every class edge, around every ring wrap, at every residue of the stage flush,
at the 64-lane look-ahead and the tile edges of the backtrack, on the tie rules and on band-edge paths; assert_claims()
checks that the cases are what they say.  Everything is seeded and uses bases 0..3 only.
"""
from __future__ import annotations

import zlib

import numpy as np

from helpers import edit_pair

BANDS = (64, 128, 256, 512)                 # the windowed classes 1..4
RING = {1: 256, 2: 256, 3: 512, 4: 1024}
G = {1: 8, 2: 8, 3: 4, 4: 2}
TILE_BYTES = 4096                           # the backtrack stages tiles of 4096 / rowBytes direction rows
SEED = 20261020


def band(tlen, qlen):
    """The band getAlignmentCigarKsw ends with (alignment.cpp:147-159: 64, doubled while ksw_extz2 finds it too
    narrow -- the last anti-diagonal decides), or 0 for an empty string."""
    if not tlen or not qlen:
        return 0
    w = 64
    while True:
        r = qlen + tlen - 2
        st = max(0, r - qlen + 1, (r - w + 1) >> 1)
        en = min(tlen - 1, r, (r + w) >> 1)
        if st <= en or w > max(qlen, tlen):
            return w
        w *= 2


def kernel_class(tlen, qlen):
    """0: the literal kernel; 1..4: the windowed kernel of band 64..512."""
    w = band(tlen, qlen)
    if not w or w > 512:
        return 0
    t16 = (tlen + 15) // 16 * 16
    if t16 <= w + 32:
        return 0
    return BANDS.index(w) + 1


def low_edge(w):
    """The smallest length difference of band w."""
    return 0 if w == 64 else w // 2 + 1


def row_bytes(tlen, qlen):
    """Bytes of one row of the direction matrix (fg_ksw.hip: nCol * 16)."""
    n = min(tlen, qlen, band(tlen, qlen) + 1)
    return ((n + 15) // 16 + 1) * 16


def _rng(name):
    return np.random.default_rng([SEED, zlib.crc32(name.encode())])


def rand(rng, n):
    return rng.integers(0, 4, size=int(n), dtype=np.uint8)


def substitute(rng, s, rate):
    s = s.copy()
    hit = rng.random(len(s)) < rate
    s[hit] = (s[hit] + 1 + rng.integers(0, 3, size=int(hit.sum()), dtype=np.uint8)) & 3
    return s


def related(name, tlen, qlen, where="mid", sub=0.03):
    """A random target of tlen and a query of qlen: the target with the whole length difference as ONE block of random
    bases put in (query longer) or cut out (target longer) at the start, the end or the middle, then substitutions at
    rate ``sub``."""
    rng = _rng(name)
    t = rand(rng, tlen)
    d = qlen - tlen
    n = min(tlen, qlen)
    at = {"start": 0, "end": n, "mid": n // 2}[where]
    if d >= 0:
        q = np.concatenate([t[:at], rand(rng, d), t[at:]])
    else:
        q = np.concatenate([t[:at], t[at - d:]])
    q = substitute(rng, q, sub)
    assert (len(t), len(q)) == (tlen, qlen)
    return t, q


def class_lengths(c, k):
    """The k-th of the smallest length pairs of class c (k >= 0): the shorter string 0..3 above the class's shortest,
    the difference 0..3 above the class's smallest, the longer side alternating.  Class 0: tiny strings."""
    if c == 0:
        return 17 + k % 29, 17 + (7 * k) % 31
    w = BANDS[c - 1]
    short = w + 33 + k % 4
    long_ = short + low_edge(w) + (k // 4) % 4
    return (short, long_) if k % 2 == 0 else (long_, short)


def class_batch(c, n=61):
    """n distinct pairs of class c at the class's smallest lengths (the second-job batches tile them)."""
    out = []
    for k in range(n):
        tlen, qlen = class_lengths(c, k)
        assert kernel_class(tlen, qlen) == c
        out.append(related(f"batch/c{c}/{k}", tlen, qlen, where=("start", "mid", "end")[k % 3], sub=0.05))
    return out


def cases():
    """[(name, target, query)]: see the module text; the name's first part is the group."""
    out = []

    def add(name, t, q):
        out.append((name, np.ascontiguousarray(t, np.uint8), np.ascontiguousarray(q, np.uint8)))

    def add_related(name, tlen, qlen, **kw):
        add(name, *related(name, tlen, qlen, **kw))

    # ---- lengths at every class edge: both sides of T16 > w + 32, tlen mod 16 in {0, 1, 15}, the band's edges ----
    for w in BANDS:
        lo = low_edge(w)
        for tlen in (w + 32, w + 33, w + 47, w + 48, w + 49):
            for d in (lo, lo + 1, w - 1, w):
                for sign in (1, -1):
                    if d == 0 and sign < 0:
                        continue
                    add_related(f"edge/w{w}/t{tlen}/d{sign * d:+d}", tlen, tlen + sign * d)
    for tlen, qlen in ((600, 1113), (1113, 600), (545, 1058), (1200, 175), (175, 1200), (1100, 2125)):
        add_related(f"edge/wide/t{tlen}/q{qlen}", tlen, qlen)       # differences 513 and 1025: bands 1024 and 2048

    # ---- ring wrap: the target ring, and with the query longer the query ring as well ----
    for c in (1, 2, 3, 4):
        r, d = RING[c], low_edge(BANDS[c - 1]) + 2
        for tlen in (r - 1, r, r + 1, r + 63, r + 64, r + 65, 2 * r + 65):
            for sign in (-1, 1):
                add_related(f"ring/c{c}/t{tlen}/d{sign * d:+d}", tlen, tlen + sign * d)

    # ---- stage flush: every residue of (qlen + tlen - 1) mod G ----
    for c in (1, 2, 3, 4):
        w = BANDS[c - 1]
        tlen = w + 86
        for k in range(G[c]):
            add_related(f"flush/c{c}/k{k}", tlen, tlen + low_edge(w) + 4 + k)

    # ---- the 64-lane match look-ahead and the tile edges of the backtrack ----
    rows = TILE_BYTES // row_bytes(1500, 1500)          # rows per tile for identical strings longer than the band
    ident = [63, 64, 65, 127, 128, 129] + [rows * k + s for k in (1, 2, 3, 4) for s in (-1, 1)] + [1500]
    for n in sorted(set(ident)):
        s = rand(_rng(f"ident/{n}"), n)
        add(f"ident/{n}", s, s.copy())
    for n in (129, 4 * rows + 1, 1500):
        s = rand(_rng(f"ident/{n}"), n)
        # columns of a decode step from the string's start; columns before the end (the first look-ahead takes cells
        # n-1 .. n-64); half a tile of rows before the end (a diagonal step is two rows)
        places = [63, 64, n - 64, n - 65, n - 66, n - 1 - rows // 2, n - rows // 2, n - 2 - rows // 2]
        for i, p in enumerate(dict.fromkeys(places)):
            x = s.copy()
            x[p] = (x[p] + 1) & 3
            add(f"look/sub/{n}/p{p}", s, x)
            if i % 3 == 2:          # every third place: a deletion (the query lacks base p)
                add(f"look/del/{n}/p{p}", s, np.delete(s, p))
            else:                   # a 1-base insertion that differs from both neighbours' continuation
                add(f"look/ins/{n}/p{p}", s, np.insert(s, p, (s[p] + 2) & 3))

    # ---- tie rules: the strict-greater direction choice ----
    for a, b in ((100, 120), (120, 100), (300, 200), (50, 60), (700, 180)):
        add(f"tie/homo/{a}x{b}", np.zeros(a, np.uint8), np.zeros(b, np.uint8))
    for a, b in ((100, 100), (97, 97), (200, 201), (301, 200)):
        add(f"tie/acac/{a}x{b}", np.tile(np.array([0, 1], np.uint8), a)[:a], np.tile(np.array([1, 0], np.uint8), b)[:b])
    for unit, reps in ((7, 20), (13, 30), (3, 150), (90, 6)):
        u = rand(_rng(f"tie/tandem/{unit}"), unit)
        add(f"tie/tandem/{unit}x{reps}/more", np.tile(u, reps), np.tile(u, reps + 1))
        add(f"tie/tandem/{unit}x{reps}/less", np.tile(u, reps + 1), np.tile(u, reps))
    for i, (n, m) in enumerate(((100, 100), (97, 160), (300, 350), (700, 1000), (1000, 480))):
        add(f"tie/unrelated/{n}x{m}", *edit_pair(dict(seed=SEED + i, n=n, err=1.0, m=m)))
    for n, m in ((100, 100), (130, 200)):
        add(f"tie/nomatch/{n}x{m}", np.zeros(n, np.uint8), np.ones(m, np.uint8))

    # ---- band-edge paths: the whole difference as one block; the backtrack's forced steps ----
    for w in BANDS:
        for d in (w, w - 1):
            for where in ("start", "end", "mid"):
                short = w + 100
                add_related(f"bandedge/w{w}/d{d}/{where}/query", short, short + d, where=where, sub=0.0)
                add_related(f"bandedge/w{w}/d{d}/{where}/target", short + d, short, where=where, sub=0.0)

    # ---- tiny strings: the literal kernel's piece-by-piece path ----
    seen = set()
    for a in (1, 2, 15, 16, 17):
        for b in (1, 17, 64, 65, 66):
            for tlen, qlen in ((a, b), (b, a)):
                if (tlen, qlen) not in seen:
                    seen.add((tlen, qlen))
                    add_related(f"tiny/{tlen}x{qlen}", tlen, qlen, where="end", sub=0.1)

    # ---- noise: edit_pair at two error rates inside each class (n, shift: the middle of the class's differences) ----
    shape = {0: (1500, 750), 1: (300, 20), 2: (400, 96), 3: (600, 192), 4: (1000, 384)}
    for c in range(5):
        n, shift = shape[c]
        for err in (0.02, 0.15):
            for k in range(4):
                a, b = edit_pair(dict(seed=SEED + 100 * c + 10 * k + int(err * 100), n=n + 37 * k, err=err, shift=shift))
                if k % 2:
                    a, b = b, a
                add(f"noise/c{c}/e{err}/{k}", a, b)
    return out


def assert_claims(cs):
    """The cases are what they say (see cases())."""
    names = [n for n, _, _ in cs]
    assert len(set(names)) == len(names)
    assert 400 <= len(cs) <= 600
    shapes = []
    for name, t, q in cs:
        assert len(t) > 0 and len(q) > 0, name                                   # no pair is empty
        assert max(len(t), len(q)) <= 2400, name
        assert t.dtype == np.uint8 and q.dtype == np.uint8 and t.max() <= 3 and q.max() <= 3, name
        shapes.append((name, len(t), len(q), band(len(t), len(q)), kernel_class(len(t), len(q))))
    assert {c for *_, c in shapes} == {0, 1, 2, 3, 4}
    assert {w for _, _, _, w, _ in shapes} == {64, 128, 256, 512, 1024, 2048}
    # the band is a function of the length difference alone
    for _, tlen, qlen, w, _ in shapes:
        assert abs(qlen - tlen) <= w and (w == 64 or abs(qlen - tlen) > w // 2)
    for c in (1, 2, 3, 4):
        w = BANDS[c - 1]
        mine = [(tlen, qlen) for _, tlen, qlen, ww, _ in shapes if ww == w]
        # both sides of T16 > w + 32, the target longer and the query longer; the class is what the side says
        for t16, cls in ((w + 32, 0), (w + 48, c)):
            side = [(tlen, qlen) for tlen, qlen in mine if (tlen + 15) // 16 * 16 == t16]
            assert all(kernel_class(tlen, qlen) == cls for tlen, qlen in side)
            assert any(qlen > tlen for tlen, qlen in side) and any(qlen < tlen for tlen, qlen in side), (w, t16)
        assert {w + 32, w + 33} <= {tlen for tlen, _ in mine}
        # both edges of the band, in both signs
        diffs = {qlen - tlen for tlen, qlen in mine}
        lo = low_edge(w)
        assert {lo, -lo, lo + 1, -lo - 1, w - 1, 1 - w, w, -w} <= diffs, w
        inside = [(tlen, qlen) for _, tlen, qlen, _, cc in shapes if cc == c]
        assert {(tlen + qlen - 1) % G[c] for tlen, qlen in inside} == set(range(G[c])), c
        assert any(tlen > 2 * RING[c] for tlen, _ in inside), c
        assert any(qlen > 2 * RING[c] for _, qlen in inside), c
    # a case that names its class is in it
    for name, tlen, qlen, _, c in shapes:
        part = name.split("/")
        if part[0] in ("ring", "flush", "noise"):
            assert c == int(part[1][1:]), name
        if part[0] == "tiny":
            assert c == 0, name
