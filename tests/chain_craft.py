"""Crafted read sets and honest indexes whose target groups have exactly the sizes and shapes a chaining
case asks for (tests only).

Every case is built from random sequence (17-mers unique) that is copied, shifted, cut and repeated; the
index holds a chosen set of canonical k-mers, each with ALL of its occurrences in the read set (positions
0 .. len-k-1 of every forward read: the reference never yields the last k-mer, kmer.h), strand bit and
position in the k-mer's canonical orientation, lists ascending.  Group structure therefore comes only from
which keys are present and from how the sequences are built.

A case declares up front, per (query record, target record) group, the exact hit list (cur, ext) its
construction creates -- including the query's hits on itself inside tandem repeats (trivial self hits
skipped) and hits on odd (reverse-complement) records -- and from it the prefilter verdict of
overlap.cpp:216-262.  tests/test_chain_craft.py checks those declarations against a direct enumeration and
against the oracle's counters; tests/test_chain_classes.py runs the device against the oracle on them.
"""
from __future__ import annotations

import numpy as np

K = 17
MIN_OVERLAP = 1000          # the detector's minOverlap (config.DETECTOR_MIN_OVERLAP)
MAX_JUMP = 1500             # raw preset maximum_jump
MAX_OVERHANG = 1500         # raw preset maximum_overhang
MIN_UNIQUE = float(np.float32(0.01) * np.float32(MIN_OVERLAP))   # minKmerSruvivalRate * minOverlap, in float
MIN_SIZE = int(np.ceil(MIN_UNIQUE))                             # smallest group that can reach it (10)
FIN_CAP_S = 256             # fg_chain.hip size classes
PREP_CAP = 320
FIN_CAP_M = 1024


def revcomp(x):
    return (3 - np.asarray(x, np.uint8)[::-1]).astype(np.uint8)


def kmer_codes(seq, k=K):
    """(forward, reverse-complement) codes of the k-mers at positions 0 .. len-k-1 (kmer.h order: first
    base most significant)."""
    b = np.asarray(seq, np.uint64)
    n = len(b) - k
    if n <= 0:
        return np.empty(0, np.uint64), np.empty(0, np.uint64)
    fw = np.zeros(n, np.uint64)
    rv = np.zeros(n, np.uint64)
    for t in range(k):
        fw = (fw << np.uint64(2)) | b[t:t + n]
        rv = rv | ((np.uint64(3) - b[t:t + n]) << np.uint64(2 * t))
    return fw, rv


def prefilter(hits, cur_len, ext_len, force_local=False):
    """overlap.cpp:220-262 on a group's hits sorted by cur: (listed by k_group_list, passes)."""
    cur = np.sort(np.asarray([h[0] for h in hits], np.int64))
    ext = np.asarray([h[1] for h in hits], np.int64)
    n = len(cur)
    uniq = int(np.count_nonzero(cur != np.concatenate([[0], cur[:-1]])))   # prevPos starts at 0
    listed = n >= MIN_SIZE and cur[-1] - cur[0] >= MIN_OVERLAP
    ok = uniq >= MIN_UNIQUE and cur[-1] - cur[0] >= MIN_OVERLAP and ext.max() - ext.min() >= MIN_OVERLAP
    if ok and not force_local:
        ok = (min(cur[0], ext.min()) <= MAX_OVERHANG and
              min(cur_len - cur[-1], ext_len - ext.max()) <= MAX_OVERHANG)
    return bool(listed), bool(ok)


class Case:
    """Reads, key set, queries and the declared groups of one crafted case.

    ``groups[(q, t)]`` = list of (cur, ext) hits, record ids relative to the container (add first_id for
    FastaRecord ids); ``runs`` lists the detector / call variants the device tests use."""

    def __init__(self, name, seed, first_id=0, runs=None):
        self.name, self.first_id = name, first_id
        self.rng = np.random.default_rng(seed)
        self.seqs, self.key_codes, self.groups, self.queries = [], [], {}, []
        self.runs = runs or [dict()]

    # ---- construction ---------------------------------------------------------------------------
    def rand(self, n):
        return self.rng.integers(0, 4, size=int(n), dtype=np.uint8)

    def add_read(self, seq):
        self.seqs.append(np.ascontiguousarray(seq, np.uint8))
        return len(self.seqs) - 1

    def add_keys(self, seq, positions):
        fw, rv = kmer_codes(seq)
        p = np.asarray(positions, np.int64)
        self.key_codes.append(np.minimum(fw[p], rv[p]))

    def declare(self, q, t, hits):
        assert (q, t) not in self.groups
        self.groups[(q, t)] = [(int(c), int(e)) for c, e in hits]
        if q not in self.queries:
            self.queries.append(q)

    def rec_len(self, rec):
        return len(self.seqs[rec >> 1])

    # ---- the crafted index ----------------------------------------------------------------------
    def readset(self):
        from flye_amd import synth
        return synth.ReadSet.from_arrays(self.seqs)

    def index(self):
        """IndexExport (keys ascending, key_off, entries = record << 32 | position, no repetitive k-mers)."""
        from oracle import oracle as O
        keys = np.unique(np.concatenate(self.key_codes)) if self.key_codes else np.empty(0, np.uint64)
        kk, ee = [], []
        for r, s in enumerate(self.seqs):
            fw, rv = kmer_codes(s)
            if not len(fw):
                continue
            can = np.minimum(fw, rv)
            pos = np.nonzero(np.isin(can, keys))[0]
            flip = rv[pos] < fw[pos]
            rec = 2 * r + flip.astype(np.int64)
            p = np.where(flip, len(s) - pos - K, pos)
            kk.append(can[pos])
            ee.append((rec.astype(np.uint64) << np.uint64(32)) | p.astype(np.uint64))
        kk = np.concatenate(kk) if kk else np.empty(0, np.uint64)
        ee = np.concatenate(ee) if ee else np.empty(0, np.uint64)
        order = np.lexsort((ee, kk))
        kk, ee = kk[order], ee[order]
        assert np.array_equal(np.unique(kk), keys), "a key of the case occurs nowhere"
        off = np.zeros(len(keys) + 1, np.uint64)
        off[1:] = np.searchsorted(kk, keys, side="right").astype(np.uint64)
        return O.IndexExport(np.ascontiguousarray(keys), off, np.ascontiguousarray(ee), np.empty(0, np.uint64))

    # ---- what the case declares -----------------------------------------------------------------
    def query_ids(self):
        return (np.asarray(self.queries, np.int64) + self.first_id).astype(np.uint32)

    def verdicts(self, force_local=False):
        """{(q, t): (n, listed, passes)}."""
        return {g: (len(h),) + prefilter(h, self.rec_len(g[0]), self.rec_len(g[1]), force_local)
                for g, h in self.groups.items()}

    def totals(self, force_local=False):
        """(seed_hits, dp_groups, dp_elements) the oracle must count for the case's queries."""
        v = self.verdicts(force_local)
        return (sum(n for n, _, _ in v.values()), sum(1 for _, _, p in v.values() if p),
                sum(n for n, _, p in v.values() if p))

    def sizes(self, force_local=False):
        """(listed group sizes, passing group sizes)."""
        v = self.verdicts(force_local)
        return [n for n, l, _ in v.values() if l], [n for n, _, p in v.values() if p]


def enumerate_groups(case):
    """Seed collection of overlap.cpp:176-196 on the crafted index, in plain Python: {(q, t): sorted hits}."""
    ex = case.index()
    keys = ex.keys
    off = ex.key_off.astype(np.int64)
    out = {}
    for q in case.queries:
        seq = case.seqs[q >> 1]
        s = revcomp(seq) if q & 1 else seq
        fw, rv = kmer_codes(s)
        can = np.minimum(fw, rv)
        idx = np.searchsorted(keys, can)
        ok = idx < len(keys)
        ok[ok] &= keys[idx[ok]] == can[ok]
        for p in np.nonzero(ok)[0]:
            flip = bool(rv[p] < fw[p])
            i = int(idx[p])
            for e in ex.entries[off[i]:off[i + 1]]:
                rec, pos = int(e >> np.uint64(32)), int(e & np.uint64(0xFFFFFFFF))
                if flip:
                    rec ^= 1
                    pos = case.rec_len(rec) - pos - K
                if rec == q and pos == p:
                    continue
                out.setdefault((q, rec), []).append((int(p), pos))
    return {g: sorted(h) for g, h in out.items()}


# ---- building blocks ---------------------------------------------------------------------------------
def pair(case, seg_len, offsets, left_q=500, right_q=300, left_t=200, rel=1, rc=False, dups=(), strays=0,
         edits=(), both_strands=False, q_read=None, t_len=None):
    """A query read holding a random segment S at ``left_q`` and a target read holding S (with ``edits``:
    (segment offset, +len insertion / -len deletion)) at ``left_t``; keys: the k-mers of the query at
    S offsets ``offsets``; ``dups``: offsets whose k-mer is copied once more into the target's tail (one
    extra hit each, off the diagonal, at a query position that already has one); ``strays``: k-mers of the
    query's left flank copied into the target's tail and keyed (hits at query positions of their own whose
    target positions break the ascending order).  The target is ``rel`` bases longer than the query
    (ext-sorted groups: rel > 0; None: as short as it can be) or ``t_len`` long; ``rc``: the target read is stored reverse-complemented (hits land on its odd
    record).  Returns (query read, target read)."""
    S = case.rand(seg_len)
    offsets = np.asarray(offsets, np.int64)
    assert len(np.unique(offsets)) == len(offsets) and offsets.min() >= 0 and offsets.max() + K <= seg_len
    # the target's copy of S with its edits, and where each key lands in it
    tseg, shift = [], np.zeros(len(offsets), np.int64)
    prev = 0
    for o, d in sorted(edits):
        tseg.append(S[prev:o])
        assert not np.any((offsets < o) & (offsets + K > o)), "a key k-mer spans an edit"
        if d > 0:
            tseg.append(case.rand(d))
            prev = o
        else:
            assert not np.any((offsets >= o) & (offsets < o - d)), "a key k-mer lies in a deletion"
            prev = o - d
        shift += np.where(offsets >= o, d, 0)
    tseg.append(S[prev:])
    tseg = np.concatenate(tseg)
    if q_read is None:
        Q = np.concatenate([case.rand(left_q), S, case.rand(right_q)])
        qr = case.add_read(Q)
    else:       # S written into an existing query read at left_q
        qr = q_read
        Q = case.seqs[qr]
        Q[left_q:left_q + seg_len] = S
    tail = [case.rand(40)]
    extra = []          # (query position, target position)
    base = left_t + len(tseg) + 40
    stray_pos = [20 + 30 * i for i in range(strays)]
    assert not stray_pos or stray_pos[-1] + K <= left_q
    for qp in [left_q + int(o) for o in dups] + stray_pos:
        tail += [Q[qp:qp + K], case.rand(40)]
        extra.append((qp, base))
        base += K + 40
    body = np.concatenate([case.rand(left_t), tseg] + tail)
    pad = t_len - len(body) if t_len is not None else 1 if rel is None else len(Q) + rel - len(body)
    assert pad >= 1, "target too short for the requested length relation"
    F = np.concatenate([body, case.rand(pad)])
    tr = case.add_read(revcomp(F) if rc else F)
    case.add_keys(Q, np.concatenate([left_q + offsets, np.asarray(stray_pos, np.int64)]))
    hits = [(left_q + o, left_t + o + s) for o, s in zip(offsets, shift)] + extra
    t_rec = 2 * tr + (1 if rc else 0)
    case.declare(2 * qr, t_rec, hits)
    if both_strands:        # the query's reverse complement: the mirrored group on the other target strand
        Lq, Lt = len(Q), len(F)
        case.declare(2 * qr + 1, t_rec ^ 1, [(Lq - c - K, Lt - e - K) for c, e in hits])
    return qr, tr


def spread(n, span):
    """n distinct offsets from 0 to span, as evenly as integers allow."""
    o = np.unique(np.round(np.linspace(0, span, n)).astype(np.int64))
    assert len(o) == n, (n, span)
    return o


def tandem_pair(case, m, r_q, r_t, flank=700, key_step=50, left_q=300, right_q=300, left_t=200, rel=1):
    """Query and target share flank L, a tandem array, flank R; the query's array has r_q copies of an
    m-base motif, the target's r_t.  Keys: every k-mer of the arrays (m distinct ones) and every
    key_step-th k-mer of the flanks.  Each query k-mer of the array hits every target position of the
    same phase (deep look-backs; equal target positions when r_q > r_t), and the query hits itself inside
    its own array."""
    motif = case.rand(m)
    FL, FR = case.rand(flank), case.rand(flank)
    FL[-1] = (motif[-1] + 1) & 3         # no k-mer across an array's end continues the period
    FR[0] = (motif[0] + 1) & 3

    def arr(r):
        return np.tile(motif, r)
    Aq, At = arr(r_q), arr(r_t)
    Q = np.concatenate([case.rand(left_q), FL, Aq, FR, case.rand(right_q)])
    body = np.concatenate([case.rand(left_t), FL, At, FR, case.rand(40)])
    pad = len(Q) + rel - len(body)
    assert pad >= 1
    T = np.concatenate([body, case.rand(pad)])
    qr, tr = case.add_read(Q), case.add_read(T)
    fo = np.arange(0, flank - K + 1, key_step)
    q_fl, q_arr, q_fr = left_q, left_q + flank, left_q + flank + len(Aq)
    t_fl, t_arr, t_fr = left_t, left_t + flank, left_t + flank + len(At)
    case.add_keys(Q, np.concatenate([q_fl + fo, q_fr + fo, q_arr + np.arange(m)]))
    pq = np.arange(len(Aq) - K + 1)
    pt = np.arange(len(At) - K + 1)
    hits = [(q_fl + o, t_fl + o) for o in fo] + [(q_fr + o, t_fr + o) for o in fo]
    hits += [(q_arr + a, t_arr + b) for a in pq for b in pt if (a - b) % m == 0]
    case.declare(2 * qr, 2 * tr, hits)
    self_hits = [(q_arr + a, q_arr + b) for a in pq for b in pq if a != b and (a - b) % m == 0]
    if self_hits:
        case.declare(2 * qr, 2 * qr, self_hits)
    return qr, tr


# ---- the cases ---------------------------------------------------------------------------------------
SIZES = {"sizes_s": [10, 63, 64, 65, 255, 256],
         "sizes_m": [257, 320, 321, 448],
         "sizes_l": [449, 1024, 1025, 4096, 4097, 6000]}


def sizes_case(name, seed):
    """Exact group sizes, each as ext-sorted (target one base longer) and unsorted (same length, one
    shorter) groups, with target positions strictly ascending (collinear copy) or not (one extra hit
    of a key copied into the target's tail)."""
    c = Case(name, seed, runs=[dict(), dict(only_max=False)])
    for n in SIZES[name]:
        for rel in (1, 0, -1):
            for asc in (True, False):
                seg = max(1300, n + 60)
                nk = n if asc else n - 1
                offs = spread(nk, seg - K - 20)
                pair(c, seg, offs, rel=rel, rc=(asc and rel == 0), strays=0 if asc else 1)
    return c


def prefilter_case():
    """One group on each side of each prefilter boundary (distinct query positions, query and target span,
    both overhangs), small (LDS prefilter) and > 320 hits (global-memory prefilter); run with and without
    forceLocal.  first_id != 0."""
    c = Case("prefilter", 31, first_id=1000, runs=[dict(), dict(force_local=True)])
    # distinct query positions: minUnique - 1 and minUnique with n >= minSize (a key hit twice)
    for nu in (MIN_UNIQUE - 1, MIN_UNIQUE):
        offs = spread(int(nu), 1100)
        pair(c, 1200, offs, dups=(int(offs[3]),))
    # ... a hit at query position 0 is not counted (prevPos starts at 0)
    pair(c, 1200, spread(MIN_SIZE, 1100), left_q=0)
    pair(c, 1200, spread(MIN_SIZE + 1, 1100), left_q=0)
    # ... > 320 hits from 9 / 10 distinct positions: every key copied 40 times into the target
    for nu in (MIN_UNIQUE - 1, MIN_UNIQUE):
        offs = spread(int(nu), 1100)
        pair(c, 1200, offs, dups=[int(o) for o in offs for _ in range(39)], rel=None)
    # query / target span at minOverlap - 1 and minOverlap
    for span in (MIN_OVERLAP - 1, MIN_OVERLAP):
        pair(c, 1100, spread(12, span))
    # cur span minOverlap, target span one shorter (a deleted base) / cur one short, target full (an insertion)
    pair(c, 1100, spread(12, MIN_OVERLAP), edits=[(500, -1)])
    pair(c, 1100, spread(12, MIN_OVERLAP + 1), edits=[(500, -1)])
    pair(c, 1100, spread(12, MIN_OVERLAP - 1), edits=[(500, 1)])
    # left overhang at maxOverhang, maxOverhang + 1 (min of the two starts)
    for lq in (MAX_OVERHANG, MAX_OVERHANG + 1):
        pair(c, 1200, spread(20, 1150), left_q=lq, left_t=1600)
        pair(c, 1200, spread(400, 1150), left_q=lq, left_t=1600, right_q=300)   # global-memory prefilter
    # right overhang: query end - last hit at maxOverhang, maxOverhang + 1 (the target's tail is longer)
    for rq in (MAX_OVERHANG, MAX_OVERHANG + 1):
        # last key at seg offset 1150: curLen - maxCur = (seg_len - 1150) + right_q
        pair(c, 1200, spread(20, 1150), left_q=100, right_q=rq - 50, left_t=100, rel=400)
    return c


def dp_case():
    """DP edges: same-diagonal gaps k-1, k, k+1 (the dc < k early exit), cur gaps maxJump-1 .. +1 between
    two runs, indels of 100 and 101 bases (the gap cost changes form at |dc - de| = 100); ext-sorted and
    not, both query strands."""
    c = Case("dp", 47, runs=[dict(), dict(only_max=False)])
    for rel in (1, -1):
        for g in (K - 1, K, K + 1):
            pair(c, 1400, np.arange(0, 1300, g), rel=rel, both_strands=True)
        for j in (MAX_JUMP - 1, MAX_JUMP, MAX_JUMP + 1):
            run = np.arange(0, 12 * 20, 20)
            pair(c, 2 * 240 + j, np.concatenate([run, run[-1] + j + run]), rel=rel, both_strands=True)
        for d in (100, 101):
            run = np.arange(0, 30 * 20, 20)
            second = run[-1] + 150 + d + run
            pair(c, int(second[-1]) + 60, np.concatenate([run, second]), edits=[(int(run[-1]) + 40, d)],
                 rel=rel, both_strands=True)
            pair(c, int(second[-1]) + 60, np.concatenate([run, second]), edits=[(int(run[-1]) + 40, -d)],
                 rel=rel, both_strands=True)
    return c


def tandem_case():
    """Deep look-backs: tandem arrays in query and target within maxJump, groups over 320, 1024 and 4096
    hits (through the LDS ring, into memory, across tile 64 = position 4096)."""
    c = Case("tandem", 53, runs=[dict(), dict(only_max=False)])
    tandem_pair(c, 25, 6, 6)
    tandem_pair(c, 40, 8, 8)
    tandem_pair(c, 40, 8, 8, rel=-1)
    tandem_pair(c, 50, 12, 12)
    return c


def ties_case():
    """Equal target positions (a query tandem array against a single target copy of the motif; ext-sorted,
    so the groups are re-sorted by target position with many ties) at group sizes in the fused kernel, the
    LDS prefilter and the global-memory prefilter; and targets holding two exact copies of the query
    segment (chains of equal score), at three sizes; with only_max_ext 0 / 1 and a max_overlaps limit."""
    c = Case("ties", 61, runs=[dict(), dict(only_max=False), dict(max_overlaps=2), dict(only_max=False, max_overlaps=3)])
    for r in (5, 10, 20):
        tandem_pair(c, 40, r, 1)
    for nk in (40, 150, 600):
        seg = max(1300, nk + 60)
        offs = spread(nk, seg - K - 20)
        S_len = seg
        qr, tr = pair(c, S_len, offs, left_t=200, rel=S_len + 800)
        # second exact copy of the segment further along the target
        S = c.seqs[qr][500:500 + S_len]
        T = c.seqs[tr]
        at = 200 + S_len + 300
        T[at:at + S_len] = S
        h = c.groups[(2 * qr, 2 * tr)]
        h += [(500 + int(o), at + int(o)) for o in offs]
    return c


def key_mode_case(name, n_reads):
    """curBits + recBits = 32 (n_reads = 2048) or 33 (2049): a 530 kb query (20 position bits) whose end
    overlaps two targets, and short filler reads."""
    c = Case(name, 71 if n_reads == 2048 else 73)
    L = 530_000
    q = c.add_read(c.rand(L))
    pair(c, 1300, spread(100, 1250), left_q=L - 3000, q_read=q, t_len=1700)
    pair(c, 1300, spread(600, 1250), left_q=L - 1500, q_read=q, t_len=1800)
    while len(c.seqs) < n_reads:
        c.add_read(c.rand(60))
    return c


KEY33_HIGH_CUR_BITS = 20    # a 530 kb query: 20 position bits beside the 13 record bits of 2049 reads


def key33_high_case(name, first_id=0):
    """The key33 construction with the target records at the top of the record range: 2046 short filler reads first,
    then the 530 kb query (read 2046; 20 position bits, 13 record bits: 33 key bits) and its two targets, reads 2047
    and 2048, the second stored reverse-complemented.  The hit keys ``record << 20 | cur`` of the one query then lie
    below 2^32 on record 4094 and at or above it on the odd record 4097: its segment straddles 2^32.  ``first_id``:
    the packed form keys on ext_id - first_id, the 64-bit key + value form on ext_id itself."""
    c = Case(name, 79, first_id=first_id)
    L = 530_000
    while len(c.seqs) < 2046:
        c.add_read(c.rand(60))
    q = c.add_read(c.rand(L))
    pair(c, 1300, spread(100, 1250), left_q=L - 3000, q_read=q, t_len=1700)
    pair(c, 1300, spread(600, 1250), left_q=L - 1500, q_read=q, t_len=1800, rc=True)
    assert len(c.seqs) == 2049 and sorted(t for _, t in c.groups) == [2 * 2047, 2 * 2048 + 1]
    return c


def hit_key_range(case, cur_bits):
    """(smallest, largest) ``record << cur_bits | cur`` over the declared hits of every query"""
    keys = [(t << cur_bits) | cur for (_, t), hits in case.groups.items() for cur, _ in hits]
    return min(keys), max(keys)


CASE_NAMES = ["sizes_s", "sizes_m", "sizes_l", "prefilter", "dp", "tandem", "ties", "key32", "key33", "key33_high",
              "key33_high_id"]


def make_case(name):
    return {"sizes_s": lambda: sizes_case("sizes_s", 11), "sizes_m": lambda: sizes_case("sizes_m", 13),
            "sizes_l": lambda: sizes_case("sizes_l", 17), "prefilter": prefilter_case, "dp": dp_case,
            "tandem": tandem_case, "ties": ties_case, "key32": lambda: key_mode_case("key32", 2048),
            "key33": lambda: key_mode_case("key33", 2049),
            "key33_high": lambda: key33_high_case("key33_high"),
            "key33_high_id": lambda: key33_high_case("key33_high_id", first_id=1000)}[name]()
