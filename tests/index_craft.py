"""Read sets crafted for the edges of the index build (flye_amd/csrc/fg_index.hip), the build parameters each one is
run with, and numpy restatements that say what a case shows.  The restatements are only ever used to assert the
PURPOSE of a case (that a threshold of 2047 exists, that a k-mer sits at exactly tandemFreq + 1 copies, ...); the
yardstick for the device is the oracle, pinned to the reference by tests/golden/index_edges.json
(tests/golden/make_index_edge_golden.py).

Cases (``case(name)`` -> Case, seeded, a few hundred ms to construct):

``threshold``   k_threshold: per-read thresholds of exactly 2046 / 2047 / 2048 / 5000 (the histogram's last bin holds
                every frequency >= 2047; above it the kernel bisects on the values), reads that mix two families so
                that the rank falls on the upper one (the exact threshold decides what is kept) or on the lower one
                (ties keep more than maxKmers), reads with nk = L - k of <= 0, 1, 2 (maxKmers == 0) and 255 .. 257
                (one block is 256 threads).
``tandem13`` / ``tandem17``   k_mark / k_tandem_insert / k_tandem_apply: a motif at tandemFreq and tandemFreq + 1
                copies in two reads, the count made up of forward and reverse-complement copies, a motif that only
                ever occurs in the read that drops it, one that is tandem in one read and kept in three others.
``lists``       k_accept / filterFrequentKmers / k_classify / k_finalize: keys whose capacity stays at or below
                _repetitiveFrequency while their global frequency exceeds it (kept, with an empty list), repetitive
                keys, capacity == _repetitiveFrequency against + 1, frequency 1 / 2 / 3 against min_freq.
``windows13`` / ``windows12``   k_minimizers at windows 1, 2, 10, 63, 64: equal hashes inside one window (periods
                below the window, homopolymers), stretches of thousands of positions without a sync point, reads
                shorter than k + w, palindromic k-mers (k = 12).
"""
import collections
import functools
import hashlib

import numpy as np

from helpers import canonical_kmers

Case = collections.namedtuple("Case", "name k reads seqs psets marks")


# ---- parameter sets ------------------------------------------------------------------------------------------------------
def solid(k, rate, tandem, repeat, min_freq=2):
    return dict(mode="solid", k=k, rate=rate, tandem=tandem, repeat=repeat, min_freq=min_freq)


def mini(k, window, repeat=100.0):
    return dict(mode="min", k=k, window=window, repeat=repeat)


def pset_name(p):
    if p["mode"] == "solid":
        return f"solid_k{p['k']}_rate{p['rate']:g}_tandem{p['tandem']}_repeat{p['repeat']:g}_minfreq{p['min_freq']}"
    return f"min_k{p['k']}_w{p['window']}_repeat{p['repeat']:g}"


def has_reference(p):
    """the reference program fixes min_freq = 2, and its flat counter takes 90 s (8 GiB) at k = 17"""
    return p["mode"] == "min" or (p["min_freq"] == 2 and p["k"] != 17)


def cfg_of(p):
    """The parameter set as a config dict (for the calls that take one: they use min_freq 2)."""
    from flye_amd import config
    cfg = config.preset("raw")
    cfg["kmer_size"] = float(p["k"])
    cfg["repeat_kmer_rate"] = float(np.float32(p["repeat"]))
    if p["mode"] == "solid":
        cfg.update(use_minimizers=0.0, meta_read_top_kmer_rate=float(np.float32(p["rate"])),
                   meta_read_filter_kmer_freq=float(p["tandem"]))
    else:
        cfg.update(use_minimizers=1.0, minimizer_window=float(p["window"]))
    return cfg


def ref_params(p):
    """--params of the reference dumper: the raw preset with the set's values"""
    from flye_amd import config
    d = dict(config.PRESETS["raw"])
    d.update(kmer_size=p["k"], repeat_kmer_rate=p["repeat"])
    if p["mode"] == "solid":
        d.update(use_minimizers=0, meta_read_top_kmer_rate=p["rate"], meta_read_filter_kmer_freq=p["tandem"])
    else:
        d.update(use_minimizers=1, minimizer_window=p["window"])
    return ",".join(f"{k}={v!r}" if isinstance(v, float) else f"{k}={v}" for k, v in d.items())


def oracle_build(o, p):
    if p["mode"] == "solid":
        return o.build_index_solid(p["min_freq"], p["rate"], p["tandem"], p["repeat"], 1.0)
    return o.build_index_minimizers(1, p["window"], p["repeat"])


def device_build(vi, p):
    if p["mode"] == "solid":
        vi.countKmers()
        return vi.buildIndexUnevenCoverage(p["min_freq"], p["rate"], p["tandem"], p["repeat"])
    return vi.buildIndexMinimizers(1, p["window"], p["repeat"])


def reads_sha256(rs):
    return hashlib.sha256(rs.words.tobytes() + rs.length.tobytes()).hexdigest()


# ---- constructions ----------------------------------------------------------------------------------------------------------
def revcomp(x):
    return (3 - np.asarray(x, np.uint8)[::-1]).astype(np.uint8)


def _rand(rng, n):
    return rng.integers(0, 4, size=n, dtype=np.uint8)


def _motif_read(rng, parts, filler, length=None):
    """filler, then every part followed by filler (fresh random bases each time); padded with random bases to
    ``length``"""
    out = [_rand(rng, filler)]
    for m in parts:
        out += [m, _rand(rng, filler)]
    s = np.concatenate(out)
    if length is not None:
        assert len(s) <= length
        s = np.concatenate([s, _rand(rng, length - len(s))])
    return s


def _finish(name, k, seqs, **marks):
    from flye_amd import synth
    return Case(name, k, synth.ReadSet.from_arrays(seqs), seqs, PSETS[name], marks)


THRESHOLD_COPIES = (2046, 2047, 2048, 5000)


def _threshold():
    k = 13
    rng = np.random.default_rng(7102)
    motifs = [_rand(rng, 30) for _ in THRESHOLD_COPIES]
    used = [0] * len(motifs)
    seqs = []

    def add(spec, filler, length=None):
        parts = []
        for m, c in spec:
            parts += [motifs[m]] * c
            used[m] += c
        seqs.append(_motif_read(rng, parts, filler, length))

    # the rank on the UPPER family: the exact threshold decides whether the lower one is kept
    add([(2, 9), (1, 1)], 6)        # 162 k-mers at 2048 above maxKmers = 141: threshold 2048, the 2047 copy is dropped
    add([(3, 9), (2, 1)], 6)        # threshold 5000 over a 2048 copy
    # the rank on the LOWER family with the upper one above it: ties keep 180 positions for maxKmers = 167
    add([(1, 5), (0, 5)], 12)       # threshold 2046 (last histogram bin but one), 2047 above
    add([(2, 5), (1, 5)], 12)       # threshold 2047 (the overflow bin's lowest value), 2048 above
    add([(3, 5), (2, 5)], 12)       # threshold 2048, 5000 above
    for nk in (255, 256, 257):      # one block of 256 threads and one position less / more
        add([(3, 6)], 12, length=k + nk)
    # nk = 2, 2, 2, 1, 0, -1.  s[0:13] occurs in four reads, s[1:14] in two: maxKmers = 0 keeps the most frequent only
    s = _rand(rng, 14)
    short = [np.concatenate([s, [0]]), np.concatenate([s, [1]]), np.concatenate([s[:13], _rand(rng, 2)]),
             np.concatenate([s[:13], _rand(rng, 1)]), _rand(rng, k), _rand(rng, k - 1)]
    seqs += short
    for m, total in enumerate(THRESHOLD_COPIES):        # at most 10 copies per read (tandemFreq)
        left = total - used[m]
        while left:
            c = min(10, left)
            add([(m, c)], 12)
            left -= c
    assert used == list(THRESHOLD_COPIES)
    return _finish("threshold", k, seqs, motifs=motifs, short=s, first_short=8)


def _tandem(k):
    rng = np.random.default_rng(7200 + k)
    a, b, c, d = (_rand(rng, 30) for _ in range(4))
    rb = revcomp(b)
    seqs = [_motif_read(rng, [a] * 10, 12), _motif_read(rng, [a] * 11, 12),                  # 0, 1: tandemFreq, + 1
            _motif_read(rng, [b, rb] * 5 + [b], 12), _motif_read(rng, [b, rb] * 5, 12),      # 2, 3: 6 + 5 and 5 + 5
            _motif_read(rng, [c] * 11, 12),                                                  # 4: global = local = 11
            _motif_read(rng, [d] * 11, 12)]                                                  # 5: tandem here ...
    for _ in range(3):                                                                       # 6 .. 8: ... kept here
        seqs.append(np.concatenate([_rand(rng, 190), d, _rand(rng, 180)]))
    genome = _rand(rng, 1200)
    seqs += [genome[s:s + 600].copy() for s in range(0, 601, 60)]
    return _finish(f"tandem{k}", k, seqs, motifs=dict(a=a, b=b, c=c, d=d))


LISTS_RATES = (100.0, 5.0, 2.0)


def _lists():
    k = 13
    rng = np.random.default_rng(7302)
    big, hidden, pair, triple = (_rand(rng, 30) for _ in range(4))
    seqs = []
    for i in range(300):        # 162 k-mers of `big` above maxKmers = 150: the threshold is big's, `hidden` is not selected
        parts = [big] * 9
        parts.insert(i % 10, hidden)
        seqs.append(_motif_read(rng, parts, 8))
    for i in range(3):          # threshold 1: everything is selected; `hidden` reaches capacity 3 at frequency 303
        x = [_rand(rng, 150), hidden, _rand(rng, 150), triple]
        if i < 2:
            x += [_rand(rng, 100), pair]                  # frequency exactly 2
        x = np.concatenate(x)
        seqs.append(np.concatenate([x, _rand(rng, 630 - len(x))]))
    genome = _rand(rng, 3000)
    seqs += [genome[s:s + 1000].copy() for s in range(0, 2000, 100)]
    return _finish("lists", k, seqs, motifs=dict(big=big, hidden=hidden, pair=pair, triple=triple))


# _repetitiveFrequency = rate * (sum of capacities / (keys + 1)) must land inside the capacities of the tiled reads
# (1 .. 4 at their ends, 10 in the middle): the mean is dominated by the 18 keys of `big` at capacity 2700 (about 35
# over some 1700 keys), so 0.1 gives 3 -- capacity 3 stays, capacity 4 is repetitive
LISTS_FOURTH_RATE = 0.1

WINDOWS = (1, 2, 10, 63, 64)
WINDOWS_SOLID = ((0.75, 0, 3.0), (0.75, 0, 1.0), (0.1, 3, 2.0))


def _windows(k):
    rng = np.random.default_rng(7400)       # the same stream for both k: only the lengths around k differ
    seqs = [_rand(rng, k + d) for d in (-1, 0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513)]
    seqs.append(np.zeros(3000, np.uint8))
    seqs.append(np.concatenate([_rand(rng, 300), np.full(700, 1, np.uint8), _rand(rng, 300)]))
    for period in (1, 2, 3, 5, 7, 20, 70):
        unit = _rand(rng, period)
        while period > 1 and len(set(unit.tolist())) == 1:
            unit = _rand(rng, period)
        arr = np.tile(unit, 1500 // period + 1)[:1500]
        seqs.append(np.concatenate([_rand(rng, 100), arr, _rand(rng, 100)]))
    acgt = np.tile(np.array([0, 1, 2, 3], np.uint8), 200)      # ACGTACGTACGT is its own reverse complement
    seqs.append(np.concatenate([_rand(rng, 150), acgt, _rand(rng, 150)]))
    genome = _rand(rng, 4000)
    seqs += [genome[s:s + 1000].copy() for s in np.linspace(0, 3000, 12).astype(int)]
    seqs.append(revcomp(genome[1200:2100]))
    return _finish(f"windows{k}", k, seqs)


CASE_NAMES = ("threshold", "tandem13", "tandem17", "lists", "windows13", "windows12")


@functools.lru_cache(maxsize=None)
def case(name):
    return {"threshold": _threshold, "tandem13": lambda: _tandem(13), "tandem17": lambda: _tandem(17), "lists": _lists,
            "windows13": lambda: _windows(13), "windows12": lambda: _windows(12)}[name]()


def all_sets():
    """every (case name, parameter set name) in a fixed order -- importable without constructing the reads"""
    return [(n, pset_name(p)) for n in CASE_NAMES for p in PSETS[n]]


def pset(name, pname):
    return next(p for p in PSETS[name] if pset_name(p) == pname)


PSETS = {
    "threshold": [solid(13, 0.40, 10, 100.0), solid(13, 0.40, 10, 1.5)],
    "tandem13": [solid(13, 0.40, 10, 100.0), solid(13, 0.40, 0, 100.0)],
    "tandem17": [solid(17, 0.40, 10, 100.0), solid(17, 0.40, 0, 100.0)],
    "lists": [solid(13, 0.40, 10, r) for r in LISTS_RATES + (LISTS_FOURTH_RATE,)]
             + [solid(13, 0.40, 10, 5.0, min_freq=1), solid(13, 0.40, 10, 5.0, min_freq=3)],
    "windows13": [mini(13, w) for w in WINDOWS] + [solid(13, r, t, rep) for r, t, rep in WINDOWS_SOLID],
    "windows12": [mini(12, w) for w in WINDOWS] + [solid(12, r, t, rep) for r, t, rep in WINDOWS_SOLID],
}


# ---- restatements (fresh, numpy; they assert what a case shows and nothing else) ----------------------------------------------
class Counts:
    """canonical k-mer, global frequency and per-read local frequency of every k-mer position the reference
    iterates (nk = L - k per read: kmer.h:185-198 stops one short)"""

    def __init__(self, rs, k):
        self.per_read = [canonical_kmers(rs, r, k)[:-1] for r in range(rs.n)]
        self.nk = np.array([len(x) for x in self.per_read], np.int64)
        self.off = np.concatenate([[0], np.cumsum(self.nk)])
        self.canon = np.concatenate(self.per_read) if rs.n else np.empty(0, np.uint64)
        self.keys, inv, cnt = np.unique(self.canon, return_inverse=True, return_counts=True)
        self.freq = cnt[inv].astype(np.int64)
        self.local = np.zeros(len(self.canon), np.int64)
        for r in range(rs.n):
            _, li, lc = np.unique(self.per_read[r], return_inverse=True, return_counts=True)
            self.local[self.off[r]:self.off[r + 1]] = lc[li]

    def of(self, r):
        return slice(int(self.off[r]), int(self.off[r + 1]))

    def freq_of(self, kmer):
        return int((self.canon == np.uint64(kmer)).sum())


def max_kmers(rate, nk):
    """vertex_index.cpp:339: a float multiply, truncated"""
    return int(np.float32(rate) * np.float32(nk))


def thresholds(cnt, rate):
    """per read: (maxKmers, threshold) of vertex_index.cpp:336-340; (0, None) for a read without k-mers"""
    out = []
    for r in range(len(cnt.nk)):
        f = np.sort(cnt.freq[cnt.of(r)])[::-1]
        if not len(f):
            out.append((0, None))
            continue
        m = max_kmers(rate, len(f))
        out.append((m, int(f[m])))
    return out


def yielded(cnt, p):
    """bool per position: what yieldFrequentKmers returns for the read (selected by the threshold, not tandem)"""
    keep = np.zeros(len(cnt.canon), bool)
    for r, (_, t) in enumerate(thresholds(cnt, p["rate"])):
        if t is not None:
            keep[cnt.of(r)] = cnt.freq[cnt.of(r)] >= t
    if p["tandem"] > 0:
        keep &= ~(cnt.local > p["tandem"])
    return keep


def capacities(cnt, p):
    """(keys, capacity) of _kmerIndex before filterFrequentKmers (vertex_index.cpp:46-56)"""
    take = yielded(cnt, p) & (cnt.freq >= p["min_freq"])
    return np.unique(cnt.canon[take], return_counts=True)


def repetitive_frequency(caps, min_coverage, rate):
    """filterFrequentKmers (vertex_index.cpp:175-186): float arithmetic, stored in a size_t"""
    caps = np.asarray(caps, np.int64)
    counted = caps[caps >= min_coverage]
    mean = np.float32(np.float32(int(counted.sum())) / np.float32(len(counted) + 1))
    return int(np.float32(rate) * mean)


def kmer_hash(x):
    """Kmer::hash (kmer.h:91-98)"""
    with np.errstate(over="ignore"):
        z = np.asarray(x, np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def sketch(hashes, w):
    """positions yieldMinimizers returns (kmer.h:222-258, the literal deque loop)"""
    n = len(hashes)
    if w == 1:
        return list(range(n))
    hs = [int(h) for h in hashes]
    q = collections.deque()
    out = []
    for p in range(n):
        h = hs[p]
        while q and q[-1][1] > h:
            q.pop()
        q.append((p, h))
        if q[0][0] <= p - w:
            while q[0][0] <= p - w:
                q.popleft()
            while len(q) >= 2 and q[0][1] == q[1][1]:
                q.popleft()
        if not out or out[-1] != q[0][0]:
            out.append(q[0][0])
    return out


def sync_points(hashes, w):
    """bool per position: strictly below the (up to) w previous hashes -- where the deque collapses to one entry"""
    h = np.asarray(hashes, np.uint64)
    ok = np.ones(len(h), bool)
    for d in range(1, w + 1):
        ok[d:] &= h[:-d] > h[d:] if d < len(h) else True
    return ok


def longest_gap(flags):
    """longest run of False"""
    idx = np.nonzero(np.concatenate([[True], flags, [True]]))[0]
    return int(np.diff(idx).max()) - 1 if len(idx) > 1 else 0


def equal_hash_in_window(hashes, w):
    h = np.asarray(hashes, np.uint64)
    return any(bool((h[:-d] == h[d:]).any()) for d in range(1, min(w, len(h))))


def sketch_entries(cnt, w, rate):
    """(accepted positions, entries of the minimizer index) by the restated sketch and filter (minCoverage 1,
    vertex_index.cpp:408-442)"""
    sel = []
    for r in range(len(cnt.nk)):
        c = cnt.per_read[r]
        sel.append(c[sketch(kmer_hash(c), w)] if len(c) else c)
    sel = np.concatenate(sel)
    _, caps = np.unique(sel, return_counts=True)
    rep = repetitive_frequency(caps, 1, rate)
    return len(sel), int(caps[caps <= rep].sum())


def key_lists(ix):
    """{key: tuple of entries} of an exported index"""
    off = ix.key_off.astype(np.int64)
    return {int(k): tuple(ix.entries[off[i]:off[i + 1]].tolist()) for i, k in enumerate(ix.keys)}


def canon_of(seq, k):
    """canonical codes of ALL k-mers of a 0..3 array (the last one included)"""
    b = np.asarray(seq, np.uint64)
    n = len(b) - k + 1
    fw = np.zeros(n, np.uint64)
    rv = np.zeros(n, np.uint64)
    for t in range(k):
        fw = (fw << np.uint64(2)) | b[t:t + n]
        rv = rv | ((np.uint64(3) - b[t:t + n]) << np.uint64(2 * t))
    return np.minimum(fw, rv), fw, rv
