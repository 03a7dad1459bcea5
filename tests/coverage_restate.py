"""Yardstick and inputs of tests/test_coverage.py.

No program built from the reference prints coverage vectors, so ChimeraDetector's window coverage (reference
src/assemble/chimera.cpp:106-202, :280-343) and the first half of MultiplicityInferer::estimateCoverage
(src/repeat_graph/multiplicity_inferer.cpp:14-41, :63) are restated twice, independently:

* ``restate_reads`` / ``restate_edges`` below: numpy difference arrays, ``np.float32`` for the float steps;
* ``tests/native/coverage_driver.cpp``: the loops as the reference writes them, on ``std::vector::at``, with
  ``std::sort``, ``std::ceil`` on float and ``std::lround`` (``native_reads`` / ``native_edges``).

The CPU test pins that the two agree on every case; the device is compared with them."""
import math
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT32_MAX = 2 ** 31 - 1
READ_FIELDS = ("win_off", "full", "junction", "sum", "max", "median", "min_good", "threshold", "chimeric", "degenerate")
EDGE_FIELDS = ("win_off", "cov", "sum", "max", "median")
COLS = ("cur_id", "ext_id", "cur_begin", "cur_end", "cur_len", "ext_begin", "ext_end", "ext_len")
PARAMS = dict(window=100, max_overhang=500, max_drop_rate=5.0, overlap_coverage=10, uneven_coverage=0)


class ReadBatch:
    """Per-read record lists with the reads' lengths: what fg_read_coverage takes."""

    def __init__(self, queries, params=None):
        """queries: a list of (length, [(cur_id, ext_id, cur_begin, cur_end, cur_len, ext_begin, ext_end, ext_len), ...])"""
        self.params = dict(PARAMS, **(params or {}))
        self.query_len = np.array([q[0] for q in queries], np.int32)
        self.query_off = np.zeros(len(queries) + 1, np.uint64)
        self.query_off[1:] = np.cumsum([len(q[1]) for q in queries])
        self.table = np.array([r for q in queries for r in q[1]], np.int64).reshape(-1, 8)

    @property
    def n_queries(self):
        return len(self.query_len)

    def recs(self):
        """The records as fg_overlap_rec (the fields the step does not read are filled in plausibly)."""
        from flye_amd import gpu
        r = np.zeros(len(self.table), gpu.REC_DTYPE)
        for j, f in enumerate(COLS):
            r[f] = self.table[:, j]
        r["score"] = r["cur_end"] - r["cur_begin"]
        r["edit_distance"] = -1
        return r

    def coverage_params(self, want_vectors=True):
        from flye_amd import gpu
        return gpu.CoverageParams(want_vectors=int(want_vectors), **self.params)


def rec(cb, ce, cl, eb=0, ee=None, el=None, cur_id=1000, ext_id=2000):
    """A record; by default the ext side leaves no overhang on either end (ext_begin = 0, ext_end = ext_len)."""
    el = (ce - cb) + eb if el is None else el
    ee = el if ee is None else ee
    return (cur_id, ext_id, cb, ce, cl, eb, ee, el)


# ---- numpy form -----------------------------------------------------------------------------------------------------
def windows(seq_len, window):
    """(vector size, degenerate): chimera.cpp:114-117 in single precision"""
    num = int(np.float32(np.ceil(np.float32(seq_len) / np.float32(window))) + np.float32(1))
    n = num - 2
    return (1, True) if n <= 0 else (n, False)


def max_flank(max_overhang, window):
    return int(np.float32(int(max_overhang)) / np.float32(window))


def lround(x):
    x = float(x)
    return int(math.floor(abs(x) + 0.5)) * (1 if x >= 0 else -1)


def verdict(P, n_windows, total, median, min_good):
    """(threshold, chimeric): chimera.cpp:153-182"""
    if total == 0:
        return 0, True
    x = np.float32(median) if P["uneven_coverage"] else np.float32(P["overlap_coverage"])
    thr = max(1, lround(x / np.float32(P["max_drop_rate"])))
    flank = max_flank(P["max_overhang"], P["window"])
    good_start, good_end = flank, n_windows - flank - 1
    return thr, bool(good_end <= good_start or min_good < thr)


def cdiv(a, b):
    """C's integer division on arrays (b > 0)"""
    a = np.asarray(a, np.int64)
    return np.where(a >= 0, a // b, -((-a) // b))


def restate_reads(batch):
    P = batch.params
    W = int(P["window"])
    flank = max_flank(P["max_overhang"], W)
    out = {k: [] for k in READ_FIELDS}
    win_off = [0]
    off = batch.query_off.astype(np.int64)
    for q in range(batch.n_queries):
        n, deg = windows(int(batch.query_len[q]), W)
        t = batch.table[off[q]:off[q + 1]]
        diff = np.zeros((2, n + 1), np.int64)
        if not deg and len(t):
            cur, ext, cb, ce, cl, eb, ee, el = t.T
            keep = (ext != cur) & (ext != (cur ^ 1))
            hang = np.maximum(np.minimum(cb, eb), np.minimum(cl - ce, el - ee))
            cls = (hang > P["max_overhang"]).astype(np.int64)
            lo, hi = cb // W, ce // W - 1                   # windows lo .. hi - 1
            keep &= hi > lo
            assert (hi[keep] <= n).all(), "a window past the vector: the reference's .at() throws"
            np.add.at(diff, (cls[keep], lo[keep]), 1)
            np.add.at(diff, (cls[keep], hi[keep]), -1)
        full, junction = np.cumsum(diff[:, :n], axis=1)
        good = full[flank:max(n - flank, flank)] if n - flank - 1 >= flank else full[:0]
        med = int(np.sort(full)[min(n * 50 // 100, n - 1)])
        mn = int(good.min()) if len(good) else INT32_MAX
        thr, chim = verdict(P, n, int(full.sum()), med, mn)
        win_off.append(win_off[-1] + n)
        for k, v in (("full", full), ("junction", junction)):
            out[k].append(v)
        for k, v in (("sum", int(full.sum())), ("max", int(full.max())), ("median", med), ("min_good", mn), ("threshold", thr),
                     ("chimeric", chim), ("degenerate", deg)):
            out[k].append(v)
    res = dict(win_off=np.array(win_off, np.uint64),
               full=np.concatenate(out["full"]).astype(np.int32) if out["full"] else np.zeros(0, np.int32),
               junction=np.concatenate(out["junction"]).astype(np.int32) if out["junction"] else np.zeros(0, np.int32),
               sum=np.array(out["sum"], np.int64))
    for k in ("max", "median", "min_good", "threshold"):
        res[k] = np.array(out[k], np.int32)
    for k in ("chimeric", "degenerate"):
        res[k] = np.array(out[k], bool)
    return res


class EdgeBatch:
    """Read paths over graph edges: what fg_edge_coverage takes.  alns: (ext_id, ext_begin, ext_end) per record; paths:
    lists of record indices."""

    def __init__(self, window, alns, paths, first_ext_id, edge_of, edge_len):
        self.window, self.first_ext_id = int(window), int(first_ext_id)
        self.table = np.array(alns, np.int64).reshape(-1, 3)
        self.aln_off = np.zeros(len(paths) + 1, np.uint64)
        self.aln_off[1:] = np.cumsum([len(p) for p in paths])
        self.aln = np.array([i for p in paths for i in p], np.uint64)
        self.edge_of = np.ascontiguousarray(edge_of, np.uint32)
        self.edge_len = np.ascontiguousarray(edge_len, np.int32)

    def recs(self):
        from flye_amd import gpu
        r = np.zeros(len(self.table), gpu.REC_DTYPE)
        r["ext_id"], r["ext_begin"], r["ext_end"] = self.table.T
        r["ext_len"] = np.maximum(r["ext_end"], 0) + 5
        r["cur_id"] = 900000
        return r


def restate_edges(batch):
    W = batch.window
    size = (batch.edge_len.astype(np.int64) // W)
    win_off = np.zeros(len(size) + 1, np.int64)
    win_off[1:] = np.cumsum(size)
    diff = np.zeros(int(win_off[-1]) + len(size), np.int64)          # one spare slot per edge for the -1 at its end
    base = win_off[:-1] + np.arange(len(size))
    off = batch.aln_off.astype(np.int64)
    if len(batch.aln):
        idx = batch.aln.astype(np.int64)
        path = np.repeat(np.arange(len(off) - 1), np.diff(off))
        j = np.arange(len(idx)) - off[path]
        m = np.diff(off)[path]
        ext, eb, ee = batch.table[idx].T
        e = batch.edge_of[ext - batch.first_ext_id].astype(np.int64)
        frm = np.where(j > 0, 0, np.maximum(0, cdiv(eb, W) + 1))
        to = np.where(j < m - 1, size[e], np.minimum(size[e], cdiv(ee, W)))
        keep = frm < to
        np.add.at(diff, base[e[keep]] + frm[keep], 1)
        np.add.at(diff, base[e[keep]] + to[keep], -1)
    cov, total, mx, med = [], [], [], []
    for e in range(len(size)):
        v = np.cumsum(diff[base[e]:base[e] + size[e]])
        cov.append(v)
        total.append(int(v.sum()))
        mx.append(int(v.max()) if len(v) else 0)
        med.append(int(np.sort(v)[min(len(v) * 50 // 100, len(v) - 1)]) if len(v) else 0)
    return dict(win_off=win_off.astype(np.uint64), cov=np.concatenate(cov).astype(np.int32) if cov else np.zeros(0, np.int32),
                sum=np.array(total, np.int64), max=np.array(mx, np.int32), median=np.array(med, np.int32))


def same(a, b, fields):
    return [k for k in fields if not np.array_equal(np.asarray(a[k]).astype(np.int64), np.asarray(b[k]).astype(np.int64))] == []


# ---- the literal form -----------------------------------------------------------------------------------------------
_DRIVER = {}


def native_driver():
    if "exe" not in _DRIVER:
        d = tempfile.mkdtemp(prefix="coverage_driver_")
        exe = os.path.join(d, "coverage_driver")
        subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", os.path.join(ROOT, "tests", "native", "coverage_driver.cpp"), "-o", exe],
                       check=True)
        _DRIVER["exe"] = exe
    return _DRIVER["exe"]


def write_reads_input(batch, path):
    P = batch.params
    with open(path, "wb") as f:
        np.array([0, P["window"], P["max_overhang"], P["overlap_coverage"], P["uneven_coverage"]], np.int32).tofile(f)
        np.array([P["max_drop_rate"]], np.float32).tofile(f)
        np.array([batch.n_queries], np.uint32).tofile(f)
        np.array([len(batch.table)], np.uint64).tofile(f)
        batch.query_len.tofile(f)
        batch.query_off.tofile(f)
        batch.table.astype(np.int32).tofile(f)


def _take(raw, p, n, dtype):
    size = np.dtype(dtype).itemsize * n
    return raw[p:p + size].view(dtype).copy(), p + size


def native_reads(batch, threads=1, repeats=1):
    """The same ten arrays from tests/native/coverage_driver.cpp; ["seconds"] is its best wall time."""
    exe = native_driver()
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        write_reads_input(batch, src)
        r = subprocess.run([exe, src, dst, str(threads), str(repeats)], check=True, capture_output=True, text=True)
        raw = np.fromfile(dst, np.uint8)
    nq = batch.n_queries
    res = {}
    res["win_off"], p = _take(raw, 0, nq + 1, np.uint64)
    nw = int(res["win_off"][nq])
    for k, n, dt in (("full", nw, np.int32), ("junction", nw, np.int32), ("sum", nq, np.int64), ("max", nq, np.int32),
                     ("median", nq, np.int32), ("min_good", nq, np.int32), ("threshold", nq, np.int32), ("chimeric", nq, np.uint8),
                     ("degenerate", nq, np.uint8)):
        res[k], p = _take(raw, p, n, dt)
    assert p == len(raw)
    res["seconds"] = float(r.stdout.split()[-1])
    return res


def native_edges(batch):
    exe = native_driver()
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(src, "wb") as f:
            np.array([1, batch.window], np.int32).tofile(f)
            np.array([len(batch.edge_len), len(batch.edge_of), batch.first_ext_id], np.uint32).tofile(f)
            np.array([len(batch.table), len(batch.aln_off) - 1, len(batch.aln)], np.uint64).tofile(f)
            batch.edge_len.tofile(f)
            batch.edge_of.tofile(f)
            batch.table.astype(np.int32).tofile(f)
            batch.aln_off.tofile(f)
            batch.aln.tofile(f)
        subprocess.run([exe, src, dst], check=True, capture_output=True, text=True)
        raw = np.fromfile(dst, np.uint8)
    ne = len(batch.edge_len)
    res = {}
    res["win_off"], p = _take(raw, 0, ne + 1, np.uint64)
    nw = int(res["win_off"][ne])
    for k, n, dt in (("cov", nw, np.int32), ("sum", ne, np.int64), ("max", ne, np.int32), ("median", ne, np.int32)):
        res[k], p = _take(raw, p, n, dt)
    assert p == len(raw)
    return res


# ---- crafted read batches -------------------------------------------------------------------------------------------
def span(first, last, cl, w=100, **kw):
    """a record that covers exactly the windows first .. last of a read of cl bases"""
    return rec(first * w, min((last + 2) * w, cl), cl, **kw)


def crafted_reads():
    """name -> ReadBatch"""
    B = {}
    # window counts 1 (degenerate: lengths 0, 1, 100), one real window (101), 63 / 64 / 65, 255 / 256 / 257; queries
    # without records in between
    qs = [(0, [rec(0, 0, 0)]), (1, [rec(0, 1, 1)]), (100, [rec(0, 100, 100)]), (101, [rec(0, 101, 101)] * 3), (101, [])]
    for n in (63, 64, 65, 255, 256, 257):
        cl = (n + 1) * 100
        qs.append((cl, [span(0, n - 1, cl), span(1, n - 2, cl), span(n - 1, n - 1, cl), span(n // 2, n - 1, cl), span(0, 0, cl)]))
        qs.append((cl - 37, []))
    B["window_counts"] = ReadBatch(qs)
    # lrOverhang() = max_overhang (full) and one above (junction), through each of its four terms
    qs = []
    for hang in (50, 51):
        qs.append((5000, [rec(hang, 2000, 5000, eb=200, el=2300)]))                                # min(cur_begin, .)
        qs.append((5000, [rec(300, 2000, 5000, eb=hang, el=1700 + hang)]))                         # min(., ext_begin)
        qs.append((5000, [rec(0, 5000 - hang, 5000, eb=0, ee=4000, el=4200)]))                     # cur_len - cur_end
        qs.append((5000, [rec(0, 4700, 5000, eb=0, ee=4000, el=4000 + hang)]))                     # ext_len - ext_end
    B["overhang"] = ReadBatch(qs, dict(max_overhang=50))
    # a self hit and a reverse-complement hit are skipped, for a forward and a reverse-complement query id
    qs = []
    for cur in (1000, 1001):
        qs.append((3000, [rec(0, 3000, 3000, cur_id=cur, ext_id=cur)]))
        qs.append((3000, [rec(0, 3000, 3000, cur_id=cur, ext_id=cur ^ 1)]))
        qs.append((3000, [rec(0, 3000, 3000, cur_id=cur, ext_id=cur + 2), rec(0, 3000, 3000, cur_id=cur, ext_id=cur),
                          rec(0, 3000, 3000, cur_id=cur, ext_id=(cur ^ 1) + 2)]))
    B["skips"] = ReadBatch(qs)
    # empty (cur_end / w - 2 < cur_begin / w), one window, the whole vector with cur_end == cur_len on a multiple of w
    B["intervals"] = ReadBatch([(1000, [rec(300, 499, 1000)]), (1000, [rec(300, 599, 1000)]), (1000, [rec(0, 1000, 1000)]),
                                (1000, [rec(399, 400, 1000)]), (1000, [rec(0, 199, 1000)]), (1000, [rec(0, 200, 1000)]),
                                (1000, [rec(800, 1000, 1000)]), (1000, [rec(700, 1000, 1000)])])
    # 5000 records on the same two windows
    B["pileup"] = ReadBatch([(2000, [rec(500, 899, 2000, ext_id=2000 + 2 * i) for i in range(5000)]), (2000, [span(0, 18, 2000)])])
    # the median of even and odd n, with ties: [1, 1, 2, 2] -> 2 (the upper one), [3, 1, 1, 2, 2] -> 2, [1, 1, 1, 5] -> 1
    B["median"] = ReadBatch([
        (500, [span(0, 3, 500), span(2, 3, 500)]),
        (600, [span(0, 4, 600), span(0, 0, 600), span(0, 0, 600), span(3, 4, 600)]),
        (500, [span(0, 3, 500)] + [span(3, 3, 500)] * 4),
        (200, [span(0, 0, 200)] * 7),
        (300, [span(0, 1, 300), span(1, 1, 300)]),
    ], dict(uneven_coverage=1, max_drop_rate=2.0))
    # min_good at max_flank 0, 5, 15: a dip just outside and just inside the good range on either side, and the vector
    # sizes at which good_end is below, equal to and one above good_start
    for flank in (0, 5, 15):
        n = 40
        cl = (n + 1) * 100
        qs = []
        for dip in sorted({max(flank - 1, 0), flank, n - flank - 1, min(n - flank, n - 1), n // 2}):
            cover = [span(0, n - 1, cl, ext_id=2000 + 2 * i) for i in range(3)]
            cover[0] = span(0, dip - 1, cl) if dip > 0 else span(1, n - 1, cl, ext_id=2010)
            if 0 < dip < n - 1:
                cover.append(span(dip + 1, n - 1, cl, ext_id=2012))
            qs.append((cl, cover))
        for m in sorted({max(2 * flank, 1), 2 * flank + 1, 2 * flank + 2}):
            c2 = (m + 1) * 100
            qs.append((c2, [span(0, m - 1, c2, ext_id=2000 + 2 * i) for i in range(4)]))
        B["flank%d" % flank] = ReadBatch(qs, dict(max_overhang=flank * 100 + (37 if flank else 0), overlap_coverage=15,
                                                  max_drop_rate=5.0))
    # tiles of 64 windows: an interval from one tile into the next, one that ends exactly on a tile edge, one over
    # three tiles, and the running sum carried across all of them
    cl = 25800
    B["tiles"] = ReadBatch([(cl, [span(60, 70, cl), span(10, 63, cl), span(60, 200, cl), span(0, 256, cl), span(64, 127, cl),
                                  span(128, 128, cl), span(63, 64, cl, eb=900, el=1100)]),
                            (cl, [span(255, 256, cl)]), (cl, [])], dict(max_overhang=100))
    # thresholds at lround ties and around them, both modes
    for rate, cov in ((2, 1), (2, 3), (2, 5), (5, 12), (5, 13), (4, 6), (4, 10)):
        for uneven in (0, 1):
            n = 12
            cl = (n + 1) * 100
            qs = [(cl, [span(0, n - 1, cl, ext_id=2000 + 2 * i) for i in range(c)]) for c in (cov, max(lround_half(cov, rate) - 1, 1),
                                                                                                lround_half(cov, rate), cov + 1)]
            B["thr_%d_%d_%d" % (rate, cov, uneven)] = ReadBatch(qs, dict(max_drop_rate=float(rate), overlap_coverage=cov,
                                                                        uneven_coverage=uneven, max_overhang=100))
    return B


def lround_half(cov, rate):
    """the threshold the tie cases are built around (exact rationals: halves round away from zero)"""
    return max(1, (2 * cov + rate) // (2 * rate))


def fuzz_reads(seed, n_queries=200):
    rng = np.random.default_rng(seed)
    W = (100, 7, 1)[seed % 3]
    P = dict(window=W, max_overhang=int(rng.choice([0, 50, 500, 1500])), max_drop_rate=float(rng.choice([2.0, 4.0, 5.0, 2.5])),
             overlap_coverage=int(rng.integers(0, 40)), uneven_coverage=int(seed // 3 % 2))
    qs = []
    for q in range(n_queries):
        cl = int(rng.integers(1, 30001)) if q % 9 else int(rng.choice([1, W, W + 1, 2 * W, 2 * W + 1, 64 * W, 65 * W + 1]))
        n = int(rng.integers(0, 301)) if rng.integers(0, 4) else 0
        cur = 2 * q + int(rng.integers(0, 2))
        recs = _random_records(rng, cl, n, cur)
        if q % 3 == 1:                  # a blanket of whole-read records: the verdict then hangs on the threshold
            recs += [rec(0, cl, cl, cur_id=cur, ext_id=5000 + 2 * i) for i in range(int(rng.integers(1, 16)))]
        qs.append((cl, recs))
    if W == 100:
        cl = 16777301                   # (float)cl rounds: 167772 windows, several tiles at the default tile size
        qs.append((cl, _random_records(rng, cl, 6, 2 * n_queries) + [rec(0, cl, cl, cur_id=2 * n_queries, ext_id=7),
                                                                      rec(204800, 409700, cl, cur_id=2 * n_queries, ext_id=9)]))
    return ReadBatch(qs, P)


def _random_records(rng, cl, n, cur_id):
    if not n:
        return []
    a = rng.integers(0, cl + 1, n)
    b = rng.integers(0, cl + 1, n)
    cb, ce = np.minimum(a, b), np.maximum(a, b)
    ext = rng.integers(0, 400, n) * 2 + rng.integers(0, 2, n)
    ext[rng.integers(0, n)] = cur_id ^ int(rng.integers(0, 2))          # a self or reverse-complement hit now and then
    el = (ce - cb) + rng.choice([0, 0, 10, 60, 600, 2000], n) + rng.choice([0, 0, 30, 501, 1501], n)
    eb = np.minimum(rng.choice([0, 0, 49, 50, 51, 500, 501, 1500, 1501], n), el - (ce - cb))
    ee = np.minimum(eb + (ce - cb) + rng.integers(0, 3, n), el)
    return [(cur_id, int(ext[i]), int(cb[i]), int(ce[i]), cl, int(eb[i]), int(ee[i]), int(el[i])) for i in range(n)]


# ---- crafted edge batches -------------------------------------------------------------------------------------------
def crafted_edges():
    """name -> EdgeBatch.  Sequences 10 .. : edge_of maps two sequences (10, 11) to edge 0."""
    W = 100
    edge_len = [1000, 2550, 99, 0, 700, 1000, 100]              # 10, 25, 0, 0, 7, 10, 1 windows; edge 5 is never touched
    edge_of = [0, 0, 1, 2, 3, 4, 6]                             # ids 10 .. 16
    alns = [(10, 250, 800), (11, 0, 1000), (12, 130, 2400), (13, 10, 90), (14, 0, 0), (15, 350, 650), (16, 0, 100),
            (12, 2600, 2700), (15, 100, 5000), (10, 999, 1000), (12, -250, 300), (15, 300, -100), (12, 900, 400)]
    paths = [[0], [1], [2], [0, 2], [2, 0], [0, 2, 5], [5, 1, 2], [3], [4], [3, 5, 4], [6], [7], [8], [9], [10], [11], [12], [],
             [7, 8], [8, 7], [6, 6, 6]]
    return {"rules": EdgeBatch(W, alns, paths, 10, edge_of, edge_len),
            "no_paths": EdgeBatch(W, alns, [], 10, edge_of, edge_len),
            "window7": EdgeBatch(7, alns, paths, 10, edge_of, edge_len)}


def fuzz_edges(seed, n_edges=None):
    rng = np.random.default_rng(seed)
    if n_edges is None:
        n_edges = int(rng.choice([3, 40, 300]))
    W = int(rng.choice([100, 7, 1000]))
    edge_len = rng.integers(0, 60 * W, n_edges)
    edge_len[rng.integers(0, n_edges, max(1, n_edges // 10))] = rng.integers(0, W)
    n_ext = 2 * n_edges + 3
    edge_of = rng.integers(0, n_edges, n_ext)
    n_rec = 40 * n_edges if n_edges < 100 else 8 * n_edges
    ext = rng.integers(0, n_ext, n_rec)
    ln = edge_len[edge_of[ext]]
    a = rng.integers(0, ln + 1 + 2 * W)
    b = rng.integers(0, ln + 1 + 2 * W)
    alns = np.stack([ext + 500, np.minimum(a, b), np.maximum(a, b)], 1)
    paths, i = [], 0
    while i < n_rec:
        m = int(rng.choice([1, 1, 1, 2, 3, 5]))
        paths.append(list(range(i, min(i + m, n_rec))))
        i += m
    order = rng.permutation(len(paths))
    return EdgeBatch(W, alns, [paths[k] for k in order], 500, edge_of, edge_len)
