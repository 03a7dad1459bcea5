"""Yardstick and inputs of tests/test_read_chains.py.

The edge-chain step of ReadAligner::alignReads (reference src/repeat_graph/read_aligner.cpp:212-262) has no program of
the reference behind it that could be built and asked for chains, so it is restated twice, independently:

* ``restate`` below: numpy / Python on predecessor arrays (a chain is the alignment it ends in), both permutations taken
  from ``oracle.std_sort_perm`` (``perm=`` swaps another sort in);
* ``tests/native/read_chain_driver.cpp``: chains as objects with index vectors in two ``std::deque``s, ordered by the
  real ``std::sort`` (``run_native``).

The CPU test pins that the two agree on every case; the device is compared with them."""
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REC_FIELDS = ("cur_begin", "cur_end", "ext_begin", "ext_end", "ext_len", "score", "ext_id")

# the crafted cases use a small max_jump so that every threshold sits at round numbers
PARAMS = dict(max_jump=300, max_read_overlap=50, min_alignment=50, max_separation=20, long_edge=900, big_alignment=500)


def std_perm(keys):
    from oracle import oracle as O
    return O.std_sort_perm(np.asarray(keys, np.uint64))


def stable_perm(keys):
    return np.argsort(np.asarray(keys, np.uint64), kind="stable").astype(np.uint32)


def _i32(x):
    return ((int(x) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


class Batch:
    """Per-read record lists with node tables: what fg_chain_alignments takes."""

    def __init__(self, queries, node_left, node_right, first_ext_id=0, params=None):
        """queries: a list of lists of (cur_begin, cur_end, ext_begin, ext_end, ext_len, score, ext_id)"""
        self.params = dict(params or PARAMS)
        self.first_ext_id = int(first_ext_id)
        self.node_left = np.ascontiguousarray(node_left, np.uint32)
        self.node_right = np.ascontiguousarray(node_right, np.uint32)
        self.query_off = np.zeros(len(queries) + 1, np.uint64)
        self.query_off[1:] = np.cumsum([len(q) for q in queries])
        flat = [r for q in queries for r in q]
        self.table = np.array(flat, np.int64).reshape(-1, 7)

    @property
    def n_queries(self):
        return len(self.query_off) - 1

    def recs(self):
        """The records as fg_overlap_rec (the fields the step does not read are filled in plausibly)."""
        from flye_amd import gpu
        r = np.zeros(len(self.table), gpu.REC_DTYPE)
        for j, f in enumerate(REC_FIELDS):
            r[f] = self.table[:, j]
        q = np.repeat(np.arange(self.n_queries), np.diff(self.query_off.astype(np.int64)))
        r["cur_id"] = 100000 + 2 * q
        r["cur_len"] = r["cur_end"] + 10
        r["edit_distance"] = -1
        return r


def from_specs(queries, params=None):
    """queries: lists of dicts(cb, ce, eb, ee, el, sc, nl, nr): every record gets an indexed sequence of its own, so
    that a case can choose the two nodes per record."""
    out, nl, nr = [], [], []
    for q in queries:
        rows = []
        for a in q:
            rows.append((a["cb"], a["ce"], a["eb"], a["ee"], a["el"], a["sc"], 7 + len(nl)))
            nl.append(a["nl"])
            nr.append(a["nr"])
        out.append(rows)
    return Batch(out, nl or [0], nr or [0], first_ext_id=7, params=params)


# ---- the restatement on predecessor arrays ------------------------------------------------------------------------
def restate_query(tab, node_left, node_right, first_ext_id, P, perm, stats):
    """tab: (n, 7) integers of one query.  Returns [(score, [positions in tab, front first]), ...]."""
    n = len(tab)
    keep = [i for i in range(n)
            if tab[i][4] < P["long_edge"] or min(tab[i][1] - tab[i][0], tab[i][3] - tab[i][2]) > P["big_alignment"]]
    keys = [int(tab[i][0]) for i in keep]
    if len(keys) > 16 and len(set(keys)) < len(keys):
        stats["tied_first"] += 1
    order = [keep[int(j)] for j in perm(keys)] if keys else []
    m = len(order)
    cb = [int(tab[i][0]) for i in order]
    ce = [int(tab[i][1]) for i in order]
    eb = [int(tab[i][2]) for i in order]
    gap_r = [int(tab[i][4]) - int(tab[i][3]) for i in order]
    sc = [int(tab[i][5]) for i in order]
    nl = [int(node_left[int(tab[i][6]) - first_ext_id]) for i in order]
    nr = [int(node_right[int(tab[i][6]) - first_ext_id]) for i in order]
    max_jump = P["max_jump"]
    pred, score, first = [-1] * m, [0] * m, [0] * m
    active, frozen = [], []
    for i in range(m):
        best, best_j, outdated = 0, -1, 0
        if eb[i] < max_jump:
            for j in active:
                read_diff = cb[i] - ce[j]
                graph = eb[i] + gap_r[j]
                if nr[j] == nl[i] and max_jump > read_diff > -P["max_read_overlap"] and graph < max_jump:
                    jump_div = abs(read_diff - graph)
                    s = _i32(score[j] + sc[i] - (jump_div // 50 if jump_div > 100 else 0))
                    if s > best:
                        best, best_j = s, j
                if read_diff > max_jump:
                    outdated += 1
        if best_j >= 0:
            pred[i], score[i], first[i] = best_j, best, first[best_j]
            active.append(i)
        else:
            pred[i], score[i], first[i] = -1, sc[i], i
            (active if gap_r[i] < max_jump else frozen).append(i)
        if outdated > len(active) // 2:
            stats["cleanups"] += 1
            frozen += [j for j in active if cb[i] - ce[j] > max_jump]
            active = [j for j in active if not cb[i] - ce[j] > max_jump]
    chains = active + frozen
    keys2 = [(1 << 31) - score[c] for c in chains]
    if len(keys2) > 16 and len(set(keys2)) < len(keys2):
        stats["tied_second"] += 1
    chains = [chains[int(j)] for j in perm(keys2)] if chains else []
    accepted = []
    for c in chains:
        start, end = cb[first[c]], ce[c]
        if end - start < P["min_alignment"]:
            continue
        if any(min(end, e) - max(start, s) > P["max_separation"] for s, e, _ in accepted):
            stats["rejected"] += 1
            continue
        accepted.append((start, end, c))
    out = []
    for _, _, c in accepted:
        walk, j = [], c
        while j >= 0:
            walk.append(order[j])
            j = pred[j]
        out.append((score[c], walk[::-1]))
    return out


def new_stats():
    return dict(cleanups=0, tied_first=0, tied_second=0, rejected=0)


def restate(batch, perm=std_perm, queries=None):
    """(chain_off, aln_off, aln, score, stats) of the batch, as fg_chain_alignments returns them."""
    stats = new_stats()
    chain_off, aln_off, aln, score = [0], [0], [], []
    off = batch.query_off.astype(np.int64)
    for q in range(batch.n_queries):
        a, b = int(off[q]), int(off[q + 1])
        if queries is None or q in queries:
            for s, walk in restate_query(batch.table[a:b].tolist(), batch.node_left, batch.node_right, batch.first_ext_id,
                                         batch.params, perm, stats):
                aln += [a + i for i in walk]
                aln_off.append(len(aln))
                score.append(s)
        chain_off.append(len(score))
    return (np.array(chain_off, np.uint64), np.array(aln_off, np.uint64), np.array(aln, np.uint64),
            np.array(score, np.int32), stats)


# ---- the literal form ---------------------------------------------------------------------------------------------
_DRIVER = {}


def native_driver():
    if "exe" not in _DRIVER:
        d = tempfile.mkdtemp(prefix="read_chain_driver_")
        exe = os.path.join(d, "read_chain_driver")
        subprocess.run(["g++", "-std=c++17", "-O2", "-pthread", os.path.join(ROOT, "tests", "native", "read_chain_driver.cpp"),
                        "-o", exe], check=True)
        _DRIVER["exe"], _DRIVER["dir"] = exe, d
    return _DRIVER["exe"]


def write_native_input(batch, path):
    P = batch.params
    with open(path, "wb") as f:
        np.array([P[k] for k in ("max_jump", "max_read_overlap", "min_alignment", "max_separation", "long_edge",
                                 "big_alignment")], np.int32).tofile(f)
        np.array([batch.first_ext_id, len(batch.node_left), batch.n_queries, 0], np.uint32).tofile(f)
        np.array([len(batch.table)], np.uint64).tofile(f)
        batch.node_left.tofile(f)
        batch.node_right.tofile(f)
        batch.query_off.tofile(f)
        batch.table.astype(np.int32).tofile(f)


def run_native(batch, threads=1, repeats=1):
    """The same five values from tests/native/read_chain_driver.cpp, and its best wall time."""
    exe = native_driver()
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        write_native_input(batch, src)
        r = subprocess.run([exe, src, dst, str(threads), str(repeats)], check=True, capture_output=True, text=True)
        raw = np.fromfile(dst, np.uint8)
    head = raw[:48].view(np.uint64)
    nc, na = int(head[0]), int(head[1])
    nq = batch.n_queries
    p = 48
    chain_off = raw[p:p + 8 * (nq + 1)].view(np.uint64); p += 8 * (nq + 1)
    aln_off = raw[p:p + 8 * (nc + 1)].view(np.uint64); p += 8 * (nc + 1)
    aln = raw[p:p + 8 * na].view(np.uint64); p += 8 * na
    score = raw[p:p + 4 * nc].view(np.int32)
    stats = dict(cleanups=int(head[2]), tied_first=int(head[3]), tied_second=int(head[4]), rejected=int(head[5]))
    return chain_off.copy(), aln_off.copy(), aln.copy(), score.copy(), stats, float(r.stdout.split()[-1])


def same(a, b):
    return all(np.array_equal(np.asarray(x).astype(np.int64), np.asarray(y).astype(np.int64)) for x, y in zip(a[:4], b[:4]))


# ---- crafted queries ----------------------------------------------------------------------------------------------
def aln(cb, ce, gl=0, gr=0, sc=100, nl=1, nr=1, ext_range=None, el=None):
    """An alignment on a short edge (it passes the filter): ext_begin = gl, ext_len - ext_end = gr."""
    er = 560 if ext_range is None else ext_range
    el = gl + er + gr if el is None else el
    return dict(cb=cb, ce=ce, eb=gl, ee=el - gr, el=el, sc=sc, nl=nl, nr=nr)


def pair(read_diff, gl=0, gr=0, sc=(100, 100), nodes=(1, 1)):
    """Two alignments: the second may continue the first"""
    return [aln(0, 600, gr=gr, sc=sc[0], nr=nodes[0], ext_range=280), aln(600 + read_diff, 1200 + read_diff, gl=gl, sc=sc[1], nl=nodes[1],
                                                                         ext_range=280)]


def cleanup_query(n_outdated, n_live):
    """n_outdated chains on [0, 100), n_live on [50, 1000), all of one score, then an alignment at 1000 that continues
    none of them but counts the outdated ones: with a cleanup the order "active then frozen" puts a live chain first
    and it wins its span, without one an outdated chain does."""
    q = [aln(0, 100, nr=5) for _ in range(n_outdated)] + [aln(50, 1000, nr=5) for _ in range(n_live)]
    return q + [aln(1000, 1600, nl=9)]


def crafted_cases():
    """name -> list of queries (each a list of alignment specs)"""
    J = PARAMS["max_jump"]
    cases = {}
    # filter (:224-226): ext_len 899 / 900 at a range of 500, range 500 / 501 at ext_len 900
    cases["filter"] = [[dict(cb=0, ce=500, eb=0, ee=500, el=el, sc=10, nl=1, nr=2)] for el in (899, 900)] + \
                      [[dict(cb=0, ce=cr, eb=0, ee=er, el=900, sc=10, nl=1, nr=2)] for cr, er in ((500, 600), (501, 501), (600, 500), (501, 900))]
    cases["read_diff"] = [pair(d) for d in (J - 1, J, -PARAMS["max_read_overlap"], -PARAMS["max_read_overlap"] + 1, 0)]
    cases["graph_diff"] = [pair(250, gl=150, gr=149), pair(250, gl=150, gr=150), pair(250, gl=149, gr=150), pair(250, gl=0, gr=J - 1),
                           pair(250, gl=0, gr=J)]
    cases["jump_div"] = [pair(d) for d in (100, 101, 149, 150)] + [pair(0, gl=60, gr=41), pair(0, gl=100, gr=50), pair(10, gl=100, gr=10)]
    cases["can_extend"] = [pair(250, gl=J - 1), pair(250, gl=J)]
    # ext_len - ext_end at max_jump - 1 / max_jump: active or frozen, seen in the order of two equal overlapping chains
    cases["can_be_extended"] = [[aln(0, 600, gr=g, nr=3, ext_range=280), aln(100, 700, gr=0, nr=4, nl=8, ext_range=280)] for g in (J - 1, J)]
    cases["node_mismatch"] = [pair(10, nodes=(1, 2)), pair(10, nodes=(2, 2))]
    # gapCost = 2 at jumpDiv 101 .. 149, 3 at 150: totals of 1, 0 and -1
    cases["score_edges"] = [pair(120, sc=(2, 1)), pair(120, sc=(1, 1)), pair(150, sc=(1, 1)), pair(150, sc=(1, 3)), pair(10, sc=(-5, 5)),
                            pair(10, sc=(-5, 6))]
    two = [aln(0, 600, sc=50, nr=1), aln(0, 600, sc=50, nr=1), aln(10, 600, sc=49, nr=1), aln(610, 1200, nl=1)]
    cases["equal_best"] = [two, two[1::-1] + two[2:], [two[2], two[0], two[1], two[3]]]
    cases["cleanup"] = [cleanup_query(a, b) for a, b in ((3, 2), (4, 1), (2, 2), (3, 1), (1, 1), (2, 0), (1, 0), (7, 6), (8, 6))]
    cases["empty_shapes"] = [[], [aln(0, 600)], [dict(cb=0, ce=500, eb=0, ee=500, el=900, sc=10, nl=1, nr=1)] * 3, [], [], pair(10), [],
                             [aln(0, 20)], []]
    return cases


def tied_begin_queries(seed=1):
    """16, 17 and about 100 alignments of equal score with few distinct cur_begin on different edges, all ending where
    one later alignment can continue every one of them: the chain that wins is the first in std::sort's order."""
    rng = np.random.default_rng(seed)
    out = []
    for n in (16, 17, 17, 23, 100, 101):
        q = [aln(int(rng.integers(0, 3)) * 10, 600, sc=50, nr=1) for _ in range(n - 2)]
        q.append(aln(610, 1200, nl=1))
        q.append(aln(20, 590, sc=50, nr=2))
        out.append([q[i] for i in rng.permutation(len(q))])
    return out


def tied_score_queries(seed=2):
    """17 and more chains of equal score whose spans all overlap: the order the second sort leaves decides the winner"""
    rng = np.random.default_rng(seed)
    out = []
    for n in (16, 17, 20, 33, 100):
        q = [aln(i, 600 + i, sc=100 if i % 5 else 99, nr=2, nl=3) for i in range(n)]
        out.append([q[i] for i in rng.permutation(n)])
    return out


def wave_edge_queries(seed=3):
    rng = np.random.default_rng(seed)
    out = []
    for n in (63, 64, 65, 129, 200):
        q = [aln(i, 600, sc=int(rng.integers(40, 44)), nr=int(rng.integers(1, 4)), nl=7) for i in range(n)]
        q += [aln(620 + k, 1200, nl=k + 1, nr=8, sc=30 + k) for k in range(3)]
        out.append(q)
    # more than 64 accepted chains: disjoint alignments further than max_jump apart (the cleanup fires as well)
    perm = rng.permutation(70)
    out.append([aln(1000 * i, 1000 * i + 600, sc=100 + int(perm[i])) for i in range(70)])
    out.append([aln(1000 * i, 1000 * i + 600, sc=100) for i in range(70)])
    # one chain 150 alignments deep
    out.append([aln(610 * i, 610 * i + 600, sc=10) for i in range(150)])
    return out


def fuzz_batch(seed, n_queries=3000):
    rng = np.random.default_rng(seed)
    n_ext = 64
    node_left = rng.integers(0, 4, n_ext)
    node_right = rng.integers(0, 4, n_ext)
    queries = []
    for _ in range(n_queries):
        n = int(rng.integers(0, 41))
        if rng.integers(0, 400) == 0:
            n = int(rng.integers(200, 400))
        span = 40 if n < 100 else 200
        cb = rng.integers(0, span, n) * 50 + rng.choice([0, 0, 0, 1, -1, 10], n)
        cb = np.maximum(cb, 0)
        ce = cb + rng.choice([100, 300, 501, 550, 600], n)
        el = rng.choice([400, 700, 899, 900, 1200], n)
        eb = rng.choice([0, 0, 10, 100, 150, 299, 300], n)
        gr = rng.choice([0, 0, 50, 149, 150, 299, 300, 400], n)
        ee = np.maximum(el - gr, eb)
        sc = rng.choice([1, 2, 3, 5, 100, 100, 100], n)
        ext = rng.integers(0, n_ext, n) + 1000
        queries.append(list(zip(cb.tolist(), ce.tolist(), eb.tolist(), ee.tolist(), el.tolist(), sc.tolist(), ext.tolist())))
    return Batch(queries, node_left, node_right, first_ext_id=1000)


# ---- end to end: the inputs of the edges_* golden cases, as tests/test_gpu_parity.py sets them up -----------------
def edges_context(case, cfg):
    """(context, detector parameters, query ids of both strands, number of edge sequences)"""
    from flye_amd import gpu
    from helpers import edges_setup, golden_queries, golden_reads
    edges = golden_reads(case)
    reads = golden_queries(case)
    wnd, dk = edges_setup(case, cfg)
    ctx = gpu.Context(int(cfg["kmer_size"]), 0)
    ctx.set_reads(edges, 0)
    vi = gpu.VertexIndex(ctx, float(int(cfg["assemble_kmer_sample"])))
    vi.buildIndexMinimizers(1, wnd, cfg["repeat_kmer_rate"])
    ctx.set_queries(reads, 2 * edges.n)
    det = gpu.OverlapDetector(ctx, vi, int(cfg["maximum_jump"]), dk["min_overlap"], dk["max_overhang"], False, dk["only_max_ext"],
                              1.0, False, False, bool(cfg["hpc_scoring_on"]))
    fwd = (2 * edges.n + np.arange(0, 2 * reads.n, 2)).astype(np.uint32)
    return ctx, det, fwd, edges.n


def synthetic_nodes(n_edges, seed=5):
    """Node tables over both strands in which consecutive edge sequences share a node: edge i runs from node i to node
    i + 1 (a few seeded edges end elsewhere); the complement edge runs between the complement nodes, the other way."""
    rng = np.random.default_rng(seed)
    left = np.arange(n_edges, dtype=np.int64)
    right = left + 1
    broken = rng.random(n_edges) < 0.15
    right[broken] = 10_000 + np.flatnonzero(broken)
    nl = np.zeros(2 * n_edges, np.uint32)
    nr = np.zeros(2 * n_edges, np.uint32)
    nl[0::2], nr[0::2] = left, right
    nl[1::2], nr[1::2] = right + 100_000, left + 100_000      # complement node of x: x + 100000
    return nl, nr
