"""The short-plasmid passes of the reference (flye/short_plasmids/, flye/utils/sam_parser.py:55-120) restated in numpy
and plain Python, the crafted and fuzzed inputs of tests/test_plasmids.py and tests/golden/make_plasmid_golden.py, and
the array-level cases of the device tests.  Nothing here is taken from the reference's text: the functions are written
from what its loops do, and tests/golden/plasmid_cases.json.gz holds what the unmodified reference gives on the same
files."""
import gzip
import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

HIT_DTYPE = np.dtype([("query", "<u4"), ("target", "<u4"), ("query_len", "<i4"), ("query_start", "<i4"), ("query_end", "<i4"),
                      ("target_len", "<i4"), ("target_start", "<i4"), ("target_end", "<i4")])


# ---- text level ------------------------------------------------------------------------------------------------------
def tokenize(paf):
    """per line (query name, target name, the six integers), as PafHit.__init__ reads them"""
    out = []
    for line in _lines(paf):
        f = line.split()
        out.append((f[0], f[5], int(f[1]), int(f[2]), int(f[3]), int(f[6]), int(f[7]), int(f[8])))
    return out


def _lines(data):
    """what iterating over a binary file gives: pieces that end behind every \\n"""
    at = 0
    while at < len(data):
        end = data.find(b"\n", at)
        end = len(data) if end < 0 else end + 1
        yield data[at:end]
        at = end


def to_hits(tokens):
    """-> (hits, names): ids are ranks of the distinct names, queries and targets together, in ascending byte order"""
    names = sorted(set(t[0] for t in tokens) | set(t[1] for t in tokens))
    rank = {n: i for i, n in enumerate(names)}
    hits = np.zeros(len(tokens), HIT_DTYPE)
    for i, t in enumerate(tokens):
        hits[i] = (rank[t[0]], rank[t[1]]) + t[2:]
    return hits, names


def first_seen(tokens):
    """the names in order of first appearance, the query before the target of a line"""
    seen = {}
    for t in tokens:
        seen.setdefault(t[0], None)
        seen.setdefault(t[1], None)
    return list(seen)


# ---- array level: what the device calls return ------------------------------------------------------------------------
def united_length(pairs):
    """the bases the united segments hold: segments by start; one that starts at or before the end of the last united
    segment is folded into it, any other opens a new one"""
    pairs = sorted(pairs, key=lambda p: p[0])
    total, cur_start, cur_end = 0, pairs[0][0], pairs[0][1]
    for s, e in pairs[1:]:
        if s <= cur_end:
            cur_end = max(cur_end, e)
        else:
            total += cur_end - cur_start + 1
            cur_start, cur_end = s, e
    return total + cur_end - cur_start + 1


def group_lists(hits):
    """hit indices per group: runs in file order, inside a run the targets ascending, file order inside a group"""
    groups, run = [], {}
    q = hits["query"].tolist()
    t = hits["target"].tolist()
    for i in range(len(hits)):
        if i and q[i] != q[i - 1]:
            groups += [run[k] for k in sorted(run)]
            run = {}
        run.setdefault(t[i], []).append(i)
    return groups + [run[k] for k in sorted(run)]


def groups(hits):
    gl = group_lists(hits)
    qs, qe, ts, te = (hits[k].tolist() for k in ("query_start", "query_end", "target_start", "target_end"))
    return dict(order=np.array([i for g in gl for i in g], np.uint32),
                group_off=np.cumsum([0] + [len(g) for g in gl]).astype(np.uint64),
                group_query=np.array([hits["query"][g[0]] for g in gl], np.uint32),
                group_target=np.array([hits["target"][g[0]] for g in gl], np.uint32),
                query_cover=np.array([united_length([(qs[i], qe[i]) for i in g]) for g in gl], np.int64),
                target_cover=np.array([united_length([(ts[i], te[i]) for i in g]) for g in gl], np.int64))


def circular(hits, max_overhang_read=150, max_overhang_pair=300):
    H = [tuple(int(x) for x in h) for h in hits.tolist()]
    Q, T, QL, QS, QE, TL, TS, TE = range(8)
    kept, order = {}, []
    for i, h in enumerate(H):
        if h[Q] == h[T] and h[QS] < h[QE] < h[TS] < h[TE] and h[QS] < max_overhang_read and h[TL] - h[TE] + 1 < max_overhang_read:
            if h[Q] not in kept:
                order.append(h[Q])
                kept[h[Q]] = i
            elif h[QE] - h[QS] > H[kept[h[Q]]][QE] - H[kept[h[Q]]][QS]:
                kept[h[Q]] = i
    gl = group_lists(hits)
    first, second, ok = [], [], []
    for g in gl:
        a = b = -1
        if H[g[0]][Q] != H[g[0]][T]:
            for i in g:
                h = H[i]
                if a < 0 and h[QL] - h[QE] + 1 < max_overhang_pair and h[TS] < max_overhang_pair:
                    a = i
                elif b < 0 and h[QS] < max_overhang_pair and h[TL] - h[TE] + 1 < max_overhang_pair:
                    b = i
        good = 0
        if a >= 0 and b >= 0:
            p0, p1 = H[a], H[b]
            good = int(p1[QS] < p1[QE] < p0[QS] < p0[QE] and p0[TS] < p0[TE] < p1[TS] < p1[TE])
        first.append(a), second.append(b), ok.append(good)
    return dict(circ_query=np.array(order, np.uint32), circ_hit=np.array([kept[q] for q in order], np.uint32),
                group_query=np.array([H[g[0]][Q] for g in gl], np.uint32), group_target=np.array([H[g[0]][T] for g in gl], np.uint32),
                pair_first=np.array(first, np.int32), pair_second=np.array(second, np.int32), pair_ok=np.array(ok, np.uint8))


def components(n_vertices, edge_u, edge_v):
    """labels[v]: the smallest vertex of v's component (union by smaller root)"""
    root = list(range(n_vertices))

    def find(v):
        while root[v] != v:
            root[v] = root[root[v]]
            v = root[v]
        return v

    for u, v in zip(np.asarray(edge_u).tolist(), np.asarray(edge_v).tolist()):
        a, b = find(u), find(v)
        if a != b:
            root[max(a, b)] = min(a, b)
    return np.array([find(v) for v in range(n_vertices)], np.uint32)


# ---- the reference's functions, from the passes above -----------------------------------------------------------------
def mapping_rates(paf):
    tokens = tokenize(paf)
    hits, names = to_hits(tokens)
    g = groups(hits)
    out = {}
    for k in range(len(g["group_query"])):
        h = hits[int(g["order"][int(g["group_off"][k])])]
        out.setdefault(names[h["query"]].decode(), {})[names[h["target"]].decode()] = round(int(g["query_cover"][k]) / int(h["query_len"]), 3)
    return out


def hit_fields(tokens, i):
    t = tokens[i]
    return [t[0].decode(), t[2], t[3], t[4], t[1].decode(), t[5], t[6], t[7]]


def circular_reads(paf, max_overhang=150):
    """[[name, hit fields]] in the order of the reference's dict"""
    tokens = tokenize(paf)
    hits, names = to_hits(tokens)
    c = circular(hits, max_overhang, 300)
    return [[names[q].decode(), hit_fields(tokens, int(i))] for q, i in zip(c["circ_query"].tolist(), c["circ_hit"].tolist())]


def circular_pairs(paf, max_overhang=300):
    """[[first hit fields, second hit fields]] after the greedy filter over the groups in order"""
    tokens = tokenize(paf)
    hits, _ = to_hits(tokens)
    c = circular(hits, 150, max_overhang)
    used, out = set(), []
    for q, t, a, b, ok in zip(c["group_query"].tolist(), c["group_target"].tolist(), c["pair_first"].tolist(), c["pair_second"].tolist(),
                              c["pair_ok"].tolist()):
        if q == t or q in used or t in used or not ok:
            continue
        used.update((q, t))
        out.append([hit_fields(tokens, a), hit_fields(tokens, b)])
    return out


def read_fasta(data):
    out, header = {}, None
    for line in data.splitlines():
        line = line.strip()
        if line.startswith(b">"):
            header = line[1:].split()[0].decode()
            out[header] = ""
        elif line and header is not None:
            out[header] += line.decode()
    return {h: s for h, s in out.items() if s}


def unmapped_fasta(reads, paf, threshold):
    """(the FASTA text extract_unmapped_reads writes, total bases, unmapped bases) for the reads of one FASTA text"""
    rates = mapping_rates(paf)
    text, total, unmapped = [], 0, 0
    for hdr, seq in read_fasta(reads).items():
        total += len(seq)
        if not any(r >= threshold for r in rates.get(hdr, {}).values()):
            unmapped += len(seq)
            text.append(">%s\n%s\n" % (hdr, seq))
    return "".join(text), total, unmapped


def trimmed_reads(circ, seqs):
    return {"circular_read_%d" % i: seqs[name][:f[6]].upper() for i, (name, f) in enumerate(circ)}


def trimmed_pairs(pairs, seqs):
    return {"circular_pair_%d" % i: (seqs[p0[0]][p1[3]:p0[3]] + seqs[p0[4]][p0[7]:]).upper() for i, (p0, p1) in enumerate(pairs)}


def unique_plasmids(paf, fasta, vertex_order, mapping_rate_threshold=0.8, min_sequence_length=1000):
    tokens = tokenize(paf)
    hits, names = to_hits(tokens)
    g = groups(hits)
    number = {n: i for i, n in enumerate(vertex_order)}
    eu, ev = [], []
    for k in range(len(g["group_query"])):
        h = hits[int(g["order"][int(g["group_off"][k])])]
        if h["query"] == h["target"]:
            continue
        if (round(int(g["query_cover"][k]) / int(h["query_len"]), 3) > mapping_rate_threshold or
                round(int(g["target_cover"][k]) / int(h["target_len"]), 3) > mapping_rate_threshold):
            eu.append(number[names[h["query"]].decode()])
            ev.append(number[names[h["target"]].decode()])
    labels = components(len(vertex_order), eu, ev)
    seqs = read_fasta(fasta)
    out = {}
    for v in range(len(vertex_order)):
        if labels[v] == v and int((labels == v).sum()) > 1 and len(seqs[vertex_order[v]]) >= min_sequence_length:
            out[vertex_order[v]] = seqs[vertex_order[v]]
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------
def paf_line(rng, q, ql, qs, qe, t, tl, ts, te):
    sep = " " if rng.randint(8) == 0 else "\t"
    fields = [q, ql, qs, qe, "+-"[rng.randint(2)], t, tl, ts, te, rng.randint(1000), rng.randint(1000) + 1, rng.randint(61)]
    return sep.join(str(f) for f in fields) + "\n"


def make_names(rng, n):
    # r1 / r10 / r2: byte order is not numeric order; one name is a prefix of another
    return ["r%d" % i for i in range(n // 2)] + ["ctg_%d%s" % (i, "x" * rng.randint(3)) for i in range(n - n // 2)]


def random_sequences(rng, names, lo, hi):
    out = []
    for n in names:
        s = "".join("ACGTacgt"[k] for k in rng.randint(0, 8, rng.randint(lo, hi)))
        out.append(">%s some description\n" % n + "\n".join(s[i:i + 70] for i in range(0, len(s), 70)) + "\n")
    return "".join(out)


def fuzz_case(seed, n_names, n_runs, start_values=None, self_rate=0.2, edge=400):
    """a PAF of runs of 1 - 12 hits over few targets, with overhangs around the two thresholds, and a FASTA of its names"""
    rng = np.random.RandomState(seed)
    names = make_names(rng, n_names)
    length = {n: int(rng.randint(600, 3000)) for n in names}
    lines = []
    for _ in range(n_runs):
        q = names[rng.randint(n_names)]
        targets = [names[rng.randint(n_names)] for _ in range(rng.randint(1, 4))]
        for _ in range(rng.randint(1, 13)):
            t = q if rng.rand() < self_rate else targets[rng.randint(len(targets))]
            ql, tl = length[q], length[t]

            def span(L, low, high):
                if start_values is not None:
                    s = int(start_values[rng.randint(len(start_values))]) % L
                    return s, int(min(L, s + rng.randint(0, 300)))
                s = int(rng.randint(0, edge)) if low else int(rng.randint(0, L))
                e = int(L - rng.randint(0, edge)) if high else int(rng.randint(s, L + 1))
                return s, max(s, e)
            kind = rng.randint(4)
            if t == q and kind < 2:            # a circular read's shape: a head on a tail
                qs = int(rng.randint(0, 200)); qe = qs + int(rng.randint(1, 200))
                te = tl - int(rng.randint(0, 200)); ts = max(qe + int(rng.randint(0, 3)), te - int(rng.randint(1, 200)))
                te = max(te, ts)
            elif kind == 0:                    # A: the query's tail on the target's head
                qs, qe = span(ql, False, True)
                ts, te = span(tl, True, False)
            elif kind == 1:                    # B: the query's head on the target's tail
                qs, qe = span(ql, True, False)
                ts, te = span(tl, False, True)
            else:
                qs, qe = span(ql, False, False)
                ts, te = span(tl, False, False)
            lines.append(paf_line(rng, q, ql, qs, qe, t, tl, ts, te))
    return dict(paf="".join(lines).encode(), fasta=random_sequences(rng, names, 30, 160).encode())


def crafted_case():
    """one file that walks the rules: a query in two runs, targets out of order, joins at start == end and not at end + 1,
    both circular-read boundaries, equal-length and longer later circular hits, pairs with B before A"""
    L = []

    def add(q, ql, qs, qe, t, tl, ts, te, sep="\t"):
        L.append(sep.join(str(x) for x in (q, ql, qs, qe, "+", t, tl, ts, te, 10, 20, 60)) + "\n")
    add("r2", 1000, 0, 100, "ctg_b", 5000, 0, 100)
    add("r2", 1000, 100, 200, "ctg_a", 5000, 10, 20)          # target below the one before: groups come out ascending
    add("r2", 1000, 201, 300, "ctg_a", 5000, 21, 30)          # start == end + 1: no join
    add("r2", 1000, 100, 150, "ctg_b", 5000, 100, 400, " ")   # start == end: joins
    add("r10", 2000, 5, 1999, "ctg_a", 5000, 0, 1994)
    add("r2", 1000, 500, 999, "ctg_a", 5000, 40, 539)         # r2 again: a new run, a new (r2, ctg_a) group
    add("r1", 800, 0, 0, "ctg_a", 5000, 7, 7)
    add("r1", 800, 0, 0, "ctg_a", 5000, 7, 7)                 # identical segments
    add("r1", 800, 0, 799, "ctg_a", 5000, 0, 5000)            # cover above the length on the target side
    # circular reads
    add("c1", 1000, 149, 300, "c1", 1000, 600, 852)           # 149 < 150 and 1000 - 852 + 1 = 149 < 150
    add("c2", 1000, 150, 300, "c2", 1000, 600, 900)           # query_start == 150: not circular
    add("c3", 1000, 10, 300, "c3", 1000, 600, 851)            # right overhang == 150: not circular
    add("c4", 1000, 10, 300, "c4", 1000, 300, 990)            # query_end == target_start: not circular
    add("c5", 1000, 10, 110, "c5", 1000, 500, 990)
    add("c5", 1000, 20, 120, "c5", 1000, 600, 990)            # equal length: the first stays
    add("c1", 1000, 0, 400, "c1", 1000, 700, 999)             # longer and later: replaces, c1 keeps its place in the order
    # circular pairs
    add("p1", 1000, 700, 990, "p2", 1200, 5, 300)             # A
    add("p1", 1000, 10, 600, "p2", 1200, 400, 1100)           # B, no intersection: a pair
    add("p3", 1000, 10, 600, "p4", 1200, 400, 1100)           # B before A
    add("p3", 1000, 700, 990, "p4", 1200, 5, 300)
    add("p5", 1000, 5, 995, "p6", 1000, 5, 995)               # A and B in one hit, alone: no pair
    add("p7", 1000, 600, 990, "p8", 1200, 5, 400)             # A
    add("p7", 1000, 10, 600, "p8", 1200, 400, 1100)           # B; query_end == first.query_start, target_end == second.target_start
    add("p2", 1200, 900, 1190, "p9", 1000, 5, 200)            # p2 is used already
    add("p2", 1200, 5, 800, "p9", 1000, 300, 990)
    rng = np.random.RandomState(5)
    names = sorted(set(x.split()[0] for x in L) | set(x.split()[5] for x in L))
    return dict(paf="".join(L).encode(), fasta=random_sequences(rng, names, 1000, 1300).encode())


CASES = {
    "crafted": crafted_case,
    "fuzz_reads": lambda: fuzz_case(11, 40, 260, self_rate=0.05),
    "fuzz_self": lambda: fuzz_case(12, 24, 220, self_rate=0.5),
    "fuzz_ties": lambda: fuzz_case(13, 16, 200, start_values=[0, 3, 50, 51, 52, 299, 300, 301]),
}
# per case: the mapping-rate threshold of extract_unmapped_reads, then threshold and shortest sequence of extract_unique_plasmids
PARAMS = {"crafted": (0.9, 0.8, 1000), "fuzz_reads": (0.95, 0.9, 40), "fuzz_self": (0.9, 0.8, 40), "fuzz_ties": (0.35, 0.3, 40)}


def stored_case(name):
    """the input files as tests/golden holds them"""
    return dict(paf=gzip.open(os.path.join(GOLDEN, "plasmid_%s.paf.gz" % name)).read(),
                fasta=gzip.open(os.path.join(GOLDEN, "plasmid_%s.fa.gz" % name)).read())


def stored_golden():
    return json.loads(gzip.open(os.path.join(GOLDEN, "plasmid_cases.json.gz")).read().decode())


def sha(text):
    return hashlib.sha256(text if isinstance(text, bytes) else text.encode()).hexdigest()


# ---- array-level inputs of the device tests ----------------------------------------------------------------------------
def hits_of(rows):
    """rows of (query, target, query_start, query_end, target_start, target_end[, query_len, target_len])"""
    hits = np.zeros(len(rows), HIT_DTYPE)
    for i, r in enumerate(rows):
        ql, tl = (r[6], r[7]) if len(r) > 6 else (1 << 30, 1 << 30)
        hits[i] = (r[0], r[1], ql, r[2], r[3], tl, r[4], r[5])
    return hits


def fuzz_hits(seed, n, n_names=50, max_run=40, start_values=None, big_groups=()):
    """n hits in runs; big_groups: sizes of single-target runs put in front (they reach the larger size classes)"""
    rng = np.random.RandomState(seed)
    length = rng.randint(600, 4000, n_names)
    q = np.zeros(n, np.int64)
    t = np.zeros(n, np.int64)
    at = 0
    for size in big_groups:
        q[at:at + size] = rng.randint(n_names)
        t[at:at + size] = rng.randint(n_names)
        at += size
    while at < n:
        k = min(n - at, int(rng.randint(1, max_run + 1)))
        q[at:at + k] = rng.randint(n_names)
        pool = rng.randint(0, n_names, int(rng.randint(1, 5)))
        t[at:at + k] = pool[rng.randint(0, len(pool), k)]
        self_hit = rng.rand(k) < 0.2
        t[at:at + k][self_hit] = q[at]
        at += k
    hits = np.zeros(n, HIT_DTYPE)
    hits["query"], hits["target"] = q, t
    hits["query_len"], hits["target_len"] = length[q], length[t]
    for side in ("query", "target"):
        L = hits[side + "_len"].astype(np.int64)
        if start_values is not None:
            s = np.asarray(start_values)[rng.randint(0, len(start_values), n)]
            e = s + rng.randint(0, 4, n) * 100
        else:
            near = rng.rand(n) < 0.5
            s = np.where(near, rng.randint(0, 400, n), (rng.rand(n) * L).astype(np.int64))
            e = np.where(rng.rand(n) < 0.5, L - rng.randint(0, 400, n), s + (rng.rand(n) * 600).astype(np.int64))
            e = np.maximum(s, e)
        hits[side + "_start"], hits[side + "_end"] = s, e
    return hits
