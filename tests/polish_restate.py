"""Yardstick and inputs of tests/test_polish.py: the bubble polishing of flye-modules polisher, restated in numpy from
the description of fg_polish_bubbles in include/flye_gpu.h (byte classes, the F / R matrices, the alignment score with
its empty-string rule, the edit scores, makeStep's order, optimize's three ways to stop, the pre-polish on the sorted
middle five, the dinucleotide fixer, the skip rule).  It shares no code with the library: all branches of a bubble are
filled at once as padded rows, the horizontal move of a row is ``np.maximum.accumulate``, and std::sort's permutation
is written out here a second time.  tests/golden/make_polish_golden.py records what the reference program itself does
on the same inputs; test_polish.py pins this module on those records and compares the device with both.

Also here: the seeded bubble generator, the crafted bubbles, and the reader and writers of the reference's file forms
(bubbles in, consensus out, the --debug step log)."""
import gzip
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LETTERS = "ACGT"
GAP = 5
NEG = -(1 << 60)
SKIPPED, OVERFLOW, ITER_LIMIT, FIXED = 1, 2, 4, 8
MAX_BUBBLE = 5000
BUBBLES_CACHE = 100

_CLASS = np.full(128, 4, np.int64)
for _i, _c in enumerate(LETTERS):
    _CLASS[ord(_c)] = _i
_CLASS[ord("-")] = GAP


def classes(seq):
    """byte string -> class per byte; a byte >= 128 has none"""
    b = np.frombuffer(seq if isinstance(seq, bytes) else seq.encode("latin-1"), np.uint8)
    if len(b) and b.max() >= 128:
        raise ValueError("byte >= 128")
    return _CLASS[b]


def _round_half_away(x):
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


def load_matrix(path):
    """the 6 x 6 table [consensus class][read class] of a *_substitutions.mat text"""
    s = np.zeros((6, 6), np.int64)
    with open(path, "rb") as f:
        text = f.read().decode("latin-1")
    for line in text.split("\n"):
        if line.endswith("\r"):
            line = line[:-1]
        items = line.split("\t")
        if items[0] not in ("mat", "mis", "del", "ins"):
            continue
        if len(items) < 3 or not items[1]:
            raise ValueError("malformed line: " + line)
        x, y = LETTERS.find(items[1][0]), LETTERS.find(items[1][-1])
        if x < 0 or (items[0] == "mis" and y < 0):
            raise ValueError("letter outside ACGT: " + line)
        sc = _round_half_away(math.log(float(items[2])) * 131072.0)
        if items[0] == "mat":
            s[x, x] = sc
        elif items[0] == "mis":
            s[x, y] = sc
        elif items[0] == "del":
            s[x, GAP] = sc
        else:
            s[GAP, x] = sc
    return s


# ---- std::sort of libstdc++ as a permutation ------------------------------------------------------------------------

def std_sort_perm(keys, trace=None, leaf=0):
    """the order std::sort(first, last, key(a) < key(b)) of libstdc++ leaves n elements in: introsort down to pieces of
    16 with the median of three moved to the front and an unguarded partition, heap sort where the depth budget
    2 * floor(log2 n) runs out, then one insertion pass.

    ``trace(first, last, depth, heap)`` is called for every range the introsort loop comes to hold, at the moment it gets
    it (the whole input, then both sides of every partition), with the depth budget left; ``heap`` says that the range
    is heap sorted because the budget ran out (more than 16 elements at depth 0).  ``leaf`` > 16: ranges of at most
    ``leaf`` elements are reported and then left as they are, and there is no insertion pass -- the partitions of the
    larger ranges alone, which is what a caller wants who asks where the pieces of that size come from."""
    n = len(keys)
    a = list(range(n))
    stop = max(16, leaf)

    def less(x, y):
        return keys[x] < keys[y]

    def adjust_heap(first, hole, length, value):
        top, child = hole, hole
        while child < (length - 1) // 2:
            child = 2 * (child + 1)
            if less(a[first + child], a[first + child - 1]):
                child -= 1
            a[first + hole] = a[first + child]
            hole = child
        if length % 2 == 0 and child == (length - 2) // 2:
            child = 2 * (child + 1)
            a[first + hole] = a[first + child - 1]
            hole = child - 1
        parent = (hole - 1) // 2
        while hole > top and less(a[first + parent], value):
            a[first + hole] = a[first + parent]
            hole = parent
            parent = (hole - 1) // 2
        a[first + hole] = value

    def heap_sort(first, last):
        length = last - first
        if length >= 2:
            parent = (length - 2) // 2
            while True:
                adjust_heap(first, parent, length, a[first + parent])
                if parent == 0:
                    break
                parent -= 1
        while last - first > 1:
            last -= 1
            value = a[last]
            a[last] = a[first]
            adjust_heap(first, 0, last - first, value)

    def partition_pivot(first, last):
        mid = first + (last - first) // 2
        x, y, z = first + 1, mid, last - 1
        if less(a[x], a[y]):
            m = y if less(a[y], a[z]) else (z if less(a[x], a[z]) else x)
        else:
            m = x if less(a[x], a[z]) else (z if less(a[y], a[z]) else y)
        a[first], a[m] = a[m], a[first]
        lo, hi = first + 1, last
        while True:
            while less(a[lo], a[first]):
                lo += 1
            hi -= 1
            while less(a[first], a[hi]):
                hi -= 1
            if not lo < hi:
                return lo
            a[lo], a[hi] = a[hi], a[lo]
            lo += 1

    def loop(first, last, depth):
        while True:
            if trace:
                trace(first, last, depth, last - first > stop and depth == 0)
            if last - first <= stop:
                return
            if depth == 0:
                heap_sort(first, last)
                return
            depth -= 1
            cut = partition_pivot(first, last)
            loop(cut, last, depth)
            last = cut

    def linear_insert(i):
        v = a[i]
        while less(v, a[i - 1]):
            a[i] = a[i - 1]
            i -= 1
        a[i] = v

    def insertion(first, last):
        for i in range(first + 1, last):
            if less(a[i], a[first]):
                v = a[i]
                a[first + 1:i + 1] = a[first:i]
                a[first] = v
            else:
                linear_insert(i)

    if n:
        loop(0, n, 2 * (n.bit_length() - 1))
        if leaf > 16:
            return a
        if n > 16:
            insertion(0, 16)
            for i in range(16, n):
                linear_insert(i)
        else:
            insertion(0, n)
    return a


# ---- the matrices and the scores ------------------------------------------------------------------------------------

def _pad(branch_cls, reverse):
    m = max([len(w) for w in branch_cls] + [0])
    out = np.full((len(branch_cls), m), 4, np.int64)
    for b, w in enumerate(branch_cls):
        out[b, :len(w)] = w[::-1] if reverse else w
    return out


def _fill(vc, wc, s):
    """F[i][b][j] for every branch b at once (rows of wc are the branches, padded to the right; a padded column never
    feeds a real one because a row only moves rightwards)"""
    nb, m = wc.shape
    f = np.zeros((len(vc) + 1, nb, m + 1), np.int64)
    p = np.zeros((nb, m + 1), np.int64)
    p[:, 1:] = np.cumsum(s[GAP][wc], axis=1)
    f[0] = p
    for i in range(1, len(vc) + 1):
        c = vc[i - 1]
        t = f[i - 1] + s[c, GAP]
        t[:, 1:] = np.maximum(t[:, 1:], f[i - 1][:, :-1] + s[c][wc])
        f[i] = p + np.maximum.accumulate(t - p, axis=1)
    return f


class Scores:
    """A(v) and every edit score of one candidate against a list of branches"""

    def __init__(self, v, branches, s):
        vc = classes(v)
        bc = [classes(w) for w in branches]
        lens = np.array([len(w) for w in bc], np.int64)
        L, nb = len(vc), len(bc)
        wc = _pad(bc, False)
        m = wc.shape[1]
        f = _fill(vc, wc, s)
        at = f[L][np.arange(nb), lens] if nb else np.zeros(0, np.int64)
        self.per_branch = np.where((lens > 0) & (L > 0), at, 0)
        self.total = int(self.per_branch.sum())
        self.f, self.s, self.wc, self.lens, self.vc, self.rc, self.bc = f, s, wc, lens, vc, None, bc
        self.L, self.m = L, m

    def edits(self):
        """(deletions [L], insertions [L + 1][4], substitutions [L][4]) as sums over the branches"""
        L, m, s, f, lens = self.L, self.m, self.s, self.f, self.lens
        r = _fill(self.vc[::-1], _pad(self.bc, True), s)
        j = np.arange(m + 1)[None, :]
        idx = np.clip(lens[:, None] - j, 0, None)
        flip = np.take_along_axis(r, np.broadcast_to(idx[None], r.shape), axis=2)
        flip[:, j[0][None, :] > lens[:, None]] = NEG
        back = flip[::-1]                               # back[k] = the R row L - k, columns as Lb - j
        dele = (f[:L] + back[1:]).max(axis=2).sum(axis=1) if L else np.zeros(0, np.int64)
        ins = np.zeros((L + 1, 4), np.int64)
        sub = np.zeros((L, 4), np.int64)
        for b in range(4):
            e = f + s[b, GAP]
            e[:, :, 1:] = np.maximum(e[:, :, 1:], f[:, :, :-1] + s[b][self.wc][None])
            ins[:, b] = (e + back).max(axis=2).sum(axis=1)
            if L:
                sub[:, b] = (e[:L] + back[1:]).max(axis=2).sum(axis=1)
        return dele, ins, sub


def alignment_score(v, branches, s):
    return Scores(v, branches, s).total


def make_step(v, branches, s, detail=None):
    """(sequence, score) of one step; detail (a dict) receives the stage, the best score and how many edits of that
    stage reach it"""
    sc = Scores(v, branches, s)
    best, seq = sc.total, v
    dele, ins, sub = sc.edits()
    stage = "none"
    for p in range(len(v)):
        if dele[p] > best:
            best, seq, stage = int(dele[p]), v[:p] + v[p + 1:], "del"
    if stage == "none":
        for p in range(len(v) + 1):
            for b in range(4):
                if ins[p, b] > best:
                    best, seq, stage = int(ins[p, b]), v[:p] + LETTERS[b] + v[p:], "ins"
    if stage == "none":
        for p in range(len(v)):
            for b in range(4):
                if LETTERS[b] == v[p]:
                    continue
                if sub[p, b] > best:
                    best, seq, stage = int(sub[p, b]), v[:p] + LETTERS[b] + v[p + 1:], "sub"
    if detail is not None:
        if stage == "sub":
            vals = [int(sub[p, b]) for p in range(len(v)) for b in range(4) if LETTERS[b] != v[p]]
        else:
            vals = {"del": dele, "ins": ins, "none": np.zeros(0)}[stage].ravel().tolist()
        detail.update(stage=stage, best=best, ties=sum(1 for x in vals if x == best))
    return seq, best


def optimize(v0, branches, s, steps, details=None):
    """-> (candidate, status bits)"""
    prev, it = v0, 0
    while True:
        d = {} if details is not None else None
        seq, score = make_step(prev, branches, s, d)
        steps.append((seq, score))
        if details is not None:
            details.append(d)
        if seq == prev:
            return prev, 0
        if score > 0:
            return prev, OVERFLOW
        it += 1
        if it - 1 > 10 * len(v0):
            return prev, ITER_LIMIT
        prev = seq


def middle_five(branches):
    order = std_sort_perm([len(w) for w in branches])
    left = len(branches) // 2 - 2
    return [branches[k] for k in order[left:left + 5]]


def dinucleotide_run(v):
    """(position, run) of the longest run of a pair of two different bases that is ended by a different pair"""
    max_run, max_pos = 0, 0
    if len(v) < 2:
        return 0, 0
    for shift in (0, 1):
        prev, run = "--", 0
        for pos in range((len(v) - shift) // 2):
            cur = v[pos * 2 + shift:pos * 2 + shift + 2]
            if cur != prev:
                if run > max_run and prev[0] != prev[1]:
                    max_run, max_pos = run, pos * 2 + shift - run * 2
                run, prev = 1, cur
            else:
                run += 1
    return max_pos, max_run


def polish_bubble(cand, branches, s, fix=True, details=None):
    """-> (candidate, [(sequence, score), ...], status bits)"""
    if not (len(cand) < MAX_BUBBLE and len(branches) > 1):
        return cand, [], SKIPPED
    steps, status = [], 0
    if len(branches) > 10:
        cand, st = optimize(cand, middle_five(branches), s, steps, details)
        status |= st
    cand, st = optimize(cand, branches, s, steps, details)
    status |= st
    if fix:
        pos, run = dinucleotide_run(cand)
        if run >= 3:
            inc = cand[:pos] + cand[pos:pos + 2] + cand[pos:]
            dec = cand[:pos] + cand[pos + 2:]
            normal = alignment_score(cand, branches, s)
            if alignment_score(inc, branches, s) > normal:
                cand, status = inc, status | FIXED
                steps.append((inc, 0))
            elif alignment_score(dec, branches, s) > normal:
                cand, status = dec, status | FIXED
                steps.append((dec, 0))
    return cand, steps, status


# ---- the file forms ---------------------------------------------------------------------------------------------------

class Bubble:
    def __init__(self, header, position, cand, branches):
        self.header, self.position, self.cand, self.branches = header, int(position), cand, list(branches)


def write_bubbles(bubbles):
    """the bubbles file: '>name position n', the candidate, then n pairs of (header line, sequence line)"""
    out = []
    for b in bubbles:
        out.append(">%s %d %d\n%s\n" % (b.header, b.position, len(b.branches), b.cand))
        for k, w in enumerate(b.branches):
            out.append(">%d\n%s\n" % (k, w))
    return "".join(out)


def parse_bubbles(text):
    """what the reference's reader makes of a bubbles file: everything upper-cased, the end at the first empty header
    line; ValueError where it throws"""
    lines = text.split("\n")
    at = 0

    def getline():
        nonlocal at
        line = lines[at] if at < len(lines) else ""
        at += 1
        return line

    out = []
    while at < len(lines):
        buf = getline()
        if not buf:
            break
        elems = buf.split(" ")
        if len(elems) < 3 or not elems[0].startswith(">"):
            raise ValueError("Error parsing bubbles file")
        cand = getline().upper()
        n = int(elems[2])
        branches = []
        while len(branches) < n:
            if not buf:
                break
            getline()
            buf = getline().upper()
            branches.append(buf)
        if len(branches) != n:
            raise ValueError("Error parsing bubbles file")
        out.append(Bubble(elems[0][1:], int(elems[1]), cand, branches))
    return out


def consensus_order(n):
    """the order one worker thread writes n bubbles in: blocks of BUBBLES_CACHE as read, each block last to first"""
    order = []
    for a in range(0, n, BUBBLES_CACHE):
        order += list(range(min(a + BUBBLES_CACHE, n) - 1, a - 1, -1))
    return order


def write_consensus(bubbles, cands):
    return "".join(">%s %d %d\n%s\n" % (bubbles[i].header, bubbles[i].position, len(bubbles[i].branches), cands[i])
                   for i in consensus_order(len(bubbles)))


def write_log(steps_per_bubble):
    """the --debug log: steps_per_bubble[i] = [(sequence, score), ...] in the order of consensus_order"""
    out = []
    for i in consensus_order(len(steps_per_bubble)):
        for seq, score in steps_per_bubble[i]:
            out.append("%-22s%s\n%-22s%d\n\n" % ("Consensus: ", seq, "Score: ", score))
        out.append("-----------------\n")
    return "".join(out)


def parse_log(text):
    """-> per bubble, in file order, [(sequence, score), ...]"""
    out, cur = [], []
    lines = text.split("\n")
    k = 0
    while k < len(lines):
        if lines[k].startswith("Consensus: "):
            cur.append((lines[k][22:], int(lines[k + 1][22:])))
            k += 3
        elif lines[k] == "-----------------":
            out.append(cur)
            cur = []
            k += 1
        else:
            k += 1
    return out


def read_gz(name):
    with gzip.open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read().decode("latin-1")


# ---- inputs -------------------------------------------------------------------------------------------------------------

def mutate(rng, seq, rate):
    out = []
    for c in seq:
        if rng.random() < rate:
            kind = rng.integers(3)
            if kind == 0:
                out.append(LETTERS[rng.integers(4)])
            elif kind == 1:
                out.append(c)
                out.append(LETTERS[rng.integers(4)])
        else:
            out.append(c)
    return "".join(out)


def generate(seed, n, cand_len=(1, 60), n_branches=(2, 50), rate=0.15, name="ctg"):
    """seeded bubbles: a random truth, the candidate and every branch mutated from it at `rate` (a string mutated to
    nothing is replaced by the truth: the reference's reader throws on an empty branch that is not the last line)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        truth = "".join(LETTERS[k] for k in rng.integers(4, size=int(rng.integers(cand_len[0], cand_len[1] + 1))))
        cand = mutate(rng, truth, rate) or truth
        nb = int(rng.integers(n_branches[0], n_branches[1] + 1))
        out.append(Bubble("%s_%d" % (name, seed), i * 100, cand, [mutate(rng, truth, rate) or truth for _ in range(nb)]))
    return out


def generate_fast(seed, n, cand_len=(50, 100), n_branches=(2, 50), rate=0.15, name="bench"):
    """the same kind of bubbles as generate(), drawn a string at a time (for tools/polish_bench.py and the reference's
    timing: tens of thousands of bubbles); bubble i does not depend on n"""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(LETTERS.encode(), np.uint8)

    def mut(truth):
        k = len(truth)
        hit = rng.random(k) < rate
        kind = rng.integers(3, size=k)
        new = letters[rng.integers(4, size=k)]
        two = np.stack([np.where(hit & (kind == 0), new, truth), new], axis=1)
        keep = np.stack([~(hit & (kind == 2)), hit & (kind == 1)], axis=1)
        out = two[keep]
        return (out if len(out) else truth).tobytes().decode()

    out = []
    for i in range(n):
        truth = letters[rng.integers(4, size=int(rng.integers(cand_len[0], cand_len[1] + 1)))]
        cand = mut(truth)
        nb = int(rng.integers(n_branches[0], n_branches[1] + 1))
        out.append(Bubble("%s_%d" % (name, seed), i * 100, cand, [mut(truth) for _ in range(nb)]))
    return out


def _rand(rng, n):
    return "".join(LETTERS[k] for k in rng.integers(4, size=n))


def crafted_pacbio():
    """the crafted bubbles of golden run (a); the name says what each is for.  Lower case is written into the file as it
    is here (the reader upper-cases it)."""
    rng = np.random.default_rng(7)
    out = []

    def add(name, cand, branches):
        out.append(Bubble(name, len(out), cand, branches))

    add("empty_candidate", "", ["ACGT", "ACT", "AGT"])
    add("classes_n", "ACNGTNA", ["ACGGTCA", "ACNGTA", "ACGTNA", "ANGTCA"])
    add("classes_lower", "acgtacgt", ["acgtaCGt", "ACGTTCGT", "acgacgt"])
    add("classes_gap", "AC-GT-A", ["ACGGTA", "AC-GTA", "ACGT-A", "ACGTA"])
    add("iteration_limit", "A", [_rand(rng, 30), _rand(rng, 30)])
    # stops on the limit before the run of AT is complete, so the fixer has something to do
    add("iteration_limit_fixer", "A", ["CGCATATATATAGA"] * 3)
    add("skip_one_branch", "ACGTACGT", ["ACGTTACGT"])
    add("skip_5000", _rand(rng, 5000), ["ACG", "ACT"])
    # the dinucleotide fixer's run search and its three scores (optimize has converged here, so nothing changes; the
    # runs that grow and shrink are in crafted_overflow): runs of 4 and of 2, the longest run at the end of the string
    # (never counted), equal runs at shift 0 and shift 1
    add("dinuc_grow", "GGCATATATATCCGA", ["GGCATATATATATCCGA"] * 3 + ["GGCATATATATCCGA"] * 2)
    add("dinuc_shrink", "GGCATATATATCCGA", ["GGCATATATCCGA"] * 3 + ["GGCATATATATCCGA"] * 2)
    add("dinuc_run2", "GGCATATCCGA", ["GGCATATATCCGA", "GGCATATCCGA", "GGCATCCGA"])
    add("dinuc_at_end", "GGACACACCTGTGTGTG", ["GGACACACACCTGTGTGTG", "GGACACACCTGTGTGTGTG", "GGACACACCTGTGTGTG"])
    add("dinuc_both_shifts", "CACACACTTGAGAGAGC", ["CACACACACTTGAGAGAGC", "CACACACTTGAGAGAGAGC", "CACACACTTGAGAGAGC",
                                                 "CACACACTTGAGAGAGC"])
    # sizes at the edges of a piece of 64 columns
    for n in (1, 2, 63, 64, 65, 127, 128, 129):
        truth = _rand(rng, n)
        add("size_%d" % n, mutate(rng, truth, 0.08) or truth, [mutate(rng, truth, 0.08) or truth for _ in range(3)] + [truth])
    truth = _rand(rng, 70)
    add("size_mixed", truth[:64], [truth[:1], truth[:2], truth[:63], truth[:64], truth[:65], truth + truth[:57],
                                   truth + truth[:58], truth + truth[:59]])
    # branch counts around the pre-polish threshold (10 / 11) and the threshold of std::sort's insertion pass (16 / 17),
    # with many equal lengths
    for nb in (2, 10, 11, 16, 17, 50):
        truth = _rand(rng, 24)
        branches = []
        for k in range(nb):
            w = mutate(rng, truth, 0.15)
            # three lengths only, so that the unstable sort has ties to permute
            w = (w + truth)[:22 + k % 3]
            branches.append(w)
        add("count_%d" % nb, mutate(rng, truth, 0.15) or truth, branches)
    for nb in (23, 37):
        truth = _rand(rng, 30)
        branches = [(mutate(rng, truth, 0.2) + truth)[:28 + (k * 7) % 4] for k in range(nb)]
        add("count_%d" % nb, mutate(rng, truth, 0.2) or truth, branches)
    return out


def crafted_empty_branch():
    """a bubble whose last branch is empty; it closes the file of run (a)"""
    return [Bubble("plain", 0, "ACGTTGCA", ["ACGTGCA", "ACGTTGCA", "ACGTTTGCA"]),
            Bubble("empty_branch", 1, "ACGT", ["ACGT", ""])]


def crafted_ties():
    """golden run (c), under tie.mat"""
    return [Bubble("tie_insert", 0, "AT", ["ACT", "AGT"]),
            Bubble("tie_delete", 1, "ACGT", ["AGT", "ACT"]),
            Bubble("tie_substitute", 2, "ATA", ["ACA", "ACA", "AGA", "AGA", "ATA"]),
            Bubble("tie_insert_t", 3, "CC", ["CTC", "CGC", "CAC"])]


def crafted_overflow():
    """golden run (d), under pos.mat"""
    return [Bubble("overflow", 0, "AAC", ["AAAC", "AAAC"]),
            Bubble("after_overflow", 1, "ACGGT", ["ACGT", "ACGT", "ACGGT"]),
            # optimize stops on its first step (score > 0) and leaves the run as it is: the fixer grows / shrinks it
            Bubble("dinuc_grow", 2, "A" * 40 + "GCTATATATCCG", ["A" * 40 + "GCTATATATATCCG"] * 3),
            Bubble("dinuc_shrink", 3, "A" * 40 + "GCTATATATATCCG", ["A" * 40 + "GCTATATATCCG"] * 3 + ["A" * 40 + "GCTATATATATCCG"])]


RUNS = {
    # name: (matrix file under tests/golden/bin_cfg, the bubbles)
    "polish_a": ("pacbio_substitutions.mat", lambda: crafted_pacbio() + generate(101, 150) + crafted_empty_branch()),
    "polish_b": ("nano_r94_substitutions.mat", lambda: generate(202, 60, name="nano")),
    "polish_c": ("tie.mat", crafted_ties),
    "polish_d": ("pos.mat", crafted_overflow),
}


def flatten(bubbles):
    """the five flat arrays of fg_polish_bubbles"""
    cand = "".join(b.cand for b in bubbles).encode("latin-1")
    cand_off = np.zeros(len(bubbles) + 1, np.uint64)
    cand_off[1:] = np.cumsum([len(b.cand) for b in bubbles])
    all_br = [w for b in bubbles for w in b.branches]
    br = "".join(all_br).encode("latin-1")
    br_off = np.zeros(len(all_br) + 1, np.uint64)
    br_off[1:] = np.cumsum([len(w) for w in all_br])
    bb_off = np.zeros(len(bubbles) + 1, np.uint64)
    bb_off[1:] = np.cumsum([len(b.branches) for b in bubbles])
    return cand, cand_off, br, br_off, bb_off
