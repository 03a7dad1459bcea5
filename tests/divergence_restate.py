"""A second writing of Trestle's divergence profile (flye/trestle/divergence.py: _contig_profile, _count_freqs,
_call_position and the three writers) in the forms the device uses, and the inputs of tests/test_divergence.py.  Nothing
here is copied from the reference: tests/golden/make_divergence_golden.py runs the reference's own functions on these
inputs and stores what they give.

Forms that differ from the reference's loops, each pinned by the golden runs:
* matches and insertions are dense tables position x byte; beside every count stands the smallest (alignment, column)
  that added to it.  max(d, key=d.get) returns the key that entered the dict first, so a tie of the largest count goes
  to the smallest such pair, not to the smallest byte;
* nucl is the byte of the largest (alignment, column) that set it;
* ct / float(cov) >= thresh is ct >= the smallest count that passes, found per coverage by dividing in double;
* the summary's windows are counted by position // 1000.

Inputs: the crafted run divergence_e, the seeded run divergence_f, fuzz seeds, and two SAM files."""
import collections
import hashlib
import json
import math

import numpy as np

import bubbles_restate as R
import cigar_restate as G

WINDOW = 1000
VALUE_KEYS = ("cov", "nucl", "mat_ct", "sub_base", "sub_ct", "del_ct", "ins_base", "ins_ct", "flags")
LIST_KEYS = ("total", "sub", "del", "ins")
NO_TAG = (1 << 62, 0)


def min_count(thresh, cov):
    """the smallest ct with ct / float(cov) >= thresh (None: no count passes)"""
    if math.isinf(thresh):
        return None
    ct = max(0, int(math.ceil(thresh * cov)))
    while ct > 0 and (ct - 1) / float(cov) >= thresh:
        ct -= 1
    while ct / float(cov) < thresh:
        ct += 1
    return ct


def divergence(alns, length, thresholds):
    """alns in list order -> dict of the arrays of VALUE_KEYS per position (sub_base / ins_base 0 for none), the four
    ascending lists of LIST_KEYS, and ins_table (position x byte counts of insertions, for the tests)"""
    mat = np.zeros((length, 128), np.int64)
    ins = np.zeros((length, 128), np.int64)
    mat_first, ins_first = {}, {}
    tag = [0] * length
    for k, aln in enumerate(alns):
        qry = R.shift_gaps(aln.trg_seq, aln.qry_seq)
        trg = R.shift_gaps(qry, aln.trg_seq)
        t = np.frombuffer(trg.encode("latin-1"), np.uint8)
        q = np.frombuffer(qry.encode("latin-1"), np.uint8)
        ng = t != 45
        before = np.cumsum(ng) - ng
        pos = np.where(ng, aln.trg_start + before, aln.trg_start + before - 1)
        pos = np.where(pos >= length, pos - length, pos)
        pos = np.where(pos < 0, length - 1, pos)
        for col in range(len(t)):
            p, b = int(pos[col]), int(q[col])
            if ng[col]:
                mat[p, b] += 1
                mat_first.setdefault((p, b), (k, col))
                tag[p] = max(tag[p], ((k + 1) << 40) | (col << 8) | int(t[col]))
            else:
                ins[p, b] += 1
                ins_first.setdefault((p, b), (k, col))
    out = {key: np.zeros(length, np.uint8 if key in ("nucl", "sub_base", "ins_base", "flags") else np.int32) for key in VALUE_KEYS}
    lists = {key: [] for key in LIST_KEYS}
    tables = {}
    for p in range(length):
        nucl = (tag[p] & 255) if tag[p] else 45
        cov = int(mat[p].sum())
        best = lambda table, first, skip: min(((-int(table[p, b]), first[(p, b)], b) for b in range(128) if table[p, b] and b not in skip),
                                              default=(0, NO_TAG, 0))
        sub, insb = best(mat, mat_first, (nucl, 45)), best(ins, ins_first, ())
        row = dict(cov=cov, nucl=nucl, mat_ct=int(mat[p, nucl]), sub_base=sub[2], sub_ct=-sub[0], del_ct=int(mat[p, 45]), ins_base=insb[2],
                   ins_ct=-insb[0])
        flags = 0
        if cov:
            if cov not in tables:
                tables[cov] = [min_count(t, cov) for t in thresholds]
            for bit, key in enumerate(("sub_ct", "del_ct", "ins_ct")):
                if tables[cov][bit] is not None and row[key] >= tables[cov][bit]:
                    flags |= 1 << bit
                    lists[LIST_KEYS[bit + 1]].append(p)
            if flags:
                lists["total"].append(p)
        row["flags"] = flags
        for key in VALUE_KEYS:
            out[key][p] = row[key]
    out.update(lists)
    out["ins_table"] = ins
    return out


# ---- the three writers -----------------------------------------------------------------------------------------------
def frequency_text(res):
    out = ["Index\tCov\tMatch\tCount\tSub\tCount\tDel\tCount\tIns\tCount\n"]
    name = lambda b: chr(b) if b else ""
    for p in range(len(res["cov"])):
        out.append("\t".join([str(p), str(res["cov"][p]), chr(res["nucl"][p]), str(res["mat_ct"][p]), name(res["sub_base"][p]),
                              str(res["sub_ct"][p]), "-", str(res["del_ct"][p]), "^" + name(res["ins_base"][p]), str(res["ins_ct"][p])]) + "\n")
    return "".join(out)


def positions_text(res, thresholds):
    s, d, i = thresholds
    heads = ["Total_positions_%d_with_thresholds_sub_%s_del_%s_ins_%s" % (len(res["total"]), s, d, i),
             "Sub_positions_%d_with_threshold_sub_%s" % (len(res["sub"]), s), "Del_positions_%d_with_threshold_del_%s" % (len(res["del"]), d),
             "Ins_positions_%d_with_threshold_ins_%s" % (len(res["ins"]), i)]
    return "".join(">%s\n%s\n" % (h, ",".join(map(str, res[k]))) for h, k in zip(heads, LIST_KEYS))


def summary_text(res, length):
    called = res["total"]
    gaps = [b - a for a, b in zip([0] + called, called + [length])]
    counts = [0] * ((length - 1) // WINDOW + 1)
    for p in called:
        counts[p // WINDOW] += 1
    divs = [counts[w] / float(min((w + 1) * WINDOW, length) - w * WINDOW) for w in range(len(counts))]
    ordered, mid = sorted(divs), len(divs) // 2
    median = ordered[mid] if len(divs) % 2 else (ordered[mid - 1] + ordered[mid]) / 2
    n = {k: len(res[k]) for k in LIST_KEYS}
    lines = ["Tentative Divergent Position Summary\n\n", "%-33s\t%d\n" % ("Sequence Length:", length),
             "%-33s\t%.4f\n\n" % ("Average Divergence:", len(called) / float(length)),
             "%-33s\t%d\n" % ("Total Substitution Positions:", n["sub"]), "%-33s\t%d\n" % ("Total Deletion Positions:", n["del"]),
             "%-33s\t%d\n" % ("Total Insertion Positions:", n["ins"]), "%-33s\t%d\n" % ("Total Positions:", n["total"]),
             "%-33s\t%d\n\n" % ("Mixed Positions:", n["sub"] + n["del"] + n["ins"] - n["total"]),
             "%-33s\t%.2f\n" % ("Mean Position Gap:", sum(gaps) / len(gaps)), "%-33s\t%d\n" % ("Max Position Gap:", max(gaps)),
             "%-33s\t%d\n" % ("Window Length:", WINDOW), "%-33s\t%.5f\n" % ("Mean Window Divergence:", sum(divs) / len(divs)),
             "%-33s\t%.5f\n" % ("Median Window Divergence:", median), "%-33s\t%.5f\n" % ("Min Window Divergence:", min(divs))]
    return "".join(lines)


def texts(res, length, thresholds):
    return dict(frequency=frequency_text(res), positions=positions_text(res, thresholds), summary=summary_text(res, length))


def digests(res):
    d = {k: hashlib.sha256(np.ascontiguousarray(res[k]).tobytes()).hexdigest() for k in VALUE_KEYS}
    d.update({k: hashlib.sha256(np.array(res[k], np.int32).tobytes()).hexdigest() for k in LIST_KEYS})
    return d


def text_digests(t):
    return {k: hashlib.sha256(v.encode("latin-1")).hexdigest() for k, v in t.items()}


# ---- the crafted run -------------------------------------------------------------------------------------------------
THRESHOLDS = (0.1, 0.2, 0.3)
EDGE_COLUMNS = (1, 63, 64, 65, 128, 129)
TILE_COLUMNS = (1023, 1024, 1025, 2049)           # around one and two tiles of the counting kernel


def _set(seq, at, ch):
    return seq[:at] + ch + seq[at + 1:]


def cols(cid, seq, start, end, qid, ins=None, sub=None, dele=(), lead="", trg_sub=None):
    """seq[start:end] (end may pass the contig's end: the alignment wraps) with strings inserted behind positions, query
    bases replaced or deleted, target bytes replaced (trg_sub), and `lead` inserted before the first column"""
    ins, sub, trg_sub = ins or {}, sub or {}, trg_sub or {}
    L = len(seq)
    t, q = ["-" * len(lead)], [lead]
    for p in range(start, end):
        base = seq[p % L]
        t.append(trg_sub.get(p, base))
        q.append("-" if p in dele else sub.get(p, base))
        if p in ins:
            t.append("-" * len(ins[p]))
            q.append(ins[p])
    return R.record(cid, L, start, "".join(t), "".join(q), qid, 0.01 * (1 + len(qid) % 7))


def exact_columns(rng, cid, seq, start, n_cols, qid):
    """an alignment of exactly n_cols columns from start: about one column in nine an insertion, some substitutions"""
    n_ins = n_cols // 9
    n_trg = n_cols - n_ins
    behind = set(int(x) for x in rng.choice(np.arange(start, start + n_trg), n_ins, replace=False)) if n_ins else set()
    ins = {p: "ACGT"[int(rng.integers(0, 4))] for p in behind}
    sub = {int(p): "ACGT"[int(rng.integers(0, 4))] for p in rng.integers(start, start + n_trg, n_trg // 12)}
    a = cols(cid, seq, start, start + n_trg, qid, ins, sub)
    assert len(a.trg_seq) == n_cols
    return a


def stack(cid, seq, n, plan):
    """n alignments over the whole of seq; plan = {alignment index: keyword arguments of cols}"""
    return [cols(cid, seq, 0, len(seq), "%s_%d" % (cid, k), **plan.get(k, {})) for k in range(n)]


def run_e():
    rng = np.random.default_rng(606)
    contigs, alns = [], {}

    def add(cid, seq, lst, kind="linear"):
        assert len(seq) < 3000
        contigs.append((R.Contig(cid, len(seq), kind), seq))
        alns[cid] = lst

    # alignments of 1 .. 129 columns, and around the tiles of the counting kernel
    seq = R.rand_seq(rng, 2600)
    add("edges", seq, [exact_columns(rng, "edges", seq, 40 * k, n, "e%d" % n) for k, n in enumerate(EDGE_COLUMNS)] +
        [exact_columns(rng, "edges", seq, 300 + 60 * k, n, "t%d" % n) for k, n in enumerate(TILE_COLUMNS)])
    # ties.  Ten alignments: cov 10 everywhere, so one substitution is 1/10 = sub_thresh exactly
    seq = R.rand_seq(rng, 120)
    for at in (20, 40, 80, 100, 119):
        seq = _set(seq, at, "A")
    seq = _set(seq, 60, "C")              # neither 'A' nor 'G': shift_gaps leaves the insertions behind 60 where they are
    plan = {
        # 20: 'T' (alignment 0) against 'C' (alignment 1), one each: first arrival says T, byte order C
        0: dict(sub={20: "T", 80: "N", 100: "g"}, ins={60: "GA"}, lead="GA"),
        1: dict(sub={20: "C", 80: "c", 100: "G"}, ins={60: "AG"}, lead="AG"),
        # 60 and the lead: "GA" against "AG" make G 2 and A 2; G entered first.  The lead lands on the last position
        2: dict(sub={80: "c"}),
        3: dict(sub={80: "N"}),
        # 100: 'g' then 'G', one each: case is kept, first arrival says g
    }
    lst = stack("ties", seq, 10, plan)
    # 40: alignment 4 starts at 0 and reaches position 40 at column 40 with 'T'; an eleventh alignment starts at 40 and has
    # 'C' at its column 0: the earlier alignment has the later column, and still wins
    lst[4] = cols("ties", seq, 0, 120, "ties_4", sub={40: "T"})
    lst.append(cols("ties", seq, 40, 120, "ties_10", sub={40: "C"}))
    add("ties", seq, lst)
    # a '-' against a '-'; a position nobody covers; a position everybody deletes; nucl from a later alignment's target
    seq = _set(_set(_set(R.rand_seq(rng, 200), 30, "A"), 150, "A"), 29, "C")        # 29: the deletion at 30 stays at 30
    left = [cols("odd", seq, 0, 90, "l%d" % k, ins={10: "-"} if k == 0 else {}, dele=(30,), trg_sub={50: "G"} if k == 2 else {})
            for k in range(3)]
    right = [cols("odd", seq, 120, 200, "r%d" % k, sub={150: "t"} if k else {}) for k in range(3)]
    add("odd", seq, left + right)
    # a circular contig: alignments start at 250 and wrap, with an insertion behind the last position and one behind
    # position 0; one alignment starts at 0 with an insertion before its first column
    seq = _set(_set(R.rand_seq(rng, 300), 299, "A"), 0, "A")
    lst = [cols("circ", seq, 250, 480, "w%d" % k, ins={299: "CT", 300: "G"}) for k in range(3)]
    lst.append(cols("circ", seq, 0, 250, "z0", lead="TC"))
    add("circ", seq, lst, "circular")
    # thresholds hit exactly.  30 alignments: 3/30 substitutions, 6/30 deletions, 9/30 insertions, and one below each
    seq = R.rand_seq(rng, 100)
    for at in (10, 20, 30, 40, 50, 60):
        seq = _set(_set(seq, at, "A"), at - 1, "C")           # at - 1: shift_gaps leaves a deletion at `at` where it is
    plan = collections.defaultdict(lambda: dict(sub={}, dele=set(), ins={}))
    for at, kind, n in ((10, "sub", 3), (20, "sub", 2), (30, "dele", 6), (40, "dele", 5), (50, "ins", 9), (60, "ins", 8)):
        for k in range(n):
            if kind == "sub":
                plan[k]["sub"][at] = "C"
            elif kind == "dele":
                plan[k]["dele"].add(at)
            else:
                plan[k]["ins"][at] = "T"
    add("c30", seq, stack("c30", seq, 30, plan))
    # 70 alignments over every position: 7/70 passes; 21 alignments: 2/21 does not
    seq = _set(R.rand_seq(rng, 90), 45, "A")
    add("c70", seq, stack("c70", seq, 70, {k: dict(sub={45: "G"}) for k in range(7)}))
    seq = _set(R.rand_seq(rng, 90), 45, "A")
    add("c21", seq, stack("c21", seq, 21, {k: dict(sub={45: "G"}) for k in range(2)}))
    # a contig without alignments
    add("bare", R.rand_seq(rng, 50), [])
    order = ["edges", "bare", "odd", "circ", "c30", "c70", "c21", "ties"]         # the last one's texts are stored whole
    contigs.sort(key=lambda c: order.index(c[0].id))
    return dict(thresholds=THRESHOLDS, contigs=contigs, alns=alns)


def run_f():
    """seeded alignments with substitutions, insertions and deletions, linear and circular, N and lower case"""
    rng = np.random.default_rng(707)
    contigs, alns = [], {}
    for cid, L, n, kind in (("f_lin", 2500, 40, "linear"), ("f_circ", 900, 35, "circular"), ("f_small", 130, 25, "linear")):
        seq = G.rand_contig(rng, L)
        lst = []
        for k in range(n):
            n_trg = int(rng.integers(min(60, L // 2), L + 1))
            start = int(rng.integers(0, L)) if kind == "circular" else int(rng.integers(0, L - n_trg + 1))
            lst.append(R.gen_aln(rng, cid, seq, start, n_trg, 0.05, 0.04, 0.04, "q%d" % k))
        contigs.append((R.Contig(cid, L, kind), seq))
        alns[cid] = lst
    return dict(thresholds=(0.15, 0.1, 0.05), contigs=contigs, alns=alns)


RUNS = dict(divergence_e=run_e, divergence_f=run_f)


def fuzz(seed):
    run = R.fuzz(seed)
    rng = np.random.default_rng(seed)
    return dict(thresholds=tuple(float(x) for x in rng.choice([0.0, 0.05, 0.1, 0.25, 0.5, 1.0, 1.5], 3)), contigs=run["contigs"],
                alns=run["alns"])


def restate_run(run):
    return {c.id: divergence(run["alns"][c.id], c.length, run["thresholds"]) for c, _ in run["contigs"]}


def input_digest(run):
    h = hashlib.sha256(json.dumps(list(run["thresholds"])).encode())
    h.update(R.input_digest(run).encode())
    return h.hexdigest()


# ---- the SAM files ---------------------------------------------------------------------------------------------------
SAM_THRESHOLDS = (0.1, 0.2, 0.3)


def _sam(seed, sizes):
    """sizes: (contig id, length, records, longest target span); a contig with 0 records has none in the file"""
    rng = np.random.default_rng(seed)
    contigs = {cid: G.rand_contig(rng, n) for cid, n, _, _ in sizes}
    text = ["@HD\tVN:1.6\tSO:coordinate\n"] + ["@SQ\tSN:%s\tLN:%d\n" % (cid, n) for cid, n, _, _ in sizes]
    k = 0
    for cid, n, count, span in sizes:
        for _ in range(count):
            n_trg = int(rng.integers(span // 2, span + 1))
            start = int(rng.integers(0, n - n_trg + 1))
            runs = G.noisy_runs(rng, n_trg, max_run=12)
            if k % 4 == 1:
                runs = [("S", int(rng.integers(1, 9)))] + runs
            text.append(G.sam_line("read_%d" % k, 16 if k % 3 == 1 else 0, cid, start + 1, G.cigar_of(runs),
                                   G.noisy_read(rng, contigs[cid], start, runs, sub=0.08)))
            k += 1
    return dict(sam="".join(text).encode(), contigs=contigs, thresholds=SAM_THRESHOLDS)


def sam_one():
    return _sam(808, (("template_1", 1200, 40, 500),))


def sam_three():
    return _sam(909, (("ctg_a", 700, 25, 300), ("ctg_none", 400, 0, 0), ("ctg_b", 900, 30, 400)))


SAMS = dict(sam_one=sam_one, sam_three=sam_three)


def fasta_of(contigs):
    return "".join(">%s\n%s\n" % (cid, seq) for cid, seq in contigs.items())


def sam_digest(run):
    h = hashlib.sha256(run["sam"])
    h.update(fasta_of(run["contigs"]).encode())
    h.update(json.dumps(list(run["thresholds"])).encode())
    return h.hexdigest()
