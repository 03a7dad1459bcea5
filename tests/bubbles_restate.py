"""A second writing of the reference's bubble partition (flye/polishing/bubbles.py: _compute_profile, _get_partition,
_get_bubble_seqs, _postprocess_bubbles; flye/polishing/alignment.py: shift_gaps) in the forms the device uses, and the
seeded generator of the golden inputs.  Nothing here is copied from the reference: tests/golden/make_bubbles_golden.py
runs the reference's own functions on these inputs and stores what they give; tests/test_bubbles.py pins this file on
those records, bubble by bubble, and the device on both.

Forms that differ from the reference's loops, each pinned by the golden runs:
* shift_gaps closes a gap run [a, b) by counting m = the k < min(b - a, a) in a row with second[a-1-k] == first[b-1-k]
  and moving the block of m bases at once.  The "$" sentinels only close a run at the end and stop the walk at column 0.
* the first loop of _get_partition in closed form: in a maximal run of good positions [s, e] the greedy walk marks
  min((e - s + 1) // SOLID, (len - SOLID - 1 - s) // SOLID + 1) k-mers from s on, none when s >= len - SOLID.
* the second loop jumps from event to event: the next landmark or prev_partition + max_bubble_length + 1.
* a cut of _get_bubble_seqs is a non-gap target column at position 0 or at a partition point, except the alignment's
  first non-gap column unless it is position 0 (positions rise by one, so "trg_pos >= next_bubble_start" first holds AT
  the partition point).
* _postprocess_bubbles in integers: incons_rate < 0.5 is 2 |d| < med (|d| / med <= 1/2 - 1/(2 med), further from 1/2 than
  a double rounds for med < 2^31); len > MAX_BUBBLE * 1.5 is 2 len > 3 MAX_BUBBLE (1.5 * int is exact in double).  A branch
  of length 0 never passes 2 |d| < med (it gives 2 med < med), so the reference's '"A" for an empty branch' cannot run.
* the two rate tests through a table: per coverage the largest numerator n with n / coverage <= rate in double."""
import bisect
import collections
import gzip
import hashlib
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

Aln = collections.namedtuple("Aln", ["qry_id", "trg_id", "qry_start", "qry_end", "qry_sign", "qry_len", "trg_start", "trg_end",
                                     "trg_sign", "trg_len", "qry_seq", "trg_seq", "err_rate", "is_secondary"])
Contig = collections.namedtuple("Contig", ["id", "length", "type"])

DEFAULTS = dict(simple_kmer_length=4, solid_kmer_length=10, max_bubble_length=500, max_bubble_branches=50,
                min_polish_aln_len=500)
ERR_MODES = dict(pacbio=dict(solid_missmatch=0.2, solid_indel=0.2, max_aln_error=0.25),
                 nano=dict(solid_missmatch=0.3, solid_indel=0.3, max_aln_error=0.25))

_FROM = b"URYKMSWBVDHNXurykmswbvdhnx"
_TO = b"ACGTACGTACGTAacgtacgtacgta"
TO_ACGT = bytes.maketrans(_FROM, _TO)


def params_for(err_mode, overrides=None):
    p = dict(DEFAULTS)
    p.update(ERR_MODES[err_mode])
    p.update(overrides or {})
    return p


def supported(p):
    s, k = p["simple_kmer_length"], p["solid_kmer_length"]
    return s % 2 == 0 and s >= 2 and s <= 2 * k and 3 * s // 2 <= k + 1


# ---- shift_gaps --------------------------------------------------------------------------------------------------
def shift_gaps(first, second, events=None):
    """second with every gap run moved left as far as first allows; events (optional list) receives (a, b, m, reached)
    per run, reached = the walk compared a byte that an earlier run had written"""
    f = first.encode("latin-1")
    out = bytearray(second.encode("latin-1"))
    n = len(out)
    written = set()
    i = 0
    while i < n:
        if out[i] != 45:
            i += 1
            continue
        a = i
        while i < n and out[i] == 45:
            i += 1
        b = i
        lim = min(b - a, a)
        m = 0
        reached = False
        while m < lim:
            reached = reached or (a - 1 - m) in written
            if out[a - 1 - m] != f[b - 1 - m]:
                break
            m += 1
        if m:
            block = bytes(out[a - m:a])
            out[a - m:a] = b"-" * m
            out[b - m:b] = block
            if events is not None:
                written.update(range(a - m, a))
                written.update(range(b - m, b))
        if events is not None:
            events.append((a, b, m, reached))
    return out.decode("latin-1")


# ---- the profile -------------------------------------------------------------------------------------------------
def in_profile(aln, p):
    return not (aln.err_rate > p["max_aln_error"]) and len(aln.qry_seq) >= p["min_polish_aln_len"]


def profile(alns, p, length):
    """-> dict of int32 arrays coverage / num_inserts / num_deletions / num_missmatch, nucl (uint8, 0 = no base),
    has (bool: a base was set), aln_errors, in_profile"""
    cov, ins, dele, mis = (np.zeros(length, np.int32) for _ in range(4))
    tag = np.zeros(length, np.int64)
    errors, flags = [], []
    for k, aln in enumerate(alns):
        ok = in_profile(aln, p)
        flags.append(int(ok))
        if not ok:
            continue
        errors.append(aln.err_rate)
        qry = shift_gaps(aln.trg_seq, aln.qry_seq)
        trg = shift_gaps(qry, aln.trg_seq)
        t = np.frombuffer(trg.encode("latin-1"), np.uint8)
        q = np.frombuffer(qry.encode("latin-1"), np.uint8)
        ng = t != 45
        before = np.cumsum(ng) - ng              # non-gap target columns before the column
        pos = aln.trg_start + before
        pos_ng = pos[ng]
        pos_ng = np.where(pos_ng >= length, pos_ng - length, pos_ng)
        np.add.at(cov, pos_ng, 1)
        np.add.at(dele, pos_ng[q[ng] == 45], 1)
        np.add.at(mis, pos_ng[(q[ng] != 45) & (q[ng] != t[ng])], 1)
        tag[pos_ng] = np.maximum(tag[pos_ng], ((k + 1) << 8) | t[ng].astype(np.int64))
        pos_g = pos[~ng] - 1
        pos_g = np.where(pos_g >= length, pos_g - length, pos_g)
        pos_g = np.where(pos_g < 0, length - 1, pos_g)
        np.add.at(ins, pos_g, 1)
    return dict(coverage=cov, num_inserts=ins, num_deletions=dele, num_missmatch=mis, nucl=(tag & 255).astype(np.uint8),
                has=tag != 0, aln_errors=errors, in_profile=flags)


def max_numerator(rate, cov):
    """the largest integer n with n / cov <= rate (Python's true division)"""
    n = int(math.floor(rate * cov))
    while (n + 1) / cov <= rate:
        n += 1
    while n > 0 and n / cov > rate:
        n -= 1
    return n


def good_positions(prof, p):
    cov = prof["coverage"]
    top = int(cov.max()) if len(cov) else 0
    tab_m = np.array([0] + [max_numerator(p["solid_missmatch"], c) for c in range(1, top + 1)], np.int64)
    tab_i = np.array([0] + [max_numerator(p["solid_indel"], c) for c in range(1, top + 1)], np.int64)
    return (cov > 0) & (prof["num_missmatch"].astype(np.int64) + prof["num_deletions"] <= tab_m[cov]) & \
        (prof["num_inserts"] <= tab_i[cov])


# ---- the partition -----------------------------------------------------------------------------------------------
def solid_flags(good, solid_len):
    n = len(good)
    solid = np.zeros(n, bool)
    s = 0
    while s < n:
        if not good[s]:
            s += 1
            continue
        e = s
        while e + 1 < n and good[e + 1]:
            e += 1
        if s <= n - solid_len - 1:
            nk = min((e - s + 1) // solid_len, (n - solid_len - 1 - s) // solid_len + 1)
            solid[s:s + nk * solid_len] = True
        s = e + 1
    return solid


def landmarks(prof, solid, p):
    n = len(solid)
    SOLID, SIMPLE = p["solid_kmer_length"], p["simple_kmer_length"]
    code = np.where(prof["has"], 256 + prof["nucl"].astype(np.int64), 0)
    lm = np.zeros(n, bool)
    for pos in range(SOLID, n - SOLID):
        if not solid[pos:pos + SIMPLE].all():
            continue
        N = code[pos + SIMPLE // 2 - SIMPLE:pos + SIMPLE // 2 + SIMPLE]
        ok = True
        for i in range(SIMPLE - SIMPLE // 2, SIMPLE + SIMPLE // 2 - 1):
            ok = ok and N[i] != N[i + 1]
        for shift in (0, 1):
            for i in range(SIMPLE - shift - 1):
                q = shift + 2 * i
                ok = ok and not (N[q] == N[q + 2] and N[q + 1] == N[q + 3])
        lm[pos] = ok
    return lm


def walk(lm, p):
    n = len(lm)
    SOLID, SIMPLE, MAXB = p["solid_kmer_length"], p["simple_kmer_length"], p["max_bubble_length"]
    where = np.flatnonzero(lm)
    partition, long_bubbles = [], 0
    pos = prev = SOLID
    end = n - SOLID
    while pos < end:
        forced_at = max(pos, prev + MAXB + 1)
        k = np.searchsorted(where, pos)
        q = int(where[k]) if k < len(where) and where[k] < min(forced_at, end) else -1
        if q < 0:
            if forced_at >= end:
                break
            q = forced_at
        if q - prev > MAXB:
            long_bubbles += 1
        prev = q + SIMPLE // 2
        partition.append(prev)
        pos = q + SOLID
    return partition, long_bubbles


def partition_of(prof, p):
    return walk(landmarks(prof, solid_flags(good_positions(prof, p), p["solid_kmer_length"]), p), p)


# ---- the bubbles -------------------------------------------------------------------------------------------------
def degap(s):
    return s.replace("-", "").encode("latin-1").translate(TO_ACGT).decode("latin-1")


def raw_bubbles(alns, prof, partition, contig):
    """-> [(position, consensus, [branches])] before post-processing"""
    if not partition:
        return []
    length, linear = contig.length, contig.type != "circular"
    ext = [0] + list(partition) + [length]
    is_part = np.zeros(length, bool)
    is_part[partition] = True
    nucl, has = prof["nucl"], prof["has"]
    out = []
    for left, right in zip(ext[:-1], ext[1:]):
        out.append((left, bytes(nucl[left:right][has[left:right]]).decode("latin-1"), []))
    for aln in alns:
        t = np.frombuffer(aln.trg_seq.encode("latin-1"), np.uint8)
        ng = t != 45
        j = np.cumsum(ng) - ng
        pos = aln.trg_start + j
        pos = np.where(pos >= length, pos - length, pos)
        cut = ng & ((pos == 0) | ((j > 0) & is_part[np.clip(pos, 0, max(length - 1, 0))]))
        cols = np.flatnonzero(cut)
        bub = bisect.bisect_right(partition, aln.trg_start)
        chrom_start = bub == 0 and linear
        chrom_end = aln.trg_end > partition[-1] and linear
        start = 0
        for k, col in enumerate(cols):
            if k > 0 or chrom_start:
                out[bub][2].append(degap(aln.qry_seq[start:col]))
            bub = bisect.bisect_right(partition, int(pos[col]))
            start = int(col)
        if chrom_end:
            out[-1][2].append(degap(aln.qry_seq[start:]))
    return out


def postprocess(raw, p):
    """-> ([(position, consensus, branches)], n_empty, n_long_branch)"""
    MAXB, MAXBR = p["max_bubble_length"], p["max_bubble_branches"]
    kept, empty, long_branch = [], 0, 0
    for position, cons, branches in raw:
        n = len(branches)
        if n == 0:
            empty += 1
            continue
        order = sorted(range(n), key=lambda i: (len(branches[i]), i))
        median = branches[order[n // 2]]
        med = len(median)
        if med == 0:
            continue
        if 2 * med > 3 * MAXB:
            new = [median]
            long_branch += 1
        else:
            new = [w for w in branches if 2 * abs(len(w) - med) < med][:MAXBR]
        if abs(med - len(cons)) > med // 2:
            cons = median
        kept.append((position, cons, new))
    return kept, empty, long_branch


def make_contig(contig, alns, p):
    prof = profile(alns, p, contig.length)
    partition, n_long = partition_of(prof, p)
    raw = raw_bubbles(alns, prof, partition, contig)
    mean_cov = sum(len(b[2]) for b in raw) // (len(raw) + 1)
    bubbles, n_empty, n_long_branch = postprocess(raw, p)
    return dict(profile=prof, partition=partition, n_long_bubbles=n_long, raw=raw, mean_cov=mean_cov, bubbles=bubbles,
                n_empty=n_empty, n_long_branch=n_long_branch)


def write_bubbles(contig_id, bubbles):
    out = []
    for position, cons, branches in bubbles:
        out.append(">%s %d %d\n%s\n" % (contig_id, position, len(branches), cons))
        for k, w in enumerate(branches):
            out.append(">%d\n%s\n" % (k, w))
    return "".join(out)


def profile_digests(prof):
    return {k: hashlib.sha256(np.ascontiguousarray(prof[k]).tobytes()).hexdigest()
            for k in ("coverage", "num_inserts", "num_deletions", "num_missmatch", "nucl")}


# ---- the generator -----------------------------------------------------------------------------------------------
def rand_seq(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def record(contig_id, length, start, trg, qry, qid, err_rate=None, secondary=False):
    assert len(trg) == len(qry), (qid, len(trg), len(qry))
    n_trg = sum(1 for ch in trg if ch != "-")
    n_qry = sum(1 for ch in qry if ch != "-")
    if err_rate is None:
        err_rate = sum(1 for a, b in zip(trg, qry) if a != b) / max(1, len(trg))
    end = start + n_trg
    if end > length:
        end -= length
    return Aln(qid, contig_id, 0, n_qry, "+", n_qry, start, end, "+", length, qry, trg, err_rate, secondary)


def gen_aln(rng, contig_id, seq, start, n_trg, sub, ins, dele, qid, secondary=False, err_rate=None):
    """columns drawn along seq from start (wrapping at its end): insertion / deletion / substitution / match"""
    L = len(seq)
    t, q = [], []
    pos, done = start, 0
    while done < n_trg:
        r = rng.random()
        if r < ins:
            t.append("-")
            q.append("ACGT"[rng.integers(0, 4)])
            continue
        b = seq[pos % L]
        pos += 1
        done += 1
        t.append(b)
        if r < ins + dele:
            q.append("-")
        elif r < ins + dele + sub:
            q.append("ACGT"[("ACGT".index(b) + 1 + rng.integers(0, 3)) % 4] if b in "ACGT" else "A")
        else:
            q.append(b)
    return record(contig_id, L, start, "".join(t), "".join(q), qid, err_rate, secondary)


def perfect(contig_id, seq, start, end, qid, err_rate=0.0):
    return record(contig_id, len(seq), start, seq[start:end], seq[start:end], qid, err_rate)


def run_a():
    rng = np.random.default_rng(101)
    contigs, alns = [], {}
    for cid, L, n in (("contig_1", 3000, 45), ("contig_2", 800, 30)):
        seq = rand_seq(rng, L)
        contigs.append((Contig(cid, L, "linear"), seq))
        lst = []
        for k in range(n):
            n_trg = int(rng.integers(min(600, L // 2), L + 1))
            start = int(rng.integers(0, L - n_trg + 1))
            rate = float(rng.uniform(0.04, 0.2))
            lst.append(gen_aln(rng, cid, seq, start, n_trg, rate * 0.4, rate * 0.35, rate * 0.25, "read_%d" % k,
                               secondary=bool(k % 7 == 3)))
        lst.sort(key=lambda a: a.trg_start)
        alns[cid] = lst
    return dict(err_mode="pacbio", overrides={}, uniform=True, contigs=contigs, alns=alns)


def run_b():
    rng = np.random.default_rng(202)
    contigs, alns = [], {}
    for cid, L, n in (("circular_1", 1500, 30), ("circular_2", 700, 12)):
        seq = rand_seq(rng, L)
        contigs.append((Contig(cid, L, "circular"), seq))
        lst = []
        for k in range(n):
            n_trg = int(rng.integers(520, L + 1))
            start = int(rng.integers(0, L))                    # many of them run past the end and wrap
            rate = float(rng.uniform(0.08, 0.22))
            lst.append(gen_aln(rng, cid, seq, start, n_trg, rate * 0.3, rate * 0.3, rate * 0.4, "read_%d" % k))
        alns[cid] = lst
    return dict(err_mode="nano", overrides={}, uniform=False, contigs=contigs, alns=alns)


def _with(seq, at, ch):
    return seq[:at] + ch + seq[at + 1:]


def run_c():
    """crafted cases; min_polish_aln_len 1 so that short alignments make a profile"""
    rng = np.random.default_rng(303)
    contigs, alns = [], {}

    def add(cid, seq, lst, kind="linear"):
        contigs.append((Contig(cid, len(seq), kind), seq))
        alns[cid] = lst

    for L in (0, 1, 19, 20, 21, 22, 25):
        seq = "ACGTCATGCTAGTCAGTACGATCAG"[:L]
        add("len_%d" % L, seq, [perfect("len_%d" % L, seq, 0, L, "r%d" % k) for k in range(3)] if L else [])
    # trg_start == 0 on a linear contig (the empty first branch), chromosome_end, and an insertion before position 0
    seq = rand_seq(rng, 120)
    lst = [perfect("ins_first", seq, 0, 120, "r%d" % k) for k in range(4)]
    lst.append(record("ins_first", 120, 0, "--" + seq, "GT" + seq, "r_ins"))
    lst.append(perfect("ins_first", seq, 30, 120, "r_inner"))
    add("ins_first", seq, lst)
    # a stretch nobody covers
    seq = rand_seq(rng, 200)
    add("uncovered", seq, [perfect("uncovered", seq, 0, 80, "l%d" % k) for k in range(4)] +
        [perfect("uncovered", seq, 110, 200, "r%d" % k) for k in range(4)])
    # no landmark: forced cuts
    for cid, seq in (("homopolymer", "A" * 700), ("dinucleotide", "AC" * 350)):
        add(cid, seq, [perfect(cid, seq, 0, 700, "r%d" % k) for k in range(3)])
    # unprofiled alignments (err_rate above the limit) still give branches: a deleted stretch makes the median empty,
    # an inserted one makes the median three times the consensus
    seq = rand_seq(rng, 160)
    gone = seq[:30] + "-" * 70 + seq[100:]
    add("median_empty", seq, [perfect("median_empty", seq, 0, 160, "r%d" % k) for k in range(2)] +
        [record("median_empty", 160, 0, seq, gone, "d%d" % k, err_rate=0.9) for k in range(3)])
    seq = rand_seq(rng, 160)
    extra = rand_seq(rng, 60)
    add("cons_replaced", seq, [perfect("cons_replaced", seq, 0, 160, "r%d" % k) for k in range(2)] +
        [record("cons_replaced", 160, 0, seq[:80] + "-" * 60 + seq[80:], seq[:80] + extra + seq[80:], "i%d" % k, err_rate=0.9)
         for k in range(3)])
    # err_rate exactly at the limit (in) and just above (out)
    seq = rand_seq(rng, 100)
    add("err_limit", seq, [perfect("err_limit", seq, 0, 100, "at0", err_rate=0.25), perfect("err_limit", seq, 0, 100, "at1", err_rate=0.25),
                           record("err_limit", 100, 0, seq, _with(seq, 50, "-"), "above", err_rate=float(np.nextafter(0.25, 1.0)))])
    # (mismatches + deletions) / coverage exactly 1/5 (good under 0.2) and 2/5 (bad)
    seq = rand_seq(rng, 100)
    other = lambda at: "ACGT"[("ACGT".index(seq[at]) + 1) % 4]
    add("one_fifth", seq, [record("one_fifth", 100, 0, seq, _with(seq, 50, other(50)), "m0", err_rate=0.01),
                           record("one_fifth", 100, 0, seq, _with(_with(seq, 60, other(60)), 70, "-"), "m1", err_rate=0.01),
                           record("one_fifth", 100, 0, seq, _with(seq, 60, "-"), "m2", err_rate=0.01)] +
        [perfect("one_fifth", seq, 0, 100, "r%d" % k) for k in range(2)])
    # two alignments that disagree on a target byte (the last in list order names the base); a gap in both strings
    seq = rand_seq(rng, 100)
    alt = _with(seq, 40, "ACGT"[("ACGT".index(seq[40]) + 2) % 4])
    add("disagree", seq, [perfect("disagree", seq, 0, 100, "r0"),
                          record("disagree", 100, 0, seq[:70] + "-" + seq[70:], seq[:70] + "-" + seq[70:], "r_both"),
                          record("disagree", 100, 0, alt, alt, "r_alt")])
    # shift_gaps: runs at both ends, adjacent runs, a later run walking over bytes an earlier run moved
    seq = "GATTACA" + "A" * 12 + "CGCGCG" + "T" * 10 + "GACTGACTGA" + "C" * 8 + "AGTCAGTC"
    L = len(seq)
    lst = [perfect("shifts", seq, 0, L, "r%d" % k) for k in range(3)]
    lst.append(record("shifts", L, 0, seq, "--" + seq[2:9] + "--" + seq[11:14] + "-" + seq[15:19] + "---" + seq[22:L - 3] + "---", "ends"))
    lst.append(record("shifts", L, 0, seq, seq[:8] + "-" + seq[9] + "-" + seq[11:27] + "--" + seq[29] + "-" + seq[31:], "adjacent"))
    lst.append(record("shifts", L, 0, seq[:10] + "-" + seq[10:16] + "--" + seq[16:], seq[:10] + "A" + seq[10:13] + "-" + seq[14:16] + "AA" +
                      seq[16:30] + "-" + seq[31:], "mixed"))
    for k in range(6):
        lst.append(gen_aln(rng, "shifts", seq, 0, L, 0.02, 0.15, 0.2, "g%d" % k, err_rate=0.1))
    add("shifts", seq, lst)
    # column counts around the wave width and the scan tile
    seq = rand_seq(rng, 1100)
    lst = [perfect("columns", seq, 0, 1100, "r%d" % k) for k in range(3)]
    for n in (1, 63, 64, 65, 255, 256, 257, 1025):
        a = gen_aln(rng, "columns", seq, int(rng.integers(0, 1100 - n)), n, 0.03, 0.0, 0.03, "n%d" % n, err_rate=0.05)
        assert len(a.trg_seq) == n
        lst.append(a)
    add("columns", seq, lst)
    # query bytes outside ACGT and in lower case
    seq = rand_seq(rng, 120)
    odd = "".join(("NRYKMSWBVDHXUnacgtryk"[(i // 3) % 21] if i % 3 == 0 else ch) for i, ch in enumerate(seq))
    add("letters", seq, [perfect("letters", seq, 0, 120, "r%d" % k) for k in range(3)] +
        [record("letters", 120, 0, seq, odd, "odd", err_rate=0.9)])
    # more than 64 branches in a bubble (and more than the cap of 50); gap runs whose walk is longer than 64 columns: one
    # that moves 80 bases at once, one that stops at the first mismatch after 70
    seq = "C" * 30 + "A" * 170 + rand_seq(rng, 60)
    lst = [perfect("wide", seq, 0, 260, "r%d" % k) for k in range(66)]
    lst.append(record("wide", 260, 0, seq, seq[:120] + "-" * 80 + seq[200:], "moves_80", err_rate=0.1))
    lst.append(record("wide", 260, 0, seq, seq[:100] + "-" * 100 + seq[200:], "stops_at_70", err_rate=0.1))
    lst += [gen_aln(rng, "wide", seq, 0, 260, 0.03, 0.03, 0.03, "g%d" % k, err_rate=0.1) for k in range(3)]
    add("wide", seq, lst)
    return dict(err_mode="pacbio", overrides=dict(min_polish_aln_len=1), uniform=False, contigs=contigs, alns=alns)


def run_d():
    rng = np.random.default_rng(404)
    contigs, alns = [], {}
    seq = rand_seq(rng, 1500)
    contigs.append((Contig("small_1", 1500, "linear"), seq))
    lst = []
    for k in range(30):
        n_trg = int(rng.integers(20, 1200))                   # some are shorter than min_polish_aln_len
        start = int(rng.integers(0, 1500 - n_trg + 1))
        rate = float(rng.uniform(0.05, 0.2))
        lst.append(gen_aln(rng, "small_1", seq, start, n_trg, rate * 0.4, rate * 0.3, rate * 0.3, "read_%d" % k))
    alns["small_1"] = lst
    seq = "A" * 300
    contigs.append((Contig("forced", 300, "linear"), seq))
    alns["forced"] = [perfect("forced", seq, 0, 300, "r%d" % k) for k in range(8)]
    seq = rand_seq(rng, 300)
    extra = rand_seq(rng, 120)
    contigs.append((Contig("long_branch", 300, "linear"), seq))
    alns["long_branch"] = [perfect("long_branch", seq, 0, 300, "r%d" % k) for k in range(2)] + \
        [record("long_branch", 300, 0, seq[:150] + "-" * 120 + seq[150:], seq[:150] + extra + seq[150:], "i%d" % k, err_rate=0.9)
         for k in range(3)]
    seq = rand_seq(rng, 200)
    contigs.append((Contig("short_alns", 200, "linear"), seq))
    alns["short_alns"] = [perfect("short_alns", seq, 0, 200, "r%d" % k) for k in range(2)] + \
        [perfect("short_alns", seq, 10 + 30 * k, 50 + 30 * k, "s%d" % k) for k in range(5)]
    return dict(err_mode="pacbio", overrides=dict(max_bubble_length=60, max_bubble_branches=5, min_polish_aln_len=50,
                                                  solid_kmer_length=6, simple_kmer_length=2),
                uniform=False, contigs=contigs, alns=alns)


RUNS = dict(bubbles_a=run_a, bubbles_b=run_b, bubbles_c=run_c, bubbles_d=run_d)


def fuzz(seed):
    rng = np.random.default_rng(9000 + seed)
    contigs, alns = [], {}
    for c in range(int(rng.integers(2, 5))):
        L = int(rng.integers(100, 1501))
        kind = "circular" if rng.random() < 0.5 else "linear"
        seq = rand_seq(rng, L) if rng.random() < 0.8 else ("ACGGT" * L)[:L]
        cid = "fz%d_%d" % (seed, c)
        contigs.append((Contig(cid, L, kind), seq))
        lst = []
        for k in range(int(rng.integers(0, 41))):
            n_trg = int(rng.integers(1, L + 1))
            start = int(rng.integers(0, L)) if kind == "circular" else int(rng.integers(0, L - n_trg + 1))
            rate = float(rng.uniform(0.05, 0.3))
            lst.append(gen_aln(rng, cid, seq, start, n_trg, rate * 0.4, rate * 0.3, rate * 0.3, "q%d" % k))
        alns[cid] = lst
    overrides = dict(min_polish_aln_len=int(rng.choice([1, 50, 200])), max_bubble_length=int(rng.choice([40, 500])),
                     max_bubble_branches=int(rng.choice([4, 50])))
    if seed % 2:
        overrides.update(solid_kmer_length=6, simple_kmer_length=2)
    return dict(err_mode="nano" if seed % 2 else "pacbio", overrides=overrides, uniform=False, contigs=contigs, alns=alns)


def input_digest(run):
    h = hashlib.sha256()
    for contig, seq in run["contigs"]:
        h.update(json.dumps([list(contig), seq, [list(a) for a in run["alns"][contig.id]]]).encode())
    return h.hexdigest()


def read_gz(name):
    with gzip.open(os.path.join(GOLDEN, name), "rb") as f:
        return f.read().decode("latin-1")
