"""A second writing of the reference's consensus stage (flye/polishing/consensus.py: _contig_profile, _flatten_profile) and
of the coverage cap in front of it (flye/polishing/alignment.py: get_uniform_alignments) in the forms the device uses, and
the inputs of tests/test_contig_consensus.py.  Nothing here is copied from the reference:
tests/golden/make_contig_consensus_golden.py runs the reference's own functions on these inputs and stores what they give.

Forms that differ from the reference's loops, each pinned by the golden runs:
* the windows' lists are (window, err_rate bits) pairs in one sort: a non-negative double orders as its bit pattern;
* cov_threshold = max(5 * m2 // 8, 10) with m2 twice the median of the primary coverages.  int(1.25 * median) is exact in
  double: median = m2 / 2, and 5 * m2 / 8 has at most three fractional bits below 2^35, so nothing is rounded;
* the insertions are records (position, read, alignment, column, byte) in one sort; the bytes of one (position, read)
  stand together as the read's string, whichever of its alignments they came from;
* nucl is the byte of the largest (alignment, column) that set it; matches is a dense table position x byte.

Inputs: the four runs of bubbles_restate (every contig goes through the uniform step first, as get_consensus does), its
fuzz seeds with some reads given two alignments, and the crafted run consensus_e."""
import collections
import hashlib
import struct

import numpy as np

import bubbles_restate as R

WINDOW, MIN_COV = 100, 10


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", 0.0 if x == 0.0 else x))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


# ---- get_uniform_alignments ------------------------------------------------------------------------------------------
def uniform(alns, length):
    """-> dict(keep=[0 / 1 per alignment], cov_threshold, thresholds=[double per window])"""
    n_w = length // WINDOW + 1
    diff_all, diff_prim = [0] * (n_w + 1), [0] * (n_w + 1)
    pairs = []
    for a in alns:
        first, last = a.trg_start // WINDOW, a.trg_end // WINDOW
        if a.trg_start < 0 or a.trg_end < 0 or max(first, last) > length // WINDOW:
            raise ValueError("uniform: an alignment outside the windows of its contig")
        if not a.err_rate >= 0.0:
            raise ValueError("uniform: err_rate NaN or negative")
        if last > first:
            diff_all[first] += 1
            diff_all[last] -= 1
            if not a.is_secondary:
                diff_prim[first] += 1
                diff_prim[last] -= 1
            pairs += [(w, bits(a.err_rate)) for w in range(first, last)]
    count, prim = list(np.cumsum(diff_all)[:n_w]), sorted(int(x) for x in np.cumsum(diff_prim)[:n_w])
    m2 = 2 * prim[n_w // 2] if n_w % 2 else prim[n_w // 2 - 1] + prim[n_w // 2]
    cov_threshold = max(5 * m2 // 8, MIN_COV)
    pairs.sort()
    start = [0] + [int(x) for x in np.cumsum(count)]
    thr = [pairs[start[w] + cov_threshold][1] if count[w] > cov_threshold else bits(1.0) for w in range(n_w)]
    keep = []
    for a in alns:
        first, last = a.trg_start // WINDOW, a.trg_end // WINDOW
        good = sum(1 for w in range(first, last) if bits(a.err_rate) <= thr[w])
        keep.append(int(good > (last - first) // 2))
    return dict(keep=keep, cov_threshold=cov_threshold, thresholds=[from_bits(t) for t in thr], counts=[int(x) for x in count])


# ---- _contig_profile and _flatten_profile ----------------------------------------------------------------------------
def number_reads(alns):
    """qry_id strings -> numbers in the order they first appear"""
    number = {}
    return [number.setdefault(a.qry_id, len(number)) for a in alns]


def consensus(alns, qry_id, use, length):
    """alns in list order, qry_id a number per alignment, use a flag per alignment (None: all) -> dict(seq (bytes), nucl,
    match_total, num_ins, max_match, accepted (arrays per position), ins ([bytes per position]: the chosen string))"""
    matches = np.zeros((length, 128), np.int64)
    tag = [0] * length
    records = []
    for k, aln in enumerate(alns):
        if use is not None and not use[k]:
            continue
        if length == 0:
            raise ValueError("consensus: an alignment in use on a contig of length 0")
        qry = R.shift_gaps(aln.trg_seq, aln.qry_seq)
        trg = R.shift_gaps(qry, aln.trg_seq)
        t = np.frombuffer(trg.encode("latin-1"), np.uint8)
        q = np.frombuffer(qry.encode("latin-1"), np.uint8)
        ng = t != 45
        before = np.cumsum(ng) - ng
        pos = np.where(ng, aln.trg_start + before, aln.trg_start + before - 1)
        pos = np.where(pos >= length, pos - length, pos)
        pos = np.where(pos < 0, length - 1, pos)
        ins = ~ng & (q != 45)
        for col in np.flatnonzero(ins):
            records.append((int(pos[col]), qry_id[k], k, int(col), int(q[col])))
        rest = np.flatnonzero(~ins)
        np.add.at(matches, (pos[rest], q[rest]), 1)
        for col in rest:
            p = int(pos[col])
            tag[p] = max(tag[p], ((k + 1) << 40) | (int(col) << 8) | int(t[col]))
    records.sort()
    strings = collections.defaultdict(lambda: collections.defaultdict(bytearray))         # position -> read -> bytes
    for p, read, _, _, byte in records:
        strings[p][read].append(byte)
    nucl = np.array([(v & 255) if v else 45 for v in tag], np.uint8)
    total = matches.sum(axis=1).astype(np.int32)
    best = matches.argmax(axis=1)                      # the first of the largest: the smallest byte
    max_match = np.where(total > 0, best, nucl).astype(np.uint8)
    num_ins = np.zeros(length, np.int32)
    accepted = np.zeros(length, np.uint8)
    chosen = [b""] * length
    for p, by_read in strings.items():
        counts = collections.Counter(bytes(s) for s in by_read.values())
        chosen[p] = min(counts, key=lambda s: (-counts[s], s))
        num_ins[p] = len(by_read)
        accepted[p] = int(num_ins[p] > total[p] // 2)
    seq = bytearray()
    for p in range(length):
        if max_match[p] != 45:
            seq.append(int(max_match[p]))
        if accepted[p]:
            seq += chosen[p]
    return dict(seq=bytes(seq), nucl=nucl, match_total=total, num_ins=num_ins, max_match=max_match, accepted=accepted, ins=chosen)


PROFILE_KEYS = ("nucl", "match_total", "num_ins", "max_match", "accepted")


def profile_digests(res):
    d = {k: hashlib.sha256(np.ascontiguousarray(res[k]).tobytes()).hexdigest() for k in PROFILE_KEYS}
    d["ins"] = hashlib.sha256(b"\n".join(res["ins"])).hexdigest()
    return d


def write_fasta(seqs):
    """{id: sequence} as the reference's writer lays it out: sorted headers, lines of 60"""
    out = []
    for header in sorted(seqs):
        out.append(">%s\n" % header)
        out += [seqs[header][i:i + 60] + "\n" for i in range(0, len(seqs[header]), 60)]
    return "".join(out)


# ---- the crafted run -------------------------------------------------------------------------------------------------
def _set(seq, at, ch):
    return seq[:at] + ch + seq[at + 1:]


def edited(cid, seq, start, end, qid, ins=None, sub=None, dele=(), lead="", err_rate=0.1, secondary=False):
    """seq[start:end] with strings inserted behind positions (ins: {position: string}), bases replaced (sub: {position:
    base}) or deleted (dele), and `lead` inserted before the first column"""
    ins, sub = ins or {}, sub or {}
    t, q = ["-" * len(lead)], [lead]
    for p in range(start, end):
        t.append(seq[p])
        q.append("-" if p in dele else sub.get(p, seq[p]))
        if p in ins:
            t.append("-" * len(ins[p]))
            q.append(ins[p])
    return R.record(cid, len(seq), start, "".join(t), "".join(q), qid, err_rate, secondary)


LONG = {50: 63, 100: 64, 150: 65, 200: 257, 250: 1}         # position -> length of the string inserted behind it


def run_e():
    rng = np.random.default_rng(505)
    contigs, alns = [], {}

    def add(cid, seq, lst, kind="linear"):
        assert len(seq) < 3000 and len(lst) <= 100
        contigs.append((R.Contig(cid, len(seq), kind), seq))
        alns[cid] = lst

    # "votes": eight alignments over the whole contig (match_total 8 everywhere, so an insertion needs five reads), one of
    # them a second alignment of the read "dup", and one inside a single window, which the uniform step drops
    seq = R.rand_seq(rng, 300)
    for at, ch in ((20, "A"), (40, "A"), (60, "G"), (80, "A"), (100, "A"), (119, "C"), (120, "A"), (140, "G"), (299, "A")):
        seq = _set(seq, at, ch)
    plan = [  # qry_id, insertions, substitutions, deletions, lead
        ("dup", {20: "C", 40: "G", 60: "A", 80: "C", 100: "C"}, {140: "C"}, (120,), ""),
        ("dup", {20: "G"}, {140: "C"}, (120,), ""),
        ("other", {20: "CG", 40: "G", 60: "A", 80: "C", 100: "C"}, {140: "C"}, (120,), ""),
        ("r3", {20: "CG", 40: "C", 60: "AC", 80: "C", 100: "C"}, {140: "C"}, (120,), "GT"),
        ("r4", {20: "G", 40: "C", 60: "AC", 80: "G", 100: "G"}, {}, (), "GT"),
        ("r5", {20: "G", 40: "T", 60: "T", 100: "G"}, {}, (), "GT"),
        ("r6", {}, {}, (), "GT"),
        ("r7", {}, {}, (), "GT"),
    ]
    lst = [edited("votes", seq, 0, 300, qid, ins, sub, dele, lead) for qid, ins, sub, dele, lead in plan]
    lst.append(edited("votes", seq, 110, 190, "inside", {}, {}, (), "", err_rate=0.01))        # 'G' at 140 would break the tie
    add("votes", seq, lst)
    # a stretch nobody covers
    seq = R.rand_seq(rng, 400)
    add("hole", seq, [R.perfect("hole", seq, 0, 200, "l%d" % k, err_rate=0.05) for k in range(3)] +
        [R.perfect("hole", seq, 250, 400, "r%d" % k, err_rate=0.05) for k in range(3)])
    # a circular contig: alignments that start at 250 and wrap, with an insertion behind the last position and one behind
    # position 0 (its column count has passed the contig's length); one alignment that starts at 0 with an insertion
    # before its first column
    seq = _set(_set(R.rand_seq(rng, 300), 299, "A"), 0, "A")
    lst = []
    for k in range(3):
        a = edited("circ", seq + seq, 250, 480, "w%d" % k, {299: "CT", 300: "GC"})
        lst.append(a._replace(trg_end=180, trg_len=300))
    lst.append(edited("circ", seq, 0, 250, "z0", {}, {}, (), "TC"))
    add("circ", seq, lst, "circular")
    # strings of 1, 63, 64, 65 and 257 bytes: two reads agree, the third differs in its last byte
    seq = R.rand_seq(rng, 300)
    for at in LONG:
        seq = _set(seq, at, "A")
    body = {at: "".join("CGT"[i] for i in rng.integers(0, 3, n)) for at, n in LONG.items()}
    other = {at: s[:-1] + ("C" if s[-1] != "C" else "G") for at, s in body.items()}
    add("long", seq, [edited("long", seq, 0, 300, "a", body), edited("long", seq, 0, 300, "b", other),
                      edited("long", seq, 0, 300, "c", body)])
    # 70 reads insert at one position, 5 do not
    seq = _set(R.rand_seq(rng, 250), 100, "A")
    add("deep", seq, [edited("deep", seq, 0, 250, "d%d" % k, {100: "C" if k < 30 else ("G" if k < 55 else "CT")} if k < 70 else {})
                      for k in range(75)])
    # the uniform step.  uni_odd: 11 windows; eight primaries over windows 0 .. 9 make the median 8 and cov_threshold 10
    seq = R.rand_seq(rng, 1050)
    lst = [R.perfect("uni_odd", seq, 0, 1000, "p%d" % k, err_rate=0.10 + 0.01 * k) for k in range(8)]
    lst += [R.perfect("uni_odd", seq, 200, 400, "s2_%d" % k, err_rate=0.2)._replace(is_secondary=True) for k in range(2)]   # 10 entries
    lst += [R.perfect("uni_odd", seq, 500, 700, "s5_%d" % k, err_rate=0.05 + 0.2 * k)._replace(is_secondary=True) for k in range(3)]  # 11
    lst += [R.perfect("uni_odd", seq, 700, 900, "s7_%d" % k, err_rate=0.01 + 0.01 * k)._replace(is_secondary=True) for k in range(5)]
    lst.append(R.perfect("uni_odd", seq, 700, 900, "bad", err_rate=0.3))             # fails in both of its windows
    lst.append(R.perfect("uni_odd", seq, 710, 790, "one_window", err_rate=0.0))
    add("uni_odd", seq, lst)
    # uni_even: 10 windows, the two middle coverages are 10 and 11: m2 = 21 gives 13 where a median of 10 would give 12
    seq = R.rand_seq(rng, 950)
    lst = [R.perfect("uni_even", seq, 0, 900, "p%d" % k, err_rate=0.10 + 0.01 * k) for k in range(10)]
    lst.append(R.perfect("uni_even", seq, 400, 900, "p_half", err_rate=0.09))
    lst += [R.perfect("uni_even", seq, 0, 200, "s0_%d" % k, err_rate=0.3)._replace(is_secondary=True) for k in range(3)]     # 13 entries
    lst += [R.perfect("uni_even", seq, 200, 400, "s2_%d" % k, err_rate=0.02 * (k + 1))._replace(is_secondary=True) for k in range(4)]  # 14
    add("uni_even", seq, lst)
    # trg_end == len with len % 100 == 0: the last window index is len // 100 and stays empty
    seq = R.rand_seq(rng, 1000)
    add("uni_1000", seq, [R.perfect("uni_1000", seq, 0, 1000, "p%d" % k, err_rate=0.1) for k in range(6)])
    return dict(err_mode="pacbio", overrides={}, uniform=True, contigs=contigs, alns=alns)


RUNS = dict(R.RUNS, consensus_e=run_e)


def fuzz(seed):
    """bubbles_restate's fuzz input; every third alignment becomes a second alignment of the read before it"""
    run = R.fuzz(seed)
    for cid, lst in run["alns"].items():
        run["alns"][cid] = [a._replace(qry_id=lst[k - 1].qry_id) if k % 3 == 2 else a for k, a in enumerate(lst)]
    return run


def restate_run(run, with_uniform=True):
    """per contig: dict(uniform=..., use=[flags], consensus=...)"""
    out = {}
    for contig, _ in run["contigs"]:
        lst = run["alns"][contig.id]
        uni = uniform(lst, contig.length) if with_uniform else None
        use = uni["keep"] if uni else None
        out[contig.id] = dict(uniform=uni, use=use, consensus=consensus(lst, number_reads(lst), use, contig.length))
    return out


def input_digest(run):
    return R.input_digest(run)
