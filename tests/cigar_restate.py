"""A second writing of the reference's SAM reader (flye/utils/sam_parser.py: SynchronizedSamReader.get_chunk and
_parse_cigar) in plain Python, and the inputs of tests/test_expand_cigars.py: seeded generators of SAM text plus contigs.
Nothing here is copied from the reference: tests/golden/make_cigar_golden.py runs the reference's own class on these
inputs and stores what it gives.

Forms that differ from the reference's loops, each pinned by the golden runs:
* the file is cut into chunks in one pass, not by a reader process;
* a run is a pair (operation byte, length); the gapped strings are filled column by column from the two positions, not
  joined from slices;
* the clips follow from the runs alone: the left hard clip is the first run if it is H, the left soft clip the first run
  that is not H if it is S, every other H / S lies on the right.

A run of the generators is dict(sam=bytes, contigs={id: str}, max_coverage=int, use_secondary=bool)."""
import collections
import hashlib
import random
import re

import numpy as np

Alignment = collections.namedtuple("Alignment", ["qry_id", "trg_id", "qry_start", "qry_end", "qry_sign", "qry_len", "trg_start",
                                                 "trg_end", "trg_sign", "trg_len", "qry_seq", "trg_seq", "err_rate", "is_secondary"])
HEADERS = (b"@PG", b"@HD", b"@SQ", b"@RG", b"@CO")
TOKEN = re.compile(b"[0-9]+[MIDNSHP=X]")


class Unsupported(Exception):
    pass


# ---- _parse_cigar ----------------------------------------------------------------------------------------------------
def tokens_of(cigar):
    return [(t[-1], int(t[:-1])) for t in TOKEN.findall(cigar)]


def clips(runs):
    """(left hard, right hard, left soft, right soft)"""
    hard = [n for op, n in runs if op == ord("H")]
    soft = [n for op, n in runs if op == ord("S")]
    hard_left = runs[0][1] if runs and runs[0][0] == ord("H") else 0
    rest = [(op, n) for op, n in runs if op != ord("H")]
    soft_left = rest[0][1] if rest and rest[0][0] == ord("S") else 0
    return hard_left, sum(hard) - hard_left, soft_left, sum(soft) - soft_left


def parse_cigar(runs, read, contig, ctg_pos):
    """-> dict(trg_start, trg_end, qry_start, qry_end, qry_len, trg (bytes), qry (bytes), matches, err_rate); read and contig
    are bytes.  Raises Unsupported for N P = X, ValueError where a slice of the reference would come out short or the
    alignment has no columns (the reference divides by zero)."""
    trg, qry = bytearray(), bytearray()
    t, q = ctg_pos - 1, 0
    for op, n in runs:
        ch = chr(op)
        if ch in "NP=X":
            raise Unsupported(ch)
        if ch not in "MIDSH":
            raise ValueError("operation %r" % ch)
        if ch == "S":
            q += n
        if ch in "MID":
            for _ in range(n):
                if ch != "I" and t >= len(contig) or ch != "D" and q >= len(read):
                    raise ValueError("the runs leave the read or the contig")
                trg.append(45 if ch == "I" else contig[t])
                qry.append(45 if ch == "D" else read[q])
                t += ch != "I"
                q += ch != "D"
    if q > len(read):
        raise ValueError("the runs leave the read")
    if not trg:
        raise ValueError("no columns")
    trg, qry = bytes(trg).upper(), bytes(qry).upper()
    matches = sum(1 for a, b in zip(trg, qry) if a == b)
    hard_left, hard_right, soft_left, soft_right = clips(runs)
    return dict(trg_start=ctg_pos - 1, trg_end=t, qry_start=hard_left + soft_left, qry_end=q + hard_left - soft_right,
                qry_len=q + hard_left + hard_right, trg=trg, qry=qry, matches=matches, err_rate=1 - matches / len(trg))


# ---- get_chunk -------------------------------------------------------------------------------------------------------
def file_chunks(sam):
    """[(contig bytes, [line])] in file order; ValueError when a contig comes back"""
    out, seen = [], set()
    for line in sam.splitlines(keepends=True):
        if line[:3] in HEADERS:
            continue
        fields = line.split(b"\t", 3)
        if len(fields) < 4:
            continue
        contig = fields[2]
        if out and out[-1][0] == contig:
            out[-1][1].append(line)
            continue
        if contig in seen:
            raise ValueError("Alignment file is not sorted")
        seen.add(contig)
        out.append((contig, [line]))
    return out


def records(run):
    """per chunk (contig id, [record], cut): the records get_chunk parses, in the order it parses them (after the shuffle,
    before the sort); a record is dict(qry_id, contig, flags, pos, runs, seq); cut says the coverage cut ended the chunk"""
    contigs = {k.encode(): v.encode() for k, v in run["contigs"].items()}
    out = []
    for contig, lines in file_chunks(run["sam"]):
        lines = list(lines)
        random.Random(42).shuffle(lines)
        total, recs, cut = 0, [], False
        for line in lines:
            tok = line.strip().split()
            if len(tok) < 11:
                continue
            flags = int(tok[1])
            if flags & 4 or (flags & 256 and not run["use_secondary"]):
                continue
            if tok[9] == b"*":
                raise Exception("record without read sequence")
            runs = tokens_of(tok[5])
            recs.append(dict(qry_id=tok[0].decode(), contig=tok[2], flags=flags, pos=int(tok[3]), runs=runs, seq=tok[9]))
            hard_left, _, soft_left, soft_right = clips(runs)
            q = sum(n for op, n in runs if chr(op) in "MIS")
            total += (q + hard_left - soft_right) - (hard_left + soft_left)
            if run["max_coverage"] is not None and total // len(contigs[contig]) > run["max_coverage"]:
                cut = True
                break
        out.append((contig.decode(), recs, cut))
    return out


def alignment_of(rec, contigs):
    ctg = contigs[rec["contig"].decode()].encode()
    p = parse_cigar(rec["runs"], rec["seq"], ctg, rec["pos"])
    return Alignment(rec["qry_id"], rec["contig"].decode(), p["qry_start"], p["qry_end"], "-" if rec["flags"] & 0x16 else "+",
                     p["qry_len"], p["trg_start"], p["trg_end"], "+", len(ctg), p["qry"].decode(), p["trg"].decode(), p["err_rate"],
                     rec["flags"] & 0x100)


def chunks(run):
    """[(contig id, [Alignment])]: what successive get_chunk calls return"""
    out = []
    for contig, recs, _ in records(run):
        alns = [alignment_of(r, run["contigs"]) for r in recs]
        alns.sort(key=lambda a: (a.qry_id, -(a.qry_end - a.qry_start)))
        out.append((contig, alns))
    return out


def call_arrays(recs, contigs):
    """the arguments of Context.expand_cigars for a list of records: every contig of the run goes up, in sorted order"""
    names = sorted(contigs)
    return dict(contig_off=np.cumsum([0] + [len(contigs[k]) for k in names]).astype(np.uint64),
                contig_seq=np.frombuffer("".join(contigs[k] for k in names).encode(), np.uint8),
                aln_contig=np.array([names.index(r["contig"].decode()) for r in recs], np.uint32),
                ctg_pos=np.array([r["pos"] for r in recs], np.int32),
                run_off=np.cumsum([0] + [len(r["runs"]) for r in recs]).astype(np.uint64),
                run_op=np.array([op for r in recs for op, _ in r["runs"]], np.uint8),
                run_len=np.array([n for r in recs for _, n in r["runs"]], np.uint32),
                read_off=np.cumsum([0] + [len(r["seq"]) for r in recs]).astype(np.uint64),
                read_seq=np.frombuffer(b"".join(r["seq"] for r in recs), np.uint8))


def expand(recs, contigs):
    """what fg_expand_cigars returns for these records, arrays under the names of the header"""
    ps = [parse_cigar(r["runs"], r["seq"], contigs[r["contig"].decode()].encode(), r["pos"]) for r in recs]
    out = dict(col_off=np.cumsum([0] + [len(p["trg"]) for p in ps]).astype(np.uint64),
               trg_cols=np.frombuffer(b"".join(p["trg"] for p in ps), np.uint8),
               qry_cols=np.frombuffer(b"".join(p["qry"] for p in ps), np.uint8),
               matches=np.array([p["matches"] for p in ps], np.int64), err_rate=np.array([p["err_rate"] for p in ps], np.float64))
    for k in ("trg_start", "trg_end", "qry_start", "qry_end", "qry_len"):
        out[k] = np.array([p[k] for p in ps], np.int32)
    return out


def input_digest(run):
    h = hashlib.sha256(run["sam"])
    for k in sorted(run["contigs"]):
        h.update(("%s %s\n" % (k, run["contigs"][k])).encode())
    h.update(("%r %r" % (run["max_coverage"], run["use_secondary"])).encode())
    return h.hexdigest()


# ---- the generators --------------------------------------------------------------------------------------------------
def rand_contig(rng, n, lower=0.1, n_rate=0.01):
    """ACGT with some N and lower-case stretches"""
    seq = ["ACGT"[i] for i in rng.integers(0, 4, n)]
    for i in range(n):
        if rng.random() < n_rate:
            seq[i] = "N"
    i = 0
    while i < n:
        if rng.random() < lower / 8:
            for j in range(i, min(n, i + 8)):
                seq[j] = seq[j].lower()
            i += 8
        i += 1
    return "".join(seq)


def noisy_read(rng, contig, start, runs, sub=0.04):
    """the SEQ bytes that the runs (with their clips) consume along contig from start; some bases differ, some are
    lower-case"""
    out, t = [], start
    for op, n in runs:
        if op in "SI":
            out += ["ACGTacgtN"[rng.integers(0, 9)] for _ in range(n)]
        elif op == "M":
            for b in contig[t:t + n]:
                r = rng.random()
                out.append("ACGT"[rng.integers(0, 4)] if r < sub else b.lower() if r < sub + 0.05 else b)
            t += n
        elif op == "D":
            t += n
    return "".join(out)


def noisy_runs(rng, n_trg, max_run=20):
    """M / I / D runs of 1 .. max_run that consume n_trg contig bases; M between the others more often than not"""
    runs, left, last = [], n_trg, None
    while left > 0:
        op = "M" if last != "M" and rng.random() < 0.7 else "MID"[rng.integers(0, 3)]
        n = int(rng.integers(1, max_run + 1))
        if op != "I":
            n = min(n, left)
            left -= n
        runs.append((op, n))
        last = op
    return runs


def cigar_of(runs):
    return "".join("%d%s" % (n, op) for op, n in runs)


def sam_line(qid, flag, contig, pos, cigar, seq, extra=()):
    return "\t".join([qid, str(flag), contig, str(pos), "60", cigar, "*", "0", "0", seq, "*"] + list(extra)) + "\n"


def sam_a(use_secondary=True):
    rng = np.random.default_rng(4242)
    sizes = (("ctg_1", 1500, 48, 260), ("ctg_2", 700, 30, 160), ("ctg_3", 300, 42, 140))
    contigs = {cid: rand_contig(rng, n) for cid, n, _, _ in sizes}
    flags = [0, 16, 0, 16, 256, 272, 2048, 4, 0, 16, 0, 2064]
    text = ["@HD\tVN:1.6\tSO:coordinate\n"] + ["@SQ\tSN:%s\tLN:%d\n" % (cid, n) for cid, n, _, _ in sizes]
    text += ["@PG\tID:aligner\n", "@CO\ta comment\n"]
    k = 0
    for cid, n, count, span in sizes:
        for j in range(count):
            flag = flags[k % len(flags)]
            n_trg = int(rng.integers(span // 2, span + 1))
            start = int(rng.integers(0, n - n_trg + 1))
            runs = noisy_runs(rng, n_trg)
            clip = k % 5
            left = [("H", int(rng.integers(1, 30)))] if clip in (1, 3) else []
            left += [("S", int(rng.integers(1, 12)))] if clip in (2, 3) else []
            right = [("S", int(rng.integers(1, 12)))] if clip in (2, 4) else []
            right += [("H", int(rng.integers(1, 30)))] if clip in (1, 4) else []
            runs = left + runs + right
            seq = noisy_read(rng, contigs[cid], start, runs)
            qid = "read_%d" % k
            if flag == 4:
                text.append(sam_line(qid, 4, cid, 0, "*", seq))
            else:
                text.append(sam_line(qid, flag, cid, start + 1, cigar_of(runs), seq, ["NM:i:%d" % j]))
            k += 1
        if cid == "ctg_1":
            # two records of one qry_id with equal spans: the stable sort keeps the shuffled order
            for start in (100, 700):
                runs = [("M", 50), ("I", 2), ("M", 48)]
                text.append(sam_line("read_twice", 0, cid, start + 1, cigar_of(runs), noisy_read(rng, contigs[cid], start, runs)))
            text.append("short\t0\t%s\t5\t60\t10M\t*\t0\n" % cid)            # 8 tokens: skipped
    return dict(sam="".join(text).encode(), contigs=contigs, max_coverage=7, use_secondary=use_secondary)


def sam_a_primary():
    return sam_a(use_secondary=False)


EDGE_CIGARS = ["1M", "63M", "64M", "65M", "128M", "129M", "64M", "10M65I10M", "10M1000D10M", "1M1I1M1D" * 75, "5M2H3M", "3M2S3M",
               "4M0M4M", "7M0I0D7M", "30I", "40D", "2H3S20M1I20M4S5H"]


def runs_of(cigar):
    return [(chr(op), n) for op, n in tokens_of(cigar.encode())]


def sam_edges():
    """crafted for a tile of 64 columns"""
    rng = np.random.default_rng(64)
    contigs = {"edge_1": rand_contig(rng, 1400), "edge_2": rand_contig(rng, 200)}
    text = ["@HD\tVN:1.6\n"]
    k = 0
    for cigar in EDGE_CIGARS:
        runs = runs_of(cigar)
        need = sum(n for op, n in runs if op in "MD")
        start = int(rng.integers(0, 1400 - need + 1))
        # an empty SEQ would be no token at all: the only-D alignment gets a base that no run consumes
        seq = noisy_read(rng, contigs["edge_1"], start, runs) or "A"
        text.append(sam_line("edge_%d" % k, 16 if k % 2 else 0, "edge_1", start + 1, cigar, seq))
        k += 1
    # an alignment that ends on its contig's last base
    runs = runs_of("20M3D37M")
    text.append(sam_line("last_base", 0, "edge_1", 1400 - 60 + 1, "20M3D37M", noisy_read(rng, contigs["edge_1"], 1340, runs)))
    # two one-column alignments and a long one: with the shuffle their places in the call vary, so several such triples
    for j in range(6):
        for cigar in ("1M", "1I", "150M"):
            runs = runs_of(cigar)
            start = 10 * j
            text.append(sam_line("tri_%d_%s" % (j, cigar), 0, "edge_2", start + 1, cigar, noisy_read(rng, contigs["edge_2"], start, runs)))
    return dict(sam="".join(text).encode(), contigs=contigs, max_coverage=1000, use_secondary=True)


RUNS = dict(sam_a=sam_a, sam_a_primary=sam_a_primary, sam_edges=sam_edges)


def fuzz(seed):
    """<= 200 alignments of <= 400 columns with small random CIGARs, zero-length runs and clips anywhere"""
    rng = np.random.default_rng(9000 + seed)
    contigs = {"f_%d" % i: rand_contig(rng, int(rng.integers(50, 600)), lower=0.3, n_rate=0.03) for i in range(4)}
    text = []
    k = 0
    for cid in sorted(contigs):
        L = len(contigs[cid])
        for _ in range(int(rng.integers(1, 50))):
            runs, cols, trg = [], 0, 0
            start = int(rng.integers(0, L))
            for _ in range(int(rng.integers(1, 40))):
                op = "MIDSH"[rng.integers(0, 5)] if rng.random() < 0.9 else "M"
                n = int(rng.integers(0, 12)) if rng.random() < 0.9 else int(rng.integers(0, 130))
                if op in "MID" and cols + n > 400:
                    continue
                if op in "MD" and start + trg + n > L:
                    continue
                runs.append((op, n))
                cols += n if op in "MID" else 0
                trg += n if op in "MD" else 0
            if cols == 0:
                runs.append(("I", 1))
            text.append(sam_line("fz_%d" % (k % 37), [0, 16, 256][k % 3], cid, start + 1, cigar_of(runs),
                                 noisy_read(rng, contigs[cid], start, runs) + "ACGT"[:k % 3]))
            k += 1
    return dict(sam="".join(text).encode(), contigs=contigs, max_coverage=None, use_secondary=True)
