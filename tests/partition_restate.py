"""A second writing of Trestle's read partitioning (flye/trestle/trestle.py: _evaluate_positions, _classify_reads with
_index_mapping, and the two writers) in the forms the device uses, and the inputs of tests/test_partition.py.  Nothing
here is copied from the reference: tests/golden/make_partition_golden.py runs the reference's own functions on these
inputs and stores what they give.

Forms that differ from the reference's loops, each pinned by the golden runs:
* _evaluate_positions' walk is closed per (edge, position): the column of a position is the rank-th non-gap target column,
  qry_ind a prefix count of non-gap query bytes, an insertion a difference of two such counts;
* the first edge in alignment gives the byte every later edge is compared with, and it is never replaced;
* _classify_reads' per-alignment reset is "the last of one or two alignments counts, three or more give 0";
* a position list is a count array: an entry counts once per occurrence.

A confirm job is dict(side, edges=[Aln], pos={total, sub, del, ins}); an Aln is the record of bubbles_restate (qry_start,
trg_start, trg_end, trg_seq, qry_seq).  A classify job is dict(n_reads, edges=[dict(pos=[...], alns=[Aln])]) where an
alignment's qry_id is "read_<number>"; a run is dict(buffer_count, jobs)."""
import hashlib
import json

import numpy as np

import bubbles_restate as R
import cigar_restate as G
import divergence_restate as DR

LIST_KEYS = ("total", "sub", "del", "ins")
CONFIRM_KEYS = tuple(pre + k for pre in ("conf_", "rej_") for k in LIST_KEYS)
READ_KEYS = ("status", "top_edge", "top_score", "total_score")
STATUS = ("None", "Tied", "Partitioned")


def read_number(aln):
    return int(aln.qry_id.split("_")[1])


# ---- _evaluate_positions ---------------------------------------------------------------------------------------------
def edge_values(aln):
    """per position of [trg_start, trg_end): (query byte, qry_ind, has_ins) after both shifts"""
    qry = R.shift_gaps(aln.trg_seq, aln.qry_seq)
    trg = R.shift_gaps(qry, aln.trg_seq)
    t, q = np.frombuffer(trg.encode("latin-1"), np.uint8), np.frombuffer(qry.encode("latin-1"), np.uint8)
    cols = np.flatnonzero(t != 45)
    before = np.concatenate([[0], np.cumsum(q != 45)])          # non-gap query bytes before a column
    qcount = before[cols]
    prev = np.concatenate([[0], before[cols[:-1] + 1]]) if len(cols) else qcount
    return q[cols], aln.qry_start + qcount, qcount - prev > 0


def confirm(job):
    """-> dict of the eight lists and cons (one list per edge)"""
    edges = job["edges"]
    vals = [edge_values(a) for a in edges]
    assert all(len(v[0]) == a.trg_end - a.trg_start for v, a in zip(vals, edges))
    min_start, max_end = min(a.trg_start for a in edges), max(a.trg_end for a in edges)
    min_end, max_start = min(a.trg_end for a in edges), max(a.trg_start for a in edges)
    out = {k: [] for k in CONFIRM_KEYS}
    cons = [[] for _ in edges]
    held = {k: set(job["pos"][k]) for k in LIST_KEYS}
    for t in sorted(p for p in held["total"] if min_start <= p < max_end):
        if not (t < min_end if job["side"] == 0 else t >= max_start):
            continue
        inside = [(i, t - a.trg_start) for i, a in enumerate(edges) if a.trg_start <= t < a.trg_end]
        flag = dict(ins=False, sub=False)
        flag["del"] = False
        for n, (i, r) in enumerate(inside):
            nuc = vals[i][0][r]
            if vals[i][2][r]:
                flag["ins"] = True
                cons[i].append(int(vals[i][1][r]) - 1)
            ref = vals[inside[0][0]][0][inside[0][1]]
            if n and nuc != ref and ref != 78 and nuc != 78:
                flag["del" if ref == 45 else "sub"] = True
        if flag["del"] or flag["sub"]:
            for i, r in inside:
                cons[i].append(int(vals[i][1][r]))
        if any(flag.values()):
            out["conf_total"].append(t)
            for k in ("sub", "del", "ins"):
                if t in held[k]:
                    out[("conf_" if flag[k] else "rej_") + k].append(t)
        else:
            for k in LIST_KEYS:
                if t in held[k]:
                    out["rej_" + k].append(t)
    out["cons"] = cons
    return out


# ---- _classify_reads -------------------------------------------------------------------------------------------------
def aln_score(aln, pos):
    t, q = np.frombuffer(aln.trg_seq.encode("latin-1"), np.uint8), np.frombuffer(aln.qry_seq.encode("latin-1"), np.uint8)
    cols = np.flatnonzero(t != 45)
    equal = t[cols] == q[cols]
    p = np.asarray(pos, np.int64)
    p = p[(p >= aln.trg_start) & (p < aln.trg_end)]
    return int(equal[p - aln.trg_start].sum())


def classify(job, buffer_count):
    """-> dict(status, top_edge, top_score, total_score per read number; aln_score, aln_counted per alignment)"""
    n = job["n_reads"]
    scores = [dict() for _ in range(n)]                          # read -> {edge: [score of every alignment]}
    per_aln = []
    for e, edge in enumerate(job["edges"]):
        for a in edge["alns"]:
            per_aln.append(aln_score(a, edge["pos"]))
            scores[read_number(a)].setdefault(e, []).append(len(per_aln) - 1)
    counted = [0] * len(per_aln)
    out = {k: [] for k in READ_KEYS}
    for r in range(n):
        top_edge, top, total, tie = -1, 0, 0, False
        for e in sorted(scores[r]):
            mine = scores[r][e]
            s = per_aln[mine[-1]] if len(mine) <= 2 else 0
            if len(mine) <= 2:
                counted[mine[-1]] = 1
            if s - buffer_count > top:
                top_edge, top, tie = e, s, False
            elif s >= top:
                top, tie = s, True
            elif s >= top - buffer_count:
                tie = True
            total += s
        status = 0 if not scores[r] or total == 0 else 1 if tie else 2
        for k, v in zip(READ_KEYS, (status, top_edge if status == 2 else -1, top, total)):
            out[k].append(v)
    out["aln_score"], out["aln_counted"] = per_aln, counted
    return out


# ---- the writers -----------------------------------------------------------------------------------------------------
def confirmed_text(res, pos):
    parts = [("Confirmed", "conf_"), ("Rejected", "rej_"), ("Tentative", None)]
    out = []
    for label, pre in parts:
        for k in ("total", "sub", "del", "ins"):
            lst = sorted(pos[k]) if pre is None else res[pre + k]
            out.append(">%s_%s_positions_%d\n%s\n" % (label, k, len(lst), ",".join(str(x) for x in lst)))
    return "".join(out)


def partitioning_text(res, edge_ids, headers_to_id):
    rows = []
    for r, header in enumerate(headers_to_id):
        st = res["status"][r]
        rows.append((headers_to_id[header], STATUS[st], str(edge_ids[res["top_edge"][r]]) if st == 2 else "NA", res["top_score"][r],
                     res["total_score"][r], header))
    line = lambda row: "\t".join("{:11}".format(h) for h in row) + "\n"
    return line(["Read_ID", "Status", "Edge", "Top Score", "Total Score", "Header"]) + "".join(line(r) for r in sorted(rows))


def digests(res, keys):
    return {k: hashlib.sha256(np.asarray(res[k], np.int32).tobytes()).hexdigest() for k in keys}


def cons_digest(cons):
    h = hashlib.sha256()
    for lst in cons:
        h.update(np.asarray([len(lst)] + lst, np.int32).tobytes())
    return h.hexdigest()


def _aln_part(a):
    return [a.qry_id, a.qry_start, a.trg_start, a.trg_end, a.trg_seq, a.qry_seq]


def confirm_digest(run):
    return hashlib.sha256(json.dumps([[j["side"], [_aln_part(a) for a in j["edges"]], [list(j["pos"][k]) for k in LIST_KEYS]]
                                      for j in run["jobs"]]).encode()).hexdigest()


def classify_digest(run):
    return hashlib.sha256(json.dumps([run["buffer_count"]] + [[j["n_reads"], [[list(e["pos"]), [_aln_part(a) for a in e["alns"]]]
                                                                               for e in j["edges"]]] for j in run["jobs"]]).encode()).hexdigest()


# ---- the crafted confirm run -----------------------------------------------------------------------------------------
def both_gap(a, col):
    """a column of two gaps in front of column col"""
    return a._replace(trg_seq=a.trg_seq[:col] + "-" + a.trg_seq[col:], qry_seq=a.qry_seq[:col] + "-" + a.qry_seq[col:])


def confirm_c_template():
    """48 bases without two equal neighbours, so that a deleted base stays where it is -- except positions 20..23 "ATTC":
    the deletion of 22 in an edge is a gap run shift_gaps moves to 21"""
    rng = np.random.default_rng(717)
    seq = []
    for i in range(48):
        fixed = {20: "A", 21: "T", 22: "T", 23: "C"}.get(i)
        seq.append(fixed or str(rng.choice([b for b in "ACGT" if b != (seq[-1] if seq else "") and not (i == 19 and b == "A")])))
    if seq[24] == "C":
        seq[24] = "G" if seq[25] != "G" else "A"
    return "".join(seq)


def confirm_c():
    seq = confirm_c_template()
    other = lambda p: "ACGT"[("ACGT".index(seq[p]) + 1) % 4]
    # e0 [0, 30), e1 [5, 40) with two bases before its first target column, e2 [2, 35)
    e0 = DR.cols("t", seq, 0, 30, "e0", dele={8, 22}, sub={12: "N", 14: other(14), 16: other(16)}, ins={25: "G"})
    e1 = DR.cols("t", seq, 5, 40, "e1", lead="AC", sub={13: "N", 16: other(16), 33: other(33)}, dele={10})._replace(qry_start=0)
    e2 = DR.cols("t", seq, 2, 35, "e2", dele={10, 18}, sub={16: other(16)})._replace(qry_start=7)
    e2 = both_gap(e2, 15)
    edges = [e0, e1, e2]
    total = [5, 8, 10, 12, 13, 14, 16, 18, 20, 22, 26, 1, 3, 31, 33, 36, 44, -1, 48, 26, 8]
    pos = dict(total=total, sub=[14, 16, 20, 33, 7], ins=[5, 26, 14, 26], **{"del": [8, 10, 14, 18, 3]})
    apart = [DR.cols("t", seq, 0, 10, "a0", sub={4: other(4)}), DR.cols("t", seq, 20, 30, "a1", ins={24: "TT"})._replace(qry_start=-7)]
    apart_pos = dict(total=[4, 15, 25, 9, 20], sub=[4], ins=[25, 15], **{"del": []})
    lone = [DR.cols("t", seq, 3, 20, "l0", ins={6: "A"}, dele={9})._replace(qry_start=0)]
    lone_pos = dict(total=[7, 9, 11], sub=[9], ins=[7], **{"del": [9]})
    jobs = [dict(side=0, edges=edges, pos=pos), dict(side=1, edges=edges, pos=pos), dict(side=0, edges=apart, pos=apart_pos),
            dict(side=1, edges=apart, pos=apart_pos), dict(side=1, edges=lone, pos=lone_pos),
            dict(side=0, edges=edges[::-1], pos=dict(total=[], sub=[1], ins=[], **{"del": []}))]
    return dict(jobs=jobs)


def confirm_job(rng, length, n_edges, side, rate=0.06):
    seq = G.rand_contig(rng, length, lower=0.05, n_rate=0.02)
    edges = []
    for e in range(n_edges):
        start = int(rng.integers(0, length // 4))
        n_trg = int(rng.integers(length // 2, length - start + 1))
        a = R.gen_aln(rng, "t", seq, start, n_trg, rate, rate, rate, "e%d" % e)
        edges.append(a._replace(qry_start=int(rng.integers(0, 50))))
    total = [int(x) for x in rng.integers(-2, length + 3, length // 3)]
    pick = lambda n: [int(x) for x in rng.choice(total, n)] + [int(x) for x in rng.integers(0, length, 3)]
    return dict(side=side, edges=edges, pos=dict(total=total, sub=pick(length // 8), ins=pick(length // 8), **{"del": pick(length // 8)}))


def confirm_d():
    rng = np.random.default_rng(727)
    return dict(jobs=[confirm_job(rng, int(n), int(e), int(s)) for n, e, s in ((1500, 2, 0), (1500, 2, 1), (2900, 3, 0), (700, 1, 1), (1100, 4, 1))])


def confirm_fuzz(seed):
    rng = np.random.default_rng(9000 + seed)
    return dict(jobs=[confirm_job(rng, int(rng.integers(100, 2500)), int(rng.integers(1, 5)), int(rng.integers(0, 2)),
                                  float(rng.choice([0.01, 0.08, 0.2]))) for _ in range(int(rng.integers(1, 6)))])


CONFIRM_RUNS = dict(confirm_c=confirm_c, confirm_d=confirm_d)


# ---- the crafted classify run ----------------------------------------------------------------------------------------
COLUMNS = (63, 64, 65, 1023, 1024, 1025, 2049)


def _read(a, number):
    return a._replace(qry_id="read_%d" % number)


def classify_c_tiles():
    """job 0: one edge; alignments of every edge length in columns, and one with a whole tile of target gaps"""
    rng = np.random.default_rng(737)
    seq = R.rand_seq(rng, 2600)
    alns = [_read(DR.exact_columns(rng, "c", seq, 10 * k, n, "x"), k) for k, n in enumerate(COLUMNS)]
    # columns 0..1023 match positions 100..1123, columns 1024..2047 are target gaps, column 2048 is position 1124
    gap = DR.cols("c", seq, 100, 1140, "x", ins={1123: R.rand_seq(rng, 1024)}, sub={1130: seq[1130].lower()})
    alns.append(_read(gap, len(COLUMNS)))
    # positions: the first and last column of a tile of the gap alignment (1123 is column 1023, 1124 column 2048), its
    # trg_start, trg_end - 1 and trg_end, -1, one beyond every alignment, one twice and one three times
    pos = [100, 1123, 1124, 1139, 1140, -1, 2600, 500, 500, 600, 600, 600, 1130] + [int(x) for x in rng.integers(0, 2100, 40)]
    return dict(n_reads=len(alns) + 1, edges=[dict(pos=pos, alns=alns)])


def _scored(seq, start, end, number, score, pos):
    """an alignment over [start, end) that matches exactly `score` of the positions pos (all inside it)"""
    inside = [p for p in pos if start <= p < end]
    assert len(set(inside)) == len(inside) and score <= len(inside)
    miss = {p: "ACGT"[("ACGT".index(seq[p]) + 1) % 4] for p in inside[score:]}
    return _read(DR.cols("c", seq, start, end, "x", sub=miss), number)


def classify_c_votes():
    """job 1: three edges, positions 10, 20, .. 200 on each; reads by number:
    0 one alignment per edge, scores (9, 2, 1): Partitioned to edge 0 at buffer 3
    1 scores (2, 9, 1): the same, edge 1 -- a first edge below the buffer ties, a later one resets the tie
    2 scores (5, 7): Tied by the second branch     3 scores (7, 5): Tied by the third branch
    4 one, two and three alignments on edges 0, 1, 2: the last, the last, 0
    5 on edge 1 only                                6 no alignment
    7 alignments that match nothing: None           8 scores (3, 0): Tied at buffer 3, Partitioned at buffer 0
    9 scores (0, 3): the same in the other order"""
    rng = np.random.default_rng(747)
    seq = R.rand_seq(rng, 260)
    pos = list(range(10, 210, 10))
    S = lambda number, score, start=0, end=230: _scored(seq, start, end, number, score, pos)
    lower = DR.cols("c", seq, 0, 230, "x", trg_sub={30: seq[30].lower()})
    e0 = [S(0, 9), S(1, 2), S(2, 5), S(3, 7), S(4, 6), S(7, 0), S(8, 3), S(9, 0)]
    e1 = [S(0, 2), S(1, 9), S(2, 7), S(3, 5), S(4, 11), S(4, 4, 5, 150), S(5, 8), S(7, 0), S(8, 0), S(9, 3)]
    e2 = [S(0, 1), S(1, 1), S(4, 12), S(4, 13), S(4, 14, 0, 205), _read(lower, 10)]
    return dict(n_reads=12, edges=[dict(pos=pos, alns=e0), dict(pos=pos, alns=e1), dict(pos=pos + [-1, 230], alns=e2)])


def classify_job(rng, length, n_edges, n_reads, n_alns, rate=0.1):
    edges = []
    for e in range(n_edges):
        seq = G.rand_contig(rng, length, lower=0.05, n_rate=0.01)
        alns = []
        for _ in range(n_alns):
            n_trg = int(rng.integers(1, length + 1))
            start = int(rng.integers(0, length - n_trg + 1))
            alns.append(_read(R.gen_aln(rng, "c", seq, start, n_trg, rate, rate, rate, "x"), int(rng.integers(0, max(1, n_reads - 1)))))
        pos = [int(x) for x in rng.integers(-1, length + 2, int(rng.integers(5, 60)))]
        edges.append(dict(pos=pos + pos[:5], alns=alns))
    return dict(n_reads=n_reads, edges=edges)


def classify_c():
    return dict(buffer_count=3, jobs=[classify_c_tiles(), classify_c_votes()])


def classify_c0():
    return dict(buffer_count=0, jobs=[classify_c_votes()])


def classify_d():
    rng = np.random.default_rng(757)
    return dict(buffer_count=3, jobs=[classify_job(rng, 2900, 2, 12, 20), classify_job(rng, 400, 3, 25, 30), classify_job(rng, 900, 1, 4, 6),
                                      dict(n_reads=3, edges=[dict(pos=[1, 2], alns=[])])])


def classify_fuzz(seed):
    rng = np.random.default_rng(9500 + seed)
    return dict(buffer_count=int(rng.integers(0, 5)),
                jobs=[classify_job(rng, int(rng.integers(50, 2500)), int(rng.integers(1, 5)), int(rng.integers(1, 12)), int(rng.integers(0, 25)),
                                   float(rng.choice([0.02, 0.1, 0.3]))) for _ in range(int(rng.integers(1, 5)))])


CLASSIFY_RUNS = dict(classify_c=classify_c, classify_c0=classify_c0, classify_d=classify_d)


# ---- the arrays of the two calls -------------------------------------------------------------------------------------
def _columns(alns):
    return dict(col_off=np.cumsum([0] + [len(a.trg_seq) for a in alns]).astype(np.uint64),
                trg_cols="".join(a.trg_seq for a in alns).encode("latin-1"), qry_cols="".join(a.qry_seq for a in alns).encode("latin-1"))


def confirm_arrays(jobs):
    edges = [a for j in jobs for a in j["edges"]]
    out = dict(side=np.array([j["side"] for j in jobs], np.uint8),
               job_edge_off=np.cumsum([0] + [len(j["edges"]) for j in jobs]).astype(np.uint64),
               trg_start=np.array([a.trg_start for a in edges], np.int32), trg_end=np.array([a.trg_end for a in edges], np.int32),
               qry_start=np.array([a.qry_start for a in edges], np.int32), **_columns(edges))
    for k in LIST_KEYS:
        out[k + "_off"] = np.cumsum([0] + [len(j["pos"][k]) for j in jobs]).astype(np.uint64)
        out[k + "_pos"] = np.array([p for j in jobs for p in j["pos"][k]], np.int32)
    return out


def classify_arrays(jobs):
    edges = [e for j in jobs for e in j["edges"]]
    alns = [a for e in edges for a in e["alns"]]
    return dict(job_edge_off=np.cumsum([0] + [len(j["edges"]) for j in jobs]).astype(np.uint64),
                job_n_reads=np.array([j["n_reads"] for j in jobs], np.uint32),
                edge_pos_off=np.cumsum([0] + [len(e["pos"]) for e in edges]).astype(np.uint64),
                edge_pos=np.array([p for e in edges for p in e["pos"]], np.int32),
                edge_aln_off=np.cumsum([0] + [len(e["alns"]) for e in edges]).astype(np.uint64),
                read=np.array([read_number(a) for a in alns], np.uint32), trg_start=np.array([a.trg_start for a in alns], np.int32),
                trg_end=np.array([a.trg_end for a in alns], np.int32), **_columns(alns))


# ---- the SAM-file runs of partition_reads ----------------------------------------------------------------------------
def _sam_records(rng, target_id, target, prefix, count, span, flags=(0,)):
    """reads 0 .. 23 once, 0 .. 3 a second time, read 0 twice more: four alignments score 0"""
    lines = []
    for k in range(count):
        n_trg = int(rng.integers(span // 2, span + 1))
        start = int(rng.integers(0, len(target) - n_trg + 1))
        runs = G.noisy_runs(rng, n_trg, max_run=15)
        lines.append((start, G.sam_line("%s%d" % (prefix, k % 24 if k < 28 else 0), flags[k % len(flags)], target_id, start + 1, G.cigar_of(runs),
                                        G.noisy_read(rng, target, start, runs, sub=0.05))))
    return "".join(text for _, text in lines)


def _trg_len(runs):
    return sum(n for op, n in runs if op in "MD")


def sam_run(seed, it=1, side="in", edges=(3, -7), missing=(), split_first=False):
    """the files of one partition_reads call as {name: text}: the template, the positions file, per edge the consensus, its
    alignment to the template and the reads' alignments to it; `missing` names files that are left out"""
    rng = np.random.default_rng(seed)
    template = G.rand_contig(rng, 1400, lower=0.0, n_rate=0.0)
    files = {"template.fasta": ">template\n%s\n" % template}
    total = sorted(set(int(x) for x in rng.integers(0, 1400, 220)))
    part = lambda n: sorted(set(int(x) for x in rng.choice(total, n)))
    pos = dict(total=total, sub=part(90), ins=part(60), **{"del": part(60)})
    files["positions.txt"] = "".join(">%s_positions\n%s\n" % (k, ",".join(str(x) for x in pos[k])) for k in LIST_KEYS)
    headers = ["read_%d" % k for k in range(36)]
    for e in edges:
        # the consensus: the template's stretch with its own differences, aligned back in one or two records
        lo, hi = (0, 1250) if e == edges[0] else (100, 1400)
        if split_first and e == edges[0]:
            # two records, the second supplementary and 7 template bases further on: _collapse_cons_aln joins them
            runs_a = G.noisy_runs(rng, 600, max_run=40) + [("M", 5)]
            runs_b = [("M", 5)] + G.noisy_runs(rng, 500, max_run=40)
            mid = lo + _trg_len(runs_a) + 7
            cons_a, cons_b = G.noisy_read(rng, template, lo, runs_a, sub=0.03), G.noisy_read(rng, template, mid, runs_b, sub=0.03)
            cons = cons_a + cons_b
            sam = G.sam_line("edge_%d" % e, 0, "template", lo + 1, G.cigar_of(runs_a) + "%dS" % len(cons_b), cons) + \
                G.sam_line("edge_%d" % e, 2048, "template", mid + 1, "%dS" % len(cons_a) + G.cigar_of(runs_b), cons)
        else:
            runs = G.noisy_runs(rng, hi - lo, max_run=40)
            cons = G.noisy_read(rng, template, lo, runs, sub=0.03)
            sam = G.sam_line("edge_%d" % e, 0, "template", lo + 1, G.cigar_of(runs), cons)
        files["cons_%d.fasta" % e] = ">edge_%d\n%s\n" % (e, cons)
        files["cons_aln_%d.sam" % e] = "@HD\tVN:1.6\n" + sam
        files["read_aln_%d.sam" % e] = "@HD\tVN:1.6\n" + _sam_records(rng, "edge_%d" % e, cons, "read_", 30, 500, flags=(0, 16, 0, 2048))
    for name in missing:
        del files[name]
    return dict(files=files, it=it, side=side, edges=list(edges), headers_to_id={h: 100 + 3 * k for k, h in enumerate(headers)})


def sam_first():
    return sam_run(818)


def sam_out():
    return sam_run(828, it=2, side="out", edges=(5, 6, 11), split_first=True)


def _earlier_part(run, it):
    """a partitioning file of iteration `it` as the step before would have left it"""
    n = len(run["headers_to_id"])
    res = dict(status=[k % 3 for k in range(n)], top_edge=[k % len(run["edges"]) if k % 3 == 2 else -1 for k in range(n)],
               top_score=[k % 7 for k in range(n)], total_score=[k % 7 + k % 3 for k in range(n)])
    run["files"]["part.%d.%s.txt" % (it, run["side"])] = partitioning_text(res, run["edges"], run["headers_to_id"])
    return run


def sam_skip():
    """iteration 1 without one consensus alignment: empty lists, and the partitioning of iteration 0 again"""
    return _earlier_part(sam_run(838, missing=("cons_aln_3.sam",)), 0)


def sam_skip_later():
    """iteration 3 with a consensus alignment file that holds no record: the confirmed file of iteration 2 again"""
    run = _earlier_part(sam_run(848, it=3, side="out"), 2)
    run["files"]["cons_aln_-7.sam"] = "@HD\tVN:1.6\n"
    res = confirm(confirm_c()["jobs"][1])
    run["files"]["confirmed.2.out.txt"] = confirmed_text(res, confirm_c()["jobs"][1]["pos"])
    return run


SAMS = dict(sam_first=sam_first, sam_out=sam_out, sam_skip=sam_skip, sam_skip_later=sam_skip_later)


def sam_digest(run):
    return hashlib.sha256(json.dumps([run["it"], run["side"], run["edges"], run["headers_to_id"], sorted(run["files"].items())]).encode()).hexdigest()


def write_files(run, folder):
    """writes the run's files; -> the arguments of partition_reads behind (edges, it, side)"""
    import os
    p = lambda name: os.path.join(folder, name)
    for name, text in run["files"].items():
        with open(p(name), "w") as f:
            f.write(text)
    it, side = run["it"], run["side"]
    for e in run["edges"]:
        for src, dst in (("cons_aln_%d.sam" % e, "cons_aln.%d.%s.%d.sam" % (it, side, e)), ("read_aln_%d.sam" % e, "read_aln.%d.%s.%d.sam" % (it, side, e))):
            if os.path.exists(p(src)):
                os.replace(p(src), p(dst))
    consensuses = {(it, side, e): p("cons_%d.fasta" % e) for e in run["edges"]}
    return dict(position_path=p("positions.txt"), cons_align_path=p("cons_aln.{0}.{1}.{2}.sam"), template=p("template.fasta"),
                read_align_path=p("read_aln.{0}.{1}.{2}.sam"), consensuses=consensuses, confirmed_pos_path=p("confirmed.{0}.{1}.txt"),
                part_file=p("part.{0}.{1}.txt"), headers_to_id=run["headers_to_id"])
