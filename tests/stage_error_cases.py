"""The nine stage calls of the C ABI on one tiny input, valid and with one (or, where named, two) faults: what
tests/test_stage_errors.py runs and tests/golden/make_stage_errors_golden.py records.

The input: 3 contigs of 60, 48 and 72 bases, the second without alignments; 5 alignments of 30 - 70 columns with gaps on
both sides; the same alignments as CIGAR runs for the three calls that take records; 2 jobs of 2 edges for the two
partition calls.  A call is described once (CALLS): its symbol, the arguments in the ABI's order, the wrapper of
gpu.Context that copies a result out, and how the largest cost of an item is counted for the budget switch.

variants(call) yields (name, arguments, environment).  A variant exists for a call where the argument exists:
  null:X            pointer X is NULL (an optional pointer gives 0: recorded as such)
  null:out, null:params
  swapped:X         two ascending entries of offsets array X change places
  contig_len:-1, byte128:trg_cols, byte128:qry_cols, trg_start:-1 (ctg_pos 0 for records), trg_start:len (ctg_pos
  past the contig for records; fg_uniform_alignments takes a start on the last base's window: 0), short_contig (one base
  fewer than its longest alignment covers), nan:err_rate, nan:threshold, budget (the switch at largest cost - 1; not for
  fg_uniform_alignments, whose costs are 0 on contigs below 100 bases)
  two:trg_start+byte128, two:col_off+contig_len     the order of the reports, for the three calls that take columns
"""
import ctypes as C

import numpy as np


def _alignment(rng, contig, start, n_trg):
    """gapped strings over contig[start : start + n_trg]: a match column first and last"""
    t, q = bytearray(), bytearray()
    for k in range(n_trg):
        base = contig[start + k]
        inner = 0 < k < n_trg - 1
        if inner and rng.random_sample() < 0.08:
            for _ in range(int(rng.randint(1, 3))):
                t.append(ord("-")); q.append(b"ACGT"[rng.randint(4)])
        if inner and rng.random_sample() < 0.08:
            t.append(base); q.append(ord("-"))
        else:
            t.append(base); q.append(b"ACGT"[rng.randint(4)] if inner and rng.random_sample() < 0.1 else base)
    return bytes(t), bytes(q)


def _runs(t, q):
    ops, lens = [], []
    for a, b in zip(t, q):
        op = ord("I") if a == ord("-") else ord("D") if b == ord("-") else ord("M")
        if ops and ops[-1] == op:
            lens[-1] += 1
        else:
            ops.append(op); lens.append(1)
    return ops, lens


def inputs():
    """every array of every call, by the ABI's argument name (fg_confirm_positions' per-edge arrays under pt_)"""
    rng = np.random.RandomState(20240)
    u8, i32, u32, u64, f64 = np.uint8, np.int32, np.uint32, np.uint64, np.float64
    contig_len = [60, 48, 72]
    contigs = [bytes(b"ACGT"[i] for i in rng.randint(4, size=n)) for n in contig_len]
    placed = [(0, 0, 48), (0, 5, 35), (0, 10, 30), (2, 3, 60), (2, 12, 40)]          # contig, trg_start, target bases
    cols = [_alignment(rng, contigs[c], s, n) for c, s, n in placed]
    assert all(30 <= len(t) <= 120 and b"-" in t + q for t, q in cols) and any(b"-" in t for t, _ in cols) and any(b"-" in q for _, q in cols)
    runs = [_runs(t, q) for t, q in cols]
    reads = [q.replace(b"-", b"") for _, q in cols]
    off = lambda lens: np.concatenate([[0], np.cumsum(lens)]).astype(u64)
    A = dict(
        contig_len=np.array(contig_len, i32), contig_circular=np.zeros(3, u8), contig_aln_off=np.array([0, 3, 3, 5], u64),
        trg_start=np.array([s for _, s, _ in placed], i32), trg_end=np.array([s + n for _, s, n in placed], i32),
        err_rate=np.array([0.05, 0.1, 0.02, 0.08, 0.12], f64), is_secondary=np.array([0, 0, 1, 0, 0], u8),
        qry_id=np.array([0, 1, 2, 0, 3], i32), use=np.array([1, 1, 0, 1, 1], u8),
        col_off=off([len(t) for t, _ in cols]), trg_cols=np.frombuffer(b"".join(t for t, _ in cols), u8).copy(),
        qry_cols=np.frombuffer(b"".join(q for _, q in cols), u8).copy(),
        contig_off=off(contig_len), contig_seq=np.frombuffer(b"".join(contigs), u8).copy(),
        aln_contig=np.array([c for c, _, _ in placed], u32), ctg_pos=np.array([s + 1 for _, s, _ in placed], i32),
        run_off=off([len(o) for o, _ in runs]), run_op=np.array([o for ops, _ in runs for o in ops], u8),
        run_len=np.array([n for _, lens in runs for n in lens], u32), read_off=off([len(r) for r in reads]),
        read_seq=np.frombuffer(b"".join(reads), u8).copy())
    # confirm: the first four alignments as the edges of two jobs; the tentative lists hold positions of both jobs' ranges
    e = slice(0, 4)
    A.update(side=np.array([0, 1], u8), job_edge_off=np.array([0, 2, 4], u64), pt_trg_start=A["trg_start"][e].copy(),
             pt_trg_end=A["trg_end"][e].copy(), qry_start=np.array([0, 2, 1, 0], i32), pt_col_off=A["col_off"][:5].copy(),
             total_off=np.array([0, 4, 8], u64), total_pos=np.array([12, 15, 20, 30, 15, 20, 25, 40], i32),
             sub_off=np.array([0, 2, 4], u64), sub_pos=np.array([12, 20, 15, 25], i32),
             del_off=np.array([0, 1, 3], u64), del_pos=np.array([15, 20, 40], i32),
             ins_off=np.array([0, 2, 3], u64), ins_pos=np.array([20, 30, 25], i32))
    # classify: the five alignments on four edges (the third has two)
    A.update(job_n_reads=np.array([3, 2], u32), edge_pos_off=np.array([0, 3, 5, 8, 10], u64),
             edge_pos=np.array([5, 12, 30, 8, 20, 15, 15, 33, 20, 41], i32), edge_aln_off=np.array([0, 1, 2, 4, 5], u64),
             read=np.array([0, 2, 1, 0, 1], u32))
    return A


def _bubble_params():
    from flye_amd import gpu
    return gpu.BubbleParams.for_mode("pacbio", min_polish_aln_len=20)


COLUMNS = ("contig_len", "contig_aln_off", "trg_start", "col_off", "trg_cols", "qry_cols")
RECORDS = ("contig_off", "contig_seq", "contig_aln_off", "ctg_pos", "run_off", "run_op", "run_len", "read_off", "read_seq")
# name: symbol, release, batch class, arguments in the ABI's order (names of inputs() or SCALARS, or params), whether a
# want flag stands before out, the wrapper of gpu.Context as (method, its arguments, the keyword of the want flag), the
# switch of the budget
CALLS = dict(
    uniform=("fg_uniform_alignments", "fg_release_uniform", "UniformResultStruct",
             ["n_contigs", "contig_len", "contig_aln_off", "trg_start", "trg_end", "err_rate", "is_secondary"], True,
             ("uniform_alignments", ["contig_len", "contig_aln_off", "trg_start", "trg_end", "err_rate", "is_secondary"], "want_thresholds"), None),
    consensus=("fg_contig_consensus", "fg_release_consensus", "ConsensusBatch",
               ["n_contigs", "contig_len", "contig_aln_off", "trg_start", "qry_id", "use", "col_off", "trg_cols", "qry_cols"], True,
               ("contig_consensus", ["contig_len", "contig_aln_off", "trg_start", "qry_id", "col_off", "trg_cols", "qry_cols", "use"], "want_profile"),
               "FG_CONSENSUS_BATCH_COLS"),
    bubbles=("fg_make_bubbles", "fg_release_bubbles", "BubbleBatch",
             ["params", "n_contigs", "contig_len", "contig_circular", "contig_aln_off", "trg_start", "trg_end", "err_rate", "col_off",
              "trg_cols", "qry_cols"], True,
             ("make_bubbles", ["params", "contig_len", "contig_circular", "contig_aln_off", "trg_start", "trg_end", "err_rate", "col_off",
                               "trg_cols", "qry_cols"], "want_profile"), "FG_BUBBLE_BATCH_COLS"),
    expand=("fg_expand_cigars", "fg_release_expand", "ExpandBatch",
            ["n_contigs", "contig_off", "contig_seq", "n_alignments", "aln_contig", "ctg_pos", "run_off", "run_op", "run_len", "read_off",
             "read_seq"], True,
            ("expand_cigars", ["contig_off", "contig_seq", "aln_contig", "ctg_pos", "run_off", "run_op", "run_len", "read_off", "read_seq"],
             "want_cols"), "FG_CIGAR_BATCH_COLS"),
    consensus_cigars=("fg_contig_consensus_cigars", "fg_release_consensus", "ConsensusBatch",
                      ["n_contigs"] + list(RECORDS) + ["qry_id", "use"], True,
                      ("contig_consensus_cigars", list(RECORDS) + ["qry_id", "use"], "want_profile"), "FG_CONSENSUS_BATCH_COLS"),
    bubbles_cigars=("fg_make_bubbles_cigars", "fg_release_bubbles", "BubbleBatch",
                    ["params", "n_contigs", "contig_off", "contig_seq", "contig_circular"] + list(RECORDS[2:]) + ["err_rate"], True,
                    ("make_bubbles_cigars", ["params", "contig_off", "contig_seq", "contig_circular"] + list(RECORDS[2:]) + ["err_rate"],
                     "want_profile"), "FG_BUBBLE_BATCH_COLS"),
    divergence=("fg_divergence_profile", "fg_release_divergence", "DivergenceBatch",
                ["sub_thresh", "del_thresh", "ins_thresh", "n_contigs"] + list(COLUMNS), True,
                ("divergence_profile", ["sub_thresh", "del_thresh", "ins_thresh"] + list(COLUMNS), "want_profile"), "FG_DIVERGENCE_BATCH_COLS"),
    confirm=("fg_confirm_positions", "fg_release_confirm", "ConfirmBatch",
             ["n_jobs", "side", "job_edge_off", "pt_trg_start", "pt_trg_end", "qry_start", "pt_col_off", "trg_cols", "qry_cols", "total_off",
              "total_pos", "sub_off", "sub_pos", "del_off", "del_pos", "ins_off", "ins_pos"], False,
             ("confirm_positions", ["side", "job_edge_off", "pt_trg_start", "pt_trg_end", "qry_start", "pt_col_off", "trg_cols", "qry_cols",
                                    "total_off", "total_pos", "sub_off", "sub_pos", "del_off", "del_pos", "ins_off", "ins_pos"], None),
             "FG_PARTITION_BATCH_COLS"),
    classify=("fg_classify_reads", "fg_release_classify", "ClassifyBatch",
              ["buffer_count", "n_jobs", "job_edge_off", "job_n_reads", "edge_pos_off", "edge_pos", "edge_aln_off", "read", "trg_start",
               "trg_end", "col_off", "trg_cols", "qry_cols"], True,
              ("classify_reads", ["buffer_count", "job_edge_off", "job_n_reads", "edge_pos_off", "edge_pos", "edge_aln_off", "read", "trg_start",
                                  "trg_end", "col_off", "trg_cols", "qry_cols"], "want_scores"), "FG_PARTITION_BATCH_COLS"))
SCALARS = dict(n_contigs=3, n_alignments=5, n_jobs=2, buffer_count=1, sub_thresh=0.1, del_thresh=0.2, ins_thresh=0.3)
TAKES_COLUMNS = ("consensus", "bubbles", "divergence")
TAKES_RECORDS = ("expand", "consensus_cigars", "bubbles_cigars")


def valid(call):
    """the arguments of a call by name: arrays, scalars and the bubble parameters"""
    A = dict(inputs(), **SCALARS)
    A["params"] = _bubble_params()
    return A


def largest_cost(call, A):
    """the largest cost of one item as the call counts it for its budget switch"""
    cols = lambda off, lo, hi: int(off[hi]) - int(off[lo])
    cao = A["contig_aln_off"]
    per_contig = [cols(A["col_off"], int(cao[i]), int(cao[i + 1])) for i in range(3)]
    if call in ("consensus", "bubbles", "consensus_cigars", "bubbles_cigars"):
        return max(int(A["contig_len"][i]) + per_contig[i] for i in range(3))
    if call == "divergence":
        return max(int(A["contig_len"][i]) * len(set(A["qry_cols"].tolist())) + per_contig[i] for i in range(3))
    if call == "expand":
        return max(cols(A["col_off"], a, a + 1) for a in range(5))
    jeo = A["job_edge_off"]
    if call == "confirm":
        return max(cols(A["pt_col_off"], int(jeo[j]), int(jeo[j + 1])) + int(A["pt_trg_end"][int(jeo[j]):int(jeo[j + 1])].max()) -
                   int(A["pt_trg_start"][int(jeo[j]):int(jeo[j + 1])].min()) for j in range(2))
    eao, cost = A["edge_aln_off"], []
    for j in range(2):
        alns = lambda e: slice(int(eao[e]), int(eao[e + 1]))
        cells = sum(int(A["trg_end"][alns(e)].max()) - int(A["trg_start"][alns(e)].min()) for e in range(int(jeo[j]), int(jeo[j + 1])))
        cost.append(cells + cols(A["col_off"], int(eao[int(jeo[j])]), int(eao[int(jeo[j + 1])])))
    return max(cost)


def _changed(A, name, at, value):
    bad = A[name].copy()
    bad[at] = value
    return {name: bad}


def _swapped(A, name):
    bad = A[name].copy()
    i = next(i for i in range(1, len(bad) - 1) if bad[i] < bad[i + 1])
    bad[i], bad[i + 1] = A[name][i + 1], A[name][i]
    return {name: bad}


def variants(call):
    """(name, the arguments that differ from valid(call), environment) of every faulty variant of a call"""
    A = valid(call)
    args, budget = CALLS[call][3], CALLS[call][6]
    arrays = [k for k in args if isinstance(A[k], np.ndarray)]
    pre = "pt_" if call == "confirm" else ""
    for k in arrays:
        yield "null:" + k, {k: None}, {}
    yield "null:out", {"out": None}, {}
    if "params" in args:
        yield "null:params", {"params": None}, {}
    for k in arrays:
        if k.endswith("_off"):
            yield "swapped:" + k, _swapped(A, k), {}
    if "contig_len" in args:
        yield "contig_len:-1", _changed(A, "contig_len", 2, -1), {}
    if pre + "col_off" in args:
        for k in ("trg_cols", "qry_cols"):
            yield "byte128:" + k, _changed(A, k, int(A["col_off"][3]) + 7, 128), {}
    if pre + "trg_start" in args:
        last = len(A[pre + "trg_start"]) - 1
        yield "trg_start:-1", _changed(A, pre + "trg_start", last, -1), {}
        if "contig_len" in args:
            yield "trg_start:len", _changed(A, "trg_start", 4, int(A["contig_len"][2])), {}
    if "ctg_pos" in args:
        yield "trg_start:-1", _changed(A, "ctg_pos", 4, 0), {}
        yield "trg_start:len", _changed(A, "ctg_pos", 4, int(A["contig_len"][2]) + 1), {}
    if call in TAKES_COLUMNS:
        yield "short_contig", _changed(A, "contig_len", 0, 47), {}
        yield "two:trg_start+byte128", dict(_changed(A, "trg_start", 3, -1), **_changed(A, "qry_cols", int(A["col_off"][3]) + 7, 128)), {}
        yield "two:col_off+contig_len", dict(_swapped(A, "col_off"), **_changed(A, "contig_len", 2, -1)), {}
    if "err_rate" in args:
        yield "nan:err_rate", _changed(A, "err_rate", 1, float("nan")), {}
    if call == "divergence":
        yield "nan:threshold", {"del_thresh": float("nan")}, {}
    if budget:
        yield "budget", {}, {budget: str(largest_cost(call, A) - 1)}


def run_raw(lib, ctx, call, changed=None):
    """the call through ctypes with `changed` over valid(call); *out starts non-zero.  Returns (code, fg_last_error's text,
    *out is all zero, None without out); a batch that was handed out is released."""
    from flye_amd import gpu
    symbol, release, batch, args, want = CALLS[call][:5]
    A = dict(valid(call), out=True)
    A.update(changed or {})
    b = getattr(gpu, batch)()
    C.memset(C.byref(b), 0x5a, C.sizeof(b))
    raw = []
    for k in args:
        v = A[k]
        raw.append(v.ctypes.data if isinstance(v, np.ndarray) else C.byref(v) if isinstance(v, C.Structure) else v)
    rc = getattr(lib, symbol)(ctx.h, *raw, *([1] if want else []), C.byref(b) if A["out"] else None)
    text = lib.fg_last_error(ctx.h).decode()
    zero = bytes(b) == bytes(C.sizeof(b)) if A["out"] else None
    if rc == 0:
        getattr(lib, release)(C.byref(b))
    return rc, text, zero


def run_wrapped(ctx, call):
    """the valid call through gpu.Context: the result copied out, every optional array asked for"""
    A = valid(call)
    method, names, want = CALLS[call][5]
    kw = {want: True} if want else {}
    pos = [A[k] for k in names]
    if call in ("consensus", "consensus_cigars"):
        kw["use"] = pos.pop()
    return getattr(ctx, method)(*pos, **kw)
