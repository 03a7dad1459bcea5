"""fg_divergence_profile_cigars and fg_classify_reads_cigars against the two-step path on seeded synthetic records
(tools/expand_cigars_bench.py) in the shapes of tools/divergence_bench.py and tools/partition_bench.py:
    divergence   one template of 200 kb, 2000 alignments of 10 kb with ~12 % errors
    classify     one job, two edge consensuses of 200 kb, 2000 alignments of 10 kb (1000 reads, one alignment on each
                 edge), 2000 positions per edge
First checks that every array of both fused results equals the two-step result (the profile and the scores included), then
times, after one warm-up each and over --repeat repetitions, through gpu.Context:
    two-step   fg_expand_cigars(want_cols = 1), then fg_divergence_profile / fg_classify_reads on the columns it returned
    fused      the one call on the records
Prints the wall times (best and median), the bytes the two-step path moves over the bus for the columns and the device time
per kernel of the last repetition; --json writes the same as a file.  There is no pass bar: parity is the condition.
    python tools/trestle_fused_bench.py [--length 200000] [--alignments 2000] [--read 10000] [--positions 2000] [--seed 2024]
                                        [--repeat 5] [--json PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import cigar_restate as G  # noqa: E402
from expand_cigars_bench import bench_input  # noqa: E402

THRESHOLDS = (0.1, 0.2, 0.3)
BUFFER_COUNT = 3


def same(a, b):
    return a.__dict__.keys() == b.__dict__.keys() and all(
        (v is None and b.__dict__[k] is None) or (v.dtype == b.__dict__[k].dtype and v.tobytes() == b.__dict__[k].tobytes())
        for k, v in a.__dict__.items())


def kernels(ctx):
    return {name: dict(ms=round(sec * 1e3, 4), launches=int(n)) for name, (sec, n) in ctx.kernel_times().items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=200000)
    ap.add_argument("--alignments", type=int, default=2000)
    ap.add_argument("--read", type=int, default=10000)
    ap.add_argument("--positions", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from flye_amd import gpu
    t0 = time.perf_counter()
    # divergence: one template
    run, recs = bench_input(a.length, a.alignments, a.read, a.seed)
    dv_ex = G.call_arrays(recs, run["contigs"])
    dv_rec = {k: v for k, v in dv_ex.items() if k != "aln_contig"}
    dv_rec["contig_aln_off"] = np.array([0, len(recs)], np.uint64)
    # classify: two edges, read k has alignment k of each
    half = a.alignments // 2
    contigs, cl_recs = {}, []
    for e in range(2):
        r, rs = bench_input(a.length, half, a.read, a.seed + 1 + e)
        contigs["edge_%d" % e] = r["contigs"]["contig_1"]
        cl_recs += [dict(x, contig=b"edge_%d" % e) for x in rs]
    cl_ex = G.call_arrays(cl_recs, contigs)
    rng = np.random.default_rng(a.seed + 3)
    job = dict(job_edge_off=np.array([0, 2], np.uint64), job_n_reads=np.array([half], np.uint32),
               edge_pos_off=np.array([0, a.positions, 2 * a.positions], np.uint64),
               edge_pos=rng.integers(0, a.length, 2 * a.positions).astype(np.int32),
               edge_aln_off=np.array([0, half, 2 * half], np.uint64), read=np.tile(np.arange(half, dtype=np.uint32), 2))
    cl_rec = {k: v for k, v in cl_ex.items() if k not in ("aln_contig", "contig_off", "contig_seq")}
    print("divergence: %d bp, %d alignments, %d runs; classify: 2 edges of %d bp, %d alignments, %d runs; generated in %.1f s" %
          (a.length, len(recs), len(dv_ex["run_len"]), a.length, len(cl_recs), len(cl_ex["run_len"]), time.perf_counter() - t0), flush=True)
    ctx = gpu.Context(17, 0)
    lens = [a.length]

    def two_step_div(full=False):
        ex = ctx.expand_cigars(**dv_ex)
        k = kernels(ctx)
        return ctx.divergence_profile(*THRESHOLDS, lens, dv_rec["contig_aln_off"], ex.trg_start, ex.col_off, ex.trg_cols, ex.qry_cols, full), k, ex

    def two_step_cl(full=False):
        ex = ctx.expand_cigars(**cl_ex)
        k = kernels(ctx)
        return ctx.classify_reads(BUFFER_COUNT, job["job_edge_off"], job["job_n_reads"], job["edge_pos_off"], job["edge_pos"], job["edge_aln_off"],
                                  job["read"], ex.trg_start, ex.trg_end, ex.col_off, ex.trg_cols, ex.qry_cols, full), k, ex

    fused_div = lambda full=False: (ctx.divergence_profile_cigars(*THRESHOLDS, want_profile=full, **dv_rec), {}, None)
    fused_cl = lambda full=False: (ctx.classify_reads_cigars(
        BUFFER_COUNT, job["job_edge_off"], job["job_n_reads"], job["edge_pos_off"], job["edge_pos"], cl_ex["contig_off"], cl_ex["contig_seq"],
        job["edge_aln_off"], job["read"], want_scores=full, **cl_rec), {}, None)

    # the check, which is the warm-up of all four as well
    want_div, _, ex_div = two_step_div(True)
    assert same(fused_div(True)[0], want_div), "fg_divergence_profile_cigars differs from the two-step path"
    want_cl, _, ex_cl = two_step_cl(True)
    assert same(fused_cl(True)[0], want_cl), "fg_classify_reads_cigars differs from the two-step path"
    cols = dict(divergence_profile=int(ex_div.col_off[-1]), classify_reads=int(ex_cl.col_off[-1]))
    print("check: %d and %d columns, %d called positions, None / Tied / Partitioned %s; both fused calls identical to the two-step path, "
          "profile and scores included" % (cols["divergence_profile"], cols["classify_reads"], len(want_div.total_pos),
                                           np.bincount(want_cl.status, minlength=3).tolist()), flush=True)
    out = dict(length=a.length, alignments=a.alignments, positions=a.positions, repeat=a.repeat, stages={})
    for stage, paths in (("divergence_profile", (("two_step", two_step_div), ("fused", fused_div))),
                         ("classify_reads", (("two_step", two_step_cl), ("fused", fused_cl)))):
        s = out["stages"][stage] = dict(columns=cols[stage], column_bytes_down_and_up_two_step=4 * cols[stage])
        for label, fn in paths:
            fn()                                                       # one warm-up
            walls = []
            for _ in range(a.repeat):
                t0 = time.perf_counter()
                _, expand_kernels, _ = fn()
                walls.append(time.perf_counter() - t0)
            k = dict(expand_kernels, **kernels(ctx)) if label == "two_step" else kernels(ctx)
            s[label] = dict(best_s=round(min(walls), 5), median_s=round(statistics.median(walls), 5),
                            kernel_ms_total=round(sum(v["ms"] for v in k.values()), 3), kernels=k)
            print("%-18s %-8s best %.4f s, median %.4f s, kernels %.2f ms" %
                  (stage, label, min(walls), statistics.median(walls), sum(v["ms"] for v in k.values())), flush=True)
            for name, v in k.items():
                print("   %-15s %9.3f ms in %3d launches" % (name, v["ms"], v["launches"]))
        s["fused_over_two_step_median"] = round(s["fused"]["median_s"] / s["two_step"]["median_s"], 4)
        print("%s: fused / two-step = %.3f (median wall time)" % (stage, s["fused_over_two_step_median"]), flush=True)
    ctx.close()
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
