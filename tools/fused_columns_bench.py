"""fg_contig_consensus_cigars and fg_make_bubbles_cigars against the two-step path on the seeded synthetic input of
tools/expand_cigars_bench.py: one contig of 200 kb, 2000 alignments of 10 kb with ~12 % errors.  First checks that the
fused results equal the two-step results array for array (profiles included), then times, after one warm-up each and over
--repeat repetitions, through gpu.Context:
    two-step   fg_expand_cigars(want_cols = 1), then fg_contig_consensus / fg_make_bubbles on the columns it returned
    fused      the one call on the records
The coverage cap (fg_uniform_alignments on a want_cols = 0 expansion) is the same for both and is not timed.  Prints the
wall times (best and median), the bytes the two-step path moves over the bus for the columns and the device time per kernel
of the last repetition; --json writes the same as a file.  There is no pass bar.
    python tools/fused_columns_bench.py [--length 200000] [--alignments 2000] [--read 10000] [--seed 2024] [--repeat 5] [--json PATH]"""
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
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from flye_amd import gpu
    t0 = time.perf_counter()
    run, recs = bench_input(a.length, a.alignments, a.read, a.seed)
    ex_args = G.call_arrays(recs, run["contigs"])
    n = len(recs)
    rec_args = {k: v for k, v in ex_args.items() if k != "aln_contig"}
    rec_args["contig_aln_off"] = np.array([0, n], np.uint64)
    qry_id = np.arange(n, dtype=np.int32)
    lens, aln_off = [a.length], rec_args["contig_aln_off"]
    print("contig of %d bp, %d alignments, %d runs, generated in %.1f s" % (a.length, n, len(ex_args["run_len"]), time.perf_counter() - t0),
          flush=True)
    ctx = gpu.Context(17, 0)
    params = gpu.BubbleParams.for_mode("pacbio")
    scal = ctx.expand_cigars(want_cols=False, **ex_args)
    use = ctx.uniform_alignments(lens, aln_off, scal.trg_start, scal.trg_end, scal.err_rate).keep
    n_cols = int(scal.col_off[-1])

    def two_step_cons(profile=False):
        ex = ctx.expand_cigars(**ex_args)
        k = kernels(ctx)
        res = ctx.contig_consensus(lens, aln_off, ex.trg_start, qry_id, ex.col_off, ex.trg_cols, ex.qry_cols, use, profile)
        return res, k

    def two_step_bub(profile=False):
        ex = ctx.expand_cigars(**ex_args)
        k = kernels(ctx)
        res = ctx.make_bubbles(params, lens, None, aln_off, ex.trg_start, ex.trg_end, scal.err_rate, ex.col_off, ex.trg_cols, ex.qry_cols,
                               profile)
        return res, k

    fused_cons = lambda profile=False: (ctx.contig_consensus_cigars(qry_id=qry_id, use=use, want_profile=profile, **rec_args), {})
    fused_bub = lambda profile=False: (ctx.make_bubbles_cigars(params, contig_circular=None, err_rate=scal.err_rate, want_profile=profile,
                                                               **rec_args), {})

    # the check, which is the warm-up of all four as well
    assert same(fused_cons(True)[0], two_step_cons(True)[0]), "fg_contig_consensus_cigars differs from the two-step path"
    assert same(fused_bub(True)[0], two_step_bub(True)[0]), "fg_make_bubbles_cigars differs from the two-step path"
    print("check: %d columns, %d of %d alignments in use; both fused calls identical to the two-step path, profiles included" %
          (n_cols, int(use.sum()), n), flush=True)
    out = dict(length=a.length, alignments=n, runs=int(len(ex_args["run_len"])), columns=n_cols, repeat=a.repeat,
               column_bytes_down_and_up_two_step=4 * n_cols, stages={})
    for stage, paths in (("contig_consensus", (("two_step", two_step_cons), ("fused", fused_cons))),
                         ("make_bubbles", (("two_step", two_step_bub), ("fused", fused_bub)))):
        out["stages"][stage] = {}
        for label, fn in paths:
            fn()                                                       # one warm-up
            walls = []
            for _ in range(a.repeat):
                t0 = time.perf_counter()
                _, expand_kernels = fn()
                walls.append(time.perf_counter() - t0)
            k = dict(expand_kernels, **kernels(ctx)) if label == "two_step" else kernels(ctx)
            out["stages"][stage][label] = dict(best_s=round(min(walls), 5), median_s=round(statistics.median(walls), 5),
                                               kernel_ms_total=round(sum(v["ms"] for v in k.values()), 3), kernels=k)
            print("%-17s %-8s best %.4f s, median %.4f s, kernels %.2f ms" %
                  (stage, label, min(walls), statistics.median(walls), sum(v["ms"] for v in k.values())), flush=True)
            for name, v in k.items():
                print("   %-15s %9.3f ms in %3d launches" % (name, v["ms"], v["launches"]))
        s = out["stages"][stage]
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
