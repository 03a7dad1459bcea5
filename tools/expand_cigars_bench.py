"""fg_expand_cigars on one seeded synthetic contig: 200 kb, 2000 alignments of 10 kb with ~12 % errors (4 % each of
substitutions, insertions and deletions, so runs of a few columns).  Checks the call against the restatement
(tests/cigar_restate.py) on the first alignments, then prints the device call's wall time and the device time per kernel,
for want_cols 0 and 1.  There is no pass bar.
    python tools/expand_cigars_bench.py [--length 200000] [--alignments 2000] [--read 10000] [--seed 2024] [--repeat 3]
The reference's own time on this input: python tests/golden/make_cigar_golden.py --time"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import cigar_restate as G  # noqa: E402


def bench_input(length=200000, alignments=2000, read=10000, seed=2024, rate=0.04):
    """-> (run without SAM text, records in the form of cigar_restate.records)"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    contig = acgt[rng.integers(0, 4, length)]
    recs = []
    for k in range(alignments):
        start = int(rng.integers(0, length - read + 1))
        # per column: 0 match or substitution, 1 insertion, 2 deletion, until `read` contig bases are consumed
        kind = rng.choice(3, size=read + read // 4, p=[1 - 2 * rate, rate, rate]).astype(np.uint8)
        used = np.cumsum(kind != 1)
        kind = kind[:int(np.searchsorted(used, read)) + 1]
        edge = np.flatnonzero(np.diff(kind)) + 1
        first = np.concatenate([[0], edge])
        lens = np.diff(np.concatenate([first, [len(kind)]]))
        ops = np.frombuffer(b"MID", np.uint8)[kind[first]]
        trg_at = start + np.cumsum(kind != 1) - (kind != 1)
        bases = contig[np.minimum(trg_at, length - 1)].copy()
        change = rng.random(len(kind)) < rate
        bases[change | (kind == 1)] = acgt[rng.integers(0, 4, int((change | (kind == 1)).sum()))]
        recs.append(dict(qry_id="read_%d" % k, contig=b"contig_1", flags=0, pos=start + 1,
                         runs=list(zip(ops.tolist(), lens.tolist())), seq=bases[kind != 2].tobytes()))
    run = dict(contigs={"contig_1": contig.tobytes().decode()}, max_coverage=None, use_secondary=True)
    return run, recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=200000)
    ap.add_argument("--alignments", type=int, default=2000)
    ap.add_argument("--read", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    from flye_amd import gpu
    t0 = time.perf_counter()
    run, recs = bench_input(a.length, a.alignments, a.read, a.seed)
    args = G.call_arrays(recs, run["contigs"])
    print("contig of %d bp, %d alignments, %d runs, generated in %.1f s" %
          (a.length, len(recs), len(args["run_len"]), time.perf_counter() - t0), flush=True)
    ctx = gpu.Context(17, 0)
    # a check at small size: the first alignments against the restatement
    few = recs[:8]
    want, got = G.expand(few, run["contigs"]), ctx.expand_cigars(**G.call_arrays(few, run["contigs"]))
    assert all(np.array_equal(getattr(got, k), v) for k, v in want.items())
    print("check: %d alignments, %d columns identical to the restatement, mean err_rate %.4f" %
          (len(few), int(want["col_off"][-1]), float(want["err_rate"].mean())), flush=True)
    for want_cols in (0, 1):
        for rep in range(a.repeat):
            res = ctx.expand_cigars(want_cols=want_cols, **args)
            times = ctx.kernel_times()
            ksum = sum(v[0] for v in times.values())
            print("want_cols %d run %d: %d columns, call %.4f s, kernels %.4f s, host and copies %.4f s" %
                  (want_cols, rep, int(res.col_off[-1]), ctx.last_expand_seconds, ksum, ctx.last_expand_seconds - ksum), flush=True)
            for name, (sec, launches) in times.items():
                print("   %-15s %9.3f ms in %3d launches" % (name, sec * 1e3, launches))
    ctx.close()


if __name__ == "__main__":
    main()
