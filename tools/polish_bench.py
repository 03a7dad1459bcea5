"""fg_polish_bubbles on seeded bubbles of the kind Flye's polisher sees (candidates of 50 - 100 bp, 2 - 50 branches, 15 %
divergence from a common truth): checks the first bubbles against the numpy restatement, then prints the device call's
wall time, the kernel split and bubbles per second.  There is no pass bar.
    python tools/polish_bench.py [--bubbles 20000] [--check 200] [--seed 2024] [--repeat 2]
The reference's own time on the first 2000 of these bubbles: python tests/golden/make_polish_golden.py --time"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import polish_restate as R  # noqa: E402
from flye_amd import gpu  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bubbles", type=int, default=20000)
    ap.add_argument("--check", type=int, default=200)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--repeat", type=int, default=2)
    a = ap.parse_args()
    path = os.path.join(ROOT, "tests", "golden", "bin_cfg", "pacbio_substitutions.mat")
    matrix = gpu.SubstitutionMatrix(path)
    t0 = time.perf_counter()
    bubbles = R.generate_fast(a.seed, a.bubbles)
    n_br = sum(len(b.branches) for b in bubbles)
    print("%d bubbles, %d branches, %d candidate bases, generated in %.1f s" %
          (len(bubbles), n_br, sum(len(b.cand) for b in bubbles), time.perf_counter() - t0), flush=True)
    ctx = gpu.Context(17, 0)
    if a.check:
        head = bubbles[:a.check]
        s = R.load_matrix(path)
        t0 = time.perf_counter()
        want = [R.polish_bubble(b.cand, b.branches, s) for b in head]
        t1 = time.perf_counter()
        res = ctx.polish_bubbles(matrix, *R.flatten(head))
        for i, (cand, steps, status) in enumerate(want):
            assert res.candidates[i].decode() == cand and int(res.status[i]) == status, i
            assert [(q.decode(), sc) for q, sc in res.steps[i]] == steps, i
        print("check: %d bubbles, %d steps identical to the restatement (numpy: %.1f s, device call: %.3f s)" %
              (len(head), sum(len(w[1]) for w in want), t1 - t0, ctx.last_polish_seconds), flush=True)
    flat = R.flatten(bubbles)
    for rep in range(a.repeat):
        res = ctx.polish_bubbles(matrix, *flat, want_steps=False)
        dt = ctx.last_polish_seconds
        times = ctx.kernel_times()
        print("run %d: %d bubbles in %.3f s = %.0f bubbles/s; %d steps, %d changed by the fixer, %d at the iteration limit" %
              (rep, len(bubbles), dt, len(bubbles) / dt, int(res.n_steps.sum()), int(((res.status & 8) != 0).sum()),
               int(((res.status & 4) != 0).sum())), flush=True)
        ksum = sum(v[0] for v in times.values())
        for name, (sec, launches) in times.items():
            print("   %-14s %9.3f ms in %5d launches" % (name, sec * 1e3, launches))
        print("   kernels %.3f s, host and copies %.3f s" % (ksum, dt - ksum), flush=True)
    now, peak = gpu.memory_stats() if hasattr(gpu, "memory_stats") else (0, 0)
    if peak:
        print("device memory: %.1f MiB now, %.1f MiB at most" % (now / 2 ** 20, peak / 2 ** 20))
    ctx.close()


if __name__ == "__main__":
    main()
