"""fg_make_bubbles on one seeded synthetic contig: 100 kb, 500 alignments of 10 kb (50x) with 12 % errors, the pacbio
parameters.  Checks the call against the restatement (tests/bubbles_restate.py) on the alignments that lie inside the
first three tenths of the contig, then prints the device call's wall time and the device time per kernel.  There is no pass bar.
    python tools/bubbles_bench.py [--length 100000] [--alignments 500] [--read 10000] [--seed 2024] [--repeat 2]
The reference's own time on this input: python tests/golden/make_bubbles_golden.py --time"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import bubbles_restate as R  # noqa: E402


def bench_input(length=100000, alignments=500, read=10000, seed=2024):
    rng = np.random.default_rng(seed)
    seq = R.rand_seq(rng, length)
    contig = R.Contig("contig_1", length, "linear")
    lst = []
    for k in range(alignments):
        start = int(rng.integers(0, length - read + 1))
        lst.append(R.gen_aln(rng, contig.id, seq, start, read, 0.04, 0.04, 0.04, "read_%d" % k, err_rate=0.12))
    lst.sort(key=lambda a: a.trg_start)
    return dict(err_mode="pacbio", overrides={}, uniform=False, contigs=[(contig, seq)], alns={contig.id: lst})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=100000)
    ap.add_argument("--alignments", type=int, default=500)
    ap.add_argument("--read", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--repeat", type=int, default=2)
    a = ap.parse_args()
    from flye_amd import gpu
    t0 = time.perf_counter()
    run = bench_input(a.length, a.alignments, a.read, a.seed)
    (contig, _), = run["contigs"]
    alns = run["alns"][contig.id]
    print("contig of %d bp, %d alignments, %d columns, generated in %.1f s" %
          (contig.length, len(alns), sum(len(x.trg_seq) for x in alns), time.perf_counter() - t0), flush=True)
    ctx = gpu.Context(17, 0)
    maker = gpu.BubbleMaker(ctx)
    # a check at small size: the alignments that lie inside the first three tenths, against the restatement
    small = R.Contig("contig_1", 3 * contig.length // 10, "linear")
    inside = [x for x in alns if x.trg_start + a.read <= small.length]
    want = R.make_contig(small, inside, R.params_for("pacbio"))
    got, _, _ = maker.make([small], {small.id: inside}, "pacbio")
    assert inside and got
    assert [(p, c.decode("latin-1"), [w.decode("latin-1") for w in ws]) for _, p, c, ws in got] == want["bubbles"]
    print("check: %d alignments on %d bp, %d bubbles identical to the restatement" % (len(inside), small.length, len(got)), flush=True)
    for rep in range(a.repeat):
        t0 = time.perf_counter()
        bubbles, cov, err = maker.make([contig], run["alns"], "pacbio")
        wall = time.perf_counter() - t0
        times = ctx.kernel_times()
        print("run %d: %d bubbles, %d branches, mean coverage %d; call %.3f s (with the Python mirror %.3f s)" %
              (rep, len(bubbles), sum(len(b[3]) for b in bubbles), cov[contig.id], ctx.last_bubbles_seconds, wall), flush=True)
        ksum = sum(v[0] for v in times.values())
        for name, (sec, launches) in times.items():
            print("   %-15s %9.3f ms in %3d launches" % (name, sec * 1e3, launches))
        print("   kernels %.3f s, host and copies %.3f s" % (ksum, ctx.last_bubbles_seconds - ksum), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
