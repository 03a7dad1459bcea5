"""fg_classify_reads on one seeded synthetic job: two edges with consensuses of 200 kb, 2000 alignments of 10 kb (1000 reads,
one alignment on each edge) with 12 % errors, 2000 confirmed positions per edge.  Checks the call against the restatement
(tests/partition_restate.py) on the first reads, then prints the device call's wall time and the device time per kernel.
There is no pass bar.
    python tools/partition_bench.py [--length 200000] [--alignments 2000] [--read 10000] [--positions 2000] [--seed 2025] [--repeat 3]
The reference's own time on this input: python tests/golden/make_partition_golden.py --time"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import partition_restate as P  # noqa: E402
from divergence_bench import fast_aln  # noqa: E402

BUFFER_COUNT = 3


def bench_input(length=200000, alignments=2000, read=10000, positions=2000, seed=2025):
    """one classify job (tests/partition_restate.py): read k has alignment k of each edge"""
    rng = np.random.default_rng(seed)
    edges = []
    for e in range(2):
        seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, length)]
        alns = [fast_aln(rng, "edge_%d" % e, seq, int(rng.integers(0, length - read + 1)), read, "read_%d" % k) for k in range(alignments // 2)]
        edges.append(dict(pos=[int(x) for x in rng.integers(0, length, positions)], alns=alns))
    return dict(buffer_count=BUFFER_COUNT, jobs=[dict(n_reads=alignments // 2, edges=edges)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=200000)
    ap.add_argument("--alignments", type=int, default=2000)
    ap.add_argument("--read", type=int, default=10000)
    ap.add_argument("--positions", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=2025)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    from flye_amd import gpu
    t0 = time.perf_counter()
    run = bench_input(a.length, a.alignments, a.read, a.positions, a.seed)
    job, = run["jobs"]
    print("2 edges of %d bp, %d alignments, %d columns, %d positions, generated in %.1f s" %
          (a.length, sum(len(e["alns"]) for e in job["edges"]), sum(len(x.trg_seq) for e in job["edges"] for x in e["alns"]),
           sum(len(e["pos"]) for e in job["edges"]), time.perf_counter() - t0), flush=True)
    ctx = gpu.Context(17, 0)
    # a check at small size: the first 50 reads
    small = dict(n_reads=50, edges=[dict(pos=e["pos"], alns=e["alns"][:50]) for e in job["edges"]])
    want = P.classify(small, BUFFER_COUNT)
    got = ctx.classify_reads(BUFFER_COUNT, want_scores=True, **P.classify_arrays([small]))
    assert all(np.array_equal(getattr(got, k), want[k]) for k in P.READ_KEYS + ("aln_score", "aln_counted"))
    print("check: 50 reads, %d alignments, status counts %s, every array identical to the restatement" %
          (len(want["aln_score"]), np.bincount(want["status"], minlength=3).tolist()), flush=True)
    arrays = P.classify_arrays([job])
    for rep in range(a.repeat):
        t0 = time.perf_counter()
        res = ctx.classify_reads(BUFFER_COUNT, **arrays)
        wall = time.perf_counter() - t0
        times = ctx.kernel_times()
        print("run %d: None / Tied / Partitioned %s; device call %.3f s (with the copy out of the arena %.3f s)" %
              (rep, np.bincount(res.status, minlength=3).tolist(), ctx.last_classify_seconds, wall), flush=True)
        ksum = sum(v[0] for v in times.values())
        for name, (sec, launches) in times.items():
            print("   %-15s %9.3f ms in %3d launches" % (name, sec * 1e3, launches))
        print("   kernels %.4f s, host and copies %.4f s" % (ksum, ctx.last_classify_seconds - ksum), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
