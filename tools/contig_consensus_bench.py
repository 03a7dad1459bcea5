"""fg_uniform_alignments + fg_contig_consensus on one seeded synthetic contig: 100 kb, 500 alignments of 10 kb (50x) with
12 % errors.  Checks the two calls against the restatement (tests/contig_consensus_restate.py) on the alignments that lie
inside the first three tenths of the contig, then prints the device calls' wall time and the device time per kernel.
There is no pass bar.
    python tools/contig_consensus_bench.py [--length 100000] [--alignments 500] [--read 10000] [--seed 2024] [--repeat 2]
The reference's own time on this input: python tests/golden/make_contig_consensus_golden.py --time"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import bubbles_restate as R  # noqa: E402
import contig_consensus_restate as CR  # noqa: E402


def bench_input(length=100000, alignments=500, read=10000, seed=2024):
    rng = np.random.default_rng(seed)
    seq = R.rand_seq(rng, length)
    contig = R.Contig("contig_1", length, "linear")
    lst = []
    for k in range(alignments):
        start = int(rng.integers(0, length - read + 1))
        lst.append(R.gen_aln(rng, contig.id, seq, start, read, 0.04, 0.04, 0.04, "read_%d" % k, err_rate=float(rng.uniform(0.08, 0.16)),
                             secondary=bool(k % 9 == 4)))
    lst.sort(key=lambda a: a.trg_start)
    return dict(err_mode="pacbio", overrides={}, uniform=True, contigs=[(contig, seq)], alns={contig.id: lst})


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
    cc = gpu.ContigConsensus(ctx)
    # a check at small size: the alignments that lie inside the first three tenths, against the restatement
    small = R.Contig("contig_1", 3 * contig.length // 10, "linear")
    inside = [x for x in alns if x.trg_start + a.read <= small.length]
    uni = CR.uniform(inside, small.length)
    want = CR.consensus(inside, CR.number_reads(inside), uni["keep"], small.length)
    got, _ = cc.consensus([small], {small.id: inside})
    assert inside and list(cc.uniform.keep) == uni["keep"] and int(cc.uniform.cov_threshold[0]) == uni["cov_threshold"]
    assert got[small.id].encode("latin-1") == want["seq"]
    print("check: %d alignments on %d bp, %d kept, %d bases identical to the restatement" %
          (len(inside), small.length, sum(uni["keep"]), len(want["seq"])), flush=True)
    for rep in range(a.repeat):
        t0 = time.perf_counter()
        seqs, err = cc.consensus([contig], run["alns"])
        wall = time.perf_counter() - t0
        times = ctx.kernel_times()           # of the consensus call; the uniform call's were replaced by it
        print("run %d: %d of %d alignments kept, %d bases; uniform call %.4f s, consensus call %.3f s (with the Python mirror %.3f s)" %
              (rep, int(cc.uniform.keep.sum()), len(alns), len(seqs.get(contig.id, "")), ctx.last_uniform_seconds,
               ctx.last_consensus_seconds, wall), flush=True)
        ksum = sum(v[0] for v in times.values())
        for name, (sec, launches) in times.items():
            print("   %-15s %9.3f ms in %3d launches" % (name, sec * 1e3, launches))
        print("   consensus kernels %.4f s, host and copies %.4f s" % (ksum, ctx.last_consensus_seconds - ksum), flush=True)
        ar = dict(contig_len=[contig.length], contig_aln_off=[0, len(alns)], trg_start=[x.trg_start for x in alns],
                  trg_end=[x.trg_end for x in alns], err_rate=[x.err_rate for x in alns], is_secondary=[x.is_secondary for x in alns])
        ctx.uniform_alignments(**ar)
        times = ctx.kernel_times()
        print("   uniform kernels %.4f s of %.4f s: %s" % (sum(v[0] for v in times.values()), ctx.last_uniform_seconds,
                                                            ", ".join("%s %.3f ms" % (k, v[0] * 1e3) for k, v in times.items())), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
