"""fg_divergence_profile on one seeded synthetic contig: 200 kb, 2000 alignments of 10 kb (100x) with 12 % errors.  Checks
the call against the restatement (tests/divergence_restate.py) on the alignments that lie inside the first fortieth of the
contig, then prints the device call's wall time and the device time per kernel.  There is no pass bar.
    python tools/divergence_bench.py [--length 200000] [--alignments 2000] [--read 10000] [--seed 2024] [--repeat 3]
The reference's own time on this input: python tests/golden/make_divergence_golden.py --time"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import bubbles_restate as R  # noqa: E402
import divergence_restate as DR  # noqa: E402

THRESHOLDS = (0.1, 0.2, 0.3)


def fast_aln(rng, cid, seq, start, n_trg, qid, rate=0.04):
    """n_trg target bases from start: substitutions, deletions and single inserted bases at `rate` each, drawn at once"""
    base = seq[start:start + n_trg]
    r = rng.random(n_trg)
    q = base.copy()
    sub = r < rate
    q[sub] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(sub.sum()))]
    q[(r >= rate) & (r < 2 * rate)] = 45
    behind = np.flatnonzero(rng.random(n_trg) < rate) + 1
    t = np.insert(base, behind, 45)
    q = np.insert(q, behind, np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, len(behind))])
    return R.Aln(qid, cid, 0, 0, "+", 0, start, start + n_trg, "+", len(seq), q.tobytes().decode(), t.tobytes().decode(),
                 float(rng.uniform(0.08, 0.16)), False)


def bench_input(length=200000, alignments=2000, read=10000, seed=2024):
    rng = np.random.default_rng(seed)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, length)]
    contig = R.Contig("contig_1", length, "linear")
    lst = [fast_aln(rng, contig.id, seq, int(rng.integers(0, length - read + 1)), read, "read_%d" % k) for k in range(alignments)]
    lst.sort(key=lambda a: a.trg_start)
    return dict(thresholds=THRESHOLDS, contigs=[(contig, seq.tobytes().decode())], alns={contig.id: lst})


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
    run = bench_input(a.length, a.alignments, a.read, a.seed)
    (contig, _), = run["contigs"]
    alns = run["alns"][contig.id]
    print("contig of %d bp, %d alignments, %d columns, generated in %.1f s" %
          (contig.length, len(alns), sum(len(x.trg_seq) for x in alns), time.perf_counter() - t0), flush=True)
    ctx = gpu.Context(17, 0)
    finder = gpu.DivergenceFinder(ctx)
    # a check at small size: the alignments that start inside the first fortieth, on a contig that holds them
    small = R.Contig("contig_1", contig.length // 40 + a.read, "linear")
    inside = [x for x in alns if x.trg_start < contig.length // 40]
    want = DR.divergence(inside, small.length, THRESHOLDS)
    got = finder.profile({small.id: inside}, [small], *THRESHOLDS)
    assert inside and all(np.array_equal(getattr(got, k), want[k]) for k in DR.VALUE_KEYS)
    assert got.positions(0) == {k: want[k] for k in DR.LIST_KEYS}
    print("check: %d alignments on %d bp, %d positions called, every array identical to the restatement" %
          (len(inside), small.length, len(want["total"])), flush=True)
    lengths, aln_off = [contig.length], [0, len(alns)]
    starts = [x.trg_start for x in alns]
    col_off = np.cumsum([0] + [len(x.trg_seq) for x in alns])
    trg, qry = "".join(x.trg_seq for x in alns).encode("latin-1"), "".join(x.qry_seq for x in alns).encode("latin-1")
    for rep in range(a.repeat):
        t0 = time.perf_counter()
        res = ctx.divergence_profile(*THRESHOLDS, lengths, aln_off, starts, col_off, trg, qry, want_profile=True)
        wall = time.perf_counter() - t0
        times = ctx.kernel_times()
        print("run %d: %d positions called (sub %d, del %d, ins %d); device call %.3f s (with the copy out of the arena %.3f s)" %
              (rep, len(res.total_pos), len(res.sub_pos), len(res.del_pos), len(res.ins_pos), ctx.last_divergence_seconds, wall), flush=True)
        ksum = sum(v[0] for v in times.values())
        for name, (sec, launches) in times.items():
            print("   %-15s %9.3f ms in %3d launches" % (name, sec * 1e3, launches))
        print("   kernels %.4f s, host and copies %.4f s" % (ksum, ctx.last_divergence_seconds - ksum), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
