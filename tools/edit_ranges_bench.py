"""Throughput of fg_edit_ranges (getAlignmentErrEdlib for ranges of the resident sequences) on seeded synthetic pairs,
two mixes of 20 000 pairs each:

  hifi   15 kb ranges, 0.5 % errors, homopolymer compression on
  raw    10 kb ranges, 12 % errors, compression off

As in ReadAligner, the cur side is a range of a read in the fg_set_queries container and the ext side a range of an
"edge" in the indexed one: 256 random sequences of 40 kb are the edges, a copy of each with sub / ins / del errors at
the mix's rate is the read, and a pair is a random window of a read against the window of its edge that the copy's
coordinate map gives.  Everything is resident before the clock starts; the call moves 32 B per pair up and 12 B down.

Prints pairs/s and compared bases/s (sum of max(len_cur, len_ext)) of the C call, and the kernel split from
fg_kernel_times.  Where oracle/_ref/ref_dumper exists, also the rate of its --edlib-pairs mode on a 500-pair sample at
one thread -- a figure that INCLUDES that program's reading and parsing of the strings as text (and excludes the
homopolymer compression, done here before the strings are written)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from flye_amd import gpu, synth
from oracle import oracle as O

N_PAIRS = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
N_TEMPLATES, TEMPLATE_LEN, REF_SAMPLE, RUNS = 256, 40000, 500, 3
MIXES = [("hifi", 15000, 0.005, True), ("raw", 10000, 0.12, False)]


def mutate(rng, a, err):
    """A copy of `a` with substitutions, insertions and deletions at rate err / 3 each, and for every position of `a`
    the position of the copy it went to (len(a) + 1 entries)."""
    n = len(a)
    u = rng.random(n)
    sub, ins, dele = u < err / 3, (u >= err / 3) & (u < 2 * err / 3), (u >= 2 * err / 3) & (u < err)
    b = a.copy()
    b[sub] = (a[sub] + 1 + rng.integers(0, 3, size=int(sub.sum()), dtype=np.uint8)) & 3
    cnt = np.ones(n, np.int64)
    cnt[ins] = 2
    cnt[dele] = 0
    pos = np.zeros(n + 1, np.int64)
    pos[1:] = np.cumsum(cnt)
    out = np.repeat(b, cnt)
    out[pos[:-1][ins] + 1] = rng.integers(0, 4, size=int(ins.sum()), dtype=np.uint8)
    return out, pos


def hpc(x):
    keep = np.ones(len(x), bool)
    keep[1:] = x[1:] != x[:-1]
    return x[keep]


def main():
    out = {}
    for name, length, err, use_hpc in MIXES:
        rng = np.random.default_rng(218247 + length)
        edges = [rng.integers(0, 4, size=TEMPLATE_LEN, dtype=np.uint8) for _ in range(N_TEMPLATES)]
        made = [mutate(rng, e, err) for e in edges]
        reads, maps = [m[0] for m in made], [m[1] for m in made]
        ctx = gpu.Context(17, 0)
        ctx.set_reads(synth.ReadSet.from_arrays(edges), 0)
        first_q = 2 * N_TEMPLATES
        ctx.set_queries(synth.ReadSet.from_arrays(reads), first_q)
        t = rng.integers(0, N_TEMPLATES, size=N_PAIRS)
        eb = rng.integers(0, TEMPLATE_LEN - length, size=N_PAIRS)
        pairs = np.array([(first_q + 2 * ti, 2 * ti, maps[ti][b], maps[ti][b + length], b, b + length)
                          for ti, b in zip(t, eb)], np.int64)
        ctx.edit_ranges(pairs[:64], use_hpc=use_hpc)
        secs = []
        for _ in range(RUNS):
            dist, len_cur, len_ext, div = ctx.edit_ranges(pairs, use_hpc=use_hpc)
            secs.append(ctx.last_edit_seconds)
        kt = ctx.kernel_times()
        bases = int(np.maximum(len_cur, len_ext).astype(np.int64).sum())
        best = min(secs)
        dev = sum(v[0] for v in kt.values())
        print(f"{name}: {N_PAIRS} pairs of {length} bases, {err * 100:g} % errors, HPC {'on' if use_hpc else 'off'}; "
              f"mean distance {dist.mean():.1f}, mean divergence {np.nanmean(div):.5f}")
        print(f"  call: {' '.join(f'{s * 1e3:.1f}' for s in secs)} ms -> best {N_PAIRS / best:.0f} pairs/s, "
              f"{bases / best / 1e9:.3f} G compared bases/s")
        print("  kernels of the last call (ms, launches): " +
              ", ".join(f"{k} {v[0] * 1e3:.2f} ({v[1]})" for k, v in kt.items()) + f"; sum {dev * 1e3:.2f} ms")
        res = dict(pairs=N_PAIRS, length=length, err=err, use_hpc=use_hpc, call_ms=[round(s * 1e3, 3) for s in secs],
                   pairs_per_s=round(N_PAIRS / best), compared_bases_per_s=round(bases / best),
                   kernel_ms={k: round(v[0] * 1e3, 3) for k, v in kt.items()})
        if O.have_ref():
            n = min(REF_SAMPLE, N_PAIRS)
            strings = []
            for (cid, eid, cb, ce, b0, b1) in pairs[:n]:
                a, b = reads[(cid - first_q) >> 1][cb:ce], edges[eid >> 1][b0:b1]
                strings.append((hpc(a), hpc(b)) if use_hpc else (a, b))
            t0 = time.perf_counter()
            ref = O.ref_edlib_distances(strings)
            dr = time.perf_counter() - t0
            rb = sum(max(len(a), len(b)) for a, b in strings)
            print(f"  reference edlib, one thread, {n} pairs (includes writing, reading and parsing the strings as text): "
                  f"{n / dr:.0f} pairs/s, {rb / dr / 1e9:.4f} G compared bases/s; distances equal the device's: "
                  f"{ref == dist[:n].tolist()}")
            res.update(ref_pairs_per_s=round(n / dr), ref_compared_bases_per_s=round(rb / dr),
                       ref_equal=ref == dist[:n].tolist())
        out[name] = res
        ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
