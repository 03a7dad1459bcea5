"""Time of fg_chain_alignments (the edge-chain step of ReadAligner::alignReads) on a seeded batch of per-read record
lists at alignReads-like sizes, beside the literal host form of the step (tests/native/read_chain_driver.cpp) on 1 and
on 16 threads.

A read walks along a path of consecutive graph edges (edge e runs from node e to node e + 1, lengths 300 - 5000): one
alignment per edge of the walk with a few bases of jitter, so that neighbours chain, plus one noise alignment in five
at a random place of a random edge (repeat copies).  The reference's parameters: maximum_jump 1500, max_separation 500,
minimum overlap 1000.

  python tools/read_chain_bench.py [reads=50000] [mean alignments per read=24]

Prints the device call's wall time (best of three after a warm-up: table up, chains back), the kernel split from
fg_kernel_times, the host form's best wall time of three on 1 and on 16 threads (its chaining only, no file I/O), and
one JSON line.  The three results are compared before anything is printed."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from flye_amd import gpu
import read_chain_restate as R

N_READS = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
MEAN_ALNS = int(sys.argv[2]) if len(sys.argv) > 2 else 24
N_EDGES, RUNS = 4096, 3
PARAMS = dict(max_jump=1500, max_read_overlap=50, min_alignment=1000, max_separation=500, long_edge=900, big_alignment=500)


def make_batch(seed=20261):
    rng = np.random.default_rng(seed)
    edge_len = rng.integers(300, 5000, N_EDGES)
    n = rng.poisson(MEAN_ALNS, N_READS) + 1
    off = np.zeros(N_READS + 1, np.int64)
    off[1:] = np.cumsum(n)
    total = int(off[-1])
    read = np.repeat(np.arange(N_READS), n)
    j = np.arange(total) - off[read]
    edge = (rng.integers(0, N_EDGES, N_READS)[read] + j) % N_EDGES
    el = edge_len[edge]
    # position of the walk's j-th edge on the read: the lengths of the edges before it
    csum = np.concatenate([[0], np.cumsum(el)])
    start = csum[:-1] - csum[off[read]]
    jit = rng.integers(-20, 21, (2, total))
    cb = np.maximum(start + jit[0], 0)
    eb = rng.integers(0, 30, total)
    ee = el - rng.integers(0, 30, total)
    ce = cb + (ee - eb) + jit[1]
    noise = rng.random(total) < 0.2
    nl = int(noise.sum())
    edge[noise] = rng.integers(0, N_EDGES, nl)
    el = edge_len[edge]
    span = np.minimum(rng.integers(100, 2000, nl), el[noise])
    eb[noise] = rng.integers(0, el[noise] - span + 1)
    ee[noise] = eb[noise] + span
    ee = np.minimum(ee, el)
    ce[noise] = cb[noise] + span + rng.integers(-20, 21, nl)
    ce = np.maximum(ce, cb)
    score = np.maximum((ce - cb) // 10, 1)
    ext_id = 2 * edge                      # forward strands; the node tables list both
    order = rng.permutation(total)         # records arrive in any order inside a read
    order = order[np.argsort(read[order], kind="stable")]
    tab = np.stack([cb, ce, eb, ee, el, score, ext_id], 1)[order]
    queries = [tab[off[i]:off[i + 1]].tolist() for i in range(N_READS)]
    node_left = np.zeros(2 * N_EDGES, np.uint32)
    node_right = np.zeros(2 * N_EDGES, np.uint32)
    node_left[0::2], node_right[0::2] = np.arange(N_EDGES), np.arange(N_EDGES) + 1
    node_left[1::2], node_right[1::2] = np.arange(N_EDGES) + 1 + N_EDGES + 1, np.arange(N_EDGES) + N_EDGES + 1
    return R.Batch(queries, node_left, node_right, 0, PARAMS)


def main():
    b = make_batch()
    recs = b.recs()
    ctx = gpu.Context(17, 0)
    p = gpu.ChainParams(**b.params)
    args = (recs, b.query_off, p, b.first_ext_id, b.node_left, b.node_right)
    ctx.chain_alignments(*args)
    secs = []
    for _ in range(RUNS):
        got = ctx.chain_alignments(*args)
        secs.append(ctx.last_chain_seconds)
    kt = ctx.kernel_times()
    one = R.run_native(b, threads=1, repeats=RUNS)
    many = R.run_native(b, threads=16, repeats=RUNS)
    same = R.same(got, one) and R.same(got, many)
    depth = np.diff(got[1].astype(np.int64))
    print(f"{N_READS} reads, {len(recs)} records, {len(depth)} chains, mean depth {depth.mean():.2f}, deepest {int(depth.max())}; "
          f"cleanups {one[4]['cleanups']}, tied sorts above 16: {one[4]['tied_first']} + {one[4]['tied_second']}")
    print(f"  device call: {' '.join(f'{s * 1e3:.1f}' for s in secs)} ms; kernels of the last call (ms, launches): " +
          ", ".join(f"{k} {v[0] * 1e3:.2f} ({v[1]})" for k, v in kt.items()) + f"; sum {sum(v[0] for v in kt.values()) * 1e3:.2f} ms")
    print(f"  host form: {one[5] * 1e3:.1f} ms on 1 thread, {many[5] * 1e3:.1f} ms on 16; all three results equal: {same}")
    print(json.dumps(dict(reads=N_READS, records=len(recs), chains=len(depth), device_call_ms=[round(s * 1e3, 3) for s in secs],
                          kernel_ms={k: round(v[0] * 1e3, 3) for k, v in kt.items()}, host_1_thread_ms=round(one[5] * 1e3, 3),
                          host_16_threads_ms=round(many[5] * 1e3, 3), equal=same)))
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
