#!/usr/bin/env python3
"""How many lookup-table misses of one overlap pass the build's frequency bit covers, on the host.

Counts, for a raw-read workload queried against its own index (every read once, forward strand):
  positions   forward k-mer positions (sum of max(len - k, 0));
  misses      those whose canonical k-mer has no slot in the lookup table (neither a kept nor a repetitive key);
  rare        the misses whose canonical k-mer occurs fewer than minFreq times in the whole read set.
The index comes from the CPU oracle, the k-mers and their counts from numpy: no device is used.

    python tools/probe_skip_coverage.py [--scale 1.0] [--seed 12345]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def canonical_kmers(rs, k: int) -> np.ndarray:
    """canonical k-mer (Kmer repr: first base most significant, kmer.h:32-52) of every forward position p < len - k
    of every read, read after read"""
    out = []
    sh = np.arange(32, dtype=np.uint64) * np.uint64(2)
    mask = np.uint64((1 << (2 * k)) - 1)
    for i in range(rs.n):
        n = int(rs.length[i])
        nk = n - k
        if nk <= 0:
            continue
        w = rs.words[int(rs.word_off[i]):int(rs.word_off[i + 1])]
        b = ((w[:, None] >> sh[None, :]) & np.uint64(3)).reshape(-1)[:n]
        fw = np.zeros(nk, np.uint64)
        rv = np.zeros(nk, np.uint64)
        for j in range(k):
            x = b[j:j + nk]
            fw |= x << np.uint64(2 * (k - 1 - j))
            rv |= (np.uint64(3) - x) << np.uint64(2 * j)
        out.append(np.minimum(fw, rv & mask))
    return np.concatenate(out) if out else np.zeros(0, np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=12345)
    a = ap.parse_args()
    from flye_amd import config, workloads
    from oracle import oracle as O
    rs, _, preset = workloads.ecoli_pb50(seed=a.seed, scale=a.scale)
    cfg = config.preset(preset)
    k = int(cfg["kmer_size"])
    min_freq = 2        # what VertexIndex.build passes for solid k-mers (main_assemble.cpp:195-223)
    o = O.Oracle(k)
    o.set_reads(rs)
    o.build_index(cfg)
    ex = o.export_index()
    table = np.union1d(ex.keys.astype(np.uint64), ex.repetitive.astype(np.uint64))
    km = canonical_kmers(rs, k)
    uniq, inv, cnt = np.unique(km, return_inverse=True, return_counts=True)
    in_table = np.isin(uniq, table, assume_unique=True)
    miss = ~in_table[inv]
    rare = miss & (cnt[inv] < min_freq)
    # the invariant the probe skip rests on: a k-mer below minFreq has no slot
    assert not np.any(in_table & (cnt < min_freq))
    print(json.dumps({"reads": rs.n, "bases": int(rs.total_bases), "k": k, "min_freq": min_freq,
                      "positions": int(len(km)), "misses": int(miss.sum()), "rare_misses": int(rare.sum()),
                      "table_keys": int(len(table)),
                      "miss_share": round(float(miss.mean()), 4),
                      "rare_share_of_misses": round(float(rare.sum() / max(1, miss.sum())), 4)}))


if __name__ == "__main__":
    main()
