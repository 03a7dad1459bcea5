"""Time of fg_read_coverage (ChimeraDetector's window coverage and verdict) on the bench workload's own overlap records:
the E. coli PacBio 50x read set of bench.py, one fg_overlaps pass over all forward reads, then the coverage of every
read from those records -- with and without the vectors -- beside the literal host form of the step
(tests/native/coverage_driver.cpp) on 1 and on 16 threads and beside the upload of the record table alone.

  python tools/coverage_bench.py [scale=1.0]

Prints the device call's wall time (best of three after a warm-up: records up, values and vectors back), the kernel
split from fg_kernel_times, the host form's best wall time of three (its computation only, no file I/O), the time of a
plain host-to-device copy of the record table, and one JSON line.  The results are compared before anything is
printed."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from flye_amd import config, gpu, workloads
import coverage_restate as R

SCALE = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
RUNS = 3


def main():
    rs, _, preset = workloads.ecoli_pb50(seed=12345, scale=SCALE)
    cfg = config.preset(preset)
    ctx = gpu.Context(int(cfg["kmer_size"]), 0)
    ctx.set_reads(rs)
    vi = gpu.VertexIndex(ctx, float(int(cfg["assemble_kmer_sample"])))
    vi.build(cfg)
    det = gpu.OverlapDetector.for_assemble(ctx, vi, cfg, min_overlap=config.DETECTOR_MIN_OVERLAP)
    fwd = np.arange(0, 2 * rs.n, 2).astype(np.uint32)
    res = det.getSeqOverlapsBatch(fwd)
    recs = np.asarray(res.recs).copy()
    off = np.asarray(res.query_off).astype(np.uint64)
    params = dict(window=100, max_overhang=int(cfg["maximum_overhang"]), max_drop_rate=5.0, overlap_coverage=25, uneven_coverage=0)

    out = {}
    for vectors in (True, False):
        p = gpu.CoverageParams(want_vectors=int(vectors), **params)
        got = ctx.read_coverage(recs, off, rs.length, p)
        secs = []
        for _ in range(RUNS):
            got = ctx.read_coverage(recs, off, rs.length, p)
            secs.append(ctx.last_coverage_seconds)
        out[vectors] = (got, secs, ctx.kernel_times())

    # the record table alone, host to device (pageable memory, as the call takes it)
    raw = torch.from_numpy(recs.view(np.uint8))
    up = []
    for _ in range(RUNS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dev = raw.to("cuda")
        torch.cuda.synchronize()
        up.append(time.perf_counter() - t0)
        del dev
    up = up[1:]

    b = R.ReadBatch.__new__(R.ReadBatch)
    b.params, b.query_len, b.query_off = params, rs.length.astype(np.int32), off
    b.table = np.stack([recs[f].astype(np.int64) for f in R.COLS], 1)
    one = R.native_reads(b, threads=1, repeats=RUNS)
    many = R.native_reads(b, threads=16, repeats=RUNS)
    full = {k: getattr(out[True][0], k) for k in R.READ_FIELDS}
    bare = {k: getattr(out[False][0], k) for k in R.READ_FIELDS}
    scalars = [k for k in R.READ_FIELDS if k not in ("full", "junction")]
    same = R.same(full, one, R.READ_FIELDS) and R.same(full, many, R.READ_FIELDS) and R.same(bare, one, scalars)

    windows = np.diff(full["win_off"].astype(np.int64))
    print(f"{rs.n} reads, {len(recs)} records ({recs.nbytes / 1e6:.1f} MB), {int(windows.sum())} windows (mean {windows.mean():.1f} per read), "
          f"{int(full['chimeric'].sum())} chimeric")
    for vectors in (True, False):
        _, secs, kt = out[vectors]
        print(f"  device call, {'with' if vectors else 'without'} vectors: {' '.join(f'{s * 1e3:.2f}' for s in secs)} ms; kernels (ms, launches): " +
              ", ".join(f"{k} {v[0] * 1e3:.3f} ({v[1]})" for k, v in kt.items()))
    print(f"  record table upload alone: {' '.join(f'{s * 1e3:.2f}' for s in up)} ms")
    print(f"  host form: {one['seconds'] * 1e3:.1f} ms on 1 thread, {many['seconds'] * 1e3:.1f} ms on 16; all results equal: {same}")
    print(json.dumps(dict(reads=int(rs.n), records=len(recs), windows=int(windows.sum()),
                          device_call_ms={("vectors" if v else "no_vectors"): [round(s * 1e3, 3) for s in out[v][1]] for v in (True, False)},
                          kernel_ms={("vectors" if v else "no_vectors"): {k: round(t[0] * 1e3, 3) for k, t in out[v][2].items()}
                                     for v in (True, False)},
                          upload_ms=[round(s * 1e3, 3) for s in up], host_1_thread_ms=round(one["seconds"] * 1e3, 3),
                          host_16_threads_ms=round(many["seconds"] * 1e3, 3), equal=bool(same))))
    ctx.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
