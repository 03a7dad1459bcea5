"""fg_sam_parse and SamAlignments(device_text=True) on the input of tools/expand_cigars_bench.py written as SAM text: one
contig of 200 kb, 2000 alignments of 10 kb with ~12 % errors, QUAL as long as SEQ.  First the equality:
SamAlignments(want_cols=False, device_text=True).chunks() against device_text=False, record for record.  Then, after one
warm-up each, the median and the best of five: the wall time of both constructions (file read included, it is the same
file), the fg_sam_parse call alone, its kernels by kernel_times(), and the bytes sent up.  The yardstick is the host
tokeniser (device_text=False), which this change leaves as it was.  There is no pass bar.
    python tools/sam_parse_bench.py [--length 200000] [--alignments 2000] [--read 10000] [--seed 2024] [--repeat 5]
                                    [--out profiles/sam_parse_bench.json]"""
import argparse
import datetime
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

import cigar_restate as G  # noqa: E402
from expand_cigars_bench import bench_input  # noqa: E402


def sam_text(run, recs, seed):
    rng = np.random.default_rng(seed)
    lines = ["@HD\tVN:1.6\tSO:coordinate\n"] + ["@SQ\tSN:%s\tLN:%d\n" % (c, len(s)) for c, s in run["contigs"].items()]
    for r in recs:
        seq = r["seq"].decode()
        qual = (rng.integers(33, 74, len(seq)).astype(np.uint8)).tobytes().decode()
        lines.append("\t".join([r["qry_id"], str(r["flags"]), r["contig"].decode(), str(r["pos"]), "60",
                                G.cigar_of([(chr(op), n) for op, n in r["runs"]]), "*", "0", "0", seq, qual, "NM:i:0"]) + "\n")
    return "".join(lines).encode()


def same_records(a, b):
    if [c for c, _ in a] != [c for c, _ in b]:
        return False
    for (_, x), (_, y) in zip(a, b):
        if len(x) != len(y):
            return False
        for r, s in zip(x, y):
            if r[:13] != s[:13] or not np.array_equal(r.ops, s.ops) or not np.array_equal(r.lens, s.lens) or r.seq != s.seq:
                return False
    return True


def timed(fn, repeat):
    fn()                                            # warm-up
    out = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return dict(median_s=round(statistics.median(out), 5), best_s=round(min(out), 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=200000)
    ap.add_argument("--alignments", type=int, default=2000)
    ap.add_argument("--read", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sam_parse_bench.json"))
    a = ap.parse_args()
    from flye_amd import gpu
    run, recs = bench_input(a.length, a.alignments, a.read, a.seed)
    text = sam_text(run, recs, a.seed)
    ctx = gpu.Context(17, 0)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bench.sam")
        with open(path, "wb") as f:
            f.write(text)
        make = lambda device_text: gpu.SamAlignments(ctx, path, run["contigs"], max_coverage=None, use_secondary=True, want_cols=False,
                                                     device_text=device_text)
        host, dev = make(False).chunks(), make(True).chunks()
        assert same_records(dev, host), "device_text=True and device_text=False give different records"
        n = sum(len(x) for _, x in host)
        print("check: %d records in %d chunks identical from both tokenisers" % (n, len(host)), flush=True)
        res = dict(date=datetime.date.today().isoformat(), shape=dict(contig=a.length, alignments=a.alignments, read=a.read, seed=a.seed),
                   text_bytes=len(text), records=n, runs=int(sum(len(r.ops) for _, x in host for r in x)), repeat=a.repeat,
                   warm_up=1, sam_alignments_host=timed(lambda: make(False), a.repeat),
                   sam_alignments_device_text=timed(lambda: make(True), a.repeat))
    kernel_runs = []

    def parse():
        ctx.sam_parse(text)
        kernel_runs.append({k: v[0] for k, v in ctx.kernel_times().items()})

    res["fg_sam_parse_call"] = timed(parse, a.repeat)
    kernel_runs = kernel_runs[1:]
    res["kernels_median_ms"] = {k: round(statistics.median(r[k] for r in kernel_runs) * 1e3, 4) for k in kernel_runs[0]}
    res["kernels_sum_median_ms"] = round(statistics.median(sum(r.values()) for r in kernel_runs) * 1e3, 4)
    res["bytes_sent_up"] = len(text)
    for k, v in res.items():
        print("%-28s %s" % (k, v), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
