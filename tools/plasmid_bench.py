"""fg_paf_groups / fg_paf_circular / fg_components on the shape of the short-plasmid stage: a seeded reads-to-contigs
PAF of about 2 M hits and an all-vs-all PAF of 200 k hits, both made in memory.  First every output array is compared
with the restatement (tests/plasmid_restate.py), then the tokeniser, the id assignment, the calls and their kernels are
timed.  The reference's own time on the same input: python tests/golden/make_plasmid_golden.py --time (host only).

    python tools/plasmid_bench.py [--out profiles/plasmid_bench.json] [--repeat 3] [--small]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def bench_input(n_reads=1_000_000, n_pairs_reads=20_000, seed=7):
    """{"reads2contigs": PAF bytes, "allvsall": PAF bytes}.  Reads against 200 contigs: 1 - 4 hits per read (2 on
    average), most of a read's hits on one contig, sorted by query as minimap2 writes them.  Unmapped reads against
    themselves: runs of about ten hits over a few targets, the query among them."""
    rng = np.random.RandomState(seed)
    per = rng.choice([1, 2, 3, 4], n_reads, p=[0.4, 0.3, 0.2, 0.1])
    n = int(per.sum())
    read = np.repeat(np.arange(n_reads), per)
    rlen = rng.randint(3000, 30000, n_reads)[read]
    home = np.repeat(rng.randint(0, 200, n_reads), per)
    ctg = np.where(rng.rand(n) < 0.8, home, rng.randint(0, 200, n))
    clen = rng.randint(200_000, 5_000_000, 200)[ctg]
    qs = (rng.rand(n) * rlen * 0.7).astype(np.int64)
    qe = np.minimum(rlen, qs + (rng.rand(n) * rlen * 0.6).astype(np.int64) + 50)
    ts = (rng.rand(n) * (clen - 40000)).astype(np.int64)
    te = ts + (qe - qs)
    a = "".join("read_%d\t%d\t%d\t%d\t+\tcontig_%d\t%d\t%d\t%d\t%d\t%d\t60\n" % r
                for r in zip(read.tolist(), rlen.tolist(), qs.tolist(), qe.tolist(), ctg.tolist(), clen.tolist(), ts.tolist(), te.tolist(),
                             (qe - qs).tolist(), (qe - qs).tolist())).encode()
    per = rng.randint(4, 17, n_pairs_reads)
    n = int(per.sum())
    q = np.repeat(np.arange(n_pairs_reads), per)
    t = np.where(rng.rand(n) < 0.15, q, (q + rng.randint(1, 6, n) * 37) % n_pairs_reads)
    length = rng.randint(1500, 9000, n_pairs_reads)
    ql, tl = length[q], length[t]
    head = rng.rand(n) < 0.5
    qs = np.where(head, rng.randint(0, 400, n), (rng.rand(n) * ql * 0.5).astype(np.int64))
    qe = np.where(head, qs + (rng.rand(n) * (ql - qs) * 0.5).astype(np.int64), ql - rng.randint(0, 400, n))
    qe = np.maximum(qs + 1, qe)
    ts = np.where(head, (tl * 0.5).astype(np.int64) + rng.randint(0, 400, n), rng.randint(0, 400, n))
    te = np.where(head, tl - rng.randint(0, 400, n), ts + (rng.rand(n) * (tl - ts) * 0.4).astype(np.int64))
    te = np.maximum(ts + 1, te)
    b = "".join("u_%d\t%d\t%d\t%d\t+\tu_%d\t%d\t%d\t%d\t100\t200\t60\n" % r
                for r in zip(q.tolist(), ql.tolist(), qs.tolist(), qe.tolist(), t.tolist(), tl.tolist(), ts.tolist(), te.tolist())).encode()
    return {"reads2contigs": a, "allvsall": b}


def timed(f, repeat):
    best, out = None, None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = f()
        dt = time.perf_counter() - t0
        best = dt if best is None or dt < best else best
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="a fiftieth of the input (a quick check of the tool itself)")
    args = ap.parse_args()
    from flye_amd import gpu
    import plasmid_restate as PR

    t0 = time.perf_counter()
    texts = bench_input(20_000, 400) if args.small else bench_input()
    res = dict(tool="tools/plasmid_bench.py", input_seconds=round(time.perf_counter() - t0, 2), inputs={})
    ctx = gpu.Context(17, 0)
    ctx.components(4, [0], [1])         # the first call of a process pays the code object's load
    for label, text in texts.items():
        r = dict(bytes=len(text))
        parsed = None
        parse_s, id_s = [], []
        for _ in range(args.repeat):
            parsed = gpu.paf_parse(text)
            parse_s.append(parsed.parse_seconds)
            id_s.append(parsed.id_seconds)
        hits = parsed.hits
        r.update(hits=len(hits), names=len(parsed.names), fg_paf_parse_s=round(min(parse_s), 4), ids_numpy_s=round(min(id_s), 4))
        # equality first
        t0 = time.perf_counter()
        want_g, want_c = PR.groups(hits), PR.circular(hits)
        r["restatement_s"] = round(time.perf_counter() - t0, 2)
        got_g, got_c = ctx.paf_groups(hits), ctx.paf_circular(hits)
        for got, want in ((got_g, want_g), (got_c, want_c)):
            for k in want:
                assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (label, k)
        r.update(groups=len(want_g["group_query"]), largest_group=int(np.diff(want_g["group_off"].astype(np.int64)).max()),
                 circular_reads=len(want_c["circ_query"]), pair_candidates=int(want_c["pair_ok"].sum()), identical=True)
        for name, call in (("fg_paf_groups", lambda: ctx.paf_groups(hits)), ("fg_paf_circular", lambda: ctx.paf_circular(hits))):
            dt, _ = timed(call, args.repeat)
            kt = ctx.kernel_times()
            r[name] = dict(call_s=round(dt, 4), kernels_s=round(sum(v[0] for v in kt.values()), 5),
                           kernels={k: round(v[0], 5) for k, v in sorted(kt.items())})
        # the graph extract_unique_plasmids would build from these groups at its threshold
        first = hits[got_g["order"][got_g["group_off"][:-1].astype(np.int64)].astype(np.int64)]
        keep = (first["query"] != first["target"]) & ((got_g["query_cover"] / first["query_len"] > 0.8) |
                                                      (got_g["target_cover"] / first["target_len"] > 0.8))
        eu, ev = first["query"][keep], first["target"][keep]
        labels = ctx.components(len(parsed.names), eu, ev)
        assert np.array_equal(labels, PR.components(len(parsed.names), eu, ev)), label
        dt, _ = timed(lambda: ctx.components(len(parsed.names), eu, ev), args.repeat)
        kt = ctx.kernel_times()
        r["fg_components"] = dict(vertices=len(parsed.names), edges=int(keep.sum()), components=int(len(np.unique(labels))), call_s=round(dt, 4),
                                  kernels_s=round(sum(v[0] for v in kt.values()), 5), rounds=int(kt.get("k_cc_hook", (0, 0))[1]))
        res["inputs"][label] = r
        print(label, json.dumps(r), flush=True)
    line = json.dumps(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
