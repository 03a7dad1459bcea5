"""Generates the fixtures of tests/test_bubbles.py: what the UNMODIFIED Python of the reference (flye.polishing.bubbles
and flye.polishing.alignment, imported from the reference tree, nothing of them copied) does with the alignments of
tests/bubbles_restate.py.  Stored, as data only: the text _output_bubbles wrote (bubbles_*.fa.gz) and bubbles_cases.json
(per contig the partition, the counters, aln_errors, sha256 of each profile array; per run the sha256 of the generated
input, the cfg.vals overrides and, for the run that goes through get_uniform_alignments, the indices it kept).

    python tests/golden/make_bubbles_golden.py            # the fixtures
    python tests/golden/make_bubbles_golden.py --time     # also: the reference's time on the input of tools/bubbles_bench.py
"""
import gzip
import io
import json
import os
import sys
import time

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
REF = os.environ.get("FLYE_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

import numpy as np  # noqa: E402

import bubbles_restate as R  # noqa: E402
import flye.config.py_cfg as cfg  # noqa: E402
import flye.polishing.alignment as ref_aln  # noqa: E402
import flye.polishing.bubbles as ref_bub  # noqa: E402


def put(name, text):
    path = os.path.join(HERE, name)
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(text.encode("latin-1"))
    assert os.path.getsize(path) <= 64 * 1024, (name, os.path.getsize(path))


def reference_contig(contig, alns, err_mode):
    """_thread_worker from _compute_profile onward (bubbles.py:66-78)"""
    profile, aln_errors = ref_bub._compute_profile(alns, err_mode, contig.length)
    partition, n_long = ref_bub._get_partition(profile, err_mode)
    bubbles = ref_bub._get_bubble_seqs(alns, err_mode, profile, partition, contig)
    mean_cov = sum(len(b.branches) for b in bubbles) // (len(bubbles) + 1)
    bubbles, n_empty, n_long_branch = ref_bub._postprocess_bubbles(bubbles)
    out = io.StringIO()
    ref_bub._output_bubbles(bubbles, out)
    prof = dict(coverage=np.array([p.coverage for p in profile], np.int32),
                num_inserts=np.array([p.num_inserts for p in profile], np.int32),
                num_deletions=np.array([p.num_deletions for p in profile], np.int32),
                num_missmatch=np.array([p.num_missmatch for p in profile], np.int32),
                nucl=np.array([ord(p.nucl) if p.nucl else 0 for p in profile], np.uint8))
    meta = dict(partition=[int(x) for x in partition], n_long_bubbles=n_long, n_empty=n_empty, n_long_branch=n_long_branch,
                mean_cov=mean_cov, n_bubbles=len(bubbles), aln_errors=[float(e) for e in aln_errors],
                profile_sha256=R.profile_digests(prof))
    return out.getvalue(), meta


def run_reference(run):
    saved = dict(cfg.vals)
    cfg.vals.update(run["overrides"])
    try:
        text, meta = [], dict(err_mode=run["err_mode"], overrides=run["overrides"], input_sha256=R.input_digest(run), contigs={})
        for contig, _ in run["contigs"]:
            alns = run["alns"][contig.id]
            if run["uniform"]:
                kept = ref_aln.get_uniform_alignments(alns, contig.length)
                ids = [id(a) for a in kept]
                meta.setdefault("uniform_kept", {})[contig.id] = [k for k, a in enumerate(alns) if id(a) in ids]
                alns = kept
            t, m = reference_contig(contig, alns, run["err_mode"])
            text.append(t)
            meta["contigs"][contig.id] = m
        return "".join(text), meta
    finally:
        cfg.vals.clear()
        cfg.vals.update(saved)


def main():
    cases = {}
    for name, make in sorted(R.RUNS.items()):
        text, meta = run_reference(make())
        put(name + ".fa.gz", text)
        cases[name] = meta
        print(name, "bubbles", sum(m["n_bubbles"] for m in meta["contigs"].values()), "branches", text.count("\n") // 2 -
              sum(m["n_bubbles"] for m in meta["contigs"].values()), flush=True)
    path = os.path.join(HERE, "bubbles_cases.json")
    json.dump(cases, open(path, "w"), indent=0, sort_keys=True)
    assert os.path.getsize(path) <= 64 * 1024, os.path.getsize(path)
    if "--time" in sys.argv:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from bubbles_bench import bench_input
        run = bench_input()
        (contig, _), = run["contigs"]
        t0 = time.perf_counter()
        text, meta = reference_contig(contig, run["alns"][contig.id], run["err_mode"])
        dt = time.perf_counter() - t0
        print("reference bubbles.py, one process: contig of %d bp, %d alignments, %d columns: %.2f s, %d bubbles" %
              (contig.length, len(run["alns"][contig.id]), sum(len(a.trg_seq) for a in run["alns"][contig.id]), dt,
               meta["n_bubbles"]), flush=True)


if __name__ == "__main__":
    main()
