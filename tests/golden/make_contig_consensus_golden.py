"""Generates the fixtures of tests/test_contig_consensus.py: what the UNMODIFIED Python of the reference
(flye.polishing.consensus and flye.polishing.alignment, imported from the reference tree, nothing of them copied) does with
the alignments of tests/contig_consensus_restate.py.  Stored, as data only: the FASTA text the reference's writer makes of
get_consensus's dictionary (contig_consensus_*.fa.gz) and contig_consensus_cases.json (per contig the sequence's sha256
and length, the indices get_uniform_alignments kept, its cov_threshold and the sha256 of its window thresholds -- both read
from the function's frame when it returns --, aln_errors and the sha256 of each profile array; per run the sha256 of the
generated input).

    python tests/golden/make_contig_consensus_golden.py            # the fixtures
    python tests/golden/make_contig_consensus_golden.py --time     # also: the reference's time on the input of
                                                                   # tools/contig_consensus_bench.py
"""
import collections
import gzip
import hashlib
import json
import os
import sys
import tempfile
import time

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
REF = os.environ.get("FLYE_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

import numpy as np  # noqa: E402

import contig_consensus_restate as CR  # noqa: E402
import flye.polishing.alignment as ref_aln  # noqa: E402
import flye.polishing.consensus as ref_cons  # noqa: E402
import flye.utils.fasta_parser as ref_fp  # noqa: E402


def put(name, text):
    path = os.path.join(HERE, name)
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(text.encode("latin-1"))
    assert os.path.getsize(path) <= 64 * 1024, (name, os.path.getsize(path))


def uniform_with_locals(alns, length):
    """get_uniform_alignments, and the two locals the device call also returns, read from its frame on return"""
    seen = {}

    def watch(frame, event, arg):
        if event == "return" and frame.f_code is ref_aln.get_uniform_alignments.__code__:
            seen["cov_threshold"] = frame.f_locals["cov_threshold"]
            seen["thresholds"] = list(frame.f_locals["wnd_qual_thresholds"])

    sys.setprofile(watch)
    try:
        kept = ref_aln.get_uniform_alignments(alns, length)
    finally:
        sys.setprofile(None)
    ids = set(id(a) for a in kept)
    return [k for k, a in enumerate(alns) if id(a) in ids], seen["cov_threshold"], seen["thresholds"]


def reference_contig(contig, alns, platform):
    """_thread_worker (consensus.py:43-46)"""
    profile, aln_errors = ref_cons._contig_profile(alns, platform, contig.length)
    sequence = ref_cons._flatten_profile(profile)
    chosen, accepted, max_match = [], [], []
    for elem in profile:
        groups = collections.Counter(elem.insertions.values())
        total = sum(elem.matches.values())
        chosen.append(min(groups, key=lambda s: (-groups[s], s)).encode("latin-1") if groups else b"")
        accepted.append(int(bool(groups) and len(elem.insertions) > total // 2))
        max_match.append(ord(min(elem.matches, key=lambda b: (-elem.matches[b], b)) if elem.matches else elem.nucl))
    prof = dict(nucl=np.array([ord(e.nucl) for e in profile], np.uint8),
                match_total=np.array([sum(e.matches.values()) for e in profile], np.int32),
                num_ins=np.array([len(e.insertions) for e in profile], np.int32),
                max_match=np.array(max_match, np.uint8), accepted=np.array(accepted, np.uint8), ins=chosen)
    return sequence, [float(e) for e in aln_errors], prof


def run_reference(run):
    meta = dict(input_sha256=CR.input_digest(run), contigs={})
    fasta = {}
    for contig, _ in run["contigs"]:
        alns = run["alns"][contig.id]
        kept, cov_threshold, thresholds = uniform_with_locals(alns, contig.length)
        sequence, aln_errors, prof = reference_contig(contig, alns, run["err_mode"])
        if len(sequence) > 0:
            fasta[contig.id] = sequence
        meta["contigs"][contig.id] = dict(
            uniform_kept=kept, cov_threshold=int(cov_threshold),
            thresholds_sha256=hashlib.sha256(np.array(thresholds, np.float64).tobytes()).hexdigest(),
            aln_errors=aln_errors, seq_len=len(sequence), seq_sha256=hashlib.sha256(sequence.encode("latin-1")).hexdigest(),
            n_accepted=int(prof["accepted"].sum()), profile_sha256=CR.profile_digests(prof))
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "consensus.fasta")
        ref_fp.write_fasta_dict(fasta, path)
        text = open(path).read()
    return text, meta


def main():
    cases = {}
    for name, make in sorted(CR.RUNS.items()):
        text, meta = run_reference(make())
        put("contig_consensus_" + name + ".fa.gz", text)
        cases[name] = meta
        print(name, "contigs", len(meta["contigs"]), "bases", sum(m["seq_len"] for m in meta["contigs"].values()), "accepted insertions",
              sum(m["n_accepted"] for m in meta["contigs"].values()), flush=True)
    path = os.path.join(HERE, "contig_consensus_cases.json")
    json.dump(cases, open(path, "w"), indent=0, sort_keys=True)
    assert os.path.getsize(path) <= 64 * 1024, os.path.getsize(path)
    if "--time" in sys.argv:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from contig_consensus_bench import bench_input
        run = bench_input()
        (contig, _), = run["contigs"]
        alns = run["alns"][contig.id]
        t0 = time.perf_counter()
        profile, _ = ref_cons._contig_profile(alns, run["err_mode"], contig.length)
        sequence = ref_cons._flatten_profile(profile)
        dt = time.perf_counter() - t0
        print("reference consensus.py, one process: contig of %d bp, %d alignments, %d columns: %.2f s, %d bases" %
              (contig.length, len(alns), sum(len(a.trg_seq) for a in alns), dt, len(sequence)), flush=True)


if __name__ == "__main__":
    main()
