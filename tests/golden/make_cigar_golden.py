"""Generates the fixture of tests/test_expand_cigars.py: what the UNMODIFIED reader of the reference
(flye.utils.sam_parser.SynchronizedSamReader, imported from the reference tree, its IO process included; nothing of it
copied) returns for the SAM files of tests/cigar_restate.py, and, for the end-to-end check, what the reference's consensus
stage (flye.polishing.consensus: _contig_profile and _flatten_profile) makes of those alignments.  Stored, as data only, in
cigar_cases.json: per run the sha256 of the generated input; per chunk the contig, its alignments as lists in the order of
FIELDS (err_rate as float.hex(), the gapped strings as length and sha256) and the sha256 and length of the consensus.

    python tests/golden/make_cigar_golden.py            # the fixture
    python tests/golden/make_cigar_golden.py --time     # also: the reference's _parse_cigar on the input of
                                                        # tools/expand_cigars_bench.py, one process
"""
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

import cigar_restate as G  # noqa: E402
import flye.polishing.consensus as ref_cons  # noqa: E402
from flye.utils.sam_parser import SynchronizedSamReader  # noqa: E402

FIELDS = ["qry_id", "trg_id", "qry_start", "qry_end", "qry_sign", "qry_len", "trg_start", "trg_end", "trg_sign", "trg_len",
          "err_rate", "is_secondary", "trg_seq_len", "trg_seq_sha256", "qry_seq_len", "qry_seq_sha256"]


def sha(text):
    return hashlib.sha256(text.encode("latin-1")).hexdigest()


def row(a):
    return [a.qry_id, a.trg_id, a.qry_start, a.qry_end, a.qry_sign, a.qry_len, a.trg_start, a.trg_end, a.trg_sign, a.trg_len,
            float(a.err_rate).hex(), int(a.is_secondary), len(a.trg_seq), sha(a.trg_seq), len(a.qry_seq), sha(a.qry_seq)]


def run_reference(run):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "aln.sam")
        with open(path, "wb") as f:
            f.write(run["sam"])
        reader = SynchronizedSamReader(path, run["contigs"], max_coverage=run["max_coverage"], use_secondary=run["use_secondary"])
        chunks = []
        try:
            while True:
                contig, alns = reader.get_chunk()
                if contig is None:
                    break
                chunks.append((contig, alns))
        finally:
            reader.close()
    out = []
    for contig, alns in chunks:
        length = len(run["contigs"][contig])
        sequence = ref_cons._flatten_profile(ref_cons._contig_profile(alns, "pacbio", length)[0])
        out.append(dict(contig=contig, alignments=[row(a) for a in alns], consensus_len=len(sequence), consensus_sha256=sha(sequence)))
    return dict(input_sha256=G.input_digest(run), fields=FIELDS, chunks=out)


def main():
    cases = {}
    for name, make in sorted(G.RUNS.items()):
        cases[name] = run_reference(make())
        print(name, "chunks", len(cases[name]["chunks"]), "alignments", sum(len(c["alignments"]) for c in cases[name]["chunks"]),
              "consensus bases", sum(c["consensus_len"] for c in cases[name]["chunks"]), flush=True)
    path = os.path.join(HERE, "cigar_cases.json")
    json.dump(cases, open(path, "w"), separators=(",", ":"), sort_keys=True)
    assert os.path.getsize(path) <= 64 * 1024, os.path.getsize(path)
    if "--time" in sys.argv:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from expand_cigars_bench import bench_input
        run, recs = bench_input()
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "empty.sam")
            open(path, "wb").close()
            reader = SynchronizedSamReader(path, run["contigs"], max_coverage=1000)
            try:
                t0 = time.perf_counter()
                cols = 0
                for r in recs:
                    cols += len(reader._parse_cigar(G.cigar_of([(chr(op), n) for op, n in r["runs"]]).encode(), r["seq"], r["contig"], r["pos"])[3])
                dt = time.perf_counter() - t0
            finally:
                reader.close()
        print("reference _parse_cigar, one process: %d alignments, %d columns: %.2f s" % (len(recs), cols, dt), flush=True)


if __name__ == "__main__":
    main()
