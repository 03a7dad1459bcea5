"""Generates tests/golden/index_edges.json.  Run in the build container (needs oracle/_ref/ref_dumper, see
oracle/Makefile):

    python tests/golden/make_index_edge_golden.py

Per case of tests/index_craft.py: the sha256 of the crafted reads; per parameter set the UNMODIFIED reference
(Flye 2.8.1) can run -- its dumper fixes min_freq = 2, and its flat counter takes 90 s at k = 17 -- the digest
(helpers.index_digest) of the index it built over those reads with the set's values as --params, the key, entry and
repetitive counts and the bits of _sampleRate.  The other sets are marked "oracle_only".  Digests and counts only;
the reads are regenerated from their seeds.  --query-limit 1: the overlap pass of the dumper over a sparse w = 63 /
64 index would take 30 s and nothing of it is stored.
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import index_craft as ic  # noqa: E402
from helpers import index_digest  # noqa: E402
from oracle import oracle as O  # noqa: E402


def reference_entry(fasta, rs, p, tmp):
    out = os.path.join(tmp, "index.txt")
    O.run_ref(fasta, params_string=ic.ref_params(p), threads=4, index_out=out, query_limit=1)
    hdr, ix = O.parse_ref_index(out, rs)
    return dict(sha256=index_digest(ix), sample_rate_bits=hdr["sampleRateBits"], repetitive_frequency=int(hdr["repFreq"]),
                total_kmers=int(hdr["numKmers"]), selected_kmers=int(hdr["keys"]), repetitive_kmers=int(hdr["rep"]),
                index_entries=int(len(ix.entries)))


def main():
    assert O.have_ref(), "oracle/_ref/ref_dumper missing: make -C oracle ref"
    meta = {}
    for name in ic.CASE_NAMES:
        case = ic.case(name)
        with tempfile.TemporaryDirectory() as tmp:
            fa = os.path.join(tmp, "reads.fasta")
            case.reads.write_fasta(fa)
            sets = {}
            for p in case.psets:
                sets[ic.pset_name(p)] = reference_entry(fa, case.reads, p, tmp) if ic.has_reference(p) else {"oracle_only": True}
                print(name, ic.pset_name(p), sets[ic.pset_name(p)], flush=True)
        meta[name] = dict(n_reads=case.reads.n, total_bases=int(case.reads.total_bases), reads_sha256=ic.reads_sha256(case.reads),
                          sets=sets)
    with open(os.path.join(HERE, "index_edges.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
