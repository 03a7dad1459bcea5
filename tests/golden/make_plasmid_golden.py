"""Generates the fixtures of tests/test_plasmids.py: what the UNMODIFIED Python of the reference (flye.short_plasmids.*
and flye.utils.sam_parser, imported from the reference tree, nothing of it copied) does with the inputs of
tests/plasmid_restate.py.  Stored, as data only: per case the two input files (plasmid_<case>.paf.gz, plasmid_<case>.fa.gz)
and, in plasmid_cases.json.gz, the mapping-rate dict, the circular reads (name and hit fields, in dict order), the
circular pairs, the sha256 of the unmapped-reads FASTA with its two counters, the sha256 of both trimmed dicts, and the
unique-plasmid dict with the vertex order the process used (the same set, rebuilt by the same insertions in the same
process).

    python tests/golden/make_plasmid_golden.py            # the fixtures
    python tests/golden/make_plasmid_golden.py --time     # also: the reference's time on the input of tools/plasmid_bench.py
"""
import collections
import gzip
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

import plasmid_restate as PR  # noqa: E402
import flye.short_plasmids.circular_sequences as ref_circ  # noqa: E402
import flye.short_plasmids.unmapped_reads as ref_unmapped  # noqa: E402
import flye.utils.fasta_parser as ref_fp  # noqa: E402
from flye.utils.sam_parser import read_paf  # noqa: E402

Args = collections.namedtuple("Args", ["reads"])


def put(name, data):
    path = os.path.join(HERE, name)
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(data)
    assert os.path.getsize(path) <= 64 * 1024, (name, os.path.getsize(path))


def fields(h):
    return [h.query, h.query_length, h.query_start, h.query_end, h.target, h.target_length, h.target_start, h.target_end]


def run_reference(case, params):
    unmapped_threshold, unique_threshold, min_length = params
    with tempfile.TemporaryDirectory() as tmp:
        paf, fasta, out = os.path.join(tmp, "hits.paf"), os.path.join(tmp, "reads.fasta"), os.path.join(tmp, "unmapped.fasta")
        open(paf, "wb").write(case["paf"])
        open(fasta, "wb").write(case["fasta"])
        seqs = ref_fp.read_sequence_dict(fasta)
        rates = ref_unmapped.calc_mapping_rates(paf)
        circ = ref_circ.extract_circular_reads(paf)
        pairs = ref_circ.extract_circular_pairs(paf)
        # the numbers extract_unmapped_reads only logs: the same sums over the same stream
        ref_unmapped.extract_unmapped_reads(Args([fasta]), paf, out, unmapped_threshold)
        unmapped = open(out).read()
        total = sum(len(s) for s in seqs.values())
        unmapped_bases = sum(len(line) for line in unmapped.splitlines() if not line.startswith(">"))
        # the vertex order of extract_unique_plasmids: the same set by the same insertions in this process
        names = set()
        for hit in read_paf(paf):
            names.add(hit.query)
            names.add(hit.target)
        unique = ref_circ.extract_unique_plasmids(paf, fasta, unique_threshold, 500, min_length)
        return dict(paf_sha256=PR.sha(case["paf"]), fasta_sha256=PR.sha(case["fasta"]),
                    mapping_rates={q: dict(t) for q, t in rates.items()},
                    circular_reads=[[name, fields(h)] for name, h in circ.items()],
                    circular_pairs=[[fields(p[0]), fields(p[1])] for p in pairs],
                    trimmed_reads_sha256=PR.sha(json.dumps(ref_circ.trim_circular_reads(circ, seqs), sort_keys=True)),
                    trimmed_pairs_sha256=PR.sha(json.dumps(ref_circ.trim_circular_pairs(pairs, seqs), sort_keys=True)),
                    unmapped_sha256=PR.sha(unmapped), total_bases=total, unmapped_bases=unmapped_bases,
                    vertex_order=list(names), unique_plasmids=unique)


def main():
    cases = {}
    for name, make in sorted(PR.CASES.items()):
        case = make()
        put("plasmid_%s.paf.gz" % name, case["paf"])
        put("plasmid_%s.fa.gz" % name, case["fasta"])
        cases[name] = run_reference(case, PR.PARAMS[name])
        g = cases[name]
        print(name, "hits", case["paf"].count(b"\n"), "queries", len(g["mapping_rates"]), "circular reads", len(g["circular_reads"]),
              "pairs", len(g["circular_pairs"]), "unique", len(g["unique_plasmids"]), "unmapped", g["unmapped_bases"], "/", g["total_bases"],
              flush=True)
    put("plasmid_cases.json.gz", json.dumps(cases, separators=(",", ":")).encode())
    if "--time" in sys.argv:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from plasmid_bench import bench_input
        with tempfile.TemporaryDirectory() as tmp:
            for label, text in bench_input().items():
                paf = os.path.join(tmp, label + ".paf")
                open(paf, "wb").write(text)
                t0 = time.perf_counter()
                rates = ref_unmapped.calc_mapping_rates(paf)
                t1 = time.perf_counter()
                circ = ref_circ.extract_circular_reads(paf)
                t2 = time.perf_counter()
                pairs = ref_circ.extract_circular_pairs(paf)
                t3 = time.perf_counter()
                print(json.dumps(dict(input=label, hits=text.count(b"\n"), calc_mapping_rates_s=round(t1 - t0, 3),
                                      extract_circular_reads_s=round(t2 - t1, 3), extract_circular_pairs_s=round(t3 - t2, 3),
                                      queries=len(rates), circular_reads=len(circ), circular_pairs=len(pairs))), flush=True)


if __name__ == "__main__":
    main()
