"""Generates tests/golden/*.  Run in the build container (needs /root/reference
and oracle/_ref/ref_dumper, see oracle/Makefile):

    python tests/golden/make_golden.py [case names ...]

Each case = seeded simulator parameters (inputs are regenerated from the seed, not
stored) + what the UNMODIFIED reference (Flye 2.8.1 compiled from /root/reference)
produced on those reads: an index digest and the full OverlapRange list.  The
reference's own tests hold no vectors for this path, so these are
the golden vectors; nothing of the reference's source is stored here.
"""
import gzip
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
from flye_amd import config, synth  # noqa: E402
from oracle import oracle as O  # noqa: E402

CFG_DIR = "/root/reference/flye/config/bin_cfg/"

CASES = [
    dict(name="raw_pb", preset="raw", sim=dict(seed=101, genome_len=60_000, coverage=30, kind="pb_raw"),
         min_read_len=1000),
    dict(name="raw_ont_rc", preset="raw",
         sim=dict(seed=102, genome_len=60_000, coverage=25, kind="ont_raw", n_homopolymers=40, n_tandems=60),
         min_read_len=1000, rc_queries=True, max_overlaps=30),
    dict(name="raw_div", preset="raw",
         sim=dict(seed=103, genome_len=50_000, coverage=35, kind="pb_raw", n_tandems=80, n_homopolymers=30,
                  n_repeat_families=10),
         min_read_len=1000, div_mode="assemble"),
    dict(name="raw_local", preset="raw", sim=dict(seed=104, genome_len=40_000, coverage=30, kind="pb_raw"),
         min_read_len=1000, force_local=True),
    dict(name="hifi", preset="hifi", sim=dict(seed=105, genome_len=60_000, coverage=25, kind="hifi"),
         min_read_len=1000),
    dict(name="corrected_local", preset="corrected",
         sim=dict(seed=106, genome_len=50_000, coverage=25, kind="hifi", n_homopolymers=40, n_tandems=40),
         min_read_len=1000, force_local=True),
    dict(name="hifi_rc_max", preset="hifi", sim=dict(seed=107, genome_len=50_000, coverage=25, kind="hifi03"),
         min_read_len=1000, rc_queries=True, max_overlaps=20),
    # ReadAligner-style use (src/repeat_graph/read_aligner.cpp:178-217): index = long "edge"
    # sequences, queries = reads from a second container, all primaries (onlyMax = false),
    # minOverlap = 100, no overhang check, k-mer divergence only
    dict(name="edges_raw", preset="raw",
         sim=dict(seed=108, genome_len=60_000, coverage=3, kind="hifi03", median_len=20000, min_len=8000,
                  max_len=30000, read_seed=7),
         queries_sim=dict(seed=108, genome_len=60_000, coverage=12, kind="pb_raw", read_seed=9),
         min_read_len=0, min_overlap=100, only_max=False, max_overhang=0, nucl_aln=False, minimizer_index=True),
    dict(name="edges_raw_max", preset="raw",
         sim=dict(seed=110, genome_len=50_000, coverage=4, kind="hifi03", median_len=12000, min_len=5000,
                  max_len=30000, read_seed=7, n_repeat_families=10),
         queries_sim=dict(seed=110, genome_len=50_000, coverage=10, kind="ont_raw", read_seed=9, n_repeat_families=10),
         min_read_len=0, min_overlap=100, only_max=False, max_overhang=0, nucl_aln=False, minimizer_index=True,
         max_overlaps=4),
    dict(name="edges_hifi", preset="hifi",
         sim=dict(seed=109, genome_len=60_000, coverage=3, kind="hifi03", median_len=20000, min_len=8000,
                  max_len=30000, read_seed=7, n_repeat_families=8),
         queries_sim=dict(seed=109, genome_len=60_000, coverage=10, kind="hifi", read_seed=9, n_repeat_families=8),
         min_read_len=0, min_overlap=1000, only_max=False, max_overhang=0, nucl_aln=False, minimizer_index=True),
    # keepAlignment = true (kmerMatches of every overlap; the files hold count + digest per
    # overlap, oracle.py match_hashes): the ReadAligner flag set in full (read_aligner.cpp:186-192)
    # and an assemble-style run with the chains kept
    dict(name="edges_raw_aln", preset="raw",
         sim=dict(seed=111, genome_len=60_000, coverage=3, kind="hifi03", median_len=20000, min_len=8000,
                  max_len=30000, read_seed=7, n_repeat_families=6),
         queries_sim=dict(seed=111, genome_len=60_000, coverage=10, kind="ont_raw", read_seed=9, n_repeat_families=6),
         min_read_len=0, min_overlap=100, only_max=False, max_overhang=0, nucl_aln=False, minimizer_index=True,
         keep_aln=True),
    dict(name="edges_hifi_aln", preset="hifi",
         sim=dict(seed=112, genome_len=50_000, coverage=3, kind="hifi03", median_len=20000, min_len=8000,
                  max_len=30000, read_seed=7, n_repeat_families=8, n_tandems=30),
         queries_sim=dict(seed=112, genome_len=50_000, coverage=8, kind="hifi", read_seed=9, n_repeat_families=8,
                          n_tandems=30),
         min_read_len=0, min_overlap=1000, only_max=False, max_overhang=0, nucl_aln=False, minimizer_index=True,
         keep_aln=True),
    dict(name="raw_pb_aln", preset="raw", sim=dict(seed=113, genome_len=40_000, coverage=25, kind="pb_raw"),
         min_read_len=1000, keep_aln=True),
    # RepeatGraph::build flag set (repeat_graph.cpp:72-97): the assembled sequences against
    # themselves, all-k-mer / minimizer index with min coverage 1, no overhang check, every primary,
    # kmerMatches kept, base-level divergence with the gate applied.  (partitionBadMappings is off in
    # the reference run: its ksw2 step is outside the path; the library returns the gated-out
    # primaries marked instead, tested against these vectors + a max_div = 1 run.)
    dict(name="repeat_raw", preset="raw",
         sim=dict(seed=114, genome_len=60_000, coverage=4, kind="hifi03", median_len=15000, min_len=6000,
                  max_len=30000, n_repeat_families=8),
         min_read_len=0, min_overlap=1000, only_max=False, max_overhang=0, nucl_aln=True, minimizer_index=True,
         keep_aln=True, max_div=0.006),
    dict(name="repeat_raw_all", preset="raw",
         sim=dict(seed=114, genome_len=60_000, coverage=4, kind="hifi03", median_len=15000, min_len=6000,
                  max_len=30000, n_repeat_families=8),
         min_read_len=0, min_overlap=1000, only_max=False, max_overhang=0, nucl_aln=True, minimizer_index=True,
         keep_aln=True, max_div=1.0),
    dict(name="repeat_hifi", preset="hifi",
         sim=dict(seed=115, genome_len=60_000, coverage=4, kind="hifi", median_len=15000, min_len=6000,
                  max_len=30000, n_repeat_families=8, n_homopolymers=40),
         min_read_len=0, min_overlap=1000, only_max=False, max_overhang=0, nucl_aln=True, minimizer_index=True,
         keep_aln=True, max_div=0.015),
    # k-mer sizes other than 17: the wide lookup table (k >= 18), the subassembly preset (k = 31, its own cfg
    # file) and the counter below 17.  ``kmer_size`` overrides the preset's value (--params kmer_size=N); the
    # tandem repeats make some k-mers repetitive at these widths too (index.repetitive_kmers > 0).
    dict(name="subasm", preset="subasm",
         sim=dict(seed=201, genome_len=30_000, coverage=20, kind="hifi", n_tandems=40, n_repeat_families=6),
         min_read_len=1000),
    dict(name="subasm_rc_max", preset="subasm",
         sim=dict(seed=202, genome_len=30_000, coverage=20, kind="hifi03", n_tandems=20, n_homopolymers=20),
         min_read_len=1000, rc_queries=True, max_overlaps=20),
    dict(name="corrected_k18", preset="corrected", kmer_size=18,
         sim=dict(seed=203, genome_len=30_000, coverage=20, kind="hifi03", n_tandems=20, n_homopolymers=10),
         min_read_len=1000),
    dict(name="raw_k15", preset="raw", kmer_size=15,
         sim=dict(seed=204, genome_len=30_000, coverage=20, kind="pb_raw"),
         min_read_len=1000),
    dict(name="edges_subasm_aln", preset="subasm",
         sim=dict(seed=205, genome_len=40_000, coverage=4, kind="hifi03", median_len=20000, min_len=8000,
                  max_len=30000, read_seed=7, n_repeat_families=6, n_tandems=8),
         queries_sim=dict(seed=205, genome_len=40_000, coverage=8, kind="hifi", read_seed=9, n_repeat_families=6,
                          n_tandems=8),
         min_read_len=0, min_overlap=1000, only_max=False, max_overhang=0, nucl_aln=False, minimizer_index=True,
         keep_aln=True),
    dict(name="repeat_subasm", preset="subasm",
         sim=dict(seed=206, genome_len=40_000, coverage=4, kind="hifi03", median_len=15000, min_len=6000,
                  max_len=30000, n_repeat_families=8),
         min_read_len=0, min_overlap=1000, only_max=False, max_overhang=0, nucl_aln=True, minimizer_index=True,
         keep_aln=True, max_div=0.03),
]


def index_digest(ix):
    h = hashlib.sha256()
    for a in (ix.keys, ix.key_off, ix.entries, ix.repetitive):
        h.update(np.ascontiguousarray(a, np.uint64).tobytes())
    return h.hexdigest()


def main():
    assert O.have_ref(), "oracle/_ref/ref_dumper missing: make -C oracle ref"
    only = set(sys.argv[1:])
    meta_path = os.path.join(HERE, "cases.json")
    meta = json.load(open(meta_path)) if os.path.exists(meta_path) else {}
    for case in CASES:
        name = case["name"]
        if only and name not in only:
            continue
        with tempfile.TemporaryDirectory() as tmp:
            fa = os.path.join(tmp, "reads.fasta")
            rs = synth.simulate(fasta_path=fa, **case["sim"]).filter_min_len(case["min_read_len"])
            extra = {}
            params = []
            if "kmer_size" in case:
                params.append(f"kmer_size={int(case['kmer_size'])}")
            if case.get("minimizer_index"):
                cfgd = config.preset(case["preset"])
                wnd = int(cfgd["minimizer_window"]) if cfgd["use_minimizers"] else 1
                params.append(f"use_minimizers=1,minimizer_window={wnd}")     # read_aligner.cpp:180-182
                extra = dict(only_max=case["only_max"], max_overhang=case["max_overhang"],
                             nucl_aln=case["nucl_aln"], min_overlap=case["min_overlap"])
                if "max_div" in case:
                    extra["max_div"] = case["max_div"]
                if "queries_sim" in case:
                    qfa = os.path.join(tmp, "queries.fasta")
                    synth.simulate(fasta_path=qfa, **case["queries_sim"])
                    extra["queries_fasta"] = qfa
            info = O.run_ref(fa, config=CFG_DIR + config.CFG_FILES[case["preset"]], params_string=",".join(params) or None, threads=8,
                             min_read_len=case["min_read_len"], max_overlaps=case.get("max_overlaps", 0),
                             force_local=case.get("force_local", False),
                             div_mode=case.get("div_mode", "none"),
                             index_out=os.path.join(tmp, "index.txt"), ovlp_out=os.path.join(tmp, "ovlp.txt"),
                             rc_queries=case.get("rc_queries", False), keep_aln=case.get("keep_aln", False),
                             **extra)
            hdr, ix = O.parse_ref_index(os.path.join(tmp, "index.txt"), rs)
            lines = open(os.path.join(tmp, "ovlp.txt")).read()
            first = lines.split("\n", 1)[0].split()
            ovhdr = {first[i]: first[i + 1] for i in range(1, len(first), 2)}
            with gzip.GzipFile(os.path.join(HERE, name + ".ovlp.gz"), "wb", mtime=0) as f:
                f.write(lines.encode())
            entry = dict(case)
            entry.update(n_reads=rs.n, total_bases=rs.total_bases,
                         reads_sha256=hashlib.sha256(rs.words.tobytes() + rs.length.tobytes()).hexdigest(),
                         index=dict(sample_rate_bits=hdr["sampleRateBits"], repetitive_frequency=int(hdr["repFreq"]),
                                    total_kmers=int(hdr["numKmers"]), selected_kmers=int(hdr["keys"]),
                                    repetitive_kmers=int(hdr["rep"]), index_entries=int(len(ix.entries)),
                                    sha256=index_digest(ix)),
                         max_div_bits=ovhdr["maxDivBits"], mean_div_bits=ovhdr["meanDivBits"],
                         n_overlaps=info["overlaps"])
            meta[name] = entry
            print(name, "reads", rs.n, "overlaps", info["overlaps"], "ref overlap_s", info["overlap_s"], flush=True)
    json.dump(meta, open(meta_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
