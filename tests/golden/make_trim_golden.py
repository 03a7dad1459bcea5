"""Generates tests/golden/trim_repeat_raw*.ovlp.gz: getSeqOverlaps of the UNMODIFIED reference (oracle/_ref/ref_dumper,
plain per-read mode) on the reads of the repeat_raw case with RepeatGraph::build's detector and partitionBadMappings ON,
so that every primary that fails the divergence gate is replaced by what the reference's own checkIdyAndTrim
(src/sequence/alignment.cpp:306-495) keeps of it -- once as is and once with hpc_scoring_on=1.  Only recorded results
are stored.

    python tests/golden/make_trim_golden.py
"""
import gzip
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from flye_amd import config, synth  # noqa: E402
from oracle import oracle as O  # noqa: E402

CFG_DIR = "/root/reference/flye/config/bin_cfg/"
MAX_DIV = 0.006
VARIANTS = {"trim_repeat_raw": "", "trim_repeat_raw_hpc": ",hpc_scoring_on=1"}


def main():
    assert O.have_ref(), "oracle/_ref/ref_dumper missing: make -C oracle ref"
    case = json.load(open(os.path.join(HERE, "cases.json")))["repeat_raw"]
    cfgd = config.preset(case["preset"])
    wnd = int(cfgd["minimizer_window"]) if cfgd["use_minimizers"] else 1
    meta = {}
    for name, extra in VARIANTS.items():
        with tempfile.TemporaryDirectory() as tmp:
            fa = os.path.join(tmp, "reads.fasta")
            synth.simulate(fasta_path=fa, **case["sim"]).filter_min_len(case["min_read_len"])
            params = f"use_minimizers=1,minimizer_window={wnd}" + extra
            out = os.path.join(tmp, "ovlp.txt")
            info = O.run_ref(fa, config=CFG_DIR + config.CFG_FILES[case["preset"]], params_string=params, threads=8,
                             min_read_len=case["min_read_len"], min_overlap=case["min_overlap"], partition_bad=True,
                             max_div=MAX_DIV, nucl_aln=1, only_max=0, max_overhang=0, keep_aln=True, ovlp_out=out)
            text = open(out).read()
            with gzip.GzipFile(os.path.join(HERE, name + ".ovlp.gz"), "wb", mtime=0) as f:
                f.write(text.encode())
            n = sum(1 for l in text.splitlines() if l.strip() and not l.startswith("#"))
            meta[name] = dict(case="repeat_raw", params=params, max_div=MAX_DIV, min_overlap=case["min_overlap"],
                              nucl_aln=1, only_max=0, max_overhang=0, keep_aln=1, partition_bad=1,
                              use_hpc=int(bool(extra)), n_records=n, n_overlaps=info["overlaps"])
            print(name, meta[name], flush=True)
    json.dump(meta, open(os.path.join(HERE, "trim_cases.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
