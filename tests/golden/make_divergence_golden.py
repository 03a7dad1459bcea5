"""Generates the fixtures of tests/test_divergence.py: what the UNMODIFIED Python of the reference
(flye.trestle.divergence, imported from the reference tree, nothing of it copied) does with the inputs of
tests/divergence_restate.py.  Stored, as data only:
* per run of generated alignments, the three text files _write_frequency_path, _write_positions and _write_div_summary
  write for its LAST contig (divergence_<run>.<kind>.gz) and, in divergence_cases.json, per contig the sha256 of every
  array read from _count_freqs / _call_position and of its three texts, aln_errors, and the sha256 of the generated input;
* per SAM file, the three text files the reference's own find_divergence leaves at num_proc = 1 (divergence_<sam>.<kind>.gz)
  and the err_rate of the alignments its reader returns on the contigs as its read_sequence_dict reads them.

    python tests/golden/make_divergence_golden.py            # the fixtures
    python tests/golden/make_divergence_golden.py --time     # also: the reference's time on the input of
                                                             # tools/divergence_bench.py
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

import numpy as np  # noqa: E402

import divergence_restate as DR  # noqa: E402
import flye.config.py_cfg as ref_cfg  # noqa: E402
import flye.trestle.divergence as ref_div  # noqa: E402
import flye.utils.fasta_parser as ref_fp  # noqa: E402
from flye.utils.sam_parser import SynchronizedSamReader  # noqa: E402

KINDS = ("frequency", "positions", "summary")
Info = collections.namedtuple("Info", ["length"])


def put(name, text):
    path = os.path.join(HERE, name)
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(text.encode("latin-1"))
    assert os.path.getsize(path) <= 64 * 1024, (name, os.path.getsize(path))


def reference_contig(alns, length, thresholds, tmp):
    """_contig_profile, then the three writers as find_divergence calls them -> (arrays, texts, aln_errors)"""
    s, d, i = thresholds
    profile, aln_errors = ref_div._contig_profile(alns, "pacbio", length)
    paths = {k: os.path.join(tmp, k) for k in KINDS}
    positions = ref_div._write_frequency_path(paths["frequency"], profile, s, d, i)
    heads = ["Total_positions_{0}_with_thresholds_sub_{1}_del_{2}_ins_{3}".format(len(positions["total"]), s, d, i),
             "Sub_positions_{0}_with_threshold_sub_{1}".format(len(positions["sub"]), s),
             "Del_positions_{0}_with_threshold_del_{1}".format(len(positions["del"]), d),
             "Ins_positions_{0}_with_threshold_ins_{1}".format(len(positions["ins"]), i)]
    ref_div._write_positions(paths["positions"], positions, *heads)
    ref_div._write_div_summary(paths["summary"], "Tentative Divergent Position Summary", positions, len(profile), 1000)
    texts = {k: open(p).read() for k, p in paths.items()}
    counts = [ref_div._count_freqs(e) for e in profile]
    byte = lambda s: ord(s) if s else 0
    res = dict(cov=[c["cov"] for c in counts], nucl=[ord(c["mat_base"]) for c in counts], mat_ct=[c["mat_ct"] for c in counts],
               sub_base=[byte(c["sub_base"]) for c in counts], sub_ct=[c["sub_ct"] for c in counts], del_ct=[c["del_ct"] for c in counts],
               ins_base=[byte(c["ins_base"][1:]) for c in counts], ins_ct=[c["ins_ct"] for c in counts])
    in_list = {k: set(positions[k]) for k in DR.LIST_KEYS}
    res["flags"] = [(p in in_list["sub"]) + 2 * (p in in_list["del"]) + 4 * (p in in_list["ins"]) for p in range(length)]
    res = {k: np.array(v, np.uint8 if k in ("nucl", "sub_base", "ins_base", "flags") else np.int32) for k, v in res.items()}
    for k in DR.LIST_KEYS:
        assert positions[k] == sorted(positions[k])
        res[k] = positions[k]
    return res, texts, [float(e) for e in aln_errors]


def run_reference(run):
    meta = dict(input_sha256=DR.input_digest(run), thresholds=list(run["thresholds"]), contigs={})
    texts = None
    with tempfile.TemporaryDirectory() as tmp:
        for contig, _ in run["contigs"]:
            res, texts, aln_errors = reference_contig(run["alns"][contig.id], contig.length, run["thresholds"], tmp)
            meta["contigs"][contig.id] = dict(arrays_sha256=DR.digests(res), texts_sha256=DR.text_digests(texts), aln_errors=aln_errors,
                                              n_called=[len(res[k]) for k in DR.LIST_KEYS])
    return texts, meta


def run_find_divergence(run):
    """the reference's find_divergence on a SAM file and a FASTA file, one worker"""
    s, d, i = run["thresholds"]
    info = {cid: Info(len(seq)) for cid, seq in run["contigs"].items()}
    with tempfile.TemporaryDirectory() as tmp:
        sam, fasta = os.path.join(tmp, "aln.sam"), os.path.join(tmp, "template.fasta")
        with open(sam, "wb") as f:
            f.write(run["sam"])
        with open(fasta, "w") as f:
            f.write(DR.fasta_of(run["contigs"]))
        paths = {k: os.path.join(tmp, k + ".txt") for k in KINDS}
        ref_div.find_divergence(sam, fasta, info, paths["frequency"], paths["positions"], paths["summary"], 0.0, "pacbio", 1, s, d, i)
        texts = {k: open(p).read() for k, p in paths.items()}
        reader = SynchronizedSamReader(sam, ref_fp.read_sequence_dict(fasta), ref_cfg.vals["max_read_coverage"])
        errors, chunks = [], []
        try:
            while True:
                contig, alns = reader.get_chunk()
                if contig is None:
                    break
                chunks.append(contig)
                errors += [float(a.err_rate).hex() for a in alns]
        finally:
            reader.close()
    return texts, dict(input_sha256=DR.sam_digest(run), thresholds=[s, d, i], chunks=chunks, aln_errors=errors,
                       max_read_coverage=ref_cfg.vals["max_read_coverage"])


def main():
    cases = dict(runs={}, sams={})
    for name, make in sorted(DR.RUNS.items()):
        texts, meta = run_reference(make())
        for k in KINDS:
            put("%s.%s.gz" % (name, k), texts[k])
        cases["runs"][name] = meta
        print(name, "contigs", len(meta["contigs"]), "called", [sum(m["n_called"][j] for m in meta["contigs"].values()) for j in range(4)],
              flush=True)
    for name, make in sorted(DR.SAMS.items()):
        texts, meta = run_find_divergence(make())
        for k in KINDS:
            put("divergence_%s.%s.gz" % (name, k), texts[k])
        cases["sams"][name] = meta
        print(name, "chunks", meta["chunks"], "alignments", len(meta["aln_errors"]), flush=True)
    path = os.path.join(HERE, "divergence_cases.json")
    json.dump(cases, open(path, "w"), separators=(",", ":"), sort_keys=True)
    assert os.path.getsize(path) <= 64 * 1024, os.path.getsize(path)
    if "--time" in sys.argv:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from divergence_bench import bench_input
        run = bench_input()
        (contig, _), = run["contigs"]
        alns = run["alns"][contig.id]
        s, d, i = run["thresholds"]
        with tempfile.TemporaryDirectory() as tmp:
            t0 = time.perf_counter()
            profile, _ = ref_div._contig_profile(alns, "pacbio", contig.length)
            t1 = time.perf_counter()
            positions = ref_div._write_frequency_path(os.path.join(tmp, "f"), profile, s, d, i)
            t2 = time.perf_counter()
        print("reference divergence.py, one process: contig of %d bp, %d alignments, %d columns: _contig_profile %.2f s, "
              "_write_frequency_path %.2f s, %d positions called" %
              (contig.length, len(alns), sum(len(a.trg_seq) for a in alns), t1 - t0, t2 - t1, len(positions["total"])), flush=True)


if __name__ == "__main__":
    main()
