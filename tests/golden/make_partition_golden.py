"""Generates the fixtures of tests/test_partition.py: what the UNMODIFIED Python of the reference (flye.trestle.trestle,
imported from the reference tree, nothing of it copied) does with the inputs of tests/partition_restate.py.  Stored, as
data only:
* per generated confirm job, the sha256 of the eight lists and of the per-edge consensus_pos lists _evaluate_positions
  returns; per generated classify job, the sha256 of the four per-read arrays read from _classify_reads' rows and of the
  per-alignment scores (each alignment alone through _classify_reads at buffer 0); the sha256 of the generated input
  (partition_cases.json);
* per SAM-file run, the confirmed-positions and partitioning files the reference's own partition_reads leaves
  (partition_<run>.confirmed.gz, partition_<run>.part.gz).

    python tests/golden/make_partition_golden.py            # the fixtures
    python tests/golden/make_partition_golden.py --time     # also: the reference's _classify_reads time on the input of
                                                            # tools/partition_bench.py
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

import partition_restate as P  # noqa: E402
import flye.trestle.trestle as ref  # noqa: E402

SIDES = ("in", "out")


def put(name, text):
    path = os.path.join(HERE, name)
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(text.encode("latin-1"))
    assert os.path.getsize(path) <= 64 * 1024, (name, os.path.getsize(path))


def reference_confirm(job):
    cons_aligns = collections.OrderedDict((i, a) for i, a in enumerate(job["edges"]))
    confirmed, rejected, cons = ref._evaluate_positions(job["pos"], cons_aligns, SIDES[job["side"]])
    res = {pre + k: d[k] for pre, d in (("conf_", confirmed), ("rej_", rejected)) for k in P.LIST_KEYS}
    for k in P.CONFIRM_KEYS:
        assert res[k] == sorted(res[k])
    res["cons"] = [cons[i] for i in range(len(job["edges"]))]
    return res


def reference_rows(job, buffer_count):
    headers = collections.OrderedDict(("read_%d" % r, r) for r in range(job["n_reads"]))
    read_aligns = collections.OrderedDict((e, [edge["alns"]]) for e, edge in enumerate(job["edges"]))
    rows = ref._classify_reads(read_aligns, {e: edge["pos"] for e, edge in enumerate(job["edges"])}, headers, buffer_count)
    assert [r[0] for r in rows] == list(range(job["n_reads"]))
    return rows


def reference_classify(job, buffer_count):
    rows = reference_rows(job, buffer_count)
    res = dict(status=[P.STATUS.index(r[1]) for r in rows], top_edge=[int(r[2]) if r[2] != "NA" else -1 for r in rows],
               top_score=[r[3] for r in rows], total_score=[r[4] for r in rows], aln_score=[])
    for edge in job["edges"]:
        for a in edge["alns"]:
            alone = dict(n_reads=job["n_reads"], edges=[dict(pos=edge["pos"], alns=[a])])
            res["aln_score"].append(reference_rows(alone, 0)[P.read_number(a)][4])
    return res


def run_partition_reads(run):
    with tempfile.TemporaryDirectory() as tmp:
        args = P.write_files(run, tmp)
        ref.partition_reads(run["edges"], run["it"], run["side"], **args)
        texts = dict(confirmed=open(args["confirmed_pos_path"].format(run["it"], run["side"])).read(),
                     part=open(args["part_file"].format(run["it"], run["side"])).read())
    return texts


def main():
    cases = dict(confirm={}, classify={}, sams={})
    for name, make in sorted(P.CONFIRM_RUNS.items()):
        run = make()
        jobs = []
        for job in run["jobs"]:
            res = reference_confirm(job)
            jobs.append(dict(lists_sha256=P.digests(res, P.CONFIRM_KEYS), cons_sha256=P.cons_digest(res["cons"]),
                             n=[len(res[k]) for k in P.CONFIRM_KEYS] + [sum(len(c) for c in res["cons"])]))
        cases["confirm"][name] = dict(input_sha256=P.confirm_digest(run), jobs=jobs)
        print(name, [j["n"] for j in jobs], flush=True)
    for name, make in sorted(P.CLASSIFY_RUNS.items()):
        run = make()
        jobs = []
        for job in run["jobs"]:
            res = reference_classify(job, run["buffer_count"])
            jobs.append(dict(arrays_sha256=P.digests(res, P.READ_KEYS + ("aln_score",)), statuses=[res["status"].count(k) for k in range(3)]))
        cases["classify"][name] = dict(input_sha256=P.classify_digest(run), buffer_count=run["buffer_count"], jobs=jobs)
        print(name, [j["statuses"] for j in jobs], flush=True)
    for name, make in sorted(P.SAMS.items()):
        run = make()
        texts = run_partition_reads(run)
        for k, text in texts.items():
            put("partition_%s.%s.gz" % (name, k), text)
        cases["sams"][name] = dict(input_sha256=P.sam_digest(run), lines=[texts["confirmed"].count("\n"), texts["part"].count("\n")])
        print(name, cases["sams"][name]["lines"], texts["confirmed"].split("\n")[0], flush=True)
    path = os.path.join(HERE, "partition_cases.json")
    json.dump(cases, open(path, "w"), separators=(",", ":"), sort_keys=True)
    assert os.path.getsize(path) <= 64 * 1024, os.path.getsize(path)
    if "--time" in sys.argv:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from partition_bench import bench_input
        run = bench_input()
        job, = run["jobs"]
        t0 = time.perf_counter()
        rows = reference_rows(job, run["buffer_count"])
        t1 = time.perf_counter()
        print("reference trestle.py, one process: %d edges, %d alignments, %d columns, %d positions: _classify_reads %.2f s, "
              "None / Tied / Partitioned %s" %
              (len(job["edges"]), sum(len(e["alns"]) for e in job["edges"]), sum(len(a.trg_seq) for e in job["edges"] for a in e["alns"]),
               sum(len(e["pos"]) for e in job["edges"]), t1 - t0, [sum(1 for r in rows if r[1] == s) for s in P.STATUS]), flush=True)


if __name__ == "__main__":
    main()
