"""Generates the fixtures of tests/test_polish.py: what the UNMODIFIED polisher of the reference (src/polishing/*.cpp,
compiled here into a temporary directory with a two-line main, and removed again) does with the bubble files of
tests/polish_restate.py.  Stored, as data only: the bubble files (polish_*.fa.gz), the reference's consensus files
(polish_*.cons.gz), its --debug step logs (polish_*.log.gz), polish_cases.json, and the matrix files under bin_cfg/
(two copied from the reference's configuration, tie.mat and pos.mat ours).

    python tests/golden/make_polish_golden.py            # the fixtures
    python tests/golden/make_polish_golden.py --time     # also: the reference's time on the bubbles of tools/polish_bench.py

The reference assigns `true` to the std::string that names the log, so with --debug the log lands in a file whose name
is the byte 0x01, in the working directory."""
import glob
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import polish_restate as PR  # noqa: E402

REF = os.environ.get("FLYE_REFERENCE", "/root/reference")
CFG = os.path.join(REF, "flye", "config", "bin_cfg")
FLAGS = ["-O3", "-DNDEBUG", "-std=c++11", "-fsigned-char", "-pthread", "-w"]
MAIN = "int polisher_main(int argc, char* argv[]);\nint main(int argc, char* argv[]) { return polisher_main(argc, argv); }\n"

TIE_MAT = "".join(["mat\t%s\t0.9\n" % x for x in "ACTG"] +
                  ["mis\t%s->%s\t0.01\n" % (x, y) for x in "ACTG" for y in "ACTG" if x != y] +
                  ["del\t%s\t0.03\n" % x for x in "ACTG"] + ["ins\t%s\t0.02\n" % x for x in "ACTG"])


def build(tmp):
    with open(os.path.join(tmp, "main.cpp"), "w") as f:
        f.write(MAIN)
    exe = os.path.join(tmp, "polisher")
    src = sorted(glob.glob(os.path.join(REF, "src", "polishing", "*.cpp")))
    subprocess.run(["g++"] + FLAGS + ["-I", os.path.join(REF, "src")] + src + [os.path.join(tmp, "main.cpp"), "-o", exe], check=True)
    return exe


def run(exe, tmp, text, matrix, threads=1, debug=True):
    """-> (consensus text, log text, seconds, stderr)"""
    work = tempfile.mkdtemp(dir=tmp)
    with open(os.path.join(work, "bubbles.fa"), "w", encoding="latin-1") as f:
        f.write(text)
    cmd = [exe, "--bubbles", "bubbles.fa", "--subs-mat", matrix, "--hopo-mat", os.path.join(CFG, "pacbio_homopolymers.mat"),
           "--out", "cons.fa", "--threads", str(threads), "--quiet"] + (["--debug"] if debug else [])
    t0 = time.perf_counter()
    r = subprocess.run(cmd, cwd=work, check=True, capture_output=True)
    dt = time.perf_counter() - t0
    cons = open(os.path.join(work, "cons.fa"), encoding="latin-1").read()
    log = open(os.path.join(work, "\x01"), encoding="latin-1").read() if debug else ""
    return cons, log, dt, r.stderr.decode("latin-1")


def put(name, text):
    data = text.encode("latin-1")
    path = os.path.join(HERE, name)
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(data)
    assert os.path.getsize(path) <= 64 * 1024, (name, os.path.getsize(path))


def main():
    cfg_out = os.path.join(HERE, "bin_cfg")
    for m in ("pacbio_substitutions.mat", "nano_r94_substitutions.mat"):
        shutil.copyfile(os.path.join(CFG, m), os.path.join(cfg_out, m))
    with open(os.path.join(cfg_out, "tie.mat"), "w") as f:
        f.write(TIE_MAT)
    with open(os.path.join(cfg_out, "pos.mat"), "w") as f:
        f.write(open(os.path.join(CFG, "pacbio_substitutions.mat")).read().replace("mat\tA\t0.9582463498", "mat\tA\t1.5"))
    tmp = tempfile.mkdtemp()
    try:
        exe = build(tmp)
        meta = {}
        for name, (matrix, make) in PR.RUNS.items():
            bubbles = make()
            text = PR.write_bubbles(bubbles)
            cons, log, dt, err = run(exe, tmp, text, os.path.join(cfg_out, matrix))
            put(name + ".fa.gz", text)
            put(name + ".cons.gz", cons)
            put(name + ".log.gz", log)
            lens = [sorted(len(w) for w in b.branches) for b in bubbles]
            meta[name] = dict(matrix=matrix, n_bubbles=len(bubbles), n_steps=log.count("Consensus: "),
                              more_than_10=sum(1 for b in bubbles if len(b.branches) > 10),
                              more_than_16=sum(1 for b in bubbles if len(b.branches) > 16),
                              more_than_16_with_length_ties=sum(1 for l in lens if len(l) > 16 and len(set(l)) < len(l)),
                              overflow_messages=err.count("Overflow!"), iteration_limit_messages=err.count("Too many iters!"))
            print(name, meta[name], "%.1f s" % dt, flush=True)
        json.dump(meta, open(os.path.join(HERE, "polish_cases.json"), "w"), indent=1, sort_keys=True)
        if "--time" in sys.argv:
            text = PR.write_bubbles(PR.generate_fast(2024, 2000))     # the first 2000 bubbles of tools/polish_bench.py
            for threads in (1, 16):
                _, _, dt, _ = run(exe, tmp, text, os.path.join(cfg_out, "pacbio_substitutions.mat"), threads=threads, debug=False)
                print("reference polisher, 2000 bubbles (generate_fast, seed 2024), %d thread(s): %.1f s" % (threads, dt),
                      flush=True)
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
