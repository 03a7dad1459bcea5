"""The ordered task pass with a chained prefix (flye_amd/csrc/fg_taskchain.h, host only): bases, order, totals and
the way a failing task ends the pass, under several threads.  Built with the thread sanitizer where the toolchain
has its runtime, plainly otherwise."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_task_chain_under_threads(tmp_path):
    src = os.path.join(ROOT, "tests", "native", "task_chain_driver.cpp")
    exe = str(tmp_path / "task_chain_driver")
    base = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-I", os.path.join(ROOT, "flye_amd", "csrc"), src, "-o", exe]
    tsan = subprocess.run(base + ["-fsanitize=thread"], capture_output=True, text=True)
    if tsan.returncode != 0:
        assert "tsan" in tsan.stderr.lower() or "sanitize" in tsan.stderr.lower(), tsan.stderr    # a real compile error
        subprocess.run(base, check=True)
    # where address-space randomisation is incompatible with the sanitizer's shadow memory the plain build stands in
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66"))
    if tsan.returncode == 0 and run.returncode not in (0, 1, 66) or "unexpected memory mapping" in run.stderr:
        subprocess.run(base, check=True)
        run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr[-4000:])
