"""Records tests/golden/stage_errors.json: the code and fg_last_error's text of every variant of
tests/stage_error_cases.py, from the library that is loaded (FLYE_GPU_LIB, or the tree's own build) on a machine with a
GPU.  The fixture pins the texts of ONE commit for every later one: it is recorded once, from the library built at the
commit named on the command line, and a change of the host code is checked against it, never recorded from it.
Texts of FG_ERR_HIP are left out (they carry a source line), and so is the text behind a code of 0.

    FLYE_GPU_LIB=<libflyegpu.so built at COMMIT> python tests/golden/make_stage_errors_golden.py COMMIT [output file]
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import stage_error_cases as S  # noqa: E402
from flye_amd import gpu  # noqa: E402

FG_ERR_HIP = -2


def main(commit, path):
    lib, ctx = gpu.load_library(), gpu.Context(17, 0)
    calls = {}
    for call in S.CALLS:
        rc, _, _ = S.run_raw(lib, ctx, call)
        assert rc == 0, (call, rc, lib.fg_last_error(ctx.h))
        calls[call] = {}
        for name, changed, env in S.variants(call):
            os.environ.update(env)
            rc, text, zero = S.run_raw(lib, ctx, call, changed)
            for k in env:
                del os.environ[k]
            assert zero is None or zero == (rc != 0), (call, name, rc, zero)
            calls[call][name] = dict(code=rc, text=None if rc in (0, FG_ERR_HIP) else text)
    ctx.close()
    with open(path, "w") as f:
        json.dump(dict(recorded_at_commit=commit, calls=calls), f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d variants of %d calls -> %s" % (sum(len(v) for v in calls.values()), len(calls), path))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "stage_errors.json"))
