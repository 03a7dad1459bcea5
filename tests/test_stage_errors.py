"""The host frame the stage calls share (flye_amd/csrc/fg_stage.h).

1. On the device: every variant of tests/stage_error_cases.py on each of the nine calls against
   tests/golden/stage_errors.json, the codes and fg_last_error texts recorded from the library of ONE commit (named in the
   file; made by tests/golden/make_stage_errors_golden.py and never re-recorded from later code): the valid input gives 0,
   a variant gives its code and, byte for byte, its text (the two-fault variants pin which fault a call reports), *out is
   all zero after an error, and the valid call afterwards still gives the first result.
2. Without a device: tests/stage_host_check.cpp, a program over the host part of the header alone (g++, no HIP): the cut
   against a restatement of its rule, the argument checks, the switch readers."""
import json
import os
import subprocess

import pytest

import stage_error_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "stage_errors.json")))
FG_ERR_HIP, FG_ERR_ARG, FG_ERR_NOMEM = -2, -3, -8


def test_the_input_is_the_one_the_issue_describes():
    A = S.inputs()
    assert list(A["contig_len"]) == [60, 48, 72] and list(A["contig_aln_off"]) == [0, 3, 3, 5]
    widths = [int(b) - int(a) for a, b in zip(A["col_off"], A["col_off"][1:])]
    assert len(widths) == 5 and all(30 <= w <= 120 for w in widths)
    assert ord("-") in A["trg_cols"] and ord("-") in A["qry_cols"]
    assert list(A["job_edge_off"]) == [0, 2, 4]


def test_every_call_has_its_variants_recorded():
    assert sorted(GOLDEN["calls"]) == sorted(S.CALLS) and len(GOLDEN["recorded_at_commit"]) >= 7
    for call in S.CALLS:
        names = [name for name, _, _ in S.variants(call)]
        assert len(set(names)) == len(names) and sorted(names) == sorted(GOLDEN["calls"][call]), call
        want = GOLDEN["calls"][call]
        assert want["null:out"]["code"] == FG_ERR_ARG
        assert all(v["code"] != FG_ERR_HIP and (v["text"] is None) == (v["code"] == 0) for v in want.values()), call
        if "budget" in want:
            assert want["budget"]["code"] == FG_ERR_NOMEM and S.CALLS[call][6] in want["budget"]["text"]
    for call in S.TAKES_COLUMNS:
        assert {"two:trg_start+byte128", "two:col_off+contig_len"} <= set(GOLDEN["calls"][call])


@pytest.fixture(scope="module")
def ctx(built):
    from flye_amd import gpu
    c = gpu.Context(17, 0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("call", sorted(S.CALLS))
def test_codes_and_texts_are_the_recorded_ones(ctx, call, monkeypatch):
    from flye_amd import gpu
    lib = gpu.load_library()
    want = GOLDEN["calls"][call]
    first = S.run_wrapped(ctx, call)
    assert S.run_raw(lib, ctx, call)[0] == 0
    for name, changed, env in S.variants(call):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)
            rc, text, zero = S.run_raw(lib, ctx, call, changed)
        print(call, name, rc, repr(text) if rc else "")
        assert rc == want[name]["code"], (name, rc, text)
        if want[name]["text"] is not None:
            assert text == want[name]["text"], name
        if rc != 0 and zero is not None:
            assert zero, name + ": *out is not all zero after the error"
        assert S.run_wrapped(ctx, call).same_as(first), name + ": the valid call no longer gives the first result"


def test_host_part_of_the_header_alone(tmp_path):
    exe = str(tmp_path / "stage_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "stage_host_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "stage_host_check ok" in r.stdout
