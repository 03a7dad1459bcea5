"""fg_paf_groups / fg_paf_circular / fg_components / fg_paf_parse and gpu.PlasmidFinder: the short-plasmid rescue
(reference flye/short_plasmids/).  Without a GPU: the restatement of tests/plasmid_restate.py against what the
unmodified reference gave (tests/golden/plasmid_cases.json.gz, made by tests/golden/make_plasmid_golden.py), the
tokeniser against Python's, the ABI.  With a GPU: every output array of the device calls against the restatement, on
crafted inputs at the edges of every size class and tile, on fuzzed inputs along every route, and the mirror's results
against the goldens byte for byte.

The issue's "cover above 2^31 from two disjoint segments of about 1.1e9 each" cannot be formed: coordinates are int32,
so disjoint segments hold at most 2^31 - 1 bases between them.  COVER_ROWS keeps the two segments (1.1e9 and 1.05e9
bases, cover 2^31 - 1) and adds the touching pair over 0 .. 2^31 - 1, whose cover 2^31 does not fit 32 bits."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import plasmid_restate as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("FG_PAF_WAVE_MAX", "FG_PAF_WG_MAX", "FG_PAF_TILE")
NEW_SYMBOLS = ["fg_paf_groups", "fg_release_paf_groups", "fg_paf_circular", "fg_release_paf_circular", "fg_components",
               "fg_paf_parse", "fg_release_paf_text"]


@pytest.fixture(scope="module")
def golden():
    return PR.stored_golden()


# ---- without a GPU ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PR.CASES))
def test_restatement_equals_the_reference(golden, name):
    case, g, (unmapped_thr, unique_thr, min_len) = PR.stored_case(name), golden[name], PR.PARAMS[name]
    assert PR.sha(case["paf"]) == g["paf_sha256"] and PR.sha(case["fasta"]) == g["fasta_sha256"]
    assert PR.mapping_rates(case["paf"]) == g["mapping_rates"]
    circ, pairs = PR.circular_reads(case["paf"]), PR.circular_pairs(case["paf"])
    assert circ == g["circular_reads"]
    assert pairs == g["circular_pairs"]
    text, total, unmapped = PR.unmapped_fasta(case["fasta"], case["paf"], unmapped_thr)
    assert (PR.sha(text), total, unmapped) == (g["unmapped_sha256"], g["total_bases"], g["unmapped_bases"])
    seqs = PR.read_fasta(case["fasta"])
    assert PR.sha(json.dumps(PR.trimmed_reads(circ, seqs), sort_keys=True)) == g["trimmed_reads_sha256"]
    assert PR.sha(json.dumps(PR.trimmed_pairs(pairs, seqs), sort_keys=True)) == g["trimmed_pairs_sha256"]
    unique = PR.unique_plasmids(case["paf"], case["fasta"], g["vertex_order"], unique_thr, min_len)
    assert unique == g["unique_plasmids"] and list(unique) == list(g["unique_plasmids"])


def test_golden_inputs_are_the_generators(golden):
    """the stored files are what tests/plasmid_restate.py generates (the maker and the tests read the same input)"""
    for name, make in PR.CASES.items():
        assert PR.sha(make()["paf"]) == golden[name]["paf_sha256"], name


def test_closed_form_of_the_cover():
    """the sum the kernels form equals the union, also with the segments shuffled"""
    rng = np.random.RandomState(3)
    for _ in range(300):
        n = int(rng.randint(1, 12))
        s = rng.randint(0, 60, n)
        e = s + rng.randint(0, 25, n)
        pairs = sorted(zip(s.tolist(), e.tolist()), key=lambda p: p[0])
        total, m = 0, -1
        for a, b in pairs:
            total += max(0, b - max(m, a - 1))
            m = max(m, b)
        assert total == PR.united_length(list(zip(s.tolist(), e.tolist())))


@pytest.mark.parametrize("name", sorted(PR.CASES))
def test_paf_parse_equals_python(built, name):
    from flye_amd import gpu
    text = PR.stored_case(name)["paf"]
    tokens = PR.tokenize(text)
    hits, names = PR.to_hits(tokens)
    got = gpu.paf_parse(text)
    assert got.names == names
    assert got.hits.tobytes() == hits.tobytes()
    assert [got.names[i] for i in got.first_seen.tolist()] == PR.first_seen(tokens)


def test_paf_parse_lines_and_blanks(built):
    from flye_amd import gpu
    line = b"q\t10\t1\t2\t+\tt\t20\t3\t4\t9\t9\t60"
    for text in (line, line + b"\n", line.replace(b"\t", b" "), line.replace(b"\t", b" \t ") + b"\r\n",
                 b"  " + line.replace(b"\t", b"\x0b\x0c") + b"\n" + line, line[:line.index(b"\t9")] + b"\n",
                 b"q +10 -1 2 + t 20 3 4\n", b"q 2147483647 -2147483648 2 + t 20 3 4 more fields here\n"):
        got, want = gpu.paf_parse(text), PR.to_hits(PR.tokenize(text))
        assert got.hits.tobytes() == want[0].tobytes() and got.names == want[1], text
    assert len(gpu.paf_parse(b"").hits) == 0


@pytest.mark.parametrize("text,line", [
    (b"q 10 1 2 + t 20 3\n", 1),                                   # a short line
    (b"q 10 1 2 + t 20 3 4\n\nq 10 1 2 + t 20 3 4\n", 2),          # an empty line
    (b"q 10 1 2 + t 20 3 4\n\n", 2),
    (b"q 10 1 2 + t 20 3 4\nq 1e3 1 2 + t 20 3 4\n", 2),
    (b"q 10 1 2 + t 20 3 2147483648\n", 1),                        # 2^31
    (b"q 10 1 2 + t 20 3 -2147483649\n", 1),
    (b"q 10 1 2 + t 20 3 99999999999999999999999\n", 1),
    (b"q 10 1 2 + t 20 - 4\n", 1),
    (b"q 10 0x1 2 + t 20 3 4\n", 1),
    (b"q 10 1. 2 + t 20 3 4\n", 1),
])
def test_paf_parse_refuses(built, text, line):
    from flye_amd import gpu
    try:                                                           # Python refuses the same input, or a value leaves int32
        assert any(not -2 ** 31 <= v < 2 ** 31 for t in PR.tokenize(text) for v in t[2:])
    except (ValueError, IndexError):
        pass
    with pytest.raises(gpu.FlyeGpuError) as e:
        gpu.paf_parse(text)
    assert e.value.code == -3 and ("line %d" % line) in str(e.value)
    assert len(gpu.paf_parse(b"q 10 1 2 + t 20 3 4\n").hits) == 1  # the next call is clean


def test_abi_has_the_plasmid_calls(built):
    from flye_amd import gpu
    lib = gpu.load_library()
    text = open(os.path.join(ROOT, "include", "flye_gpu.h")).read()
    for sym in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % sym, text), sym + " is not declared in include/flye_gpu.h"
        assert hasattr(lib, sym), sym + " is not exported"
        assert sym in gpu.ABI_SYMBOLS
    assert lib.fg_abi_version() == 4 and re.search(r"#define FG_ABI_VERSION 4\b", text)
    assert np.dtype(gpu.PAF_HIT_DTYPE).itemsize == 32 and gpu.PAF_HIT_DTYPE == PR.HIT_DTYPE


# ---- with a GPU ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx(built):
    from flye_amd import gpu
    c = gpu.Context(17, 0)          # no reads, no index: the calls need a device and a stream
    yield c
    c.close()


def same(got, want, label):
    assert sorted(got) == sorted(want), label
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (label, k, got[k].shape, want[k].shape)
        bad = np.flatnonzero(got[k] != want[k])
        assert len(bad) == 0, "%s: %s differs at %s: %s, expected %s" % (label, k, bad[:5], got[k][bad[:5]], want[k][bad[:5]])


def set_switches(monkeypatch, wave=None, wg=None, tile=None):
    for k, v in zip(SWITCHES, (wave, wg, tile)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


# (wave, workgroup, tile): the defaults; every group on a workgroup; everything flat in the smallest tiles; lowered caps
ROUTES = [(None, None, None), (0, None, None), (0, 0, 64), (8, 16, 64), (64, 64, 1024)]


def group(q, t, segments):
    """rows of one group, the same segments on both sides (target side shifted by 7)"""
    return [(q, t, s, e, s + 7, e + 7) for s, e in segments]


BIG = 2147483647
COVER_ROWS = {
    "single": group(0, 1, [(5, 9)]),
    "single_base": group(0, 1, [(0, 0)]),
    "identical": group(0, 1, [(10, 20)] * 3),
    "equal_starts": group(0, 1, [(10, 12), (10, 30), (10, 11), (10, 30)]),
    "nested": group(0, 1, [(0, 100), (10, 20), (30, 99), (100, 100), (50, 101)]),
    "joins_at_end": group(0, 1, [(0, 10), (10, 20)]),
    "no_join_behind_end": group(0, 1, [(0, 10), (11, 20)]),
    "join_and_no_join": group(0, 1, [(40, 50), (0, 10), (51, 60), (10, 15), (16, 16), (60, 61)]),
    "later_start_first": group(0, 1, [(500, 600), (0, 550), (551, 552)]),
    "two_disjoint_large": [(0, 1, 0, 1100000000, 0, 1100000000), (0, 1, 1100000002, BIG, 1100000002, BIG)],
    "cover_of_2_31": [(0, 1, 1100000000, BIG, 0, 1100000000), (0, 1, 0, 1100000000, 1100000000, BIG)],
}


def sized_group(q, t, size, seed):
    rng = np.random.RandomState(seed)
    s = rng.randint(0, 40 * size, size)
    return [(q, t, int(a), int(a + b), int(c), int(c + d)) for a, b, c, d in zip(s, rng.randint(0, 60, size), rng.permutation(s),
                                                                                 rng.randint(0, 90, size))]


def check_groups(ctx, hits, label):
    same(ctx.paf_groups(hits), PR.groups(hits), label)


@pytest.mark.gpu
def test_crafted_covers(ctx, monkeypatch):
    for route in ROUTES:
        set_switches(monkeypatch, *route)
        for name, rows in COVER_ROWS.items():
            check_groups(ctx, PR.hits_of(rows), "%s, switches %s" % (name, route))
        # all of them as the groups of one file
        rows = [(2 * i, 2 * i + 1) + r[2:] for i, (_, rows) in enumerate(sorted(COVER_ROWS.items())) for r in rows]
        check_groups(ctx, PR.hits_of(rows), "all crafted covers, switches %s" % (route,))
    hits = PR.hits_of(COVER_ROWS["cover_of_2_31"])
    set_switches(monkeypatch)
    got = ctx.paf_groups(hits)
    assert got["query_cover"].tolist() == [1 << 31] and got["target_cover"].tolist() == [1 << 31]


@pytest.mark.gpu
def test_group_sizes_at_the_class_edges(ctx, monkeypatch):
    def rows_of(sizes):
        return [r for i, n in enumerate(sizes) for r in sized_group(i, i + 1, n, 100 + n)]
    set_switches(monkeypatch)
    check_groups(ctx, PR.hits_of(rows_of([1, 2, 63, 64, 65, 1023, 1024, 1025])), "default classes")
    assert {"k_paf_cover_wave", "k_paf_cover_wg", "k_paf_cover_flat"} <= set(ctx.kernel_times())
    set_switches(monkeypatch, 8, 16, 64)
    check_groups(ctx, PR.hits_of(rows_of([7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129])), "caps 8 and 16, tiles of 64")
    assert {"k_paf_cover_wave", "k_paf_cover_wg", "k_paf_cover_flat"} <= set(ctx.kernel_times())
    set_switches(monkeypatch, 0, 0, 64)
    check_groups(ctx, PR.hits_of(rows_of([1, 63, 64, 65, 2, 128, 1])), "flat alone, tiles of 64")
    assert not {"k_paf_cover_wave", "k_paf_cover_wg"} & set(ctx.kernel_times())


@pytest.mark.gpu
def test_flat_route_carries_across_tiles(ctx, monkeypatch):
    """tiles of 64: a group that starts mid-tile and spans four tiles, its largest end on its first segment, so the
    carry of the first tile has to pass through two whole tiles; then the same with the large end in the second tile"""
    set_switches(monkeypatch, 0, 0, 64)
    for big_at in (0, 30):
        rows = sized_group(0, 1, 40, 1)
        body = [(10 * i, 10 * i + 5) for i in range(200)]
        body[big_at] = (10 * big_at, 1000000)
        rng = np.random.RandomState(2)
        rows += [(2, 3, s, e, s, e) for s, e in (body[i] for i in rng.permutation(200))]
        rows += sized_group(4, 5, 70, 3)
        hits = PR.hits_of(rows)
        want = PR.groups(hits)
        assert want["query_cover"][1] == 6 * big_at + 1000000 - 10 * big_at + 1     # 6 bases per segment before it, then one stretch
        same(ctx.paf_groups(hits), want, "carry from segment %d" % big_at)
    # a tile boundary exactly at a group boundary, and a group of exactly one tile
    check_groups(ctx, PR.hits_of(sized_group(0, 1, 64, 4) + sized_group(2, 3, 64, 5) + sized_group(4, 5, 1, 6)), "groups of one tile")


@pytest.mark.gpu
def test_grouping(ctx, monkeypatch):
    set_switches(monkeypatch)
    seg = (1, 2, 3, 4)
    cases = {
        "a query in two runs": [(5, 1) + seg, (6, 1) + seg, (5, 1) + seg, (5, 1) + seg],
        "targets out of order": [(5, 9) + seg, (5, 2) + seg, (5, 9) + seg, (5, 0) + seg, (5, 2) + seg, (4, 3) + seg, (4, 1) + seg],
        "self groups": [(3, 3) + seg, (3, 2) + seg, (3, 3) + seg, (2, 2) + seg, (2, 3) + seg],
        "sparse ids": [(1000000, 7) + seg, (1000000, 999999) + seg, (0, 999999) + seg],
    }
    rng = np.random.RandomState(8)
    cases["70 targets in one run"] = [(100, int(t), i, i + 5, 2 * i, 2 * i + 1) for i, t in enumerate(rng.permutation(140) % 70)]
    for name, rows in cases.items():
        hits = PR.hits_of(rows)
        check_groups(ctx, hits, name)
        same(ctx.paf_circular(hits), PR.circular(hits), name + ", circular")
    got = ctx.paf_groups(PR.hits_of(cases["a query in two runs"]))
    assert got["group_off"].tolist() == [0, 1, 2, 4] and got["order"].tolist() == [0, 1, 2, 3]
    got = ctx.paf_groups(PR.hits_of(cases["targets out of order"]))
    assert got["group_target"].tolist() == [0, 2, 9, 1, 3] and got["order"].tolist() == [3, 1, 4, 0, 2, 6, 5]
    empty = ctx.paf_groups(np.zeros(0, PR.HIT_DTYPE))
    assert empty["group_off"].tolist() == [0] and len(empty["order"]) == 0
    assert len(ctx.paf_circular(np.zeros(0, PR.HIT_DTYPE))["pair_ok"]) == 0


def circ(q, qs, qe, ts, te, length=1000):
    return (q, q, qs, qe, ts, te, length, length)


@pytest.mark.gpu
def test_circular_reads(ctx):
    rows = [
        circ(1, 149, 300, 600, 852),            # both overhangs 149: circular
        circ(2, 150, 300, 600, 900),            # query_start == max_overhang
        circ(3, 10, 300, 600, 851),             # target_len - target_end + 1 == max_overhang
        circ(4, 10, 300, 300, 990),             # query_end == target_start
        circ(5, 10, 10, 500, 990),              # query_start == query_end
        circ(6, 10, 300, 600, 600, 700),        # target_start == target_end
        (7, 8, 10, 300, 600, 990, 1000, 1000),  # query != target
        circ(9, 10, 110, 500, 990),
        circ(9, 20, 120, 600, 990),             # equal length: the first stays
        circ(1, 0, 400, 700, 999),              # longer, later: replaces; query 1 keeps its place
        circ(0, 5, 50, 500, 999),
        circ(11, 5, 50, 500, 999),
        circ(0, 5, 60, 500, 999),               # query 0 again in a later run, longer
        circ(11, 5, 40, 500, 999),              # shorter: stays out
    ]
    hits = PR.hits_of(rows)
    want = PR.circular(hits)
    assert want["circ_query"].tolist() == [1, 9, 0, 11] and want["circ_hit"].tolist() == [9, 7, 12, 11]
    same(ctx.paf_circular(hits), want, "circular reads")
    same(ctx.paf_circular(hits, 151, 300), PR.circular(hits, 151, 300), "circular reads, overhang 151")
    # target_len - target_end + 1 near 2^31, and query_len - query_end + 1 == 2^31: 32-bit sums would wrap
    wide = PR.hits_of([(1, 1, 0, 1, 2, 3, 5, BIG), (1, 1, 0, 1, 2, BIG - 10, 5, BIG), (1, 2, 0, 0, 0, 0, BIG, BIG)])
    same(ctx.paf_circular(wide, BIG, BIG), PR.circular(wide, BIG, BIG), "overhangs near 2^31")


def pair(q, t, qs, qe, ts, te):
    return (q, t, qs, qe, ts, te, 1000, 1200)


@pytest.mark.gpu
def test_circular_pairs(ctx):
    A, B = (700, 990, 5, 300), (10, 600, 400, 1100)
    rows = [
        pair(1, 2, *A), pair(1, 2, *B),                          # a pair
        pair(3, 4, *B), pair(3, 4, *A),                          # B before A
        pair(5, 6, 5, 995, 5, 1195),                             # A and B in one hit, alone
        pair(7, 8, 5, 995, 5, 1195), pair(7, 8, *B),             # the A hit is also the first B: the second is the next B
        pair(9, 10, 600, 990, 5, 400), pair(9, 10, 10, 600, 400, 1100),     # second.query_end == first.query_start
        pair(11, 12, 601, 990, 5, 400), pair(11, 12, 10, 600, 400, 1100),   # first.target_end == second.target_start
        pair(13, 14, 601, 990, 5, 399), pair(13, 14, 10, 600, 400, 1100),   # strictly apart: a pair
        pair(15, 16, 702, 990, 299, 300), pair(15, 16, 299, 600, 400, 902),     # every overhang 299
        pair(17, 18, 701, 990, 300, 301), pair(17, 18, 300, 600, 400, 1100),    # target_start == 300; query_start == 300
        pair(19, 20, 500, 701, 5, 300), pair(19, 20, 10, 400, 400, 901),        # query overhang == 300; target overhang == 300
        pair(21, 21, *A), pair(21, 21, *B),                      # query == target
        pair(23, 24, *B), pair(23, 24, *B), pair(23, 24, 200, 300, 500, 600), pair(23, 24, *A), pair(23, 24, *A),
        pair(25, 26, 400, 500, 500, 600),                        # neither
    ]
    hits = PR.hits_of(rows)
    want = PR.circular(hits)
    assert want["pair_ok"].tolist() == [1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0]
    assert want["pair_first"].tolist()[:4] == [0, 3, 4, 5] and want["pair_second"].tolist()[:4] == [1, 2, -1, 6]
    same(ctx.paf_circular(hits), want, "circular pairs")
    same(ctx.paf_circular(hits, 150, 301), PR.circular(hits, 150, 301), "circular pairs, overhang 301")


@pytest.mark.gpu
def test_components(ctx):
    def check(n, u, v, label):
        got, want = ctx.components(n, u, v), PR.components(n, u, v)
        assert got.dtype == np.uint32 and got.tolist() == want.tolist(), label
        return got
    rng = np.random.RandomState(4)
    p = rng.permutation(1000)
    assert set(check(1000, p[:-1], p[1:], "a path numbered at random").tolist()) == {0}
    down = np.arange(999, 0, -1)
    check(1000, down, down - 1, "a path, every edge from the larger vertex, listed from the far end")
    zig = np.array([i // 2 if i % 2 == 0 else 999 - i // 2 for i in range(1000)])       # 0, 999, 1, 998, ...
    check(1000, zig[:-1], zig[1:], "a path against the grain")
    check(501, np.full(500, 500), np.arange(500), "a star around the largest vertex")
    check(6, [1, 1, 4, 4, 2], [1, 1, 4, 5, 2], "self loops")
    check(7, [5, 6, 5, 6, 5, 2, 3, 2], [6, 5, 6, 5, 6, 3, 2, 3], "duplicate edges")
    assert check(5, [], [], "no edges").tolist() == [0, 1, 2, 3, 4]
    assert len(ctx.components(0, [], [])) == 0
    half = 3000
    u = np.concatenate([rng.randint(0, half, 4 * half), half + rng.randint(0, half, 4 * half)])
    v = np.concatenate([rng.randint(0, half, 4 * half), half + rng.randint(0, half, 4 * half)])
    before = check(2 * half, u, v, "two large components")
    after = check(2 * half, np.append(u, 2 * half - 1), np.append(v, 7), "joined by the last edge")
    assert (after <= before).all() and (after != before).any()
    n = 20000
    check(n, rng.randint(0, n, n // 2), rng.randint(0, n, n // 2), "a sparse random graph")


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n,kw", [
    (21, 20000, dict(big_groups=(1500, 1025, 1024, 3000, 65, 64))),
    (22, 30000, dict(n_names=400, max_run=12)),
    (23, 20000, dict(start_values=[0, 3, 50, 51, 100, 150, 151, 299], big_groups=(2100, 300))),     # ties: starts of 8 values
    (24, 5000, dict(n_names=3, max_run=300)),
])
def test_fuzz_every_route(ctx, monkeypatch, seed, n, kw):
    hits = PR.fuzz_hits(seed, n, **kw)
    want = PR.groups(hits)
    for route in ROUTES:
        set_switches(monkeypatch, *route)
        same(ctx.paf_groups(hits), want, "seed %d, switches %s" % (seed, route))
    set_switches(monkeypatch)
    same(ctx.paf_circular(hits), PR.circular(hits), "seed %d, circular" % seed)
    same(ctx.paf_circular(hits, 40, 2000), PR.circular(hits, 40, 2000), "seed %d, circular, other overhangs" % seed)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(PR.CASES))
def test_mirror_equals_the_reference(ctx, golden, tmp_path, name):
    from flye_amd import gpu
    case, g, (unmapped_thr, unique_thr, min_len) = PR.stored_case(name), golden[name], PR.PARAMS[name]
    paf, fasta, out = str(tmp_path / "hits.paf"), str(tmp_path / "reads.fasta"), str(tmp_path / "unmapped.fasta")
    open(paf, "wb").write(case["paf"])
    open(fasta, "wb").write(case["fasta"])
    pf = gpu.PlasmidFinder(ctx)
    assert pf.calc_mapping_rates(paf) == g["mapping_rates"]
    circ, pairs = pf.extract_circular_reads(paf), pf.extract_circular_pairs(paf)
    assert [[k, list(h)] for k, h in circ.items()] == g["circular_reads"]
    assert [[list(p[0]), list(p[1])] for p in pairs] == g["circular_pairs"]
    assert pf.extract_unmapped_reads([fasta], paf, out, unmapped_thr) == (g["total_bases"], g["unmapped_bases"])
    assert PR.sha(open(out, "rb").read()) == g["unmapped_sha256"]
    seqs = dict(pf.stream_sequence(fasta))
    assert PR.sha(json.dumps(pf.trim_circular_reads(circ, seqs), sort_keys=True)) == g["trimmed_reads_sha256"]
    assert PR.sha(json.dumps(pf.trim_circular_pairs(pairs, seqs), sort_keys=True)) == g["trimmed_pairs_sha256"]
    unique = pf.extract_unique_plasmids(paf, fasta, unique_thr, 500, min_len, vertex_order=g["vertex_order"])
    assert unique == g["unique_plasmids"] and list(unique) == list(g["unique_plasmids"])
    # the default order: first appearance in the file
    order = [n.decode() for n in PR.first_seen(PR.tokenize(case["paf"]))]
    assert pf.extract_unique_plasmids(paf, fasta, unique_thr, 500, min_len) == PR.unique_plasmids(case["paf"], case["fasta"], order,
                                                                                                 unique_thr, min_len)


@pytest.mark.gpu
def test_refused_arguments_leave_the_context_usable(ctx):
    from flye_amd import gpu
    good = PR.hits_of(COVER_ROWS["nested"])
    want = PR.groups(good)
    for field, value in (("query_start", -1), ("target_start", -1), ("query_end", 9), ("target_end", 16)):
        bad = good.copy()
        bad[field][1] = value               # row 1 is (10, 20) / (17, 27): an end below its start, or a start below 0
        for call in (ctx.paf_groups, ctx.paf_circular):
            with pytest.raises(gpu.FlyeGpuError) as e:
                call(bad)
            assert e.value.code == -3 and "hit 1" in str(e.value)
            same(ctx.paf_groups(good), want, "after a refused " + field)
    gb, cb = gpu.PafGroupBatch(), gpu.PafCircularBatch()
    assert ctx.L.fg_paf_groups(ctx.h, good.ctypes.data, 1 << 31, C.byref(gb)) == -3 and not gb.owner_
    assert ctx.L.fg_paf_groups(ctx.h, None, 3, C.byref(gb)) == -3
    assert ctx.L.fg_paf_groups(ctx.h, good.ctypes.data, len(good), None) == -3
    assert ctx.L.fg_paf_circular(ctx.h, good.ctypes.data, 1 << 31, 150, 300, C.byref(cb)) == -3 and not cb.owner_
    assert ctx.L.fg_paf_circular(ctx.h, None, 3, 150, 300, C.byref(cb)) == -3
    same(ctx.paf_groups(good), want, "after refused counts and pointers")
    for u, v in (([0, 5], [1, 2]), ([0, 1], [1, 5]), ([4294967295], [0])):
        with pytest.raises(gpu.FlyeGpuError) as e:
            ctx.components(5, u, v)
        assert e.value.code == -3
    labels = np.zeros(3, np.uint32)
    one = np.zeros(1, np.uint32)
    assert ctx.L.fg_components(ctx.h, 3, 1, None, one.ctypes.data, labels.ctypes.data) == -3
    assert ctx.L.fg_components(ctx.h, 3, 0, None, None, None) == -3
    assert ctx.components(5, [0, 3], [1, 4]).tolist() == [0, 0, 2, 3, 3]
    same(ctx.paf_circular(good), PR.circular(good), "circular after the refusals")
