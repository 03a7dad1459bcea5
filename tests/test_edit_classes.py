"""The edit-distance kernels of fg_editdist.hip -- O(ND) (k_edit_ond, timed as k_edit_distance), the one-wave banded
bit-vector kernel (k_edit_myers) and its 8-wave form (k_edit_myers_wide) -- on the crafted pairs of tests/edit_craft.py:
both sides of every edge of the hand-over rule (also shrunk by FG_ED_EMAX and FG_ED_LDS_BASES), paths on the band's edge
at every doubling step, strip and block edges, strip counts around the 8 waves, the branches of the homopolymer
compression; batches that give a block a second pair; one slab shared by a long pair and the short ones behind it; the
range caller on both strands.

Everything is an integer compared for equality.  The expected values are what the compiled reference's edlib returned
(tests/golden/edlib_edge_pairs.json, tests/golden/make_edlib_edge_golden.py); the oracle is pinned on them here too.
The route tests say WHICH kernel a pair took: the launched edit kernels of a call on one route's pairs are exactly the
ones edit_craft.route() predicts."""
import json
import os

import numpy as np
import pytest

import edit_craft as E
from helpers import GOLDEN, edit_pair, hpc, pairs_readset

HAVE_REF = os.path.exists(os.path.join(os.path.dirname(GOLDEN), "..", "oracle", "_ref", "ref_dumper"))
PLAIN = ("dist", "n", "m")
HPC = ("hpc_dist", "hpc_n", "hpc_m")


@pytest.fixture(scope="module")
def rows():
    with open(os.path.join(GOLDEN, "edlib_edge_pairs.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def crafted(built):
    """(cases, their strings), built once."""
    cs = E.cases()
    return cs, [E.build(c["spec"]) for c in cs]


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_fixture_describes_the_crafted_cases(crafted, rows):
    cs, pairs = crafted
    assert 300 <= len(cs) <= 450 and len({c["tag"] for c in cs}) == len(cs)
    assert [{k: r[k] for k in ("tag", "env", "use_hpc", "spec")} for r in rows] == json.loads(json.dumps(cs))
    for r, (a, b) in zip(rows, pairs):
        assert (len(a), len(b), len(hpc(a)), len(hpc(b))) == (r["n"], r["m"], r["hpc_n"], r["hpc_m"]), r["tag"]
        assert a.dtype == np.uint8 and b.dtype == np.uint8 and max(a.max(initial=0), b.max(initial=0)) <= 3
        assert max(r["n"], r["m"]) <= 70000


def test_oracle_equals_reference_edlib_on_crafted_cases(crafted, rows):
    from oracle import oracle as O
    for r, (a, b) in zip(rows, crafted[1]):
        assert O.edit_distance(a, b) == r["dist"], r["tag"]
        assert O.edit_distance(hpc(a), hpc(b)) == r["hpc_dist"], r["tag"]


@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref/ref_dumper not built")
def test_oracle_live_against_reference_on_crafted_cases(crafted, rows):
    from oracle import oracle as O
    pairs = crafted[1]
    assert O.ref_edlib_distances(pairs) == [r["dist"] for r in rows]
    assert O.ref_edlib_distances([(hpc(a), hpc(b)) for a, b in pairs]) == [r["hpc_dist"] for r in rows]


def test_oracle_band_doubling_from_the_kernels_starts(crafted, rows):
    """The oracle's banded form from k0 = 64, 1024 and the case's own start gives the fixture's distance."""
    from oracle import oracle as O
    cs, pairs = crafted
    for c, r, (a, b) in zip(cs, rows, pairs):
        emax, lds = E.env_params(c["env"])
        own = E.k0(r["n"], r["m"], max(lds, r["n"], r["m"]), emax, lds)
        assert own in (64, 2 * emax)
        x, y, want = (hpc(a), hpc(b), r["hpc_dist"]) if c["use_hpc"] else (a, b, r["dist"])
        for start in sorted({64, 1024, own}):
            assert O.edit_distance_k0(x, y, start) == want, (r["tag"], start)


def test_route_rule_on_hand_written_triples():
    R = E.route
    big = 1 << 20
    table = [
        # (raw_n, raw_m, dist, container_max_len, emax, lds) -> route
        ((1000, 1000, 512, big, 512, 32768), "ond"), ((1000, 1000, 513, big, 512, 32768), "myers"),
        ((1000, 1512, 512, big, 512, 32768), "ond"), ((1513, 1000, 513, big, 512, 32768), "myers"),
        ((32768, 100, 3, big, 512, 32768), "ond"), ((100, 32769, 3, big, 512, 32768), "myers"),
        ((32768, 32768, 0, 32768, 512, 32768), "ond"), ((32769, 32769, 0, 32769, 512, 32768), "myers"),
        ((49152, 10, 49142, big, 512, 32768), "myers"), ((10, 49153, 49143, big, 512, 32768), "wide"),
        ((49153, 49153, 0, big, 512, 32768), "wide"), ((49153, 1, 49152, big, 512, 1 << 17), "wide"),
        ((49153, 49153, 512, big, 512, 1 << 17), "ond"), ((49153, 49153, 513, big, 512, 1 << 17), "wide"),
        ((300, 300, 8, big, 8, 32768), "ond"), ((300, 300, 9, big, 8, 32768), "myers"),
        ((300, 300, 1, big, 1, 32768), "ond"), ((300, 300, 2, big, 1, 32768), "myers"),
        ((2000, 1990, 40, big, 512, 2000), "ond"), ((2001, 1990, 40, big, 512, 2000), "ond"),
        ((1990, 2048, 40, big, 512, 2000), "ond"), ((2049, 1990, 40, big, 512, 2000), "myers"),
        ((2048, 2048, 40, big, 512, 2048), "ond"), ((2048, 2049, 40, big, 512, 2048), "myers"),
        # the container's longest sequence caps the piece as well, rounded up the same way
        ((1000, 1000, 5, 1000, 512, 32768), "ond"), ((1024, 1000, 5, 1000, 512, 32768), "ond"),
        ((1025, 1000, 5, 1024, 512, 32768), "myers"), ((1025, 1000, 5, 1025, 512, 32768), "ond"),
        # an empty compared side: nothing to search, whatever the other length
        ((0, 1000, 1000, big, 512, 32768), "ond"), ((40000, 0, 40000, big, 512, 32768), "myers"),
        ((0, 50000, 50000, big, 512, 32768), "wide"), ((0, 0, 0, big, 512, 32768), "ond"),
    ]
    for args, want in table:
        assert R(*args) == want, args
    assert E.k0(1000, 1000, big) == 1024 and E.k0(32768, 5, big) == 1024 and E.k0(5, 32769, big) == 64
    assert E.k0(300, 300, big, emax=8) == 16 and E.k0(2048, 7, big, lds_bases=2000) == 1024
    assert E.k0(2049, 7, big, lds_bases=2000) == 64 and E.k0(1025, 7, 1024) == 64 and E.k0(1024, 7, 1000) == 1024
    assert E.launches({"ond"}) == {"k_edit_distance"}
    assert E.launches({"ond", "myers"}) == {"k_edit_distance", "k_edit_myers"}
    assert E.launches({"wide"}) == {"k_edit_distance", "k_edit_myers_wide"}
    assert E.launches({"myers", "wide"}) == set(E.EDIT_KERNELS)


def test_crafted_cases_are_what_they_claim(crafted, rows):
    """By the fixture's numbers: exact distances, band-edge paths, route sides, strip counts, compressed lengths."""
    by = {r["tag"]: r for r in rows}
    for r in rows:
        want = E.claimed_dist(r["spec"])
        if want is not None:
            assert r["dist"] == want, r["tag"]
        if r["spec"]["kind"] in ("subs", "dels", "excursion", "substring"):
            assert abs(r["m"] - r["n"]) <= r["dist"]
    # ---- exact distances at the route edge and on k at the doubling steps; |m - n| at the early return ----
    for d in (511, 512, 513):
        assert by[f"route/subs/D{d}"]["dist"] == d and by[f"route/subs/D{d}"]["n"] == by[f"route/subs/D{d}"]["m"]
        assert by[f"route/dels/D{d}"]["dist"] == d == by[f"route/dels/D{d}"]["n"] - by[f"route/dels/D{d}"]["m"]
    assert {by[f"route/subs/D{d}"]["dist"] for d in (1023, 1024, 1025, 2047, 2048, 2049)} == {1023, 1024, 1025, 2047, 2048, 2049}
    assert [by[f"route/lds/n{n}"]["n"] for n in (32767, 32768, 32769)] == [32767, 32768, 32769]
    assert [by[f"route/big/n{n}"]["m"] for n in (49151, 49152, 49153)] == [49151, 49152, 49153]
    for d in (7, 8, 9, 15, 16, 17):
        assert by[f"shrunk/emax8/subs/D{d}"]["dist"] == by[f"shrunk/emax8/dels/D{d}"]["dist"] == d
    # ---- the route of the named cases ----
    route = {r["tag"]: E.case_route(r, r) for r in rows}
    assert [route[f"route/{k}/D{d}"] for k in ("subs", "dels") for d in (511, 512, 513)] == ["ond", "ond", "myers"] * 2
    assert [route[f"route/lds/n{n}"] for n in (32767, 32768, 32769)] == ["ond", "ond", "myers"]
    assert [route[f"route/big/n{n}"] for n in (49151, 49152, 49153)] == ["myers", "myers", "wide"]
    assert route["route/unrelated/1x511"] == route["route/unrelated/1x512"] == "ond"
    for t in ("1x513", "513x1", "64x576", "576x64"):                    # |m - n| = distance = eMax: found in the last round
        assert route[f"route/unrelated/{t}"] == "ond" and by[f"route/unrelated/{t}"]["dist"] == 512
    assert route["route/unrelated/1x514"] == "myers" and by["route/unrelated/1x514"]["dist"] == 513
    assert [route[f"shrunk/emax8/{k}/D{d}"] for k in ("subs", "dels") for d in (7, 8, 9)] == ["ond", "ond", "myers"] * 2
    for env in ("lds2000", "lds2048"):
        got = [route[f"shrunk/{env}/n{n}"] for n in (2000, 2001, 2047, 2048, 2049, 2050)]
        assert got == ["ond"] * 4 + ["myers"] * 2, env
    # ---- at least 10 cases on each side of every edge, under every set of switches that has it ----
    side = {}
    for r in rows:
        emax, lds = E.env_params(r["env"])
        fit = E.fits(r["n"], r["m"], max(lds, r["n"], r["m"]), lds)
        rt = route[r["tag"]]
        key = ("fit/" + ("done" if rt == "ond" else "handed")) if fit else ("nofit/" + rt)
        side[(r["env"], key)] = side.get((r["env"], key), 0) + 1
    for env in ("default", "emax8"):                                    # distance against eMax
        assert side[(env, "fit/done")] >= 10 and side[(env, "fit/handed")] >= 10, (env, side)
    for env in ("default", "lds2000", "lds2048"):                       # length against the LDS piece
        fit = side[(env, "fit/done")] + side.get((env, "fit/handed"), 0)
        nofit = side.get((env, "nofit/myers"), 0) + side.get((env, "nofit/wide"), 0)
        assert fit >= 10 and nofit >= 10, (env, side)
    assert side[("default", "nofit/myers")] >= 10 and side[("default", "nofit/wide")] >= 10      # length against ED_BIG_MIN
    groups = {(r["env"], r["use_hpc"], route[r["tag"]]) for r in rows}
    assert groups == set(E.GROUPS) and len(E.GROUPS) == len(set(E.GROUPS))
    # ---- band edges: distance 2 X (+ the single indels), the path's diagonal against the band of the pass that ends ----
    on_edge = 0
    for r in rows:
        s = r["spec"]
        if not r["tag"].startswith("band/"):
            continue
        delta = s.get("delta", 0)
        assert r["m"] - r["n"] == delta
        if delta == 0:
            assert r["dist"] == 2 * s["X"]
        emax, lds = E.env_params(r["env"])
        k = max(E.k0(r["n"], r["m"], max(lds, r["n"], r["m"]), emax, lds), abs(delta))
        assert k == (1024 if r["tag"].startswith("band/k1024") else 64)
        while k < r["dist"]:
            k *= 2
        dhi, dlo = (k + delta) // 2, -((k - delta) // 2)
        diag = delta + s["X"] if s["first"] == "ins" else delta - s["X"]
        assert dlo <= diag <= dhi, r["tag"]
        on_edge += diag in (dlo, dhi)
    assert on_edge >= 20
    for k in (64, 128, 256, 512):                                       # on k exactly at every doubling step
        assert by[f"band/k64/X{k // 2}/ins/d+0"]["dist"] == by[f"band/k64/X{k // 2}/del/d+0"]["dist"] == k
    assert by["band/k1024/X512/ins/d+0"]["dist"] == 1024
    # ---- strips ----
    for n in (4095, 4096, 4097, 8191, 8192, 8193):
        for dm in (0, 1, -1, 63, 64):
            r = by[f"strip/n{n}/dm{dm:+d}/e15"]
            assert (r["n"], r["m"] - r["n"]) == (n, dm) and route[r["tag"]] == "myers"
        assert route[f"strip/n{n}/dm+0/e05"] == route[f"strip/n{n}/dm+63/e05"] == "ond"
    assert {(by[f"strip/mod64/n{a}/m{b}"]["n"] % 64, by[f"strip/mod64/n{a}/m{b}"]["m"] % 64)
            for a in (0, 1, 63) for b in (0, 1, 63)} == {(a, b) for a in (0, 1, 63) for b in (0, 1, 63)}
    for row in (4095, 4096, 4097):
        for form in ("ins", "del", "del-ins"):
            r = by[f"strip/run/{form}/r{row}"]
            assert r["dist"] == 80 and route[r["tag"]] == "myers"
    # ---- the 8-wave kernel ----
    wide = [r for r in rows if r["tag"].startswith("wide/")]
    assert all(route[r["tag"]] == "wide" and max(r["n"], r["m"]) > E.ED_BIG_MIN for r in wide)
    assert [E.strips(by[f"wide/substring/n{n}"]["n"]) for n in (1, 64, 4096, 28672, 32768, 32769)] == [1, 1, 1, 7, 8, 9]
    assert [by[f"wide/substring/n{n}"]["dist"] for n in (1, 64, 4096)] == [49152, 49089, 45057]
    assert E.strips(by["wide/S16"]["n"]) == 16 and E.strips(by["wide/S17"]["n"]) == 17 and by["wide/S16"]["m"] == 66000
    assert by["wide/unrelated"]["dist"] > 16384 and by["wide/identical"]["dist"] == 0
    # ---- compression ----
    for name in ("63", "64", "65", "127", "128", "129"):
        assert by[f"hpc/len/{name}"]["hpc_n"] == int(name)
    assert by["hpc/len/64/fill"]["hpc_n"] == 64 and by["hpc/len/65/tail"]["hpc_n"] == 65
    for n in (1, 64, 65, 4097, 49153):
        r = by[f"hpc/one/{n}/random"]
        assert (r["n"], r["hpc_n"]) == (n, 1) and r["hpc_m"] > 100
    assert route["hpc/one/49153/random"] == "wide" and route["hpc/one/49153/one/1"] == "wide"
    assert by["hpc/one/1/one/64"]["hpc_dist"] == 0 and by["hpc/one/65/one/4097"]["hpc_dist"] == 1
    r = by["hpc/run/l40000"]
    assert r["n"] == 49153 and r["hpc_n"] < 9153 and route[r["tag"]] == "wide"
    assert route["hpc/far"] == "myers" and by["hpc/far"]["hpc_dist"] > 512
    assert sum(r["tag"].startswith("noise/") and r["spec"]["kind"] == "pair" for r in rows) >= 60
    assert sum(r["tag"].startswith("range/") for r in rows) == 20


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def set_switches(monkeypatch, env):
    for k in E.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def device_distances(pairs, use_hpc):
    """(distances, lengths of a, lengths of b, launched edit kernels) of one fg_debug_edit_distances call."""
    from flye_amd import gpu
    ctx = gpu.Context(17, 0)
    try:
        ctx.set_reads(pairs_readset(pairs))
        d, la, lb = ctx.debug_edit_distances(len(pairs), use_hpc)
        kt = ctx.kernel_times()
    finally:
        ctx.close()
    return d.tolist(), la.tolist(), lb.tolist(), set(kt) & set(E.EDIT_KERNELS)


def assert_equals_fixture(got, picked, use_hpc):
    key = HPC if use_hpc else PLAIN
    d, la, lb = got
    assert la == [r[key[1]] for r in picked] and lb == [r[key[2]] for r in picked]
    bad = [(r["tag"], x, r[key[0]]) for r, x in zip(picked, d) if x != r[key[0]]]
    assert not bad, bad[:10]


@pytest.mark.gpu
@pytest.mark.parametrize("env,use_hpc,route", E.GROUPS, ids=["-".join((e, "hpc" if h else "plain", r)) for e, h, r in E.GROUPS])
def test_routes(monkeypatch, crafted, rows, env, use_hpc, route):
    """The cases of one route in a container of their own: the fixture's values, and the launched edit kernels are
    exactly the route's -- a pair at distance eMax that reaches the bit-vector kernel fails here, a pair at eMax + 1 that
    does not, a pair of ED_BIG_MIN bases in the 8-wave kernel, a pair of one more outside it."""
    idx = [i for i, r in enumerate(rows) if (r["env"], r["use_hpc"]) == (env, use_hpc) and E.case_route(r, r) == route]
    assert idx
    pairs = [crafted[1][i] for i in idx]
    emax, lds = E.env_params(env)
    if max(max(len(a), len(b)) for a, b in pairs) < lds:
        pairs.append(E.pad_pair(env))                   # route "ond": adds no kernel to the call
    longest = max(max(len(a), len(b)) for a, b in pairs)
    assert longest >= lds
    picked = [rows[i] for i in idx]
    assert all(E.route(r["n"], r["m"], r[HPC[0] if use_hpc else PLAIN[0]], longest, emax, lds) == route for r in picked)
    set_switches(monkeypatch, E.ENVS[env])
    d, la, lb, ran = device_distances(pairs, use_hpc)
    assert_equals_fixture((d[:len(idx)], la[:len(idx)], lb[:len(idx)]), picked, use_hpc)
    assert ran == E.launches({route})


PAST_EDGE = (("default", "emax"), ("emax8", "emax"), ("default", "lds"), ("lds2000", "lds"), ("lds2048", "lds"), ("default", "big"))


def just_past(rows, env, edge):
    """Indices of the cases that lie one step past an edge of the rule under env's switches (plain form): the first
    distance O(ND) gives up on, the first length that does not fit the LDS piece (at a distance O(ND) would find), the
    first length of the 8-wave kernel."""
    emax, lds = E.env_params(env)
    cap = E.roundup64(lds)
    out = []
    for i, r in enumerate(rows):
        longer, fit = max(r["n"], r["m"]), max(r["n"], r["m"]) <= cap
        if {"emax": fit and min(r["n"], r["m"]) > 0 and r["dist"] == emax + 1,
            "lds": longer == cap + 1 and r["dist"] <= emax,
            "big": longer == E.ED_BIG_MIN + 1}[edge]:
            out.append(i)
    return out


def test_cases_just_past_every_edge_exist(rows):
    assert {(env, edge): len(just_past(rows, env, edge)) >= 2 for env, edge in PAST_EDGE} == {k: True for k in PAST_EDGE}


@pytest.mark.gpu
@pytest.mark.parametrize("env,edge", PAST_EDGE, ids=["-".join(p) for p in PAST_EDGE])
def test_first_pairs_past_an_edge_are_handed_over(monkeypatch, crafted, rows, env, edge):
    """Only the pairs one step past an edge in a call: the kernel they are handed to did launch.  (In a call with other
    pairs of the same route, a pair the O(ND) kernel kept would not show: that kernel runs in every call.)"""
    idx = just_past(rows, env, edge)
    picked = [rows[i] for i in idx]
    emax, lds = E.env_params(env)
    longest = max(max(r["n"], r["m"]) for r in picked)
    routes = {E.route(r["n"], r["m"], r["dist"], longest, emax, lds) for r in picked}
    assert routes == {"wide" if edge == "big" else "myers"}
    set_switches(monkeypatch, E.ENVS[env])
    d, la, lb, ran = device_distances([crafted[1][i] for i in idx], False)
    assert_equals_fixture((d, la, lb), picked, False)
    assert ran == E.launches(routes)


@pytest.mark.gpu
@pytest.mark.parametrize("use_hpc", [False, True], ids=["plain", "hpc"])
@pytest.mark.parametrize("env", list(E.ENVS))
def test_whole_set_in_one_call(monkeypatch, crafted, rows, env, use_hpc):
    """Every case in one mixed call, under each set of switches, plain and compressed."""
    set_switches(monkeypatch, E.ENVS[env])
    d, la, lb, ran = device_distances(crafted[1], use_hpc)
    assert_equals_fixture((d, la, lb), rows, use_hpc)
    assert ran == E.launches({E.case_route(r, r, env, use_hpc) for r in rows})


@pytest.fixture(scope="module")
def small_batch(built):
    """4096 + 65 pairs of 40 .. 200 bases at 30 % errors and their distances by the oracle."""
    from oracle import oracle as O
    rng = np.random.default_rng(4161)
    pairs = [edit_pair(dict(seed=int(rng.integers(1, 1 << 30)), n=int(rng.integers(40, 201)), err=0.3)) for _ in range(4096 + 65)]
    return pairs, [O.edit_distance(a, b) for a, b in pairs]


@pytest.mark.gpu
@pytest.mark.parametrize("emax", [None, 1])
def test_second_pair_on_a_block(monkeypatch, small_batch, emax):
    """More pairs than the 4096 blocks of k_edit_ond: 65 blocks take a second pair behind their first (LDS planes and
    the furthest-point arrays of the first are left in place).  Under FG_ED_EMAX = 1 more than 4096 of them are handed
    over, so blocks of the bit-vector kernel take a second pair in their slab as well."""
    pairs, want = small_batch
    assert len(pairs) > 4096 and max(want) <= E.ED_EMAX
    set_switches(monkeypatch, {} if emax is None else {"FG_ED_EMAX": emax})
    if emax is not None:
        assert sum(w > emax for w in want) > 4096
    d, la, lb, ran = device_distances(pairs, False)
    assert d == want and la == [len(a) for a, _ in pairs] and lb == [len(b) for _, b in pairs]
    assert ran == E.launches({"ond"} if emax is None else {"ond", "myers"})


@pytest.mark.gpu
def test_one_slab_long_pair_then_short_ones(monkeypatch, built):
    """FG_ED_SLAB_BYTES = 1: one block and one slab for the whole list, so a short pair's planes and delta words lie
    where a 6000-base pair's were (the list's order is the atomics': equality only)."""
    from oracle import oracle as O
    rng = np.random.default_rng(6000)
    pairs = []
    for _ in range(3):
        pairs.append(edit_pair(dict(seed=int(rng.integers(1, 1 << 30)), n=6000, err=0.2)))
        pairs += [edit_pair(dict(seed=int(rng.integers(1, 1 << 30)), n=int(rng.integers(70, 301)), err=0.3)) for _ in range(5)]
    want = [O.edit_distance(a, b) for a, b in pairs]
    assert min(want) > 3
    set_switches(monkeypatch, {"FG_ED_SLAB_BYTES": 1, "FG_ED_EMAX": 3})
    d, la, lb, ran = device_distances(pairs, False)
    assert d == want and la == [len(a) for a, _ in pairs] and lb == [len(b) for _, b in pairs]
    assert ran == E.launches({"myers"})


@pytest.mark.gpu
def test_one_slab_wide_pairs(monkeypatch, built):
    """The same for the 8-wave kernel: 70 000, 49 153, 66 000 and 49 153 bases through one slab, two with a tiny n."""
    from oracle import oracle as O
    specs = [dict(kind="lens", seed=1, n=70000, m=69000, err=0.03), dict(kind="substring", seed=2, n=5, m=49153),
             dict(kind="lens", seed=3, n=66000, m=66000, err=0.02), dict(kind="substring", seed=4, n=64, m=49153, off=49000)]
    pairs = [E.build(s) for s in specs]
    want = [O.edit_distance(a, b) for a, b in pairs]
    assert want[1] == 49148 and want[3] == 49089
    set_switches(monkeypatch, {"FG_ED_SLAB_BYTES": 1})
    d, la, lb, ran = device_distances(pairs, False)
    assert d == want and la == [len(a) for a, _ in pairs] and lb == [len(b) for _, b in pairs]
    assert ran == E.launches({"wide"})


@pytest.mark.gpu
@pytest.mark.parametrize("use_hpc", [True, False], ids=["hpc", "plain"])
def test_ranges_on_both_strands(monkeypatch, built, rows, use_hpc):
    """The range cases through fg_edit_ranges on the resident reads: both strands of both sides, ranges that begin and
    end inside long runs.  Distances, compared lengths and divergence bits, as test_edit_ranges compares them."""
    from flye_amd import gpu, synth
    from test_edit_ranges import assert_same
    picked = [r for r in rows if r["spec"]["kind"] == "range"]
    table = np.array([(2 * s["cur"][0] + s["cur"][1], 2 * s["ext"][0] + s["ext"][1], s["cur"][2], s["cur"][3], s["ext"][2], s["ext"][3])
                      for s in (r["spec"] for r in picked)], np.int64)
    assert len(table) == 20 and {tuple(t) for t in table[:, :2] % 2} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    key = HPC if use_hpc else PLAIN
    d, la, lb = (np.array([r[k] for r in picked], np.int32) for k in key)
    want = (d, la, lb, d.astype(np.float32) / np.maximum(la, lb).astype(np.float32))
    set_switches(monkeypatch, {})
    ctx = gpu.Context(17, 0)
    try:
        ctx.set_reads(synth.ReadSet.from_arrays(E.range_reads()), 0)
        assert_same(ctx.edit_ranges(table, use_hpc=use_hpc), want)
    finally:
        ctx.close()
