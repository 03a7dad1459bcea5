"""Crafted string pairs for the edit-distance kernels of fg_editdist.hip (k_edit_ond, k_edit_myers<1>, k_edit_myers<8>),
and the hand-over rule between them restated (tests only).

The rule (fg_editdist.hip, fgEditDistances / k_edit_ond): the O(ND) kernel stages both substrings in an LDS piece of
roundup64(min(longest sequence of the container, FG_ED_LDS_BASES or ED_LDS_BASES)) bases.  A pair whose longer RAW
substring (before homopolymer compression) fits that piece is tried there and is done if its distance is at most
FG_ED_EMAX or ED_EMAX (or if one compared side is empty); else the band doubling of the bit-vector kernel starts at
2 * eMax.  A pair that does not fit is not tried: its band doubling starts at 64.  Of the pairs handed over, those with
a raw substring longer than ED_BIG_MIN take the ED_BIG_WAVES-wave workgroup ("wide"), the others one wave ("myers").

cases() places pairs on both sides of every edge of that rule (also shrunk by the two switches), on the band's edge at
every doubling step, on the 4096-row strip edges and the 64-row / 64-column block edges, on the strip counts around the
wide kernel's 8 waves, and on the branches of the homopolymer compression.  A case is a small dict (tag, env, use_hpc,
spec); build(spec) makes the strings, everything is seeded and uses bases 0..3 only.  Builders that claim an exact
distance are checked through the oracle when the list is made and move to their next seed if they miss.
"""
from __future__ import annotations

import functools
import zlib

import numpy as np

from helpers import edit_pair, hpc

# mirrored from flye_amd/csrc/fg_editdist.hip
ED_EMAX = 512               # O(ND) rounds before the bit-vector path takes over
ED_LDS_BASES = 32768        # longest substring k_edit_ond stages in LDS
ED_STRIP = 4096             # rows per strip = 64 lanes x 64-row blocks
ED_BIG_MIN = 49152          # pairs with a longer substring get the multi-wave workgroup
ED_BIG_WAVES = 8

SEED = 20261020
EDIT_KERNELS = ("k_edit_distance", "k_edit_myers", "k_edit_myers_wide")      # fg_kernel_times labels
ENVS = {"default": {}, "emax8": {"FG_ED_EMAX": 8}, "lds2000": {"FG_ED_LDS_BASES": 2000},
        "lds2048": {"FG_ED_LDS_BASES": 2048}}
SWITCHES = ("FG_ED_EMAX", "FG_ED_LDS_BASES", "FG_ED_SLAB_BYTES")


def env_params(env):
    """(eMax, LDS bases) the kernels use under ENVS[env]."""
    e = ENVS[env]
    return int(e.get("FG_ED_EMAX", ED_EMAX)), int(e.get("FG_ED_LDS_BASES", ED_LDS_BASES))


# ---- the rule ----------------------------------------------------------------------------------------------------------
def roundup64(x):
    return (x + 63) // 64 * 64


def fits(raw_n, raw_m, container_max_len, lds_bases=ED_LDS_BASES):
    return max(raw_n, raw_m) <= roundup64(min(container_max_len, lds_bases))


def route(raw_n, raw_m, dist, container_max_len, emax=ED_EMAX, lds_bases=ED_LDS_BASES):
    """"ond", "myers" or "wide": the kernel that writes the pair's distance.  raw_n, raw_m: lengths before compression;
    dist: the distance of the strings actually compared."""
    if fits(raw_n, raw_m, container_max_len, lds_bases) and (min(raw_n, raw_m) == 0 or dist <= emax):
        return "ond"
    return "wide" if max(raw_n, raw_m) > ED_BIG_MIN else "myers"


def k0(raw_n, raw_m, container_max_len, emax=ED_EMAX, lds_bases=ED_LDS_BASES):
    """Where the band doubling starts for a pair that is handed over."""
    return 2 * emax if fits(raw_n, raw_m, container_max_len, lds_bases) else 64


def launches(routes):
    """The edit kernels a call with pairs of these routes launches."""
    out = {"k_edit_distance"}
    if "myers" in routes:
        out.add("k_edit_myers")
    if "wide" in routes:
        out.add("k_edit_myers_wide")
    return out


def strips(n):
    return (n + ED_STRIP - 1) // ED_STRIP


# ---- builders ----------------------------------------------------------------------------------------------------------
def _rng(seed):
    return np.random.default_rng([SEED, int(seed)])


def rand(rng, n):
    return rng.integers(0, 4, size=int(n), dtype=np.uint8)


def spaced(rng, lo, hi, count):
    """count positions in [lo, hi), at least half a step apart."""
    if not count:
        return np.empty(0, np.int64)
    step = (hi - lo) // count
    assert step >= 8, (lo, hi, count)
    return lo + np.arange(count, dtype=np.int64) * step + rng.integers(0, step // 2, size=count)


def mutate(rng, a, err):
    """a with substitutions, 1-base insertions and 1-base deletions, each at rate err / 3."""
    n = len(a)
    u = rng.random(n)
    r = rng.integers(0, 4, size=n, dtype=np.uint8)
    s = a.copy()
    sub = u < err / 3
    s[sub] = (a[sub] + 1 + r[sub] % 3) & 3
    ins = (u >= err / 3) & (u < 2 * err / 3)
    dele = (u >= 2 * err / 3) & (u < err)
    cnt = 1 + ins.astype(np.int64) - dele.astype(np.int64)
    out = np.repeat(s, cnt)
    out[np.cumsum(cnt)[ins] - 1] = r[ins]
    return out


def _subs(spec):
    """Exactly D spaced substitutions in a random string of n >= 20 D bases."""
    rng = _rng(spec["seed"])
    n, d = spec["n"], spec["D"]
    assert n >= 20 * d
    a = rand(rng, n)
    b = a.copy()
    p = spaced(rng, 0, n, d)
    b[p] = (a[p] + 1 + rng.integers(0, 3, size=d, dtype=np.uint8)) & 3
    return a, b


def _dels(spec):
    """D spaced single-base deletions: m = n - D, so the distance is D."""
    rng = _rng(spec["seed"])
    n, d = spec["n"], spec["D"]
    a = rand(rng, n)
    return a, np.delete(a, spaced(rng, 0, n, d))


def _excursion(spec):
    """first = "ins": X random bases put into b at row r and X bases of a left out `gap` rows later, so the path runs on
    diagonal +X in between; first = "del": the other way round, diagonal -X.  delta > 0 / < 0: |delta| spaced 1-base
    insertions / deletions before row r.  Distance 2 X + |delta| (the gap is too long to cross by mismatches)."""
    rng = _rng(spec["seed"])
    n, x, r, gap, delta = spec["n"], spec["X"], spec["r"], spec["gap"], spec.get("delta", 0)
    assert gap >= 3000 and r + x + gap + x <= n
    a = rand(rng, n)
    head = a[:r]
    if delta:
        p = spaced(rng, 10, r - 10, abs(delta))
        head = np.insert(head, p, (head[p] + 2) & 3) if delta > 0 else np.delete(head, p)
    block = rand(rng, x)
    if spec.get("first", "ins") == "ins":
        b = np.concatenate([head, block, a[r:r + gap], a[r + gap + x:]])
    else:
        b = np.concatenate([head, a[r + x:r + x + gap], block, a[r + x + gap:]])
    return a, b


def _substring(spec):
    """a = b[off, off + n): the distance is m - n."""
    rng = _rng(spec["seed"])
    b = rand(rng, spec["m"])
    off = spec.get("off", (spec["m"] - spec["n"]) // 2)
    return b[off:off + spec["n"]].copy(), b


def _second(rng, a, how):
    """The other string of a pair: {"err": e} = a mutated at rate e, {"rand": m} = m unrelated bases."""
    if "rand" in how:
        return rand(rng, how["rand"])
    return mutate(rng, a, how["err"])


def plant_runs(a, runs):
    """Homopolymer runs [off, off + len) of exactly that extent (the bases on both sides differ from the run's)."""
    for off, ln in runs:
        c = a[off]
        a[off:off + ln] = c
        if off:
            a[off - 1] = (c + 1) & 3
        if off + ln < len(a):
            a[off + ln] = (c + 2) & 3
    return a


def _runs(spec):
    rng = _rng(spec["seed"])
    a = plant_runs(rand(rng, spec["n"]), spec["runs"])
    return a, _second(rng, a, spec["b"])


def _chunks(spec):
    """kept[i] = bases that survive the compression in the i-th 64-base chunk of a (the last chunk has `last` bases):
    the chunk's first kept[i] bases each differ from the base before, the rest repeat."""
    rng = _rng(spec["seed"])
    kept, last = spec["kept"], spec.get("last", 64)
    out, prev = [], 4
    for i, k in enumerate(kept):
        ln = last if i == len(kept) - 1 else 64
        assert 0 <= k <= ln and (i or k)
        for j in range(ln):
            if j < k:
                prev = (prev + 1 + int(rng.integers(0, 3))) & 3 if prev < 4 else int(rng.integers(0, 4))
            out.append(prev)
    a = np.array(out, np.uint8)
    return a, _second(rng, a, spec["b"])


def _homo(spec):
    """a: n copies of one base; b: m copies of base_b, or m random bases."""
    rng = _rng(spec["seed"])
    a = np.full(spec["n"], spec["base"], np.uint8)
    b = np.full(spec["m"], spec["base_b"], np.uint8) if "base_b" in spec else rand(rng, spec["m"])
    return a, b


def _lens(spec):
    """n against exactly m bases: a mutated at rate err, then cut or padded with random bases at the end."""
    rng = _rng(spec["seed"])
    a = rand(rng, spec["n"])
    b = mutate(rng, a, spec["err"])
    m = spec["m"]
    b = b[:m] if len(b) >= m else np.concatenate([b, rand(rng, m - len(b))])
    return a, b


RANGE_RUNS = ((100, 130), (500, 200), (1000, 400), (2000, 64), (2300, 127), (2600, 65), (2900, 101))
RANGE_READ_LEN = 3001


@functools.lru_cache(maxsize=None)
def range_reads():
    """The resident reads of the range cases: 0 with RANGE_RUNS planted, 1 = read 0 at 3 % errors, 2 and 3 the same with
    the runs shifted by 37 bases."""
    rng = _rng(410434)
    out = []
    for shift in (0, 37):
        a = plant_runs(rand(rng, RANGE_READ_LEN), [(o - shift, ln) for o, ln in RANGE_RUNS])
        out += [a, mutate(rng, a, 0.03)]
    return out


def strand(read, rc):
    return (3 - read)[::-1].copy() if rc else read


def _range(spec):
    """cur / ext = [read of range_reads(), strand, begin, end] in the strand's own coordinates."""
    reads = range_reads()
    cut = []
    for rd, rc, beg, end in (spec["cur"], spec["ext"]):
        cut.append(strand(reads[rd], rc)[beg:end].copy())
    return cut[0], cut[1]


BUILDERS = {"pair": edit_pair, "subs": _subs, "dels": _dels, "excursion": _excursion, "substring": _substring,
            "runs": _runs, "chunks": _chunks, "homo": _homo, "lens": _lens, "range": _range}


def build(spec):
    """(a, b) as 0..3 arrays; "mirror" swaps the two (rows <-> columns)."""
    a, b = BUILDERS[spec["kind"]](spec)
    a, b = np.ascontiguousarray(a, np.uint8), np.ascontiguousarray(b, np.uint8)
    return (b, a) if spec.get("mirror") else (a, b)


def claimed_dist(spec):
    """The plain distance a builder promises, or None."""
    kind = spec["kind"]
    if kind in ("subs", "dels"):
        return spec["D"]
    if kind == "excursion":
        # single indels of the block's own direction add up with it; of the other direction a few of them are absorbed
        # (the reference's 12 kb pair at X = 511, delta = -37: 1055, not 1059): recorded, not claimed
        delta = spec.get("delta", 0)
        same = delta == 0 or (delta > 0) == (spec.get("first", "ins") == "ins")
        return 2 * spec["X"] + abs(delta) if same else None
    if kind == "substring":
        return spec["m"] - spec["n"]
    return None


def settle(spec):
    """The spec at the first of its seeds (seed, seed + 1, ...) whose strings have the claimed distance."""
    want = claimed_dist(spec)
    if want is None:
        return spec
    from oracle import oracle as O
    for t in range(8):
        s = dict(spec, seed=spec["seed"] + t)
        if O.edit_distance(*build(s)) == want:
            return s
    raise AssertionError(("no seed gives the claimed distance", spec))


# ---- the cases ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    """[dict(tag, env, use_hpc, spec)]: see the module text.  `env` names the switches the case is meant for (ENVS),
    use_hpc the form it is meant for; the tag's first part is its group."""
    out = []

    def add(tag, kind, env="default", use_hpc=False, **spec):
        spec = dict(kind=kind, seed=zlib.crc32(tag.encode()) & 0x3fffffff, **spec)
        out.append(dict(tag=tag, env=env, use_hpc=use_hpc, spec=settle(spec)))

    # ---- route edges, default switches ----
    for d in (511, 512, 513):
        add(f"route/subs/D{d}", "subs", n=20 * d + 77, D=d)
        add(f"route/dels/D{d}", "dels", n=20 * d + 77, D=d)                     # |m - n| = D: the early return at 513
    for d in (1024, 1025):
        add(f"route/dels/D{d}", "dels", n=24000, D=d)
    for d in (1023, 1024, 1025, 2047, 2048, 2049):                              # on k at the doubling steps 1024, 2048
        add(f"route/subs/D{d}", "subs", n=20 * d + 13, D=d)
    for n in (32767, 32768, 32769):                                             # the LDS piece: full to its last block
        add(f"route/lds/n{n}", "subs", n=n, D=n // 100)
        add(f"route/lds/n{n}/short", "lens", n=n - 200, m=n, err=0.005)
        add(f"route/lds/n{n}/short/mirror", "lens", n=n - 200, m=n, err=0.005, mirror=1)
    for n in (49151, 49152, 49153):
        add(f"route/big/n{n}", "subs", n=n, D=n // 50)
        add(f"route/big/n{n}/short", "lens", n=n - 300, m=n, err=0.02)
        add(f"route/big/n{n}/short/mirror", "lens", n=n - 300, m=n, err=0.02, mirror=1)
    for n, m in ((1, 511), (1, 512), (1, 513), (64, 576)):
        add(f"route/unrelated/{n}x{m}", "pair", n=n, err=1.0, m=m)
        add(f"route/unrelated/{m}x{n}", "pair", n=m, err=1.0, m=n)
    add("route/unrelated/1x514", "pair", n=1, err=1.0, m=514)                   # |m - n| = 513 on a one-base string

    # ---- the same edges shrunk by the switches ----
    for d in (7, 8, 9, 15, 16, 17):
        add(f"shrunk/emax8/subs/D{d}", "subs", env="emax8", n=1500 + 20 * d, D=d)
        add(f"shrunk/emax8/dels/D{d}", "dels", env="emax8", n=1500 + 20 * d, D=d)
    for env in ("lds2000", "lds2048"):                      # the piece rounds up to 64: 2001..2048 fit under 2000 too
        for n in (2000, 2001, 2047, 2048, 2049, 2050):
            add(f"shrunk/{env}/n{n}", "subs", env=env, n=n, D=n // 30)
            add(f"shrunk/{env}/n{n}/short", "lens", env=env, n=n - 150, m=n, err=0.03)
            add(f"shrunk/{env}/n{n}/short/mirror", "lens", env=env, n=n - 150, m=n, err=0.03, mirror=1)

    # ---- band edges: the path on diagonal +X or -X, 2 X = k at the doubling steps ----
    deltas = (0, 1, -1, 37, -37)
    for x in (511, 512, 513):                               # 12 kb pairs, k0 = 1024: inside, on the edge, one doubling
        for first in ("ins", "del"):
            for delta in deltas:
                add(f"band/k1024/X{x}/{first}/d{delta:+d}", "excursion", n=12000, X=x, r=3000 + 64 * (x % 3), gap=3500,
                    first=first, delta=delta)
    for x in (31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257):            # k0 = 64 and each doubling step
        for first in ("ins", "del"):
            for delta in deltas:
                add(f"band/k64/X{x}/{first}/d{delta:+d}", "excursion", env="lds2048", n=1100 + 3000 + 2 * x + 37 * (x % 5),
                    X=x, r=1000 + x % 7, gap=3000, first=first, delta=delta)

    # ---- strip edges ----
    edge_n = (4095, 4096, 4097, 8191, 8192, 8193)
    for n in edge_n:
        for dm in (0, 1, -1, 63, 64):
            add(f"strip/n{n}/dm{dm:+d}/e15", "lens", n=n, m=n + dm, err=0.15)   # bit-vector pairs
        for dm in (0, 63):
            add(f"strip/n{n}/dm{dm:+d}/e05", "lens", n=n, m=n + dm, err=0.005)  # O(ND)
    for rn in (0, 1, 63):                                   # ed_pad_correction and the rounding of ch
        for rm in (0, 1, 63):
            add(f"strip/mod64/n{rn}/m{rm}", "lens", n=5120 + rn, m=5184 + rm, err=0.15)
    for row in (4095, 4096, 4097):                          # a horizontal / vertical run on the strip's last / next first row
        add(f"strip/run/ins/r{row}", "excursion", env="emax8", n=8000, X=40, r=row, gap=3000, first="ins")
        add(f"strip/run/del/r{row}", "excursion", env="emax8", n=8000, X=40, r=row, gap=3000, first="del")
        add(f"strip/run/del-ins/r{row}", "excursion", env="emax8", n=8000, X=40, r=row - 3040, gap=3000, first="del")

    # ---- the 8-wave kernel: S = 1, 1, 1, 7, 8, 9, 16, 17 strips against 8 waves ----
    for n in (1, 64, 4096, 28672, 32768, 32769):
        add(f"wide/substring/n{n}", "substring", n=n, m=49153)
    add("wide/S16", "lens", n=65536, m=66000, err=0.03)
    add("wide/S17", "lens", n=65537, m=66000, err=0.03)
    add("wide/unrelated", "pair", n=49153, err=1.0, m=49153)                    # every doubling step up to n + m
    add("wide/identical", "pair", n=50000, err=0.0)

    # ---- the compression inside extract_planes (use_hpc, whole forward reads) ----
    for ln in (64, 65, 127, 128, 129, 200, 400):            # from 127 on a 64-base chunk is dropped whole
        for off in (0, 1, 63, 64):
            add(f"hpc/run/l{ln}/o{off}", "runs", use_hpc=True, n=off + ln + 300, runs=[[off, ln]], b={"err": 0.03})
    for name, kept, last in (("63", [63], 64), ("64", [64], 64), ("65", [64, 1], 64), ("127", [40, 24, 63], 64),
                             ("128", [40, 24, 64], 64), ("129", [64, 0, 64, 1], 64), ("64/fill", [1, 0, 0, 63], 64),
                             ("65/tail", [30, 34, 1], 1), ("128/tail", [64, 63, 1], 9), ("63/dropped", [62, 0, 0, 1], 64)):
        add(f"hpc/len/{name}", "chunks", use_hpc=True, kept=kept, last=last, b={"err": 0.02})
    one_base = (1, 64, 65, 4097, 49153)                     # compressed length 1; 49153: the wide kernel with n = 1
    for i, n in enumerate(one_base):
        add(f"hpc/one/{n}/random", "homo", use_hpc=True, n=n, base=i % 4, m=300)
        add(f"hpc/one/{n}/random/mirror", "homo", use_hpc=True, n=n, base=(i + 1) % 4, m=70, mirror=1)
        m = one_base[(i + 1) % len(one_base)]
        add(f"hpc/one/{n}/one/{m}", "homo", use_hpc=True, n=n, base=i % 4, m=m, base_b=(i + i // 2) % 4)
    add("hpc/run/l40000", "runs", use_hpc=True, n=49153, runs=[[5000, 40000]], b={"err": 0.02})
    for n in (33000, 40000, 49152):                         # no O(ND) attempt by the raw length, whatever the compressed one
        add(f"hpc/raw/n{n}", "runs", use_hpc=True, n=n, runs=[[1000, 20000], [25000, 129]], b={"err": 0.02})
    add("hpc/far", "runs", use_hpc=True, n=9000, runs=[[100, 200], [4096, 127]], b={"err": 0.3})    # compressed distance > 512

    # ---- the compression on ranges of resident reads: both strands of both sides, ranges that begin inside a long run
    #      and end inside one (on a reverse strand the runs cross other 64-base chunk edges) ----
    L = RANGE_READ_LEN
    spans = ((550, 1200), (1100, 2350), (120, 2950), (2001, 2063), (600, 1063))
    k = 0
    for beg, end in spans:
        for sc in (0, 1):
            for se in (0, 1):
                cb, ce = (L - end, L - beg) if sc else (beg, end)               # the same bases on either strand
                eb, ee = (L - end - 5, L - beg + 3) if se else (beg - 3, end + 5)
                add(f"range/{beg}-{end}/s{sc}{se}", "range", use_hpc=True, cur=[2 * (k % 2), sc, cb, ce],
                    ext=[2 * (k % 2) + 1, se, eb, ee])
                k += 1

    # ---- noise around the edges ----
    rng = _rng(60)
    for i in range(60):
        env = ("default", "default", "default", "emax8", "lds2000", "lds2048")[i % 6]
        if env == "default":
            n = int((32768, 49152, 4096, 8192)[(i // 6) % 4] + rng.integers(-600, 600))
            err = float(rng.choice([0.002, 0.01, 0.03]))
        elif env == "emax8":
            n, err = int(rng.integers(200, 3000)), float(rng.choice([0.0, 0.001, 0.003]))
        else:
            n, err = int(rng.integers(1850, 2200)), float(rng.choice([0.005, 0.05]))
        spec = dict(n=n, err=err, hp=int(rng.integers(0, 30)))
        if i % 5 == 4:
            spec["shift"] = int(rng.integers(0, 40))
        add(f"noise/{env}/{i}", "pair", env=env, use_hpc=bool((i // 6) % 2), **spec)
    add("noise/empty/fits", "pair", n=0, err=1.0, m=700)                        # an empty side: no distance to search
    add("noise/empty/long", "pair", n=40000, err=1.0, m=0)
    add("noise/empty/both", "pair", n=0, err=1.0, m=0)
    return out


def case_route(case, row, env=None, use_hpc=None):
    """route() of a case by the fixture's numbers, in a container whose longest read is at least the LDS switch."""
    env = case["env"] if env is None else env
    use_hpc = case["use_hpc"] if use_hpc is None else use_hpc
    emax, lds = env_params(env)
    dist = row["hpc_dist"] if use_hpc else row["dist"]
    return route(row["n"], row["m"], dist, max(lds, row["n"], row["m"]), emax, lds)


def pad_pair(env):
    """Two equal strings as long as the LDS switch of env: route "ond" in every form, and a container that holds them has
    a longest read of at least the switch."""
    s = rand(_rng(2048), env_params(env)[1])
    return s, s.copy()


# the (env, use_hpc, route) groups the cases fall into (test_edit_classes.py runs one call per group)
GROUPS = (("default", False, "ond"), ("default", False, "myers"), ("default", False, "wide"),
          ("default", True, "ond"), ("default", True, "myers"), ("default", True, "wide"),
          ("emax8", False, "ond"), ("emax8", False, "myers"), ("emax8", True, "ond"),
          ("lds2000", False, "ond"), ("lds2000", False, "myers"), ("lds2000", True, "ond"), ("lds2000", True, "myers"),
          ("lds2048", False, "ond"), ("lds2048", False, "myers"), ("lds2048", True, "ond"), ("lds2048", True, "myers"))


def measure(a, b):
    """What the fixture records of a pair, by the oracle."""
    from oracle import oracle as O
    ha, hb = hpc(a), hpc(b)
    return dict(n=len(a), m=len(b), dist=O.edit_distance(a, b), hpc_n=len(ha), hpc_m=len(hb), hpc_dist=O.edit_distance(ha, hb))
