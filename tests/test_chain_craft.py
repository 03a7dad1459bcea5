"""The crafted chaining cases (tests/chain_craft.py) are what they declare: an honest index, and exactly
the declared target groups, hit for hit, as the oracle's seed collection and prefilter count them.  CPU
only (liboracle.so); the device runs them in tests/test_chain_classes.py."""
import numpy as np
import pytest

import chain_craft as cc
from helpers import canonical_kmers


@pytest.fixture(scope="module", params=cc.CASE_NAMES)
def case(request):
    return cc.make_case(request.param)


def test_index_is_honest(built, case):
    ex = case.index()
    rs = case.readset()
    keys, off = ex.keys, ex.key_off.astype(np.int64)
    assert np.all(np.diff(keys.astype(np.uint64)) > 0) and off[0] == 0 and off[-1] == len(ex.entries)
    can = {r: canonical_kmers(rs, r, cc.K) for r in range(rs.n)}
    fwd = {r: cc.kmer_codes(case.seqs[r])[0] for r in range(rs.n)}
    for i, key in enumerate(keys):
        ent = ex.entries[off[i]:off[i + 1]]
        assert len(ent) and np.all(np.diff(ent) > 0)                  # ascending, no duplicates
        for e in ent:
            rec, pos = int(e >> np.uint64(32)), int(e & np.uint64(0xFFFFFFFF))
            r, flip = rec >> 1, rec & 1
            L = int(rs.length[r])
            p = L - pos - cc.K if flip else pos                      # the forward position of the entry
            assert 0 <= p < L - cc.K and can[r][p] == key            # true canonical k-mer, never the last one
            assert (fwd[r][p] != key) == bool(flip)                  # strand bit = orientation of the k-mer
    # every occurrence of a present key is listed
    n_occ = sum(int(np.isin(can[r][:max(0, int(rs.length[r]) - cc.K)], keys).sum()) for r in range(rs.n))
    assert n_occ == len(ex.entries)


def test_declared_groups_are_the_seed_collection(case):
    got = cc.enumerate_groups(case)
    assert got == {g: sorted(h) for g, h in case.groups.items()}


def test_oracle_counts_the_declared_groups(built, case):
    from flye_amd import config
    from oracle import oracle as O
    cfg = config.preset("raw")
    o = O.Oracle(cc.K)
    o.set_reads(case.readset(), case.first_id)
    o.import_index(case.index(), 1.0)
    q = case.query_ids()
    for fl in sorted({bool(r.get("force_local")) for r in case.runs}):
        res = o.overlaps(O.detector_params(cfg, min_overlap=cc.MIN_OVERLAP), q, force_local=fl)
        assert (res.seed_hits, res.dp_groups, res.dp_elements) == case.totals(fl)
        assert len(res.recs) > 0


@pytest.mark.parametrize("name", ["key33_high", "key33_high_id"])
def test_key33_high_straddles_2_to_the_32(name):
    """from the declared hits: the one query's keys record << 20 | cur lie on both sides of 2^32, an odd record among
    the high ones, while key33's stay far below"""
    c = cc.make_case(name)
    bits = cc.KEY33_HIGH_CUR_BITS
    assert len(c.queries) == 1 and (1 << (bits - 1)) < c.rec_len(c.queries[0]) <= (1 << bits)
    assert len(c.seqs) == 2049                                       # 13 record bits: 33 with the position bits
    lo, hi = cc.hit_key_range(c, bits)
    assert lo < (1 << 32) <= hi
    by_side = {t: (t << bits) >= (1 << 32) for _, t in c.groups}
    assert sorted(by_side.values()) == [False, True] and any(t & 1 for t, high in by_side.items() if high)
    assert c.first_id == (1000 if name.endswith("_id") else 0)
    assert cc.hit_key_range(cc.make_case("key33"), bits)[1] < 1 << 24


def test_cases_reach_every_boundary():
    """The size classes and boundaries the device tests rely on are among the declared groups."""
    passing = {}
    for name in cc.CASE_NAMES:
        c = cc.make_case(name)
        passing[name] = sorted(c.sizes()[1])
    allp = sorted(n for v in passing.values() for n in v)
    for n in (10, 63, 64, 65, 255, 256, 257, 320, 321, 448, 449, 1024, 1025, 4096, 4097, 6000):
        assert n in allp, n
    assert max(passing["sizes_s"]) <= cc.FIN_CAP_S and max(passing["sizes_m"]) <= 448
    assert max(passing["tandem"]) > 4096 and any(cc.PREP_CAP < n <= cc.FIN_CAP_M for n in passing["tandem"])
    assert any(cc.FIN_CAP_M < n <= 4096 for n in passing["tandem"])
