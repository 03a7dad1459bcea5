"""The k-mer lookup table (fg_index.hip fgIndexLookupStructures / k_table_insert, fg_ctx.h fg_probe) at its spill, wrap,
part and load edges, on the crafted indexes of tests/table_craft.py imported with fg_import_index.

CPU tests: each crafted case is what it claims -- by the restatement's occupied slot sets and walks, and where the
insertion order could matter by counting (table_craft.stored_beyond) -- and prints its walk statistics.

GPU tests: fg_debug_table equals the restatement (geometry, the occupied slot set of every part, every stored value, the
invariant a probe's early stop rests on); fg_probe_hits over all queries and both strands equals the CPU seed hits
(helpers.cpu_seed_hits: is the k-mer in the sorted key array, and what is its list); getSeqOverlapsBatch equals the
oracle's overlaps on the same imported index.  Every comparison is exact and leaves no k-mer and no key out."""
import numpy as np
import pytest

import table_craft as tc
from helpers import check_overlaps_equal, cpu_seed_hits

NARROW_KS, WIDE_KS = (17, 11), (18, 32)
CASES = ([("chain", k) for k in NARROW_KS + WIDE_KS] + [("wrap", k) for k in NARROW_KS + WIDE_KS] +
         [("parts", k) for k in NARROW_KS] + [("degenerate_" + w, k) for w in "abc" for k in (17, 32)])
SWITCHES = ("FG_TABLE_LOAD_PCT", "FG_TABLE_PART_KEYS", "FG_PROBE_PARTITION", "FG_PROBE_SUB_KMERS", "FG_HIT_BUDGET",
            "FG_KMER_BUDGET", "FG_LANES", "FG_PROBE_SKIP", "FG_ABLATE_PROBE")
EMPTY = np.uint64(tc.EMPTY)


def _id(c):
    return f"{c[0]}-k{c[1]}"


# ---- the references, computed once per case and never changed -------------------------------------------------------
_CPU_HITS, _ORACLE = {}, {}


def _cpu_hits(case):
    key = (case.name, case.k)
    if key not in _CPU_HITS:
        _CPU_HITS[key] = cpu_seed_hits(case.readset(), case.ex, case.k, case.queries())
    return _CPU_HITS[key]


def _cfg():
    from flye_amd import config
    return config.preset("raw")


def _oracle_overlaps(case, ex=None):
    from oracle import oracle as O
    key = (case.name, case.k)
    if ex is None and key in _ORACLE:
        return _ORACLE[key]
    o = O.Oracle(case.k)
    o.set_reads(case.readset())
    o.import_index(case.ex if ex is None else ex, 1.0)
    res = o.overlaps(O.detector_params(_cfg(), min_overlap=tc.MIN_OVERLAP), case.queries())
    o.close()
    if ex is None:
        _ORACLE[key] = res
    return res


def _print_stats(case, st, where):
    print(f"{case.name} k={case.k} ({where}): {st['probed']} probed k-mers = {st['present']} present + "
          f"{st['repetitive']} repetitive + {st['empty_list']} with an empty list + {st['absent']} absent; "
          f"{st['multi']} read more than one {'slot' if case.geom.wide else 'group'} (longest walk {st['max_units']}; "
          f"present keys: {st['present_multi']}, longest {st['present_max']}; repetitive: {st['repetitive_multi']}), "
          f"{st['wrapped']} wrapped ({st['present_wrapped']} present, {st['repetitive_wrapped']} repetitive, "
          f"{st['absent_wrapped']} absent), {st['inside_part']} stayed inside their part")


# ---- CPU: the restatement and the cases ------------------------------------------------------------------------------
def _mix_int(x):
    m = (1 << 64) - 1
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & m
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & m
    return x ^ (x >> 33)


def test_restated_hash_geometry_and_clamp():
    rng = np.random.default_rng(1)
    keys = np.concatenate([rng.integers(0, 1 << 63, size=200, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
                           np.array([0, 1, (1 << 34) - 1, (1 << 64) - 2], np.uint64)])
    assert [int(v) for v in tc.fg_mix(keys)] == [_mix_int(int(v)) for v in keys]
    for n in (16, 249, 1000, (1 << 32) - 1):
        assert [int(v) for v in tc.home_group(keys, n)] == [((_mix_int(int(v)) >> 32) * n) >> 32 for v in keys]
        assert [int(v) for v in tc.wide_start(keys, n)] == \
            [(((_mix_int(int(v)) >> 32) * n) >> 32) * 8 + (_mix_int(int(v)) & 7) for v in keys]
    assert [tc.load_pct(10, 0, v) for v in ("1", "4", "5", "25", "90", "91", "99")] == [5, 5, 5, 25, 90, 90, 90]
    assert tc.load_pct(1 << 26, 0) == 25 and tc.load_pct((1 << 26) - 5, 6) == 50       # (keys + repetitive) * 32 <= 2^31
    assert tc.groups_for(0, 25) == tc.groups_for(32, 25) == 16 and tc.groups_for(33, 25) == 17
    assert tc.groups_for(115, 90) == tc.groups_for(116, 90) == 16 and tc.groups_for(117, 90) == 17
    assert not tc.is_wide(17) and tc.is_wide(18)
    g = tc.geometry(1989, [1, 1, 0, 0, 9], 17, 497)
    assert (g.n_parts, g.key_base, g.kept) == (5, [0, 497, 994, 1491, 1988], [497, 497, 497, 497, 1])
    assert tc.geometry(1989, 11, 18, 497).n_parts == 1 and tc.geometry(0, 24, 17, 497).n_parts == 1
    bound = [0, 10, 20, tc.EMPTY]
    assert list(tc.part_of([0, 9, 10, 19, 20, tc.EMPTY], bound)) == [0, 0, 1, 1, 2, 2]


def test_occupied_set_is_order_free_and_walks_follow_it():
    """a hand-made part: 3 groups (narrow) / 24 slots (wide)"""
    start = np.array([16] * 10 + [0] * 3, np.int64)                # 10 keys from slot 16: 8 stay, 2 wrap to slots 0, 1
    a, b = tc.insert(start, 24, range(13)), tc.insert(start, 24, range(12, -1, -1))
    assert np.array_equal(a >= 0, b >= 0) and not np.array_equal(a, b)
    assert list(np.nonzero(a >= 0)[0]) == [0, 1, 2, 3, 4] + list(range(16, 24))
    keys = np.arange(13, dtype=np.uint64)
    narrow, wide = tc.PartTable(keys, 3, False, start), tc.PartTable(keys, 3, True, start)
    assert np.array_equal(narrow.occ, a >= 0) and np.array_equal(wide.occ, a >= 0)
    # narrow: group 2 is full, so a miss from it reads group 0 too; groups 0 and 1 have empty slots
    assert narrow.miss_len.tolist() == [1, 1, 2] and narrow.miss_wraps.tolist() == [False, False, True]
    assert narrow.walk_to(16, 23) == (1, False) and narrow.walk_to(16, 1) == (2, True) and narrow.walk_to(0, 4) == (1, False)
    # wide: slot by slot, from slot 23 on to slot 0
    assert wide.miss_len[16] == 14 and wide.miss_wraps[16] and wide.miss_len[5] == 1 and wide.miss_len[23] == 7
    assert wide.walk_to(16, 1) == (10, True) and wide.walk_to(23, 0) == (2, True) and wide.walk_to(16, 23) == (8, False)
    assert tc.stored_beyond(narrow, 2, 1, 1) == 2
    with pytest.raises(AssertionError):
        narrow.walk_to(0, 16)               # group 0 has an empty slot: a probe from it never reaches group 2


@pytest.mark.parametrize("case_id", CASES, ids=_id)
def test_case_is_what_it_claims(built, case_id):
    name, k = case_id
    case = tc.get_case(name, k)
    g, ex = case.geom, case.ex
    cand, cls, part, units, wraps = case.walks()
    st = case.stats()
    _print_stats(case, st, "keys inserted in ascending order")
    rev = case.stats([pt.place_rev for pt in case.parts])
    _print_stats(case, rev, "keys inserted in descending order")
    # what does not depend on the order: the walks of k-mers the table does not store
    for f in ("absent", "absent_multi", "absent_wrapped", "absent_max", "empty_list_multi", "empty_list_wrapped"):
        assert st[f] == rev[f], f
    assert st["probed"] == len(cand) == st["inside_part"] and st["absent"] > 0
    unit = 1 if g.wide else 8
    if name in ("chain", "wrap"):
        pt, G, h = case.parts[0], g.groups[0], case.notes["g"]
        assert (G, g.n_slots, len(pt.keys)) == (16, 128, 115) and h == (15 if name == "wrap" else 5)
        home = tc.home_group(pt.keys, G)
        assert [int((home == (h + i) % G).sum()) for i in range(5)] == list(tc.CLUSTER)
        far, out = tc.stored_beyond(pt, h, 5, 3), tc.stored_beyond(pt, h, 1, 1)
        print(f"  in every order at least {far} stored keys sit three or more groups from home, {out} of home {h} outside it")
        assert far >= 3 and out >= 11
        assert pt.occ[[(h * 8 + i) % pt.n for i in range(40)]].all()       # groups g .. g + 4 are full
        # absent k-mers of home g walk over the five full groups to the first group with an empty slot
        ab = (cls == 0) & (tc.home_group(cand, G) == h)
        st0 = tc.start_slot(cand[ab], G, g.wide)
        print(f"  {int(ab.sum())} absent k-mers of home {h}: walks of {units[ab].min()} to {units[ab].max()}")
        assert ab.sum() > 0 and np.all(units[ab] >= (40 - (st0 - h * 8)) // unit + 1)
        # the repetitive keys: one whose home group spilled, one inside the stretch the cut reads share
        rc, ro = case.notes["rep_in_cluster"], case.notes["rep_in_overlap"]
        assert sorted([rc, ro]) == [int(v) for v in ex.repetitive]
        assert tc.home_group([rc], G)[0] == h and ro in set(int(v) for v in case.reads.shared_kmers(k))
        assert st["repetitive"] == 2 and st["present"] == 113
        if name == "wrap":
            w_abs = ab & wraps
            print(f"  {int(w_abs.sum())} absent k-mers of the last group wrap; at least {out} stored keys of it wrapped")
            assert w_abs.sum() == ab.sum() > 0 and st["present_wrapped"] + st["repetitive_wrapped"] >= 11
            assert pt.occ[pt.n - 1] and pt.occ[0]
            if g.wide:          # misses that start in the part's last slots and read slot slotsInPart - 1, then slot 0
                assert np.any(st0 >= pt.n - 8)
    elif name == "parts":
        assert g.groups == [249, 249, 249, 249, 16] and g.kept[-1] == 1 and g.groups[-1] == tc.MIN_GROUPS
        for p, pt in enumerate(case.parts):
            G = g.groups[p]
            over = tc.stored_beyond(pt, G - 1, 1, 1)
            ab = (cls == 0) & (part == p) & (tc.home_group(cand, G) == G - 1) if p < 4 else None
            print(f"  part {p}: {int((tc.home_group(pt.keys, G) == G - 1).sum())} keys of the last group, at least {over} "
                  f"wrap to group 0; occupied slots of group 0: {int(pt.occ[:8].sum())}")
            assert over >= 1 and pt.occ[-8:].all() and pt.occ[0]
            if ab is not None:
                assert ab.sum() > 0 and wraps[ab].all()
        assert case.notes == dict(rep_below_bound1=1, rep_at_or_above_last=9, rep_between=1)
        inner = np.asarray(g.bound[1:-1], np.uint64)
        assert np.all(cls[np.searchsorted(cand, inner)] == 1) and np.array_equal(cand[np.searchsorted(cand, inner)], inner)
        assert np.array_equal(part[np.searchsorted(cand, inner)], np.arange(1, 5))
        assert st["present"] == tc.N_PARTS_KEEP and st["repetitive"] == 11
        assert st["absent_wrapped"] > 0 and st["present_wrapped"] + st["repetitive_wrapped"] > 0
        # the same keys under every load setting of the `load` test: 1 clamps to 5, 99 to 90
        shapes = {v: case.with_env(FG_TABLE_LOAD_PCT=v).geom for v in ("1", "5", "25", "90", "99")}
        assert shapes["1"].same_shape(shapes["5"]) and shapes["99"].same_shape(shapes["90"])
        assert shapes["25"].same_shape(g) and not shapes["5"].same_shape(g) and not shapes["90"].same_shape(g)
        assert shapes["5"].groups == [1245, 1245, 1243, 1243, 25] and shapes["90"].groups == [70, 70, 69, 69, 16]
    else:
        which = name[-1]
        want = dict(a=(0, 24, 0), b=(1, 0, 0), c=(300, 5, 40))[which]
        assert (st["present"], st["repetitive"], st["empty_list"]) == want
        assert len(ex.keys) == want[0] + want[2] and len(tc.stored_keys(ex)[0]) == want[0] + want[1]
        assert sum(len(pt.keys) for pt in case.parts) == want[0] + want[1]      # empty lists are stored nowhere


@pytest.mark.parametrize("k", NARROW_KS + WIDE_KS)
def test_repetitive_key_in_an_overlap_moves_the_divergence(built, k):
    """the chain case's repetitive key of the shared stretch: without it the oracle reports another divergence for
    records that span it -- so the device's repetitive lookups are visible in the records compared below"""
    case = tc.get_case("chain", k)
    want = _oracle_overlaps(case)
    ro = case.notes["rep_in_overlap"]
    ex2 = case.reads.index(k, case.ex.keys, [v for v in case.ex.repetitive if int(v) != ro])
    got = _oracle_overlaps(case, ex2)
    a = {(int(r["cur_id"]), int(r["ext_id"])): r for r in want.recs}
    b = {(int(r["cur_id"]), int(r["ext_id"])): r for r in got.recs}
    both = [p for p in a if p in b]
    moved = [p for p in both if a[p]["seq_divergence"].view(np.uint32) != b[p]["seq_divergence"].view(np.uint32)]
    print(f"chain k={k}: {len(want.recs)} records, {len(moved)} change their divergence without the repetitive key")
    assert len(want.recs) > 0 and len(moved) > 0


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def _device(case, monkeypatch, extra=None):
    """fresh context with the case's index imported under the case's environment (the table is built at import)"""
    from flye_amd import gpu
    for sw in SWITCHES:
        monkeypatch.delenv(sw, raising=False)
    for name, v in dict(case.env, **(extra or {})).items():
        monkeypatch.setenv(name, v)
    ctx = gpu.Context(case.k, 0)
    ctx.set_reads(case.readset())
    vi = gpu.VertexIndex(ctx, 1.0)
    ex = case.ex
    vi.import_index(gpu.IndexExport(ex.keys, ex.key_off, ex.entries, ex.repetitive), 1.0)
    det = gpu.OverlapDetector.for_assemble(ctx, vi, _cfg(), min_overlap=tc.MIN_OVERLAP)
    return ctx, vi, det


def _hits(det, q):
    from flye_amd import gpu
    counts, ptr, n = det.probe_hits(q)
    return counts, gpu.seed_hits_to_host(ptr, n)


def _check_table(case, tab):
    """fg_debug_table against the restatement; returns the device's placement (per part: slot -> index into the part's
    keys, -1 where empty)"""
    g, ex = case.geom, case.ex
    assert (tab["wide"], tab["n_parts"], tab["n_slots"]) == (g.wide, g.n_parts, g.n_slots)
    assert [int(v) for v in tab["bound"]] == g.bound
    assert [int(v) for v in tab["slot_base"]] == g.slot_base and [int(v) for v in tab["key_base"]] == g.key_base
    assert [int(v) for v in tab["groups"]] == g.groups
    cnt = np.diff(ex.key_off.astype(np.int64))
    slots = tab["slots"]
    assert len(slots) == g.n_slots
    placement, found = [], []
    for p, pt in enumerate(case.parts):
        a, n = g.slot_base[p], g.groups[p] * 8
        if g.wide:
            key, idx = slots[a:a + n, 0], slots[a:a + n, 1]
            occ = key != EMPTY
            assert np.all(idx[~occ] == EMPTY)
            rep = occ & (idx == EMPTY)
        else:
            v = slots[a:a + n]
            occ = v != EMPTY
            key, idx = v >> np.uint64(tc.IDX_BITS), v & np.uint64(tc.IDX_MASK)
            rep = occ & (idx == np.uint64(tc.IDX_MASK))
            idx = idx + np.uint64(g.key_base[p])
        assert np.array_equal(occ, pt.occ), f"part {p}: occupied slots differ from the restated set"
        k_occ = key[occ]
        assert len(pt.keys) == len(k_occ)
        at = np.minimum(np.searchsorted(pt.keys, k_occ), max(len(pt.keys) - 1, 0))
        assert np.array_equal(pt.keys[at], k_occ), f"part {p}: a slot holds a key that is none of the part's"
        assert len(np.unique(k_occ)) == len(k_occ), f"part {p}: a key is stored twice"
        kept = occ & ~rep
        ki = idx[kept].astype(np.int64)
        assert np.all(ki < len(ex.keys)) and np.array_equal(ex.keys[ki], key[kept]) and np.all(cnt[ki] > 0)
        assert np.all(np.isin(key[rep], ex.repetitive)) and not np.any(np.isin(key[kept], ex.repetitive))
        place = -np.ones(n, np.int64)
        place[occ] = at
        # every stored key lies on its own walk: no empty slot before it (narrow: no group with an empty slot)
        st = tc.start_slot(pt.keys, pt.n_groups, g.wide) if len(pt.keys) else []
        for slot in np.nonzero(occ)[0]:
            pt.walk_to(st[place[slot]], slot)
        placement.append(place)
        found.append(k_occ)
    found = np.concatenate(found) if found else np.zeros(0, np.uint64)
    assert np.array_equal(np.sort(found), np.sort(tc.stored_keys(ex)[0]))       # each stored exactly once, nothing else
    assert not np.any(np.isin(ex.keys[cnt == 0], found))                          # empty lists are stored nowhere
    return placement


def _check_hits(case, det, counts=None, hits=None):
    if counts is None:
        counts, hits = _hits(det, case.queries())
    ccounts, chits = _cpu_hits(case)
    assert np.array_equal(counts, ccounts)
    assert hits.tobytes() == chits.tobytes()
    return counts, hits


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", CASES, ids=_id)
def test_table_hits_and_overlaps(built, monkeypatch, case_id):
    name, k = case_id
    case = tc.get_case(name, k)
    ctx, vi, det = _device(case, monkeypatch)
    try:
        placement = _check_table(case, ctx.debug_table())
        st = case.stats(placement)
        _print_stats(case, st, "the device's table")
        if name in ("chain", "wrap"):
            pt, h = case.parts[0], case.notes["g"]
            slot_of = np.zeros(len(pt.keys), np.int64)
            slot_of[placement[0][placement[0] >= 0]] = np.nonzero(placement[0] >= 0)[0]
            dist = (slot_of // 8 - pt.start // 8) % pt.n_groups
            print(f"  stored keys by groups from home: {np.bincount(dist).tolist()}")
            assert int((dist >= 3).sum()) >= 3                   # what stored_beyond promises for every order
            if name == "wrap":
                assert st["present_wrapped"] + st["repetitive_wrapped"] >= 11
        counts, _ = _check_hits(case, det)
        gres = det.getSeqOverlapsBatch(case.queries())
        check_overlaps_equal(gres, _oracle_overlaps(case), False)
        print(f"  {int(counts.sum())} seed hits, {len(gres.recs)} records")
        if name in ("chain", "wrap", "parts", "degenerate_c"):
            assert counts.sum() > 0 and len(gres.recs) > 0
        if name == "degenerate_a":
            assert counts.sum() == 0 and len(gres.recs) == 0
    finally:
        ctx.close()


@pytest.mark.gpu
def test_no_index_is_a_state_error(built):
    from flye_amd import gpu
    ctx = gpu.Context(17, 0)
    try:
        with pytest.raises(gpu.FlyeGpuError) as e:
            ctx.debug_table()
        assert e.value.code == -4
    finally:
        ctx.close()


def _result_bytes(res):
    return (res.recs.tobytes(), res.query_off.tobytes(), res.stat_off.tobytes(), res.stats.tobytes(),
            (res.query_kmers, res.seed_hits, res.dp_groups, res.dp_elements))


@pytest.mark.gpu
@pytest.mark.parametrize("k", NARROW_KS)
def test_load_settings_change_the_table_and_nothing_else(built, monkeypatch, k):
    base = tc.get_case("parts", k)
    seen, tables = {}, {}
    for pct in ("5", "25", "90", "1", "99"):
        case = base.with_env(FG_TABLE_LOAD_PCT=pct)
        ctx, vi, det = _device(case, monkeypatch)
        try:
            tab = ctx.debug_table()
            _check_table(case, tab)
            counts, hits = _check_hits(case, det)
            res = det.getSeqOverlapsBatch(case.queries())
            seen[pct] = (counts.tobytes(), hits.tobytes()) + _result_bytes(res)
            tables[pct] = tab
            print(f"parts k={k} FG_TABLE_LOAD_PCT={pct}: groups {tab['groups'].tolist()}, {int(counts.sum())} hits, "
                  f"{len(res.recs)} records")
            assert len(res.recs) > 0
        finally:
            ctx.close()
    assert all(seen[p] == seen["25"] for p in seen)
    for a, b in (("1", "5"), ("99", "90")):
        for f in ("n_slots", "n_parts"):
            assert tables[a][f] == tables[b][f]
        for f in ("bound", "slot_base", "key_base", "groups"):
            assert np.array_equal(tables[a][f], tables[b][f]), (a, b, f)
        assert np.array_equal(tables[a]["slots"] != EMPTY, tables[b]["slots"] != EMPTY)
    assert tables["5"]["n_slots"] > tables["25"]["n_slots"] > tables["90"]["n_slots"]
    check_overlaps_equal(res, _oracle_overlaps(base), False)


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", [("chain", k) for k in NARROW_KS + WIDE_KS] + [("parts", k) for k in NARROW_KS], ids=_id)
def test_shard_keeps_the_table_and_rewrites_the_offsets(built, monkeypatch, case_id):
    name, k = case_id
    case = tc.get_case(name, k)
    ccounts, chits = _cpu_hits(case)
    q = case.queries()
    qi = np.repeat(np.arange(len(q)), ccounts.astype(np.int64))
    cnt = np.diff(case.ex.key_off.astype(np.int64))
    total = np.zeros(len(q), np.int64)
    emptied = 0
    for r in range(3):
        ctx, vi, det = _device(case, monkeypatch)
        try:
            before = ctx.debug_table()
            kept = vi.keep_targets(3, r)
            after = ctx.debug_table()
            for f in ("bound", "slot_base", "key_base", "groups", "slots"):
                assert np.array_equal(before[f], after[f]), f
            _check_table(case, after)
            own = ((case.ex.entries >> np.uint64(33)) % np.uint64(3)) == np.uint64(r)
            assert kept == int(own.sum())
            # keys whose list became empty stay in the table and give no hits
            left = np.add.reduceat(np.concatenate([own, [False]]).astype(np.int64), case.ex.key_off[:-1].astype(np.int64)) \
                if len(cnt) else np.zeros(0, np.int64)
            left = np.where(cnt > 0, left, 0)
            emptied += int(((cnt > 0) & (left == 0)).sum())
            counts, hits = _hits(det, q)
            m = (chits["ext_id"] >> 1) % 3 == r
            assert np.array_equal(counts, np.bincount(qi[m], minlength=len(q)).astype(np.uint64))
            assert hits.tobytes() == chits[m].tobytes()
            total += counts.astype(np.int64)
            print(f"{name} k={k} shard {r} of 3: {kept} entries, {int(counts.sum())} of {len(chits)} hits")
            assert 0 < counts.sum() < len(chits)
        finally:
            ctx.close()
    assert np.array_equal(total, ccounts.astype(np.int64))            # the shards' hits add up to the full set
    print(f"  {emptied} (key, shard) pairs with a list emptied by the restriction")
    assert emptied > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain", "wrap", "parts"])
def test_partitioned_probe_on_crafted_geometry(built, monkeypatch, name):
    """k_probe_emit computes a probe's table region from the part geometry: same hits as the direct probe"""
    case = tc.get_case(name, 17)
    q = case.queries()
    ctx, vi, det = _device(case, monkeypatch)
    try:
        direct = _check_hits(case, det)
        assert "k_probe_emit" not in ctx.kernel_times()
        res0 = det.getSeqOverlapsBatch(q)
    finally:
        ctx.close()
    total = int(sum(len(s) for s in case.reads.seqs))
    ctx, vi, det = _device(case, monkeypatch, {"FG_PROBE_PARTITION": "1", "FG_PROBE_SUB_KMERS": str(total // 7)})
    try:
        _check_table(case, ctx.debug_table())
        counts, hits = _check_hits(case, det)
        kt = ctx.kernel_times()
        assert "k_probe_emit" in kt and "k_probe_partition" in kt
        assert kt["k_probe_emit"][1] > 1                              # several sub-ranges
        assert counts.tobytes() == direct[0].tobytes() and hits.tobytes() == direct[1].tobytes()
        res = det.getSeqOverlapsBatch(q)
        assert _result_bytes(res) == _result_bytes(res0)
        check_overlaps_equal(res, _oracle_overlaps(case), False)
    finally:
        ctx.close()
