"""The record pass behind the last kernel (gate, maxOverlaps rule, window statistics, records written by ordered
tasks with a chained prefix) against the CPU oracle, in the shapes the benchmark does not reach: a gate that drops
part of a query's primaries, a limit that cuts queries at a group start, several primaries per group, the
needs_trim marks, kmerMatches, a call cut into sub-ranges on one lane and on two, results below the
single-thread threshold, empty results.

The read set is large enough (> 100 000 primaries over > 128 queries) for several host threads, several tasks and
several copy pieces.  What each case must contain is asserted on the ORACLE's result (_contains), so that no
case can pass vacuously; test_cases_contain_what_they_claim runs those assertions without a GPU."""
import numpy as np
import pytest

from helpers import check_overlaps_equal

K = 17
CASES = {
    # name: (detector overrides, max_overlaps)
    "gate": (dict(max_divergence="median"), 0),
    "limit": (dict(), 4),
    "all_primaries": (dict(only_max_ext=False), 0),
    "all_primaries_limit_gate": (dict(only_max_ext=False, max_divergence="median"), 5),
    "partition": (dict(max_divergence="median", partition_bad_mappings=True), 0),
    "keep_alignment": (dict(keep_alignment=True, max_divergence="median"), 0),
    "keep_alignment_all_limit": (dict(keep_alignment=True, only_max_ext=False), 6),
    "nothing_kept": (dict(max_divergence=0.0), 0),
}


@pytest.fixture(scope="module")
def world():
    from flye_amd import config, synth
    from oracle import oracle as O
    rs = synth.simulate(seed=77, genome_len=150_000, coverage=40, kind="pb_raw", n_repeat_families=10,
                        n_tandems=30).filter_min_len(1000)
    cfg = config.preset("raw")
    o = O.Oracle(K)
    o.set_reads(rs)
    o.build_index(cfg)
    q = np.arange(0, 2 * rs.n, dtype=np.uint32)
    open_res = o.overlaps(O.detector_params(cfg), q)
    # the gate of the "median" cases: half of all primaries fail it
    gate = float(np.median(open_res.recs["seq_divergence"]))
    return dict(rs=rs, cfg=cfg, o=o, q=q, open=open_res, gate=gate, cache={})


def _overrides(w, name):
    ov, mo = CASES[name]
    ov = dict(ov)
    if ov.get("max_divergence") == "median":
        ov["max_divergence"] = w["gate"]
    return ov, mo


def _oracle(w, name):
    from oracle import oracle as O
    if name not in w["cache"]:
        ov, mo = _overrides(w, name)
        w["cache"][name] = w["o"].overlaps(O.detector_params(w["cfg"], **ov), w["q"], max_overlaps=mo)
    return w["cache"][name]


def _per_query(res):
    return np.diff(res.query_off.astype(np.int64))


def _contains(w, name, ores):
    """the oracle's result of the case holds what the case is meant to exercise"""
    open_res = w["open"]
    n_open, n = _per_query(open_res), _per_query(ores)
    assert len(w["q"]) > 2 * 128 and len(open_res.recs) > 100_000     # several tasks, threads and copy pieces
    if name in ("gate", "keep_alignment"):
        assert np.any((n > 0) & (n < n_open))              # kept and dropped primaries inside one query
    if name == "limit":
        assert np.any(n_open > 4) and np.all(n <= 4) and np.any(n == 4)
    if name.startswith("all_primaries") or name == "keep_alignment_all_limit":
        pair = ores.recs["cur_id"].astype(np.uint64) << np.uint64(32) | ores.recs["ext_id"].astype(np.uint64)
        assert np.any(pair[1:] == pair[:-1])               # a group with several primaries
    if name == "all_primaries_limit_gate":
        assert np.any(n > 5)                               # the limit is tested at group starts only
    if name == "partition":
        t = ores.needs_trim.astype(bool)
        assert t.any() and not t.all()
        first = ores.query_off[:-1].astype(np.int64)
        both = [t[a:a + c].any() and not t[a:a + c].all() for a, c in zip(first, n) if c]
        assert any(both)                                   # marked and unmarked records inside one query
    if name.startswith("keep_alignment"):
        assert len(ores.matches) > 2 * len(ores.recs) > 0
    if name == "nothing_kept":
        assert len(ores.recs) == 0 and len(ores.stats) > 0  # no record, but the window statistics stay


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_contain_what_they_claim(world, name):
    _contains(world, name, _oracle(world, name))


@pytest.fixture(scope="module")
def device(built, world):
    from flye_amd import gpu
    cfg = world["cfg"]
    ctx = gpu.Context(K, 0)
    ctx.set_reads(world["rs"])
    vi = gpu.VertexIndex(ctx, float(int(cfg["assemble_kmer_sample"])))
    vi.build(cfg)
    yield ctx, vi
    ctx.close()


def _detector(world, device, name):
    from flye_amd import gpu
    ctx, vi = device
    ov, mo = _overrides(world, name)
    det = gpu.OverlapDetector.for_assemble(ctx, vi, world["cfg"])
    det.p.max_divergence = ov.get("max_divergence", 1.0)
    det.p.only_max_ext = int(ov.get("only_max_ext", True))
    det.p.keep_alignment = int(ov.get("keep_alignment", False))
    det.p.partition_bad_mappings = int(ov.get("partition_bad_mappings", False))
    return det, ov, mo


def _same(gres, ores, ov, mo):
    check_overlaps_equal(gres, ores, bool(ov.get("keep_alignment")), counts=not mo)
    assert np.array_equal(gres.stat_off, ores.stat_off)
    if ov.get("partition_bad_mappings"):
        assert np.array_equal(gres.needs_trim, ores.needs_trim)
    else:
        assert gres.needs_trim is None


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_record_pass_against_oracle(world, device, name):
    ores = _oracle(world, name)
    _contains(world, name, ores)
    det, ov, mo = _detector(world, device, name)
    gres = det.getSeqOverlapsBatch(world["q"], maxOverlaps=mo)
    _same(gres, ores, ov, mo)
    # the same call again: the arena and the scratch of the first are reused
    _same(det.getSeqOverlapsBatch(world["q"], maxOverlaps=mo), ores, ov, mo)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("name", ["gate", "partition", "keep_alignment_all_limit"])
def test_sub_ranges_on_one_lane_and_two(world, device, monkeypatch, name, lanes):
    ores = _oracle(world, name)
    det, ov, mo = _detector(world, device, name)
    budget = max(1, ores.seed_hits // 7)
    hits = det.getSeqOverlapsBatch(world["q"][:1]).seed_hits
    assert hits < budget and ores.seed_hits > 4 * budget      # the call is cut into at least five sub-ranges
    monkeypatch.setenv("FG_HIT_BUDGET", str(budget))
    monkeypatch.setenv("FG_KMER_BUDGET", str(1 << 30))
    monkeypatch.setenv("FG_LANES", str(lanes))
    gres = det.getSeqOverlapsBatch(world["q"], maxOverlaps=mo)
    _same(gres, ores, ov, mo)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["gate", "partition", "all_primaries_limit_gate", "keep_alignment"])
def test_small_results_on_one_thread(world, device, name):
    """fewer than 20 000 primaries: one task runner on the calling thread, one copy"""
    from oracle import oracle as O
    det, ov, mo = _detector(world, device, name)
    for sub in (world["q"][10:13], world["q"][200:330]):      # one task; two tasks
        ores = world["o"].overlaps(O.detector_params(world["cfg"], **ov), sub, max_overlaps=mo)
        assert 0 < len(ores.recs) and len(world["open"].recs) * len(sub) // len(world["q"]) < 20_000
        _same(det.getSeqOverlapsBatch(sub, maxOverlaps=mo), ores, ov, mo)


@pytest.mark.gpu
def test_empty_results(world, device):
    from oracle import oracle as O
    det, ov, mo = _detector(world, device, "nothing_kept")
    ores = _oracle(world, "nothing_kept")
    gres = det.getSeqOverlapsBatch(world["q"])
    assert len(gres.recs) == 0 and int(gres.query_off[-1]) == 0
    _same(gres, ores, ov, mo)
    # no query at all
    det, ov, mo = _detector(world, device, "partition")
    none = det.getSeqOverlapsBatch(np.empty(0, np.uint32))
    assert len(none.recs) == 0 and len(none.query_off) == 1 and len(none.stat_off) == 1
