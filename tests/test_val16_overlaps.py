"""Seed hits with 16-bit target positions, end to end.  The overlap stage carries a hit's target position as a uint16
beside its 32-bit key when the indexed container's longest read has at most 65536 bases (FG_VAL16=0 keeps 32-bit
values); nothing it returns may depend on the form.

* a small raw-read set (a few hundred reads, planted tandems: tied and tie-free queries, every sort route that small
  queries reach), both detector forms -- the assemble stage's and the repeat stage's with kmerMatches kept
  (keep_alignment): the 16-bit form, the 32-bit form and the oracle give identical records, field by field, floats by
  bit pattern;
* the boundary: a container whose longest read has exactly 65536 bases takes the 16-bit form (target positions up to
  65519 occur), one with a read of 65537 bases does not; the records equal the oracle's in both."""
import numpy as np
import pytest

SEED = 7
SCALE = 0.02
MIN_OVERLAP = 1000
SWITCHES = ("FG_VAL16", "FG_HIT_BUDGET", "FG_KMER_BUDGET", "FG_LANE_MIN_HITS", "FG_FORCE_KEY64", "FG_SORT_TIEFREE",
            "FG_SORT_SCREEN", "FG_SORT_RADIX_MAX")
FORMS = ["assemble", "repeat"]


def _detector(ctx, vi, cfg, form):
    from flye_amd import gpu
    if form == "assemble":
        return gpu.OverlapDetector.for_assemble(ctx, vi, cfg, MIN_OVERLAP)
    # the repeat stage's detector form: every overlap of a pair, kmerMatches kept
    return gpu.OverlapDetector(ctx, vi, int(cfg["maximum_jump"]), MIN_OVERLAP, int(cfg["maximum_overhang"]), True, False, 1.0,
                               bool(cfg["reads_base_alignment"]), False, bool(cfg["hpc_scoring_on"]))


def _oracle_params(cfg, form):
    from oracle import oracle as O
    return O.detector_params(cfg, min_overlap=MIN_OVERLAP, only_max_ext=form == "assemble", keep_alignment=form == "repeat")


def _arrays(res):
    out = dict(recs=res.recs.tobytes(), query_off=np.asarray(res.query_off).tobytes(), stat_off=np.asarray(res.stat_off).tobytes(),
               stats=np.asarray(res.stats).view(np.uint32).tobytes(),
               counters=(res.query_kmers, res.seed_hits, res.dp_groups, res.dp_elements, res.dp_elements_small))
    if res.match_off is not None:
        out["match_off"], out["matches"] = np.asarray(res.match_off).tobytes(), np.ascontiguousarray(res.matches).tobytes()
    return out


@pytest.fixture(scope="module")
def world(built):
    """the read set, the oracle's records of both forms (computed once), one device context with the index built"""
    import os
    from flye_amd import config, gpu, workloads
    from oracle import oracle as O
    saved = {sw: os.environ.pop(sw) for sw in SWITCHES if sw in os.environ}
    rs = workloads.ecoli_pb50(seed=SEED, scale=SCALE)[0]
    cfg = config.preset("raw")
    k = int(cfg["kmer_size"])
    o = O.Oracle(k)
    o.set_reads(rs)
    o.build_index(cfg)
    q = np.arange(0, 2 * rs.n, dtype=np.uint32)
    want = {form: o.overlaps(_oracle_params(cfg, form), q) for form in FORMS}
    w = dict(rs=rs, cfg=cfg, q=q, want=want)
    yield w
    if "ctx" in w:
        w["ctx"].close()
    os.environ.update(saved)


def _device(world):
    from flye_amd import gpu
    if "ctx" not in world:
        cfg = world["cfg"]
        ctx = gpu.Context(int(cfg["kmer_size"]), 0)
        ctx.set_reads(world["rs"])
        vi = gpu.VertexIndex(ctx, float(int(cfg["assemble_kmer_sample"])))
        vi.build(cfg)
        world["ctx"], world["vi"] = ctx, vi
    return world["ctx"], world["vi"]


def test_read_set_is_small_and_below_the_bound(world):
    rs = world["rs"]
    assert 100 <= rs.n <= 1000 and int(rs.length.max()) <= 65536
    assert all(len(world["want"][form].recs) > 0 for form in FORMS)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_records_identical_in_both_forms_and_to_the_oracle(world, monkeypatch, form):
    from helpers import check_overlaps_equal
    ctx, vi = _device(world)
    det = _detector(ctx, vi, world["cfg"], form)
    monkeypatch.delenv("FG_VAL16", raising=False)
    res16 = det.getSeqOverlapsBatch(world["q"])
    assert ctx.debug_hit_val16() is True
    monkeypatch.setenv("FG_VAL16", "0")
    res32 = det.getSeqOverlapsBatch(world["q"])
    assert ctx.debug_hit_val16() is False
    a16, a32 = _arrays(res16), _arrays(res32)
    assert sorted(a16) == sorted(a32) and ("matches" in a16) == (form == "repeat")
    for f in a16:
        assert a16[f] == a32[f], f
    assert len(res16.recs) > 0
    check_overlaps_equal(res16, world["want"][form], form == "repeat")
    check_overlaps_equal(res32, world["want"][form], form == "repeat")


# ---- the boundary ------------------------------------------------------------------------------------------------------------
def _boundary_reads(longest):
    """one read of ``longest`` bases from the start of a random genome and error-free 8 kb reads every 1000 bases along
    all of it: the long read is the target of overlaps that reach its last k-mer"""
    from flye_amd import synth
    rng = np.random.default_rng(65536)
    g = rng.integers(0, 4, size=longest + 12000, dtype=np.uint8)
    seqs = [g[:longest]] + [g[s:s + 8000] for s in range(0, len(g) - 8000 + 1, 1000)]
    return synth.ReadSet.from_arrays([np.ascontiguousarray(s) for s in seqs])


@pytest.mark.gpu
@pytest.mark.parametrize("longest", [65536, 65537])
def test_boundary_of_the_16_bit_form(built, monkeypatch, longest):
    from flye_amd import config, gpu
    from oracle import oracle as O
    from helpers import check_overlaps_equal
    for sw in SWITCHES:
        monkeypatch.delenv(sw, raising=False)
    rs = _boundary_reads(longest)
    assert int(rs.length.max()) == longest == int(rs.length[0])
    cfg = config.preset("raw")
    k = int(cfg["kmer_size"])
    q = np.arange(0, 2 * rs.n, dtype=np.uint32)
    o = O.Oracle(k)
    o.set_reads(rs)
    o.build_index(cfg)
    want = o.overlaps(_oracle_params(cfg, "repeat"), q)
    # the long read is a target up to its end: positions that need all 16 bits (and one more bit of length at 65537)
    to_long = want.recs[(want.recs["ext_id"] >> 1) == 0]
    assert len(to_long) > 0 and int(to_long["ext_end"].max()) >= longest - 2
    ctx = gpu.Context(k, 0)
    ctx.set_reads(rs)
    vi = gpu.VertexIndex(ctx, float(int(cfg["assemble_kmer_sample"])))
    vi.build(cfg)
    res = _detector(ctx, vi, cfg, "repeat").getSeqOverlapsBatch(q)
    took16 = ctx.debug_hit_val16()
    ctx.close()
    assert took16 is (longest <= 65536)
    check_overlaps_equal(res, want, True)
