"""The probe skip of seed collection: a solid-k-mer build leaves one bit per forward k-mer position, "the k-mer's
frequency over the whole read set reached minFreq"; where it is clear, k_probe / k_probe_emit take the position for a
miss without looking the k-mer up (a key enters the index only through a position with that frequency).

* the invariant itself (fg_debug_probe_skip_check): no position with a clear bit has a slot in the lookup table, and
  the number of clear bits is exactly the number of positions whose k-mer numpy counts below minFreq -- after the
  one-call build and after the build in steps with the counters sharded over two key ranges, through the gather and
  keep_targets.  minFreq = 1 can clear no bit (every k-mer occurs at least once): the count asserted there is 0,
  for 2 and 3 it is asserted to be above 0;
* records, offsets, statistics and counters byte for byte with FG_PROBE_SKIP=0 and =1, each in a fresh process:
  forward and reverse-strand queries, internal chunking, two lanes, FG_PROBE_PARTITION=1;
* no bits after an import, a minimizer build and the direct option-B split: everything is probed, the oracle agrees.

A test of the gloo sharded build without a device was left out: the bits exist in device memory only.

Run as a program (`python tests/test_probe_skip.py OUT.npz`) this file is the child of the parity tests."""
import os
import subprocess
import sys

import numpy as np
import pytest

K = 17
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reads():
    from flye_amd import synth
    return synth.simulate(seed=91, genome_len=120_000, coverage=30, kind="pb_raw", n_repeat_families=8,
                          n_tandems=20).filter_min_len(1000)


def _all_queries(rs):
    return np.arange(0, 2 * rs.n, dtype=np.uint32)        # every read, forward and reverse strand


def _child_main(out_path):
    sys.path.insert(0, ROOT)
    from flye_amd import config, gpu
    rs = _reads()
    cfg = config.preset("raw")
    ctx = gpu.Context(K, 0)
    ctx.set_reads(rs)
    vi = gpu.VertexIndex(ctx, float(int(cfg["assemble_kmer_sample"])))
    vi.build(cfg)
    clear, bad = ctx.debug_probe_skip_check()
    det = gpu.OverlapDetector.for_assemble(ctx, vi, cfg)
    res = det.getSeqOverlapsBatch(_all_queries(rs))
    np.savez(out_path, recs=np.frombuffer(res.recs.tobytes(), np.uint8), query_off=res.query_off, stat_off=res.stat_off,
             stats=res.stats.view(np.uint32),
             counters=np.array([res.query_kmers, res.seed_hits, res.dp_groups, res.dp_elements, res.dp_elements_small,
                                clear, bad], np.uint64))
    ctx.close()


if __name__ == "__main__":
    _child_main(sys.argv[1])
    sys.exit(0)


from helpers import canonical_kmers, check_overlaps_equal, index_digest  # noqa: E402


@pytest.fixture(scope="module")
def world():
    from flye_amd import config
    from oracle import oracle as O
    rs = _reads()
    cfg = config.preset("raw")
    o = O.Oracle(K)
    o.set_reads(rs)
    o.build_index(cfg)
    q = _all_queries(rs)
    # global count of every forward position's canonical k-mer (positions p < len - k, kmer.h:193-198)
    per_read = [canonical_kmers(rs, r, K)[:-1] for r in range(rs.n)]
    km = np.concatenate(per_read)
    assert len(km) == int(np.maximum(rs.length.astype(np.int64) - K, 0).sum())
    _, inv, cnt = np.unique(km, return_inverse=True, return_counts=True)
    return dict(rs=rs, cfg=cfg, o=o, q=q, ores=o.overlaps(O.detector_params(cfg), q), freq=cnt[inv])


def _expected_clear(world, min_freq):
    return int((world["freq"] < min_freq).sum())


def _solid_args(cfg):
    return cfg["meta_read_top_kmer_rate"], int(cfg["meta_read_filter_kmer_freq"]), cfg["repeat_kmer_rate"]


def _new(world):
    from flye_amd import gpu
    ctx = gpu.Context(K, 0)
    ctx.set_reads(world["rs"])
    return ctx, gpu.VertexIndex(ctx, float(int(world["cfg"]["assemble_kmer_sample"])))


@pytest.mark.gpu
@pytest.mark.parametrize("min_freq", [1, 2, 3])
def test_invariant_after_the_one_call_build(built, world, min_freq):
    ctx, vi = _new(world)
    vi.countKmers()
    vi.buildIndexUnevenCoverage(min_freq, *_solid_args(world["cfg"]))
    clear, bad = ctx.debug_probe_skip_check()
    print(f"minFreq {min_freq}: {clear} of {len(world['freq'])} positions skipped, {bad} violations")
    assert bad == 0
    assert clear == _expected_clear(world, min_freq)
    assert (clear > 0) == (min_freq > 1)
    ctx.close()


def _to_device(ptr, arr, dev):
    import torch
    from flye_amd import dist
    a = np.ascontiguousarray(arr, np.uint64).view(np.int64)
    if len(a):
        dist._view(ptr, len(a), dev).copy_(torch.from_numpy(a))


@pytest.mark.gpu
@pytest.mark.parametrize("min_freq", [1, 2, 3])
def test_invariant_through_the_sharded_build_in_steps(built, world, monkeypatch, min_freq):
    """Two 'ranks' = two contexts on one GPU: counters of one key range each, the batches' frequencies summed over
    both (the all-reduce), selection, the own range sorted, finish; then the gather of both pieces into each context
    and keep_targets.  The bits hold for the piece, the gathered index and the target shard."""
    import ctypes as C
    import torch
    from flye_amd import dist, gpu
    monkeypatch.setenv("FG_INDEX_BATCH_KMERS", "400000")
    cfg = world["cfg"]
    dev = torch.device("cuda", 0)
    W = 2
    rk = [_new(world) for _ in range(W)]
    ranges = dist.balanced_bin_ranges(rk[0][1].kmer_hist(), W)
    nb = None
    for r, (ctx, vi) in enumerate(rk):
        vi.countKmers()
        d, n = C.c_uint64(), C.c_uint32()
        ctx._check(ctx.L.fg_index_count_slice(ctx.h, min_freq, cfg["meta_read_top_kmer_rate"],
                                              int(cfg["meta_read_filter_kmer_freq"]), cfg["repeat_kmer_rate"],
                                              vi._sample_rate_init, int(ranges[r][0]), int(ranges[r][1]), C.byref(d), C.byref(n)))
        assert nb in (None, n.value)
        nb = n.value
    assert nb > 1                                            # words of the bit arrays shared between batches
    for b in range(nb):
        views = [dist._view(*vi.batch_freq(b), dev, "<i4") for _, vi in rk]
        total = views[0].clone()
        for v in views[1:]:
            total += v
        for v in views:
            v.copy_(total)
        torch.cuda.synchronize()
        for _, vi in rk:
            vi.batch_select(b)
    sums = np.zeros(2, np.uint64)
    for r, (_, vi) in enumerate(rk):
        vi.selection_done()
        sums += vi.build_range(*ranges[r])
    expected = _expected_clear(world, min_freq)
    pieces = []
    for ctx, vi in rk:
        vi.finish(sums)
        assert ctx.debug_probe_skip_check() == (expected, 0)    # the piece's table: a subset of the keys
        pieces.append(vi.export())
    whole = dist.concat_pieces(pieces)
    one_ctx, one = _new(world)
    one.countKmers()
    one.buildIndexUnevenCoverage(min_freq, *_solid_args(cfg))
    assert index_digest(whole) == index_digest(one.export())
    one_ctx.close()
    nK, nE, nR = len(whole.keys), len(whole.entries), len(whole.repetitive)
    for r, (ctx, vi) in enumerate(rk):
        full, _, _ = vi.gather_begin(nK, nE, nR)
        for ptr, a in zip(full, (whole.keys, whole.key_off, whole.entries, whole.repetitive)):
            _to_device(ptr, a, dev)
        torch.cuda.synchronize()
        vi.gather_end(vi._sample_rate_init)
        assert ctx.debug_probe_skip_check() == (expected, 0)
        if min_freq == 2 and r == 0:
            det = gpu.OverlapDetector.for_assemble(ctx, vi, cfg)
            check_overlaps_equal(det.getSeqOverlapsBatch(world["q"]), world["ores"], False)
        vi.keep_targets(W, r)
        assert ctx.debug_probe_skip_check() == (expected, 0)
        ctx.close()


CASES = {
    "plain": {},
    "chunked": {"FG_KMER_BUDGET": "200000", "FG_HIT_BUDGET": "20000"},
    "two_lanes": {"FG_LANES": "2", "FG_HIT_BUDGET": "20000", "FG_KMER_BUDGET": str(1 << 30)},
    "partitioned": {"FG_PROBE_PARTITION": "1", "FG_PROBE_SUB_KMERS": "300000"},
}


def _run_child(tmp_path, name, skip):
    out = str(tmp_path / f"{name}_{skip}.npz")
    env = dict(os.environ, FG_PROBE_SKIP=str(skip), **CASES[name])
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_results_identical_with_and_without_the_skip(built, world, tmp_path, name):
    off, on = _run_child(tmp_path, name, 0), _run_child(tmp_path, name, 1)
    for f in ("recs", "query_off", "stat_off", "stats", "counters"):
        assert off[f].tobytes() == on[f].tobytes(), f
    assert len(on["recs"]) > 0
    clear, bad = (int(x) for x in on["counters"][-2:])
    assert bad == 0 and clear == _expected_clear(world, 2)     # the bits were there to be used
    # and both are what the oracle says (forward and reverse-strand queries)
    ores = world["ores"]
    assert np.array_equal(on["query_off"], ores.query_off)
    assert np.array_equal(on["stats"], ores.stats.view(np.uint32))
    assert tuple(int(x) for x in on["counters"][:2]) == (ores.query_kmers, ores.seed_hits)


@pytest.mark.gpu
def test_no_bits_after_import_and_piece_split(built, world):
    from flye_amd import gpu
    ctx, vi = _new(world)
    vi.build(world["cfg"])
    assert ctx.debug_probe_skip_check()[0] > 0
    ex = vi.export()
    vi.import_index(ex, vi.getSampleRate())
    assert ctx.debug_probe_skip_check() == (0, 0)
    det = gpu.OverlapDetector.for_assemble(ctx, vi, world["cfg"])
    check_overlaps_equal(det.getSeqOverlapsBatch(world["q"]), world["ores"], False)
    # the direct option-B build gives the bits up with the split (its stated peak has no term for them)
    vi.build(world["cfg"])
    assert ctx.debug_probe_skip_check()[0] > 0
    vi.split_piece(1)
    assert ctx.debug_probe_skip_check() == (0, 0)
    check_overlaps_equal(det.getSeqOverlapsBatch(world["q"]), world["ores"], False)
    ctx.close()


@pytest.mark.gpu
def test_no_bits_for_a_minimizer_index(built):
    from flye_amd import config, gpu, synth
    from oracle import oracle as O
    rs = synth.simulate(seed=5, genome_len=60_000, coverage=20, kind="hifi03").filter_min_len(1000)
    cfg = config.preset("hifi")
    assert cfg["use_minimizers"]
    k = int(cfg["kmer_size"])
    ctx = gpu.Context(k, 0)
    ctx.set_reads(rs)
    vi = gpu.VertexIndex(ctx, float(int(cfg["assemble_kmer_sample"])))
    vi.build(cfg)
    assert ctx.debug_probe_skip_check() == (0, 0)
    o = O.Oracle(k)
    o.set_reads(rs)
    o.build_index(cfg)
    q = _all_queries(rs)
    det = gpu.OverlapDetector.for_assemble(ctx, vi, cfg)
    ores = o.overlaps(O.detector_params(cfg), q)
    assert len(ores.recs) > 0
    check_overlaps_equal(det.getSeqOverlapsBatch(q), ores, False)
    ctx.close()
