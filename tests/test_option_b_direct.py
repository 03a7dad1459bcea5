"""Option B built DIRECTLY from the key-range pieces (``fg_index_piece_split`` / ``fg_index_scatter_begin`` /
``_end``, ``dist.scatter_pieces_inplace``): no rank ever holds the full entry array.

CPU: ``dist.split_piece_host`` + ``dist.exchange_split_parts`` on 2 and 3 gloo ranks against the oracle's index.
GPU: the device split against the host one; the direct shard against the ``fg_index_keep_targets`` shard, array for
array; the overlap stage on direct shards against the full index; two gloo processes on one GPU; refusals; and the
build peak against the formula of DESIGN.md §6, with the gather + keep_targets path shown to exceed it."""
import gc
import os
import sys

import numpy as np
import pytest

from test_option_b import _detector, _free_port, _index, _reads, _run_option_b, _shard_hits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 17
PRESETS = [("raw", "pb_raw"), ("hifi", "hifi")]


def _owner(entries, world):
    return ((np.asarray(entries, np.uint64) >> np.uint64(33)) % np.uint64(world)).astype(np.int64)


# ---- CPU: host split + the exchange on CPU tensors ------------------------------------------------------------
def _exchange_worker(rank, world, port, out_dir):
    """Each rank holds the piece of the oracle's index that a key-range-sharded build would leave it with (cut as
    tests/test_dist.py cuts it), splits it on the host and runs the exchange over gloo: what it assembles must be the
    oracle's whole index filtered by (entry >> 33) % world == rank, list order kept."""
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as td
    from flye_amd import config, dist, synth
    from oracle import oracle as O
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    td.init_process_group("gloo", rank=rank, world_size=world)
    rs = synth.simulate(seed=77, genome_len=50_000, coverage=20, kind="pb_raw", n_tandems=20).filter_min_len(1000)
    cfg = config.preset("raw")
    o = O.Oracle(K, threads=2)
    o.set_reads(rs)
    o.build_index(cfg)
    full = o.export_index()
    shift = max(0, 2 * K - 12)
    cnt = np.diff(full.key_off.astype(np.int64))
    hist = np.bincount((full.keys >> np.uint64(shift)).astype(np.int64), weights=cnt, minlength=4096)
    lo, hi = dist.balanced_bin_ranges(hist, world)[rank]
    sel = ((full.keys >> np.uint64(shift)) >= lo) & ((full.keys >> np.uint64(shift)) < hi)
    idx = np.nonzero(sel)[0]
    rsel = ((full.repetitive >> np.uint64(shift)) >= lo) & ((full.repetitive >> np.uint64(shift)) < hi)
    assert len(idx) > 0
    a, b = int(full.key_off[idx[0]]), int(full.key_off[idx[-1] + 1])
    pk, po, pe = full.keys[idx], full.key_off[idx[0]:idx[-1] + 2] - np.uint64(a), full.entries[a:b]

    counts, split, totals = dist.split_piece_host(pk, po, pe, world)
    assert counts.shape == (world, len(pk)) and int(totals.sum()) == len(pe)
    assert np.array_equal(counts.sum(axis=0).astype(np.int64), np.diff(po.astype(np.int64)))
    assert np.array_equal(np.sort(split), np.sort(pe))
    seg = np.concatenate([[0], np.cumsum(totals.astype(np.int64))])
    for d in range(world):
        assert (_owner(split[seg[d]:seg[d + 1]], world) == d).all()

    def t(x):
        return torch.from_numpy(np.ascontiguousarray(x, np.uint64).view(np.int64))

    keys, off, ent, rep, (nK, nE, nR), e_shard, moved = dist.exchange_split_parts(
        t(pk), t(full.repetitive[rsel]), t(counts.reshape(-1)), t(split), totals, rank, world, on_device=False)
    assert (nK, nE, nR) == (len(full.keys), len(full.entries), len(full.repetitive))
    own = _owner(full.entries, world) == rank
    assert e_shard == int(own.sum()) and 0 < e_shard < nE
    assert np.array_equal(keys.numpy().view(np.uint64), full.keys)
    assert np.array_equal(rep.numpy().view(np.uint64), full.repetitive)
    assert np.array_equal(ent.numpy().view(np.uint64), full.entries[own])          # every list filtered, in its order
    key_of = np.repeat(np.arange(nK, dtype=np.int64), cnt)
    want_counts = np.bincount(key_of[own], minlength=nK)
    assert np.array_equal(off.numpy()[:nK], want_counts)       # the counts, as scatter_end receives them
    # ... whose exclusive scan is the shard's key_off
    assert np.array_equal(np.concatenate([[0], np.cumsum(off.numpy()[:nK])])[:-1],
                          np.concatenate([[0], np.cumsum(want_counts)])[:-1])
    assert moved >= 8 * (nK + nR)
    open(os.path.join(out_dir, f"ok{rank}"), "w").write(str(e_shard))
    td.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_split_host_and_exchange_gloo(built, tmp_path, world):
    import torch.multiprocessing as mp
    mp.spawn(_exchange_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    assert all(int(open(tmp_path / f"ok{r}").read()) > 1000 for r in range(world))


def test_split_piece_host_small():
    """two keys, three destinations, by hand: destination major, key major, list order"""
    from flye_amd import dist

    def e(read, pos):
        return ((2 * read) << 32) | pos

    ent = np.array([e(0, 5), e(1, 1), e(3, 2), e(4, 9), e(2, 7), e(5, 3), e(8, 1)], np.uint64)
    counts, split, totals = dist.split_piece_host(np.array([10, 20], np.uint64), np.array([0, 4, 7], np.uint64), ent, 3)
    assert counts.tolist() == [[2, 0], [2, 0], [0, 3]] and totals.tolist() == [2, 2, 3]
    assert split.tolist() == [e(0, 5), e(3, 2), e(1, 1), e(4, 9), e(2, 7), e(5, 3), e(8, 1)]


# ---- GPU helpers: pieces as contexts on device 0, split parts through the host -----------------------------------
def _cuda():
    import torch
    return torch.device("cuda", 0)


def _to_host(ptr, n):
    from flye_amd import dist
    return dist._view(ptr, n, _cuda()).cpu().numpy().view(np.uint64).copy()


def _to_device(ptr, arr):
    import torch
    from flye_amd import dist
    if len(arr):
        dist._view(ptr, len(arr), _cuda()).copy_(torch.from_numpy(np.ascontiguousarray(arr, np.uint64).view(np.int64)))


def _new_vi(rs, cfg, first_id=0):
    from flye_amd import gpu
    ctx = gpu.Context(K, 0)
    ctx.set_reads(rs, first_id)
    return ctx, gpu.VertexIndex(ctx, float(int(cfg["assemble_kmer_sample"])))


def _pieces(rs, cfg, world, first_id=0):
    """``world`` contexts; context r holds the finished piece of key range r (the build of dist._build_piece without
    the process group: the two sums are added up here)"""
    from flye_amd import dist
    out, sums = [], np.zeros(2, np.uint64)
    for r in range(world):
        ctx, vi = _new_vi(rs, cfg, first_id)
        ranges = dist.balanced_bin_ranges(vi.begin(cfg), world)
        sums += vi.build_range(*ranges[r])
        out.append((ctx, vi))
    for _, vi in out:
        vi.finish(sums)
    return out


def _split_parts(vi, world):
    """the piece and its device split, on the host"""
    x = vi.export()
    cnt_ptr, ent_ptr, totals = vi.split_piece(world)
    return dict(keys=x.keys, key_off=x.key_off, entries=x.entries, rep=x.repetitive,
                counts=_to_host(cnt_ptr, world * len(x.keys)).reshape(world, len(x.keys)),
                split=_to_host(ent_ptr, len(x.entries)), totals=totals)


def _shard_arrays(parts, d):
    """what rank d receives from the sources in rank order: (keys, count rows, entry segments, repetitive)"""
    segs = []
    for p in parts:
        b = np.concatenate([[0], np.cumsum(p["totals"].astype(np.int64))])
        segs.append(p["split"][b[d]:b[d + 1]])
    return (np.concatenate([p["keys"] for p in parts]), np.concatenate([p["counts"][d] for p in parts]),
            np.concatenate(segs), np.concatenate([p["rep"] for p in parts]))


def _scatter(vi, arrays, world, d, sample_rate):
    import torch
    keys, counts, ent, rep = arrays
    full = vi.scatter_begin(world, d, len(keys), len(ent), len(rep))
    for ptr, a in zip(full, (keys, counts, ent, rep)):
        _to_device(ptr, a)
    torch.cuda.synchronize()
    vi.scatter_end(sample_rate)


def _sample_rate(cfg, rs, vi, n_entries):
    """VertexIndex::getSampleRate() of the whole index, as dist._build_piece's sample_rate_of gives it"""
    if cfg["use_minimizers"]:
        return float(np.float32(rs.total_bases) / np.float32(n_entries))
    return vi._sample_rate_init


def _direct_shards(rs, cfg, world, first_id=0):
    """-> [(ctx, vi)] per rank, built from the ranks' pieces without a full index anywhere; the total entry count"""
    pcs = _pieces(rs, cfg, world, first_id)
    parts = [_split_parts(vi, world) for _, vi in pcs]
    total = sum(len(p["entries"]) for p in parts)
    for d, (_, vi) in enumerate(pcs):
        _scatter(vi, _shard_arrays(parts, d), world, d, _sample_rate(cfg, rs, vi, total))
    return pcs, total


# ---- GPU: the device split against the host reference ---------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3, 8, 64])
@pytest.mark.parametrize("preset,kind", PRESETS)
def test_device_split_equals_host_split(built, preset, kind, world):
    """count matrix, split entries and totals; a piece that is the whole index and the piece of a real key range;
    the split kernels report their time under their own names"""
    from flye_amd import config, dist
    cfg = config.preset(preset)
    rs = _reads(kind, seed=23)
    ctx_a, whole = _new_vi(rs, cfg)
    whole.build(cfg)
    ctx_b, part = _new_vi(rs, cfg)
    part.begin(cfg)
    part.build_range(700, 2900)
    part.finish(None)
    (nk_a, _, _), _ = whole.device_arrays()
    (nk_b, ne_b, _), _ = part.device_arrays()
    assert 0 < nk_b < nk_a and ne_b > 0
    for ctx, vi in ((ctx_a, whole), (ctx_b, part)):
        p = _split_parts(vi, world)
        times = ctx.kernel_times()
        for name in ("k_split_count", "k_split_scan", "k_split_copy"):
            assert name in times, (name, sorted(times))
        counts, split, totals = dist.split_piece_host(p["keys"], p["key_off"], p["entries"], world)
        assert np.array_equal(p["totals"], totals)
        assert np.array_equal(p["counts"], counts)
        assert np.array_equal(p["split"], split)
        assert int((totals > 0).sum()) >= min(world, 8)          # the destinations are really used
        after = vi.export()                                       # the piece itself is untouched
        assert np.array_equal(after.entries, p["entries"]) and np.array_equal(after.key_off, p["key_off"])
        ctx.close()


# ---- GPU: the direct shard against the keep_targets shard -----------------------------------------------------------
def _check_direct_equals_keep_targets(rs, cfg, world, first_id):
    ctx, vi_full = _index(rs, cfg, first_id)
    want_rate = np.float32(vi_full.getSampleRate()).tobytes()
    n_full = len(vi_full.export().entries)
    ctx.close()
    shards, total = _direct_shards(rs, cfg, world, first_id)
    assert total == n_full
    kept = 0
    for r, (c, v) in enumerate(shards):
        cw, want = _index(rs, cfg, first_id)
        want.keep_targets(world, r)
        assert v.shard() == want.shard() == (world, r)
        a, b = v.export(), want.export()
        for f in ("keys", "key_off", "entries", "repetitive"):
            assert np.array_equal(getattr(a, f), getattr(b, f)), (f, r)
        assert np.float32(_sample_rate(cfg, rs, v, total)).tobytes() == want_rate
        kept += len(a.entries)
        cw.close()
        c.close()
    assert kept == n_full


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("preset,kind", PRESETS)
def test_direct_shard_equals_keep_targets_shard(built, preset, kind, world):
    from flye_amd import config
    _check_direct_equals_keep_targets(_reads(kind, seed=8), config.preset(preset), world, 0)


@pytest.mark.gpu
def test_direct_shard_equals_keep_targets_shard_first_id(built):
    from flye_amd import config
    _check_direct_equals_keep_targets(_reads("pb_raw", seed=77), config.preset("raw"), 3, 10)


# ---- GPU: the overlap stage on direct shards --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("preset,kind", PRESETS)
def test_option_b_on_direct_shards_equals_full_index(built, preset, kind, world):
    """records, offsets, divergence statistics and counters (test_option_b._same) of every owner's queries; the
    self hit is dropped through the "owns an entry" bits scatter_end builds, so a wrong bit changes seed_hits"""
    from flye_amd import config, gpu
    cfg = config.preset(preset)
    rs = _reads(kind)
    ctx, vi = _index(rs, cfg)
    full = _detector(ctx, vi, cfg)
    pcs, _ = _direct_shards(rs, cfg, world)
    shards = [_detector(c, v, cfg) for c, v in pcs]
    q = np.arange(0, 2 * rs.n, 2, dtype=np.uint32)
    probes = _run_option_b(full, shards, q, (q >> 1) % world, np.random.default_rng(world))
    fc, fh = _shard_hits(full, q)
    assert np.array_equal(sum(c for c, _ in probes), fc)
    # tied (extId, curPos) keys exist: the receiver's re-ordering decides the unstable sort's result
    keys = np.stack([np.repeat(np.arange(len(fc)), fc.astype(np.int64)), fh["ext_id"].astype(np.int64),
                     fh["cur_pos"].astype(np.int64)], axis=1)
    assert len(np.unique(keys, axis=0)) < len(keys)
    with pytest.raises(gpu.FlyeGpuError) as e:                  # a direct shard refuses what a keep_targets shard refuses
        shards[0].getSeqOverlapsBatch(q)
    assert e.value.code == -4 and "fg_overlaps_from_hits" in str(e.value)
    with pytest.raises(gpu.FlyeGpuError) as e:
        gpu.BatchingOverlapContainer(shards[0])
    assert e.value.code == -4


# ---- GPU: two gloo processes on one GPU ----------------------------------------------------------------------------
def _gloo_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    import torch.distributed as td
    from flye_amd import config, dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    td.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    for preset, kind in PRESETS:
        cfg = config.preset(preset)
        rs = _reads(kind, seed=91)
        ctx, vi = _new_vi(rs, cfg)
        st = dist.build_index_option_b_direct(vi, cfg, rank, world, on_device=False)
        assert vi.shard() == (world, rank)
        det = _detector(ctx, vi, cfg)
        res, moved = dist.overlaps_option_b(det, rank, world, on_device=False, batch_reads=64)
        ctx1, vi1 = _index(rs, cfg)
        one = _detector(ctx1, vi1, cfg).getSeqOverlapsBatch(np.arange(0, 2 * rs.n, 2, dtype=np.uint32))
        lines1 = one.lines()
        got = [l for _, r in res for l in r.lines()]
        want = [l for i in range(rank, rs.n, world) for l in lines1[int(one.query_off[i]):int(one.query_off[i + 1])]]
        assert got == want and len(want) > 0, preset
        assert st["index_entries"] == vi1.stats["index_entries"] and 0 < st["shard_entries"] < st["index_entries"]
        assert st["selected_kmers"] == vi1.stats["selected_kmers"]
        assert np.float32(vi.getSampleRate()).tobytes() == np.float32(vi1.getSampleRate()).tobytes()
        assert st["collective_bytes"] > 0 and st["scatter_s"] > 0
        out[preset] = (st["index_entries"], st["shard_entries"], moved)
        ctx.close()
        ctx1.close()
    open(os.path.join(out_dir, f"d_gpu{rank}"), "w").write(repr(out))
    td.destroy_process_group()


@pytest.mark.gpu
def test_two_rank_direct_option_b_on_device(built, tmp_path):
    """two processes on one GPU, collectives through gloo: build_index_option_b_direct + overlaps_option_b; the
    merged lists equal the single-process ones; the two shards hold the whole index between them"""
    import torch.multiprocessing as mp
    mp.spawn(_gloo_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r = [eval(open(tmp_path / f"d_gpu{k}").read()) for k in range(2)]
    for preset, _ in PRESETS:
        assert r[0][preset][0] == r[1][preset][0] == r[0][preset][1] + r[1][preset][1]
        assert r[0][preset][2] > 0 and r[1][preset][2] > 0


# ---- GPU: refusals ---------------------------------------------------------------------------------------------------
def _code(fn, *a):
    from flye_amd import gpu
    with pytest.raises(gpu.FlyeGpuError) as e:
        fn(*a)
    return e.value.code, str(e.value)


@pytest.mark.gpu
def test_direct_build_refusals(built):
    """call order and argument errors give the stated codes; wrong DATA handed to scatter_end (a foreign entry, a
    descending list, counts that do not add up, keys out of order) is found by the device checks before any list is
    read through it; afterwards the context holds no index and a fresh build makes it usable again"""
    from flye_amd import config
    cfg = config.preset("raw")
    rs = _reads("pb_raw", seed=19, genome_len=30_000)
    q = np.arange(0, 2 * rs.n, 2, dtype=np.uint32)
    ctx, vi = _new_vi(rs, cfg)
    assert _code(vi.split_piece, 2)[0] == -4                    # no finished piece
    assert _code(vi.scatter_end, 1.0)[0] == -4                  # no scatter in progress
    vi.build(cfg)
    det = _detector(ctx, vi, cfg)
    want = det.getSeqOverlapsBatch(q).lines()
    assert _code(vi.split_piece, 0)[0] == -3
    assert _code(vi.split_piece, vi.SPLIT_MAX_WORLD + 1)[0] == -3
    assert _code(vi.scatter_begin, 2, 0, 1, 1, 1)[0] == -4      # no split yet
    world = 2
    p = _split_parts(vi, world)
    assert det.getSeqOverlapsBatch(q).lines() == want           # the split leaves the index as it was
    assert _code(vi.scatter_begin, world, world, 1, 1, 1)[0] == -3      # rank >= world
    assert _code(vi.scatter_begin, 3, 0, 1, 1, 1)[0] == -4      # the split was for another world
    rate = vi.getSampleRate()
    keys, counts, ent, rep = _shard_arrays([p], 0)
    long_lists = np.nonzero(counts >= 2)[0]
    assert len(long_lists) and len(ent) > 2 and len(keys) > 2
    off = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])

    def foreign():
        e = ent.copy()
        e[len(e) // 2] += np.uint64(2 << 32)                    # the next read: the other rank's
        return keys, counts, e, rep

    def descending():
        e = ent.copy()
        o = int(off[long_lists[len(long_lists) // 2]])
        e[o], e[o + 1] = ent[o + 1], ent[o]
        return keys, counts, e, rep

    def short_counts():
        c = counts.copy()
        c[long_lists[0]] -= np.uint64(1)
        return keys, c, ent, rep

    def unsorted_keys():
        k = keys.copy()
        k[1], k[2] = keys[2], keys[1]
        return k, counts, ent, rep

    for bad, text in ((foreign, "another rank"), (descending, "ascending"), (short_counts, "malformed"),
                      (unsorted_keys, "malformed")):
        code, msg = _code(_scatter, vi, bad(), world, 0, rate)
        assert code == -3 and text in msg, (bad.__name__, code, msg)
        assert vi.shard() == (1, 0)
        assert _code(vi.device_arrays)[0] == -4                 # no index left behind
        assert _code(det.probe_hits, q)[0] == -4
        vi.build(cfg)
        assert det.getSeqOverlapsBatch(q).lines() == want
        _split_parts(vi, world)
    # the good arrays pass; a shard refuses a second restriction of either kind
    _scatter(vi, (keys, counts, ent, rep), world, 0, rate)
    assert vi.shard() == (world, 0)
    assert _code(vi.split_piece, world)[0] == -4
    assert _code(vi.keep_targets, 3, 0)[0] == -4
    vi.clear()
    vi.build(cfg)
    vi.keep_targets(world, 1)
    assert _code(vi.split_piece, world)[0] == -4                # a keep_targets shard is restricted too
    vi.clear()
    assert vi.shard() == (1, 0)
    vi.build(cfg)
    assert det.getSeqOverlapsBatch(q).lines() == want
    ctx.close()


# ---- GPU: the memory the direct build needs ---------------------------------------------------------------------------
def _table_bytes(n_keys, n_rep):
    """the lookup table's sizing rule (fgIndexLookupStructures, k <= 17: 8-byte slots in groups of 8; load 0.25 while
    (keys + repetitive) * 32 B <= 2 GiB, else 0.5; one part below 2^30 keys)"""
    n = n_keys + n_rep
    load = 25 if n * 32 <= (2 << 30) else 50
    return max(16, (n * 100 // load + 7) // 8) * 64


def direct_build_peak_bound(world, k_piece, e_piece, r_piece, n_keys, n_rep, e_shard, total_kmers):
    """DESIGN.md §6, "Option B built directly": library device bytes above the resident reads, at most, between
    fg_index_finish and the end of fg_index_scatter_end.  No term in the total entry count.
      piece   P = 8 (2 K_s + 1 + E_s + R_s)       keys, offsets, entries, repetitive keys of the own piece
      shard   S = 8 (2 K + 1 + R + E_shard)       the same of the shard (keys and repetitive keys are replicated)
      bits    B = 4 (ceil(k-mer positions / 32) + 1);  tables T_s (piece), T (shard) by the sizing rule above
      split     P + T_s + B + 8 E_s + 16 (W K_s + 1)   counts + write offsets + split entries beside the usable piece
      exchange  P + 8 E_s + 8 (W K_s + 1) + S          the piece's table and bits are gone, the shard's arrays are there
      end       S + T + B                              piece and split buffers are gone
    slack, from what the allocations are: the scans' tile sums (one 8-byte element per 2048 scanned, recursively: below
    8 n / 1024 bytes for the n = W K_s + K + 2 elements scanned) + the flag / total buffers of 4 .. 1024 bytes each,
    a dozen at most: 64 KiB covers them."""
    P = 8 * (2 * k_piece + 1 + e_piece + r_piece)
    S = 8 * (2 * n_keys + 1 + n_rep + e_shard)
    B = 4 * ((total_kmers + 31) // 32 + 1)
    split = P + _table_bytes(k_piece, r_piece) + B + 8 * e_piece + 16 * (world * k_piece + 1)
    exchange = P + 8 * e_piece + 8 * (world * k_piece + 1) + S
    end = S + _table_bytes(n_keys, n_rep) + B
    slack = 8 * ((world * k_piece + n_keys + 2) // 1024 + 1) + (64 << 10)
    return max(split, exchange, end) + slack, dict(split=split, exchange=exchange, end=end, slack=slack)


@pytest.mark.gpu
def test_direct_build_peak_has_no_term_in_the_total_entries(built):
    """>= 50 Mbp of reads, world = 4, rank 1, one context alive at a time, the other ranks' split parts on the host.
    Peak (fg_memory_stats, reset after finish) of split + scatter <= direct_build_peak_bound; the gather +
    keep_targets path on the same input exceeds that bound.  The figures are printed (run with -s)."""
    import torch
    from flye_amd import config, dist, gpu
    gc.collect()
    cfg = config.preset("raw")
    rs = _reads("pb_raw", seed=3, genome_len=2_000_000, coverage=26)
    assert rs.total_bases >= 50_000_000
    total_kmers = int(np.maximum(rs.length.astype(np.int64) - K, 0).sum())
    world, me = 4, 1
    # the whole index once: the two sums of filterFrequentKmers, the bin ranges, and the arrays the gather path lands
    ctx, vi = _new_vi(rs, cfg)
    reads_bytes = gpu.memory_stats()[0]
    ranges = dist.balanced_bin_ranges(vi.begin(cfg), world)
    sums = vi.build_range(0, vi.INDEX_BINS)
    vi.finish(sums)
    whole = vi.export()
    nK, nE, nR = len(whole.keys), len(whole.entries), len(whole.repetitive)
    mine = _owner(whole.entries, world) == me
    ctx.close()

    def piece_of(r):
        c, v = _new_vi(rs, cfg)
        v.begin(cfg)
        v.build_range(*ranges[r])
        v.finish(sums)
        return c, v

    parts = [None] * world
    for r in range(world):
        if r != me:
            c, v = piece_of(r)
            parts[r] = _split_parts(v, world)
            c.close()
    # --- the direct path
    c, v = piece_of(me)
    (ks, es, rs_), _ = v.device_arrays()
    gpu.memory_stats(reset_peak=True)
    parts[me] = _split_parts(v, world)
    t_split = c.kernel_times()
    arrays = _shard_arrays(parts, me)
    _scatter(v, arrays, world, me, v._sample_rate_init)
    t_end = c.kernel_times()
    now, peak = gpu.memory_stats()
    e_shard = len(arrays[2])
    assert v.shard() == (world, me) and e_shard == int(mine.sum())
    got = v.export()
    assert np.array_equal(got.entries, whole.entries[mine])
    assert np.array_equal(got.keys, whole.keys) and np.array_equal(got.repetitive, whole.repetitive)
    bound, terms = direct_build_peak_bound(world, ks, es, rs_, nK, nR, e_shard, total_kmers)
    print(f"\ndirect build: K={nK} R={nR} E={nE} piece=({ks},{es},{rs_}) shard={e_shard} reads={reads_bytes} B "
          f"peak above reads={peak - reads_bytes} resident above reads={now - reads_bytes} bound={bound} terms={terms} "
          f"8E={8 * nE} = {8 * nE / terms['slack']:.0f} x slack")
    print("split kernels (s, launches):", {n: t_split[n] for n in t_split if n.startswith("k_split")})
    print("scatter_end kernels:", t_end)
    assert now - reads_bytes <= terms["end"] + terms["slack"]
    assert peak - reads_bytes <= bound
    assert 8 * nE > 16 * terms["slack"]          # the slack could not hide a full entry array
    c.close()
    # --- the existing path on the same input: gather the whole index, then keep_targets
    c, v = piece_of(me)
    gpu.memory_stats(reset_peak=True)
    full, _, psz = v.gather_begin(nK, nE, nR)
    assert psz == [ks, es, rs_]
    for ptr, a in zip(full, (whole.keys, whole.key_off, whole.entries, whole.repetitive)):
        _to_device(ptr, a)
    torch.cuda.synchronize()
    v.gather_end(v._sample_rate_init)
    assert v.keep_targets(world, me) == e_shard
    t_keep = c.kernel_times()
    peak_gather = gpu.memory_stats()[1]
    print(f"gather + keep_targets: peak above reads={peak_gather - reads_bytes} "
          f"({(peak_gather - reads_bytes) / bound:.2f} x the direct bound)")
    print("keep_targets kernels:", {n: t_keep[n] for n in t_keep if n.startswith("k_keep")})
    assert peak_gather - reads_bytes > bound
    assert np.array_equal(v.export().entries, got.entries)
    c.close()
