"""Option B of the multi-GPU layout: the index sharded by TARGET read, seed hits exchanged.

CPU: the exchange plumbing of ``dist.overlaps_option_b`` on 2 and 3 gloo ranks with a stand-in detector.
GPU: W shards as W contexts on one device (``fg_index_keep_targets``), every shard probes every query
(``fg_probe_hits``), each owner gets its queries' runs with the sources permuted and every run shuffled, and
``fg_overlaps_from_hits`` must give what ``fg_overlaps`` gives on the full index, record for record."""
import os
import socket
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ---- CPU: the exchange plumbing ------------------------------------------------------------------------------
FIRST = 6


def _standin_count(read, rank):
    return (read * 7 + rank * 3) % 5            # zero for some (query, source) pairs


class _StandIn:
    """A detector whose shard emits numpy hits: from source rank s, read i gets _standin_count(i, s) hits
    (cur_pos = j, ext_pos = s, ext_id = i); the receiver keeps what it was handed."""

    def __init__(self, n_reads, rank):
        self.ctx = types.SimpleNamespace(n_reads=n_reads, first_id=FIRST)
        self.rank = rank
        self.got = []

    def probe_hits(self, q):
        from flye_amd import gpu
        reads = (np.asarray(q, np.int64) - FIRST) >> 1
        counts = np.array([_standin_count(int(i), self.rank) for i in reads], np.uint64)
        hits = np.zeros(int(counts.sum()), gpu.SEED_HIT_DTYPE)
        at = 0
        for i, c in zip(reads, counts):
            c = int(c)
            hits["cur_pos"][at:at + c] = np.arange(c)
            hits["ext_pos"][at:at + c] = self.rank
            hits["ext_id"][at:at + c] = i
            at += c
        return counts, hits, len(hits)

    def getSeqOverlapsFromHits(self, mine, counts, hits):
        self.got.append((np.asarray(mine).copy(), np.asarray(counts).copy(), hits.cpu().numpy().copy()))
        return len(mine)


def _plumbing_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    import torch.distributed as td
    from flye_amd import dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    td.init_process_group("gloo", rank=rank, world_size=world)
    n_reads, batch = 23, 7
    det = _StandIn(n_reads, rank)
    out, moved = dist.overlaps_option_b(det, rank, world, on_device=False, batch_reads=batch)
    assert len(out) == len(det.got) == (n_reads + batch - 1) // batch
    runs = 0
    for b, (mine, counts, hits) in enumerate(det.got):
        reads = np.arange(b * batch, min(n_reads, (b + 1) * batch))
        want = reads[reads % world == rank]
        assert np.array_equal(mine, FIRST + 2 * want)
        assert counts.shape == (world, len(want))
        at = 0
        for s in range(world):                  # sources in rank order, inside a source the queries in batch order
            for t, i in enumerate(want):
                c = _standin_count(int(i), s)
                assert counts[s, t] == c
                run = hits[at:at + c]
                assert np.array_equal(run[:, 0], np.arange(c)) and (run[:, 1] == s).all() and (run[:, 2] == i).all()
                at += c
                runs += 1
        assert at == len(hits)
    sent = sum(_standin_count(i, rank) for i in range(n_reads) if i % world != rank)
    assert moved == 12 * sent
    open(os.path.join(out_dir, f"plumb{rank}"), "w").write(str(runs))
    td.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_option_b_exchange_plumbing_gloo(tmp_path, world):
    """counts, then hits, with all_to_all_single: every rank receives exactly its queries' runs, sources in rank order"""
    import torch.multiprocessing as mp
    mp.spawn(_plumbing_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    assert sum(int(open(tmp_path / f"plumb{r}").read()) for r in range(world)) == 23 * world


# ---- GPU: W shards as W contexts on device 0 ------------------------------------------------------------------
def _reads(kind, seed=41, genome_len=60_000, coverage=20):
    from flye_amd import synth
    return synth.simulate(seed=seed, genome_len=genome_len, coverage=coverage, kind=kind, n_repeat_families=4,
                          n_tandems=20, n_homopolymers=8).filter_min_len(1000)


def _index(rs, cfg, first_id=0, qrs=None, q_first=None):
    from flye_amd import gpu
    ctx = gpu.Context(17, 0)
    ctx.set_reads(rs, first_id)
    if qrs is not None:
        ctx.set_queries(qrs, q_first)
    vi = gpu.VertexIndex(ctx, float(int(cfg["assemble_kmer_sample"])))
    vi.build(cfg)
    return ctx, vi


def _detector(ctx, vi, cfg, **p):
    from flye_amd import gpu
    det = gpu.OverlapDetector.for_assemble(ctx, vi, cfg)
    det.p.max_divergence = 0.3
    for k, v in p.items():
        setattr(det.p, k, v)
    return det


def _same(got, want):
    assert got.lines() == want.lines()
    assert len(want.recs) > 0
    for a in ("query_off", "stat_off"):
        assert np.array_equal(getattr(got, a), getattr(want, a)), a
    assert got.stats.view(np.uint32).tolist() == want.stats.view(np.uint32).tolist()
    for a in ("seed_hits", "query_kmers", "query_bp", "dp_groups", "dp_elements", "dp_elements_small"):
        assert getattr(got, a) == getattr(want, a), a
    for a in ("match_off", "matches", "needs_trim"):
        g, w = getattr(got, a), getattr(want, a)
        assert (g is None) == (w is None), a
        if w is not None:
            assert np.array_equal(g, w), a


def _shard_hits(det, q):
    from flye_amd import gpu
    counts, ptr, n = det.probe_hits(q)
    assert int(counts.sum()) == n
    return counts, gpu.seed_hits_to_host(ptr, n)


def _run_option_b(full, shards, q, owner, rng, **call):
    """every shard probes all of q; owner o gets its queries' runs, sources permuted, runs shuffled; the result must
    equal the full index's.  Returns the shards' (counts, hits)."""
    world = len(shards)
    probes = [_shard_hits(d, q) for d in shards]
    offs = [np.concatenate([[0], np.cumsum(c.astype(np.int64))]) for c, _ in probes]
    for o in range(world):
        sel = np.nonzero(owner == o)[0]
        mine = q[sel]
        counts = np.zeros((world, len(sel)), np.uint64)
        parts = []
        for j, s in enumerate(rng.permutation(world)):
            for t, qi in enumerate(sel):
                run = probes[s][1][offs[s][qi]:offs[s][qi + 1]]
                parts.append(run[rng.permutation(len(run))])
                counts[j, t] = len(run)
        got = shards[o].getSeqOverlapsFromHits(mine, counts, np.concatenate(parts), **call)
        _same(got, full.getSeqOverlapsBatch(mine, **call))
    return probes


def _tagged(counts, hits):
    qi = np.repeat(np.arange(len(counts)), counts.astype(np.int64))
    rows = np.stack([qi, hits["cur_pos"].astype(np.int64), hits["ext_pos"].astype(np.int64),
                     hits["ext_id"].astype(np.int64)], axis=1)
    return rows[np.lexsort(rows.T[::-1])]


# FG_RECV_TWO_PASS=1: the receiver restores the emission order with two stable sorts (stored side, then query k-mer),
# the form a read set takes whose full key exceeds 64 bits
TWO_PASS = [pytest.param(False, id="auto"), pytest.param(True, id="two_pass")]


def _recv_form(monkeypatch, two_pass):
    if two_pass:
        monkeypatch.setenv("FG_RECV_TWO_PASS", "1")
    else:
        monkeypatch.delenv("FG_RECV_TWO_PASS", raising=False)


# The hit form the receiver writes (recvFill / k_recv_place): 32-bit keys on read sets of this size, and with the
# switches the two forms a read set too large for 32 key bits takes -- packed records, 64-bit keys beside values.
KEY_FORMS = {"key32": {}, "key64": {"FG_FORCE_KEY64": "1"}, "key64_unpacked": {"FG_FORCE_KEY64": "1", "FG_PACKED_KEYS": "0"}}


def _key_form(monkeypatch, form):
    for sw in ("FG_FORCE_KEY64", "FG_PACKED_KEYS"):
        monkeypatch.delenv(sw, raising=False)
    for sw, value in KEY_FORMS[form].items():
        monkeypatch.setenv(sw, value)


def _full_index_params():
    out = []
    for preset, kind in (("raw", "pb_raw"), ("hifi", "hifi")):
        for world, two_pass in ((2, False), (3, False), (2, True), (3, True)):
            for form in KEY_FORMS:
                if form != "key32" and not (preset == "raw" and world == 2):
                    continue
                name = f"{preset}-{kind}-{world}" + ("-two_pass" if two_pass else "") + ("" if form == "key32" else "-" + form)
                out.append(pytest.param(preset, kind, world, two_pass, form, id=name))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("preset,kind,world,two_pass,key_form", _full_index_params())
def test_option_b_equals_full_index(built, monkeypatch, preset, kind, world, two_pass, key_form):
    from flye_amd import config
    _recv_form(monkeypatch, two_pass)
    _key_form(monkeypatch, "key32")
    cfg = config.preset(preset)
    rs = _reads(kind)
    ctx, vi = _index(rs, cfg)
    full = _detector(ctx, vi, cfg)
    shards = []
    for r in range(world):
        c, v = _index(rs, cfg)
        v.keep_targets(world, r)
        shards.append(_detector(c, v, cfg))
    q = np.arange(0, 2 * rs.n, 2, dtype=np.uint32)
    plain = full.getSeqOverlapsBatch(q) if key_form != "key32" else None
    _key_form(monkeypatch, key_form)
    probes = _run_option_b(full, shards, q, (q >> 1) % world, np.random.default_rng(world))
    if plain is not None:       # and the form changes nothing
        _same(full.getSeqOverlapsBatch(q), plain)
    # the shards' hits are exactly the full index's, split by target owner
    fc, fh = _shard_hits(full, q)
    assert np.array_equal(sum(c for c, _ in probes), fc)
    rows = np.concatenate([_tagged(c, h) for c, h in probes])
    assert np.array_equal(_tagged(fc, fh), rows[np.lexsort(rows.T[::-1])])
    # tied (extId, curPos) keys exist: the re-ordering decides the unstable sort's result
    keys = np.stack([np.repeat(np.arange(len(fc)), fc.astype(np.int64)), fh["ext_id"].astype(np.int64),
                     fh["cur_pos"].astype(np.int64)], axis=1)
    assert len(np.unique(keys, axis=0)) < len(keys)


@pytest.mark.gpu
@pytest.mark.parametrize("two_pass,key_form",
                         [pytest.param(tp, form, id=tid + ("" if form == "key32" else "-" + form))
                          for tp, tid in ((False, "auto"), (True, "two_pass")) for form in KEY_FORMS])
def test_option_b_repeat_stage_flags_rc_queries_first_id(built, monkeypatch, two_pass, key_form):
    """only_max_ext = 0, keep_alignment, partition_bad_mappings; max_overlaps > 0; reverse-complement query ids;
    first_seq_id != 0; in every hit form (the match arrays of the 64-bit forms come from what k_recv_place<PK> and
    k_recv_place<u64> wrote)"""
    from flye_amd import config
    _recv_form(monkeypatch, two_pass)
    _key_form(monkeypatch, "key32")
    cfg = config.preset("raw")
    rs = _reads("pb_raw", seed=77)
    first, world = 10, 2
    ctx, vi = _index(rs, cfg, first)
    flags = dict(only_max_ext=0, keep_alignment=1)
    full = _detector(ctx, vi, cfg, partition_bad_mappings=1, **flags)
    full_cut = _detector(ctx, vi, cfg, **flags)
    shards, shards_cut = [], []
    for r in range(world):
        c, v = _index(rs, cfg, first)
        v.keep_targets(world, r)
        shards.append(_detector(c, v, cfg, partition_bad_mappings=1, **flags))
        shards_cut.append(_detector(c, v, cfg, **flags))
    q = (first + np.arange(1, 2 * rs.n, 2)).astype(np.uint32)          # reverse-complement strands
    owner = ((q - first) >> 1) % world
    rng = np.random.default_rng(3)
    plain = plain_cut = None
    if key_form != "key32":
        plain, plain_cut = full.getSeqOverlapsBatch(q), full_cut.getSeqOverlapsBatch(q, maxOverlaps=3)
    _key_form(monkeypatch, key_form)
    _run_option_b(full, shards, q, owner, rng)
    got = full.getSeqOverlapsBatch(q)
    assert got.needs_trim is not None and len(got.matches) > 0
    _run_option_b(full_cut, shards_cut, q, owner, rng, maxOverlaps=3)
    if plain is not None:       # and the form changes nothing
        _same(got, plain)
        _same(full_cut.getSeqOverlapsBatch(q, maxOverlaps=3), plain_cut)


@pytest.mark.gpu
def test_option_b_separate_query_container(built):
    """queries in a container of their own (fg_set_queries: the ReadAligner shape, read_aligner.cpp:178-217)"""
    from flye_amd import config
    cfg = config.preset("raw")
    rs = _reads("pb_raw", seed=12)
    qrs = _reads("pb_raw", seed=12, coverage=6)
    q_first, world = 2 * rs.n, 3
    ctx, vi = _index(rs, cfg, 0, qrs, q_first)
    full = _detector(ctx, vi, cfg, only_max_ext=0)
    shards = []
    for r in range(world):
        c, v = _index(rs, cfg, 0, qrs, q_first)
        v.keep_targets(world, r)
        shards.append(_detector(c, v, cfg, only_max_ext=0))
    q = (q_first + np.arange(0, 2 * qrs.n)).astype(np.uint32)           # both strands
    _run_option_b(full, shards, q, ((q - q_first) >> 1) % world, np.random.default_rng(5))


@pytest.mark.gpu
@pytest.mark.parametrize("preset,kind", [("raw", "pb_raw"), ("hifi", "hifi")])
def test_shard_export_against_full_index(built, preset, kind):
    from flye_amd import config
    cfg = config.preset(preset)
    rs = _reads(kind, seed=8)
    world = 3
    ctx, vi = _index(rs, cfg)
    fx = vi.export()
    total = 0
    for r in range(world):
        c, v = _index(rs, cfg)
        kept = v.keep_targets(world, r)
        assert v.shard() == (world, r)
        x = v.export()
        assert np.array_equal(x.keys, fx.keys) and np.array_equal(x.repetitive, fx.repetitive)
        assert np.array_equal(x.entries, fx.entries[((fx.entries >> np.uint64(33)) % np.uint64(world)) == r])
        # each key's list: the full list filtered, in order
        lens = np.diff(fx.key_off.astype(np.int64))
        keep = ((fx.entries >> np.uint64(33)) % np.uint64(world)) == r
        per_key = np.add.reduceat(keep.astype(np.int64), fx.key_off[:-1].astype(np.int64)) if len(keep) else keep
        per_key = np.where(lens > 0, per_key, 0)
        assert np.array_equal(np.diff(x.key_off.astype(np.int64)), per_key)
        assert kept == len(x.entries)
        assert np.float32(v.getSampleRate()).tobytes() == np.float32(vi.getSampleRate()).tobytes()
        total += kept
    assert total == len(fx.entries)


@pytest.mark.gpu
def test_keep_targets_gives_the_entry_memory_back(built):
    """>= 50 Mbp of reads: fg_memory_stats drops by at least 90 % of the removed entry bytes"""
    from flye_amd import config, gpu
    cfg = config.preset("raw")
    rs = _reads("pb_raw", seed=3, genome_len=2_000_000, coverage=26)
    assert rs.total_bases >= 50_000_000
    ctx, vi = _index(rs, cfg)
    (_, n_full, _), _ = vi.device_arrays()
    before = gpu.memory_stats()[0]
    kept = vi.keep_targets(4, 1)
    after = gpu.memory_stats()[0]
    assert 0 < kept < n_full
    assert before - after >= 0.9 * 8 * (n_full - kept)
    assert "k_keep_copy" in ctx.kernel_times()


@pytest.mark.gpu
def test_restricted_context_refuses_full_index_calls(built):
    from flye_amd import config, gpu
    cfg = config.preset("raw")
    rs = _reads("pb_raw", seed=19, genome_len=30_000)
    ctx, vi = _index(rs, cfg)
    det = _detector(ctx, vi, cfg)
    q = np.arange(0, 2 * rs.n, 2, dtype=np.uint32)
    want = det.getSeqOverlapsBatch(q).lines()
    before = vi.export()
    assert vi.keep_targets(1, 0) == len(before.entries) and vi.shard() == (1, 0)
    after = vi.export()
    for a in ("keys", "key_off", "entries", "repetitive"):
        assert np.array_equal(getattr(before, a), getattr(after, a))
    with pytest.raises(gpu.FlyeGpuError) as e:
        vi.keep_targets(2, 2)
    assert e.value.code == -3
    vi.keep_targets(2, 1)
    with pytest.raises(gpu.FlyeGpuError) as e:
        det.getSeqOverlapsBatch(q)
    assert e.value.code == -4 and "fg_overlaps_from_hits" in str(e.value)
    with pytest.raises(gpu.FlyeGpuError) as e:
        gpu.BatchingOverlapContainer(det)
    assert e.value.code == -4
    with pytest.raises(gpu.FlyeGpuError) as e:
        vi.keep_targets(3, 0)                   # another restriction on top of this one
    assert e.value.code == -4
    vi.clear()
    assert vi.shard() == (1, 0)
    vi.build(cfg)
    assert det.getSeqOverlapsBatch(q).lines() == want


def _gloo_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    import torch.distributed as td
    from flye_amd import config, dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    td.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    for preset, kind in (("raw", "pb_raw"), ("hifi", "hifi")):
        cfg = config.preset(preset)
        rs = _reads(kind, seed=91)
        ctx, vi = _index(rs, cfg)
        vi.clear()
        st = dist.build_index_option_b(vi, cfg, rank, world, on_device=False)
        det = _detector(ctx, vi, cfg)
        res, moved = dist.overlaps_option_b(det, rank, world, on_device=False, batch_reads=64)
        ctx1, vi1 = _index(rs, cfg)
        one = _detector(ctx1, vi1, cfg).getSeqOverlapsBatch(np.arange(0, 2 * rs.n, 2, dtype=np.uint32))
        lines1 = one.lines()
        got = [l for _, r in res for l in r.lines()]
        want = [l for i in range(rank, rs.n, world) for l in lines1[int(one.query_off[i]):int(one.query_off[i + 1])]]
        assert got == want and len(want) > 0, preset
        assert st["index_entries"] == vi1.stats["index_entries"] and 0 < st["shard_entries"] < st["index_entries"]
        out[preset] = (len(want), moved)
        ctx.close(); ctx1.close()
    open(os.path.join(out_dir, f"b_gpu{rank}"), "w").write(repr(out))
    td.destroy_process_group()


@pytest.mark.gpu
def test_two_rank_option_b_on_device(built, tmp_path):
    """two processes on one GPU, collectives through gloo: build_index_option_b + overlaps_option_b; the merged
    lists equal the single-process ones"""
    import torch.multiprocessing as mp
    mp.spawn(_gloo_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r = [eval(open(tmp_path / f"b_gpu{k}").read()) for k in range(2)]
    for preset in ("raw", "hifi"):
        assert r[0][preset][1] > 0 and r[1][preset][1] > 0
