"""The device group (fg_group_*, gpu.Group): option B driven from one process through the C ABI.  W members on device
0; the reference is always the single-context library -- fg_build_index_* / fg_index_keep_targets for the shards,
fg_overlaps on the full index for the overlap stage -- which the rest of the suite pins to the oracle."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PRESETS = [("raw", "pb_raw"), ("hifi", "hifi")]
STAT_FIELDS = ("total_kmers", "selected_kmers", "index_entries", "repetitive_kmers", "repetitive_frequency",
               "mean_frequency", "sample_rate")


@functools.lru_cache(maxsize=None)
def _reads(kind, seed=41, genome_len=60_000, coverage=20):
    from flye_amd import synth
    return synth.simulate(seed=seed, genome_len=genome_len, coverage=coverage, kind=kind, n_repeat_families=4,
                          n_tandems=20, n_homopolymers=8).filter_min_len(1000)


def _rate(cfg):
    return float(int(cfg["assemble_kmer_sample"]))


def _index(rs, cfg, first_id=0, qrs=None, q_first=None):
    from flye_amd import gpu
    ctx = gpu.Context(17, 0)
    ctx.set_reads(rs, first_id)
    if qrs is not None:
        ctx.set_queries(qrs, q_first)
    vi = gpu.VertexIndex(ctx, _rate(cfg))
    vi.build(cfg)
    return ctx, vi


@functools.lru_cache(maxsize=None)
def _single(preset, kind, first_id=0, seed=41, q_cov=0):
    """the reference: one context with the full index (shared, never modified)"""
    from flye_amd import config
    cfg = config.preset(preset)
    rs = _reads(kind, seed)
    qrs = _reads(kind, seed, coverage=q_cov) if q_cov else None
    ctx, vi = _index(rs, cfg, first_id, qrs, first_id + 2 * rs.n if q_cov else None)
    return cfg, rs, qrs, ctx, vi


@functools.lru_cache(maxsize=None)
def _group(world, preset, kind, first_id=0, seed=41, q_cov=0):
    """a group of `world` members on device 0 with the index built (shared between the overlap tests)"""
    from flye_amd import config, gpu
    cfg = config.preset(preset)
    rs = _reads(kind, seed)
    g = gpu.Group([0] * world, 17)
    g.set_reads(rs, first_id)
    if q_cov:
        g.set_queries(_reads(kind, seed, coverage=q_cov), first_id + 2 * rs.n)
    g.build(cfg)
    return g


def _params(cfg, **flags):
    from flye_amd import gpu
    det = gpu.OverlapDetector.for_assemble(None, None, cfg)
    det.p.max_divergence = 0.3
    for k, v in flags.items():
        setattr(det.p, k, v)
    return det.p


def _full_detector(ctx, vi, cfg, p):
    from flye_amd import gpu
    det = gpu.OverlapDetector.for_assemble(ctx, vi, cfg)
    det.p = p
    return det


def _same(got, want):
    assert got.lines() == want.lines()
    assert len(want.recs) > 0
    assert np.array_equal(got.recs, want.recs)
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


def _has_tied_keys(det, q):
    """tied (extId, curPos) sort keys inside a query: only then does the emission order the receiver restores decide
    what the unstable hit sort leaves"""
    from flye_amd import gpu
    counts, ptr, n = det.probe_hits(q)
    h = gpu.seed_hits_to_host(ptr, n)
    keys = np.stack([np.repeat(np.arange(len(counts)), counts.astype(np.int64)), h["ext_id"].astype(np.int64),
                     h["cur_pos"].astype(np.int64)], axis=1)
    return len(np.unique(keys, axis=0)) < len(keys)


def _batches_without_an_owner(q, base, world, batch):
    n = 0
    for b0 in range(0, len(q), batch):
        owners = ((q[b0:b0 + batch].astype(np.int64) - base) >> 1) % world
        n += len(np.unique(owners)) < world
    return n


def _mixed_queries(n_reads, base, world, batch, rng):
    """one batch of reads of owner 0 alone, then a shuffled subset of both strands: not sorted, not grouped by owner"""
    lone = base + 2 * np.arange(0, n_reads, world)[:batch]
    rest = base + rng.permutation(2 * n_reads)[:max(3 * batch, (2 * n_reads * 2) // 3)]
    return np.concatenate([lone, rest]).astype(np.uint32)


# ---- 0. CPU: the key ranges are the Python path's --------------------------------------------------------------------------
def test_group_bin_cuts_equal_balanced_bin_ranges(built):
    from flye_amd import dist, gpu
    L = gpu.load_library()
    rng = np.random.default_rng(2)
    hists = [np.zeros(4096, np.uint64), np.ones(4096, np.uint64), rng.integers(0, 1 << 40, 4096).astype(np.uint64),
             (rng.integers(0, 50, 4096) * (rng.random(4096) < 0.02)).astype(np.uint64),
             np.r_[np.zeros(4095), [7]].astype(np.uint64), np.r_[[1 << 52], np.zeros(4095)].astype(np.uint64),
             rng.integers(0, 3, 4096).astype(np.uint64)]
    for h in hists:
        for world in (1, 2, 3, 7, 8, 127, 128):
            cuts = np.zeros(world + 1, np.uint32)
            assert L.fg_debug_group_bin_cuts(h.ctypes.data, world, cuts.ctypes.data) == 0
            want = dist.balanced_bin_ranges(h, world)
            assert [(int(cuts[r]), int(cuts[r + 1])) for r in range(world)] == want, world
    assert L.fg_debug_group_bin_cuts(hists[0].ctypes.data, 0, None) == -3
    assert L.fg_debug_group_bin_cuts(hists[0].ctypes.data, 129, hists[0].ctypes.data) == -3


# ---- 1. the index ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("first_id", [0, 1000])
@pytest.mark.parametrize("preset,kind", PRESETS)
@pytest.mark.parametrize("world", [2, 3])
def test_group_build_gives_the_keep_targets_shards(built, monkeypatch, world, preset, kind, first_id):
    from flye_amd import gpu
    cfg, rs, _, ctx, vi = _single(preset, kind, first_id)
    # several selection batches, several staging pieces per transfer (about 1.2 M k-mer positions in all)
    monkeypatch.setenv("FG_INDEX_BATCH_KMERS", "250000")
    monkeypatch.setenv("FG_GROUP_STAGE_BYTES", "32768")
    g = gpu.Group([0] * world, 17)
    g.set_reads(rs, first_id)
    held = gpu.memory_stats(reset_peak=True)[0]
    st = g.build(cfg)
    info = g.build_info()
    now, peak = gpu.memory_stats()
    print(f"\ngroup build W={world} {preset}: peak {peak - held} B, resident {now - held} B above what the process held "
          f"with the reads set (one GPU, W contexts; the reference context included in neither), {info}")
    monkeypatch.delenv("FG_INDEX_BATCH_KMERS")
    monkeypatch.delenv("FG_GROUP_STAGE_BYTES")
    assert len(g) == world
    for f in STAT_FIELDS:
        a, b = st[f], vi.stats[f]
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), (f, a, b)
    assert np.float32(g.getSampleRate()).tobytes() == np.float32(vi.getSampleRate()).tobytes()
    if preset == "raw":
        assert info["selection_batches"] >= 3 and info["stage_pieces_max"] >= 3, info
        # more than one piece per (batch, member, source) on average, whatever the last batch holds
        assert info["stage_pieces"] > info["selection_batches"] * world * (world - 1) and info["freq_bytes"] > 0
    else:
        assert info["selection_batches"] == 0 and info["stage_pieces"] == 0
    assert info["scatter_bytes"] > 0
    # the frequency sum collects its own launches: what a member reports now is its last step call, the scatter's end
    for r in range(world):
        names = g.member(r).kernel_times()
        assert "k_scatter_scan" in names and "k_freq_accumulate" not in names, (r, sorted(names))
    total = 0
    for r in range(world):
        c1, v1 = _index(rs, cfg, first_id)
        kept = v1.keep_targets(world, r)
        want = v1.export()
        mv = gpu.VertexIndex(g.member(r), _rate(cfg))
        assert mv.shard() == (world, r)
        got = mv.export()
        for a in ("keys", "key_off", "entries", "repetitive"):
            assert np.array_equal(getattr(got, a), getattr(want, a)), (r, a)
        assert len(got.entries) == kept
        total += kept
        c1.close()
    assert total == st["index_entries"] > 0
    g.close()


# ---- 2. + 3. the overlap stage and its accounting ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("preset,kind", PRESETS)
@pytest.mark.parametrize("world,two_pass", [pytest.param(2, False, id="2"), pytest.param(3, False, id="3"),
                                            pytest.param(2, True, id="2-two_pass")])
def test_group_overlaps_assemble_flags_and_accounting(built, monkeypatch, world, two_pass, preset, kind):
    """every forward read, then a mixed list; >= 3 batches, one of them without a query for some owner; moved bytes
    and hit totals against the members' own fg_probe_hits.  two_pass: the members restore the emission order of the
    received hits with two stable sorts (FG_RECV_TWO_PASS=1), the form of read sets far beyond test size."""
    from flye_amd import gpu
    if two_pass:
        monkeypatch.setenv("FG_RECV_TWO_PASS", "1")
    else:
        monkeypatch.delenv("FG_RECV_TWO_PASS", raising=False)
    cfg, rs, _, ctx, vi = _single(preset, kind)
    g = _group(world, preset, kind)
    p = _params(cfg)
    full = _full_detector(ctx, vi, cfg, p)
    batch = 16
    monkeypatch.setenv("FG_GROUP_BATCH_READS", str(batch))
    q = np.arange(0, 2 * rs.n, 2, dtype=np.uint32)
    assert len(q) >= 3 * batch
    assert _has_tied_keys(full, q)
    want = full.getSeqOverlapsBatch(q)
    _same(g.overlaps(p, q), want)
    st = g.stats()
    assert st["hits_total"] == want.seed_hits
    moved = 0
    for s in range(world):
        ms = gpu.OverlapDetector.for_assemble(g.member(s), None, cfg)
        for b0 in range(0, len(q), batch):
            qb = q[b0:b0 + batch]
            owner = (qb.astype(np.int64) >> 1) % world
            grouped = qb[np.argsort(owner, kind="stable")]
            counts, _, n = ms.probe_hits(grouped)
            assert int(counts.sum()) == n
            moved += 12 * int(counts[np.sort(owner, kind="stable") != s].sum())
    assert st["hits_moved_bytes"] == moved > 0
    assert 0 < st["peer_copies"] <= world * world * ((len(q) + batch - 1) // batch) and st["exchange_seconds"] > 0
    print(f"\ngroup W={world} {preset}: {len(q)} queries, hits {st['hits_total']}, moved {st['hits_moved_bytes']} B in "
          f"{st['peer_copies']} copies, exchange {st['exchange_seconds'] * 1e3:.2f} ms (one GPU, W contexts)")
    # a list that is neither sorted nor grouped, both strands, with a batch that leaves an owner idle
    q2 = _mixed_queries(rs.n, 0, world, batch, np.random.default_rng(world))
    assert _batches_without_an_owner(q2, 0, world, batch) >= 1 and (q2 & 1).any() and len(q2) >= 3 * batch
    _same(g.overlaps(p, q2), full.getSeqOverlapsBatch(q2))
    monkeypatch.setenv("FG_GROUP_BATCH_READS", "4096")          # one batch gives the same
    _same(g.overlaps(p, q2), full.getSeqOverlapsBatch(q2))


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_group_overlaps_repeat_stage_flags_rc_ids_first_id(built, monkeypatch, world):
    """only_max_ext = 0, keep_alignment, partition_bad_mappings, nucl_alignment; max_overlaps > 0; reverse-complement
    ids in a shuffled subset; first_seq_id != 0"""
    first = 1000
    cfg, rs, _, ctx, vi = _single("raw", "pb_raw", first)
    g = _group(world, "raw", "pb_raw", first)
    batch = 8
    monkeypatch.setenv("FG_GROUP_BATCH_READS", str(batch))
    rng = np.random.default_rng(7 + world)
    q = _mixed_queries(rs.n, first, world, batch, rng)[:8 * batch]
    assert _batches_without_an_owner(q, first, world, batch) >= 1 and (q & 1).any()
    flags = dict(only_max_ext=0, keep_alignment=1)
    p = _params(cfg, partition_bad_mappings=1, nucl_alignment=1, **flags)
    full = _full_detector(ctx, vi, cfg, p)
    assert _has_tied_keys(full, q)
    want = full.getSeqOverlapsBatch(q)
    assert want.needs_trim is not None and len(want.matches) > 0 and (want.recs["edit_distance"] >= 0).any()
    _same(g.overlaps(p, q), want)
    # max_overlaps > 0 (not with partition_bad_mappings: refused as fg_overlaps refuses it)
    from flye_amd import gpu
    with pytest.raises(gpu.FlyeGpuError) as e:
        g.overlaps(p, q, maxOverlaps=3)
    assert e.value.code == -7
    p_cut = _params(cfg, **flags)
    full_cut = _full_detector(ctx, vi, cfg, p_cut)
    _same(g.overlaps(p_cut, q, maxOverlaps=3), full_cut.getSeqOverlapsBatch(q, maxOverlaps=3))
    _same(g.overlaps(p_cut, q, forceLocal=True), full_cut.getSeqOverlapsBatch(q, forceLocal=True))


# the hit form the members' receivers write: 32-bit keys at this size, and with the switches the packed records and the
# 64-bit keys beside values of read sets that need more than 32 key bits
KEY_FORMS = {"key32": {}, "key64": {"FG_FORCE_KEY64": "1"}, "key64_unpacked": {"FG_FORCE_KEY64": "1", "FG_PACKED_KEYS": "0"}}


@pytest.mark.gpu
@pytest.mark.parametrize("world,key_form", [pytest.param(2, "key32", id="2"), pytest.param(3, "key32", id="3"),
                                            pytest.param(2, "key64", id="2-key64"),
                                            pytest.param(2, "key64_unpacked", id="2-key64_unpacked")])
def test_group_overlaps_separate_query_container(built, monkeypatch, world, key_form):
    """queries in a container of their own (fg_group_set_queries: the ReadAligner shape); with two members also in the
    64-bit hit forms, where the group and the full index must both give what the full index gives in the 32-bit form"""
    for sw in ("FG_FORCE_KEY64", "FG_PACKED_KEYS"):
        monkeypatch.delenv(sw, raising=False)
    cfg, rs, qrs, ctx, vi = _single("raw", "pb_raw", 0, 12, 6)
    g = _group(world, "raw", "pb_raw", 0, 12, 6)
    q_first = 2 * rs.n
    monkeypatch.setenv("FG_GROUP_BATCH_READS", "16")
    q = (q_first + np.random.default_rng(5).permutation(2 * qrs.n)).astype(np.uint32)         # both strands, shuffled
    assert len(q) >= 48
    p = _params(cfg, only_max_ext=0)
    full = _full_detector(ctx, vi, cfg, p)
    assert _has_tied_keys(full, q)
    want = full.getSeqOverlapsBatch(q)
    for sw, value in KEY_FORMS[key_form].items():
        monkeypatch.setenv(sw, value)
    _same(full.getSeqOverlapsBatch(q), want)
    _same(g.overlaps(p, q), want)
    from flye_amd import gpu
    with pytest.raises(gpu.FlyeGpuError) as e:
        g.overlaps(p, np.array([0], np.uint32))            # an id of the indexed container is no query id here
    assert e.value.code == -3


# ---- 4. the one new kernel ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_freq_accumulate_kernel(built):
    from flye_amd import gpu
    ctx = gpu.Context(17, 0)
    rng = np.random.default_rng(11)

    def aligned(n, off=0):
        """n uint32 whose first element sits `off` elements behind a 16-byte boundary"""
        raw = np.zeros(n + 8, np.uint32)
        lead = ((-raw.ctypes.data) % 16) // 4 + off
        v = raw[lead:lead + n]
        assert n == 0 or v.ctypes.data % 16 == 4 * off
        return v

    for n in (0, 1, 3, 4, 5, 63, 64, 65, 4099):
        for d_off, s_off in ((0, 0), (0, 1)) + (((1, 1), (3, 2)) if n == 4099 else ()):
            dst, src = aligned(n, d_off), aligned(n, s_off)
            dst[:] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
            src[:] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
            if n:
                dst[-1], src[-1] = 0xFFFFFFFF, 2                       # wraps
                dst[0], src[0] = 0xFFFFFFF0, 0x20
            want = (dst.astype(np.uint64) + src.astype(np.uint64)).astype(np.uint32)
            if n > 1:
                assert (dst.astype(np.uint64) + src.astype(np.uint64) >= 1 << 32).any()
            keep = src.copy()
            ctx.debug_freq_accumulate(dst, src)
            assert np.array_equal(dst, want), (n, d_off, s_off)
            assert np.array_equal(src, keep)
            if n:
                assert ctx.kernel_times()["k_freq_accumulate"][1] == 1
    ctx.close()


# ---- 5. degenerate and error cases -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("preset,kind", PRESETS)
def test_group_of_one_is_the_plain_context(built, preset, kind):
    from flye_amd import gpu
    cfg, rs, _, ctx, vi = _single(preset, kind)
    g = gpu.Group([0], 17)
    g.set_reads(rs, 0)
    st = g.build(cfg)
    for f in STAT_FIELDS:
        assert np.asarray(st[f]).tobytes() == np.asarray(vi.stats[f]).tobytes(), f
    mv = gpu.VertexIndex(g.member(0), _rate(cfg))
    assert mv.shard() == (1, 0)
    got, want = mv.export(), vi.export()
    for a in ("keys", "key_off", "entries", "repetitive"):
        assert np.array_equal(getattr(got, a), getattr(want, a)), a
    p = _params(cfg)
    q = np.arange(0, 2 * rs.n, 2, dtype=np.uint32)
    want_ov = _full_detector(ctx, vi, cfg, p).getSeqOverlapsBatch(q)
    _same(g.overlaps(p, q), want_ov)
    s = g.stats()
    assert s["hits_moved_bytes"] == 0 and s["peer_copies"] == 0 and s["hits_total"] == want_ov.seed_hits
    assert g.build_info()["stage_pieces"] == 0
    g.close()


@pytest.mark.gpu
def test_group_argument_and_state_errors_and_memory(built):
    import gc
    from flye_amd import config, gpu
    L = gpu.load_library()
    h = C.c_void_p()
    assert L.fg_group_create(C.byref(h), (C.c_int * 1)(0), 0, 17) == -3 and not h.value
    assert L.fg_group_create(C.byref(h), (C.c_int * 129)(), 129, 17) == -3 and not h.value
    assert L.fg_group_create(C.byref(h), None, 2, 17) == -3
    assert L.fg_group_create(C.byref(h), (C.c_int * 2)(0, 0), 2, 33) == -6
    cfg, rs, _, ctx, vi = _single("raw", "pb_raw")
    p = _params(cfg)
    q = np.arange(0, 2 * rs.n, 2, dtype=np.uint32)[:24]
    want = _full_detector(ctx, vi, cfg, p).getSeqOverlapsBatch(q)
    gc.collect()
    before = gpu.memory_stats()[0]
    g = gpu.Group([0, 0], 17)
    g.set_reads(rs, 0)
    assert gpu.memory_stats()[0] > before
    with pytest.raises(gpu.FlyeGpuError) as e:
        g.overlaps(p, q)                                    # before a build
    assert e.value.code == -4
    g.build(cfg)
    _same(g.overlaps(p, q), want)
    with pytest.raises(gpu.FlyeGpuError) as e:
        g.overlaps(p, np.array([2 * rs.n], np.uint32))      # no such record
    assert e.value.code == -3
    g.clear()
    assert gpu.VertexIndex(g.member(0), 1.0).shard() == (1, 0)
    with pytest.raises(gpu.FlyeGpuError) as e:
        g.overlaps(p, q)
    assert e.value.code == -4
    g.build(cfg)                                             # a second build works
    got = g.overlaps(p, q)
    _same(got, want)
    with pytest.raises(gpu.FlyeGpuError) as e:
        gpu.BatchingOverlapContainer(gpu.OverlapDetector.for_assemble(g.member(1), None, cfg))
    assert e.value.code == -4                                # a member is a restricted context: no scheduler over it
    with pytest.raises(gpu.FlyeGpuError):
        g.member(2)
    # an error on a member ends the call with its code, names the member, and leaves no index behind
    rc = L.fg_group_build_index_minimizers(g.h, 1, 0, 100.0, C.byref(gpu.IndexStats()))
    text = L.fg_group_last_error(g.h).decode()
    assert rc == -3 and text.startswith("member 0 (device 0): ") and "wrong minimizer length" in text
    with pytest.raises(gpu.FlyeGpuError) as e:
        g.overlaps(p, q)
    assert e.value.code == -4
    del got
    g.close()
    gc.collect()
    assert gpu.memory_stats()[0] == before


# ---- 6. the C consumer ---------------------------------------------------------------------------------------------------
def _build_demo(tmp_path, name):
    exe = str(tmp_path / name)
    lib = os.path.join(ROOT, "flye_amd", "lib")
    subprocess.run(["cc", "-std=c99", "-pthread", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "examples", name + ".c"), "-L" + lib, "-lflyegpu", "-Wl,-rpath," + lib, "-o", exe],
                   check=True)
    return exe


def test_group_demo_is_plain_c_and_links(built, tmp_path):
    """examples/c_group_demo.c compiles as C99 against include/ and links; without a GPU it reports the error of
    fg_group_create (exit status 2)"""
    import torch
    exe = _build_demo(tmp_path, "c_group_demo")
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 2 and "no usable HIP device" in r.stdout


@pytest.mark.gpu
def test_group_demo_runs_with_two_members(built, tmp_path):
    import re
    one = subprocess.run([_build_demo(tmp_path, "c_abi_demo")], capture_output=True, text=True, timeout=300)
    two = subprocess.run([_build_demo(tmp_path, "c_group_demo")], capture_output=True, text=True, timeout=300)
    assert one.returncode == 0 and two.returncode == 0, one.stdout + two.stdout + two.stderr
    pat = r"(\d+) overlaps for 60 reads, (\d+) seed hits"
    a, b = re.search(pat, one.stdout), re.search(pat, two.stdout)
    assert a and b and a.groups() == b.groups() and int(a.group(1)) > 0, two.stdout
    assert "group of 2 members" in two.stdout
