import numpy as np


def test_complement_is_involution_and_matches_definition():
    from flye_amd import gpu
    r = np.zeros(3, gpu.REC_DTYPE)
    r["cur_id"] = [0, 4, 7]; r["ext_id"] = [3, 8, 10]
    r["cur_begin"] = [10, 0, 5]; r["cur_end"] = [2000, 1500, 999]; r["cur_len"] = [3000, 1600, 1000]
    r["ext_begin"] = [7, 100, 0]; r["ext_end"] = [1900, 1700, 900]; r["ext_len"] = [2500, 1800, 901]
    c = gpu.complement(r)
    # overlap.h:118-147: begin/end swap and map x -> len - x - 1, ids to their rc
    assert list(c["cur_begin"]) == [3000 - 2000 - 1, 1600 - 1500 - 1, 0]
    assert list(c["cur_end"]) == [3000 - 10 - 1, 1599, 1000 - 5 - 1]
    assert list(c["cur_id"]) == [1, 5, 6] and list(c["ext_id"]) == [2, 9, 11]
    back = gpu.complement(c)
    for f in r.dtype.names:
        assert np.array_equal(back[f], r[f])


def test_shard_queries_partition():
    from flye_amd import dist
    n, first = 1001, 40
    ids = [dist.shard_queries(n, r, 8, first) for r in range(8)]
    allids = np.sort(np.concatenate(ids))
    assert np.array_equal(allids, first + 2 * np.arange(n))
    assert max(len(x) for x in ids) - min(len(x) for x in ids) <= 1
    assert all(np.all(dist.owner_of((x - first) // 2, 8) == r) for r, x in enumerate(ids))


def test_synth_is_deterministic(built):
    from flye_amd import synth
    a = synth.simulate(seed=9, genome_len=20000, coverage=5, kind="ont_raw")
    b = synth.simulate(seed=9, genome_len=20000, coverage=5, kind="ont_raw")
    c = synth.simulate(seed=10, genome_len=20000, coverage=5, kind="ont_raw")
    assert np.array_equal(a.words, b.words) and np.array_equal(a.length, b.length)
    assert not np.array_equal(a.length, c.length)
    sub = a.subset([0, 2])
    assert sub.n == 2 and sub.length[1] == a.length[2]


def test_bench_byte_model_and_stage_attribution():
    """bench.py's algorithmic bytes (16.25 + 44 m + 20 d B/bp): the kernels of a stage share the
    stage's bytes, k_chain_small is credited with the DP elements of the groups it processed only, and the stage
    figures add up to the whole formula."""
    import bench
    bp, m, d, ovl, d_small = 1e6, 1.5, 1.1, 0.008, 0.8
    per = {k: bench.algorithmic_bytes(k, bp, m, d, ovl, d_small) for k in
           ("k_probe", "k_fill", "k_sort_level", "k_sort_lds", "k_chain_dp", "k_chain_small", "k_group_prep")}
    assert per["k_probe"] == (0.25 + 16.0) * bp
    assert per["k_fill"] == m * 20.0 * bp
    assert per["k_sort_level"] == per["k_sort_lds"] == m * 24.0 * bp
    assert per["k_chain_dp"] == (d * 20.0 + 44.0 * ovl) * bp
    assert per["k_chain_small"] == d_small * 20.0 * bp < per["k_chain_dp"]
    assert per["k_group_prep"] == 0.0
    assert bench.algorithmic_bytes("k_chain_small", bp, m, d, ovl) == per["k_chain_dp"]     # no counter: the stage's bytes
    times = {"k_probe": (1e-3, 1), "k_fill": (1e-3, 1), "k_exscan": (1e-4, 3), "k_sort_level": (2e-3, 20), "k_sort_lds": (1e-3, 1),
             "k_chain_small": (2e-3, 1), "k_group_prep": (1e-3, 2), "k_prim_gather": (1e-4, 1), "host:shim": (5e-3, 1)}
    st = bench.stage_rooflines(times, bp, m, d, ovl, None)
    assert set(st) == {"seed_collect", "hit_sort", "chain"}
    total = sum(v["algorithmic_bytes"] for v in st.values())
    assert abs(total - (16.25 + 44.0 * m + 20.0 * d + 44.0 * ovl) * bp) <= 3
    assert st["hit_sort"]["kernels"] == ["k_sort_lds", "k_sort_level"] and abs(st["hit_sort"]["exclusive_ms"] - 3.0) < 1e-9
    assert "traffic" not in st["chain"]


def test_bench_dump_outputs_sample(tmp_path):
    """bench.py --dump-outputs: per-query counts of every query, and every field of the records and divergence
    samples of a fixed, seeded sample of the queries, exactly (integers as float64, floats bit for bit), the same
    files from run to run and within the size budget."""
    import types
    import bench
    from flye_amd import gpu
    rng = np.random.default_rng(7)
    nq = 5000
    qoff = np.concatenate([[0], np.cumsum(rng.integers(0, 40, nq))]).astype(np.uint64)
    soff = np.concatenate([[0], np.cumsum(rng.integers(0, 4, nq))]).astype(np.uint64)
    recs = np.zeros(int(qoff[-1]), gpu.REC_DTYPE)
    for f in recs.dtype.names:
        recs[f] = rng.random(len(recs)) if f == "seq_divergence" else rng.integers(0, 1 << 24, len(recs))
    res = types.SimpleNamespace(query_off=qoff, stat_off=soff, recs=recs, stats=rng.random(int(soff[-1])).astype(np.float32),
                                query_ids=np.arange(1, 2 * nq, 2, dtype=np.uint32))
    bench.dump_outputs(res, str(tmp_path / "a"))
    bench.dump_outputs(res, str(tmp_path / "b"))
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "b").iterdir())
    assert {"records_per_query.npy", "div_stats_per_query.npy", "sample_queries.npy", "div_stats.npy"} <= set(names)
    assert sum((tmp_path / "a" / n).stat().st_size for n in names) <= bench.DUMP_MAX_BYTES
    out = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    for n in names:
        assert out[n[:-4]].dtype in (np.float32, np.float64)
        assert np.array_equal(out[n[:-4]], np.load(tmp_path / "b" / n))
    assert np.array_equal(out["records_per_query"], np.diff(qoff.astype(np.int64)))
    pick = (out["sample_queries"].astype(np.int64) - 1) // 2
    assert len(pick) == bench.DUMP_QUERIES and np.all(np.diff(pick) > 0)
    ri = np.concatenate([np.arange(qoff[i], qoff[i + 1]) for i in pick]).astype(np.int64)
    for f in recs.dtype.names:
        assert np.array_equal(out["recs_" + f], recs[f][ri])
    assert out["recs_seq_divergence"].dtype == np.float32
    si = np.concatenate([np.arange(soff[i], soff[i + 1]) for i in pick]).astype(np.int64)
    assert np.array_equal(out["div_stats"], res.stats[si])


def test_bench_options():
    """bench.py has --steps, --warmup, --dump-outputs and --full (the legs beyond the headline figure), and refuses
    a run of no timed step before it touches a device."""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = subprocess.run([sys.executable, os.path.join(here, "bench.py"), "--help"], capture_output=True, text=True, check=True)
    for opt in ("--steps", "--warmup", "--dump-outputs", "--full"):
        assert opt in h.stdout
    r = subprocess.run([sys.executable, os.path.join(here, "bench.py"), "--steps", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and "--steps" in r.stderr
