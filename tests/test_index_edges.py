"""The index build (flye_amd/csrc/fg_index.hip) at its threshold, tandem, window and list edges: the crafted read sets
of tests/index_craft.py.

Without a GPU: what each case is FOR is asserted with the numpy restatements of index_craft (never the yardstick for
the device); the craft module reproduces the stored reads; the oracle reproduces every digest the unmodified
reference left in tests/golden/index_edges.json, and runs against the live reference where it is built.

With one: every (case, parameter set) built on the device equals the oracle's index, statistics and sample-rate bits
and the stored reference digest -- in one call, with either counter form, with every read a selection batch of its
own, with the sort in 23 slices, as three key-range pieces, with the selection in steps over two counter ranges, and
as the two shards of a device group; the probe-skip bits after every solid build; overlaps over an index with empty
lists and over the sparse w = 64 sketch.

Which sets rest on what: every set with min_freq 2 below k = 17 and every minimizer set has a reference digest.
``tandem17`` (the reference's flat counter takes 90 s and 8 GiB at k = 17; the golden vectors of
tests/golden/cases.json pin the oracle there) and min_freq 1 and 3 (the reference's dumper fixes 2) rest on the
oracle alone.
"""
import functools
import json
import os

import numpy as np
import pytest

import index_craft as ic
from helpers import GOLDEN, check_index_stats, check_overlaps_equal, index_digest

STAT_FIELDS = ("total_kmers", "selected_kmers", "index_entries", "repetitive_kmers", "repetitive_frequency")
ALL_SETS = ic.all_sets()
SOLID_KERNELS = ("k_count", "k_freq", "k_threshold", "k_mark", "k_accept", "k_pack_bits")


@functools.lru_cache(maxsize=None)
def _stored():
    with open(os.path.join(GOLDEN, "index_edges.json")) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def _counts(name):
    c = ic.case(name)
    return ic.Counts(c.reads, c.k)


@functools.lru_cache(maxsize=None)
def _world(name, pname):
    """the oracle's index and statistics of one (case, parameter set): shared, never modified"""
    from oracle import oracle as O
    c, p = ic.case(name), ic.pset(name, pname)
    o = O.Oracle(c.k, threads=4)
    o.set_reads(c.reads)
    st = ic.oracle_build(o, p)
    return dict(case=c, p=p, o=o, st=st, index=o.export_index(), gold=_stored()[name]["sets"][pname])


def _first(name, **want):
    """name of the case's parameter set with the given values"""
    return next(ic.pset_name(p) for p in ic.PSETS[name] if all(p.get(k) == v for k, v in want.items()))


def _lists_of(ix):
    return np.diff(ix.key_off.astype(np.int64))


def _has(keys, kmers):
    keys = np.asarray(keys, np.uint64)
    i = np.minimum(np.searchsorted(keys, kmers), max(len(keys) - 1, 0))
    return (keys[i] == kmers) if len(keys) else np.zeros(len(kmers), bool)


def _inner(motif, k):
    """canonical k-mers of a motif (every one, they all lie inside a read)"""
    return np.unique(ic.canon_of(motif, k)[0])


# ---- what the cases are for (CPU) ----------------------------------------------------------------------------------------
def test_threshold_case_shows_its_edges(built):
    c, cnt = ic.case("threshold"), _counts("threshold")
    p = c.psets[0]
    th = ic.thresholds(cnt, p["rate"])
    values = {t for _, t in th if t is not None}
    assert {2046, 2047, 2048} <= values and max(values) >= 4096          # around the last histogram bin, far above it
    assert [t for _, t in th[:5]] == [2048, 5000, 2046, 2047, 2048]
    f0, f1 = cnt.freq[cnt.of(0)], cnt.freq[cnt.of(1)]
    assert (f0 == 2047).sum() == 18 and (f1 == 2048).sum() == 18         # one copy just below the threshold: dropped
    for r, above in ((2, 2047), (3, 2048), (4, 5000)):                     # ties at the threshold, a family above it
        m, t = th[r]
        f = cnt.freq[cnt.of(r)]
        assert (f > t).sum() == (f == above).sum() == 90 and (f >= t).sum() == 180 > m + 1
    assert sorted(cnt.nk[5:8].tolist()) == [255, 256, 257] and all(t == 5000 for _, t in th[5:8])
    s0 = c.marks["first_short"]
    assert cnt.nk[s0:s0 + 6].tolist() == [2, 2, 2, 1, 0, 0] and [len(x) - c.k for x in c.seqs[s0:s0 + 6]] == [2, 2, 2, 1, 0, -1]
    assert [th[r][0] for r in range(s0, s0 + 4)] == [0, 0, 0, 0]          # maxKmers == 0: the most frequent k-mer only
    a, b = (int(x) for x in ic.canon_of(c.marks["short"], c.k)[0])
    assert (cnt.freq_of(a), cnt.freq_of(b)) == (4, 2)
    ix = _world("threshold", ic.pset_name(p))["index"]
    assert _has(ix.keys, np.array([a, b], np.uint64)).tolist() == [True, False]  # b: frequent enough, below ITS reads' thresholds
    assert int(_lists_of(ix)[np.searchsorted(ix.keys, np.uint64(a))]) == 4
    # the motif k-mers carry exactly the planned counts, and no read repeats one more than tandemFreq times
    for m, copies in zip(c.marks["motifs"], ic.THRESHOLD_COPIES):
        assert {cnt.freq_of(x) for x in _inner(m, c.k)} == {copies}
    assert cnt.local.max() == p["tandem"] == 10


@pytest.mark.parametrize("name", ["tandem13", "tandem17"])
def test_tandem_case_shows_its_edges(built, name):
    """k = 17 rests on the oracle alone: the reference's flat counter takes 90 s and 8 GiB there, and the golden vectors
    of tests/golden/cases.json pin the oracle at 17."""
    c, cnt = ic.case(name), _counts(name)
    k, mo = c.k, c.marks["motifs"]
    on, off = (_world(name, ic.pset_name(p)) for p in c.psets)
    assert (on["p"]["tandem"], off["p"]["tandem"]) == (10, 0)

    def local_in(r, motif):
        km = _inner(motif, k)
        sel = np.isin(cnt.canon[cnt.of(r)], km)
        return set(cnt.local[cnt.of(r)][sel].tolist()), set(cnt.freq[cnt.of(r)][sel].tolist())
    assert local_in(0, mo["a"]) == ({10}, {21}) and local_in(1, mo["a"]) == ({11}, {21})       # tandemFreq and + 1
    assert local_in(2, mo["b"]) == ({11}, {21}) and local_in(3, mo["b"]) == ({10}, {21})
    # ... where 11 is 6 forward + 5 reverse-complement copies: only the canonical key merges them
    _, fw, rv = ic.canon_of(c.seqs[2], k)
    _, mfw, mrv = ic.canon_of(mo["b"], k)
    assert int((fw[:-1] == mfw[0]).sum()) == 6 and int((fw[:-1] == mrv[0]).sum()) == 5
    assert local_in(4, mo["c"]) == ({11}, {11})                                                 # global == local
    assert local_in(5, mo["d"]) == ({11}, {14})
    assert all(local_in(r, mo["d"]) == ({1}, {14}) for r in (6, 7, 8))
    # the two oracle indexes differ on exactly the k-mers the restatement calls tandem
    p = on["p"]
    sel = ic.yielded(cnt, dict(p, tandem=0)) & (cnt.freq >= p["min_freq"])
    tandem = np.unique(cnt.canon[sel & (cnt.local > p["tandem"])])
    assert sorted(tandem.tolist()) == sorted(np.concatenate([_inner(mo[x], k) for x in "abcd"]).tolist())
    a, b = ic.key_lists(on["index"]), ic.key_lists(off["index"])
    assert sorted(x for x in set(a) | set(b) if a.get(x) != b.get(x)) == sorted(tandem.tolist())
    assert not len(on["index"].repetitive) and not len(off["index"].repetitive)
    assert not _has(on["index"].keys, _inner(mo["c"], k)).any() and _has(off["index"].keys, _inner(mo["c"], k)).all()
    for x in _inner(mo["d"], k).tolist():                   # tandem in read 5, kept in the three others
        assert [e >> 33 for e in a[x]] == [6, 7, 8] and len(b[x]) == 14
    for x in _inner(mo["a"], k).tolist():
        assert {e >> 33 for e in a[x]} == {0} and len(a[x]) == 10 and len(b[x]) == 21


def test_lists_case_shows_its_edges(built):
    c, cnt = ic.case("lists"), _counts("lists")
    k, mo = c.k, c.marks["motifs"]
    w = {r: _world("lists", _first("lists", repeat=r, min_freq=2)) for r in ic.LISTS_RATES + (ic.LISTS_FOURTH_RATE,)}
    hidden, big = _inner(mo["hidden"], k), _inner(mo["big"], k)
    assert {cnt.freq_of(x) for x in hidden} == {303} and {cnt.freq_of(x) for x in big} == {2700}
    assert not (_lists_of(w[100.0]["index"]) == 0).any() and not len(w[100.0]["index"].repetitive)
    for r in (5.0, 2.0, ic.LISTS_FOURTH_RATE):
        ix, rep = w[r]["index"], w[r]["st"]["repetitive_frequency"]
        empty = ix.keys[_lists_of(ix) == 0]
        assert len(empty) and len(ix.repetitive)
        # capacity 3 <= _repetitiveFrequency < frequency 303: in the index, without entries (vertex_index.cpp:73-74)
        assert 3 <= rep < 303 and _has(empty, hidden).all() and _has(ix.repetitive, big).all()
        keys, caps = ic.capacities(cnt, w[r]["p"])
        assert ic.repetitive_frequency(caps, 2, r) == rep
        assert sorted(keys[caps > rep].tolist()) == sorted(ix.repetitive.tolist())
        assert sorted(keys[caps <= rep].tolist()) == sorted(ix.keys.tolist())
    assert (w[5.0]["st"]["repetitive_frequency"], w[2.0]["st"]["repetitive_frequency"]) == (178, 71)
    # the fourth rate puts _repetitiveFrequency between two capacities that occur
    rep = w[ic.LISTS_FOURTH_RATE]["st"]["repetitive_frequency"]
    assert rep == 3 and (caps == rep).any() and (caps == rep + 1).any()
    # min_freq: frequency 1 is selected by a threshold of 1 and dropped; exactly 2 and exactly 3 against 1, 2, 3
    sel = ic.yielded(cnt, w[5.0]["p"])
    once = np.unique(cnt.canon[sel & (cnt.freq == 1)])
    pair, triple = _inner(mo["pair"], k), _inner(mo["triple"], k)
    assert len(once) > 1000 and {cnt.freq_of(x) for x in pair} == {2} and {cnt.freq_of(x) for x in triple} == {3}
    for mf, want in ((1, (True, True, True)), (2, (False, True, True)), (3, (False, False, True))):
        ix = _world("lists", _first("lists", repeat=5.0, min_freq=mf))["index"]
        got = (_has(ix.keys, once), _has(ix.keys, pair), _has(ix.keys, triple))
        assert tuple(bool(g.all()) for g in got) == want and tuple(bool(g.any()) for g in got) == want, mf
        if mf <= 2:
            assert all(len(ic.key_lists(ix)[int(x)]) == 2 for x in pair)


@pytest.mark.parametrize("name", ["windows13", "windows12"])
def test_windows_case_shows_its_edges(built, name):
    c, cnt = ic.case(name), _counts(name)
    k = c.k
    hashes = [ic.kmer_hash(x) for x in cnt.per_read]
    for w in ic.WINDOWS:
        wd = _world(name, _first(name, mode="min", window=w))
        accepted, entries = ic.sketch_entries(cnt, w, 100.0)
        assert entries == wd["st"]["index_entries"] == len(wd["index"].entries)      # this pins the restated sketch
        assert accepted >= entries
        if w > 1:
            assert any(0 < n < w for n in cnt.nk)                                     # a read shorter than k + w
            assert any(ic.equal_hash_in_window(h, w) for h in hashes)                # the tie rules decide
            assert max(ic.longest_gap(ic.sync_points(h, w)) for h in hashes if len(h)) > 512
    assert cnt.nk[:4].tolist() == [0, 0, 1, 2]
    # periods below the window: at most p distinct hashes (a k-mer and its reverse complement share one), each again p
    # positions later
    for h, period in zip(hashes[15:22], (1, 2, 3, 5, 7, 20, 70)):
        assert 1 <= len(np.unique(h[150:1400])) <= period and (h[150:1400 - period] == h[150 + period:1400]).all()
    own_rc = [bool((f == r).any()) for _, f, r in (ic.canon_of(s, k) for s in c.seqs if len(s) >= k)]
    assert any(own_rc) == (k % 2 == 0)                                                # ACGTACGTACGT
    # the solid sets on these reads: thresholds in the overflow bin (homopolymers), tandem k-mers at tandemFreq 3
    th = {t for _, t in ic.thresholds(cnt, 0.75) if t is not None}
    assert max(th) > 2047 and 1 in th
    assert (cnt.local > 3).any()


# ---- the stored digests ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ic.CASE_NAMES)
def test_craft_reproduces_the_stored_reads(built, name):
    c, g = ic.case(name), _stored()[name]
    assert (c.reads.n, int(c.reads.total_bases), ic.reads_sha256(c.reads)) == (g["n_reads"], g["total_bases"], g["reads_sha256"])
    assert sorted(g["sets"]) == sorted(ic.pset_name(p) for p in c.psets)


@pytest.mark.parametrize("name,pname", ALL_SETS)
def test_oracle_reproduces_the_reference_digest(built, name, pname):
    w = _world(name, pname)
    assert bool(w["gold"].get("oracle_only")) == (not ic.has_reference(w["p"]))
    if ic.has_reference(w["p"]):
        check_index_stats(w["st"], w["gold"])
        assert index_digest(w["index"]) == w["gold"]["sha256"]
    else:
        assert w["st"]["index_entries"] == len(w["index"].entries) > 0


LIVE = [("threshold", dict(repeat=1.5)), ("tandem13", dict(tandem=10)), ("lists", dict(repeat=ic.LISTS_FOURTH_RATE)),
        ("windows13", dict(mode="min", window=64)), ("windows12", dict(mode="solid", rate=0.1))]


@pytest.mark.parametrize("name,want", LIVE, ids=[n for n, _ in LIVE])
def test_oracle_equals_live_reference(built, tmp_path, name, want):
    from oracle import oracle as O
    if not O.have_ref():
        pytest.skip("reference build not available")
    w = _world(name, _first(name, **want))
    fa, out = str(tmp_path / "r.fasta"), str(tmp_path / "i.txt")
    w["case"].reads.write_fasta(fa)
    O.run_ref(fa, params_string=ic.ref_params(w["p"]), threads=4, index_out=out, query_limit=1)
    hdr, refidx = O.parse_ref_index(out, w["case"].reads)
    assert w["index"].same_as(refidx)
    assert np.float32(w["st"]["sample_rate"]).view(np.uint32) == int(hdr["sampleRateBits"], 16)
    assert w["st"]["repetitive_frequency"] == int(hdr["repFreq"])


# ---- the device ---------------------------------------------------------------------------------------------------------------
def _context(w):
    from flye_amd import gpu
    ctx = gpu.Context(w["case"].k, 0)
    ctx.set_reads(w["case"].reads)
    return ctx, gpu.VertexIndex(ctx, 1.0)


def _same_as_oracle(ex, w):
    ox = w["index"]
    for a in ("keys", "key_off", "entries", "repetitive"):
        assert np.array_equal(getattr(ex, a), getattr(ox, a)), a
    if not w["gold"].get("oracle_only"):
        assert index_digest(ex) == w["gold"]["sha256"]


def _same_stats(st, w):
    for f in STAT_FIELDS:
        assert int(st[f]) == int(w["st"][f]), (f, st[f], w["st"][f])
    assert np.float32(st["sample_rate"]).tobytes() == np.float32(w["st"]["sample_rate"]).tobytes()
    assert np.float32(st["mean_frequency"]).tobytes() == np.float32(w["st"]["mean_frequency"]).tobytes()
    if not w["gold"].get("oracle_only"):
        check_index_stats(st, w["gold"])


def _probe_skip_invariant(ctx, w):
    """after a solid build: no position with a clear "frequent enough" bit has a slot in the lookup table, and the clear
    bits are exactly the positions numpy counts below min_freq"""
    clear, bad = ctx.debug_probe_skip_check()
    if w["p"]["mode"] == "solid":
        assert bad == 0
        assert clear == int((_counts(w["case"].name).freq < w["p"]["min_freq"]).sum())
    else:
        assert (clear, bad) == (0, 0)


def _build_and_check(w):
    ctx, vi = _context(w)
    st = ic.device_build(vi, w["p"])
    _same_as_oracle(vi.export(), w)
    _same_stats(st, w)
    _probe_skip_invariant(ctx, w)
    return ctx, vi


@pytest.mark.gpu
@pytest.mark.parametrize("name,pname", ALL_SETS)
def test_device_build_equals_oracle(built, name, pname):
    w = _world(name, pname)
    ctx, vi = _build_and_check(w)
    kt = ctx.kernel_times()
    if w["p"]["mode"] == "solid":
        assert all(n in kt for n in SOLID_KERNELS), sorted(kt)
        # every solid case has tandem candidates (k-mers above tandemFreq) unless the filter is off
        assert ("k_tandem_insert" in kt and "k_tandem_apply" in kt) == (w["p"]["tandem"] > 0), sorted(kt)
    else:
        assert "k_minimizers" in kt and "k_threshold" not in kt, sorted(kt)
    ctx.close()


COUNTER_SETS = [s for s in ALL_SETS if s[0] in ("threshold", "tandem17")]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["direct", "hash"])
@pytest.mark.parametrize("name,pname", COUNTER_SETS)
def test_counter_forms(built, monkeypatch, name, pname, mode):
    """frequencies of 2047 .. 5000 from the direct-addressed array and from the hashed table (whose slot keeps the key
    above 30 count bits); k = 17 fills the 34 key bits of either"""
    monkeypatch.setenv("FG_COUNT_MODE", mode)
    ctx, _ = _build_and_check(_world(name, pname))
    assert "k_count" in ctx.kernel_times()
    ctx.close()


def _batches(nk, budget):
    """batches of whole reads of at most ``budget`` k-mer positions (a longer read is a batch of its own)"""
    n, acc, first = 1, 0, 0
    for r, x in enumerate(nk.tolist()):
        if r > first and acc + x > budget:
            n, acc, first = n + 1, 0, r
        acc += x
    return n


BATCH_SETS = [("tandem13", dict(tandem=10)), ("tandem17", dict(tandem=10)), ("lists", dict(repeat=5.0, min_freq=2)),
              ("windows13", dict(mode="min", window=64)), ("windows13", dict(mode="solid", rate=0.1)),
              ("windows12", dict(mode="min", window=2)), ("windows12", dict(mode="solid", repeat=3.0))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,want", BATCH_SETS, ids=[f"{n}-{i}" for i, (n, _) in enumerate(BATCH_SETS)])
def test_every_read_a_batch_of_its_own(built, monkeypatch, name, want):
    """FG_INDEX_BATCH_KMERS=1: the tandem table is keyed by the read's number INSIDE its batch, the bit words at a
    read's ends are shared between batches (k_pack_bits), reads without k-mers are batches without positions"""
    monkeypatch.setenv("FG_INDEX_BATCH_KMERS", "1")
    w = _world(name, _first(name, **want))
    ctx, _ = _build_and_check(w)
    launches = ctx.kernel_times()["k_threshold" if w["p"]["mode"] == "solid" else "k_minimizers"][1]
    nk = _counts(name).nk
    assert launches == _batches(nk, 1) >= int((nk > 0).sum())
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pname", [s[1] for s in ALL_SETS if s[0] == "threshold"])
def test_threshold_in_twenty_batches(built, monkeypatch, pname):
    w = _world("threshold", pname)
    nk = _counts("threshold").nk
    monkeypatch.setenv("FG_INDEX_BATCH_KMERS", str(int(nk.sum()) // 20))
    ctx, _ = _build_and_check(w)
    assert 20 <= ctx.kernel_times()["k_threshold"][1] == _batches(nk, int(nk.sum()) // 20) <= 22
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,pname", ALL_SETS)
def test_sort_in_slices(built, monkeypatch, name, pname):
    """FG_INDEX_SLICE_ENTRIES at 1/23 of the entries: the sort and the CSR cut run per slice of key bins"""
    w = _world(name, pname)
    monkeypatch.setenv("FG_INDEX_SLICE_ENTRIES", str(max(1, w["st"]["index_entries"] // 23)))
    ctx, _ = _build_and_check(w)
    ctx.close()


PIECE_SETS = [s for s in ALL_SETS if ic.pset(*s).get("min_freq", 2) == 2]


@pytest.mark.gpu
@pytest.mark.parametrize("name,pname", PIECE_SETS)
def test_three_uneven_key_range_pieces(built, name, pname):
    """fg_index_build_range over three uneven bin ranges, one context each (as test_key_range_pieces_and_bin_histogram):
    every piece holds the keys of its range only, the pieces put together are the oracle's index"""
    from flye_amd import dist
    w = _world(name, pname)
    k, cfg = w["case"].k, ic.cfg_of(w["p"])
    shift = np.uint64(2 * k - 12)
    every = np.concatenate([w["index"].keys, w["index"].repetitive])
    used = np.nonzero(np.bincount((every >> shift).astype(np.int64), minlength=4096))[0]
    assert len(used) >= 10
    cuts = [0, int(used[len(used) // 10]), int(used[(6 * len(used)) // 10]), 4096]
    sums, members = np.zeros(2, np.uint64), []
    for r in range(3):
        ctx, vi = _context(w)
        sel = vi.begin(cfg)
        assert int(sel.sum()) >= w["st"]["index_entries"]
        sums += vi.build_range(cuts[r], cuts[r + 1])
        members.append((ctx, vi))
    pieces = []
    for r, (ctx, vi) in enumerate(members):
        st = vi.finish(sums)              # the filter's sums are the whole index's: so is what follows from them
        assert st["repetitive_frequency"] == w["st"]["repetitive_frequency"]
        assert np.float32(st["mean_frequency"]).tobytes() == np.float32(w["st"]["mean_frequency"]).tobytes()
        piece = vi.export()
        for a in (piece.keys, piece.repetitive):
            bins = (a >> shift).astype(np.int64)
            assert np.all((bins >= cuts[r]) & (bins < cuts[r + 1])), r
        assert len(piece.keys) + len(piece.repetitive) > 0
        _probe_skip_invariant(ctx, w)
        pieces.append(piece)
    _same_as_oracle(dist.concat_pieces(pieces), w)
    assert sum(len(p.keys) for p in pieces) == w["st"]["selected_kmers"]
    for ctx, _ in members:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pname", [s[1] for s in ALL_SETS if s[0] == "threshold"])
def test_threshold_selection_in_steps_over_two_counter_ranges(built, pname):
    """as test_solid_selection_in_steps_with_sliced_counters: two 'ranks' count a key range each, their frequency
    arrays add up to the complete one, and the selection from the sum picks the same positions per bin as the one-call
    build -- with thresholds that are sums of two ranks' counts in and above the last histogram bin"""
    import torch
    from flye_amd import dist
    w = _world("threshold", pname)
    cfg, cnt = ic.cfg_of(w["p"]), _counts("threshold")
    ctx, vi = _context(w)
    khist = vi.kmer_hist()
    assert int(khist.sum()) == int(cnt.nk.sum())
    ranges = dist.balanced_bin_ranges(khist, 2)
    dev = torch.device("cuda", 0)
    parts, distinct = [], 0
    for r in range(2):
        d, nb = vi.count_slice(cfg, *ranges[r])
        distinct += d
        assert nb == 1
        ptr, n = vi.batch_freq(0)
        parts.append(dist._view(ptr, n, dev, "<i4").clone())
    assert distinct == w["st"]["total_kmers"]
    assert int(((parts[0] != 0) & (parts[1] != 0)).sum()) == 0          # every k-mer is counted by exactly one range
    assert np.array_equal((parts[0] + parts[1]).cpu().numpy().astype(np.int64), cnt.freq)
    assert min(int(p.max()) for p in parts) >= 2048                     # both ranks hold a family of the overflow bin
    ptr, n = vi.batch_freq(0)
    dist._view(ptr, n, dev, "<i4").add_(parts[0])
    torch.cuda.synchronize()
    vi.batch_select(0)
    hist = vi.selection_done()
    vi.build_range(*ranges[1])
    ctx1, vi1 = _context(w)
    assert np.array_equal(vi1.begin(cfg), hist)
    assert int(hist.sum()) >= w["st"]["index_entries"] > 0
    ctx.close()
    ctx1.close()


def _shard_of(ix, world, rank):
    """what fg_index_keep_targets leaves of an index: the entries of the target reads i with i % world == rank; keys
    and repetitive k-mers stay"""
    from flye_amd import gpu
    own = ((ix.entries >> np.uint64(33)) % np.uint64(world)) == np.uint64(rank)
    key_of = np.repeat(np.arange(len(ix.keys)), _lists_of(ix))
    off = np.zeros(len(ix.keys) + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(key_of[own], minlength=len(ix.keys)))
    return gpu.IndexExport(ix.keys, off, ix.entries[own], ix.repetitive)


GROUP_SETS = [("threshold", dict(repeat=100.0)), ("threshold", dict(repeat=1.5)), ("lists", dict(repeat=5.0, min_freq=2)),
              ("lists", dict(repeat=ic.LISTS_FOURTH_RATE))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,want", GROUP_SETS, ids=[f"{n}-{i}" for i, (n, _) in enumerate(GROUP_SETS)])
def test_group_of_two_builds_the_shards(built, name, want):
    """gpu.Group([0, 0]): the counters of two key ranges summed on the device, the pieces scattered by target owner.
    Every member ends with the oracle's index restricted to its targets; the statistics are the whole index's."""
    from flye_amd import gpu
    w = _world(name, _first(name, **want))
    g = gpu.Group([0, 0], w["case"].k)
    g.set_reads(w["case"].reads)
    _same_stats(g.build(ic.cfg_of(w["p"]), sample_rate=1.0), w)
    total = 0
    for r in range(2):
        mv = gpu.VertexIndex(g.member(r), 1.0)
        assert mv.shard() == (2, r)
        got, want_ix = mv.export(), _shard_of(w["index"], 2, r)
        for a in ("keys", "key_off", "entries", "repetitive"):
            assert np.array_equal(getattr(got, a), getattr(want_ix, a)), (r, a)
        total += len(got.entries)
    assert total == w["st"]["index_entries"] > 0
    g.close()


# the 3000-base homopolymer and the period-1 and period-2 arrays: every one of their positions hits the same few lists
# (400 000 seed hits for the homopolymer alone) and the oracle's chaining is quadratic in them -- a minute on the CPU.
# Their probes are compared hit for hit; their records are left to the oracle-cost-bounded sweeps.
OVERLAP_SETS = [("lists", dict(repeat=5.0, min_freq=2), ()), ("windows13", dict(mode="min", window=64), (13, 15, 16)),
                ("windows12", dict(mode="min", window=64), (13, 15, 16))]


@functools.lru_cache(maxsize=None)
def _overlap_world(name, pname, skip):
    from helpers import cpu_seed_hits
    from oracle import oracle as O
    w = _world(name, pname)
    rs = w["case"].reads
    q_all = np.arange(0, 2 * rs.n, dtype=np.uint32)
    q = q_all[~np.isin(q_all >> 1, np.array(skip, np.uint32))]
    ores = w["o"].overlaps(O.detector_params(ic.cfg_of(w["p"]), min_overlap=100, only_max_ext=False), q)
    return q_all, cpu_seed_hits(rs, w["index"], w["case"].k, q_all), q, ores


@pytest.mark.parametrize("name,want,skip", OVERLAP_SETS, ids=[n for n, _, _ in OVERLAP_SETS])
def test_overlap_worlds_have_hits_and_records(built, name, want, skip):
    w = _world(name, _first(name, **want))
    q_all, (counts, hits), q, ores = _overlap_world(name, _first(name, **want), skip)
    assert len(ores.recs) > 0 and len(hits) > 10 * len(ores.recs) and len(q_all) - len(q) == 2 * len(skip)
    # a reverse-strand query whose k-mer is its own reverse complement finds its read's own entry under the FORWARD
    # record: not the trivial match of overlap.cpp:188-190, it is a hit (13 indexed ACGTACGTACGT positions at k = 12)
    rs, k = w["case"].reads, w["case"].k
    qi = np.repeat(q_all, counts.astype(np.int64)).astype(np.int64)
    own = (qi & 1 == 1) & (hits["ext_id"] == (qi ^ 1)) & (hits["ext_pos"] == rs.length[qi >> 1] - k - hits["cur_pos"])
    assert int(own.sum()) == (13 if k % 2 == 0 else 0) and set((qi[own] >> 1).tolist()) <= {22}
    if name == "lists":          # queries whose k-mers are keys with empty lists: looked up, found, no hit
        ix = w["index"]
        empty = ix.keys[_lists_of(ix) == 0]
        assert len(empty) == 18 and np.isin(_counts(name).canon, empty).sum() == 303 * 18


@pytest.mark.gpu
@pytest.mark.parametrize("partitioned", [False, True], ids=["in_query_order", "partitioned"])
@pytest.mark.parametrize("name,want,skip", OVERLAP_SETS, ids=[n for n, _, _ in OVERLAP_SETS])
def test_overlaps_over_empty_lists_and_the_sparse_sketch(built, monkeypatch, name, want, skip, partitioned):
    """All reads on both strands, minimum overlap 100, every primary: the tables built over keys with empty lists and
    over the w = 64 sketch serve probes (fg_probe_hits equals the numpy seed collection on the oracle's index, hit for
    hit) and getSeqOverlapsBatch equals the oracle's records -- with the probes in query order (k_probe) and ordered
    by table region (k_probe_emit; several sub-batches)"""
    from flye_amd import gpu
    if partitioned:
        monkeypatch.setenv("FG_PROBE_PARTITION", "1")
        monkeypatch.setenv("FG_PROBE_SUB_KMERS", "20000")
    w = _world(name, _first(name, **want))
    q_all, (ccounts, chits), q, ores = _overlap_world(name, _first(name, **want), skip)
    ctx, vi = _build_and_check(w)
    det = gpu.OverlapDetector.for_assemble(ctx, vi, ic.cfg_of(w["p"]), min_overlap=100)
    det.p.only_max_ext = 0
    counts, ptr, n = det.probe_hits(q_all)
    differ = np.nonzero(counts != ccounts)[0]
    assert not len(differ), (differ[:8], counts[differ[:8]], ccounts[differ[:8]])
    assert gpu.seed_hits_to_host(ptr, n).tobytes() == chits.tobytes()
    check_overlaps_equal(det.getSeqOverlapsBatch(q), ores, False)
    assert ("k_probe_emit" in ctx.kernel_times()) == partitioned
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["windows13", "windows12"])
def test_windows_outside_1_to_64_are_refused(built, name):
    """the ring of k_minimizers holds MAXW + 2 entries; 0 and 65 are argument errors and leave the context usable"""
    from flye_amd import gpu
    w = _world(name, _first(name, mode="min", window=64))
    ctx, vi = _context(w)
    for wnd in (0, 65, -1):
        with pytest.raises(gpu.FlyeGpuError) as e:
            vi.buildIndexMinimizers(1, wnd, 100.0)
        assert e.value.code == -3 and "wrong minimizer length" in str(e.value)
    _same_stats(ic.device_build(vi, w["p"]), w)
    _same_as_oracle(vi.export(), w)
    ctx.close()
