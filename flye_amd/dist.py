"""Multi-GPU layouts of the path: one process per GPU.

Option A (what bench.py runs): the index replicated on every rank.

* INDEX BUILD, sharded by key range (``build_index_sharded``).  ``balanced_bin_ranges`` cuts the 4096 key bins
  into ``world`` contiguous ranges of about equal weight; rank r holds the exact k-mer counters of ITS range only,
  sorts and run-length encodes only its range.  Collectives: an all-reduce of the k-mer frequencies per batch of
  reads (solid mode: each rank knows the counts of its own key range), an all-reduce of filterFrequentKmers' two
  integer sums (vertex_index.cpp:175-184 takes them over ALL keys), then an all-gather of the CSR pieces -- keys,
  list offsets, entries, repetitive keys, in rank order = key order -- straight into every rank's own full-size
  index arrays (``fg_index_gather_begin / _end``).  With the nccl backend (= RCCL over xGMI) everything travels
  device to device.
* OVERLAP STAGE: reads shard by sequence id, rank r owns the forward reads i with i % world == r and
  computes their lists against its full index copy: no data-path collective; only the barrier / max-time
  reduction of the bench.

Option B (``build_index_option_b`` + ``overlaps_option_b``): the index sharded by TARGET read.  The same key-range
build and all-gather, then every rank keeps only the list entries of the target reads it owns (read i, i % world ==
rank; ``fg_index_keep_targets``): the entry arrays -- the only part of the index that shrinks when sharded -- take
1/world of the memory; keys, lookup table and repetitive k-mers stay replicated.  Queries walk in global batches
that every rank cuts the same way; each rank probes the whole batch against its shard (``fg_probe_hits``), the
per-(destination, query) hit counts and then the 12-byte hits go to the queries' owners with two
``all_to_all_single`` (device to device with nccl = RCCL, through host copies with gloo), and each owner restores
the reference's emission order on the device and runs the rest of getSeqOverlaps (``fg_overlaps_from_hits``).
Bit-exact against the replicated index by test (tests/test_option_b.py: W shards as W contexts on one GPU, and two
gloo processes).  ``build_index_option_b`` lands the whole index on every rank before keep_targets cuts it, so its
build peak is that of option A.

Option B built directly (``build_index_option_b_direct``): the same key-range build up to ``finish``, then
``scatter_pieces_inplace`` instead of the all-gather.  Every rank splits its piece by target owner on the device
(``fg_index_piece_split``: a world x keys count matrix and the entries in destination-major order), keys and repetitive
keys are replicated by broadcasts, and the count rows and entry segments travel with one ``all_to_all_single`` each
straight into the shard's own arrays (``fg_index_scatter_begin``); sources arrive in rank order = key order, so what
lands is the shard's CSR, and ``fg_index_scatter_end`` scans the counts into offsets, checks the arrays on the device
and builds the lookup structures.  With K keys, R repetitive keys, table bytes T, bits B of the whole index, a piece
of (K_s, E_s, R_s) with table T_s and a shard of E_shard entries, the library holds above the reads at most
    max(P + T_s + B + 8 E_s + 16 (W K_s + 1),  P + 8 E_s + 8 (W K_s + 1) + S,  S + T + B) + scan scratch,
    P = 8 (2 K_s + 1 + E_s + R_s),  S = 8 (2 K + 1 + R + E_shard)
-- no term in the total entry count.  MEASURED on one GPU (tests/test_option_b_direct.py: W = 4 on 52 Mbp, asserted;
the gather + keep_targets path exceeds the bound on the same input); the figure at CHM13 scale stays
arithmetic, and no run on more than one GPU has been measured.
"""
from __future__ import annotations

import os
import time

import numpy as np


def shard_queries(n_reads: int, rank: int, world: int, first_id: int = 0) -> np.ndarray:
    """FastaRecord ids (forward strand) owned by ``rank``."""
    idx = np.arange(rank, n_reads, world, dtype=np.int64)
    return (first_id + 2 * idx).astype(np.uint32)


def owner_of(read_index, world: int):
    return np.asarray(read_index) % world


def merge_sharded(per_rank_ids, per_rank_lists):
    """Reassemble per-read overlap lists in read order from per-rank results."""
    merged = {}
    for ids, lists in zip(per_rank_ids, per_rank_lists):
        for rid, lst in zip(ids, lists):
            merged[int(rid)] = lst
    return [merged[k] for k in sorted(merged)]


# ---- option B of SURVEY.md §8(e): index sharded by TARGET read, seed hits exchanged -----------------------------
# Not the layout bench.py runs (the replicated index fits 288 GB for every BASELINE config).  The order in
# which the query's owner must line the received hits up before the std::sort emulation, in numpy (the device form is
# k_recv_keys / k_recv_place in fg_overlap.hip):
def owner_of_target(record, world: int):
    """the rank whose index shard holds the entries of this stored record (forward or reverse strand of read i)"""
    return (np.asarray(record) >> 1) % world


def option_b_receive_order(cur_pos, ext_pos, ext_id, flip_at_cur, ext_len, k: int):
    """Hits (curPos, extPos, extId) of ONE query gathered from the index shards in arbitrary order -> the
    permutation that restores the reference's emission order, i.e. the input order of its unstable hit sort
    (overlap.cpp:176-204): ascending curPos, and per query k-mer ascending STORED global position
    (vertex_index.cpp:108-114).  The stored (record, position) of a hit is recovered from what was reported:
    a flipped query k-mer reports (record ^ 1, len - pos - k) (vertex_index.h:158-174), and whether the k-mer at
    curPos was flipped is known to the receiver (``flip_at_cur[curPos]``); ``ext_len[i]`` = length of hit i's
    target.  (curPos, stored record, stored position) is a total order: no two hits of a query share it."""
    cur_pos = np.asarray(cur_pos, np.int64)
    ext_pos = np.asarray(ext_pos, np.int64)
    ext_id = np.asarray(ext_id, np.int64)
    fl = np.asarray(flip_at_cur, bool)[cur_pos]
    rec = np.where(fl, ext_id ^ 1, ext_id)
    pos = np.where(fl, np.asarray(ext_len, np.int64) - ext_pos - k, ext_pos)
    return np.lexsort((pos, rec, cur_pos))


# ---- sharded index build ------------------------------------------------------------------------------
def balanced_bin_ranges(hist, world: int):
    """``world`` contiguous bin ranges [lo, hi) covering all bins, each holding about 1/world of the accepted
    k-mer positions (cut where the running sum passes r/world of the total).  Identical on every rank: the
    histogram is."""
    h = np.asarray(hist, dtype=np.float64)
    n = len(h)
    cs = np.concatenate([[0.0], np.cumsum(h)])
    total = cs[-1]
    cuts = [0]
    for r in range(1, world):
        target = total * r / world
        c = int(np.searchsorted(cs, target, side="left"))
        cuts.append(min(n, max(cuts[-1], c)))
    cuts.append(n)
    return [(cuts[r], cuts[r + 1]) for r in range(world)]


def concat_pieces(pieces):
    """CSR pieces (keys, key_off, entries, repetitive) of ascending key ranges -> one index: the offsets of
    piece r are shifted by the entries of the pieces before it.  Host form of what the all-gather assembles."""
    from .gpu import IndexExport
    keys = np.concatenate([p.keys for p in pieces])
    ent = np.concatenate([p.entries for p in pieces])
    rep = np.concatenate([p.repetitive for p in pieces])
    off = [np.zeros(1, np.uint64)]
    base = 0
    for p in pieces:
        off.append(p.key_off[1:].astype(np.uint64) + np.uint64(base))
        base += len(p.entries)
    return IndexExport(keys, np.concatenate(off), ent, rep)


def allgather_pieces(piece, rank: int, world: int, dev):
    """All-gather of the ranks' CSR pieces (torch int64 tensors keys[nk], key_off[nk + 1] relative to the
    piece, entries[ne], repetitive[nr]; ascending key ranges in rank order) into the full arrays on every
    rank.  Pieces differ in size: their sizes are exchanged first, then every rank broadcasts its slice of
    the assembled arrays (a ring all-gather's volume, no padding).  Returns (keys, key_off, entries,
    repetitive, (K, E, R), bytes moved)."""
    import torch
    import torch.distributed as td
    pk, po, pe, pr = piece
    nk, ne, nr = len(pk), len(pe), len(pr)
    sizes = torch.zeros((world, 3), dtype=torch.int64, device=dev)
    sizes[rank] = torch.tensor([nk, ne, nr], dtype=torch.int64, device=dev)
    td.all_reduce(sizes)
    sz = sizes.cpu().numpy()
    K, E, R = (int(x) for x in sz.sum(axis=0))
    kb = np.concatenate([[0], np.cumsum(sz[:, 0])]).astype(np.int64)
    eb = np.concatenate([[0], np.cumsum(sz[:, 1])]).astype(np.int64)
    rb = np.concatenate([[0], np.cumsum(sz[:, 2])]).astype(np.int64)
    keys = torch.empty(max(K, 1), dtype=torch.int64, device=dev)
    off = torch.empty(K + 1, dtype=torch.int64, device=dev)
    ent = torch.empty(max(E, 1), dtype=torch.int64, device=dev)
    rep = torch.empty(max(R, 1), dtype=torch.int64, device=dev)
    keys[kb[rank]:kb[rank + 1]] = pk
    off[kb[rank]:kb[rank + 1]] = po[:nk] + int(eb[rank])     # list offsets shift by the entries of the pieces before
    ent[eb[rank]:eb[rank + 1]] = pe
    rep[rb[rank]:rb[rank + 1]] = pr
    off[K] = E
    moved = world * 24
    for r in range(world):
        for arr, b in ((keys, kb), (off, kb), (ent, eb), (rep, rb)):
            if b[r + 1] > b[r]:
                td.broadcast(arr[b[r]:b[r + 1]], src=r)
                moved += int(b[r + 1] - b[r]) * 8
    return keys, off, ent, rep, (K, E, R), moved


class _DevArr:
    """device memory as a ``__cuda_array_interface__`` object (torch wraps it without copying)"""

    def __init__(self, ptr: int, n: int, typestr: str = "<i8"):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def _view(ptr: int, n: int, cuda_dev, typestr="<i8"):
    """torch tensor over n elements of device memory at ptr (no copy)"""
    import torch
    if n == 0 or not ptr:
        return torch.empty(0, dtype=torch.int64 if typestr == "<i8" else torch.int32, device=cuda_dev)
    return torch.as_tensor(_DevArr(ptr, n, typestr), device=cuda_dev)


def _all_reduce_dev(t, on_device: bool):
    """sum over the ranks, in place, of a device tensor: RCCL on the tensor itself, or (gloo rehearsal) through a
    host copy"""
    import torch
    import torch.distributed as td
    if on_device:
        td.all_reduce(t)
        # the library reads the array on ITS stream next (fg_index_batch_select): the collective has to be complete on
        # the host's clock, not just ordered on torch's stream
        torch.cuda.synchronize()
    else:
        h = t.cpu()
        td.all_reduce(h)
        t.copy_(h)


def _broadcast_dev(t, src: int, on_device: bool):
    import torch.distributed as td
    if t.numel() == 0:
        return
    if on_device:
        td.broadcast(t, src=src)
    else:
        h = t.cpu()
        td.broadcast(h, src=src)
        t.copy_(h)


def gather_pieces_inplace(vi, rank: int, world: int, on_device: bool, sample_rate_of, force=False):
    """All-gather of the ranks' CSR pieces (ascending key ranges in rank order) straight into the context's own
    full-size arrays (fg_index_gather_begin / _end): no second copy of the index.  Pieces differ in size: their sizes
    are exchanged first, then every rank broadcasts its slice (a ring all-gather's volume, no padding).
    ``sample_rate_of(E)`` gives VertexIndex::getSampleRate() for the whole index.  Returns ((K, E, R), bytes moved)."""
    import torch
    import torch.distributed as td
    cuda = torch.device("cuda", torch.cuda.current_device())
    red = cuda if on_device else torch.device("cpu")
    (nk, ne, nr), _ = vi.device_arrays()
    sizes = torch.zeros((world, 3), dtype=torch.int64, device=red)
    sizes[rank] = torch.tensor([nk, ne, nr], dtype=torch.int64, device=red)
    if world > 1 or force:
        td.all_reduce(sizes)
    sz = sizes.cpu().numpy()
    K, E, R = (int(x) for x in sz.sum(axis=0))
    kb = np.concatenate([[0], np.cumsum(sz[:, 0])]).astype(np.int64)
    eb = np.concatenate([[0], np.cumsum(sz[:, 1])]).astype(np.int64)
    rb = np.concatenate([[0], np.cumsum(sz[:, 2])]).astype(np.int64)
    full, piece, psz = vi.gather_begin(K, E, R)
    assert psz == [nk, ne, nr]
    keys, off, ent, rep = _view(full[0], K, cuda), _view(full[1], K + 1, cuda), _view(full[2], E, cuda), _view(full[3], R, cuda)
    pk, po, pe, pr = _view(piece[0], nk, cuda), _view(piece[1], nk + 1, cuda), _view(piece[2], ne, cuda), _view(piece[3], nr, cuda)
    if nk:
        keys[kb[rank]:kb[rank + 1]] = pk
        off[kb[rank]:kb[rank + 1]] = po[:nk] + int(eb[rank])     # list offsets shift by the entries of the pieces before
    if ne:
        ent[eb[rank]:eb[rank + 1]] = pe
    if nr:
        rep[rb[rank]:rb[rank + 1]] = pr
    off[K:K + 1] = E
    moved = world * 24
    if world > 1 or force:
        for r in range(world):
            for arr, b in ((keys, kb), (off, kb), (ent, eb), (rep, rb)):
                if b[r + 1] > b[r]:
                    _broadcast_dev(arr[b[r]:b[r + 1]], r, on_device)
                    moved += int(b[r + 1] - b[r]) * 8
    torch.cuda.synchronize()
    vi.gather_end(sample_rate_of(E))
    vi.stats = dict(vi.stats or {}, selected_kmers=K, index_entries=E, repetitive_kmers=R,
                    sample_rate=float(np.float32(sample_rate_of(E))))
    return (K, E, R), moved


def _build_piece(vi, cfg: dict, rank: int, world: int, on_device: bool):
    """The key-range part of a sharded build, up to and including ``finish``: this rank's piece is in the context.
    -> (statistics so far, (bin ranges, piece sizes, frequency all-reduce bytes, (t0, t1, t2)), sample_rate_of,
    whether collectives run).  What follows -- the all-gather of option A, the scatter of option B built directly --
    is the caller's."""
    import torch
    import torch.distributed as td
    cuda = torch.device("cuda", torch.cuda.current_device())
    red = cuda if on_device else torch.device("cpu")
    # FLYE_FORCE_COLLECTIVES: run every collective also in a one-rank group (tools/sharded_build_check.py: one rank
    # on a one-GPU box then exercises every RCCL call of this path)
    coll = world > 1 or bool(os.environ.get("FLYE_FORCE_COLLECTIVES"))
    t0 = time.perf_counter()
    freq_bytes = 0
    distinct = 0
    if cfg["use_minimizers"]:
        hist = vi.begin(cfg)
        ranges = balanced_bin_ranges(hist, world)
    else:
        ranges = balanced_bin_ranges(vi.kmer_hist(), world)
        distinct, n_batches = vi.count_slice(cfg, *ranges[rank])
        for b in range(n_batches):
            ptr, n = vi.batch_freq(b)
            if coll and n:
                _all_reduce_dev(_view(ptr, n, cuda, "<i4"), on_device)
                freq_bytes += 4 * n
            vi.batch_select(b)
        vi.selection_done()
    sums = vi.build_range(*ranges[rank])
    t1 = time.perf_counter()
    tot = torch.tensor(np.concatenate([sums.astype(np.int64), [distinct]]), device=red)
    if coll:
        td.all_reduce(tot)
    tot = tot.cpu().numpy()
    st = dict(vi.finish(tot[:2].astype(np.uint64)))
    st["total_kmers"] = int(tot[2])
    (nk, ne, nr), _ = vi.device_arrays()
    t2 = time.perf_counter()
    total_bases = np.float32(vi.ctx.rs.total_bases)

    def sample_rate_of(E):
        # VertexIndex::getSampleRate(): the ctor value, or totalLen / totalEntries over the WHOLE index (vertex_index.cpp:480-482)
        if cfg["use_minimizers"]:
            return float(total_bases / np.float32(E)) if E else float("inf")
        return vi._sample_rate_init

    return st, (ranges, (nk, ne, nr), freq_bytes, (t0, t1, t2)), sample_rate_of, coll


def build_index_sharded(vi, cfg: dict, rank: int, world: int, on_device: bool):
    """The build main_assemble.cpp:195-223 selects, sharded over the ranks of the default process group
    (SURVEY.md §8e).  ``on_device``: collectives on device memory (nccl = RCCL over xGMI); otherwise through host
    copies (gloo rehearsal).

    * solid k-mers: the key bins are cut into ``world`` ranges holding equal numbers of k-mer positions
      (``fg_index_kmer_hist``, identical on every rank); rank r keeps the exact counters of ITS range only (an
      eighth of the 4^k array at 8 ranks) and counts those k-mers over all reads; then, batch of reads by batch
      (bounded scratch), every rank writes the frequencies it knows, an all-reduce makes the array complete, and
      every rank runs the per-read selection on it (replicated: it is cheap and leaves every rank with the same
      selection bits, so nothing else of the selection is exchanged);
    * minimizers: the selection needs no counters and no exchange; ranges are balanced on the accepted positions;
    * rank r sorts and run-length encodes its range (the same range its counters cover); all-reduce of
      filterFrequentKmers' two sums; finish; all-gather of the CSR pieces in place.
    Returns the index statistics plus what the collectives moved."""
    st, (ranges, (nk, ne, nr), freq_bytes, (t0, t1, t2)), sample_rate_of, coll = _build_piece(vi, cfg, rank, world, on_device)
    (K, E, R), moved = gather_pieces_inplace(vi, rank, world, on_device, sample_rate_of, force=coll)
    t3 = time.perf_counter()
    st.update(vi.stats)
    st.update(bin_range=ranges[rank], piece=(int(nk), int(ne), int(nr)),
              collective_bytes=moved + 24 + freq_bytes, freq_allreduce_bytes=freq_bytes,
              select_and_sort_s=t1 - t0, finish_s=t2 - t1, allgather_s=t3 - t2, import_s=0.0, build_seconds=t3 - t0)
    vi.stats = st
    return st


# ---- option B: build and overlap stage ----------------------------------------------------------------------------
def build_index_option_b(vi, cfg: dict, rank: int, world: int, on_device: bool):
    """The key-range sharded build (``build_index_sharded``), then the index restricted to the entries of the target
    reads this rank owns.  Statistics and getSampleRate() stay those of the whole index."""
    st = build_index_sharded(vi, cfg, rank, world, on_device)
    st["shard_entries"] = vi.keep_targets(world, rank)
    vi.stats = st
    return st


# ---- option B built directly: key-range pieces -> per-destination parts -> target shards ---------------------------
def split_piece_host(keys, key_off, entries, world: int):
    """Host reference of ``fg_index_piece_split``: the piece (keys, key_off[len(keys) + 1], entries ascending per
    key) partitioned by target owner ((entry >> 33) % world).  -> (counts[world, n_keys] = entries of key j owned by
    rank d, the entries destination major / key major inside a destination / list order inside a key,
    totals[world] = entries per destination), all uint64."""
    off = np.asarray(key_off).astype(np.int64)
    ent = np.ascontiguousarray(entries, np.uint64)
    nk = len(off) - 1
    assert nk == len(keys) and (nk == 0 or int(off[-1]) == len(ent))
    owner = ((ent >> np.uint64(33)) % np.uint64(world)).astype(np.int64)
    slot = owner * nk + np.repeat(np.arange(nk, dtype=np.int64), np.diff(off))
    counts = np.bincount(slot, minlength=world * nk).astype(np.uint64).reshape(world, nk)
    return counts, ent[np.argsort(slot, kind="stable")], counts.sum(axis=1, dtype=np.uint64)


def _all_to_all_dev(out, inp, out_splits, in_splits, on_device: bool, coll: bool):
    """all_to_all_single of 1-d tensors with the given split sizes: on the tensors themselves (RCCL), or (gloo
    rehearsal) through host copies; without collectives (one rank) the input is the output"""
    import torch
    import torch.distributed as td
    if not coll:
        out.copy_(inp)
    elif on_device:
        td.all_to_all_single(out, inp, output_split_sizes=out_splits, input_split_sizes=in_splits)
    else:
        h = torch.empty(out.numel(), dtype=out.dtype)
        td.all_to_all_single(h, inp.cpu().contiguous(), output_split_sizes=out_splits, input_split_sizes=in_splits)
        out.copy_(h)


def exchange_split_parts(piece_keys, piece_rep, counts, split_entries, totals, rank: int, world: int, on_device: bool,
                         alloc=None, force=False):
    """The exchange of the direct option-B build, on int64 tensors (views of the context's device arrays in
    ``scatter_pieces_inplace``; CPU tensors in the gloo rehearsal).  This rank gives its piece's keys and repetitive
    keys, the flattened [world, n_keys] count matrix, the split entries and the entries per destination
    (``fg_index_piece_split`` / ``split_piece_host``).  Sizes are exchanged first (one all-reduce: the pieces' sizes
    and every rank's per-destination totals); keys and repetitive keys are replicated by broadcasts of each rank's
    slice, as in ``gather_pieces_inplace``; the count rows and the entry segments go through one
    ``all_to_all_single`` each.  Sources arrive in rank order = key order: the received counts are the shard's
    per-key list lengths for all keys, the received entries ARE its entry array in CSR order.
    ``alloc(K, E_shard, R)`` -> the destination tensors (keys[K], key_off[K + 1], entries[E_shard], repetitive[R]).
    Returns (keys, key_off -- the COUNTS in [0, K), not yet scanned --, entries, repetitive, (K, E, R) of the whole
    index, E_shard, bytes moved)."""
    import torch
    import torch.distributed as td
    dev = piece_keys.device
    red = dev if on_device else torch.device("cpu")
    coll = world > 1 or force
    nk, ne, nr = len(piece_keys), len(split_entries), len(piece_rep)
    totals = [int(x) for x in np.asarray(totals)]
    assert len(totals) == world and sum(totals) == ne and counts.numel() == world * nk
    sizes = torch.zeros((world, 3 + world), dtype=torch.int64, device=red)
    sizes[rank] = torch.tensor([nk, ne, nr] + totals, dtype=torch.int64, device=red)
    if coll:
        td.all_reduce(sizes)
    sz = sizes.cpu().numpy()
    K, E, R = (int(x) for x in sz[:, :3].sum(axis=0))
    kb = np.concatenate([[0], np.cumsum(sz[:, 0])]).astype(np.int64)
    rb = np.concatenate([[0], np.cumsum(sz[:, 2])]).astype(np.int64)
    e_from = sz[:, 3 + rank]                                 # entries source s holds for this rank
    e_shard = int(e_from.sum())
    if alloc is None:
        def alloc(K, e_shard, R):
            return tuple(torch.empty(n, dtype=torch.int64, device=dev) for n in (K, K + 1, e_shard, R))
    keys, off, ent, rep = alloc(K, e_shard, R)
    if nk:
        keys[kb[rank]:kb[rank + 1]] = piece_keys
    if nr:
        rep[rb[rank]:rb[rank + 1]] = piece_rep
    moved = world * 8 * (3 + world)
    if coll:
        for r in range(world):
            for arr, b in ((keys, kb), (rep, rb)):
                if b[r + 1] > b[r]:
                    _broadcast_dev(arr[b[r]:b[r + 1]], r, on_device)
                    moved += int(b[r + 1] - b[r]) * 8
    _all_to_all_dev(off[:K], counts, [int(x) for x in sz[:, 0]], [nk] * world, on_device, coll)
    _all_to_all_dev(ent[:e_shard], split_entries, [int(x) for x in e_from], totals, on_device, coll)
    moved += 8 * (world * nk + ne)
    return keys, off, ent, rep, (K, E, R), e_shard, moved


def scatter_pieces_inplace(vi, rank: int, world: int, on_device: bool, sample_rate_of, force=False):
    """From the ranks' key-range pieces (what ``finish`` left in the contexts) straight to the ranks' target shards:
    split on the device (``fg_index_piece_split``), ``exchange_split_parts`` into the arrays ``fg_index_scatter_begin``
    allocates, ``fg_index_scatter_end`` (scan, device checks, lookup structures).  No rank allocates the full entry
    array: DESIGN.md §6 has the peak.  ``sample_rate_of(E)`` gives VertexIndex::getSampleRate() for the whole index.
    Returns ((K, E, R) of the whole index, this shard's entries, bytes moved)."""
    import torch
    cuda = torch.device("cuda", torch.cuda.current_device())
    (nk, ne, nr), piece = vi.device_arrays()             # the piece's arrays stay where they are until scatter_end
    cnt_ptr, ent_ptr, totals = vi.split_piece(world)

    def alloc(K, e_shard, R):
        full = vi.scatter_begin(world, rank, K, e_shard, R)
        return _view(full[0], K, cuda), _view(full[1], K + 1, cuda), _view(full[2], e_shard, cuda), _view(full[3], R, cuda)

    _, _, _, _, (K, E, R), e_shard, moved = exchange_split_parts(
        _view(piece[0], nk, cuda), _view(piece[3], nr, cuda), _view(cnt_ptr, world * nk, cuda), _view(ent_ptr, ne, cuda),
        totals, rank, world, on_device, alloc, force)
    torch.cuda.synchronize()
    vi.scatter_end(sample_rate_of(E))
    vi.stats = dict(vi.stats or {}, selected_kmers=K, index_entries=E, repetitive_kmers=R, shard_entries=e_shard,
                    sample_rate=float(np.float32(sample_rate_of(E))))
    return (K, E, R), e_shard, moved


def build_index_option_b_direct(vi, cfg: dict, rank: int, world: int, on_device: bool):
    """Option B without the all-gather: the key-range build of ``build_index_sharded`` up to and including ``finish``,
    then ``scatter_pieces_inplace``.  The context ends as after ``build_index_option_b`` -- the shard of the target
    reads this rank owns, statistics and getSampleRate() those of the whole index -- but never held more entries
    than its piece, the piece's split copy and its shard."""
    st, (ranges, (nk, ne, nr), freq_bytes, (t0, t1, t2)), sample_rate_of, coll = _build_piece(vi, cfg, rank, world, on_device)
    (K, E, R), e_shard, moved = scatter_pieces_inplace(vi, rank, world, on_device, sample_rate_of, force=coll)
    t3 = time.perf_counter()
    st.update(vi.stats)
    st.update(bin_range=ranges[rank], piece=(int(nk), int(ne), int(nr)), shard_entries=e_shard,
              collective_bytes=moved + 24 + freq_bytes, freq_allreduce_bytes=freq_bytes,
              select_and_sort_s=t1 - t0, finish_s=t2 - t1, scatter_s=t3 - t2, build_seconds=t3 - t0)
    vi.stats = st
    return st


def _hits_tensor(hits, n: int):
    """probe_hits' hits as an int32 tensor [n, 3]: a device pointer is wrapped without a copy (a stand-in detector
    may hand a SEED_HIT_DTYPE numpy array)"""
    import torch
    if isinstance(hits, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(hits).view(np.int32).reshape(-1, 3).copy())
    return _view(int(hits), 3 * n, torch.device("cuda", torch.cuda.current_device()), "<i4").reshape(-1, 3)


def exchange_hits(counts, hits, owner, rank: int, world: int, on_device: bool):
    """The two all_to_all_single of option B for one batch.  ``counts[q]`` hits of batch query q in ``hits`` (int32
    tensor [n, 3], query after query), ``owner[q]`` its rank.  Returns (counts [world, n_mine] of this rank's queries
    in batch order, sources in rank order; the received hits [sum, 3]: sources one after another, inside a source the
    queries in batch order)."""
    import torch
    import torch.distributed as td
    counts = np.asarray(counts, np.int64)
    owner = np.asarray(owner, np.int64)
    order = np.argsort(owner, kind="stable")                 # queries grouped by destination, batch order inside
    start = np.concatenate([[0], np.cumsum(counts)])[:-1]
    c_sorted = counts[order]
    before = np.concatenate([[0], np.cumsum(c_sorted)])[:-1]
    idx = np.repeat(start[order] - before, c_sorted) + np.arange(int(c_sorted.sum()), dtype=np.int64)
    n_to = np.bincount(owner, minlength=world)              # queries per destination
    h_to = np.bincount(owner, weights=counts, minlength=world).astype(np.int64)
    n_mine = int(n_to[rank])
    dev = hits.device if on_device else torch.device("cpu")
    send_c = torch.from_numpy(c_sorted.copy()).to(dev)
    recv_c = torch.empty(world * n_mine, dtype=torch.int64, device=dev)
    td.all_to_all_single(recv_c, send_c, output_split_sizes=[n_mine] * world, input_split_sizes=n_to.tolist())
    rc = recv_c.cpu().numpy().reshape(world, n_mine)
    h_from = rc.sum(axis=1)
    src = hits if on_device else hits.cpu()
    send_h = src.index_select(0, torch.from_numpy(idx).to(src.device)).reshape(-1).contiguous()
    recv_h = torch.empty(3 * int(h_from.sum()), dtype=torch.int32, device=send_h.device)
    td.all_to_all_single(recv_h, send_h, output_split_sizes=(3 * h_from).tolist(), input_split_sizes=(3 * h_to).tolist())
    return rc, recv_h.reshape(-1, 3)


def overlaps_option_b(det, rank: int, world: int, on_device: bool, batch_reads: int = 4096):
    """The overlap stage of option B over all reads of the context (forward query ids): global batches of
    ``batch_reads`` reads, every rank probes the whole batch against its shard, the hits go to the queries' owners
    (read i -> rank i % world, as ``shard_queries``), each rank computes its own queries from what it received.
    Returns ([(this rank's query ids, OverlapResult)] per batch, bytes of hits sent to other ranks)."""
    import torch
    ctx = det.ctx
    n_reads, first = int(ctx.n_reads), int(ctx.first_id)
    out, moved = [], 0
    for b0 in range(0, n_reads, batch_reads):
        reads = np.arange(b0, min(n_reads, b0 + batch_reads), dtype=np.int64)
        q = (first + 2 * reads).astype(np.uint32)
        owner = owner_of(reads, world)
        counts, hits, n = det.probe_hits(q)
        rc, recv = exchange_hits(counts, _hits_tensor(hits, n), owner, rank, world, on_device)
        moved += 12 * int(np.asarray(counts, np.int64)[owner != rank].sum())
        if on_device:
            torch.cuda.synchronize()
        mine = q[owner == rank]
        out.append((mine, det.getSeqOverlapsFromHits(mine, rc, recv)))
    return out, moved
