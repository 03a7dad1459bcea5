// Device group (include/flye_gpu.h, fg_group_*): several contexts of one process behind one handle -- option B of the
// multi-GPU layout for a caller that is one process and has no collectives.  This file is host code:
// it composes the step calls of the C ABI on every member, one host thread per member, and moves the pieces between
// the members with hipMemcpyPeerAsync.  The one kernel it adds to the library is k_freq_accumulate (fg_index.hip),
// the "+=" of the frequency sum; everything else on the device is what the step calls already run.
//
// The C++ restatement of flye_amd/dist.py: build_index_option_b_direct (balanced_bin_ranges, _build_piece,
// scatter_pieces_inplace) and overlaps_option_b, with two differences.  The frequency all-reduce is a reduce-scatter
// through a bounded staging buffer followed by an all-gather of the finished shares.  And the hits are never indexed
// one by one: the batch's queries are LISTED grouped by owner, so what fg_probe_hits writes for one owner is one
// contiguous segment, and a segment is one copy.
#include "fg_ctx.h"
#include <array>
#include <chrono>

namespace {

typedef std::chrono::steady_clock Clock;
inline double secondsSince(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

u64 envCount(const char* name, u64 dflt)
{
	const char* v = getenv(name);
	return v && *v ? std::max<u64>(1, strtoull(v, nullptr, 10)) : dflt;
}

typedef struct fg_group_stats GroupStats;			// the plain names are the accessor functions
typedef struct fg_group_build_info GroupBuildInfo;

// what a member holds for the group: the staging buffer of the frequency sum and the receive buffer of the hits
struct MemberBufs {
	DevBuf<u32> stage;
	DevBuf<fg_seed_hit> recv;
};

} // namespace

struct fg_group {
	std::vector<fg_ctx*> m;
	std::vector<std::unique_ptr<MemberBufs>> bufs;
	std::string lastError;
	bool built = false;
	ShimPool pool;		// thread i works on member i and on nothing else
	struct fg_group_stats st{};
	struct fg_group_build_info bi{};
};

namespace {

// fn(i) for every member, each on its own thread (one member: on the caller's, ShimPool::run); the code of the first member that failed, its text in lastError
template <class F>
int onMembers(fg_group* g, F fn)
{
	const unsigned W = (unsigned)g->m.size();
	std::vector<int> rc(W, FG_OK);
	std::vector<std::string> msg(W);
	const std::function<void(unsigned)> job = [&](unsigned i)
	{
		fg_ctx* c = g->m[i];
		try
		{
			HIP_CHECK(hipSetDevice(c->device));
			rc[i] = fn(i);
			if (rc[i] != FG_OK) msg[i] = c->lastError;
		}
		catch (const FgError& e) { rc[i] = e.code; msg[i] = e.msg; }
		catch (const std::bad_alloc&) { rc[i] = FG_ERR_NOMEM; msg[i] = "host allocation failed"; }
		catch (const std::exception& e) { rc[i] = FG_ERR_HIP; msg[i] = e.what(); }
		// copies and launches this file put on the member's stream drain before anything they touch is reused
		if (rc[i] != FG_OK) (void)hipStreamSynchronize(c->stream);
	};
	g->pool.run(W, job);
	for (unsigned i = 0; i < W; ++i)
		if (rc[i] != FG_OK)
		{
			g->lastError = "member " + std::to_string(i) + " (device " + std::to_string(g->m[i]->device) + "): " +
				fg_strerror(rc[i]) + (msg[i].empty() ? "" : ": " + msg[i]);
			return rc[i];
		}
	return FG_OK;
}

// dist.balanced_bin_ranges: `world` contiguous bin ranges, cut where the running sum reaches r / world of the total.
// The same doubles in the same order as the numpy form (sums of integers below 2^53 are exact), so the cuts are the
// Python path's for the same histogram.
std::vector<u32> balancedCuts(const u64* hist, u32 world)
{
	std::vector<double> cs(FG_INDEX_BINS + 1, 0.0);
	for (u32 b = 0; b < FG_INDEX_BINS; ++b) cs[b + 1] = cs[b] + (double)hist[b];
	const double total = cs[FG_INDEX_BINS];
	std::vector<u32> cuts(1, 0);
	for (u32 r = 1; r < world; ++r)
	{
		const double target = total * (double)r / (double)world;
		const u32 c = (u32)(std::lower_bound(cs.begin(), cs.end(), target) - cs.begin());	// searchsorted(side = "left")
		cuts.push_back(std::min<u32>(FG_INDEX_BINS, std::max(cuts.back(), c)));
	}
	cuts.push_back(FG_INDEX_BINS);
	return cuts;
}

struct SolidArgs { i32 minFreq; float selectRate; i32 tandemFreq; float sampleRateInit; };
struct MinimizerArgs { i32 minCoverage, window; };

// The frequencies of one batch, summed over the members in place.  Member d owns the share [bnd[d], bnd[d + 1]) of
// the array: it takes that share of every other member's array through its staging buffer and adds it to its own
// (nobody writes a share it does not own, so no source changes under a copy); when every share is complete, every
// member copies the other members' shares over its own.  Both steps end host-synchronised: fg_index_batch_select
// reads the array on the library's stream next.
int sumFrequencies(fg_group* g, const std::vector<u32*>& freq, u64 n, u64 stageElems)
{
	const u32 W = (u32)g->m.size();
	std::vector<u64> bnd(W + 1, 0);
	for (u32 j = 1; j < W; ++j) bnd[j] = (n * j / W) & ~3ULL;		// shares start on 16 bytes: the kernel's vector path
	bnd[W] = n;
	std::vector<u64> pieces(W, 0), piecesMax(W, 0), moved(W, 0);
	int rc = onMembers(g, [&](unsigned d)
	{
		fg_ctx* c = g->m[d];
		const u64 lo = bnd[d], hi = bnd[d + 1];
		if (lo == hi) return (int)FG_OK;
		c->timer.reset();
		DevBuf<u32>& stage = g->bufs[d]->stage;
		const u64 cap = std::min(stageElems, hi - lo);
		if (stage.n < cap) stage.alloc(cap);
		for (u32 s = 0; s < W; ++s)
		{
			if (s == d) continue;
			u64 cnt = 0;
			for (u64 off = lo; off < hi; off += cap, ++cnt)
			{
				const u64 len = std::min(cap, hi - off);
				HIP_CHECK(hipMemcpyPeerAsync(stage.p, c->device, freq[s] + off, g->m[s]->device, len * 4, c->stream));
				fgFreqAccumulate(c, freq[d] + off, stage.p, len);
				moved[d] += len * 4;
			}
			pieces[d] += cnt; piecesMax[d] = std::max(piecesMax[d], cnt);
		}
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipStreamSynchronize(c->stream));
		c->timer.collect();		// the launches of this batch under one name, as after every step call
		return (int)FG_OK;
	});
	if (rc != FG_OK) return rc;
	rc = onMembers(g, [&](unsigned d)
	{
		fg_ctx* c = g->m[d];
		for (u32 s = 0; s < W; ++s)
		{
			if (s == d || bnd[s] == bnd[s + 1]) continue;
			const u64 len = bnd[s + 1] - bnd[s];
			HIP_CHECK(hipMemcpyPeerAsync(freq[d] + bnd[s], c->device, freq[s] + bnd[s], g->m[s]->device, len * 4, c->stream));
			moved[d] += len * 4;
		}
		HIP_CHECK(hipStreamSynchronize(c->stream));
		return (int)FG_OK;
	});
	for (u32 d = 0; d < W; ++d)
	{
		g->bi.stage_pieces += pieces[d];
		g->bi.stage_pieces_max = std::max<u32>(g->bi.stage_pieces_max, (u32)piecesMax[d]);
		g->bi.freq_bytes += moved[d];
	}
	return rc;
}

int buildSharded(fg_group* g, const SolidArgs* solid, const MinimizerArgs* mini, float repeatRate, fg_index_stats* out)
{
	const u32 W = (u32)g->m.size();
	const auto t0 = Clock::now();
	// 1. the key ranges, from a histogram that is the same on every member
	std::vector<std::vector<u64>> hist(W, std::vector<u64>(FG_INDEX_BINS, 0));
	int rc = onMembers(g, [&](unsigned i)
	{
		return solid ? fg_index_kmer_hist(g->m[i], hist[i].data())
					 : fg_index_begin_minimizers(g->m[i], mini->minCoverage, mini->window, repeatRate, hist[i].data());
	});
	if (rc != FG_OK) return rc;
	const std::vector<u32> cuts = balancedCuts(hist[0].data(), W);
	// 2. solid mode: counters of the own range, then the selection batch by batch on the summed frequencies
	std::vector<u64> distinct(W, 0);
	if (solid)
	{
		std::vector<u32> nBatches(W, 0);
		rc = onMembers(g, [&](unsigned i)
		{
			return fg_index_count_slice(g->m[i], solid->minFreq, solid->selectRate, solid->tandemFreq, repeatRate,
										solid->sampleRateInit, cuts[i], cuts[i + 1], &distinct[i], &nBatches[i]);
		});
		if (rc != FG_OK) return rc;
		const u64 stageElems = std::max<u64>(4, (envCount("FG_GROUP_STAGE_BYTES", 1ULL << 30) / 4) & ~3ULL);
		g->bi.selection_batches = nBatches[0];
		std::vector<u32*> freq(W, nullptr);
		std::vector<u64> nPos(W, 0);
		for (u32 b = 0; b < nBatches[0]; ++b)
		{
			rc = onMembers(g, [&](unsigned i) { return fg_index_batch_freq(g->m[i], b, &freq[i], &nPos[i]); });
			if (rc == FG_OK && nPos[0]) rc = sumFrequencies(g, freq, nPos[0], stageElems);
			if (rc == FG_OK) rc = onMembers(g, [&](unsigned i) { return fg_index_batch_select(g->m[i], b); });
			if (rc != FG_OK) return rc;
		}
		rc = onMembers(g, [&](unsigned i)
		{
			g->bufs[i]->stage.release();		// the sort of build_range gets the memory
			return fg_index_selection_done(g->m[i], nullptr);
		});
		if (rc != FG_OK) return rc;
	}
	// 3. every member sorts and encodes its range; filterFrequentKmers' two sums are taken over all of them
	std::vector<u64> sums(2 * (size_t)W, 0);
	rc = onMembers(g, [&](unsigned i) { return fg_index_build_range(g->m[i], cuts[i], cuts[i + 1], &sums[2 * (size_t)i]); });
	if (rc != FG_OK) return rc;
	u64 totalSums[2] = {0, 0}, totalDistinct = 0;
	for (u32 i = 0; i < W; ++i) { totalSums[0] += sums[2 * (size_t)i]; totalSums[1] += sums[2 * (size_t)i + 1]; totalDistinct += distinct[i]; }
	std::vector<fg_index_stats> pst(W);
	rc = onMembers(g, [&](unsigned i) { return fg_index_finish(g->m[i], totalSums, &pst[i]); });
	if (rc != FG_OK) return rc;
	// 4. pieces -> per-destination parts -> shards
	struct Piece { u64 nk = 0, ne = 0, nr = 0; const u64 *keys = nullptr, *rep = nullptr, *counts = nullptr, *ents = nullptr; std::vector<u64> totals; };
	std::vector<Piece> pc(W);
	rc = onMembers(g, [&](unsigned i)
	{
		Piece& p = pc[i];
		int r = fg_index_device_arrays(g->m[i], &p.nk, &p.ne, &p.nr, &p.keys, nullptr, nullptr, &p.rep);
		if (r != FG_OK) return r;
		p.totals.assign(W, 0);
		return fg_index_piece_split(g->m[i], W, &p.counts, &p.ents, p.totals.data());
	});
	if (rc != FG_OK) return rc;
	u64 K = 0, E = 0, R = 0;
	std::vector<u64> kb(W + 1, 0), rb(W + 1, 0);
	for (u32 s = 0; s < W; ++s)
	{
		K += pc[s].nk; E += pc[s].ne; R += pc[s].nr;
		kb[s + 1] = kb[s] + pc[s].nk; rb[s + 1] = rb[s] + pc[s].nr;
	}
	// getSampleRate() of the WHOLE index: the ctor value, or totalLen / totalEntries (vertex_index.cpp:480-482)
	float sampleRate = solid ? solid->sampleRateInit : 0.0f;
	if (!solid)
	{
		size_t totalLen = g->m[0]->totalBases, totalEntries = E;
		sampleRate = (float)totalLen / totalEntries;
	}
	// A member whose fg_index_scatter_begin fails frees its piece (fg_index.hip, clearIndex), and the pieces are what
	// the other members copy from: so every member allocates its shard in a pass of its own, and the copies start
	// only when all of them have.  From there on a failing member touches its own buffers alone until the join.
	std::vector<std::array<u64*, 4>> shard(W, std::array<u64*, 4>{{nullptr, nullptr, nullptr, nullptr}});
	rc = onMembers(g, [&](unsigned r)
	{
		u64 eShard = 0;
		for (u32 s = 0; s < W; ++s) eShard += pc[s].totals[r];
		return fg_index_scatter_begin(g->m[r], W, r, K, eShard, R, shard[r].data());
	});
	if (rc != FG_OK) return rc;
	std::vector<u64> moved(W, 0);
	rc = onMembers(g, [&](unsigned r)
	{
		fg_ctx* c = g->m[r];
		u64* const* full = shard[r].data();
		// sources in rank order = key order: keys, repetitive keys, the count rows into key_off, the entry segments
		u64 eAt = 0;
		for (u32 s = 0; s < W; ++s)
		{
			const Piece& p = pc[s];
			const int sd = g->m[s]->device;
			u64 segOff = 0;
			for (u32 d = 0; d < r; ++d) segOff += p.totals[d];
			const u64 seg = p.totals[r];
			if (p.nk) HIP_CHECK(hipMemcpyPeerAsync(full[0] + kb[s], c->device, p.keys, sd, p.nk * 8, c->stream));
			if (p.nr) HIP_CHECK(hipMemcpyPeerAsync(full[3] + rb[s], c->device, p.rep, sd, p.nr * 8, c->stream));
			if (p.nk) HIP_CHECK(hipMemcpyPeerAsync(full[1] + kb[s], c->device, p.counts + (u64)r * p.nk, sd, p.nk * 8, c->stream));
			if (seg) HIP_CHECK(hipMemcpyPeerAsync(full[2] + eAt, c->device, p.ents + segOff, sd, seg * 8, c->stream));
			if (s != r) moved[r] += 8 * (2 * p.nk + p.nr + seg);
			eAt += seg;
		}
		HIP_CHECK(hipStreamSynchronize(c->stream));
		return (int)FG_OK;
	});
	if (rc != FG_OK) return rc;
	// every shard is filled: the pieces may go
	rc = onMembers(g, [&](unsigned i) { return fg_index_scatter_end(g->m[i], sampleRate); });
	if (rc != FG_OK) return rc;
	for (u32 i = 0; i < W; ++i) g->bi.scatter_bytes += moved[i];
	// 5. the statistics of the whole index
	memset(out, 0, sizeof(*out));
	out->total_kmers = solid ? totalDistinct : 0;
	out->selected_kmers = K;
	out->index_entries = E;
	out->repetitive_kmers = R;
	out->repetitive_frequency = pst[0].repetitive_frequency;
	out->mean_frequency = pst[0].mean_frequency;
	out->sample_rate = sampleRate;
	out->build_seconds = secondsSince(t0);
	return FG_OK;
}

int buildIndex(fg_group* g, const SolidArgs* solid, const MinimizerArgs* mini, float repeatRate, fg_index_stats* out)
{
	g->built = false;
	g->bi = GroupBuildInfo{};
	int rc;
	if (g->m.size() == 1)
		rc = onMembers(g, [&](unsigned)
		{
			return solid ? fg_build_index_solid(g->m[0], solid->minFreq, solid->selectRate, solid->tandemFreq, repeatRate,
												solid->sampleRateInit, out)
						 : fg_build_index_minimizers(g->m[0], mini->minCoverage, mini->window, repeatRate, out);
		});
	else
		rc = buildSharded(g, solid, mini, repeatRate, out);
	if (rc != FG_OK)
	{
		// no member keeps half a build; the first error's text stays
		const std::string keep = g->lastError;
		(void)onMembers(g, [&](unsigned i) { g->bufs[i]->stage.release(); return fg_clear_index(g->m[i]); });
		g->lastError = keep;
		return rc;
	}
	g->built = true;
	return FG_OK;
}

// the partial results of a call, released whatever way the call ends
struct Partials {
	std::vector<fg_overlap_batch> v;
	~Partials() { for (auto& b : v) fg_release_batch(&b); }
};

int overlapsSharded(fg_group* g, const fg_detector_params* p, const u32* queryIds, u32 nq, i32 maxOverlaps,
					uint8_t forceLocal, fg_overlap_batch* out)
{
	const u32 W = (u32)g->m.size();
	const fg_ctx* c0 = g->m[0];
	const u32 base = c0->hasQ ? c0->qFirstId : c0->firstId;
	const u32 batchReads = (u32)std::min<u64>(envCount("FG_GROUP_BATCH_READS", 4096), 0x7fffffffULL);
	Partials parts;
	// where the caller's query i is: partial result and position in it
	std::vector<u32> partOf(nq), posIn(nq);
	std::vector<double> memberSeconds(W, 0.0);
	for (u32 b0 = 0; b0 < nq; b0 += batchReads)
	{
		const u32 nb = std::min(batchReads, nq - b0);
		// the batch listed grouped by owner, caller's order inside an owner
		std::vector<u32> start(W + 1, 0), grouped(nb), at(W);
		for (u32 i = 0; i < nb; ++i) ++start[((queryIds[b0 + i] - base) >> 1) % W + 1];
		for (u32 d = 0; d < W; ++d) start[d + 1] += start[d];
		for (u32 d = 0; d < W; ++d) at[d] = start[d];
		std::vector<u32> partIdx(W, 0);
		for (u32 d = 0; d < W; ++d)
			if (start[d + 1] > start[d]) { partIdx[d] = (u32)parts.v.size(); parts.v.push_back(fg_overlap_batch{}); }
		for (u32 i = 0; i < nb; ++i)
		{
			const u32 d = ((queryIds[b0 + i] - base) >> 1) % W;
			partOf[b0 + i] = partIdx[d]; posIn[b0 + i] = at[d] - start[d];
			grouped[at[d]++] = queryIds[b0 + i];
		}
		// every member probes the whole batch against its shard
		std::vector<std::vector<u64>> counts(W, std::vector<u64>(nb, 0));
		std::vector<const fg_seed_hit*> dHits(W, nullptr);
		std::vector<u64> nHits(W, 0);
		int rc = onMembers(g, [&](unsigned s)
		{
			int e = fg_probe_hits(g->m[s], grouped.data(), nb, counts[s].data(), &dHits[s], &nHits[s]);
			if (e == FG_OK) for (const auto& kt : g->m[s]->timer.last) memberSeconds[s] += kt.seconds;
			return e;
		});
		if (rc != FG_OK) return rc;
		// segOff[s][d]: where source s's hits for owner d begin
		std::vector<std::vector<u64>> segOff(W, std::vector<u64>(W + 1, 0));
		for (u32 s = 0; s < W; ++s)
			for (u32 d = 0; d < W; ++d)
			{
				u64 n = 0;
				for (u32 q = start[d]; q < start[d + 1]; ++q) n += counts[s][q];
				segOff[s][d + 1] = segOff[s][d] + n;
				g->st.hits_total += n;
				if (s != d) g->st.hits_moved_bytes += n * sizeof(fg_seed_hit);
			}
		// the owners collect their segments, sources in member order
		std::vector<double> copySeconds(W, 0.0);
		std::vector<u64> copies(W, 0);
		rc = onMembers(g, [&](unsigned d)
		{
			if (start[d + 1] == start[d]) return (int)FG_OK;
			fg_ctx* c = g->m[d];
			const auto t0 = Clock::now();
			u64 total = 0;
			for (u32 s = 0; s < W; ++s) total += segOff[s][d + 1] - segOff[s][d];
			DevBuf<fg_seed_hit>& recv = g->bufs[d]->recv;
			recv.reserve(total);
			u64 to = 0;
			for (u32 s = 0; s < W; ++s)
			{
				const u64 n = segOff[s][d + 1] - segOff[s][d];
				if (!n) continue;
				HIP_CHECK(hipMemcpyPeerAsync(recv.p + to, c->device, dHits[s] + segOff[s][d], g->m[s]->device,
											 n * sizeof(fg_seed_hit), c->stream));
				to += n; ++copies[d];
			}
			HIP_CHECK(hipStreamSynchronize(c->stream));
			copySeconds[d] = secondsSince(t0);
			return (int)FG_OK;
		});
		for (u32 d = 0; d < W; ++d) g->st.peer_copies += copies[d];
		g->st.exchange_seconds += *std::max_element(copySeconds.begin(), copySeconds.end());
		if (rc != FG_OK) return rc;
		// ... and compute their own queries (the hits of fg_probe_hits may go now: every copy has landed)
		rc = onMembers(g, [&](unsigned d)
		{
			const u32 nMine = start[d + 1] - start[d];
			if (!nMine) return (int)FG_OK;
			std::vector<u64> table((size_t)W * nMine);
			for (u32 s = 0; s < W; ++s)
				std::copy(counts[s].begin() + start[d], counts[s].begin() + start[d + 1], table.begin() + (size_t)s * nMine);
			fg_overlap_batch* res = &parts.v[partIdx[d]];
			int e = fg_overlaps_from_hits(g->m[d], p, grouped.data() + start[d], nMine, maxOverlaps, forceLocal, W,
										  table.data(), g->bufs[d]->recv.p, res);
			if (e == FG_OK) memberSeconds[d] += res->device_seconds;
			return e;
		});
		if (rc != FG_OK) return rc;
	}
	// one batch in the caller's query order
	const bool keepAln = p->keep_alignment != 0, partition = p->partition_bad_mappings != 0;
	u64 nRecs = 0, nStats = 0, nMatches = 0;
	for (const auto& r : parts.v) { nRecs += r.n_recs; nStats += r.n_div_stats; nMatches += r.n_matches; }
	BatchOwner* own = BatchOwner::acquire();
	out->owner_ = own;
	own->queryOff.assign((size_t)nq + 1, 0);
	own->statOff.assign((size_t)nq + 1, 0);
	own->reserveRecs(nRecs);
	own->nRecs = nRecs;
	own->stats.resize(nStats);
	if (partition) own->needsTrim.resize(nRecs);
	if (keepAln) { own->matchOff.assign(nRecs + 1, 0); own->reserveMatches(nMatches); }
	u64 rAt = 0, sAt = 0, mAt = 0;
	for (u32 i = 0; i < nq; ++i)
	{
		const fg_overlap_batch& r = parts.v[partOf[i]];
		const u32 t = posIn[i];
		const u64 a = r.query_off[t], b = r.query_off[t + 1], sa = r.div_stats_off[t], sb = r.div_stats_off[t + 1];
		own->queryOff[i] = rAt; own->statOff[i] = sAt;
		if (b > a) memcpy(own->recs + rAt, r.recs + a, (b - a) * sizeof(fg_overlap_rec));
		if (sb > sa) memcpy(own->stats.data() + sAt, r.div_stats + sa, (sb - sa) * sizeof(float));
		if (partition && b > a) memcpy(own->needsTrim.data() + rAt, r.needs_trim + a, b - a);
		if (keepAln)
		{
			const u64 ma = r.match_off[a], mb = r.match_off[b];
			for (u64 j = a; j < b; ++j) own->matchOff[rAt + (j - a)] = mAt + (r.match_off[j] - ma);
			if (mb > ma) memcpy(own->matches + 2 * mAt, r.matches + 2 * ma, (mb - ma) * 8);
			mAt += mb - ma;
		}
		rAt += b - a; sAt += sb - sa;
	}
	own->queryOff[nq] = rAt; own->statOff[nq] = sAt;
	if (keepAln) own->matchOff[nRecs] = mAt;
	out->n_queries = nq;
	out->n_recs = nRecs;
	out->query_off = own->queryOff.data();
	out->recs = own->recs;
	out->n_div_stats = nStats;
	out->div_stats_off = own->statOff.data();
	out->div_stats = own->stats.data();
	if (partition) out->needs_trim = own->needsTrim.data();
	if (keepAln) { out->n_matches = mAt; out->match_off = own->matchOff.data(); out->matches = own->matches; }
	// every query is counted by its owner alone (query_bp, query_kmers); the work counters add up over the owners
	for (const auto& r : parts.v)
	{
		out->query_bp += r.query_bp; out->query_kmers += r.query_kmers; out->seed_hits += r.seed_hits;
		out->dp_groups += r.dp_groups; out->dp_elements += r.dp_elements; out->dp_elements_small += r.dp_elements_small;
	}
	out->device_seconds = *std::max_element(memberSeconds.begin(), memberSeconds.end());
	return FG_OK;
}

} // namespace

extern "C" {

int fg_group_create(fg_group** out, const int* devices, uint32_t n_members, int kmer_size)
{
	if (!out) return FG_ERR_ARG;
	*out = nullptr;
	if (n_members == 0 || n_members > FG_SPLIT_MAX_WORLD || !devices) return FG_ERR_ARG;
	fg_group* g = new (std::nothrow) fg_group;
	if (!g) return FG_ERR_NOMEM;
	try
	{
		for (uint32_t i = 0; i < n_members; ++i)
		{
			fg_ctx* c = nullptr;
			const int rc = fg_create(&c, devices[i], kmer_size);
			if (rc != FG_OK) { fg_group_destroy(g); return rc; }
			g->m.push_back(c);
			g->bufs.emplace_back(new MemberBufs);
		}
	}
	catch (...) { fg_group_destroy(g); return FG_ERR_NOMEM; }
	*out = g;
	return FG_OK;
}

void fg_group_destroy(fg_group* g)
{
	if (!g) return;
	g->bufs.clear();
	for (fg_ctx* c : g->m) fg_destroy(c);
	delete g;
}

int fg_group_size(const fg_group* g, uint32_t* n_members)
{
	if (!g || !n_members) return FG_ERR_ARG;
	*n_members = (uint32_t)g->m.size();
	return FG_OK;
}

fg_ctx* fg_group_member(fg_group* g, uint32_t i) { return g && i < g->m.size() ? g->m[i] : nullptr; }

const char* fg_group_last_error(const fg_group* g) { return g ? g->lastError.c_str() : ""; }

int fg_group_set_reads(fg_group* g, uint32_t n_fwd, const uint64_t* words, const uint64_t* word_off, const int32_t* len,
					   uint32_t first_seq_id)
{
	if (!g) return FG_ERR_ARG;
	g->built = false;
	return onMembers(g, [&](unsigned i) { return fg_set_reads(g->m[i], n_fwd, words, word_off, len, first_seq_id); });
}

int fg_group_set_queries(fg_group* g, uint32_t n_fwd, const uint64_t* words, const uint64_t* word_off, const int32_t* len,
						 uint32_t first_seq_id)
{
	if (!g) return FG_ERR_ARG;
	return onMembers(g, [&](unsigned i) { return fg_set_queries(g->m[i], n_fwd, words, word_off, len, first_seq_id); });
}

int fg_group_build_index_solid(fg_group* g, int32_t min_freq, float select_rate, int32_t tandem_freq, float repeat_rate,
							   float sample_rate_init, struct fg_index_stats* out)
{
	if (!g || !out) return FG_ERR_ARG;
	if (!(select_rate >= 0.0f && select_rate < 1.0f)) return FG_ERR_ARG;
	const SolidArgs a{min_freq, select_rate, tandem_freq, sample_rate_init};
	return buildIndex(g, &a, nullptr, repeat_rate, out);
}

int fg_group_build_index_minimizers(fg_group* g, int32_t min_coverage, int32_t window, float repeat_rate,
									struct fg_index_stats* out)
{
	if (!g || !out) return FG_ERR_ARG;
	const MinimizerArgs a{min_coverage, window};
	return buildIndex(g, nullptr, &a, repeat_rate, out);
}

int fg_group_clear_index(fg_group* g)
{
	if (!g) return FG_ERR_ARG;
	g->built = false;
	return onMembers(g, [&](unsigned i) { g->bufs[i]->stage.release(); return fg_clear_index(g->m[i]); });
}

int fg_group_overlaps(fg_group* g, const struct fg_detector_params* p, const uint32_t* query_ids, uint32_t n_queries,
					  int32_t max_overlaps, uint8_t force_local, struct fg_overlap_batch* out)
{
	if (!g || !p || !out || (n_queries && !query_ids)) return FG_ERR_ARG;
	memset(out, 0, sizeof(*out));
	g->st = GroupStats{};
	if (!g->built) { g->lastError = "no index: call fg_group_build_index_solid / _minimizers first"; return FG_ERR_STATE; }
	if (g->m.size() == 1)
	{
		const int rc = onMembers(g, [&](unsigned) { return fg_overlaps(g->m[0], p, query_ids, n_queries, max_overlaps, force_local, out); });
		if (rc == FG_OK) g->st.hits_total = out->seed_hits;
		return rc;
	}
	const int chk = fgCheckOverlapArgs(g->m[0], p, query_ids, n_queries, max_overlaps);
	if (chk != FG_OK) { g->lastError = fg_strerror(chk); return chk; }
	int rc;
	try { rc = overlapsSharded(g, p, query_ids, n_queries, max_overlaps, force_local, out); }
	catch (const std::bad_alloc&) { g->lastError = "host allocation failed"; rc = FG_ERR_NOMEM; }
	catch (const std::exception& e) { g->lastError = e.what(); rc = FG_ERR_HIP; }
	if (rc != FG_OK)
	{
		BatchOwner::release((BatchOwner*)out->owner_);
		memset(out, 0, sizeof(*out));
	}
	return rc;
}

int fg_debug_group_bin_cuts(const uint64_t* hist, uint32_t world, uint32_t* cuts)
{
	if (!hist || !cuts || world == 0 || world > FG_SPLIT_MAX_WORLD) return FG_ERR_ARG;
	const std::vector<u32> c = balancedCuts(hist, world);
	std::copy(c.begin(), c.end(), cuts);
	return FG_OK;
}

int fg_group_stats(const fg_group* g, struct fg_group_stats* out)
{
	if (!g || !out) return FG_ERR_ARG;
	*out = g->st;
	return FG_OK;
}

int fg_group_build_info(const fg_group* g, struct fg_group_build_info* out)
{
	if (!g || !out) return FG_ERR_ARG;
	*out = g->bi;
	return FG_OK;
}

} // extern "C"
