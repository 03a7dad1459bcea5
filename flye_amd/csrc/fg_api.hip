// C ABI of libflyegpu.so (include/flye_gpu.h): context, read upload, index
// build/export entry points and the error boundary.  No exception leaves this
// file; there is no CPU fallback -- without a HIP device fg_create fails.
#include "fg_ctx.h"
#include "fg_stage.h"		// guarded
#include <chrono>
#include <cmath>

#include <algorithm>
#include <new>

#include <mutex>
#include <atomic>

static std::mutex g_poolMutex;
static std::vector<BatchOwner*> g_pool;

BatchOwner* BatchOwner::acquire()
{
	std::lock_guard<std::mutex> lock(g_poolMutex);
	if (g_pool.empty()) return new BatchOwner;
	BatchOwner* b = g_pool.back();
	g_pool.pop_back();
	return b;
}

void BatchOwner::release(BatchOwner* b)
{
	if (!b) return;
	std::lock_guard<std::mutex> lock(g_poolMutex);
	if (g_pool.size() < 2) { b->nRecs = 0; b->stats.clear(); g_pool.push_back(b); }
	else delete b;
}

namespace {

// Initialising the HIP runtime draws from libc's rand() stream (measured: tools/rand_stream_probe.py; only
// the first runtime initialisation of a process does).  The reference picks the reads of
// estimateOverlaperParameters with rand() (overlap.cpp:752-756, also sequence_container.cpp:318-328,
// chimera.cpp:76) and never seeds it, so a host program that creates a context first would see other
// picks.  While this guard lives the process draws from a private state array; the caller's stream
// continues exactly where it was (glibc keeps the position inside the state array it hands back).
// Only the FIRST fg_create of a process takes the guard (later ones initialise nothing that draws), and swapping
// glibc's process-wide state is not thread safe: that first call must come from a thread beside which no other
// thread uses rand() -- in Flye the main thread building the index (flye_gpu.h, fg_create).
struct RandStreamGuard {
	char buf[128];
	char* old = nullptr;
	RandStreamGuard()
	{
		static std::atomic<bool> firstDone{false};
		if (!firstDone.exchange(true)) old = initstate(1u, buf, sizeof(buf));
	}
	~RandStreamGuard() { if (old) setstate(old); }
};

} // namespace

extern "C" {

int fg_abi_version(void) { return FG_ABI_VERSION; }

const char* fg_strerror(int code)
{
	switch (code)
	{
	case FG_OK: return "ok";
	case FG_ERR_NO_DEVICE: return "no usable HIP device (this library has no CPU path)";
	case FG_ERR_HIP: return "HIP runtime error";
	case FG_ERR_ARG: return "invalid argument";
	case FG_ERR_STATE: return "invalid call order";
	case FG_ERR_KMER_TOO_FREQUENT: return "k-mer is too frequent";
	case FG_ERR_KMER_SIZE: return "unsupported k-mer size";
	case FG_ERR_UNSUPPORTED: return "flag combination not supported yet";
	case FG_ERR_NOMEM: return "out of memory";
	default: return "unknown error";
	}
}

const char* fg_last_error(const fg_ctx* ctx) { return ctx ? ctx->lastError.c_str() : fgHostError().c_str(); }

int fg_create(fg_ctx** out, int device, int kmer_size)
{
	if (!out) return FG_ERR_ARG;
	*out = nullptr;
	if (kmer_size < 1 || kmer_size > 32) return FG_ERR_KMER_SIZE;
	RandStreamGuard keepCallersRandStream;
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return FG_ERR_NO_DEVICE;
	if (device < 0 || device >= count) return FG_ERR_NO_DEVICE;
	if (hipSetDevice(device) != hipSuccess) return FG_ERR_NO_DEVICE;
	fg_ctx* c = new (std::nothrow) fg_ctx;
	if (!c) return FG_ERR_NOMEM;
	c->device = device;
	c->k = kmer_size;
	if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
		hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking) != hipSuccess ||
		hipStreamCreateWithFlags(&c->stream3, hipStreamNonBlocking) != hipSuccess ||
		hipEventCreateWithFlags(&c->evJoin3, hipEventDisableTiming) != hipSuccess ||
		hipEventCreateWithFlags(&c->evOff, hipEventDisableTiming) != hipSuccess ||
		hipEventCreateWithFlags(&c->evFork, hipEventDisableTiming) != hipSuccess ||
		hipEventCreateWithFlags(&c->evJoin, hipEventDisableTiming) != hipSuccess)
	{
		delete c;
		return FG_ERR_NO_DEVICE;
	}
	for (auto& e : c->evPiece)
		if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { delete c; return FG_ERR_NO_DEVICE; }
	c->timer.stream = c->stream;
	*out = c;
	return FG_OK;
}

void fg_destroy(fg_ctx* ctx)
{
	if (!ctx) return;
	(void)hipSetDevice(ctx->device);
	(void)hipStreamSynchronize(ctx->stream);
	delete ctx;
}

int fg_container_info(const fg_ctx* c, uint32_t* first_id, uint32_t* n_fwd, uint32_t* query_first_id, uint32_t* query_n_fwd)
{
	if (!c) return FG_ERR_ARG;
	if (first_id) *first_id = c->firstId;
	if (n_fwd) *n_fwd = c->nReads;
	if (query_first_id) *query_first_id = c->hasQ ? c->qFirstId : 0;
	if (query_n_fwd) *query_n_fwd = c->hasQ ? c->nQReads : 0;
	return FG_OK;
}

int fg_set_reads(fg_ctx* c, uint32_t n, const uint64_t* words, const uint64_t* word_off,
				 const int32_t* len, uint32_t first_seq_id)
{
	if (!c || (n && (!words || !word_off || !len))) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		if ((u64)first_seq_id + 2ULL * n > 0xFFFFFFFFULL) throw FgError{FG_ERR_ARG, "sequence ids overflow uint32"};
		c->indexBuilt = false;
		c->dMaybeBits.release();	// they number the positions of the reads that leave
		c->hasQ = false; c->nQReads = 0; c->hQLen.clear();
		c->nReads = n;
		c->firstId = first_seq_id;
		c->totalWords = n ? word_off[n] : 0;
		c->hLen.assign(len, len + n);
		c->hKmerOff.assign(n + 1, 0);
		c->totalBases = 0;
		c->maxLen = 0;
		for (u32 i = 0; i < n; ++i)
		{
			if (len[i] < 0) throw FgError{FG_ERR_ARG, "negative read length"};
			if ((u64)(len[i] + 31) / 32 > word_off[i + 1] - word_off[i])
				throw FgError{FG_ERR_ARG, "word_off does not cover read " + std::to_string(i)};
			c->hKmerOff[i + 1] = c->hKmerOff[i] + (u64)std::max(0, len[i] - c->k);
			c->totalBases += len[i];
			c->maxLen = std::max(c->maxLen, len[i]);
		}
		c->totalKmers = c->hKmerOff[n];
		c->dWords.alloc(c->totalWords + 2);
		c->dWordOff.alloc(n + 1);
		c->dLen.alloc(n);
		c->dKmerOff.alloc(n + 1);
		hipStream_t s = c->stream;
		HIP_CHECK(hipMemsetAsync(c->dWords.p + c->totalWords, 0, 16, s));
		if (n)
		{
			HIP_CHECK(hipMemcpyAsync(c->dWords.p, words, c->totalWords * 8, hipMemcpyHostToDevice, s));
			HIP_CHECK(hipMemcpyAsync(c->dWordOff.p, word_off, (n + 1) * 8ULL, hipMemcpyHostToDevice, s));
			HIP_CHECK(hipMemcpyAsync(c->dLen.p, len, n * 4ULL, hipMemcpyHostToDevice, s));
		}
		HIP_CHECK(hipMemcpyAsync(c->dKmerOff.p, c->hKmerOff.data(), (n + 1) * 8ULL, hipMemcpyHostToDevice, s));
		HIP_CHECK(hipStreamSynchronize(s));
	});
}

int fg_set_queries(fg_ctx* c, uint32_t n, const uint64_t* words, const uint64_t* word_off,
				   const int32_t* len, uint32_t first_seq_id)
{
	if (!c || (n && (!words || !word_off || !len))) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		c->hasQ = n > 0;
		c->nQReads = n; c->qFirstId = first_seq_id; c->qMaxLen = 0;
		c->hQLen.clear();
		if (!n) { c->dQWords.release(); c->dQWordOff.release(); c->dQLen.release(); return; }
		if ((u64)first_seq_id + 2ULL * n > 0xFFFFFFFFULL) throw FgError{FG_ERR_ARG, "sequence ids overflow uint32"};
		// the reference hands out ids from one process-wide counter: the two containers never share ids
		const u64 a0 = c->firstId, a1 = (u64)c->firstId + 2ULL * c->nReads, b0 = first_seq_id, b1 = (u64)first_seq_id + 2ULL * n;
		if (a0 < b1 && b0 < a1) throw FgError{FG_ERR_ARG, "query ids overlap the ids of the indexed container"};
		c->hQLen.assign(len, len + n);
		for (u32 i = 0; i < n; ++i)
		{
			if (len[i] < 0) throw FgError{FG_ERR_ARG, "negative read length"};
			if ((u64)(len[i] + 31) / 32 > word_off[i + 1] - word_off[i])
				throw FgError{FG_ERR_ARG, "word_off does not cover query " + std::to_string(i)};
			c->qMaxLen = std::max(c->qMaxLen, len[i]);
		}
		const u64 nw = word_off[n];
		c->dQWords.alloc(nw + 2); c->dQWordOff.alloc(n + 1); c->dQLen.alloc(n);
		hipStream_t s = c->stream;
		HIP_CHECK(hipMemsetAsync(c->dQWords.p + nw, 0, 16, s));
		HIP_CHECK(hipMemcpyAsync(c->dQWords.p, words, nw * 8, hipMemcpyHostToDevice, s));
		HIP_CHECK(hipMemcpyAsync(c->dQWordOff.p, word_off, (n + 1) * 8ULL, hipMemcpyHostToDevice, s));
		HIP_CHECK(hipMemcpyAsync(c->dQLen.p, len, n * 4ULL, hipMemcpyHostToDevice, s));
		HIP_CHECK(hipStreamSynchronize(s));
	});
}

int fg_build_index_solid(fg_ctx* c, int32_t min_freq, float select_rate, int32_t tandem_freq,
						 float repeat_rate, float sample_rate_init, struct fg_index_stats* out)
{
	if (!c || !out) return FG_ERR_ARG;
	if (!(select_rate >= 0.0f && select_rate < 1.0f)) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgBuildIndexSolid(c, min_freq, select_rate, tandem_freq, repeat_rate, sample_rate_init, out);
	});
}

int fg_build_index_minimizers(fg_ctx* c, int32_t min_coverage, int32_t window, float repeat_rate,
							  struct fg_index_stats* out)
{
	if (!c || !out) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgBuildIndexMinimizers(c, min_coverage, window, repeat_rate, out);
	});
}

int fg_index_begin_solid(fg_ctx* c, int32_t min_freq, float select_rate, int32_t tandem_freq, float repeat_rate,
						 float sample_rate_init, uint64_t* hist)
{
	if (!c) return FG_ERR_ARG;
	if (!(select_rate >= 0.0f && select_rate < 1.0f)) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgIndexBeginSolid(c, min_freq, select_rate, tandem_freq, repeat_rate, sample_rate_init, hist);
	});
}

int fg_index_begin_minimizers(fg_ctx* c, int32_t min_coverage, int32_t window, float repeat_rate, uint64_t* hist)
{
	if (!c) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgIndexBeginMinimizers(c, min_coverage, window, repeat_rate, hist);
	});
}

int fg_index_build_range(fg_ctx* c, uint32_t bin_lo, uint32_t bin_hi, uint64_t* sums)
{
	if (!c) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		unsigned long long s2[2];
		fgIndexBuildRange(c, bin_lo, bin_hi, s2);
		if (sums) { sums[0] = s2[0]; sums[1] = s2[1]; }
	});
}

int fg_index_finish(fg_ctx* c, const uint64_t* total_sums, struct fg_index_stats* out)
{
	if (!c || !out) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		unsigned long long s2[2] = {0, 0};
		if (total_sums) { s2[0] = total_sums[0]; s2[1] = total_sums[1]; }
		fgIndexFinish(c, total_sums ? s2 : nullptr, out);
	});
}

int fg_index_kmer_hist(fg_ctx* c, uint64_t* hist)
{
	if (!c || !hist) return FG_ERR_ARG;
	return guarded(c, [&]() { HIP_CHECK(hipSetDevice(c->device)); fgIndexKmerHist(c, hist); });
}

int fg_index_count_slice(fg_ctx* c, int32_t min_freq, float select_rate, int32_t tandem_freq, float repeat_rate,
						 float sample_rate_init, uint32_t bin_lo, uint32_t bin_hi, uint64_t* distinct, uint32_t* n_batches)
{
	if (!c) return FG_ERR_ARG;
	if (!(select_rate >= 0.0f && select_rate < 1.0f)) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgIndexCountSlice(c, min_freq, select_rate, tandem_freq, repeat_rate, sample_rate_init, bin_lo, bin_hi, distinct, n_batches);
	});
}

int fg_index_batch_freq(fg_ctx* c, uint32_t batch, uint32_t** d_freq, uint64_t* n)
{
	if (!c) return FG_ERR_ARG;
	return guarded(c, [&]() { HIP_CHECK(hipSetDevice(c->device)); fgIndexBatchFreq(c, batch, d_freq, n); });
}

int fg_index_batch_select(fg_ctx* c, uint32_t batch)
{
	if (!c) return FG_ERR_ARG;
	return guarded(c, [&]() { HIP_CHECK(hipSetDevice(c->device)); fgIndexBatchSelect(c, batch); });
}

int fg_index_selection_done(fg_ctx* c, uint64_t* hist)
{
	if (!c) return FG_ERR_ARG;
	return guarded(c, [&]() { HIP_CHECK(hipSetDevice(c->device)); fgIndexSelectionDone(c, hist); });
}

int fg_index_gather_begin(fg_ctx* c, uint64_t n_keys, uint64_t n_entries, uint64_t n_repetitive, uint64_t** full,
						  uint64_t** piece, uint64_t* piece_sizes)
{
	if (!c || !full || !piece || !piece_sizes) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgIndexGatherBegin(c, n_keys, n_entries, n_repetitive, (u64**)full, (u64**)piece, (u64*)piece_sizes);
	});
}

int fg_index_gather_end(fg_ctx* c, float sample_rate)
{
	if (!c) return FG_ERR_ARG;
	return guarded(c, [&]() { HIP_CHECK(hipSetDevice(c->device)); fgIndexGatherEnd(c, sample_rate); });
}

int fg_memory_stats(uint64_t* bytes_now, uint64_t* bytes_peak, int reset_peak)
{
	if (bytes_now) *bytes_now = g_fgDevBytes.load();
	if (bytes_peak) *bytes_peak = g_fgDevPeak.load();
	if (reset_peak) g_fgDevPeak.store(g_fgDevBytes.load());
	return FG_OK;
}

int fg_import_index(fg_ctx* c, uint64_t n_keys, const uint64_t* keys, const uint64_t* key_off, uint64_t n_entries,
					const uint64_t* entries, uint64_t n_repetitive, const uint64_t* repetitive_keys, float sample_rate,
					int on_device)
{
	if (!c || !key_off || (n_keys && !keys) || (n_entries && !entries) || (n_repetitive && !repetitive_keys)) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgImportIndex(c, n_keys, keys, key_off, n_entries, entries, n_repetitive, repetitive_keys, sample_rate, on_device);
	});
}

int fg_index_device_arrays(fg_ctx* c, uint64_t* n_keys, uint64_t* n_entries, uint64_t* n_repetitive,
						   const uint64_t** keys, const uint64_t** key_off, const uint64_t** entries,
						   const uint64_t** repetitive_keys)
{
	if (!c) return FG_ERR_ARG;
	if (!c->indexBuilt) return FG_ERR_STATE;
	if (n_keys) *n_keys = c->nKeys;
	if (n_entries) *n_entries = c->nEntries;
	if (n_repetitive) *n_repetitive = c->nRep;
	if (keys) *keys = c->dKeys.p;
	if (key_off) *key_off = c->dKeyOff.p;
	if (entries) *entries = c->dEntries.p;
	if (repetitive_keys) *repetitive_keys = c->dRepKeys.p;
	return FG_OK;
}

int fg_clear_index(fg_ctx* c)
{
	if (!c) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		c->indexBuilt = false;
		c->indexBuild.reset();
		c->gathering = false;
		c->scattering = false;
		c->splitWorld = 0;
		c->sCounts.release(); c->sEntries.release();
		c->shardWorld = 1; c->shardRank = 0;
		c->gKeys.release(); c->gKeyOff.release(); c->gEntries.release(); c->gRepKeys.release();
		c->dKeys.release(); c->dKeyOff.release(); c->dEntries.release(); c->dRepKeys.release();
		c->dTable.release(); c->dIndexedBits.release(); c->dMaybeBits.release();
		c->nKeys = c->nEntries = c->nRep = c->tableSlots = 0;
	});
}

int fg_export_index(fg_ctx* c, uint64_t* n_keys, uint64_t* n_entries, uint64_t* n_repetitive,
					uint64_t* keys, uint64_t* key_off, uint64_t* entries, uint64_t* repetitive_keys)
{
	if (!c || !n_keys || !n_entries || !n_repetitive) return FG_ERR_ARG;
	if (!c->indexBuilt) return FG_ERR_STATE;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		*n_keys = c->nKeys; *n_entries = c->nEntries; *n_repetitive = c->nRep;
		hipStream_t s = c->stream;
		if (keys && c->nKeys) HIP_CHECK(hipMemcpyAsync(keys, c->dKeys.p, c->nKeys * 8, hipMemcpyDeviceToHost, s));
		if (key_off) HIP_CHECK(hipMemcpyAsync(key_off, c->dKeyOff.p, (c->nKeys + 1) * 8, hipMemcpyDeviceToHost, s));
		if (entries && c->nEntries) HIP_CHECK(hipMemcpyAsync(entries, c->dEntries.p, c->nEntries * 8, hipMemcpyDeviceToHost, s));
		if (repetitive_keys && c->nRep) HIP_CHECK(hipMemcpyAsync(repetitive_keys, c->dRepKeys.p, c->nRep * 8, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
	});
}

} // extern "C"

int fgCheckOverlapArgs(const fg_ctx* c, const fg_detector_params* p, const u32* query_ids, u32 n_queries, i32 max_overlaps)
{
	if (p->partition_bad_mappings && max_overlaps != 0) return FG_ERR_UNSUPPORTED;
	if (p->max_jump <= 0 || p->min_overlap <= 0 || max_overlaps < 0) return FG_ERR_ARG;
	const u32 base = c->hasQ ? c->qFirstId : c->firstId;
	const u32 cnt = c->hasQ ? c->nQReads : c->nReads;
	for (u32 i = 0; i < n_queries; ++i)
		if (query_ids[i] < base || query_ids[i] - base >= 2 * cnt) return FG_ERR_ARG;
	return FG_OK;
}

extern "C" {

int fg_index_keep_targets(fg_ctx* c, uint32_t world, uint32_t rank, uint64_t* n_entries_kept)
{
	if (!c) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		u64 kept = 0;
		fgIndexKeepTargets(c, world, rank, &kept);
		if (n_entries_kept) *n_entries_kept = kept;
	});
}

int fg_index_shard(const fg_ctx* c, uint32_t* world, uint32_t* rank)
{
	if (!c) return FG_ERR_ARG;
	if (world) *world = c->shardWorld;
	if (rank) *rank = c->shardRank;
	return FG_OK;
}

int fg_index_piece_split(fg_ctx* c, uint32_t world, const uint64_t** d_counts, const uint64_t** d_entries,
						 uint64_t* dest_totals)
{
	if (!c || !d_counts || !d_entries || !dest_totals) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgIndexPieceSplit(c, world, (const u64**)d_counts, (const u64**)d_entries, (u64*)dest_totals);
	});
}

int fg_index_scatter_begin(fg_ctx* c, uint32_t world, uint32_t rank, uint64_t n_keys, uint64_t n_shard_entries,
						   uint64_t n_repetitive, uint64_t** full)
{
	if (!c || !full) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgIndexScatterBegin(c, world, rank, n_keys, n_shard_entries, n_repetitive, (u64**)full);
	});
}

int fg_index_scatter_end(fg_ctx* c, float sample_rate)
{
	if (!c) return FG_ERR_ARG;
	return guarded(c, [&]() { HIP_CHECK(hipSetDevice(c->device)); fgIndexScatterEnd(c, sample_rate); });
}

int fg_probe_hits(fg_ctx* c,const uint32_t* query_ids, uint32_t n_queries, uint64_t* hit_counts,
				  const struct fg_seed_hit** d_hits, uint64_t* n_hits)
{
	if (!c || !d_hits || !n_hits || (n_queries && (!query_ids || !hit_counts))) return FG_ERR_ARG;
	*d_hits = nullptr; *n_hits = 0;
	if (!c->indexBuilt) return FG_ERR_STATE;
	{
		const u32 base = c->hasQ ? c->qFirstId : c->firstId;
		const u32 cnt = c->hasQ ? c->nQReads : c->nReads;
		for (u32 i = 0; i < n_queries; ++i)
			if (query_ids[i] < base || query_ids[i] - base >= 2 * cnt) return FG_ERR_ARG;
	}
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgProbeHits(c, query_ids, n_queries, (u64*)hit_counts, d_hits, (u64*)n_hits);
	});
}

int fg_overlaps_from_hits(fg_ctx* c, const struct fg_detector_params* p, const uint32_t* query_ids, uint32_t n_queries,
						  int32_t max_overlaps, uint8_t force_local, uint32_t n_src, const uint64_t* hit_counts,
						  const struct fg_seed_hit* d_hits, struct fg_overlap_batch* out)
{
	if (!c || !p || !out || (n_queries && !query_ids) || n_src == 0 || (n_queries && !hit_counts)) return FG_ERR_ARG;
	memset(out, 0, sizeof(*out));
	if (!c->indexBuilt) return FG_ERR_STATE;
	const int chk = fgCheckOverlapArgs(c, p, query_ids, n_queries, max_overlaps);
	if (chk != FG_OK) return chk;
	const int rc = guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgOverlapsFromHits(c, p, query_ids, n_queries, max_overlaps, force_local, n_src, (const u64*)hit_counts, d_hits, out);
	});
	if (rc != FG_OK)
	{
		BatchOwner::release((BatchOwner*)out->owner_);
		memset(out, 0, sizeof(*out));
	}
	return rc;
}

int fg_overlaps(fg_ctx* c, const struct fg_detector_params* p, const uint32_t* query_ids,
				uint32_t n_queries, int32_t max_overlaps, uint8_t force_local,
				struct fg_overlap_batch* out)
{
	if (!c || !p || !out || (n_queries && !query_ids)) return FG_ERR_ARG;
	memset(out, 0, sizeof(*out));
	if (!c->indexBuilt) return FG_ERR_STATE;
	if (c->shardWorld != 1)
	{
		c->lastError = "the index holds the entries of 1/" + std::to_string(c->shardWorld) + " of the target reads "
			"(fg_index_keep_targets): collect seed hits with fg_probe_hits and compute overlaps with fg_overlaps_from_hits";
		return FG_ERR_STATE;
	}
	const int chk = fgCheckOverlapArgs(c, p, query_ids, n_queries, max_overlaps);
	if (chk != FG_OK) return chk;
	const int rc = guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgOverlaps(c, p, query_ids, n_queries, max_overlaps, force_local, out);
	});
	if (rc != FG_OK)
	{
		BatchOwner::release((BatchOwner*)out->owner_);
		memset(out, 0, sizeof(*out));
	}
	return rc;
}

int fg_debug_sort_pairs(fg_ctx* c, uint64_t* keys, uint32_t* vals, const uint64_t* seg_off, uint32_t n_seg)
{
	if (!c || !seg_off || (seg_off[n_seg] && (!keys || !vals))) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgDebugSortPairs(c, keys, vals, seg_off, n_seg);
	});
}

int fg_debug_sort_pairs64(fg_ctx* c, uint64_t* keys, uint32_t* vals, const uint64_t* seg_off, uint32_t n_seg, int cur_bits)
{
	if (!c || !seg_off || (seg_off[n_seg] && (!keys || !vals)) || cur_bits < 0 || cur_bits > 32) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgDebugSortPairs(c, keys, vals, seg_off, n_seg, cur_bits);
	});
}

int fg_debug_sort_packed(fg_ctx* c, uint64_t* recs, const uint64_t* seg_off, uint32_t n_seg, int cur_bits)
{
	if (!c || !seg_off || (seg_off[n_seg] && !recs) || cur_bits < 0 || cur_bits + FG_PK_VALBITS >= 64) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgDebugSortPacked(c, recs, seg_off, n_seg, cur_bits);
	});
}

int fg_debug_sort_pairs32(fg_ctx* c, uint32_t* keys, uint32_t* vals, const uint64_t* seg_off, uint32_t n_seg, int cur_bits,
						  int rec_bits, const uint32_t* tie_free, uint64_t* radix_segments, uint64_t* radix_hits)
{
	if (!c || !seg_off || !radix_segments || !radix_hits || (seg_off[n_seg] && (!keys || !vals)) || cur_bits < 0 || rec_bits < 0 ||
		cur_bits + rec_bits > 32)
		return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgDebugSortPairs32(c, keys, vals, seg_off, n_seg, cur_bits, rec_bits, tie_free, radix_segments, radix_hits);
	});
}

int fg_debug_sort_pairs32_val16(fg_ctx* c, uint32_t* keys, uint16_t* vals, const uint64_t* seg_off, uint32_t n_seg, int cur_bits,
								int rec_bits, const uint32_t* tie_free, uint64_t* radix_segments, uint64_t* radix_hits)
{
	if (!c || !seg_off || !radix_segments || !radix_hits || (seg_off[n_seg] && (!keys || !vals)) || cur_bits < 0 || rec_bits < 0 ||
		cur_bits + rec_bits > 32)
		return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgDebugSortPairs32v16(c, keys, vals, seg_off, n_seg, cur_bits, rec_bits, tie_free, radix_segments, radix_hits);
	});
}

int fg_debug_hit_val16(fg_ctx* c, uint32_t* val16)
{
	if (!c || !val16) return FG_ERR_ARG;
	*val16 = c->hitVal16 ? 1u : 0u;
	return FG_OK;
}

int fg_debug_tie_free(fg_ctx* c, uint32_t* out, uint32_t max_n, uint32_t* first_query, uint32_t* n)
{
	if (!c || !first_query || !n || (max_n && !out)) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgDebugTieFree(c, out, max_n, first_query, n);
	});
}

int fg_debug_sort_screen(fg_ctx* c, const uint32_t* keys, const uint64_t* seg_off, uint32_t n_seg, int cur_bits, int rec_bits,
						 const uint32_t* tie_free, float min_unique, int32_t min_overlap, uint32_t* out_reason)
{
	if (!c || !seg_off || (n_seg && (!tie_free || !out_reason)) || (seg_off[n_seg] && !keys) || cur_bits < 0 || rec_bits < 0 ||
		cur_bits + rec_bits > 32)
		return FG_ERR_ARG;
	for (uint32_t i = 0; i < n_seg; ++i)
		if (seg_off[i] > seg_off[i + 1]) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgDebugSortScreen(c, keys, seg_off, n_seg, cur_bits, rec_bits, tie_free, min_unique, min_overlap, out_reason);
	});
}

int fg_debug_order_free(fg_ctx* c, uint32_t* out_reason, uint32_t max_n, uint32_t* first_query, uint32_t* n)
{
	if (!c || !first_query || !n || (max_n && !out_reason)) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgDebugOrderFree(c, out_reason, max_n, first_query, n);
	});
}

int fg_debug_sort_radix_segments(fg_ctx* c, uint32_t* segments)
{
	if (!c || !segments) return FG_ERR_ARG;
	*segments = c->sortRadixSegs;
	return FG_OK;
}

int fg_debug_freq_accumulate(fg_ctx* c, uint32_t* dst, const uint32_t* src, uint64_t n)
{
	if (!c || (n && (!dst || !src)) || ((uintptr_t)dst & 3u) || ((uintptr_t)src & 3u)) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgDebugFreqAccumulate(c, dst, src, n);
	});
}

int fg_debug_scan(fg_ctx* c, void* data, uint64_t n, int elem_bytes, int inclusive, int in_place)
{
	if (!c || (n && !data) || (elem_bytes != 4 && elem_bytes != 8) || ((uintptr_t)data & (uintptr_t)(elem_bytes - 1)) ||
		n > (1ULL << 40))
		return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgDebugScan(c, data, n, elem_bytes, inclusive != 0, in_place != 0);
	});
}

int fg_debug_radix_sort_pairs(fg_ctx* c, uint64_t* keys, uint64_t* vals, uint64_t n, int begin_bit, int end_bit,
							  int* passes_run)
{
	if (!c || (n && (!keys || !vals)) || begin_bit < 0 || end_bit > 64 || begin_bit > end_bit || n > (1ULL << 30) - 1 ||
		((uintptr_t)keys & 7u) || ((uintptr_t)vals & 7u))
		return FG_ERR_ARG;
	if (passes_run) *passes_run = 0;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgDebugRadixSortPairs(c, keys, vals, n, begin_bit, end_bit, passes_run);
	});
}

int fg_debug_probe_skip_check(fg_ctx* c, uint64_t* clear_bits, uint64_t* violations)
{
	if (!c || !clear_bits || !violations) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		if (!c->indexBuilt) throw FgError{FG_ERR_STATE, "no index"};
		u64 cb = 0, vi = 0;
		fgDebugProbeSkipCheck(c, &cb, &vi);
		*clear_bits = cb; *violations = vi;
	});
}

int fg_debug_table(fg_ctx* c, uint32_t* wide, uint32_t* n_parts, uint64_t* n_slots, uint64_t* bound, uint64_t* slot_base,
				   uint64_t* key_base, uint32_t* groups, uint64_t* slots)
{
	if (!c) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		if (!c->indexBuilt) throw FgError{FG_ERR_STATE, "no index"};
		const FgTable& T = c->table;
		if (wide) *wide = c->tableWide ? 1u : 0u;
		if (n_parts) *n_parts = T.nParts;
		if (n_slots) *n_slots = c->tableSlots;
		for (u32 p = 0; p < T.nParts; ++p)
		{
			if (bound) bound[p] = T.bound[p];
			if (slot_base) slot_base[p] = T.slotBase[p];
			if (key_base) key_base[p] = T.keyBase[p];
			if (groups) groups[p] = T.groups[p];
		}
		if (bound) bound[T.nParts] = T.bound[T.nParts];
		if (slots && c->tableSlots)
		{
			HIP_CHECK(hipMemcpyAsync(slots, c->dTable.p, c->tableSlots * (c->tableWide ? 16 : 8), hipMemcpyDeviceToHost, c->stream));
			HIP_CHECK(hipStreamSynchronize(c->stream));
		}
	});
}

int fg_debug_chain_lazy(fg_ctx* c, uint64_t out[6])
{
	if (!c || !out) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		u64 h[6];
		fgDebugChainLazy(c, h);
		for (int i = 0; i < 6; ++i) out[i] = h[i];
	});
}

int fg_debug_edit_distances(fg_ctx* c, uint32_t n_pairs, int use_hpc, int32_t* out_dist, int32_t* out_len_a,
							int32_t* out_len_b)
{
	if (!c || (n_pairs && (!out_dist || !out_len_a || !out_len_b))) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		fgDebugEditDistances(c, n_pairs, use_hpc, out_dist, out_len_a, out_len_b);
	});
}

namespace {
struct CigarOwner {
	std::vector<uint64_t> runOff;
	std::vector<uint8_t> ops;
	std::vector<int32_t> lens;
	std::vector<float> err;
};
}

int fg_align_cigar_ksw(fg_ctx* c, uint32_t n_pairs, const uint8_t* trg, const uint64_t* trg_off, const uint8_t* qry,
					   const uint64_t* qry_off, struct fg_cigar_batch* out)
{
	if (!c || !out || !trg_off || !qry_off || (trg_off[n_pairs] && !trg) || (qry_off[n_pairs] && !qry)) return FG_ERR_ARG;
	memset(out, 0, sizeof(*out));
	CigarOwner* own = nullptr;
	const int rc = guarded(c, [&]()
	{
		HIP_CHECK(hipSetDevice(c->device));
		std::vector<u64> runOff;
		std::vector<u32> runs;
		fgKswAlign(c, n_pairs, trg, trg_off, qry, qry_off, runOff, runs);
		const auto tDec = std::chrono::steady_clock::now();
		own = new CigarOwner;
		own->runOff.assign(n_pairs + 1, 0);
		own->err.assign(n_pairs, 0.0f);
		// the decoding loop of alignment.cpp:172-211, on the host: M runs split into '=' / 'X'.  Pairs are
		// independent: slices of the batch (cut by bases) go to the context's worker threads.
		u64 totalBp = 0;
		for (u32 i = 0; i < n_pairs; ++i) totalBp += (trg_off[i + 1] - trg_off[i]) + (qry_off[i + 1] - qry_off[i]);
		unsigned nThreads = totalBp < (1u << 20) ? 1u : std::max(1u, std::min(fg_usable_cpus(), 32u));
		if (getenv("FG_SHIM_THREADS")) nThreads = std::max(1, atoi(getenv("FG_SHIM_THREADS")));
		std::vector<u32> cut(nThreads + 1, n_pairs);
		cut[0] = 0;
		{
			u64 acc = 0; unsigned t = 1;
			for (u32 i = 0; i < n_pairs && t < nThreads; ++i)
			{
				acc += (trg_off[i + 1] - trg_off[i]) + (qry_off[i + 1] - qry_off[i]);
				while (t < nThreads && acc >= totalBp * t / nThreads) cut[t++] = i + 1;
			}
		}
		std::vector<std::vector<uint8_t>> tOps(nThreads);
		std::vector<std::vector<int32_t>> tLens(nThreads);
		std::atomic<int> workerFailed{0};		// no exception may leave a pool thread
		c->shimPool.run(nThreads, [&](unsigned th)
		{
		  try
		  {
			// thread-local vectors (the headers of tOps[] sit next to each other: appending through them would
			// bounce one cache line between all threads), handed over at the end
			std::vector<uint8_t> ops;
			std::vector<int32_t> lens;
			for (u32 i = cut[th]; i < cut[th + 1]; ++i)
			{
				const uint8_t* t = trg + trg_off[i];
				const uint8_t* q = qry + qry_off[i];
				const size_t trgLen = trg_off[i + 1] - trg_off[i], qryLen = qry_off[i + 1] - qry_off[i];
				size_t posQry = 0, posTrg = 0;
				int numMiss = 0, numIndels = 0;
				const size_t first = ops.size();
				for (u64 k = runOff[i]; k < runOff[i + 1]; ++k)
				{
					const int size = (int)(runs[k] >> 4);
					const u32 op = runs[k] & 0xf;
					if (op == 0)
					{
						for (int x = 0; x < size; ++x)
						{
							const char match = t[posTrg + x] == q[posQry + x] ? '=' : 'X';
							if (x == 0 || match != (char)ops.back()) { ops.push_back((uint8_t)match); lens.push_back(1); }
							else ++lens.back();
							numMiss += match == 'X';
						}
						posQry += size; posTrg += size;
					}
					else if (op == 1) { ops.push_back('I'); lens.push_back(size); posQry += size; numIndels += size; }
					else { ops.push_back('D'); lens.push_back(size); posTrg += size; numIndels += size; }
				}
				own->runOff[i + 1] = ops.size() - first;		// count; summed below
				own->err[i] = float(numMiss + numIndels) / std::max(trgLen, qryLen);
			}
			tOps[th].swap(ops); tLens[th].swap(lens);
		  }
		  catch (...) { workerFailed.store(1); }
		});
		if (workerFailed.load()) throw std::bad_alloc();
		for (u32 i = 0; i < n_pairs; ++i) own->runOff[i + 1] += own->runOff[i];
		own->ops.reserve(own->runOff[n_pairs]); own->lens.reserve(own->runOff[n_pairs]);
		for (unsigned th = 0; th < nThreads; ++th)
		{
			own->ops.insert(own->ops.end(), tOps[th].begin(), tOps[th].end());
			own->lens.insert(own->lens.end(), tLens[th].begin(), tLens[th].end());
		}
		if (getenv("FG_KSW_TRACE"))
			fprintf(stderr, "[ksw] decode on %u threads %.1f ms\n", nThreads, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tDec).count());
	});
	if (rc != FG_OK) { delete own; return rc; }
	out->n_pairs = n_pairs;
	out->run_off = own->runOff.data();
	out->ops = own->ops.data();
	out->lens = own->lens.data();
	out->err_rate = own->err.data();
	out->owner_ = own;
	return FG_OK;
}

namespace {
// the argument checks fg_align_ranges and fg_trim_ranges share (before any device work) and the (pair, side) table
std::vector<FgRangeSide> rangeSides(fg_ctx* c, const char* fn, const struct fg_range_pair* pairs, uint32_t n_pairs, const void* out)
{
	const std::string name = fn;
	if (n_pairs && (!pairs || !out)) throw FgError{FG_ERR_ARG, name + ": pairs and out must not be NULL"};
	if (!c->nReads) throw FgError{FG_ERR_STATE, name + ": no reads (fg_set_reads first)"};
	std::vector<FgRangeSide> sides(2 * (size_t)n_pairs);
	for (u32 i = 0; i < n_pairs; ++i)
	{
		const fg_range_pair& P = pairs[i];
		auto side = [&](const char* what, u32 id, i32 begin, i32 end, bool mayBeQuery)
		{
			const bool inQ = mayBeQuery && c->hasQ;
			const u32 first = inQ ? c->qFirstId : c->firstId, n = inQ ? c->nQReads : c->nReads;
			if (id < first || (u64)id - first >= 2ULL * n)
				throw FgError{FG_ERR_ARG, name + ": pair " + std::to_string(i) + ": unknown " + what + " id " + std::to_string(id)};
			const u32 rec = (id - first) >> 1;
			const i32 L = inQ ? c->hQLen[rec] : c->hLen[rec];
			if (begin < 0 || end < begin || end > L)
				throw FgError{FG_ERR_ARG, name + ": pair " + std::to_string(i) + ": " + what + " range [" + std::to_string(begin) +
										  ", " + std::to_string(end) + ") is not inside the sequence of length " + std::to_string(L)};
			return FgRangeSide{rec, ((id - first) & 1u) | (inQ ? 2u : 0u), begin, end - begin};
		};
		sides[2 * (size_t)i] = side("cur", P.cur_id, P.cur_begin, P.cur_end, true);
		sides[2 * (size_t)i + 1] = side("ext", P.ext_id, P.ext_begin, P.ext_end, false);
	}
	return sides;
}

struct TrimOwner {
	std::vector<uint64_t> recOff;
	std::vector<fg_trim_rec> recs;
};

struct ChainOwner {
	std::vector<uint64_t> chainOff, alnOff, aln;
	std::vector<int32_t> score;
};
struct CoverageOwner {
	std::vector<uint64_t> winOff;
	std::vector<int32_t> full, junction, max, median, minGood, threshold;
	std::vector<int64_t> sum;
	std::vector<uint8_t> chimeric, degenerate;
};
// max, median, min of target t out of the device's three values per target
void splitCoverageStats(const std::vector<i32>& stat, std::vector<int32_t>& mx, std::vector<int32_t>& med, std::vector<int32_t>* mn)
{
	const size_t n = stat.size() / 3;
	mx.resize(n); med.resize(n);
	if (mn) mn->resize(n);
	for (size_t t = 0; t < n; ++t)
	{
		mx[t] = stat[3 * t]; med[t] = stat[3 * t + 1];
		if (mn) (*mn)[t] = stat[3 * t + 2];
	}
}
}

int fg_align_ranges(fg_ctx* c, const struct fg_range_pair* pairs, uint32_t n_pairs, uint8_t use_hpc,
					struct fg_cigar_batch* out, int32_t* len_cur, int32_t* len_ext)
{
	if (!c) return FG_ERR_ARG;
	if (out) memset(out, 0, sizeof(*out));
	CigarOwner* own = nullptr;
	const int rc = guarded(c, [&]()
	{
		const std::vector<FgRangeSide> sides = rangeSides(c, "fg_align_ranges", pairs, n_pairs, out);
		if (!out) return;		// n_pairs == 0 and nowhere to put the empty batch
		HIP_CHECK(hipSetDevice(c->device));
		own = new CigarOwner;
		std::vector<u32> errBases;
		std::vector<i32> lenCur, lenExt;
		fgAlignRanges(c, sides, use_hpc != 0, own->runOff, own->ops, own->lens, errBases, lenCur, lenExt);
		own->err.assign(n_pairs, 0.0f);
		// the float of alignment.cpp:213, computed here as fg_align_cigar_ksw computes it
		for (u32 i = 0; i < n_pairs; ++i)
			own->err[i] = float((int)errBases[i]) / std::max((size_t)lenCur[i], (size_t)lenExt[i]);
		if (len_cur) std::copy(lenCur.begin(), lenCur.end(), len_cur);
		if (len_ext) std::copy(lenExt.begin(), lenExt.end(), len_ext);
	});
	if (rc != FG_OK) { delete own; return rc; }
	if (!out) return FG_OK;
	out->n_pairs = n_pairs;
	out->run_off = own->runOff.data();
	out->ops = own->ops.data();
	out->lens = own->lens.data();
	out->err_rate = own->err.data();
	out->owner_ = own;
	return FG_OK;
}

int fg_trim_ranges(fg_ctx* c, const struct fg_range_pair* pairs, uint32_t n_pairs, uint8_t use_hpc, float max_divergence,
				   int32_t min_overlap, struct fg_trim_batch* out)
{
	if (!c) return FG_ERR_ARG;
	if (out) memset(out, 0, sizeof(*out));
	TrimOwner* own = nullptr;
	const int rc = guarded(c, [&]()
	{
		const std::vector<FgRangeSide> sides = rangeSides(c, "fg_trim_ranges", pairs, n_pairs, out);
		if (!out) return;
		HIP_CHECK(hipSetDevice(c->device));
		own = new TrimOwner;
		fgTrimRanges(c, sides, use_hpc != 0, max_divergence, min_overlap, own->recOff, own->recs);
		// the float of alignment.cpp:379, from the two integers
		for (auto& r : own->recs) r.seq_divergence = float(r.range_err) / r.range_len;
		if (own->recs.empty()) own->recs.reserve(1);
	});
	if (rc != FG_OK) { delete own; return rc; }
	if (!out) return FG_OK;
	out->n_pairs = n_pairs;
	out->rec_off = own->recOff.data();
	out->recs = own->recs.data();
	out->owner_ = own;
	return FG_OK;
}

int fg_edit_ranges(fg_ctx* c, const struct fg_range_pair* pairs, uint32_t n_pairs, uint8_t use_hpc, int32_t* dist,
				   int32_t* len_cur, int32_t* len_ext, float* divergence)
{
	if (!c) return FG_ERR_ARG;
	return guarded(c, [&]()
	{
		const std::vector<FgRangeSide> sides = rangeSides(c, "fg_edit_ranges", pairs, n_pairs, dist);
		if (!n_pairs) return;
		HIP_CHECK(hipSetDevice(c->device));
		// the float needs both lengths, whether the caller wants them or not
		std::vector<i32> ownCur, ownExt;
		if (divergence && !len_cur) { ownCur.resize(n_pairs); len_cur = ownCur.data(); }
		if (divergence && !len_ext) { ownExt.resize(n_pairs); len_ext = ownExt.data(); }
		fgEditRanges(c, sides, use_hpc != 0, dist, len_cur, len_ext);
		// the float of alignment.cpp:244, from the integers, as the host shim computes it for nucl_alignment records
		// (0 / 0 = NaN for two empty strings, as that expression gives)
		if (divergence)
			for (u32 i = 0; i < n_pairs; ++i)
				divergence[i] = (float)dist[i] / std::max((size_t)len_ext[i], (size_t)len_cur[i]);
	});
}

int fg_chain_divergence(const int32_t* cur_range, const float* divergence, const uint64_t* chain_off, uint32_t n_chains,
						float* out)
{
	if (!n_chains) return FG_OK;
	if (!chain_off || !out) return FG_ERR_ARG;
	for (u32 ch = 0; ch < n_chains; ++ch)
		if (chain_off[ch + 1] < chain_off[ch]) return FG_ERR_ARG;
	if (chain_off[n_chains] > chain_off[0] && (!cur_range || !divergence)) return FG_ERR_ARG;
	// read_aligner.cpp:418-431 in single precision, every operation rounded on its own: the reference is built without
	// fused multiply-add, so none may be formed here
	{
#pragma clang fp contract(off)
		for (u32 ch = 0; ch < n_chains; ++ch)
		{
			float sum = 0.0f;
			int len = 0;
			for (u64 i = chain_off[ch]; i < chain_off[ch + 1]; ++i)
			{
				const float keep = 1.0f - divergence[i];
				const float matched = (float)cur_range[i] * keep;
				sum = sum + matched;
				len += cur_range[i];
			}
			const float q = sum / (float)len;
			out[ch] = 1.0f - q;
		}
	}
	return FG_OK;
}

int fg_chain_alignments(fg_ctx* c, const struct fg_chain_params* p, const struct fg_overlap_rec* recs,
						const uint64_t* query_off, uint32_t n_queries, uint32_t first_ext_id, uint32_t n_ext_ids,
						const uint32_t* node_left, const uint32_t* node_right, struct fg_chain_batch* out)
{
	if (!c) return FG_ERR_ARG;
	if (out) memset(out, 0, sizeof(*out));
	ChainOwner* own = nullptr;
	const int rc = guarded(c, [&]()
	{
		const std::string name = "fg_chain_alignments";
		if (!p || !out) throw FgError{FG_ERR_ARG, name + ": null parameters or result"};
		if (p->max_jump <= 0 || p->max_read_overlap < 0 || p->min_alignment < 0 || p->max_separation < 0 || p->long_edge < 0 ||
			p->big_alignment < 0)
			throw FgError{FG_ERR_ARG, name + ": max_jump must be positive, the other parameters not negative"};
		if (n_queries && !query_off) throw FgError{FG_ERR_ARG, name + ": null query_off"};
		for (u32 q = 0; q < n_queries; ++q)
		{
			if (query_off[q + 1] < query_off[q]) throw FgError{FG_ERR_ARG, name + ": query_off decreases at query " + std::to_string(q)};
			if (query_off[q + 1] - query_off[q] > (u64)FG_CHAIN_MAX_RECS)
				throw FgError{FG_ERR_ARG, name + ": query " + std::to_string(q) + " has " + std::to_string(query_off[q + 1] - query_off[q]) +
										  " records, more than FG_CHAIN_MAX_RECS"};
		}
		const u64 r0 = n_queries ? query_off[0] : 0, nRec = n_queries ? query_off[n_queries] - r0 : 0;
		if (nRec && (!recs || !node_left || !node_right)) throw FgError{FG_ERR_ARG, name + ": null records or node tables"};
		// the seven integers the step reads of a record
		std::vector<FgChainAln> tab(nRec);
		for (u64 i = 0; i < nRec; ++i)
		{
			const fg_overlap_rec& r = recs[r0 + i];
			if (r.ext_id < first_ext_id || r.ext_id - first_ext_id >= n_ext_ids)
				throw FgError{FG_ERR_ARG, name + ": record " + std::to_string(r0 + i) + ": ext_id " + std::to_string(r.ext_id) +
										  " has no entry in the node tables"};
			if (r.cur_begin < 0 || r.cur_end < r.cur_begin || r.ext_begin < 0 || r.ext_end < r.ext_begin || r.ext_end > r.ext_len)
				throw FgError{FG_ERR_ARG, name + ": record " + std::to_string(r0 + i) + ": ranges [" + std::to_string(r.cur_begin) + ", " +
										  std::to_string(r.cur_end) + ") / [" + std::to_string(r.ext_begin) + ", " + std::to_string(r.ext_end) +
										  ") of " + std::to_string(r.ext_len)};
			tab[i] = FgChainAln{r.cur_begin, r.cur_end, r.ext_begin, r.ext_end, r.ext_len, r.score, r.ext_id - first_ext_id};
		}
		own = new ChainOwner;
		std::vector<u64> qOff((size_t)n_queries + 1, 0);
		for (u32 q = 0; q <= n_queries && n_queries; ++q) qOff[q] = query_off[q] - r0;
		if (nRec) HIP_CHECK(hipSetDevice(c->device));
		fgChainAlignments(c, *p, tab, qOff, r0, node_left, node_right, n_ext_ids, own->chainOff, own->alnOff, own->aln, own->score);
		if (own->aln.empty()) own->aln.reserve(1);
		if (own->score.empty()) own->score.reserve(1);
	});
	if (rc != FG_OK) { delete own; return rc; }
	out->n_queries = n_queries;
	out->n_chains = own->score.size();
	out->n_alns = own->aln.size();
	out->chain_off = own->chainOff.data();
	out->aln_off = own->alnOff.data();
	out->aln = own->aln.data();
	out->score = own->score.data();
	out->owner_ = own;
	return FG_OK;
}

int fg_coverage_windows(int32_t seq_len, int32_t window, int32_t max_overhang, int32_t* n_windows, int32_t* max_flank,
						uint8_t* degenerate)
{
	if (seq_len < 0 || window <= 0 || max_overhang < 0) return FG_ERR_ARG;
	// chimera.cpp:114-115 as written there: float / int, + 1 in single precision, then the conversion to int
	const int numWindows = std::ceil((float)seq_len / window) + 1;
	const int n = numWindows - 2;
	if (n_windows) *n_windows = n <= 0 ? 1 : n;
	if (degenerate) *degenerate = n <= 0 ? 1 : 0;
	// :168-169: int / float, truncated
	if (max_flank) *max_flank = (int)((float)(int)max_overhang / (float)window);
	return FG_OK;
}

int fg_coverage_verdict(const struct fg_coverage_params* p, uint32_t n, const int32_t* n_windows, const int64_t* sum,
						const int32_t* median, const int32_t* min_good, int32_t* threshold, uint8_t* chimeric)
{
	if (!p || p->window <= 0 || p->max_overhang < 0 || !(p->max_drop_rate > 0)) return FG_ERR_ARG;
	if (!n) return FG_OK;
	if (!n_windows || !sum || !median || !min_good || !chimeric) return FG_ERR_ARG;
	int32_t maxFlank = 0;
	fg_coverage_windows(0, p->window, p->max_overhang, nullptr, &maxFlank, nullptr);
	const float MAX_DROP_RATE = p->max_drop_rate;
	for (u32 i = 0; i < n; ++i)
	{
		if (sum[i] == 0)		// chimera.cpp:153
		{
			if (threshold) threshold[i] = 0;
			chimeric[i] = 1;
			continue;
		}
		// :155-164
		int thr;
		if (!p->uneven_coverage) thr = std::max(1L, std::lround((float)p->overlap_coverage / MAX_DROP_RATE));
		else thr = std::max(1L, std::lround(median[i] / MAX_DROP_RATE));
		// :166-182 with the loop folded into min_good
		const int32_t goodStart = maxFlank, goodEnd = n_windows[i] - maxFlank - 1;
		if (threshold) threshold[i] = thr;
		chimeric[i] = (goodEnd <= goodStart || min_good[i] < thr) ? 1 : 0;
	}
	return FG_OK;
}

int fg_read_coverage(fg_ctx* c, const struct fg_coverage_params* p, const struct fg_overlap_rec* recs,
					 const uint64_t* query_off, uint32_t n_queries, const int32_t* query_len, struct fg_coverage_batch* out)
{
	if (!c) return FG_ERR_ARG;
	if (out) memset(out, 0, sizeof(*out));
	CoverageOwner* own = nullptr;
	const int rc = guarded(c, [&]()
	{
		const std::string name = "fg_read_coverage";
		if (!p || !out) throw FgError{FG_ERR_ARG, name + ": null parameters or result"};
		if (p->window <= 0 || p->max_overhang < 0 || !(p->max_drop_rate > 0))
			throw FgError{FG_ERR_ARG, name + ": window and max_drop_rate must be positive, max_overhang not negative"};
		if (n_queries && (!query_off || !query_len)) throw FgError{FG_ERR_ARG, name + ": null query_off or query_len"};
		for (u32 q = 0; q < n_queries; ++q)
		{
			if (query_off[q + 1] < query_off[q]) throw FgError{FG_ERR_ARG, name + ": query_off decreases at query " + std::to_string(q)};
			if (query_len[q] < 0) throw FgError{FG_ERR_ARG, name + ": query " + std::to_string(q) + " has a negative length"};
		}
		const u64 r0 = n_queries ? query_off[0] : 0, nRec = n_queries ? query_off[n_queries] - r0 : 0;
		if (nRec && !recs) throw FgError{FG_ERR_ARG, name + ": null records"};
		for (u32 q = 0; q < n_queries; ++q)
			for (u64 i = query_off[q]; i < query_off[q + 1]; ++i)
			{
				const fg_overlap_rec& r = recs[i];
				if (r.cur_len != query_len[q] || r.cur_begin < 0 || r.cur_end < r.cur_begin || r.cur_end > r.cur_len || r.ext_begin < 0 ||
					r.ext_end < r.ext_begin || r.ext_end > r.ext_len)
					throw FgError{FG_ERR_ARG, name + ": record " + std::to_string(i) + " of query " + std::to_string(q) + ": ranges [" +
											  std::to_string(r.cur_begin) + ", " + std::to_string(r.cur_end) + ") of " + std::to_string(r.cur_len) +
											  " / [" + std::to_string(r.ext_begin) + ", " + std::to_string(r.ext_end) + ") of " +
											  std::to_string(r.ext_len) + ", query length " + std::to_string(query_len[q])};
			}
		own = new CoverageOwner;
		own->winOff.assign((size_t)n_queries + 1, 0);
		own->degenerate.resize(n_queries);
		std::vector<u64> qOff((size_t)n_queries + 1, 0);
		std::vector<i32> nClip(n_queries), nWin(n_queries);
		int32_t maxFlank = 0;
		fg_coverage_windows(0, p->window, p->max_overhang, nullptr, &maxFlank, nullptr);
		for (u32 q = 0; q < n_queries; ++q)
		{
			fg_coverage_windows(query_len[q], p->window, p->max_overhang, &nWin[q], nullptr, &own->degenerate[q]);
			nClip[q] = own->degenerate[q] ? 0 : nWin[q];
			own->winOff[q + 1] = own->winOff[q] + (u64)nWin[q];
			qOff[q + 1] = query_off[q + 1] - r0;
		}
		const u64 nAll = own->winOff[n_queries];
		if (p->want_vectors) { own->full.resize(nAll); own->junction.resize(nAll); }
		own->sum.resize(n_queries);
		own->threshold.resize(n_queries); own->chimeric.resize(n_queries);
		std::vector<i32> stat(3 * (size_t)n_queries);
		if (n_queries)
		{
			HIP_CHECK(hipSetDevice(c->device));
			fgReadCoverage(c, p->window, p->max_overhang, maxFlank, recs ? recs + r0 : nullptr, qOff, own->winOff, nClip,
						   p->want_vectors != 0, own->full.data(), own->junction.data(), (long long*)own->sum.data(), stat.data());
		}
		splitCoverageStats(stat, own->max, own->median, &own->minGood);
		fg_coverage_verdict(p, n_queries, nWin.data(), own->sum.data(), own->median.data(), own->minGood.data(), own->threshold.data(),
							own->chimeric.data());
		for (auto* v : {&own->full, &own->junction, &own->max, &own->median, &own->minGood, &own->threshold})
			if (v->empty()) v->reserve(1);
		if (own->sum.empty()) own->sum.reserve(1);
		if (own->chimeric.empty()) { own->chimeric.reserve(1); own->degenerate.reserve(1); }
	});
	if (rc != FG_OK) { delete own; return rc; }
	out->n_queries = n_queries;
	out->win_off = own->winOff.data();
	out->full = p->want_vectors ? own->full.data() : nullptr;
	out->junction = p->want_vectors ? own->junction.data() : nullptr;
	out->sum = own->sum.data();
	out->max = own->max.data();
	out->median = own->median.data();
	out->min_good = own->minGood.data();
	out->threshold = own->threshold.data();
	out->chimeric = own->chimeric.data();
	out->degenerate = own->degenerate.data();
	out->owner_ = own;
	return FG_OK;
}

void fg_release_coverage(struct fg_coverage_batch* b)
{
	if (!b) return;
	delete (CoverageOwner*)b->owner_;
	memset(b, 0, sizeof(*b));
}

int fg_edge_coverage(fg_ctx* c, int32_t window, const struct fg_overlap_rec* recs, uint64_t n_recs, const uint64_t* aln,
					 const uint64_t* aln_off, uint64_t n_paths, uint32_t first_ext_id, uint32_t n_ext_ids, const uint32_t* edge_of,
					 uint32_t n_edges, const int32_t* edge_len, uint8_t want_vectors, struct fg_edge_coverage_batch* out)
{
	if (!c) return FG_ERR_ARG;
	if (out) memset(out, 0, sizeof(*out));
	CoverageOwner* own = nullptr;
	const int rc = guarded(c, [&]()
	{
		const std::string name = "fg_edge_coverage";
		if (!out) throw FgError{FG_ERR_ARG, name + ": null result"};
		if (window <= 0) throw FgError{FG_ERR_ARG, name + ": window must be positive"};
		if (n_edges && !edge_len) throw FgError{FG_ERR_ARG, name + ": null edge_len"};
		if (n_paths && !aln_off) throw FgError{FG_ERR_ARG, name + ": null aln_off"};
		if (n_ext_ids && !edge_of) throw FgError{FG_ERR_ARG, name + ": null edge_of"};
		for (u32 e = 0; e < n_edges; ++e)
			if (edge_len[e] < 0) throw FgError{FG_ERR_ARG, name + ": edge " + std::to_string(e) + " has a negative length"};
		for (u32 i = 0; i < n_ext_ids; ++i)
			if (edge_of[i] >= n_edges)
				throw FgError{FG_ERR_ARG, name + ": edge_of[" + std::to_string(i) + "] = " + std::to_string(edge_of[i]) + " is no edge"};
		for (u64 k = 0; k < n_paths; ++k)
			if (aln_off[k + 1] < aln_off[k]) throw FgError{FG_ERR_ARG, name + ": aln_off decreases at path " + std::to_string(k)};
		const u64 a0 = n_paths ? aln_off[0] : 0, nEl = n_paths ? aln_off[n_paths] - a0 : 0;
		if (nEl && (!aln || !recs)) throw FgError{FG_ERR_ARG, name + ": null records or alignment indices"};
		if (nEl >= (1ULL << 30)) throw FgError{FG_ERR_ARG, name + ": more than 2^30 - 1 path elements in one call"};
		std::vector<FgCovEdgeEl> el(nEl);
		for (u64 k = 0; k < n_paths; ++k)
			for (u64 i = aln_off[k]; i < aln_off[k + 1]; ++i)
			{
				if (aln[i] >= n_recs)
					throw FgError{FG_ERR_ARG, name + ": aln[" + std::to_string(i) + "] = " + std::to_string(aln[i]) + " is no record"};
				const fg_overlap_rec& r = recs[aln[i]];
				if (r.ext_id < first_ext_id || r.ext_id - first_ext_id >= n_ext_ids)
					throw FgError{FG_ERR_ARG, name + ": record " + std::to_string(aln[i]) + ": ext_id " + std::to_string(r.ext_id) +
											  " has no entry in edge_of"};
				el[i - a0] = FgCovEdgeEl{r.ext_begin, r.ext_end, edge_of[r.ext_id - first_ext_id],
										 (i > aln_off[k] ? 1u : 0u) | (i + 1 < aln_off[k + 1] ? 2u : 0u)};
			}
		own = new CoverageOwner;
		own->winOff.assign((size_t)n_edges + 1, 0);
		for (u32 e = 0; e < n_edges; ++e) own->winOff[e + 1] = own->winOff[e] + (u64)(edge_len[e] / window);
		if (want_vectors) own->full.resize(own->winOff[n_edges]);
		own->sum.resize(n_edges);
		std::vector<i32> stat(3 * (size_t)n_edges);
		if (n_edges)
		{
			HIP_CHECK(hipSetDevice(c->device));
			fgEdgeCoverage(c, window, el, own->winOff, want_vectors != 0, own->full.data(), (long long*)own->sum.data(), stat.data());
		}
		splitCoverageStats(stat, own->max, own->median, nullptr);
		for (auto* v : {&own->full, &own->max, &own->median})
			if (v->empty()) v->reserve(1);
		if (own->sum.empty()) own->sum.reserve(1);
	});
	if (rc != FG_OK) { delete own; return rc; }
	out->n_edges = n_edges;
	out->win_off = own->winOff.data();
	out->cov = want_vectors ? own->full.data() : nullptr;
	out->sum = own->sum.data();
	out->max = own->max.data();
	out->median = own->median.data();
	out->owner_ = own;
	return FG_OK;
}

void fg_release_edge_coverage(struct fg_edge_coverage_batch* b)
{
	if (!b) return;
	delete (CoverageOwner*)b->owner_;
	memset(b, 0, sizeof(*b));
}

namespace {
struct PolishOwner {
	std::vector<uint8_t> cand, status, stepSeq;
	std::vector<uint64_t> candOff, stepOff, stepSeqOff;
	std::vector<uint32_t> nSteps;
	std::vector<int64_t> stepScore;
};
int polishLetter(const std::string& item, bool last)
{
	if (item.empty()) return -1;
	switch (last ? item[item.size() - 1] : item[0])
	{
	case 'A': return 0;
	case 'C': return 1;
	case 'G': return 2;
	case 'T': return 3;
	default: return -1;
	}
}
}

int fg_subs_matrix_load(const char* path, struct fg_subs_matrix* out)
{
	if (!path || !out) return FG_ERR_ARG;
	memset(out, 0, sizeof(*out));
	FILE* f = fopen(path, "rb");
	if (!f) return FG_ERR_ARG;
	std::string text;
	char buf[4096];
	size_t got;
	while ((got = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, got);
	fclose(f);
	size_t at = 0;
	while (at < text.size())
	{
		size_t end = text.find('\n', at);
		if (end == std::string::npos) end = text.size();
		std::string line = text.substr(at, end - at);
		at = end + 1;
		if (!line.empty() && line[line.size() - 1] == '\r') line.pop_back();
		std::vector<std::string> items;
		size_t a = 0;
		for (;;)
		{
			const size_t t = line.find('\t', a);
			items.push_back(line.substr(a, t == std::string::npos ? t : t - a));
			if (t == std::string::npos) break;
			a = t + 1;
		}
		const std::string& kind = items[0];
		if (kind != "mat" && kind != "mis" && kind != "del" && kind != "ins") continue;
		if (items.size() < 3) return FG_ERR_ARG;
		const int x = polishLetter(items[1], false), y = polishLetter(items[1], true);
		if (x < 0 || (kind == "mis" && y < 0)) return FG_ERR_ARG;
		char* stop = nullptr;
		const double p = strtod(items[2].c_str(), &stop);
		if (stop == items[2].c_str()) return FG_ERR_ARG;
		const int64_t sc = (int64_t)std::round(std::log(p) * 131072.0);
		if (kind == "mat") out->score[x][x] = sc;
		else if (kind == "mis") out->score[x][y] = sc;
		else if (kind == "del") out->score[x][5] = sc;
		else out->score[5][x] = sc;
	}
	return FG_OK;
}

int fg_polish_bubbles(fg_ctx* c, const struct fg_subs_matrix* matrix, const uint8_t* cand, const uint64_t* cand_off,
					  const uint8_t* branches, const uint64_t* branch_off, const uint64_t* bubble_branch_off, uint32_t n_bubbles,
					  uint8_t fix_dinucleotides, uint8_t want_steps, struct fg_polish_batch* out)
{
	if (!c) return FG_ERR_ARG;
	if (out) memset(out, 0, sizeof(*out));
	PolishOwner* own = nullptr;
	const int rc = guarded(c, [&]()
	{
		const std::string name = "fg_polish_bubbles";
		if (!matrix || !out) throw FgError{FG_ERR_ARG, name + ": null matrix or result"};
		if (n_bubbles && (!cand_off || !bubble_branch_off)) throw FgError{FG_ERR_ARG, name + ": null cand_off or bubble_branch_off"};
		for (u32 i = 0; i < n_bubbles; ++i)
		{
			if (cand_off[i + 1] < cand_off[i]) throw FgError{FG_ERR_ARG, name + ": cand_off decreases at bubble " + std::to_string(i)};
			if (bubble_branch_off[i + 1] < bubble_branch_off[i])
				throw FgError{FG_ERR_ARG, name + ": bubble_branch_off decreases at bubble " + std::to_string(i)};
		}
		const u64 c0 = n_bubbles ? cand_off[0] : 0, c1 = n_bubbles ? cand_off[n_bubbles] : 0;
		const u64 r0 = n_bubbles ? bubble_branch_off[0] : 0, r1 = n_bubbles ? bubble_branch_off[n_bubbles] : 0;
		if (c1 > c0 && !cand) throw FgError{FG_ERR_ARG, name + ": null cand"};
		if (r1 > r0 && !branch_off) throw FgError{FG_ERR_ARG, name + ": null branch_off"};
		for (u64 r = r0; r < r1; ++r)
			if (branch_off[r + 1] < branch_off[r]) throw FgError{FG_ERR_ARG, name + ": branch_off decreases at branch " + std::to_string(r)};
		const u64 b0 = r1 > r0 ? branch_off[r0] : 0, b1 = r1 > r0 ? branch_off[r1] : 0;
		if (b1 > b0 && !branches) throw FgError{FG_ERR_ARG, name + ": null branches"};
		for (u64 k = c0; k < c1; ++k)
			if (cand[k] >= 128) throw FgError{FG_ERR_ARG, name + ": byte " + std::to_string(cand[k]) + " in a candidate"};
		for (u64 k = b0; k < b1; ++k)
			if (branches[k] >= 128) throw FgError{FG_ERR_ARG, name + ": byte " + std::to_string(branches[k]) + " in a branch"};
		own = new PolishOwner;
		std::vector<std::string> outCand;
		std::vector<std::vector<std::pair<std::string, int64_t>>> steps;
		if (n_bubbles)
		{
			HIP_CHECK(hipSetDevice(c->device));
			fgPolishBubbles(c, &matrix->score[0][0], cand, cand_off, branches, branch_off, bubble_branch_off, n_bubbles,
							fix_dinucleotides != 0, want_steps != 0, outCand, own->nSteps, own->status, steps);
		}
		own->candOff.assign(1, 0);
		for (const std::string& v : outCand)
		{
			own->cand.insert(own->cand.end(), v.begin(), v.end());
			own->candOff.push_back(own->cand.size());
		}
		if (want_steps)
		{
			own->stepOff.assign(1, 0);
			own->stepSeqOff.assign(1, 0);
			for (const auto& list : steps)
			{
				for (const auto& st : list)
				{
					own->stepSeq.insert(own->stepSeq.end(), st.first.begin(), st.first.end());
					own->stepSeqOff.push_back(own->stepSeq.size());
					own->stepScore.push_back(st.second);
				}
				own->stepOff.push_back(own->stepScore.size());
			}
		}
		for (auto* v : {&own->cand, &own->status, &own->stepSeq})
			if (v->empty()) v->reserve(1);
		if (own->nSteps.empty()) own->nSteps.reserve(1);
		if (own->stepScore.empty()) own->stepScore.reserve(1);
	});
	if (rc != FG_OK) { delete own; return rc; }
	out->n_bubbles = n_bubbles;
	out->cand = own->cand.data();
	out->cand_off = own->candOff.data();
	out->n_steps = own->nSteps.data();
	out->status = own->status.data();
	if (want_steps)
	{
		out->step_off = own->stepOff.data();
		out->step_score = own->stepScore.data();
		out->step_seq = own->stepSeq.data();
		out->step_seq_off = own->stepSeqOff.data();
	}
	out->owner_ = own;
	return FG_OK;
}

void fg_release_polish(struct fg_polish_batch* b)
{
	if (!b) return;
	delete (PolishOwner*)b->owner_;
	memset(b, 0, sizeof(*b));
}

void fg_release_chains(struct fg_chain_batch* b)
{
	if (!b) return;
	delete (ChainOwner*)b->owner_;
	memset(b, 0, sizeof(*b));
}

void fg_release_trims(struct fg_trim_batch* b)
{
	if (!b) return;
	delete (TrimOwner*)b->owner_;
	memset(b, 0, sizeof(*b));
}

void fg_release_cigars(struct fg_cigar_batch* b)
{
	if (!b) return;
	delete (CigarOwner*)b->owner_;
	memset(b, 0, sizeof(*b));
}

void fg_release_batch(struct fg_overlap_batch* b)
{
	if (!b) return;
	BatchOwner::release((BatchOwner*)b->owner_);
	memset(b, 0, sizeof(*b));
}

int fg_kernel_times(fg_ctx* c, struct fg_kernel_time* out, int max_entries)
{
	if (!c || (max_entries > 0 && !out)) return FG_ERR_ARG;
	int n = (int)c->timer.last.size();
	for (int i = 0; i < n && i < max_entries; ++i) out[i] = c->timer.last[i];
	return n;
}

} // extern "C"
