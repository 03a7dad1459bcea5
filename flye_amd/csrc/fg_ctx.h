// Internal context of libflyegpu.so (host side) + device helpers shared by the
// kernels.  gfx950 only.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <new>
#include <cstring>
#include <string>
#include <vector>
#include <map>
#include <memory>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <atomic>
#include <algorithm>

#include "../../include/flye_gpu.h"
#include "fg_error.h"

typedef uint64_t u64;
typedef uint32_t u32;
typedef uint16_t u16;
typedef int32_t i32;

#define FG_EMPTY_KEY 0xFFFFFFFFFFFFFFFFULL
#define FG_CNT_BITS 24
#define FG_CNT_MASK 0xFFFFFFu
#define FG_CNT_REPETITIVE 0xFFFFFFu	// probe result for a k-mer of _repetitiveKmers
#define FG_IDX_BITS 30				// narrow slot: key << 30 | key index inside its part (all ones = repetitive)
#define FG_IDX_MASK 0x3FFFFFFFULL
#define FG_TABLE_MAX_PARTS 16

// The lookup table as the kernels see it (passed by value).  Narrow form (2k <= 34 bits, i.e. k <= 17): one
// u64 per slot; keys are split into parts by key RANGE so that an index inside a part fits 30 bits
// (one part up to 2^30 - 2 keys; the split follows the sorted key array, equal key counts per part).
// Wide form (k > 17): {key, key index} pairs, one part.  Linear probing inside a part, load <= 0.5.
struct FgTable {
	const unsigned long long* slots;
	const ulonglong2* wide;
	const unsigned long long* keyOff;
	unsigned nParts;
	unsigned long long bound[FG_TABLE_MAX_PARTS + 1];	// part p: keys in [bound[p], bound[p + 1])
	unsigned long long slotBase[FG_TABLE_MAX_PARTS];
	unsigned long long keyBase[FG_TABLE_MAX_PARTS];
	unsigned groups[FG_TABLE_MAX_PARTS];				// 8-slot groups of part p
};

#define HIP_CHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
	throw FgError{FG_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_) + \
	" (" + __FILE__ + ":" + std::to_string(__LINE__) + ")"}; } } while (0)

// --- device buffer -----------------------------------------------------------
// device bytes this library holds right now / at most since the last reset, over all contexts of the process
// (fg_memory_stats): every device allocation of the library goes through DevBuf
inline std::atomic<unsigned long long> g_fgDevBytes{0}, g_fgDevPeak{0};
inline void fgDevAccount(long long delta)
{
	const unsigned long long now = g_fgDevBytes.fetch_add((unsigned long long)delta) + (unsigned long long)delta;
	unsigned long long pk = g_fgDevPeak.load();
	while (delta > 0 && now > pk && !g_fgDevPeak.compare_exchange_weak(pk, now)) {}
}

template <class T>
struct DevBuf {
	T* p = nullptr;
	size_t n = 0;
	bool owned = true;		// false: a view of another context's buffer (the second lane of fg_overlaps)
	DevBuf() {}
	DevBuf(const DevBuf&) = delete;
	DevBuf& operator=(const DevBuf&) = delete;
	~DevBuf() { release(); }
	void release()
	{
		if (p && owned) { (void)hipFree(p); fgDevAccount(-(long long)(n * sizeof(T))); }
		p = nullptr; n = 0; owned = true;
	}
	void alias(const DevBuf& o) { release(); p = o.p; n = o.n; owned = false; }
	void swap(DevBuf& o) { std::swap(p, o.p); std::swap(n, o.n); std::swap(owned, o.owned); }
	void alloc(size_t count)
	{
		release();
		if (count == 0) count = 1;
		hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
		if (e != hipSuccess)
			throw FgError{FG_ERR_NOMEM, "hipMalloc of " + std::to_string(count * sizeof(T)) + " bytes: " + hipGetErrorString(e)};
		n = count;
		fgDevAccount((long long)(n * sizeof(T)));
	}
	// grow-only (keeps capacity between batches)
	void reserve(size_t count) { if (count > n) alloc(count + count / 8); }
	size_t bytes() const { return n * sizeof(T); }
};

// page-locked host staging buffer (grow-only)
template <class T>
struct PinnedBuf {
	T* p = nullptr;
	size_t n = 0;
	PinnedBuf() {}
	PinnedBuf(const PinnedBuf&) = delete;
	PinnedBuf& operator=(const PinnedBuf&) = delete;
	~PinnedBuf() { if (p) (void)hipHostFree(p); }
	void reserve(size_t count)
	{
		if (count <= n) return;
		if (p) { (void)hipHostFree(p); p = nullptr; n = 0; }
		count += count / 8;
		hipError_t e = hipHostMalloc((void**)&p, count * sizeof(T), hipHostMallocDefault);
		if (e != hipSuccess)
			throw FgError{FG_ERR_NOMEM, "hipHostMalloc of " + std::to_string(count * sizeof(T)) + " bytes: " + hipGetErrorString(e)};
		n = count;
	}
	// grow and keep the first `used` elements (no copy is pending on them: the caller has synchronised)
	void reserveKeep(size_t count, size_t used)
	{
		if (count <= n) return;
		count += count / 2;
		T* q = nullptr;
		hipError_t e = hipHostMalloc((void**)&q, count * sizeof(T), hipHostMallocDefault);
		if (e != hipSuccess)
			throw FgError{FG_ERR_NOMEM, "hipHostMalloc of " + std::to_string(count * sizeof(T)) + " bytes: " + hipGetErrorString(e)};
		if (p && used) memcpy(q, p, used * sizeof(T));
		if (p) (void)hipHostFree(p);
		p = q; n = count;
	}
};

// --- per-kernel timing with HIP events on the library stream -------------------
struct KernelTimer {
	struct Ev { const char* name; hipEvent_t a, b; };
	std::vector<Ev> evs;
	std::vector<hipEvent_t> pool;
	hipStream_t stream = nullptr;
	bool enabled = true;
	std::vector<fg_kernel_time> last;

	hipEvent_t get()
	{
		if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
		hipEvent_t e; HIP_CHECK(hipEventCreate(&e)); return e;
	}
	// on: the stream the bracketed launches go to (default: the context's main stream)
	size_t begin(const char* name, hipStream_t on = nullptr)
	{
		if (!enabled) return 0;
		Ev ev{name, get(), get()};
		HIP_CHECK(hipEventRecord(ev.a, on ? on : stream));
		evs.push_back(ev);
		return evs.size() - 1;
	}
	void end(size_t id, hipStream_t on = nullptr)
	{
		if (!enabled) return;
		HIP_CHECK(hipEventRecord(evs[id].b, on ? on : stream));
	}
	// forget uncollected measurements (a previous call failed half way): the events go back to the pool
	void reset()
	{
		for (auto& ev : evs) { pool.push_back(ev.a); pool.push_back(ev.b); }
		evs.clear();
	}
	// after a stream sync: fold into per-name sums
	void collect()
	{
		last.clear();
		std::vector<std::string> order;
		std::map<std::string, size_t> idx;
		for (auto& ev : evs)
		{
			float ms = 0;
			HIP_CHECK(hipEventElapsedTime(&ms, ev.a, ev.b));
			auto it = idx.find(ev.name);
			if (it == idx.end())
			{
				idx[ev.name] = last.size();
				last.push_back(fg_kernel_time{ev.name, 0.0, 0});
				it = idx.find(ev.name);
			}
			last[it->second].seconds += ms * 1e-3;
			last[it->second].launches += 1;
			pool.push_back(ev.a); pool.push_back(ev.b);
		}
		evs.clear();
	}
	~KernelTimer() { for (auto e : pool) (void)hipEventDestroy(e); }
};

struct ScopedK {
	KernelTimer& t; size_t id; hipStream_t on;
	ScopedK(KernelTimer& t_, const char* name, hipStream_t on_ = nullptr) : t(t_), id(t_.begin(name, on_)), on(on_) {}
	~ScopedK() { try { t.end(id, on); } catch (...) {} }
};

// Worker threads of the host shim, kept between calls: spawning 16 std::threads per fg_overlaps call cost more
// than the shim's own arithmetic.
// CPUs this process may actually use: the cgroup's quota where there is one (a container that shows 256 threads but
// is granted 16 CPUs of time runs host loops slower on 32 threads than on 16)
inline unsigned fg_usable_cpus()
{
	static const unsigned cpus = []
	{
		unsigned n = std::max(1u, std::thread::hardware_concurrency());
		if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r"))
		{
			char quota[32]; long period = 0;
			if (fscanf(f, "%31s %ld", quota, &period) == 2 && strcmp(quota, "max") != 0 && period > 0)
				n = std::min<unsigned>(n, (unsigned)std::max(1L, atol(quota) / period));
			fclose(f);
		}
		// one process per GPU (torchrun): the ranks of this node share those CPUs
		if (const char* lw = getenv("LOCAL_WORLD_SIZE"))
			if (atoi(lw) > 1) n = std::max(1u, n / (unsigned)atoi(lw));
		return n;
	}();
	return cpus;
}

struct ShimPool {
	std::vector<std::thread> threads;
	std::mutex mu;
	std::condition_variable cvGo, cvDone;
	const std::function<void(unsigned)>* job = nullptr;
	unsigned long long epoch = 0;
	unsigned pending = 0, nActive = 0;
	bool stop = false;

	void ensure(unsigned n)
	{
		while (threads.size() < n)
		{
			const unsigned id = (unsigned)threads.size();
			threads.emplace_back([this, id]
			{
				unsigned long long seen = 0;
				std::unique_lock<std::mutex> lk(mu);
				while (true)
				{
					cvGo.wait(lk, [&] { return stop || (epoch != seen && id < nActive); });
					if (stop) return;
					seen = epoch;
					const std::function<void(unsigned)>* f = job;
					lk.unlock();
					(*f)(id);
					lk.lock();
					if (--pending == 0) cvDone.notify_all();
				}
			});
		}
	}
	// fn(0 .. n-1), one call per thread; returns when all are done.  n == 1 runs inline.
	void run(unsigned n, const std::function<void(unsigned)>& fn)
	{
		if (n <= 1) { fn(0); return; }
		ensure(n);
		std::unique_lock<std::mutex> lk(mu);
		job = &fn; nActive = n; pending = n; ++epoch;
		cvGo.notify_all();
		cvDone.wait(lk, [&] { return pending == 0; });
		// threads beyond n that woke up went back to sleep (id >= nActive); the epoch they skipped is harmless
	}
	~ShimPool()
	{
		{ std::lock_guard<std::mutex> g(mu); stop = true; }
		cvGo.notify_all();
		for (auto& t : threads) if (t.joinable()) t.join();
	}
};

struct fg_ctx {
	int device = 0;
	int k = 17;
	hipStream_t stream = nullptr;
	// side streams of the chaining stage: the big-group chains run there beside the small-group kernel of the main
	// stream (fork / join by events), so that neither class waits for the other's last waves
	hipStream_t stream2 = nullptr, stream3 = nullptr;
	hipEvent_t evFork = nullptr, evJoin = nullptr, evJoin3 = nullptr;
	// the primaries of a chunk leave for the host in nPieces copies with an event behind each; the shim's tasks start
	// on a piece as soon as ITS copy has landed (piece i covers the primaries below pieceEnd[i], counted over the
	// whole call)
#define FG_D2H_MAX_PIECES 16
	hipEvent_t evOff = nullptr, evPiece[FG_D2H_MAX_PIECES] = {};
	unsigned long long pieceEnd[FG_D2H_MAX_PIECES] = {};
	int nPieces = 0;
	std::string lastError;
	KernelTimer timer;

	// reads (the index container == the query container for now)
	u32 nReads = 0;
	u32 firstId = 0;
	u64 totalWords = 0, totalBases = 0, totalKmers = 0;
	i32 maxLen = 0;
	std::vector<i32> hLen;
	std::vector<u64> hKmerOff;
	DevBuf<u64> dWords;		// +2 padding words
	DevBuf<u64> dWordOff;	// n+1
	DevBuf<i32> dLen;		// n
	DevBuf<u64> dKmerOff;	// n+1 prefix of max(len-k,0)

	// optional second container holding the queries (ReadAligner-style use: reads vs graph
	// edges, reference src/repeat_graph/read_aligner.cpp:178-217); when absent queries are
	// the indexed reads themselves
	bool hasQ = false;
	u32 nQReads = 0, qFirstId = 0;
	i32 qMaxLen = 0;
	std::vector<i32> hQLen;
	DevBuf<u64> dQWords, dQWordOff;
	DevBuf<i32> dQLen;

	// index
	bool indexBuilt = false;
	float sampleRate = 1.0f;
	u64 nKeys = 0, nEntries = 0, nRep = 0, tableSlots = 0;
	DevBuf<u64> dKeys;		// ascending canonical k-mers of _kmerIndex (incl. empty lists)
	DevBuf<u64> dKeyOff;	// nKeys+1
	DevBuf<u64> dEntries;	// (record<<32 | pos), ascending per key
	DevBuf<u64> dRepKeys;	// ascending
	DevBuf<u64> dTable;			// narrow slots, or ulonglong2 {key, index} pairs when tableWide
	bool tableWide = false;
	FgTable table{};
	DevBuf<u32> dIndexedBits;	// one bit per forward k-mer position: contributes an entry
	// one bit per forward k-mer position, same numbering: the k-mer's frequency over the whole read set reached the
	// build's minFreq.  A CLEAR bit proves the lookup table has no slot for the k-mer (a key enters only through an
	// accepted position, k_accept), so k_probe skips the probe.  Only a solid-k-mer build of this context leaves
	// them (they outlive the gather of a sharded build and keep_targets: the table only ever holds keys of accepted
	// positions); empty after a minimizer build, an import and the direct option-B scatter: every k-mer is probed
	DevBuf<u32> dMaybeBits;
	// option B (fg_index_keep_targets): the lists hold only the entries of target reads i with i % shardWorld ==
	// shardRank; the indexed bits of the other reads are cleared.  1 / 0 = the whole index
	u32 shardWorld = 1, shardRank = 0;

	// second lane of fg_overlaps: a context of its own scratch, streams and timers whose read / index / probe buffers
	// are views of this one's (fg_overlap.hip: sub-ranges of a call's queries run on two lanes side by side)
	std::unique_ptr<fg_ctx> lane2;
	std::shared_ptr<void> indexBuild;	// state between the steps of an index build (fg_index.hip)
	// between fg_index_gather_begin and _end: this context's own piece of a sharded build, set aside while the
	// arrays above are the full-size ones the ranks' pieces are gathered into
	bool gathering = false;
	DevBuf<u64> gKeys, gKeyOff, gEntries, gRepKeys;
	u64 gNKeys = 0, gNEntries = 0, gNRep = 0;
	// option B built directly (fg_index_piece_split / fg_index_scatter_begin / _end): the piece's per-(destination,
	// key) entry counts (splitWorld rows of nKeys, + 1 element) and its entries in destination-major order;
	// splitWorld == 0: no split at hand.  Between scatter_begin and _end the piece sits in the g* buffers above and
	// the context's arrays are the shard's, being filled by the caller's all-to-all
	u32 splitWorld = 0;
	DevBuf<u64> sCounts, sEntries;
	bool scattering = false;
	u32 scatterWorld = 1, scatterRank = 0;

	// overlap-stage scratch (grow-only)
	DevBuf<u32> dQuery;			// query record indices
	u64 hitCapHint = 0;			// hits of the largest sub-range of the chunk in work (per-hit scratch is reserved for it)
	const u32* curQuery = nullptr;	// ... of the sub-range of the chunk the stage is working on (group / primary records index it)
	DevBuf<u64> dQKmerOff;		// per query prefix of k-mer counts
	DevBuf<u64> dProbe;			// per query k-mer: table value (0 = miss)
	// probes partitioned by table region (tables beyond the caches): (region | k-mer, position) pairs, twice, + sort scratch
	DevBuf<u64> dPartK0, dPartV0, dPartK1, dPartV1;
	DevBuf<char> dPartScratch;
	DevBuf<unsigned long long> dPartCount;	// pairs k_probe_emit appended
	DevBuf<u64> dHitOff;		// per query hit offsets (nq+1)
	DevBuf<u64> dFiltOff;		// per query repetitive-position offsets (nq+1)
	DevBuf<i32> dFiltPos;
	DevBuf<u64> dHitKey;		// extId<<32 | curPos
	DevBuf<u32> dHitVal;		// extPos
	DevBuf<u16> dHitVal16;		// extPos beside dHitKey32 when every target position fits 16 bits (hitVal16)
	bool hitVal16 = false;		// the value form of the last sub-range this context expanded (fg_debug_hit_val16)
	DevBuf<u32> dHitKey32;		// record << curBits | curPos, when that fits 32 bits (sort only)
	DevBuf<i32> dScore, dBack;
	DevBuf<int4> dCand;
	DevBuf<u64> dGroupStart;	// group boundaries (indices into hits)
	DevBuf<u32> dGroupQuery;
	// per group: its target id and the query position of its first and last hit (what the
	// chaining kernels and the span prefilter need of the sorted keys)
	DevBuf<u32> dGroupExt, dGroupFirstCur, dGroupLastCur;
	DevBuf<uint8_t> dGroupExtSorted;	// written by k_group_prep: the DP runs in extPos order (overlap.cpp:268-275)
	DevBuf<u32> dTmp32;
	// option B: the seed hits fg_probe_hits hands out; the receiver's run table, gather slots and error flag
	DevBuf<fg_seed_hit> dSeedHits;
	DevBuf<u64> dRecvRun, dRecvIdx;
	DevBuf<u32> dRecvErr;
	DevBuf<u64> dCntA, dCntB, dGroupCnt, dGroupOff, dPrimCnt, dPrimOff, dDpGroups, dDpElems;
	DevBuf<u32> dPrimFlag, dDpSize, dListSmall, dListBig, dListDp, dListFused, dListCnt;
	// flat listing (fg_overlap.hip, FG_GROUP_FLAT): head counts of the hit tiles (scanned in place into the tiles' first
	// group numbers, + 1 element = nGroups), every group's first record position (+ 1 element = nPrim) and the scratch
	// of their fgprim::scan calls
	DevBuf<u32> dTileCnt, dPrimPos, dScanScratch;
	DevBuf<u32> dCur, dExt;		// (cur, ext) columns of the groups in DP order
	DevBuf<char> dPrimOut;	// PrimRec array
	// keep_alignment: per primary the chain's last hit (global hit index), its group's first
	// hit, the slot offsets (chainLength + 2 pairs each) and the thinned chain itself
	DevBuf<u64> dPrimNode, dPrimBase, dMatchSize, dMatchOff, dMatches;
	DevBuf<u32> dMatchCnt;
	PinnedBuf<u64> hMatches, hMatchOff;
	PinnedBuf<u32> hMatchCnt;
	DevBuf<char> dSortTasks, dSortBig;
	// DP elements in groups of <= 256 hits (work counter); the flat listing adds the call's DP groups and DP elements
	// behind it (three totals)
	DevBuf<unsigned long long> dSmallElems;
	// fg_debug_chain_lazy: FG_LAZY_STRIPES rows of 8 counters the chaining kernels bump once per group (fg_chain.hip),
	// zeroed per fg_overlaps call; the second lane's is a view of this one
	DevBuf<unsigned long long> dLazyCnt;
	DevBuf<u32> dSortCnt;		// task counts of the sort's level loop, a row per level (fg_overlap.hip)
	DevBuf<u32> dTieFree;		// per query, written by k_fill: 1 = no two of its hits share (extId, curPos)
	u32 tieFreeQ0 = 0, tieFreeN = 0;	// the queries of the call dTieFree speaks of (0: the last sub-range had no flags)
	// per query, written by k_sort_screen: dSortFree = dTieFree | "every tied key lies in a group the chaining prefilter
	// drops" (what the sort takes the radix path by), dSortReason = its SCREEN_* word (fg_overlap.hip)
	DevBuf<u32> dSortFree, dSortReason;
	u32 sortReasonN = 0;				// tieFreeN where the last sub-range was screened, else 0 (fg_debug_order_free)
	u32 sortRadixSegs = 0;				// segments the last hit sort of this context sent to k_sort_radix
	DevBuf<int> dEditScratch;
	DevBuf<u32> dEditList;		// pairs queued for the bit-vector kernel (two lists)
	DevBuf<char> dEditCnt;
	DevBuf<u64> dEditSlab;		// per-block string planes + delta planes of the bit-vector kernel
	// fg_edit_ranges (fg_editranges.hip): the primaries and the query array k_edit_range_prims makes of a sub-batch's
	// side table (in dRangeSides), and the three dense arrays k_edit_range_collect leaves for the download
	DevBuf<char> dEditPrims;
	DevBuf<u32> dEditQuery;
	DevBuf<i32> dEditOut;
	// fg_align_ranges (fg_ksw.hip): the (pair, side) table, the compressed lengths, the byte strings the ksw kernels
	// read and where each one starts, and what the decoding of a sub-batch leaves (counts, offsets, '=' / 'X' / 'I' /
	// 'D' runs)
	DevBuf<char> dRangeSides;
	DevBuf<i32> dRangeLen;
	DevBuf<u64> dRangeOff;
	DevBuf<uint8_t> dRangeTrg, dRangeQry;
	DevBuf<u32> dDecCnt;
	DevBuf<u64> dDecOff;
	DevBuf<uint8_t> dDecOps;
	DevBuf<i32> dDecLens;
	// fg_trim_ranges (fg_trim.hip): prefix sums over a sub-batch's runs, candidate counts per (pair, interval length)
	// and their scan, the good intervals of a trim sub-batch (sort key, rank, (start, end)) with their segment
	// offsets, the accepted intervals and the records made of them
	DevBuf<i32> dTrimPre;
	DevBuf<u64> dTrimRowCnt, dTrimRowOff, dTrimScan, dTrimKeys, dTrimIvl, dTrimSeg, dTrimAcc, dTrimAccOff;
	DevBuf<unsigned long long> dTrimPairCnt;
	DevBuf<u32> dTrimVals, dTrimAccCnt, dTrimKept;
	DevBuf<char> dTrimRaw, dTrimOut;
	// fg_chain_alignments (fg_readchain.hip): the node tables, a sub-batch's side table and per-query offsets, the keys
	// and values of its two sorts, the sorted alignments, the per-alignment state of the DP and of the selection (one
	// pool of 32-bit arrays) and the chains that go back
	DevBuf<u32> dRcNodes, dRcVals, dRcU32;
	DevBuf<char> dRcTab, dRcAln;
	DevBuf<u64> dRcOff, dRcKeys, dRcOut;
	DevBuf<i32> dRcOutScore;
	// fg_read_coverage / fg_edge_coverage (fg_coverage.hip): a sub-batch's records (or path elements), its packed
	// intervals (twice for the edges' sort, with the keys), the per-target offsets and sums, the per-target 32-bit
	// arrays (clip counts, class lists, max / median / min) and the window vectors
	DevBuf<char> dCovRecs, dCovSort;
	DevBuf<u64> dCovIv, dCovKeys, dCovOff;
	DevBuf<i32> dCovI32, dCovVec;
	// fg_polish_bubbles (fg_polish.hip): the call's branches (bytes, offsets) and score table; per chunk of a round the
	// candidates, items, branch alignments, edit offsets, the F / R cells, the edit sums and the results
	DevBuf<char> dPolBytes, dPolCand, dPolItems, dPolTasks, dPolRes;
	DevBuf<u64> dPolOff, dPolEdOff;
	DevBuf<long long> dPolScore, dPolCells, dPolEdits;
	// fg_make_bubbles (fg_bubbles.hip): the buffers of one sub-batch, handed out in call order
	DevBuf<char> dBub[36];
	// fg_uniform_alignments / fg_contig_consensus (fg_contigcons.hip): likewise
	DevBuf<char> dCc[40];
	// fg_expand_cigars (fg_cigar.hip): the call's contig bytes in the first, then the buffers of one sub-batch
	DevBuf<char> dCig[20];
	// fg_divergence_profile (fg_divergence.hip): the buffers of one sub-batch, handed out in call order
	DevBuf<char> dDv[28];
	// fg_confirm_positions / fg_classify_reads (fg_partition.hip): the buffers of one sub-batch, handed out in call order
	DevBuf<char> dPt[36];
	// fg_paf_groups / fg_paf_circular / fg_components (fg_plasmid.hip): the buffers of one call, handed out in call order
	DevBuf<char> dPaf[32];
	// fg_sam_parse (fg_samtext.hip): a sub-batch's text, its per-byte and per-line tables and its results, in call order
	DevBuf<char> dSam[16];
	PinnedBuf<char> hPrim;
	PinnedBuf<u64> hOff;
	PinnedBuf<u64> hScalar;		// staging of the counts the host reads between kernels (pinned: no bounce buffer)
	// host shim: worker threads kept between calls (the record pass needs no result-sized scratch, fg_taskchain.h)
	ShimPool shimPool;

	~fg_ctx()
	{
		if (evFork) (void)hipEventDestroy(evFork);
		if (evJoin) (void)hipEventDestroy(evJoin);
		if (evJoin3) (void)hipEventDestroy(evJoin3);
		if (evOff) (void)hipEventDestroy(evOff);
		for (auto e : evPiece) if (e) (void)hipEventDestroy(e);
		if (stream2) (void)hipStreamDestroy(stream2);
		if (stream3) (void)hipStreamDestroy(stream3);
		if (stream) (void)hipStreamDestroy(stream);
	}
};

// --- device helpers ----------------------------------------------------------
#if defined(__HIPCC__)

// wave-uniform values loaded through the vector memory path: pinned to SGPRs so that loop
// control becomes scalar branches and base addresses scalar operands
__device__ __forceinline__ i32 fg_uni(i32 v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ u32 fg_uni(u32 v) { return (u32)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ u64 fg_uni(u64 v)
{
	return ((u64)(u32)__builtin_amdgcn_readfirstlane((int)(u32)(v >> 32)) << 32) |
		   (u32)__builtin_amdgcn_readfirstlane((int)(u32)v);
}

// One 64-bit sort RECORD for workloads whose (record, query position) pairs do not fit 32 bits:
// (record << (curBits + 24)) | (curPos << 24) | extPos.  Ordered (and tested for >=, <=) on the upper
// bits only -- the (extId, curPos) comparator of overlap.cpp:201-204; the target position rides in the
// low 24 bits, so a hit stays 8 bytes in the sort levels instead of 8 + 4.  == / != look at all bits.
#define FG_PK_VALBITS 24
struct PK {
	u64 v;
	PK() = default;
	__host__ __device__ PK(int x) : v((u64)(unsigned)x) {}
	__host__ __device__ explicit PK(u64 x) : v(x) {}
};
__device__ __forceinline__ bool operator<(const PK& a, const PK& b) { return (a.v >> FG_PK_VALBITS) < (b.v >> FG_PK_VALBITS); }
__device__ __forceinline__ bool operator>(const PK& a, const PK& b) { return (a.v >> FG_PK_VALBITS) > (b.v >> FG_PK_VALBITS); }
__device__ __forceinline__ bool operator<=(const PK& a, const PK& b) { return (a.v >> FG_PK_VALBITS) <= (b.v >> FG_PK_VALBITS); }
__device__ __forceinline__ bool operator>=(const PK& a, const PK& b) { return (a.v >> FG_PK_VALBITS) >= (b.v >> FG_PK_VALBITS); }
__device__ __forceinline__ bool operator==(const PK& a, const PK& b) { return a.v == b.v; }
__device__ __forceinline__ bool operator!=(const PK& a, const PK& b) { return a.v != b.v; }

// "no value array": reads give 0, writes vanish (the value travels inside a PK record)
struct NoVal {
	struct Ref {
		__device__ __forceinline__ operator u32() const { return 0u; }
		__device__ __forceinline__ const Ref& operator=(u32) const { return *this; }
	};
	__device__ __forceinline__ Ref operator[](long long) const { return Ref{}; }
	__device__ __forceinline__ NoVal operator+(long long) const { return NoVal{}; }
};

// the sorted hit keys, typed at compile time: u64 = (extId << 32 | curPos),
// u32 = ((extId - firstId) << curBits | curPos), PK = the packed record above, K32V16 = the u32 keys with
// 16-bit values (every target position below 2^16: two bytes less per hit in every pass over the values)
struct K32V16;
// key(i) hands out the stored key; ext_of / ext_raw_of / cur_of read it as ext / ext_raw / cur read hit i (a kernel that has
// the key in a register need not load it again)
template <class KT> struct HitKeyView;
template <> struct HitKeyView<u64> {
	const u64* k; const u32* v; int curBits; u32 firstId;
	__device__ __forceinline__ u32 ext(u64 i) const { return (u32)(k[i] >> 32); }
	__device__ __forceinline__ u32 ext_raw(u64 i) const { return (u32)(k[i] >> 32); }
	__device__ __forceinline__ u32 cur(u64 i) const { return (u32)k[i]; }
	typedef u64 Word;
	__device__ __forceinline__ u64 key(u64 i) const { return k[i]; }
	__device__ __forceinline__ u32 ext_of(u64 x) const { return (u32)(x >> 32); }
	__device__ __forceinline__ u32 ext_raw_of(u64 x) const { return (u32)(x >> 32); }
	__device__ __forceinline__ u32 cur_of(u64 x) const { return (u32)x; }
	__device__ __forceinline__ u32 val(u64 i) const { return v[i]; }
};
template <> struct HitKeyView<u32> {
	const u32* k; const u32* v; int curBits; u32 firstId;
	__device__ __forceinline__ u32 ext(u64 i) const { return (k[i] >> curBits) + firstId; }
	__device__ __forceinline__ u32 ext_raw(u64 i) const { return k[i] >> curBits; }
	__device__ __forceinline__ u32 cur(u64 i) const { return k[i] & ((1u << curBits) - 1u); }
	typedef u32 Word;
	__device__ __forceinline__ u32 key(u64 i) const { return k[i]; }
	__device__ __forceinline__ u32 ext_of(u32 x) const { return (x >> curBits) + firstId; }
	__device__ __forceinline__ u32 ext_raw_of(u32 x) const { return x >> curBits; }
	__device__ __forceinline__ u32 cur_of(u32 x) const { return x & ((1u << curBits) - 1u); }
	__device__ __forceinline__ u32 val(u64 i) const { return v[i]; }
};
template <> struct HitKeyView<K32V16> {
	const u32* k; const u16* v; int curBits; u32 firstId;
	__device__ __forceinline__ u32 ext(u64 i) const { return (k[i] >> curBits) + firstId; }
	__device__ __forceinline__ u32 ext_raw(u64 i) const { return k[i] >> curBits; }
	__device__ __forceinline__ u32 cur(u64 i) const { return k[i] & ((1u << curBits) - 1u); }
	typedef u32 Word;
	__device__ __forceinline__ u32 key(u64 i) const { return k[i]; }
	__device__ __forceinline__ u32 ext_of(u32 x) const { return (x >> curBits) + firstId; }
	__device__ __forceinline__ u32 ext_raw_of(u32 x) const { return x >> curBits; }
	__device__ __forceinline__ u32 cur_of(u32 x) const { return x & ((1u << curBits) - 1u); }
	__device__ __forceinline__ u32 val(u64 i) const { return v[i]; }
};
template <> struct HitKeyView<PK> {
	const PK* k; const u32* v; int curBits; u32 firstId;
	__device__ __forceinline__ u32 ext(u64 i) const { return (u32)(k[i].v >> (FG_PK_VALBITS + curBits)) + firstId; }
	__device__ __forceinline__ u32 ext_raw(u64 i) const { return (u32)(k[i].v >> (FG_PK_VALBITS + curBits)); }
	__device__ __forceinline__ u32 cur(u64 i) const { return (u32)(k[i].v >> FG_PK_VALBITS) & ((1u << curBits) - 1u); }
	typedef u64 Word;
	__device__ __forceinline__ u64 key(u64 i) const { return k[i].v; }
	__device__ __forceinline__ u32 ext_of(u64 x) const { return (u32)(x >> (FG_PK_VALBITS + curBits)) + firstId; }
	__device__ __forceinline__ u32 ext_raw_of(u64 x) const { return (u32)(x >> (FG_PK_VALBITS + curBits)); }
	__device__ __forceinline__ u32 cur_of(u64 x) const { return (u32)(x >> FG_PK_VALBITS) & ((1u << curBits) - 1u); }
	__device__ __forceinline__ u32 val(u64 i) const { return (u32)k[i].v & ((1u << FG_PK_VALBITS) - 1u); }
};

__device__ __forceinline__ u64 fg_mix(u64 x)
{
	x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33;
	x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
	return x;
}

// base `pos` of a record on the strand asked for (reference sequence.h:120-129); w = the record's forward words
__device__ __forceinline__ u32 fg_base_at(const u64* __restrict__ w, i32 L, bool rc, i32 pos)
{
	const i32 p = rc ? L - 1 - pos : pos;
	const u32 b = (u32)((w[p >> 5] >> ((p & 31) * 2)) & 3);
	return rc ? (~b & 3) : b;
}

// One 64-base step of a walk over [start, start + len) of a record, all 64 lanes: lane l takes base t0 + l of the
// range.  b = its base (0 behind the range), keep = inside the range and, with hpc, not a repeat of the base before
// it (homopolymerCompression, alignment.cpp:52-70); carry = the last base of the previous step (4 before the first
// one: the first base of a range is always kept), updated for the next.  Returns the ballot of keep.
__device__ __forceinline__ u64 fg_range_step(const u64* __restrict__ w, i32 L, bool rc, i32 start, i32 len, bool hpc,
											 i32 t0, u32& carry, u32& b, bool& keep)
{
	const int lane = threadIdx.x & 63;
	const i32 t = t0 + lane;
	const bool valid = t < len;
	b = valid ? fg_base_at(w, L, rc, start + t) : 0u;
	u32 prev = __shfl_up(b, 1);
	if (lane == 0) prev = carry;
	keep = valid && (!hpc || prev != b);
	carry = __shfl(b, 63);
	return __builtin_amdgcn_ballot_w64(keep);
}

// splitmix64 finaliser = Kmer::hash() (reference src/sequence/kmer.h:91-98)
__device__ __forceinline__ u64 fg_kmer_hash(u64 x)
{
	u64 z = (x += 0x9E3779B97F4A7C15ULL);
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
	return z ^ (z >> 31);
}

// 2k bits of the packed forward read starting at base q (base q in bits 0-1).
// `w` points at the read's first word; the caller guarantees q + k <= len.
__device__ __forceinline__ u64 fg_chunk(const u64* __restrict__ w, i32 q, int k)
{
	const int sh = (q & 31) * 2;
	u64 lo = w[q >> 5] >> sh;
	if (sh + 2 * k > 64) lo |= w[(q >> 5) + 1] << (64 - sh);
	return (k == 32) ? lo : (lo & ((1ULL << (2 * k)) - 1));
}

// reverse the order of the k 2-bit groups: packed chunk -> Kmer repr (first
// base most significant, kmer.h:32-36)
__device__ __forceinline__ u64 fg_rev2(u64 x, int k)
{
	u64 r = __brevll(x);
	r = ((r >> 1) & 0x5555555555555555ULL) | ((r & 0x5555555555555555ULL) << 1);
	return r >> (64 - 2 * k);
}

// forward / reverse-complement representation of the k-mer at forward position
// q; rc repr is simply the complemented packed chunk (kmer.h:39-52)
__device__ __forceinline__ void fg_kmer_pair(const u64* __restrict__ w, i32 q, int k, u64& fw, u64& rv)
{
	const u64 x = fg_chunk(w, q, k);
	const u64 mask = (k == 32) ? ~0ULL : ((1ULL << (2 * k)) - 1);
	fw = fg_rev2(x, k);
	rv = ~x & mask;
}

// the slot of `key` in part p of a narrow table, starting at group g: the slot's value, or FG_EMPTY_KEY when absent
__device__ __forceinline__ u64 fg_probe_slot(const FgTable& T, u32 p, u32 g, u64 key)
{
	const u32 nGroups = T.groups[p];
	while (true)
	{
		const ulonglong2* grp = (const ulonglong2*)(T.slots + T.slotBase[p] + (u64)g * 8u);
		const ulonglong2 a = grp[0], b = grp[1], c = grp[2], d = grp[3];
		const u64 sl[8] = {a.x, a.y, b.x, b.y, c.x, c.y, d.x, d.y};
		u64 hit = FG_EMPTY_KEY;
		bool empty = false;
#pragma unroll
		for (int i = 0; i < 8; ++i)
		{
			if ((sl[i] >> FG_IDX_BITS) == key) hit = sl[i];
			empty |= sl[i] == FG_EMPTY_KEY;
		}
		if (hit != FG_EMPTY_KEY || empty) return hit;
		g = g + 1 == nGroups ? 0 : g + 1;
	}
}

// probe: returns off << 24 | cnt of the k-mer's list, FG_CNT_REPETITIVE in the low bits for a k-mer of
// _repetitiveKmers, or 0 when absent.  One 8-byte slot read decides a miss (4 in 5 query k-mers: the
// table is half the size of a 16-byte layout -- E. coli 50x: 134 MB, inside the 256 MiB Infinity Cache);
// a hit reads the list bounds from the key-ordered offsets.
template <bool WIDE>
__device__ __forceinline__ u64 fg_probe(const FgTable& T, u64 key)
{
	u32 p = 0;
	if (T.nParts > 1)
		while (p + 1 < T.nParts && key >= T.bound[p + 1]) ++p;
	const u64 mix = fg_mix(key);
	const u32 nGroups = T.groups[p];
	u32 g = __umulhi((u32)(mix >> 32), nGroups);
	if (WIDE)
	{
		// {key, index} pairs, linear probing over the part's slots
		const u32 slotsInPart = nGroups * 8u;
		u32 h = g * 8u + ((u32)mix & 7u);
		while (true)
		{
			const ulonglong2 s = T.wide[T.slotBase[p] + h];
			if (s.x == FG_EMPTY_KEY) return 0;
			if (s.x != key) { h = h + 1 == slotsInPart ? 0 : h + 1; continue; }
			if (s.y == FG_EMPTY_KEY) return FG_CNT_REPETITIVE;
			const u64 o = T.keyOff[s.y];
			return (o << FG_CNT_BITS) | (T.keyOff[s.y + 1] - o);
		}
	}
	// narrow: the key's 8-slot group is one 64-byte line, fetched whole; insertion fills a group before it
	// spills into the next, so an empty slot anywhere in the group settles a miss without a second access
	const u64 hit = fg_probe_slot(T, p, g, key);
	if (hit == FG_EMPTY_KEY) return 0;
	if ((hit & FG_IDX_MASK) == FG_IDX_MASK) return FG_CNT_REPETITIVE;
	const u64 idx = T.keyBase[p] + (hit & FG_IDX_MASK);
	const u64 o = T.keyOff[idx];
	return (o << FG_CNT_BITS) | (T.keyOff[idx + 1] - o);
}

#endif // __HIPCC__

// result arena of one fg_overlaps call.  recs is a raw grow-only buffer (no value
// initialisation of ~100 MB per call); released arenas go back to a small per-process pool
// so that steady-state calls neither page-fault nor munmap.
struct BatchOwner {
	std::vector<u64> queryOff, statOff;
	fg_overlap_rec* recs = nullptr;
	size_t recCap = 0, nRecs = 0;
	std::vector<float> stats;
	std::vector<uint8_t> needsTrim;	// partition_bad_mappings: nRecs
	std::vector<u64> matchOff;	// keep_alignment: nRecs + 1, in pairs
	int32_t* matches = nullptr;	// (cur, ext) pairs
	size_t matchCap = 0;
	void reserveMatches(size_t nPairs)
	{
		if (nPairs <= matchCap) return;
		free(matches);
		matchCap = nPairs + nPairs / 8 + 16;
		matches = (int32_t*)malloc(matchCap * 8);
		if (!matches) { matchCap = 0; throw std::bad_alloc(); }
	}
	void reserveRecs(size_t n)
	{
		if (n <= recCap) return;
		free(recs);
		recCap = n + n / 8 + 16;
		recs = (fg_overlap_rec*)malloc(recCap * sizeof(fg_overlap_rec));
		if (!recs) { recCap = 0; throw std::bad_alloc(); }
	}
	~BatchOwner() { free(recs); free(matches); }
	static BatchOwner* acquire();
	static void release(BatchOwner* b);
};

// one primary overlap candidate as the device hands it to the host shim
struct PrimRec {
	u32 query;		// index into the batch
	u32 extId;
	i32 curBegin, curEnd, extBegin, extEnd, extLen, score, chainLength, filtered;
	i32 editDistance, hpcLenCur, hpcLenExt;
};

// implemented in fg_index.hip / fg_overlap.hip
void fgBuildIndexSolid(fg_ctx* c, i32 minFreq, float selectRate, i32 tandemFreq, float repeatRate,
					   float sampleRateInit, fg_index_stats* st);
void fgBuildIndexMinimizers(fg_ctx* c, i32 minCoverage, i32 window, float repeatRate, fg_index_stats* st);
// the same in steps (sharded builds): begin -> ranges of key bins -> finish; fg_index.hip
void fgIndexBeginSolid(fg_ctx* c, i32 minFreq, float selectRate, i32 tandemFreq, float repeatRate,
					   float sampleRateInit, u64* histOut);
// the solid selection in steps (bounded memory, counters of a key range only): count -> per batch of reads
// {frequencies -> [sum over ranks] -> select} -> done
void fgIndexKmerHist(fg_ctx* c, u64* histOut);
void fgIndexCountSlice(fg_ctx* c, i32 minFreq, float selectRate, i32 tandemFreq, float repeatRate, float sampleRateInit,
					   u32 binLo, u32 binHi, u64* distinctOut, u32* nBatchesOut);
void fgIndexBatchFreq(fg_ctx* c, u32 batch, u32** dFreq, u64* nPos);
void fgIndexBatchSelect(fg_ctx* c, u32 batch);
void fgIndexSelectionDone(fg_ctx* c, u64* histOut);
void fgIndexGatherBegin(fg_ctx* c, u64 nKeys, u64 nEntries, u64 nRep, u64** full, u64** piece, u64* pieceSizes);
void fgIndexGatherEnd(fg_ctx* c, float sampleRate);
void fgIndexBeginMinimizers(fg_ctx* c, i32 minCoverage, i32 window, float repeatRate, u64* histOut);
void fgIndexBuildRange(fg_ctx* c, u32 binLo, u32 binHi, unsigned long long* sumsOut);
void fgIndexFinish(fg_ctx* c, const unsigned long long* totalSums, fg_index_stats* st);
void fgIndexLookupStructures(fg_ctx* c, bool bitsHoldSelection);
void fgImportIndex(fg_ctx* c, u64 nKeys, const u64* keys, const u64* keyOff, u64 nEnt, const u64* entries, u64 nRep,
				   const u64* repKeys, float sampleRate, int onDevice);
// keyMode: 0 = 32-bit keys, 1 = packed 64-bit records (PK), 2 = 64-bit keys + values
u32 fgChainSmallMax();
// the distinct query positions a group needs, minKmerSruvivalRate * _minOverlap as the reference's float (overlap.cpp:110,
// :235): the chaining prefilter's bound, and what the hit sort's screen (k_sort_screen) decides by ahead of it
inline float fgChainMinUnique(const fg_detector_params* p)
{
	const float minKmerSruvivalRate = 0.01;
	return minKmerSruvivalRate * p->min_overlap;
}
void fgChainStage(fg_ctx* c, const fg_detector_params* p, uint8_t forceLocal, u64 nGroups, u64 nHits, int keyMode,
				  int curBits);
void fgEditDistances(fg_ctx* c, PrimRec* dPrims, u64 nPrim, int useHpc);
void fgKswAlign(fg_ctx* c, u32 nPairs, const uint8_t* trg, const u64* trgOff, const uint8_t* qry, const u64* qryOff,
				std::vector<u64>& runOff, std::vector<u32>& runs);
// fg_align_ranges behind its argument checks: sides = 2 nPairs entries (target, query of pair 0, ...); runs of pair i
// at ops / lens[runOff[i] ..), errBases = its mismatches + indel bases, lenCur / lenExt = the aligned lengths
struct FgRangeSide { u32 rec; u32 flags; i32 start, len; };		// rec: index in its container; flags: 1 = reverse
																// complement, 2 = the fg_set_queries container
void fgAlignRanges(fg_ctx* c, const std::vector<FgRangeSide>& sides, bool useHpc, std::vector<u64>& runOff,
				   std::vector<uint8_t>& ops, std::vector<i32>& lens, std::vector<u32>& errBases, std::vector<i32>& lenCur,
				   std::vector<i32>& lenExt);
// the device part of fgAlignRanges: after the decoding of each ksw sub-batch (pairs [first, first + count) of the
// call) `sink` is called while the runs are on the device: run k of pair first + i at c->dDecOps / c->dDecLens
// [off[i] + k], off (count + 1 entries, also in c->dDecOff) ending at nOut.  The caller resets and collects the timer.
struct FgDecodedRuns { u32 first, count; const u64* off; u64 nOut; };
void fgAlignRangesDevice(fg_ctx* c, const std::vector<FgRangeSide>& sides, bool useHpc, std::vector<u64>& runOff,
						 std::vector<u32>& errBases, std::vector<i32>& lenCur, std::vector<i32>& lenExt,
						 const std::function<void(const FgDecodedRuns&)>& sink);
// fg_trim_ranges behind its argument checks (fg_trim.hip): the second half of checkIdyAndTrim on the runs of
// fgAlignRangesDevice; recs of pair i at recs[recOff[i] ..), seq_divergence left for the caller
void fgTrimRanges(fg_ctx* c, const std::vector<FgRangeSide>& sides, bool useHpc, float maxDivergence, i32 minOverlap,
				  std::vector<u64>& recOff, std::vector<fg_trim_rec>& recs);
// std::sort order (ascending keys, the permutation libstdc++ produces) of each segment [segOff[i], segOff[i + 1]) of
// the device arrays keys / vals; dSegOff on the device
void fgSortSegments(fg_ctx* c, const u64* dSegOff, u32 nSeg, u64* dKeys, u32* dVals, u64 n);
// fg_edit_ranges behind its argument checks (fg_editranges.hip): fgEditDistances on the ranges of `sides` (cur, ext of
// pair 0, ...), in sub-batches of FG_EDIT_BATCH_PAIRS; dist / lenCur / lenExt: host arrays of sides.size() / 2 entries,
// the two lengths may be null.  Resets and collects the timer; c->curQuery is as before on return.
void fgEditRanges(fg_ctx* c, const std::vector<FgRangeSide>& sides, bool useHpc, i32* dist, i32* lenCur, i32* lenExt);
// fg_chain_alignments behind its argument checks (fg_readchain.hip).  tab: what the step reads of every record, in the
// caller's order (ext = ext_id - first_ext_id); qOff: n_queries + 1 offsets into it; recBase: the caller's query_off[0];
// nodeLeft / nodeRight: nExt entries.  Queries are worked on in sub-batches of FG_READCHAIN_BATCH_RECS records.  Resets
// and collects the timer.
struct FgChainAln { i32 curBegin, curEnd, extBegin, extEnd, extLen, score; u32 ext; };
void fgChainAlignments(fg_ctx* c, const fg_chain_params& p, const std::vector<FgChainAln>& tab, const std::vector<u64>& qOff,
					   u64 recBase, const u32* nodeLeft, const u32* nodeRight, u32 nExt, std::vector<u64>& chainOff,
					   std::vector<u64>& alnOff, std::vector<u64>& aln, std::vector<i32>& score);
// fg_read_coverage / fg_edge_coverage behind their argument checks (fg_coverage.hip).  Reads: recs = the caller's records
// from query_off[0] on, qOff / winOff: n_queries + 1 offsets (from 0) of the queries' records / windows, nClip[q]: the
// windows an interval of query q may touch (0 for a degenerate query); queries are worked on in sub-batches of
// FG_COVERAGE_BATCH_RECS records.  Edges: one FgCovEdgeEl per path element (flags 1 = not the first of its path, 2 = not
// the last), winOff: n_edges + 1.  full / junction / cov may be null without wantVectors; sum: one per target; stat:
// three per target (max, median, min over the good range).  Both reset and collect the timer.
struct FgCovEdgeEl { i32 extBegin, extEnd; u32 edge, flags; };
void fgReadCoverage(fg_ctx* c, i32 window, i32 maxOverhang, i32 maxFlank, const fg_overlap_rec* recs, const std::vector<u64>& qOff,
					const std::vector<u64>& winOff, const std::vector<i32>& nClip, bool wantVectors, i32* full, i32* junction,
					long long* sum, i32* stat);
void fgEdgeCoverage(fg_ctx* c, i32 window, const std::vector<FgCovEdgeEl>& el, const std::vector<u64>& winOff, bool wantVectors,
					i32* cov, long long* sum, i32* stat);
// fg_polish_bubbles behind its argument checks (fg_polish.hip): score36 = the 6 x 6 table [consensus class][read class];
// the flat inputs of the ABI call; per bubble the final candidate, the number of steps, the status bits and (wantSteps)
// the steps as (sequence, score).  Resets and collects the timer.
void fgPolishBubbles(fg_ctx* c, const int64_t* score36, const uint8_t* cand, const uint64_t* candOff, const uint8_t* branches,
					 const uint64_t* branchOff, const uint64_t* bubbleBranchOff, u32 nBubbles, bool fixDinucleotides, bool wantSteps,
					 std::vector<std::string>& outCand, std::vector<uint32_t>& nSteps, std::vector<uint8_t>& status,
					 std::vector<std::vector<std::pair<std::string, int64_t>>>& steps);
void fgDebugSortPairs(fg_ctx* c, u64* keys, u32* vals, const u64* segOff, u32 nSeg, int curBits = 0);
void fgDebugSortPacked(fg_ctx* c, u64* recs, const u64* segOff, u32 nSeg, int curBits);
void fgDebugSortPairs32(fg_ctx* c, u32* keys, u32* vals, const u64* segOff, u32 nSeg, int curBits, int recBits,
						const u32* tieFree, u64* radixSegments, u64* radixHits);
void fgDebugSortPairs32v16(fg_ctx* c, u32* keys, u16* vals, const u64* segOff, u32 nSeg, int curBits, int recBits,
						   const u32* tieFree, u64* radixSegments, u64* radixHits);
void fgDebugTieFree(fg_ctx* c, u32* out, u32 maxN, u32* firstQuery, u32* n);
void fgDebugSortScreen(fg_ctx* c, const u32* keys, const u64* segOff, u32 nSeg, int curBits, int recBits, const u32* tieFree,
					   float minUnique, i32 minOverlap, u32* outReason);
void fgDebugOrderFree(fg_ctx* c, u32* out, u32 maxN, u32* firstQuery, u32* n);
void fgDebugProbeSkipCheck(fg_ctx* c, u64* clearBits, u64* violations);
#define FG_LAZY_STRIPES 64
void fgDebugChainLazy(fg_ctx* c, u64 out[6]);
void fgDebugEditDistances(fg_ctx* c, u32 nPairs, int useHpc, i32* outDist, i32* outLenA, i32* outLenB);
// option B: seed hits gathered from index shards, as the overlap stage takes them in place of its own seed
// expansion.  Per query qi of the call and source s: the run of hits[runStart[qi * nSrc + s] ..] of runLen[..]
// hits (any order inside a run); total[qi] = the query's hits over all sources
struct RecvHits {
	u32 nSrc;
	const u64* runStart;
	const u64* runLen;
	const u64* total;
	const fg_seed_hit* hits;	// device
};
void fgOverlaps(fg_ctx* c, const fg_detector_params* p, const u32* queryIds, u32 nq, i32 maxOverlaps,
				uint8_t forceLocal, fg_overlap_batch* out, const RecvHits* recv = nullptr);
void fgIndexKeepTargets(fg_ctx* c, u32 world, u32 rank, u64* nKept);
// option B without the full entry array: piece -> per-destination parts -> shard (fg_index.hip)
#define FG_SPLIT_MAX_WORLD 128		// k_split_*: world * 64 cursors of 4 bytes + world bases in one wave's LDS
void fgIndexPieceSplit(fg_ctx* c, u32 world, const u64** dCounts, const u64** dEntries, u64* destTotals);
void fgIndexScatterBegin(fg_ctx* c, u32 world, u32 rank, u64 nKeys, u64 nShardEntries, u64 nRep, u64** full);
void fgIndexScatterEnd(fg_ctx* c, float sampleRate);
void fgProbeHits(fg_ctx* c, const u32* queryIds, u32 nq, u64* hitCounts, const fg_seed_hit** dHits, u64* nHits);
void fgOverlapsFromHits(fg_ctx* c, const fg_detector_params* p, const u32* queryIds, u32 nq, i32 maxOverlaps,
						uint8_t forceLocal, u32 nSrc, const u64* hitCounts, const fg_seed_hit* dHits, fg_overlap_batch* out);
// several contexts of one process behind one handle (fg_group.hip): the frequency sum of a build over the members
// (k_freq_accumulate, on the context's stream; dst 16-byte aligned for the vector path), its test hook, and the
// argument checks fg_overlaps makes before it touches the device
void fgFreqAccumulate(fg_ctx* c, u32* dst, const u32* src, u64 n);
void fgDebugFreqAccumulate(fg_ctx* c, u32* dst, const u32* src, u64 n);
int fgCheckOverlapArgs(const fg_ctx* c, const fg_detector_params* p, const u32* queryIds, u32 nq, i32 maxOverlaps);
// test hooks of the device primitives (fg_devprim.h) on host arrays, every device buffer followed by a guard
void fgDebugScan(fg_ctx* c, void* data, u64 n, int elemBytes, bool inclusive, bool inPlace);
void fgDebugRadixSortPairs(fg_ctx* c, u64* keys, u64* vals, u64 n, int beginBit, int endBit, int* passesRun);
