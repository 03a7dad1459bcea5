// fg_read_coverage / fg_edge_coverage: window coverage of a sequence by alignment intervals and the median of it.
//   reads  ChimeraDetector::getReadCoverage / getCachedCoverage (reference src/assemble/chimera.cpp:106-134, :280-343):
//          per record the windows curBegin / W .. curEnd / W - 2 of one of two vectors (lrOverhang() against
//          maximum_overhang), then what testReadByCoverage (:137-202) folds out of the first: sum, max, median, the
//          minimum over the good range
//   edges  MultiplicityInferer::estimateCoverage (src/repeat_graph/multiplicity_inferer.cpp:14-41, :63): per path element
//          the windows [from, to) of its edge, then sum / max / median per edge
// Integers only; every float of the two functions stays on the host (fg_coverage_windows / fg_coverage_verdict).
//
//   k_cov_iv_reads   one thread per record: the packed interval (from, to, class); a skipped record (:120-121) and a
//                    range that ends below its start become the empty interval
//   k_cov_iv_edges   one thread per path element: key = edge, value = the packed interval (:32-37)
//   (fgprim::radixSortPairs over ceil(log2 n_edges) bits) + k_cov_bounds: the intervals of every edge side by side
//   k_cov_target     one block per target (a read, an edge), 64 threads for the short ones (the bulk of a read set:
//                    about 90 windows and a dozen records) and 256 for the rest.  Per tile of T windows in LDS: zero
//                    two difference arrays, every interval of the target adds the +1 / -1 that fall into the tile with LDS
//                    atomics, barrier, inclusive scan carrying the running sums of the tile before, store, fold.
//                    Then the median of the first vector: the k-th smallest, k = min(n * 50 / 100, n - 1)
//                    (utils.h:32-51), by binary search on the value in [0, max], counting the elements <= v -- from
//                    LDS when the target is one tile, otherwise from the vector just written.
// No global atomic anywhere: a target's block alone writes the target's windows and values, and integer adds in LDS
// commute, so the result is a pure function of the input.
// Cost per target of n windows, r intervals and tiles of T: r * ceil(n / T) interval reads, n window updates and
// n * ceil(log2(max + 1)) <= 31 n value reads for the selection.
#include "fg_ctx.h"
#include "fg_stage.h"
#include "fg_devprim.h"

namespace {

#define COV_BLOCK 256
#define COV_WAVE_CAP 512		// windows of a tile of the 64-thread class (2 arrays of 2 KiB)
#define COV_WG_CAP 2048			// ... of the 256-thread class (2 arrays of 8 KiB)
#define COV_MAX_BLOCKS 16384u	// blocks of k_cov_target; the rest of a list by grid stride
#define COV_NO_MIN 0x7FFFFFFF

// from | to << 31 | class << 62, 0 <= from <= to < 2^31; from == to: empty
__device__ __forceinline__ u64 cov_pack(i32 from, i32 to, u32 cls)
{
	if (to <= from) return 0;
	return (u64)(u32)from | ((u64)(u32)to << 31) | ((u64)cls << 62);
}

// the p < n with off[p] <= g < off[p + 1]
__device__ __forceinline__ u32 cov_seg_of(const u64* __restrict__ off, u32 n, u64 g)
{
	u32 lo = 0, hi = n;
	while (hi - lo > 1)
	{
		const u32 mid = (lo + hi) >> 1;
		if (off[mid] <= g) lo = mid; else hi = mid;
	}
	return lo;
}

// nClip[q]: the windows of query q an interval may touch (0 for a degenerate query, whose one window stays 0)
__global__ void __launch_bounds__(COV_BLOCK)
k_cov_iv_reads(const fg_overlap_rec* __restrict__ recs, const u64* __restrict__ qOff, u32 nq, u64 n, const i32* __restrict__ nClip,
			   i32 window, i32 maxOverhang, u64* __restrict__ iv)
{
	for (u64 g = (u64)blockIdx.x * COV_BLOCK + threadIdx.x; g < n; g += (u64)gridDim.x * COV_BLOCK)
	{
		const fg_overlap_rec r = recs[g];
		u64 o = 0;
		if (r.ext_id != r.cur_id && r.ext_id != (r.cur_id ^ 1u))		// chimera.cpp:120-121
		{
			const i32 clip = nClip[cov_seg_of(qOff, nq, g)];
			// OverlapRange::lrOverhang (overlap.h:195-199)
			const i32 left = r.cur_begin < r.ext_begin ? r.cur_begin : r.ext_begin;
			const i32 rc = r.cur_len - r.cur_end, re = r.ext_len - r.ext_end;
			const i32 right = rc < re ? rc : re;
			const u32 cls = (left > right ? left : right) > maxOverhang ? 1u : 0u;
			// pos - FLANK for pos = curBegin / W + FLANK .. curEnd / W - FLANK, FLANK = 1 (:125-130)
			const i32 from = r.cur_begin / window;
			i32 to = r.cur_end / window - 1;
			if (to > clip) to = clip;
			o = cov_pack(from, to, cls);
		}
		iv[g] = o;
	}
}

// one path element as the host shim leaves it: flags 1 = not the first of its path, 2 = not the last
struct CovEdgeEl { i32 extBegin, extEnd; u32 edge, flags; };

__global__ void __launch_bounds__(COV_BLOCK)
k_cov_iv_edges(const CovEdgeEl* __restrict__ el, u64 n, const u64* __restrict__ winOff, i32 window, u64* __restrict__ keys,
			   u64* __restrict__ iv)
{
	for (u64 g = (u64)blockIdx.x * COV_BLOCK + threadIdx.x; g < n; g += (u64)gridDim.x * COV_BLOCK)
	{
		const CovEdgeEl e = el[g];
		const long long size = (long long)(winOff[e.edge + 1] - winOff[e.edge]);
		// multiplicity_inferer.cpp:32-37
		long long from = (long long)(e.extBegin / window) + 1;
		if (from < 0) from = 0;
		long long to = (long long)(e.extEnd / window);
		if (to > size) to = size;
		if (e.flags & 1u) from = 0;
		if (e.flags & 2u) to = size;
		if (from > size) from = size;
		keys[g] = e.edge;
		iv[g] = cov_pack((i32)from, (i32)to, 0);
	}
}

// ivOff[e] = the first sorted interval whose edge is >= e (e = 0 .. nEdges)
__global__ void __launch_bounds__(COV_BLOCK)
k_cov_bounds(const u64* __restrict__ keys, u64 n, u32 nEdges, u64* __restrict__ ivOff)
{
	for (u64 e = (u64)blockIdx.x * COV_BLOCK + threadIdx.x; e <= nEdges; e += (u64)gridDim.x * COV_BLOCK)
	{
		u64 lo = 0, hi = n;
		while (lo < hi)
		{
			const u64 mid = (lo + hi) >> 1;
			if (keys[mid] < e) lo = mid + 1; else hi = mid;
		}
		ivOff[e] = lo;
	}
}

__device__ __forceinline__ long long cov_shfl_xor(long long v, int o)
{
	const u32 lo = __shfl_xor((u32)v, o), hi = __shfl_xor((u32)((u64)v >> 32), o);
	return (long long)(((u64)hi << 32) | lo);
}

// sums, maxima and minima over the block, to every thread; sh: NT / 64 entries per call site, reused after the barrier
template <int NT>
__device__ __forceinline__ long long cov_block_sum(long long v, long long* sh)
{
	for (int o = 32; o > 0; o >>= 1) v += cov_shfl_xor(v, o);
	if (NT == 64) return v;
	if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
	__syncthreads();
	long long r = 0;
	for (int w = 0; w < NT / 64; ++w) r += sh[w];
	__syncthreads();
	return r;
}

template <int NT, bool MAX>
__device__ __forceinline__ i32 cov_block_ext(i32 v, long long* sh)
{
	for (int o = 32; o > 0; o >>= 1)
	{
		const i32 t = __shfl_xor(v, o);
		if (MAX ? t > v : t < v) v = t;
	}
	if (NT == 64) return v;
	if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
	__syncthreads();
	i32 r = (i32)sh[0];
	for (int w = 1; w < NT / 64; ++w)
	{
		const i32 t = (i32)sh[w];
		if (MAX ? t > r : t < r) r = t;
	}
	__syncthreads();
	return r;
}

// the difference array d[0 .. len) becomes its running sum + carry; returns the last value (to every thread).
// Thread t owns the `items` consecutive elements behind t * items.
template <int NT>
__device__ __forceinline__ i32 cov_tile_scan(i32* d, int len, int items, i32 carry, long long* sh)
{
	const int tid = threadIdx.x, lane = tid & 63;
	const int a = tid * items < len ? tid * items : len;
	const int b = a + items < len ? a + items : len;
	i32 mine = 0;
	for (int i = a; i < b; ++i) mine += d[i];
	i32 incl = mine;
	for (int o = 1; o < 64; o <<= 1)
	{
		const i32 t = __shfl_up(incl, o);
		if (lane >= o) incl += t;
	}
	i32 before = incl - mine, total = __shfl(incl, 63);
	if (NT > 64)
	{
		if (lane == 63) sh[tid >> 6] = incl;
		__syncthreads();
		total = 0;
		for (int w = 0; w < NT / 64; ++w)
		{
			if (w < (tid >> 6)) before += (i32)sh[w];
			total += (i32)sh[w];
		}
		__syncthreads();
	}
	i32 run = carry + before;
	for (int i = a; i < b; ++i) { run += d[i]; d[i] = run; }
	return carry + total;
}

// list: the targets of this launch; target t: intervals iv[ivOff[t] .. ivOff[t + 1]), windows winOff[t] ..
// winOff[t + 1] of full / junction (junction may be null: one class).  maxFlank < 0: no good range.  storeAll: the
// vectors are wanted; otherwise `full` is written only for a target of several tiles, as the selection's scratch.
// stat: max, median, min over the good range.
template <int NT, int CAP>
__global__ void __launch_bounds__(NT)
k_cov_target(const u32* __restrict__ list, u32 nList, const u64* __restrict__ ivOff, const u64* __restrict__ iv,
			 const u64* __restrict__ winOff, int tile, i32 maxFlank, int storeAll, i32* __restrict__ full, i32* __restrict__ junction,
			 long long* __restrict__ sum, i32* __restrict__ stat)
{
	__shared__ i32 sF[CAP], sJ[CAP];
	__shared__ long long sh[NT / 64];
	const int tid = threadIdx.x;
	if (tile > CAP) tile = CAP;
	if (tile < 1) tile = 1;
	const int items = (tile + NT - 1) / NT;
	for (u32 li = blockIdx.x; li < nList; li += gridDim.x)
	{
		const u32 t = fg_uni(list[li]);
		const u64 a = fg_uni(ivOff[t]), b = fg_uni(ivOff[t + 1]);
		const u64 w0 = fg_uni(winOff[t]);
		const long long nW = (long long)(fg_uni(winOff[t + 1]) - w0);
		const bool oneTile = nW <= tile;
		const bool store = storeAll || !oneTile;
		const long long goodLo = maxFlank, goodHi = maxFlank < 0 ? -1 : nW - maxFlank - 1;
		long long mySum = 0;
		i32 myMax = 0, myMin = COV_NO_MIN;
		i32 carryF = 0, carryJ = 0;
		for (long long t0 = 0; t0 < nW; t0 += tile)
		{
			const int len = (int)(nW - t0 < tile ? nW - t0 : tile);
			for (int i = tid; i < len; i += NT) { sF[i] = 0; sJ[i] = 0; }
			__syncthreads();
			for (u64 k = a + tid; k < b; k += NT)
			{
				const u64 v = iv[k];
				long long from = (long long)(v & 0x7FFFFFFFu), to = (long long)((v >> 31) & 0x7FFFFFFFu);
				if (to > nW) to = nW;
				if (from >= to) continue;
				// the running sum carried in from the tile before holds every interval that began there: a tile adds only
				// the starts and the ends that fall inside it (an end on the tile's first window belongs to this tile)
				const int lo = from >= t0 && from < t0 + len ? (int)(from - t0) : -1;
				const int hi = to >= t0 && to < t0 + len ? (int)(to - t0) : -1;
				if (v >> 62)
				{
					if (lo >= 0) atomicAdd(&sJ[lo], 1);
					if (hi >= 0) atomicAdd(&sJ[hi], -1);
				}
				else
				{
					if (lo >= 0) atomicAdd(&sF[lo], 1);
					if (hi >= 0) atomicAdd(&sF[hi], -1);
				}
			}
			__syncthreads();
			carryF = cov_tile_scan<NT>(sF, len, items, carryF, sh);
			if (junction) carryJ = cov_tile_scan<NT>(sJ, len, items, carryJ, sh);
			__syncthreads();
			for (int i = tid; i < len; i += NT)
			{
				const i32 v = sF[i];
				const long long w = t0 + i;
				mySum += v;
				if (v > myMax) myMax = v;
				if (w >= goodLo && w <= goodHi && v < myMin) myMin = v;
				if (store) full[w0 + w] = v;
				if (storeAll && junction) junction[w0 + w] = sJ[i];
			}
			if (!oneTile) __syncthreads();		// the tile is read before the next one zeroes it
		}
		const long long total = cov_block_sum<NT>(mySum, sh);
		const i32 mx = cov_block_ext<NT, true>(myMax, sh);
		const i32 mn = cov_block_ext<NT, false>(myMin, sh);
		// utils.h:32-51: sorted[min(n * 50 / 100, n - 1)], 0 for an empty vector: the smallest v with k + 1 elements <= v
		i32 lo = 0, hi = mx;
		if (nW > 0)
		{
			const long long half = (long long)((u64)nW * 50u / 100u);
			const long long k = half < nW - 1 ? half : nW - 1;
			__syncthreads();					// the last tile's stores before the loads below
			while (lo < hi)
			{
				const i32 mid = lo + (hi - lo) / 2;
				long long cnt = 0;
				if (oneTile) { for (int i = tid; i < (int)nW; i += NT) cnt += sF[i] <= mid; }
				else { for (long long i = tid; i < nW; i += NT) cnt += full[w0 + i] <= mid; }
				cnt = cov_block_sum<NT>(cnt, sh);
				if (cnt >= k + 1) hi = mid; else lo = mid + 1;
			}
		}
		if (tid == 0)
		{
			sum[t] = total;
			stat[3 * (u64)t] = mx; stat[3 * (u64)t + 1] = lo; stat[3 * (u64)t + 2] = mn;
		}
		__syncthreads();						// sF is read above and zeroed by the next target
	}
}

struct CovSwitches { int tile; i32 waveMax; u64 batchRecs; };

CovSwitches covSwitches()
{
	CovSwitches s{COV_WG_CAP, COV_WAVE_CAP, 1ULL << 20};
	if (const char* e = getenv("FG_COVERAGE_TILE")) s.tile = atoi(e);
	if (const char* e = getenv("FG_COVERAGE_WAVE_MAX")) s.waveMax = atoi(e);
	s.batchRecs = stageEnvU64("FG_COVERAGE_BATCH_RECS", s.batchRecs);
	s.tile = std::min(std::max(s.tile, 64), COV_WG_CAP);
	s.waveMax = std::min(std::max(s.waveMax, 0), COV_WAVE_CAP);
	s.batchRecs = std::min<u64>(std::max<u64>(s.batchRecs, 1), 1ULL << 28);
	return s;
}

// the two launches of k_cov_target over targets 0 .. n - 1 whose offsets are on the device; hWinOff: the same window
// offsets on the host (the class of a target follows its window count).  dList: room for n entries.
void covTargets(fg_ctx* c, const CovSwitches& sw, u32 n, const u64* hWinOff, u32* dList, const u64* dIvOff, const u64* dIv,
				const u64* dWinOff, i32 maxFlank, bool storeAll, i32* dFull, i32* dJunction, long long* dSum, i32* dStat)
{
	hipStream_t s = c->stream;
	std::vector<u32> list(n);
	u32 nWave = 0, nWg = 0;
	for (u32 t = 0; t < n; ++t)
		if (hWinOff[t + 1] - hWinOff[t] <= (u64)sw.waveMax) list[nWave++] = t;
	for (u32 t = 0; t < n; ++t)
		if (hWinOff[t + 1] - hWinOff[t] > (u64)sw.waveMax) list[nWave + nWg++] = t;
	HIP_CHECK(hipMemcpyAsync(dList, list.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
	if (nWave)
	{
		ScopedK t(c->timer, "k_cov_target_wave");
		hipLaunchKernelGGL((k_cov_target<64, COV_WAVE_CAP>), std::min(nWave, COV_MAX_BLOCKS), 64, 0, s, dList, nWave, dIvOff, dIv, dWinOff,
						   std::min(sw.tile, COV_WAVE_CAP), maxFlank, storeAll ? 1 : 0, dFull, dJunction, dSum, dStat);
	}
	if (nWg)
	{
		ScopedK t(c->timer, "k_cov_target_wg");
		hipLaunchKernelGGL((k_cov_target<COV_BLOCK, COV_WG_CAP>), std::min(nWg, COV_MAX_BLOCKS), COV_BLOCK, 0, s, dList + nWave, nWg, dIvOff,
						   dIv, dWinOff, sw.tile, maxFlank, storeAll ? 1 : 0, dFull, dJunction, dSum, dStat);
	}
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipStreamSynchronize(s));		// `list` lives until its copy has run
}

unsigned covGrid(u64 n) { return (unsigned)std::min<u64>(std::max<u64>((n + COV_BLOCK - 1) / COV_BLOCK, 1), 4096); }

} // namespace

// fg_read_coverage behind its argument checks.  recs: the caller's records from query_off[0] on; qOff: nq + 1 offsets
// into them, from 0; winOff: nq + 1 offsets of the queries' windows; nClip: the windows an interval of query q may
// touch.  full / junction (wantVectors): winOff[nq] entries; sum: nq; stat: 3 nq (max, median, min over the good range).
void fgReadCoverage(fg_ctx* c, i32 window, i32 maxOverhang, i32 maxFlank, const fg_overlap_rec* recs, const std::vector<u64>& qOff,
					const std::vector<u64>& winOff, const std::vector<i32>& nClip, bool wantVectors, i32* full, i32* junction,
					long long* sum, i32* stat)
{
	const u32 nq = (u32)(qOff.size() - 1);
	if (!nq) return;
	hipStream_t s = c->stream;
	const CovSwitches sw = covSwitches();
	const u64 maxWin = 1ULL << 24;			// windows of a sub-batch (a query beyond it runs alone)
	c->timer.reset();
	std::vector<u64> local;
	u32 qa = 0;
	while (qa < nq)
	{
		u32 qb = qa + 1;
		while (qb < nq && qOff[qb + 1] - qOff[qa] <= sw.batchRecs && winOff[qb + 1] - winOff[qa] <= maxWin) ++qb;
		const u32 n = qb - qa;
		const u64 r0 = qOff[qa], nRec = qOff[qb] - r0, w0 = winOff[qa], nWin = winOff[qb] - w0;
		local.resize(2 * ((size_t)n + 1));
		for (u32 i = 0; i <= n; ++i) { local[i] = qOff[qa + i] - r0; local[n + 1 + i] = winOff[qa + i] - w0; }
		c->dCovRecs.reserve(nRec * sizeof(fg_overlap_rec));
		c->dCovIv.reserve(nRec);
		c->dCovOff.reserve(3 * (size_t)n + 2);
		c->dCovI32.reserve(5 * (size_t)n);
		c->dCovVec.reserve((wantVectors ? 2 : 1) * nWin);
		u64* dQOff = c->dCovOff.p;
		u64* dWinOff = dQOff + (n + 1);
		long long* dSum = (long long*)(dWinOff + (n + 1));
		i32* dClip = c->dCovI32.p;
		u32* dList = (u32*)(dClip + n);
		i32* dStat = (i32*)(dList + n);
		i32* dFull = c->dCovVec.p;
		i32* dJunction = wantVectors ? dFull + nWin : nullptr;
		HIP_CHECK(hipMemcpyAsync(dQOff, local.data(), local.size() * 8, hipMemcpyHostToDevice, s));		// dWinOff follows it
		HIP_CHECK(hipMemcpyAsync(dClip, nClip.data() + qa, (size_t)n * 4, hipMemcpyHostToDevice, s));
		if (nRec)
		{
			HIP_CHECK(hipMemcpyAsync(c->dCovRecs.p, recs + r0, nRec * sizeof(fg_overlap_rec), hipMemcpyHostToDevice, s));
			ScopedK t(c->timer, "k_cov_intervals");
			hipLaunchKernelGGL(k_cov_iv_reads, covGrid(nRec), COV_BLOCK, 0, s, (const fg_overlap_rec*)c->dCovRecs.p, dQOff, n, nRec, dClip,
							   window, maxOverhang, c->dCovIv.p);
		}
		// without vectors the junction intervals still go to their own LDS array (they must not count), which is then
		// neither summed up nor stored
		covTargets(c, sw, n, local.data() + n + 1, dList, dQOff, c->dCovIv.p, dWinOff, maxFlank, wantVectors, dFull, dJunction, dSum,
				   dStat);
		HIP_CHECK(hipMemcpyAsync(sum + qa, dSum, (size_t)n * 8, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipMemcpyAsync(stat + 3 * (size_t)qa, dStat, 3 * (size_t)n * 4, hipMemcpyDeviceToHost, s));
		if (wantVectors && nWin)
		{
			HIP_CHECK(hipMemcpyAsync(full + w0, dFull, nWin * 4, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipMemcpyAsync(junction + w0, dJunction, nWin * 4, hipMemcpyDeviceToHost, s));
		}
		HIP_CHECK(hipStreamSynchronize(s));
		qa = qb;
	}
	c->timer.collect();
}

// fg_edge_coverage behind its argument checks.  el: one entry per path element; winOff: nEdges + 1 window offsets.
// cov (wantVectors): winOff[nEdges] entries; sum: nEdges; stat: 3 nEdges.
void fgEdgeCoverage(fg_ctx* c, i32 window, const std::vector<FgCovEdgeEl>& el, const std::vector<u64>& winOff, bool wantVectors,
					i32* cov, long long* sum, i32* stat)
{
	static_assert(sizeof(FgCovEdgeEl) == sizeof(CovEdgeEl), "one layout on both sides");
	const u32 nEdges = (u32)(winOff.size() - 1);
	if (!nEdges) return;
	hipStream_t s = c->stream;
	const CovSwitches sw = covSwitches();
	const u64 n = el.size(), nWin = winOff[nEdges];
	c->timer.reset();
	c->dCovRecs.reserve(n * sizeof(CovEdgeEl));
	c->dCovIv.reserve(2 * n);
	c->dCovKeys.reserve(2 * n);
	c->dCovSort.reserve(fgprim::radixSortScratchBytes(n));
	c->dCovOff.reserve(3 * (size_t)nEdges + 2);
	c->dCovI32.reserve(4 * (size_t)nEdges);
	c->dCovVec.reserve(nWin);
	u64* dIvOff = c->dCovOff.p;
	u64* dWinOff = dIvOff + (nEdges + 1);
	long long* dSum = (long long*)(dWinOff + (nEdges + 1));
	u32* dList = (u32*)c->dCovI32.p;
	i32* dStat = (i32*)(dList + nEdges);
	u64* k0 = c->dCovKeys.p;
	u64* k1 = k0 + n;
	u64* v0 = c->dCovIv.p;
	u64* v1 = v0 + n;
	HIP_CHECK(hipMemcpyAsync(dWinOff, winOff.data(), ((size_t)nEdges + 1) * 8, hipMemcpyHostToDevice, s));
	int at = 0;
	if (n)
	{
		HIP_CHECK(hipMemcpyAsync(c->dCovRecs.p, el.data(), n * sizeof(CovEdgeEl), hipMemcpyHostToDevice, s));
		{
			ScopedK t(c->timer, "k_cov_intervals");
			hipLaunchKernelGGL(k_cov_iv_edges, covGrid(n), COV_BLOCK, 0, s, (const CovEdgeEl*)c->dCovRecs.p, n, dWinOff, window, k0, v0);
		}
		int bits = 0;
		while ((1ULL << bits) < (u64)nEdges) ++bits;
		ScopedK t(c->timer, "k_cov_sort");
		at = fgprim::radixSortPairs(s, k0, v0, k1, v1, n, 0, bits, c->dCovSort.p);
	}
	{
		ScopedK t(c->timer, "k_cov_bounds");
		hipLaunchKernelGGL(k_cov_bounds, covGrid((u64)nEdges + 1), COV_BLOCK, 0, s, at ? k1 : k0, n, nEdges, dIvOff);
	}
	covTargets(c, sw, nEdges, winOff.data(), dList, dIvOff, at ? v1 : v0, dWinOff, -1, wantVectors, c->dCovVec.p, nullptr, dSum, dStat);
	HIP_CHECK(hipMemcpyAsync(sum, dSum, (size_t)nEdges * 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipMemcpyAsync(stat, dStat, 3 * (size_t)nEdges * 4, hipMemcpyDeviceToHost, s));
	if (wantVectors && nWin) HIP_CHECK(hipMemcpyAsync(cov, c->dCovVec.p, nWin * 4, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	c->timer.collect();
}
