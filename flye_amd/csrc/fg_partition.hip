// fg_confirm_positions / fg_classify_reads: Trestle's partition_reads (flye/trestle/trestle.py:1075-1142) on the device:
// _evaluate_positions (:1360-1473) and _classify_reads with _index_mapping (:1539-1628).  Integers only.
//
// Both calls cut alignments into tiles of PT tile columns (FG_PARTITION_TILE, default 1024) over ALL alignments of a
// sub-batch of whole jobs (FG_PARTITION_BATCH_COLS), as k_dv_tiles / k_dv_count do:
//   k_pt_tiles      one wave per tile: its non-gap target columns (and, for confirm, its non-gap query columns).  An
//                   exclusive scan over all tiles gives, minus the value at the alignment's first tile, the tile's base.
// fg_confirm_positions, per sub-batch:
//   k_bub_shift     (fg_gapshift.h) both shift_gaps passes, every edge alignment.
//   k_cf_edge       one wave per tile: per non-gap target column its rank r (ballot prefix count from the tile's base);
//                   the query byte and qry_start + the non-gap query bytes before the column go to slot (edge, r).
//   k_cf_mark       one thread per entry of the four tentative lists: a bit per list in the job's position table.
//   k_cf_judge      one thread per position of [min_start, max_end): the walk over the job's edges in order; a byte of
//                   list memberships per position, and per (edge, r) how many entries the edge's consensus_pos takes.
//   (scan)          exclusive sums over the eight list flags and the entry counts; k_cf_compact / k_cf_cons write the
//                   ascending lists, k_pt_pick takes the lists' starts per job and per edge.
// fg_classify_reads, per sub-batch:
//   k_cl_poscount   one thread per entry of the edges' consensus_pos lists: an integer atomicAdd into the edge's count
//                   array over [smallest trg_start, largest trg_end) of its alignments: exact for any multiplicity.
//   k_cl_score      one wave per tile: rank by ballot and popcount, the position's multiplicity where the bytes are equal,
//                   one wave reduction and at most one integer atomicAdd per wave into the alignment's score.
//   k_cl_keys       key = (read of the sub-batch << edge bits | edge), value = alignment; the stable radix sort of
//                   fg_devprim.h leaves every read's alignments together, by edge, in list order.
//   k_cl_vote       one lane per read: its groups of equal keys are its edges; a group of one or two keeps the score of
//                   its last alignment, a larger one 0 (the reference's reset rule); then the vote of :1578-1596.
// Integer atomics only: the result does not depend on the schedule.  The host does work proportional to jobs, edges,
// alignments and (for the byte check) columns.
//
// fg_classify_reads_cigars takes SAM records for the columns, the alignments of edge e lying on contig e (the edge's own
// consensus): a sub-batch of whole jobs expands its own alignments (fg_cigexpand.h) into the buffers k_pt_tiles and
// k_cl_score read.
#include "fg_ctx.h"
#include "fg_stage.h"
#include "fg_devprim.h"
#include "fg_gapshift.h"
#include "fg_cigexpand.h"

namespace {

// base: confirm, the edge's first slot; classify, the edge's first count cell, which stands for position minPos
struct PtAln { u64 colOff; u32 nCols; i32 trgStart; i32 trgEnd; i32 qryStart; u32 base; i32 minPos; u32 edge; u32 gread; };
struct CfJob { u64 posAt; u32 edge0; u32 nEdges; i32 minStart; i32 maxEnd; i32 minEnd; i32 maxStart; u32 side; u32 pad; };
struct ClEdge { u32 cntBase; i32 minPos; i32 maxEnd; u32 pad; };

// the last i in [0, n) with off[i] <= x (off ascending, off[0] <= x)
template <class T>
__device__ __forceinline__ u32 pt_find(const T* __restrict__ off, u32 n, u64 x)
{
	u32 lo = 0, hi = n;
	while (hi - lo > 1)
	{
		const u32 mid = (lo + hi) >> 1;
		if ((u64)off[mid] <= x) lo = mid; else hi = mid;
	}
	return lo;
}

template <bool QRY>
__global__ void __launch_bounds__(BUB_BLOCK)
k_pt_tiles(const PtAln* __restrict__ alns, u32 nAln, const u32* __restrict__ tileOff, u32 nTiles, u32 tileShift,
		   const unsigned char* __restrict__ trg, const unsigned char* __restrict__ qry, u32* __restrict__ tileNg, u32* __restrict__ tileNq)
{
	const int lane = threadIdx.x & 63;
	const u32 w = blockIdx.x * BUB_WAVES + (threadIdx.x >> 6);
	if (w >= nTiles) return;
	const u32 a = pt_find(tileOff, nAln, w);
	const PtAln al = alns[a];
	const unsigned char* t = trg + al.colOff;
	const unsigned char* q = qry + al.colOff;
	const u32 c0 = (w - tileOff[a]) << tileShift, c1 = min(c0 + (1u << tileShift), al.nCols);
	u32 ng = 0, nq = 0;
	for (u32 c = c0; c < c1; c += 64)
	{
		const u32 i = c + lane;
		ng += (u32)__popcll(__ballot(i < c1 && t[i] != '-'));
		if (QRY) nq += (u32)__popcll(__ballot(i < c1 && q[i] != '-'));
	}
	if (lane == 0)
	{
		tileNg[w] = ng;
		if (QRY) tileNq[w] = nq;
	}
}

// row k of out = off[k * stride + at[i]]
template <class T>
__global__ void __launch_bounds__(BUB_BLOCK)
k_pt_pick(u32 n, const T* __restrict__ at, const u32* __restrict__ off, u64 stride, u32 rows, u32* __restrict__ out)
{
	const u32 i = blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (i >= n) return;
	const u64 p = at[i];
	for (u32 k = 0; k < rows; ++k) out[(u64)k * n + i] = off[(u64)k * stride + p];
}

// ---- fg_confirm_positions ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BUB_BLOCK)
k_cf_edge(const PtAln* __restrict__ alns, u32 nAln, const u32* __restrict__ tileOff, u32 nTiles, u32 tileShift,
		  const u32* __restrict__ tileNg, const u32* __restrict__ tileNq, const unsigned char* __restrict__ trg,
		  const unsigned char* __restrict__ qry, unsigned char* __restrict__ nucQ, i32* __restrict__ qInd)
{
	const int lane = threadIdx.x & 63;
	const u32 w = blockIdx.x * BUB_WAVES + (threadIdx.x >> 6);
	if (w >= nTiles) return;
	const u32 a = pt_find(tileOff, nAln, w);
	const PtAln al = alns[a];
	const unsigned char* t = trg + al.colOff;
	const unsigned char* q = qry + al.colOff;
	const u64 below = bub_below(lane);
	const u32 c0 = (w - tileOff[a]) << tileShift, c1 = min(c0 + (1u << tileShift), al.nCols);
	u32 baseR = tileNg[w] - tileNg[tileOff[a]], baseQ = tileNq[w] - tileNq[tileOff[a]];
	for (u32 cc = c0; cc < c1; cc += 64)
	{
		const u32 i = cc + lane;
		const bool valid = i < c1;
		const unsigned char tb = valid ? t[i] : (unsigned char)'-', qb = valid ? q[i] : (unsigned char)'-';
		const bool ng = valid && tb != '-';
		const u64 mg = __ballot(ng), mq = __ballot(valid && qb != '-');
		if (ng)
		{
			// r < trg_end - trg_start: the host has counted the non-gap target columns
			const u64 at = (u64)al.base + baseR + (u32)__popcll(mg & below);
			nucQ[at] = qb;
			qInd[at] = (i32)((long long)al.qryStart + (long long)(baseQ + (u32)__popcll(mq & below)));
		}
		baseR += (u32)__popcll(mg);
		baseQ += (u32)__popcll(mq);
	}
}

// entries [segOff[k * nJ + j], segOff[k * nJ + j + 1]) are list k of job j
__global__ void __launch_bounds__(BUB_BLOCK)
k_cf_mark(u32 nEntries, const u32* __restrict__ segOff, u32 nJ, const i32* __restrict__ pos, const CfJob* __restrict__ jobs, u32* mark)
{
	const u32 i = blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (i >= nEntries) return;
	const u32 seg = pt_find(segOff, 4 * nJ, i);
	const CfJob jb = jobs[seg % nJ];
	const i32 t = pos[i];
	if (t >= jb.minStart && t < jb.maxEnd) atomicOr(&mark[jb.posAt + (u64)((long long)t - jb.minStart)], 1u << (seg / nJ));
}

// lists: bit k of code = confirmed total, sub, del, ins, rejected total, sub, del, ins
__global__ void __launch_bounds__(BUB_BLOCK)
k_cf_judge(u32 nPos, const CfJob* __restrict__ jobs, u32 nJ, const u64* __restrict__ jobAt, const PtAln* __restrict__ alns,
		   const u32* __restrict__ mark, const unsigned char* __restrict__ nucQ, const i32* __restrict__ qInd,
		   unsigned char* __restrict__ consCode, u32* __restrict__ consCnt, unsigned char* __restrict__ code, u32* __restrict__ is /* 8 x (nPos + 1) */)
{
	const u32 g = blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (g > nPos) return;
	const u64 stride = (u64)nPos + 1;
	if (g == nPos)
	{
		for (int k = 0; k < 8; ++k) is[k * stride + g] = 0;
		return;
	}
	const u32 j = pt_find(jobAt, nJ, g);
	const CfJob jb = jobs[j];
	const long long t = (long long)jb.minStart + (long long)(g - jb.posAt);
	const u32 mk = mark[g];
	u32 out = 0;
	if ((mk & 1u) && (jb.side == 0 ? t < jb.minEnd : t >= jb.maxStart))
	{
		bool insC = false, delC = false, subC = false, haveRef = false;
		unsigned char ref = 0;
		for (u32 e = jb.edge0; e < jb.edge0 + jb.nEdges; ++e)
		{
			const PtAln al = alns[e];
			if (t < al.trgStart || t >= al.trgEnd) continue;
			const u64 at = (u64)al.base + (u64)(t - al.trgStart);
			const unsigned char nq = nucQ[at];
			const i32 qi = qInd[at];
			const bool hasIns = t == al.trgStart ? qi != al.qryStart : (qi - qInd[at - 1] - (nucQ[at - 1] != '-' ? 1 : 0)) > 0;
			insC = insC || hasIns;
			consCode[at] = hasIns ? 1 : 0;
			if (!haveRef) { ref = nq; haveRef = true; }
			else if (nq != ref && ref != 'N' && nq != 'N') { if (ref == '-') delC = true; else subC = true; }
		}
		const bool ds = delC || subC;
		for (u32 e = jb.edge0; e < jb.edge0 + jb.nEdges; ++e)
		{
			const PtAln al = alns[e];
			if (t < al.trgStart || t >= al.trgEnd) continue;
			const u64 at = (u64)al.base + (u64)(t - al.trgStart);
			const unsigned char cc = (unsigned char)(consCode[at] | (ds ? 2 : 0));
			consCode[at] = cc;
			consCnt[at] = (cc & 1u) + (cc >> 1);
		}
		const bool f[3] = {subC, delC, insC};
		if (insC || ds)
		{
			out = 1u;
			for (int k = 0; k < 3; ++k)
				if (mk & (2u << k)) out |= f[k] ? (2u << k) : (32u << k);
		}
		else out = 16u | ((mk & 14u) << 4);
	}
	code[g] = (unsigned char)out;
	for (int k = 0; k < 8; ++k) is[k * stride + g] = (out >> k) & 1u;
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_cf_compact(u32 nPos, const CfJob* __restrict__ jobs, u32 nJ, const u64* __restrict__ jobAt, const unsigned char* __restrict__ code,
			 const u32* __restrict__ off /* 8 x (nPos + 1), scanned */, const u32* __restrict__ listAt /* 8 */, i32* __restrict__ lists)
{
	const u32 g = blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (g >= nPos) return;
	const u32 cd = code[g];
	if (!cd) return;
	const CfJob jb = jobs[pt_find(jobAt, nJ, g)];
	const i32 t = (i32)((long long)jb.minStart + (long long)(g - jb.posAt));
	for (int k = 0; k < 8; ++k)
		if (cd & (1u << k)) lists[(u64)listAt[k] + off[(u64)k * (nPos + 1) + g]] = t;
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_cf_cons(u32 nSlots, const unsigned char* __restrict__ consCode, const u32* __restrict__ off, const i32* __restrict__ qInd, i32* __restrict__ cons)
{
	const u32 g = blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (g >= nSlots) return;
	const u32 cc = consCode[g];
	if (!cc) return;
	u32 o = off[g];
	const i32 qi = qInd[g];
	if (cc & 1u) cons[o++] = qi - 1;
	if (cc & 2u) cons[o] = qi;
}

// ---- fg_classify_reads ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BUB_BLOCK)
k_cl_poscount(u32 nEntries, const u64* __restrict__ edgePosAt, u32 nE, const ClEdge* __restrict__ edges, const i32* __restrict__ pos, u32* cnt)
{
	const u32 i = blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (i >= nEntries) return;
	const ClEdge ed = edges[pt_find(edgePosAt, nE, i)];
	const i32 p = pos[i];
	if (p >= ed.minPos && p < ed.maxEnd) atomicAdd(&cnt[(u64)ed.cntBase + (u64)((long long)p - ed.minPos)], 1u);
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_cl_score(const PtAln* __restrict__ alns, u32 nAln, const u32* __restrict__ tileOff, u32 nTiles, u32 tileShift,
		   const u32* __restrict__ tileBase, const unsigned char* __restrict__ trg, const unsigned char* __restrict__ qry,
		   const u32* __restrict__ cnt, u32* alnScore)
{
	const int lane = threadIdx.x & 63;
	const u32 w = blockIdx.x * BUB_WAVES + (threadIdx.x >> 6);
	if (w >= nTiles) return;
	const u32 a = pt_find(tileOff, nAln, w);
	const PtAln al = alns[a];
	const unsigned char* t = trg + al.colOff;
	const unsigned char* q = qry + al.colOff;
	const u64 below = bub_below(lane);
	const u32 c0 = (w - tileOff[a]) << tileShift, c1 = min(c0 + (1u << tileShift), al.nCols);
	// the cell of the alignment's first position; a rank stays below trg_end - trg_start (the host has counted)
	const u32* row = cnt + al.base + (u32)((long long)al.trgStart - al.minPos);
	u32 base = tileBase[w] - tileBase[tileOff[a]];
	u32 sum = 0;
	for (u32 cc = c0; cc < c1; cc += 64)
	{
		const u32 i = cc + lane;
		const bool valid = i < c1;
		const unsigned char tb = valid ? t[i] : (unsigned char)'-', qb = valid ? q[i] : (unsigned char)'-';
		const bool ng = valid && tb != '-';
		const u64 m = __ballot(ng);
		if (ng && tb == qb) sum += row[base + (u32)__popcll(m & below)];
		base += (u32)__popcll(m);
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
	if (lane == 0 && sum) atomicAdd(&alnScore[a], sum);
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_cl_keys(const PtAln* __restrict__ alns, u32 nAln, u32 eBits, u64* __restrict__ keys, u64* __restrict__ vals)
{
	const u32 a = blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (a >= nAln) return;
	keys[a] = ((u64)alns[a].gread << eBits) | alns[a].edge;
	vals[a] = a;
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_cl_vote(u32 nReads, const u64* __restrict__ readAt, u32 nJ, const u32* __restrict__ jobEdge0, const u64* __restrict__ keys,
		  const u64* __restrict__ vals, u32 nAln, u32 eBits, const u32* __restrict__ alnScore, i32 bufferCount,
		  unsigned char* __restrict__ counted, unsigned char* __restrict__ status, i32* __restrict__ topEdge, i32* __restrict__ topScore,
		  i32* __restrict__ totalScore)
{
	const u32 g = blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (g >= nReads) return;
	const u64 first = (u64)g << eBits;
	u32 lo = 0, hi = nAln;			// the first key >= first
	while (lo < hi)
	{
		const u32 mid = (lo + hi) >> 1;
		if (keys[mid] < first) lo = mid + 1; else hi = mid;
	}
	const long long bc = bufferCount;
	long long top = 0, total = 0, edge = -1;
	bool tie = false, any = false;
	u32 i = lo;
	while (i < nAln && (keys[i] >> eBits) == g)
	{
		const u64 key = keys[i];
		const u32 k0 = i;
		while (i < nAln && keys[i] == key) ++i;
		const bool kept = i - k0 <= 2;
		for (u32 k = k0; k < i; ++k) counted[vals[k]] = kept && k == i - 1 ? 1 : 0;
		const long long s = kept ? (long long)alnScore[vals[i - 1]] : 0;
		if (s - bc > top) { edge = (long long)(key & ((1ULL << eBits) - 1)); top = s; tie = false; }
		else if (s >= top) { top = s; tie = true; }			// s - bc <= top holds here
		else if (s >= top - bc) tie = true;					// s < top holds here
		total += s;
		any = true;
	}
	const unsigned char st = !any || total == 0 ? 0 : tie ? 1 : 2;
	status[g] = st;
	topEdge[g] = st == 2 ? (i32)(edge - (long long)jobEdge0[pt_find(readAt, nJ, g)]) : -1;
	topScore[g] = (i32)top;
	totalScore[g] = (i32)total;
}

// ---- the host ---------------------------------------------------------------------------------------------------
template <class T>
void ptUp(hipStream_t s, T* dst, const std::vector<T>& src)
{
	if (!src.empty()) HIP_CHECK(hipMemcpyAsync(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, s));
}

struct PtCut { u64 budget, maxJobs; u32 tileShift; };

PtCut ptCut(const std::string& name)
{
	PtCut cut;
	cut.budget = stageEnvU64("FG_PARTITION_BATCH_COLS", 1ULL << 27);
	cut.maxJobs = stageEnvCap("FG_PARTITION_BATCH_JOBS");
	const u64 tile = stageEnvU64("FG_PARTITION_TILE", 1024);
	if (tile < 64 || tile > 4096 || (tile & (tile - 1)))
		throw FgError{FG_ERR_ARG, name + ": FG_PARTITION_TILE is " + std::to_string(tile) + ", not a power of two in 64 .. 4096"};
	cut.tileShift = 0;
	while ((1ULL << cut.tileShift) < tile) ++cut.tileShift;
	return cut;
}

// per alignment: the bytes below 128 and the non-gap target columns against trg_end - trg_start
void ptCheckColumns(const std::string& name, u64 a, const int32_t* trgStart, const int32_t* trgEnd, const uint64_t* colOff,
					const uint8_t* trgCols, const uint8_t* qryCols)
{
	if (trgStart[a] < 0) throw FgError{FG_ERR_ARG, name + ": trg_start < 0 at alignment " + std::to_string(a)};
	const u64 nonGap = stageColumnWalk(name, a, colOff, trgCols, qryCols);
	if ((long long)nonGap != (long long)trgEnd[a] - (long long)trgStart[a])
		throw FgError{FG_ERR_ARG, name + ": alignment " + std::to_string(a) + " has " + std::to_string(nonGap) +
									  " non-gap target columns, trg_end - trg_start is " +
									  std::to_string((long long)trgEnd[a] - (long long)trgStart[a])};
}

// tiles of the alignments of a sub-batch: tileOff[a] (n + 1 entries)
u64 ptTiles(const std::vector<PtAln>& alns, u32 tileShift, std::vector<u32>& tileOff)
{
	u64 nTiles = 0;
	tileOff.assign(alns.size() + 1, 0);
	for (size_t a = 0; a < alns.size(); ++a)
	{
		tileOff[a] = (u32)nTiles;
		nTiles += ((u64)alns[a].nCols + (1ULL << tileShift) - 1) >> tileShift;
	}
	tileOff[alns.size()] = (u32)nTiles;
	return nTiles;
}

struct ConfirmOwner {
	std::vector<uint64_t> listOff[8], consOff;
	std::vector<int32_t> list[8], cons;
};

struct ConfirmIn {
	const uint8_t* side; const uint64_t* jobEdgeOff; const int32_t *trgStart, *trgEnd, *qryStart; const uint64_t* colOff;
	const uint8_t *trgCols, *qryCols; const uint64_t* listOff[4]; const int32_t* listPos[4];
};

void cfSubBatch(fg_ctx* c, u32 j0, u32 j1, const ConfirmIn& in, const std::vector<CfJob>& allJobs, u32 tileShift, ConfirmOwner& own)
{
	hipStream_t s = c->stream;
	const u32 nJ = j1 - j0;
	const u64 e0 = in.jobEdgeOff[j0], e1 = in.jobEdgeOff[j1];
	const u32 nE = (u32)(e1 - e0);
	const u64 col0 = in.colOff[e0], nCols = in.colOff[e1] - col0;

	std::vector<CfJob> jobs(nJ);
	std::vector<u64> jobAt((size_t)nJ + 1), slotAt((size_t)nE + 1);
	std::vector<PtAln> alns(nE);
	std::vector<BubAln> bub(nE);
	u64 nPos = 0, nSlots = 0;
	for (u32 j = 0; j < nJ; ++j)
	{
		jobs[j] = allJobs[j0 + j];
		jobs[j].posAt = nPos;
		jobs[j].edge0 = (u32)(in.jobEdgeOff[j0 + j] - e0);
		jobAt[j] = nPos;
		nPos += (u64)((long long)jobs[j].maxEnd - jobs[j].minStart);
	}
	jobAt[nJ] = nPos;
	for (u64 e = e0; e < e1; ++e)
	{
		PtAln& al = alns[e - e0];
		al.colOff = in.colOff[e] - col0; al.nCols = (u32)(in.colOff[e + 1] - in.colOff[e]);
		al.trgStart = in.trgStart[e]; al.trgEnd = in.trgEnd[e]; al.qryStart = in.qryStart[e];
		al.base = (u32)nSlots; al.minPos = 0; al.edge = (u32)(e - e0); al.gread = 0;
		slotAt[e - e0] = nSlots;
		nSlots += (u64)(in.trgEnd[e] - in.trgStart[e]);
		bub[e - e0] = BubAln{al.colOff, al.nCols, al.trgStart, al.trgEnd, 0, 1, 0};
	}
	slotAt[nE] = nSlots;
	std::vector<u32> tileOff;
	const u64 nTiles = ptTiles(alns, tileShift, tileOff);
	// the four tentative lists of the jobs, list after list
	std::vector<u32> segOff((size_t)4 * nJ + 1);
	u64 nEntries = 0;
	for (int k = 0; k < 4; ++k)
		for (u32 j = 0; j < nJ; ++j)
		{
			segOff[(size_t)k * nJ + j] = (u32)nEntries;
			nEntries += in.listOff[k][j0 + j + 1] - in.listOff[k][j0 + j];
		}
	if (nPos >= (1ULL << 31) || nSlots >= (1ULL << 31) || nCols >= (1ULL << 31) || nEntries >= (1ULL << 31) || nTiles >= (1ULL << 31))
		throw FgError{FG_ERR_NOMEM, "fg_confirm_positions: a sub-batch of 2^31 positions, columns or list entries; lower FG_PARTITION_BATCH_COLS"};
	segOff[(size_t)4 * nJ] = (u32)nEntries;

	DevPool B{c->dPt, "fg_partition"};
	CfJob* dJobs = B.get<CfJob>(nJ);
	u64* dJobAt = B.get<u64>((size_t)nJ + 1);
	u64* dSlotAt = B.get<u64>((size_t)nE + 1);
	PtAln* dAln = B.get<PtAln>(nE);
	BubAln* dBub = B.get<BubAln>(nE);
	u32* dTileOff = B.get<u32>((size_t)nE + 1);
	u32* dSegOff = B.get<u32>((size_t)4 * nJ + 1);
	i32* dEntries = B.get<i32>(nEntries);
	u32* dTileN = B.get<u32>(2 * (nTiles + 1));
	unsigned char* dTrg = B.get<unsigned char>(nCols);
	unsigned char* dQry = B.get<unsigned char>(nCols);
	unsigned char* dTrgS = B.get<unsigned char>(nCols);
	unsigned char* dQryS = B.get<unsigned char>(nCols);
	unsigned char* dNucQ = B.get<unsigned char>(nSlots);
	i32* dQInd = B.get<i32>(nSlots);
	unsigned char* dConsCode = B.get<unsigned char>(nSlots);
	u32* dConsCnt = B.get<u32>(nSlots + 1);
	u32* dMark = B.get<u32>(nPos);
	unsigned char* dCode = B.get<unsigned char>(nPos);
	u32* dIs = B.get<u32>(8 * (nPos + 1));
	u32* dScan = B.get<u32>(fgprim::scanScratchElems(std::max<u64>(std::max<u64>(nPos + 1, nSlots + 1), nTiles + 1)) + 8);
	u32* dPick = B.get<u32>(8 * ((size_t)nJ + 1) + (size_t)nE + 1 + 8);
	u32 *dTileNg = dTileN, *dTileNq = dTileN + nTiles + 1;

	ptUp(s, dJobs, jobs); ptUp(s, dJobAt, jobAt); ptUp(s, dSlotAt, slotAt); ptUp(s, dAln, alns); ptUp(s, dBub, bub);
	ptUp(s, dTileOff, tileOff); ptUp(s, dSegOff, segOff);
	u64 at = 0;
	for (int k = 0; k < 4; ++k)
	{
		const u64 lo = in.listOff[k][j0], n = in.listOff[k][j1] - lo;
		if (n) HIP_CHECK(hipMemcpyAsync(dEntries + at, in.listPos[k] + lo, n * 4, hipMemcpyHostToDevice, s));
		at += n;
	}
	if (nCols)
	{
		HIP_CHECK(hipMemcpyAsync(dTrg, in.trgCols + col0, nCols, hipMemcpyHostToDevice, s));
		HIP_CHECK(hipMemcpyAsync(dQry, in.qryCols + col0, nCols, hipMemcpyHostToDevice, s));
	}
	HIP_CHECK(hipMemsetAsync(dTileN, 0, 2 * (nTiles + 1) * 4, s));
	HIP_CHECK(hipMemsetAsync(dConsCode, 0, nSlots + 1, s));
	HIP_CHECK(hipMemsetAsync(dConsCnt, 0, (nSlots + 1) * 4, s));
	HIP_CHECK(hipMemsetAsync(dMark, 0, nPos * 4 + 4, s));

	{
		ScopedK t(c->timer, "k_bub_shift");
		hipLaunchKernelGGL(k_bub_shift, bubWaveGrid(nE), BUB_BLOCK, 0, s, dBub, nE, dTrg, dQry, dQryS);
		hipLaunchKernelGGL(k_bub_shift, bubWaveGrid(nE), BUB_BLOCK, 0, s, dBub, nE, dQryS, dTrg, dTrgS);
	}
	if (nTiles)
	{
		{
			ScopedK t(c->timer, "k_pt_tiles");
			hipLaunchKernelGGL(k_pt_tiles<true>, bubWaveGrid(nTiles), BUB_BLOCK, 0, s, dAln, nE, dTileOff, (u32)nTiles, tileShift, dTrgS, dQryS,
							   dTileNg, dTileNq);
		}
		{
			ScopedK t(c->timer, "k_pt_scan");
			fgprim::scan<u32>(s, dTileNg, dTileNg, nTiles + 1, false, dScan);
			fgprim::scan<u32>(s, dTileNq, dTileNq, nTiles + 1, false, dScan);
		}
		ScopedK t(c->timer, "k_cf_edge");
		hipLaunchKernelGGL(k_cf_edge, bubWaveGrid(nTiles), BUB_BLOCK, 0, s, dAln, nE, dTileOff, (u32)nTiles, tileShift, dTileNg, dTileNq, dTrgS,
						   dQryS, dNucQ, dQInd);
	}
	if (nEntries)
	{
		ScopedK t(c->timer, "k_cf_mark");
		hipLaunchKernelGGL(k_cf_mark, bubGrid(nEntries), BUB_BLOCK, 0, s, (u32)nEntries, dSegOff, nJ, dEntries, dJobs, dMark);
	}
	{
		ScopedK t(c->timer, "k_cf_judge");
		hipLaunchKernelGGL(k_cf_judge, bubGrid(nPos + 1), BUB_BLOCK, 0, s, (u32)nPos, dJobs, nJ, dJobAt, dAln, dMark, dNucQ, dQInd, dConsCode,
						   dConsCnt, dCode, dIs);
	}
	{
		ScopedK t(c->timer, "k_pt_scan");
		for (int k = 0; k < 8; ++k) fgprim::scan<u32>(s, dIs + (size_t)k * (nPos + 1), dIs + (size_t)k * (nPos + 1), nPos + 1, false, dScan);
		fgprim::scan<u32>(s, dConsCnt, dConsCnt, nSlots + 1, false, dScan);
		hipLaunchKernelGGL(k_pt_pick<u64>, bubGrid((u64)nJ + 1), BUB_BLOCK, 0, s, nJ + 1, dJobAt, dIs, nPos + 1, 8u, dPick);
		hipLaunchKernelGGL(k_pt_pick<u64>, bubGrid((u64)nE + 1), BUB_BLOCK, 0, s, nE + 1, dSlotAt, dConsCnt, 0ULL, 1u, dPick + 8 * ((size_t)nJ + 1));
	}
	HIP_CHECK(hipGetLastError());
	std::vector<u32> pick(8 * ((size_t)nJ + 1) + (size_t)nE + 1);
	HIP_CHECK(hipMemcpyAsync(pick.data(), dPick, pick.size() * 4, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	const u32* consAt = pick.data() + 8 * ((size_t)nJ + 1);
	std::vector<u32> listAt(8);
	u64 nOut = 0;
	for (int k = 0; k < 8; ++k) { listAt[k] = (u32)nOut; nOut += pick[(size_t)k * (nJ + 1) + nJ]; }
	const u32 nCons = consAt[nE];
	if (nOut >= (1ULL << 32)) throw FgError{FG_ERR_NOMEM, "fg_confirm_positions: 2^32 list entries in a sub-batch; lower FG_PARTITION_BATCH_COLS"};
	i32* dLists = B.get<i32>(nOut);
	i32* dCons = B.get<i32>(nCons);
	u32* dListAt = B.get<u32>(8);
	ptUp(s, dListAt, listAt);
	if (nOut)
	{
		ScopedK t(c->timer, "k_cf_compact");
		hipLaunchKernelGGL(k_cf_compact, bubGrid(nPos), BUB_BLOCK, 0, s, (u32)nPos, dJobs, nJ, dJobAt, dCode, dIs, dListAt, dLists);
	}
	if (nCons)
	{
		ScopedK t(c->timer, "k_cf_cons");
		hipLaunchKernelGGL(k_cf_cons, bubGrid(nSlots), BUB_BLOCK, 0, s, (u32)nSlots, dConsCode, dConsCnt, dQInd, dCons);
	}
	HIP_CHECK(hipGetLastError());
	for (int k = 0; k < 8; ++k)
	{
		const size_t base = own.list[k].size();
		const u32 n = pick[(size_t)k * (nJ + 1) + nJ];
		own.list[k].resize(base + n);
		if (n) HIP_CHECK(hipMemcpyAsync(own.list[k].data() + base, dLists + listAt[k], (size_t)n * 4, hipMemcpyDeviceToHost, s));
		for (u32 j = 0; j < nJ; ++j) own.listOff[k].push_back(base + pick[(size_t)k * (nJ + 1) + j + 1]);
	}
	const size_t base = own.cons.size();
	own.cons.resize(base + nCons);
	if (nCons) HIP_CHECK(hipMemcpyAsync(own.cons.data() + base, dCons, (size_t)nCons * 4, hipMemcpyDeviceToHost, s));
	for (u32 e = 0; e < nE; ++e) own.consOff.push_back(base + consAt[e + 1]);
	HIP_CHECK(hipStreamSynchronize(s));		// also keeps listAt alive until its copy has run
}

struct ClassifyOwner {
	std::vector<uint64_t> readOff;
	std::vector<uint8_t> status, counted;
	std::vector<int32_t> topEdge, topScore, totalScore, alnScore;
};

struct ClassifyIn {
	int32_t bufferCount; const uint64_t* jobEdgeOff; const uint32_t* jobReads; const uint64_t* edgePosOff; const int32_t* edgePos;
	const uint64_t* edgeAlnOff; const uint32_t* read; const int32_t *trgStart, *trgEnd; const uint64_t* colOff;
	const uint8_t *trgCols, *qryCols;
};

void clSubBatch(fg_ctx* c, u32 j0, u32 j1, const ClassifyIn& in, const std::vector<ClEdge>& allEdges, u32 tileShift, bool wantScores,
				ClassifyOwner& own, const CigSource* cig = nullptr /* the columns are expanded here, not read from the host */)
{
	hipStream_t s = c->stream;
	const u32 nJ = j1 - j0;
	const u64 e0 = in.jobEdgeOff[j0], e1 = in.jobEdgeOff[j1];
	const u32 nE = (u32)(e1 - e0);
	const u64 a0 = in.edgeAlnOff[e0], a1 = in.edgeAlnOff[e1];
	const u64 nAln64 = a1 - a0;
	const u64 p0 = in.edgePosOff[e0], nEntries = in.edgePosOff[e1] - p0;
	const u64 col0 = nAln64 ? in.colOff[a0] : 0, nCols = nAln64 ? in.colOff[a1] - col0 : 0;

	std::vector<u64> readAt((size_t)nJ + 1), edgePosAt((size_t)nE + 1);
	std::vector<u32> jobEdge0(nJ);
	std::vector<ClEdge> edges(nE);
	u64 nReads = 0, nCells = 0;
	for (u32 j = 0; j < nJ; ++j)
	{
		readAt[j] = nReads;
		nReads += in.jobReads[j0 + j];
		jobEdge0[j] = (u32)(in.jobEdgeOff[j0 + j] - e0);
	}
	readAt[nJ] = nReads;
	for (u32 e = 0; e < nE; ++e)
	{
		edges[e] = allEdges[e0 + e - in.jobEdgeOff[0]];
		edges[e].cntBase = (u32)nCells;
		nCells += (u64)((long long)edges[e].maxEnd - edges[e].minPos);
		edgePosAt[e] = in.edgePosOff[e0 + e] - p0;
	}
	edgePosAt[nE] = nEntries;
	if (nReads >= (1ULL << 31) || nCells >= (1ULL << 31) || nCols >= (1ULL << 31) || nEntries >= (1ULL << 31) || nAln64 >= (1ULL << 30) ||
		nE >= (1u << 30))
		throw FgError{FG_ERR_NOMEM, "fg_classify_reads: a sub-batch of 2^31 reads, columns, cells or list entries or 2^30 alignments; lower "
									"FG_PARTITION_BATCH_COLS"};
	const u32 nAln = (u32)nAln64;
	std::vector<PtAln> alns(nAln);
	for (u32 j = 0; j < nJ; ++j)
		for (u64 e = in.jobEdgeOff[j0 + j]; e < in.jobEdgeOff[j0 + j + 1]; ++e)
			for (u64 a = in.edgeAlnOff[e]; a < in.edgeAlnOff[e + 1]; ++a)
			{
				PtAln& al = alns[a - a0];
				al.colOff = in.colOff[a] - col0; al.nCols = (u32)(in.colOff[a + 1] - in.colOff[a]);
				al.trgStart = in.trgStart[a]; al.trgEnd = in.trgEnd[a]; al.qryStart = 0;
				al.base = edges[e - e0].cntBase; al.minPos = edges[e - e0].minPos; al.edge = (u32)(e - e0);
				al.gread = (u32)(readAt[j] + in.read[a]);
			}
	std::vector<u32> tileOff;
	const u64 nTiles = ptTiles(alns, tileShift, tileOff);
	if (nTiles >= (1ULL << 31)) throw FgError{FG_ERR_NOMEM, "fg_classify_reads: 2^31 tiles in a sub-batch; lower FG_PARTITION_BATCH_COLS"};
	u32 eBits = 1, rBits = 1;
	while ((1ULL << eBits) < nE) ++eBits;
	while ((1ULL << rBits) < nReads) ++rBits;

	DevPool B{c->dPt, "fg_partition"};
	u64* dReadAt = B.get<u64>((size_t)nJ + 1);
	u64* dEdgePosAt = B.get<u64>((size_t)nE + 1);
	u32* dJobEdge0 = B.get<u32>(nJ);
	ClEdge* dEdges = B.get<ClEdge>(nE);
	PtAln* dAln = B.get<PtAln>(nAln);
	u32* dTileOff = B.get<u32>((size_t)nAln + 1);
	i32* dEntries = B.get<i32>(nEntries);
	u32* dCnt = B.get<u32>(nCells);
	u32* dTileNg = B.get<u32>(nTiles + 1);
	// k_cig_expand stores whole words past the last column
	unsigned char* dTrg = B.get<unsigned char>(nCols + (cig ? CIG_LANE_COLS : 0));
	unsigned char* dQry = B.get<unsigned char>(nCols + (cig ? CIG_LANE_COLS : 0));
	u32* dScore = B.get<u32>(nAln);
	unsigned char* dCounted = B.get<unsigned char>(nAln);
	u64* dKeys[2] = {B.get<u64>(nAln), B.get<u64>(nAln)};
	u64* dVals[2] = {B.get<u64>(nAln), B.get<u64>(nAln)};
	char* dSort = B.get<char>(fgprim::radixSortScratchBytes(nAln));
	u32* dScan = B.get<u32>(fgprim::scanScratchElems(nTiles + 1) + 8);
	unsigned char* dStatus = B.get<unsigned char>(nReads);
	i32* dVote = B.get<i32>(3 * nReads);

	ptUp(s, dReadAt, readAt); ptUp(s, dEdgePosAt, edgePosAt); ptUp(s, dJobEdge0, jobEdge0); ptUp(s, dEdges, edges); ptUp(s, dAln, alns);
	ptUp(s, dTileOff, tileOff);
	if (nEntries) HIP_CHECK(hipMemcpyAsync(dEntries, in.edgePos + p0, nEntries * 4, hipMemcpyHostToDevice, s));
	CigStaged staged;		// read by the expansion's uploads: alive until the stream has been waited for
	if (cig && nAln) (void)cigExpandSource(c, *cig, staged, a0, a1, dTrg, dQry);
	else if (nCols)
	{
		HIP_CHECK(hipMemcpyAsync(dTrg, in.trgCols + col0, nCols, hipMemcpyHostToDevice, s));
		HIP_CHECK(hipMemcpyAsync(dQry, in.qryCols + col0, nCols, hipMemcpyHostToDevice, s));
	}
	HIP_CHECK(hipMemsetAsync(dCnt, 0, nCells * 4 + 4, s));
	HIP_CHECK(hipMemsetAsync(dTileNg, 0, (nTiles + 1) * 4, s));
	HIP_CHECK(hipMemsetAsync(dScore, 0, (size_t)nAln * 4 + 4, s));

	if (nEntries && nCells)
	{
		ScopedK t(c->timer, "k_cl_poscount");
		hipLaunchKernelGGL(k_cl_poscount, bubGrid(nEntries), BUB_BLOCK, 0, s, (u32)nEntries, dEdgePosAt, nE, dEdges, dEntries, dCnt);
	}
	if (nTiles)
	{
		{
			ScopedK t(c->timer, "k_pt_tiles");
			hipLaunchKernelGGL(k_pt_tiles<false>, bubWaveGrid(nTiles), BUB_BLOCK, 0, s, dAln, nAln, dTileOff, (u32)nTiles, tileShift, dTrg, dQry,
							   dTileNg, (u32*)nullptr);
		}
		{
			ScopedK t(c->timer, "k_pt_scan");
			fgprim::scan<u32>(s, dTileNg, dTileNg, nTiles + 1, false, dScan);
		}
		ScopedK t(c->timer, "k_cl_score");
		hipLaunchKernelGGL(k_cl_score, bubWaveGrid(nTiles), BUB_BLOCK, 0, s, dAln, nAln, dTileOff, (u32)nTiles, tileShift, dTileNg, dTrg, dQry,
						   dCnt, dScore);
	}
	int cur = 0;
	if (nAln)
	{
		ScopedK t(c->timer, "k_cl_sort");
		hipLaunchKernelGGL(k_cl_keys, bubGrid(nAln), BUB_BLOCK, 0, s, dAln, nAln, eBits, dKeys[0], dVals[0]);
		cur = fgprim::radixSortPairs(s, dKeys[0], dVals[0], dKeys[1], dVals[1], nAln, 0, (int)(eBits + rBits), dSort);
	}
	if (nReads)
	{
		ScopedK t(c->timer, "k_cl_vote");
		hipLaunchKernelGGL(k_cl_vote, bubGrid(nReads), BUB_BLOCK, 0, s, (u32)nReads, dReadAt, nJ, dJobEdge0, dKeys[cur], dVals[cur], nAln, eBits,
						   dScore, in.bufferCount, dCounted, dStatus, dVote, dVote + nReads, dVote + 2 * nReads);
	}
	HIP_CHECK(hipGetLastError());
	const size_t rAt = own.status.size();
	for (u32 j = 0; j < nJ; ++j) own.readOff.push_back(rAt + readAt[j + 1]);
	own.status.resize(rAt + nReads);
	std::vector<int32_t>* v[3] = {&own.topEdge, &own.topScore, &own.totalScore};
	for (int k = 0; k < 3; ++k) v[k]->resize(rAt + nReads);
	if (nReads)
	{
		HIP_CHECK(hipMemcpyAsync(own.status.data() + rAt, dStatus, nReads, hipMemcpyDeviceToHost, s));
		for (int k = 0; k < 3; ++k) HIP_CHECK(hipMemcpyAsync(v[k]->data() + rAt, dVote + (size_t)k * nReads, nReads * 4, hipMemcpyDeviceToHost, s));
	}
	if (wantScores)
	{
		const size_t at = own.alnScore.size();
		own.alnScore.resize(at + nAln);
		own.counted.resize(at + nAln);
		if (nAln)
		{
			HIP_CHECK(hipMemcpyAsync(own.alnScore.data() + at, dScore, (size_t)nAln * 4, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipMemcpyAsync(own.counted.data() + at, dCounted, nAln, hipMemcpyDeviceToHost, s));
		}
	}
	HIP_CHECK(hipStreamSynchronize(s));
}

// col_off over the alignments lo .. hi.  Both calls report every decrease before any width: not stageColOff's order.
void ptColOff(const std::string& name, const uint64_t* colOff, u64 lo, u64 hi, const uint8_t* trgCols, const uint8_t* qryCols)
{
	stageOffsets(name, "col_off", "", colOff, lo, hi);
	for (u64 a = lo; a < hi; ++a) stageColWidth(name, colOff, a);
	stageColsGiven(name, colOff, lo, hi, trgCols, qryCols);
}

// the finished owner into the caller's struct
void clHandOver(struct fg_classify_batch* out, ClassifyOwner* own, uint32_t n_jobs, u64 nAlns, bool wantScores)
{
	out->n_jobs = n_jobs;
	out->n_alignments = nAlns;
	out->read_off = own->readOff.data();
	out->status = own->status.data();
	out->top_edge = own->topEdge.data();
	out->top_score = own->topScore.data();
	out->total_score = own->totalScore.data();
	if (wantScores)
	{
		out->aln_score = own->alnScore.data();
		out->aln_counted = own->counted.data();
	}
	out->owner_ = own;
}

} // namespace

extern "C" {

int fg_confirm_positions(fg_ctx* c, uint32_t n_jobs, const uint8_t* side, const uint64_t* job_edge_off, const int32_t* trg_start,
						 const int32_t* trg_end, const int32_t* qry_start, const uint64_t* col_off, const uint8_t* trg_cols,
						 const uint8_t* qry_cols, const uint64_t* total_off, const int32_t* total_pos, const uint64_t* sub_off,
						 const int32_t* sub_pos, const uint64_t* del_off, const int32_t* del_pos, const uint64_t* ins_off,
						 const int32_t* ins_pos, struct fg_confirm_batch* out)
{
	return stageCall<ConfirmOwner>(c, out, [&](ConfirmOwner*& own)
	{
		u64 nEdges = 0;
		const std::string name = "fg_confirm_positions";
		if (!out) throw FgError{FG_ERR_ARG, name + ": null result"};
		const PtCut cut = ptCut(name);
		ConfirmIn in{side, job_edge_off, trg_start, trg_end, qry_start, col_off, trg_cols, qry_cols,
					 {total_off, sub_off, del_off, ins_off}, {total_pos, sub_pos, del_pos, ins_pos}};
		std::vector<CfJob> jobs(n_jobs);
		std::vector<u64> cost(n_jobs, 0);
		if (n_jobs)
		{
			if (!side || !job_edge_off || !trg_start || !trg_end || !qry_start || !col_off)
				throw FgError{FG_ERR_ARG, name + ": null side, job_edge_off, trg_start, trg_end, qry_start or col_off"};
			stageOffsets(name, "job_edge_off", "", job_edge_off, 0, n_jobs);
			for (int k = 0; k < 4; ++k)
			{
				if (!in.listOff[k]) throw FgError{FG_ERR_ARG, name + ": null offsets of a tentative list"};
				stageOffsets(name, "a tentative list's offset array", "", in.listOff[k], 0, n_jobs);
				if (in.listOff[k][n_jobs] > in.listOff[k][0] && !in.listPos[k]) throw FgError{FG_ERR_ARG, name + ": null positions of a tentative list"};
			}
			const u64 e0 = job_edge_off[0], e1 = job_edge_off[n_jobs];
			nEdges = e1 - e0;
			ptColOff(name, col_off, e0, e1, trg_cols, qry_cols);
			for (u32 j = 0; j < n_jobs; ++j)
			{
				if (side[j] > 1) throw FgError{FG_ERR_ARG, name + ": side > 1 at job " + std::to_string(j)};
				if (job_edge_off[j + 1] == job_edge_off[j]) throw FgError{FG_ERR_ARG, name + ": job " + std::to_string(j) + " has no edges"};
				if (job_edge_off[j + 1] - job_edge_off[j] >= (1ULL << 31)) throw FgError{FG_ERR_ARG, name + ": a job of 2^31 edges"};
				CfJob& jb = jobs[j];
				jb = CfJob{0, 0, (u32)(job_edge_off[j + 1] - job_edge_off[j]), INT32_MAX, INT32_MIN, INT32_MAX, INT32_MIN, side[j], 0};
				for (u64 e = job_edge_off[j]; e < job_edge_off[j + 1]; ++e)
				{
					ptCheckColumns(name, e, trg_start, trg_end, col_off, trg_cols, qry_cols);
					jb.minStart = std::min(jb.minStart, trg_start[e]); jb.maxStart = std::max(jb.maxStart, trg_start[e]);
					jb.minEnd = std::min(jb.minEnd, trg_end[e]); jb.maxEnd = std::max(jb.maxEnd, trg_end[e]);
				}
				cost[j] = col_off[job_edge_off[j + 1]] - col_off[job_edge_off[j]] + (u64)((long long)jb.maxEnd - jb.minStart);
				stageFits(name, "job", j, cost[j], cut.budget, "columns and table cells", "FG_PARTITION_BATCH_COLS");
			}
		}
		own = new ConfirmOwner;
		for (auto& v : own->listOff) v.assign(1, 0);
		own->consOff.assign(1, 0);
		HIP_CHECK(hipSetDevice(c->device));
		c->timer.reset();
		for (u32 i = 0; i < n_jobs;)
		{
			const u32 j = stageCut(i, n_jobs, cost, cut.budget, cut.maxJobs);
			cfSubBatch(c, i, j, in, jobs, cut.tileShift, *own);
			i = j;
		}
		c->timer.collect();
		for (auto& v : own->list) stageKeep(v);
		stageKeep(own->cons);
		out->n_jobs = n_jobs;
		out->n_edges = nEdges;
		uint64_t** offs[8] = {&out->conf_total_off, &out->conf_sub_off, &out->conf_del_off, &out->conf_ins_off,
							  &out->rej_total_off, &out->rej_sub_off, &out->rej_del_off, &out->rej_ins_off};
		int32_t** poss[8] = {&out->conf_total_pos, &out->conf_sub_pos, &out->conf_del_pos, &out->conf_ins_pos,
							 &out->rej_total_pos, &out->rej_sub_pos, &out->rej_del_pos, &out->rej_ins_pos};
		for (int k = 0; k < 8; ++k) { *offs[k] = own->listOff[k].data(); *poss[k] = own->list[k].data(); }
		out->cons_off = own->consOff.data();
		out->cons_pos = own->cons.data();
		out->owner_ = own;
	});
}

void fg_release_confirm(struct fg_confirm_batch* b) { stageRelease<ConfirmOwner>(b); }

int fg_classify_reads(fg_ctx* c, int32_t buffer_count, uint32_t n_jobs, const uint64_t* job_edge_off, const uint32_t* job_n_reads,
					  const uint64_t* edge_pos_off, const int32_t* edge_pos, const uint64_t* edge_aln_off, const uint32_t* read,
					  const int32_t* trg_start, const int32_t* trg_end, const uint64_t* col_off, const uint8_t* trg_cols,
					  const uint8_t* qry_cols, uint8_t want_scores, struct fg_classify_batch* out)
{
	return stageCall<ClassifyOwner>(c, out, [&](ClassifyOwner*& own)
	{
		u64 nAlns = 0;
		const std::string name = "fg_classify_reads";
		if (!out) throw FgError{FG_ERR_ARG, name + ": null result"};
		if (buffer_count < 0) throw FgError{FG_ERR_ARG, name + ": buffer_count < 0"};
		const PtCut cut = ptCut(name);
		ClassifyIn in{buffer_count, job_edge_off, job_n_reads, edge_pos_off, edge_pos, edge_aln_off, read, trg_start, trg_end, col_off,
					  trg_cols, qry_cols};
		std::vector<ClEdge> edges;
		std::vector<u64> cost(n_jobs, 0);
		if (n_jobs)
		{
			if (!job_edge_off || !job_n_reads || !edge_pos_off || !edge_aln_off)
				throw FgError{FG_ERR_ARG, name + ": null job_edge_off, job_n_reads, edge_pos_off or edge_aln_off"};
			stageOffsets(name, "job_edge_off", "", job_edge_off, 0, n_jobs);
			const u64 e0 = job_edge_off[0], e1 = job_edge_off[n_jobs];
			stageOffsets(name, "edge_pos_off", "", edge_pos_off, e0, e1);
			stageOffsets(name, "edge_aln_off", "", edge_aln_off, e0, e1);
			if (edge_pos_off[e1] > edge_pos_off[e0] && !edge_pos) throw FgError{FG_ERR_ARG, name + ": null edge_pos"};
			const u64 a0 = edge_aln_off[e0], a1 = edge_aln_off[e1];
			nAlns = a1 - a0;
			if (a1 > a0 && (!read || !trg_start || !trg_end || !col_off)) throw FgError{FG_ERR_ARG, name + ": null read, trg_start, trg_end or col_off"};
			ptColOff(name, col_off, a0, a1, trg_cols, qry_cols);
			edges.resize(e1 - e0);
			for (u32 j = 0; j < n_jobs; ++j)
			{
				if (job_edge_off[j + 1] == job_edge_off[j]) throw FgError{FG_ERR_ARG, name + ": job " + std::to_string(j) + " has no edges"};
				if (edge_pos_off[job_edge_off[j + 1]] - edge_pos_off[job_edge_off[j]] >= (1ULL << 31))
					throw FgError{FG_ERR_ARG, name + ": the edge lists of job " + std::to_string(j) + " hold 2^31 entries: the scores do not fit int32"};
				u64 cells = 0;
				for (u64 e = job_edge_off[j]; e < job_edge_off[j + 1]; ++e)
				{
					ClEdge& ed = edges[e - e0];
					ed = ClEdge{0, INT32_MAX, INT32_MIN, 0};
					for (u64 a = edge_aln_off[e]; a < edge_aln_off[e + 1]; ++a)
					{
						if (read[a] >= job_n_reads[j])
							throw FgError{FG_ERR_ARG, name + ": read " + std::to_string(read[a]) + " of alignment " + std::to_string(a) + " is not below n_reads"};
						ptCheckColumns(name, a, trg_start, trg_end, col_off, trg_cols, qry_cols);
						ed.minPos = std::min(ed.minPos, trg_start[a]); ed.maxEnd = std::max(ed.maxEnd, trg_end[a]);
					}
					if (edge_aln_off[e + 1] == edge_aln_off[e]) ed.minPos = ed.maxEnd = 0;
					cells += (u64)((long long)ed.maxEnd - ed.minPos);
				}
				cost[j] = cells;
				if (edge_aln_off[job_edge_off[j + 1]] > edge_aln_off[job_edge_off[j]])
					cost[j] += col_off[edge_aln_off[job_edge_off[j + 1]]] - col_off[edge_aln_off[job_edge_off[j]]];
				stageFits(name, "job", j, cost[j], cut.budget, "columns and table cells", "FG_PARTITION_BATCH_COLS");
			}
		}
		own = new ClassifyOwner;
		own->readOff.assign(1, 0);
		HIP_CHECK(hipSetDevice(c->device));
		c->timer.reset();
		for (u32 i = 0; i < n_jobs;)
		{
			const u32 j = stageCut(i, n_jobs, cost, cut.budget, cut.maxJobs);
			clSubBatch(c, i, j, in, edges, cut.tileShift, want_scores != 0, *own);
			i = j;
		}
		c->timer.collect();
		stageKeep(own->status, own->topEdge, own->topScore, own->totalScore, own->alnScore, own->counted);
		clHandOver(out, own, n_jobs, nAlns, want_scores != 0);
	});
}

int fg_classify_reads_cigars(fg_ctx* c, int32_t buffer_count, uint32_t n_jobs, const uint64_t* job_edge_off, const uint32_t* job_n_reads,
							 const uint64_t* edge_pos_off, const int32_t* edge_pos, const uint64_t* edge_off, const uint8_t* edge_seq,
							 const uint64_t* edge_aln_off, const uint32_t* read, const int32_t* ctg_pos, const uint64_t* run_off,
							 const uint8_t* run_op, const uint32_t* run_len, const uint64_t* read_off, const uint8_t* read_seq,
							 uint8_t want_scores, struct fg_classify_batch* out)
{
	return stageCall<ClassifyOwner>(c, out, [&](ClassifyOwner*& own)
	{
		u64 nAlns = 0;
		const std::string name = "fg_classify_reads_cigars";
		if (!out) throw FgError{FG_ERR_ARG, name + ": null result"};
		const PtCut cut = ptCut(name);
		CigPlan plan;
		std::vector<ClEdge> edges;
		std::vector<u64> cost(n_jobs, 0), jobAlnOff((size_t)n_jobs + 1, 0);
		if (n_jobs)
		{
			if (!job_edge_off || !job_n_reads || !edge_pos_off || !edge_aln_off)
				throw FgError{FG_ERR_ARG, name + ": null job_edge_off, job_n_reads, edge_pos_off or edge_aln_off"};
			stageOffsets(name, "job_edge_off", "", job_edge_off, 0, n_jobs);
			const u64 e0 = job_edge_off[0], e1 = job_edge_off[n_jobs];
			stageOffsets(name, "edge_pos_off", "", edge_pos_off, e0, e1);
			stageOffsets(name, "edge_aln_off", "", edge_aln_off, e0, e1);
			if (e1 - e0 > 0xffffffffULL) throw FgError{FG_ERR_ARG, name + ": 2^32 edges"};
			if (e1 > e0 && !edge_off) throw FgError{FG_ERR_ARG, name + ": null edge_off"};
			const u64 a0 = edge_aln_off[e0], a1 = edge_aln_off[e1];
			nAlns = a1 - a0;
			// the edges of the call are the contigs of the expansion, numbered from the first one
			std::vector<uint32_t> alnContig((size_t)a1, 0);
			for (u64 e = e0; e < e1; ++e)
				for (u64 a = edge_aln_off[e]; a < edge_aln_off[e + 1]; ++a) alnContig[a] = (uint32_t)(e - e0);
			// every check of fg_expand_cigars, then those fg_classify_reads makes on what the expansion would hand it
			cigCheckRecords(name, (u32)(e1 - e0), edge_off ? edge_off + e0 : nullptr, edge_seq, a0, a1, alnContig.data(),
							!read || !ctg_pos || !run_off || !read_off, "null read, ctg_pos, run_off or read_off", ctg_pos, run_off, run_op,
							run_len, read_off, read_seq, plan);
		}
		if (buffer_count < 0) throw FgError{FG_ERR_ARG, name + ": buffer_count < 0"};
		if (n_jobs)
		{
			const u64 e0 = job_edge_off[0], e1 = job_edge_off[n_jobs];
			if (edge_pos_off[e1] > edge_pos_off[e0] && !edge_pos) throw FgError{FG_ERR_ARG, name + ": null edge_pos"};
			edges.resize(e1 - e0);
			for (u32 j = 0; j < n_jobs; ++j)
			{
				if (job_edge_off[j + 1] == job_edge_off[j]) throw FgError{FG_ERR_ARG, name + ": job " + std::to_string(j) + " has no edges"};
				if (edge_pos_off[job_edge_off[j + 1]] - edge_pos_off[job_edge_off[j]] >= (1ULL << 31))
					throw FgError{FG_ERR_ARG, name + ": the edge lists of job " + std::to_string(j) + " hold 2^31 entries: the scores do not fit int32"};
				u64 cells = 0;
				for (u64 e = job_edge_off[j]; e < job_edge_off[j + 1]; ++e)
				{
					ClEdge& ed = edges[e - e0];
					ed = ClEdge{0, INT32_MAX, INT32_MIN, 0};
					for (u64 a = edge_aln_off[e]; a < edge_aln_off[e + 1]; ++a)
					{
						if (read[a] >= job_n_reads[j])
							throw FgError{FG_ERR_ARG, name + ": read " + std::to_string(read[a]) + " of alignment " + std::to_string(a) + " is not below n_reads"};
						// No walk over columns on the host.  What ptCheckColumns reads from them holds by construction after
						// cigCheckRecords: every contig and SEQ byte is below 128, so every column is; trg_start = ctg_pos - 1 >= 0;
						// the non-gap target columns are the contig bytes the runs consume, which is trg_end - trg_start.
						ed.minPos = std::min(ed.minPos, plan.trgStart[a]); ed.maxEnd = std::max(ed.maxEnd, plan.trgEnd[a]);
					}
					if (edge_aln_off[e + 1] == edge_aln_off[e]) ed.minPos = ed.maxEnd = 0;
					cells += (u64)((long long)ed.maxEnd - ed.minPos);
				}
				jobAlnOff[j] = edge_aln_off[job_edge_off[j]];
				jobAlnOff[j + 1] = edge_aln_off[job_edge_off[j + 1]];
				cost[j] = cells + (plan.colOff[jobAlnOff[j + 1]] - plan.colOff[jobAlnOff[j]]);
				stageFits(name, "job", j, cost[j], cut.budget, "columns and table cells", "FG_PARTITION_BATCH_COLS");
			}
		}
		ClassifyIn in{buffer_count, job_edge_off, job_n_reads, edge_pos_off, edge_pos, edge_aln_off, read, plan.trgStart.data(),
					  plan.trgEnd.data(), plan.colOff.data(), nullptr, nullptr};
		own = new ClassifyOwner;
		own->readOff.assign(1, 0);
		HIP_CHECK(hipSetDevice(c->device));
		c->timer.reset();
		// the edge consensuses go up once per call; a sub-batch expands its own alignments
		const CigSource src{&plan, nAlns ? cigUploadContigs(c, plan, edge_seq) : nullptr, run_off, run_op, run_len, read_off, read_seq, cigTile()};
		for (u32 i = 0; i < n_jobs;)
		{
			// the "contigs i .. j" of the cut are the edges of the jobs i .. j
			const u32 j = cigCutContigs(name, "FG_PARTITION_BATCH_COLS", i, n_jobs, cost, cut.budget, cut.maxJobs, jobAlnOff.data(), run_off, read_off, "job");
			clSubBatch(c, i, j, in, edges, cut.tileShift, want_scores != 0, *own, &src);
			i = j;
		}
		c->timer.collect();
		stageKeep(own->status, own->topEdge, own->topScore, own->totalScore, own->alnScore, own->counted);
		clHandOver(out, own, n_jobs, nAlns, want_scores != 0);
	});
}

void fg_release_classify(struct fg_classify_batch* b) { stageRelease<ClassifyOwner>(b); }

} // extern "C"
