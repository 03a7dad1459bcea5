// fg_edit_ranges: getAlignmentErrEdlib (src/sequence/alignment.cpp:218-247) for (id, begin, end) ranges of the
// sequences that are resident on the device -- what ReadAligner::getChainBaseDivergence
// (src/repeat_graph/read_aligner.cpp:410-434) asks for every alignment of every chain when reads_base_alignment is set.
//
// The distances themselves come from fgEditDistances (fg_editdist.hip), unchanged: this file only feeds it.  Per
// sub-batch of FG_EDIT_BATCH_PAIRS pairs the (pair, side) table goes up (16 B per side), k_edit_range_prims turns it
// into the primaries and the per-call query array the edit kernels read, and k_edit_range_collect packs what they
// left into three dense int32 arrays (12 B per pair come back).  No PrimRec is built on or copied to the host.
#include "fg_ctx.h"
#include "fg_stage.h"

namespace {

#define ER_BLOCK 256
#define ER_MAX_BLOCKS 2048		// the rest of a sub-batch by grid stride

// sides[2 i], sides[2 i + 1] = cur, ext of pair i of the sub-batch -> prims[i], query[i].  The cur side is addressed
// through the query array (record * 2 + strand, in whichever container the call's cur ids name: EdSeqs picks it as
// rangeSides did), the ext side through its FastaRecord id.
__global__ void __launch_bounds__(ER_BLOCK)
k_edit_range_prims(const FgRangeSide* __restrict__ sides, u32 nPairs, const i32* __restrict__ extLen, u32 firstId,
				   PrimRec* __restrict__ prims, u32* __restrict__ query)
{
	for (u64 i = (u64)blockIdx.x * ER_BLOCK + threadIdx.x; i < nPairs; i += (u64)gridDim.x * ER_BLOCK)
	{
		const FgRangeSide cur = sides[2 * i], ext = sides[2 * i + 1];
		PrimRec r;
		r.query = (u32)i;
		r.extId = firstId + 2u * ext.rec + (ext.flags & 1u);
		r.curBegin = cur.start; r.curEnd = cur.start + cur.len;
		r.extBegin = ext.start; r.extEnd = ext.start + ext.len;
		r.extLen = extLen[ext.rec];
		r.score = 0; r.chainLength = 0; r.filtered = 0;
		r.editDistance = -1; r.hpcLenCur = 0; r.hpcLenExt = 0;
		prims[i] = r;
		query[i] = 2u * cur.rec + (cur.flags & 1u);
	}
}

// out[0 .. n) = distances, out[n .. 2n) = compared lengths of the cur side, out[2n .. 3n) = of the ext side
__global__ void __launch_bounds__(ER_BLOCK)
k_edit_range_collect(const PrimRec* __restrict__ prims, u32 nPairs, i32* __restrict__ out)
{
	for (u64 i = (u64)blockIdx.x * ER_BLOCK + threadIdx.x; i < nPairs; i += (u64)gridDim.x * ER_BLOCK)
	{
		out[i] = prims[i].editDistance;
		out[(u64)nPairs + i] = prims[i].hpcLenCur;
		out[2 * (u64)nPairs + i] = prims[i].hpcLenExt;
	}
}

// c->curQuery belongs to the call that set it: put back on every way out
struct CurQueryGuard {
	fg_ctx* c; const u32* saved;
	explicit CurQueryGuard(fg_ctx* c_) : c(c_), saved(c_->curQuery) {}
	~CurQueryGuard() { c->curQuery = saved; }
};

} // namespace

// fg_edit_ranges behind its argument checks: sides = 2 nPairs entries (cur, ext of pair 0, ...); dist has nPairs
// entries, lenCur / lenExt may be null
void fgEditRanges(fg_ctx* c, const std::vector<FgRangeSide>& sides, bool useHpc, i32* dist, i32* lenCur, i32* lenExt)
{
	const u64 nPairs = sides.size() / 2;
	if (!nPairs) return;
	hipStream_t s = c->stream;
	u64 batch = stageEnvU64("FG_EDIT_BATCH_PAIRS", 1ULL << 20);
	batch = std::min<u64>(std::max<u64>(batch, 1), 1ULL << 26);		// fgEditDistances' lists index a sub-batch with 32 bits
	const u64 cap = std::min(batch, nPairs);
	c->dRangeSides.reserve(2 * cap * sizeof(FgRangeSide));
	c->dEditPrims.reserve(cap * sizeof(PrimRec));
	c->dEditQuery.reserve(cap);
	c->dEditOut.reserve(3 * cap);
	FgRangeSide* dSides = (FgRangeSide*)c->dRangeSides.p;
	PrimRec* dPrims = (PrimRec*)c->dEditPrims.p;
	CurQueryGuard guard(c);
	c->curQuery = c->dEditQuery.p;
	c->timer.reset();
	for (u64 first = 0; first < nPairs; first += batch)
	{
		const u32 n = (u32)std::min(batch, nPairs - first);
		const unsigned grid = std::min<unsigned>((n + ER_BLOCK - 1) / ER_BLOCK, ER_MAX_BLOCKS);
		HIP_CHECK(hipMemcpyAsync(dSides, sides.data() + 2 * first, 2 * (size_t)n * sizeof(FgRangeSide), hipMemcpyHostToDevice, s));
		{
			ScopedK t(c->timer, "k_edit_range_prims");
			hipLaunchKernelGGL(k_edit_range_prims, grid, ER_BLOCK, 0, s, dSides, n, c->dLen.p, c->firstId, dPrims, c->dEditQuery.p);
		}
		fgEditDistances(c, dPrims, n, useHpc ? 1 : 0);
		{
			ScopedK t(c->timer, "k_edit_range_collect");
			hipLaunchKernelGGL(k_edit_range_collect, grid, ER_BLOCK, 0, s, dPrims, n, c->dEditOut.p);
		}
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipMemcpyAsync(dist + first, c->dEditOut.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
		if (lenCur) HIP_CHECK(hipMemcpyAsync(lenCur + first, c->dEditOut.p + n, (size_t)n * 4, hipMemcpyDeviceToHost, s));
		if (lenExt) HIP_CHECK(hipMemcpyAsync(lenExt + first, c->dEditOut.p + 2 * (size_t)n, (size_t)n * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));		// the buffers are the next sub-batch's
	}
	c->timer.collect();
}
