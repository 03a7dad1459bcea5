// fg_divergence_profile: Trestle's divergent positions (flye/trestle/divergence.py:55-143, _contig_profile, _count_freqs
// and _call_position) on the device.  Integers and exact compares only; the three rate tests go through tables the host
// makes in double.
//
// Per sub-batch of whole contigs (FG_DIVERGENCE_BATCH_COLS):
//   k_bub_shift     (fg_gapshift.h) both shift_gaps passes, every alignment.
//   k_dv_tiles      one wave per tile of DV_TILE columns of one alignment: its non-gap target columns.  An exclusive scan
//                   over all tiles gives, minus the value at the alignment's first tile, the tile's first position.
//   k_dv_count      one wave per tile: positions by ballot prefix counts from the tile's base.  A target-gap column adds
//                   to insertions[position][rank of the query byte] (a '-' against a '-' too), every other column to
//                   matches[position][rank] and takes nucl by an atomic max of (alignment + 1) << 40 | column << 8 | target
//                   byte, as k_cc_profile does.  Beside every count stands the smallest (alignment << 32 | column) that
//                   added to it (atomic min): the moment the key entered the reference's dict.
//   k_dv_finish     one thread per position: the eight values of _count_freqs, ties of the largest count to the smallest
//                   tag (max(d, key=d.get) returns the key inserted first), and the flags of _call_position by integer
//                   compares against minCt[cov], the smallest count with ct / float(cov) >= thresh.
//   (scan)          four exclusive sums over the flags; k_dv_compact writes the four ascending lists, k_dv_pick takes the
//                   lists' starts per contig.
// Integer atomics only: the result does not depend on the schedule.  The host does work proportional to contigs,
// alignments and (for the byte check) columns.
//
// fg_divergence_profile_cigars takes SAM records for the columns: a sub-batch expands its own alignments (fg_cigexpand.h)
// into the buffers k_bub_shift reads.  The distinct query bytes of the call size the count tables and so decide the cut
// before any column exists:
//   k_seq_present   one wave per maximal piece of SEQ that M and I runs consume: the 128-bit set of its bytes, upper-cased
//                   as k_cig_expand stores them.  The host adds '-' where a D run has a length.
#include "fg_ctx.h"
#include "fg_stage.h"
#include "fg_devprim.h"
#include "fg_gapshift.h"
#include "fg_cigexpand.h"
#include <cmath>

namespace {

#define DV_TILE 1024u		// columns per wave of k_dv_tiles / k_dv_count
#define DV_NONE 0xffu		// rank of a byte no query column holds

struct DvContig { u64 posOff; i32 len; u32 pad; };

// the last i in [0, n) with off[i] <= x (off ascending, off[0] <= x)
template <class T>
__device__ __forceinline__ u32 dv_find(const T* __restrict__ off, u32 n, u64 x)
{
	u32 lo = 0, hi = n;
	while (hi - lo > 1)
	{
		const u32 mid = (lo + hi) >> 1;
		if ((u64)off[mid] <= x) lo = mid; else hi = mid;
	}
	return lo;
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_dv_tiles(const BubAln* __restrict__ alns, u32 nAln, const u32* __restrict__ tileOff, u32 nTiles, const unsigned char* __restrict__ trg,
		   u32* __restrict__ tileNg)
{
	const int lane = threadIdx.x & 63;
	const u32 w = blockIdx.x * BUB_WAVES + (threadIdx.x >> 6);
	if (w >= nTiles) return;
	const u32 a = dv_find(tileOff, nAln, w);
	const BubAln al = alns[a];
	const unsigned char* t = trg + al.colOff;
	const u32 c0 = (w - tileOff[a]) * DV_TILE, c1 = min(c0 + DV_TILE, al.nCols);
	u32 cnt = 0;
	for (u32 c = c0; c < c1; c += 64)
	{
		const u32 i = c + lane;
		cnt += (u32)__popcll(__ballot(i < c1 && t[i] != '-'));
	}
	if (lane == 0) tileNg[w] = cnt;
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_dv_count(const BubAln* __restrict__ alns, u32 nAln, const DvContig* __restrict__ contigs, const u32* __restrict__ tileOff, u32 nTiles,
		   const u32* __restrict__ tileBase, const unsigned char* __restrict__ trg, const unsigned char* __restrict__ qry,
		   const unsigned char* __restrict__ rank, u32 nB, u32* matCnt, u32* insCnt, unsigned long long* matFirst,
		   unsigned long long* insFirst, unsigned long long* tag)
{
	const int lane = threadIdx.x & 63;
	const u32 w = blockIdx.x * BUB_WAVES + (threadIdx.x >> 6);
	if (w >= nTiles) return;
	const u32 a = dv_find(tileOff, nAln, w);
	const BubAln al = alns[a];
	const DvContig ct = contigs[al.contig];
	const long long len = ct.len;
	const unsigned char* t = trg + al.colOff;
	const unsigned char* q = qry + al.colOff;
	const u64 below = bub_below(lane);
	const u32 c0 = (w - tileOff[a]) * DV_TILE, c1 = min(c0 + DV_TILE, al.nCols);
	long long base = (long long)(tileBase[w] - tileBase[tileOff[a]]);
	for (u32 cc = c0; cc < c1; cc += 64)
	{
		const u32 i = cc + lane;
		const bool valid = i < c1;
		const unsigned char tb = valid ? t[i] : (unsigned char)'-', qb = valid ? q[i] : (unsigned char)'-';
		const bool ng = valid && tb != '-';
		const u64 m = __ballot(ng);
		const long long c = base + __popcll(m & below);
		// a target gap stands at the position before it; index -1 is Python's last element
		long long pos = ng ? al.trgStart + c : al.trgStart + c - 1;
		if (pos >= len) pos -= len;
		if (pos < 0) pos = len - 1;
		const u32 r = rank[qb & 127];
		if (valid && pos >= 0 && pos < len && r < nB)
		{
			const u64 at = ct.posOff + (u64)pos;
			const u64 cell = at * nB + r;
			const unsigned long long first = ((unsigned long long)a << 32) | i;
			if (ng)
			{
				atomicAdd(&matCnt[cell], 1u);
				atomicMin(&matFirst[cell], first);
				atomicMax(&tag[at], ((unsigned long long)(a + 1u) << 40) | ((unsigned long long)i << 8) | tb);
			}
			else
			{
				atomicAdd(&insCnt[cell], 1u);
				atomicMin(&insFirst[cell], first);
			}
		}
		base += __popcll(m);
	}
}

// the largest count of a row among the ranks that pass, ties to the smallest tag
#define DV_BEST(cntRow, firstRow, skipA, skipB, bestRank, bestCnt)                                      \
	{                                                                                                   \
		unsigned long long bestTag = ~0ULL;                                                             \
		for (u32 r = 0; r < nB; ++r)                                                                    \
		{                                                                                               \
			const u32 v = cntRow[r];                                                                    \
			if (v == 0 || r == skipA || r == skipB) continue;                                           \
			const unsigned long long f = firstRow[r];                                                   \
			if (v > bestCnt || (v == bestCnt && f < bestTag)) { bestCnt = v; bestTag = f; bestRank = r; } \
		}                                                                                               \
	}

__global__ void __launch_bounds__(BUB_BLOCK)
k_dv_finish(u32 nPos, const u32* __restrict__ matCnt,
			const u32* __restrict__ insCnt, const unsigned long long* __restrict__ matFirst, const unsigned long long* __restrict__ insFirst,
			const unsigned long long* __restrict__ tag, const unsigned char* __restrict__ rank, const unsigned char* __restrict__ byteOf,
			u32 nB, const u32* __restrict__ minCt, u32 nCov, i32* __restrict__ cov, unsigned char* __restrict__ nucl, i32* __restrict__ matCt,
			unsigned char* __restrict__ subBase, i32* __restrict__ subCt, i32* __restrict__ delCt, unsigned char* __restrict__ insBase,
			i32* __restrict__ insCt, unsigned char* __restrict__ flags, u32* __restrict__ isTotal, u32* __restrict__ isSub,
			u32* __restrict__ isDel, u32* __restrict__ isIns)
{
	const u32 g = blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (g > nPos) return;
	if (g == nPos) { isTotal[g] = 0; isSub[g] = 0; isDel[g] = 0; isIns[g] = 0; return; }
	const u32* mRow = matCnt + (u64)g * nB;
	const u32* iRow = insCnt + (u64)g * nB;
	const unsigned long long* mFirst = matFirst + (u64)g * nB;
	const unsigned long long* iFirst = insFirst + (u64)g * nB;
	const unsigned long long tg = tag[g];
	const unsigned char nu = tg ? (unsigned char)(tg & 0xffu) : (unsigned char)'-';
	const u32 rNucl = rank[nu & 127], rGap = rank['-'];
	u32 total = 0;
	for (u32 r = 0; r < nB; ++r) total += mRow[r];
	u32 sRank = DV_NONE, sCnt = 0, iRank = DV_NONE, iCnt = 0;
	DV_BEST(mRow, mFirst, rNucl, rGap, sRank, sCnt)
	DV_BEST(iRow, iFirst, DV_NONE, DV_NONE, iRank, iCnt)
	const u32 mc = rNucl < nB ? mRow[rNucl] : 0u, dc = rGap < nB ? mRow[rGap] : 0u;
	// cov <= the alignments of the contig < nCov; a table entry says the smallest count that reaches the threshold
	unsigned char fl = 0;
	if (total != 0 && total < nCov)
	{
		if (sCnt >= minCt[total]) fl |= 1;
		if (dc >= minCt[nCov + total]) fl |= 2;
		if (iCnt >= minCt[2 * nCov + total]) fl |= 4;
	}
	cov[g] = (i32)total; nucl[g] = nu; matCt[g] = (i32)mc;
	subBase[g] = sRank != DV_NONE ? byteOf[sRank] : (unsigned char)0; subCt[g] = (i32)sCnt;
	delCt[g] = (i32)dc;
	insBase[g] = iRank != DV_NONE ? byteOf[iRank] : (unsigned char)0; insCt[g] = (i32)iCnt;
	flags[g] = fl;
	isTotal[g] = fl ? 1u : 0u; isSub[g] = fl & 1 ? 1u : 0u; isDel[g] = fl & 2 ? 1u : 0u; isIns[g] = fl & 4 ? 1u : 0u;
}

// the four lists: a flagged position writes its index inside its contig at the scanned place
__global__ void __launch_bounds__(BUB_BLOCK)
k_dv_compact(u32 nPos, const u64* __restrict__ ctgAt, u32 nC, const unsigned char* __restrict__ flags, const u32* __restrict__ offTotal,
			 const u32* __restrict__ offSub, const u32* __restrict__ offDel, const u32* __restrict__ offIns, i32* __restrict__ lTotal,
			 i32* __restrict__ lSub, i32* __restrict__ lDel, i32* __restrict__ lIns)
{
	const u32 g = blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (g >= nPos) return;
	const unsigned char fl = flags[g];
	if (!fl) return;
	const i32 p = (i32)(g - ctgAt[dv_find(ctgAt, nC, g)]);
	lTotal[offTotal[g]] = p;
	if (fl & 1) lSub[offSub[g]] = p;
	if (fl & 2) lDel[offDel[g]] = p;
	if (fl & 4) lIns[offIns[g]] = p;
}

// the lists' starts per contig: row k of out = off_k[ctgAt[i]]
__global__ void __launch_bounds__(BUB_BLOCK)
k_dv_pick(u32 n, const u64* __restrict__ at, const u32* __restrict__ off0, const u32* __restrict__ off1, const u32* __restrict__ off2,
		  const u32* __restrict__ off3, u32* __restrict__ out)
{
	const u32 i = blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (i >= n) return;
	const u64 p = at[i];
	out[i] = off0[p]; out[n + i] = off1[p]; out[2 * n + i] = off2[p]; out[3 * n + i] = off3[p];
}

// present[0 .. 4) |= the set of the bytes (below 128) of the pieces seq[start[i] .. start[i] + len[i]), each mapped as
// k_cig_expand maps a SEQ byte before it stores it: bit b of the 128 stands for byte b.  One wave per piece, in the manner
// of k_col_present (fg_contigcons.hip): whole 8-byte words where the address allows, the piece's first bytes up to the
// next word boundary and its last bytes one per lane; four mask registers, folded over the wave by a butterfly; lane 0
// issues one atomic per word that has a bit.  No LDS.
__global__ void __launch_bounds__(BUB_BLOCK)
k_seq_present(const u32* __restrict__ start, const u32* __restrict__ len, u32 nSeg, const unsigned char* __restrict__ seq, u32* present)
{
	const int lane = threadIdx.x & 63;
	const u32 g = blockIdx.x * BUB_WAVES + (threadIdx.x >> 6);
	if (g >= nSeg) return;
	const unsigned char* q = seq + start[g];
	const u64 n = len[g];
	u32 m[4] = {0u, 0u, 0u, 0u};
	const auto mark = [&m](u32 raw)
	{
		const u32 b = cig_upper((unsigned char)raw);
		const u32 bit = 1u << (b & 31u), w = (b >> 5) & 3u;
		m[0] |= w == 0 ? bit : 0u; m[1] |= w == 1 ? bit : 0u; m[2] |= w == 2 ? bit : 0u; m[3] |= w == 3 ? bit : 0u;
	};
	const u64 toBoundary = (8 - ((uintptr_t)q & 7)) & 7;
	const u64 head = toBoundary < n ? toBoundary : n;
	const u64 nWords = (n - head) / 8, tail0 = head + 8 * nWords;
	if ((u64)lane < head) mark(q[lane]);
	const u64* qw = (const u64*)(q + head);
	for (u64 w = lane; w < nWords; w += 64)
	{
		const u64 v = qw[w];
#pragma unroll
		for (int i = 0; i < 8; ++i) mark((u32)(v >> (8 * i)) & 0xffu);
	}
	if (tail0 + (u64)lane < n) mark(q[tail0 + lane]);
#pragma unroll
	for (int k = 0; k < 4; ++k)
	{
		u32 v = m[k];
#pragma unroll
		for (int sh = 32; sh > 0; sh >>= 1) v |= __shfl_xor(v, sh);
		if (lane == 0 && v) atomicOr(&present[k], v);
	}
}

struct DivergenceOwner {
	std::vector<uint64_t> listOff[4], profOff;		// total, sub, del, ins
	std::vector<int32_t> list[4];
	std::vector<int32_t> cov, matCt, subCt, delCt, insCt;
	std::vector<uint8_t> nucl, subBase, insBase, flags;
};

// the smallest count ct with (double)ct / (double)cov >= thresh, as _call_position divides; 0xffffffff: none a
// sub-batch can reach (its counts stay below 2^31)
u32 dvMinCount(double thresh, u32 cov)
{
	const double want = thresh * (double)cov;
	if (!(want < 2147483648.0)) return 0xffffffffu;
	u64 ct = (u64)std::ceil(want);
	while (ct > 0 && (double)(ct - 1) / (double)cov >= thresh) --ct;
	while ((double)ct / (double)cov < thresh) ++ct;
	return ct < 0xffffffffULL ? (u32)ct : 0xffffffffu;
}

void dvSubBatch(fg_ctx* c, u32 c0, u32 c1, const double* thresh, const int32_t* contigLen, const uint64_t* contigAlnOff,
				const int32_t* trgStart, const uint64_t* colOff, const uint8_t* trgCols, const uint8_t* qryCols,
				const unsigned char* rank, const unsigned char* byteOf, u32 nB, bool wantProfile, DivergenceOwner& own,
				const CigSource* cig = nullptr /* the columns are expanded here, not read from the host */)
{
	hipStream_t s = c->stream;
	const u32 nC = c1 - c0;
	const u64 a0 = contigAlnOff[c0], a1 = contigAlnOff[c1];
	const u32 nAln = (u32)(a1 - a0);
	const u64 col0 = nAln ? colOff[a0] : 0, nCols = nAln ? colOff[a1] - col0 : 0;

	std::vector<DvContig> ctg(nC);
	std::vector<BubAln> alns(nAln);
	std::vector<u32> tileOff((size_t)nAln + 1, 0);
	std::vector<u64> ctgAt((size_t)nC + 1);
	u64 nPos = 0, nTiles = 0, maxAlns = 0;
	for (u32 i = 0; i < nC; ++i)
	{
		ctg[i] = DvContig{nPos, contigLen[c0 + i], 0};
		ctgAt[i] = nPos;
		nPos += (u64)contigLen[c0 + i];
		maxAlns = std::max<u64>(maxAlns, contigAlnOff[c0 + i + 1] - contigAlnOff[c0 + i]);
		for (u64 a = contigAlnOff[c0 + i]; a < contigAlnOff[c0 + i + 1]; ++a)
		{
			BubAln& al = alns[a - a0];
			al.colOff = colOff[a] - col0; al.nCols = (u32)(colOff[a + 1] - colOff[a]);
			al.trgStart = trgStart[a]; al.trgEnd = 0; al.contig = i; al.inProfile = 1; al.pad = 0;
			tileOff[a - a0] = (u32)nTiles;
			nTiles += ((u64)al.nCols + DV_TILE - 1) / DV_TILE;
		}
	}
	ctgAt[nC] = nPos;
	tileOff[nAln] = (u32)nTiles;
	if (nPos >= (1ULL << 31) || nAln >= (1u << 23) || nCols >= (1ULL << 31))
		throw FgError{FG_ERR_NOMEM, "fg_divergence_profile: a sub-batch of 2^31 positions or columns or 2^23 alignments; lower FG_DIVERGENCE_BATCH_COLS"};
	if (nPos * nB >= (1ULL << 32))
		throw FgError{FG_ERR_NOMEM, "fg_divergence_profile: the count tables of a sub-batch have 2^32 cells (" + std::to_string(nB) +
										" distinct bytes); lower FG_DIVERGENCE_BATCH_COLS"};
	// a position's coverage is at most the alignments of its contig: every alignment passes a position once
	const u32 nCov = (u32)maxAlns + 1;
	std::vector<u32> minCt((size_t)3 * nCov, 0xffffffffu);
	for (int k = 0; k < 3; ++k)
		for (u32 v = 1; v < nCov; ++v) minCt[(size_t)k * nCov + v] = dvMinCount(thresh[k], v);

	const u64 nCell = nPos * nB;
	DevPool B{c->dDv, "fg_divergence"};
	BubAln* dAln = B.get<BubAln>(nAln);
	DvContig* dCtg = B.get<DvContig>(nC);
	u64* dCtgAt = B.get<u64>((size_t)nC + 1);
	u32* dTileOff = B.get<u32>((size_t)nAln + 1);
	u32* dTileNg = B.get<u32>(nTiles + 1);
	// k_cig_expand stores whole words past the last column
	unsigned char* dTrg = B.get<unsigned char>(nCols + (cig ? CIG_LANE_COLS : 0));
	unsigned char* dQry = B.get<unsigned char>(nCols + (cig ? CIG_LANE_COLS : 0));
	unsigned char* dTrgS = B.get<unsigned char>(nCols);
	unsigned char* dQryS = B.get<unsigned char>(nCols);
	unsigned char* dTab = B.get<unsigned char>(256);
	u32* dMinCt = B.get<u32>((size_t)3 * nCov);
	u32* dCnt = B.get<u32>(2 * nCell);						// matches, insertions
	unsigned long long* dFirst = B.get<unsigned long long>(2 * nCell);
	unsigned long long* dTag = B.get<unsigned long long>(nPos);
	u32* dScan = B.get<u32>(fgprim::scanScratchElems(std::max<u64>(nPos + 1, nTiles + 1)) + 8);
	i32* dVal = B.get<i32>(5 * nPos);						// cov, mat_ct, sub_ct, del_ct, ins_ct
	unsigned char* dBytes = B.get<unsigned char>(4 * nPos);	// nucl, sub_base, ins_base, flags
	u32* dIs = B.get<u32>(4 * (nPos + 1));					// the four flag arrays, then their sums
	u32* dListAt = B.get<u32>(4 * ((size_t)nC + 1));
	u32 *dMat = dCnt, *dIns = dCnt + nCell;
	unsigned long long *dMatFirst = dFirst, *dInsFirst = dFirst + nCell;
	unsigned char *dNucl = dBytes, *dSubBase = dBytes + nPos, *dInsBase = dBytes + 2 * nPos, *dFlags = dBytes + 3 * nPos;
	u32* dOff[4];
	for (int k = 0; k < 4; ++k) dOff[k] = dIs + (size_t)k * (nPos + 1);

	HIP_CHECK(hipMemcpyAsync(dAln, alns.data(), (size_t)nAln * sizeof(BubAln), hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dCtg, ctg.data(), (size_t)nC * sizeof(DvContig), hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dCtgAt, ctgAt.data(), ((size_t)nC + 1) * 8, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dTileOff, tileOff.data(), ((size_t)nAln + 1) * 4, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dMinCt, minCt.data(), (size_t)3 * nCov * 4, hipMemcpyHostToDevice, s));
	CigStaged staged;		// read by the expansion's uploads: alive until the stream has been waited for
	if (cig && nAln) (void)cigExpandSource(c, *cig, staged, a0, a1, dTrg, dQry);
	else if (nCols)
	{
		HIP_CHECK(hipMemcpyAsync(dTrg, trgCols + col0, nCols, hipMemcpyHostToDevice, s));
		HIP_CHECK(hipMemcpyAsync(dQry, qryCols + col0, nCols, hipMemcpyHostToDevice, s));
	}
	HIP_CHECK(hipMemcpyAsync(dTab, rank, 128, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dTab + 128, byteOf, 128, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemsetAsync(dCnt, 0, 2 * nCell * 4 + 4, s));
	HIP_CHECK(hipMemsetAsync(dFirst, 0xff, 2 * nCell * 8 + 8, s));
	HIP_CHECK(hipMemsetAsync(dTag, 0, nPos * 8 + 8, s));
	HIP_CHECK(hipMemsetAsync(dTileNg, 0, (nTiles + 1) * 4, s));

	if (nAln)
	{
		ScopedK t(c->timer, "k_bub_shift");
		hipLaunchKernelGGL(k_bub_shift, bubWaveGrid(nAln), BUB_BLOCK, 0, s, dAln, nAln, dTrg, dQry, dQryS);
		hipLaunchKernelGGL(k_bub_shift, bubWaveGrid(nAln), BUB_BLOCK, 0, s, dAln, nAln, dQryS, dTrg, dTrgS);
	}
	if (nTiles)
	{
		{
			ScopedK t(c->timer, "k_dv_tiles");
			hipLaunchKernelGGL(k_dv_tiles, bubWaveGrid(nTiles), BUB_BLOCK, 0, s, dAln, nAln, dTileOff, (u32)nTiles, dTrgS, dTileNg);
		}
		{
			ScopedK t(c->timer, "k_dv_scan");
			fgprim::scan<u32>(s, dTileNg, dTileNg, nTiles + 1, false, dScan);
		}
		ScopedK t(c->timer, "k_dv_count");
		hipLaunchKernelGGL(k_dv_count, bubWaveGrid(nTiles), BUB_BLOCK, 0, s, dAln, nAln, dCtg, dTileOff, (u32)nTiles, dTileNg, dTrgS, dQryS, dTab,
						   nB, dMat, dIns, dMatFirst, dInsFirst, dTag);
	}
	{
		ScopedK t(c->timer, "k_dv_finish");
		hipLaunchKernelGGL(k_dv_finish, bubGrid(nPos + 1), BUB_BLOCK, 0, s, (u32)nPos, dMat, dIns, dMatFirst, dInsFirst, dTag,
						   dTab, dTab + 128, nB, dMinCt, nCov, dVal, dNucl, dVal + nPos, dSubBase, dVal + 2 * nPos,
						   dVal + 3 * nPos, dInsBase, dVal + 4 * nPos, dFlags, dOff[0], dOff[1], dOff[2], dOff[3]);
	}
	{
		ScopedK t(c->timer, "k_dv_scan");
		for (int k = 0; k < 4; ++k) fgprim::scan<u32>(s, dOff[k], dOff[k], nPos + 1, false, dScan);
		hipLaunchKernelGGL(k_dv_pick, bubGrid((u64)nC + 1), BUB_BLOCK, 0, s, nC + 1, dCtgAt, dOff[0], dOff[1], dOff[2], dOff[3], dListAt);
	}
	HIP_CHECK(hipGetLastError());
	std::vector<u32> listAt(4 * ((size_t)nC + 1));
	HIP_CHECK(hipMemcpyAsync(listAt.data(), dListAt, listAt.size() * 4, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	u32 nList[4];
	i32* dList[4];
	for (int k = 0; k < 4; ++k)
	{
		nList[k] = listAt[(size_t)k * (nC + 1) + nC];
		dList[k] = B.get<i32>(nList[k]);
	}
	if (nList[0])
	{
		ScopedK t(c->timer, "k_dv_compact");
		hipLaunchKernelGGL(k_dv_compact, bubGrid(nPos), BUB_BLOCK, 0, s, (u32)nPos, dCtgAt, nC, dFlags, dOff[0], dOff[1], dOff[2], dOff[3],
						   dList[0], dList[1], dList[2], dList[3]);
	}
	HIP_CHECK(hipGetLastError());
	for (int k = 0; k < 4; ++k)
	{
		const size_t base = own.list[k].size();
		own.list[k].resize(base + nList[k]);
		if (nList[k]) HIP_CHECK(hipMemcpyAsync(own.list[k].data() + base, dList[k], (size_t)nList[k] * 4, hipMemcpyDeviceToHost, s));
		for (u32 i = 0; i < nC; ++i) own.listOff[k].push_back(base + listAt[(size_t)k * (nC + 1) + i + 1]);
	}
	if (wantProfile)
	{
		const size_t at = own.cov.size();
		for (u32 i = 0; i < nC; ++i) own.profOff.push_back(at + ctgAt[i + 1]);
		std::vector<int32_t>* v32[5] = {&own.cov, &own.matCt, &own.subCt, &own.delCt, &own.insCt};
		std::vector<uint8_t>* v8[4] = {&own.nucl, &own.subBase, &own.insBase, &own.flags};
		for (int k = 0; k < 5; ++k)
		{
			v32[k]->resize(at + nPos);
			if (nPos) HIP_CHECK(hipMemcpyAsync(v32[k]->data() + at, dVal + (size_t)k * nPos, nPos * 4, hipMemcpyDeviceToHost, s));
		}
		for (int k = 0; k < 4; ++k)
		{
			v8[k]->resize(at + nPos);
			if (nPos) HIP_CHECK(hipMemcpyAsync(v8[k]->data() + at, dBytes + (size_t)k * nPos, nPos, hipMemcpyDeviceToHost, s));
		}
	}
	HIP_CHECK(hipStreamSynchronize(s));
}

// the query bytes of a call, ranked in byte order: the width of the count tables
u32 dvRankBytes(const bool* present, unsigned char* rank, unsigned char* byteOf)
{
	memset(rank, DV_NONE, 128);
	memset(byteOf, 0, 128);
	u32 nB = 0;
	for (int b = 0; b < 128; ++b)
		if (present[b]) { rank[b] = (unsigned char)nB; byteOf[nB++] = (unsigned char)b; }
	if (nB == 0) { rank['-'] = 0; byteOf[0] = '-'; nB = 1; }
	return nB;
}

// The set of query bytes the columns of the alignments a0 .. a1 would show, from the records (checked by cigCheckRecords):
// the SEQ bytes that M and I runs consume, as k_cig_expand stores them, and '-' where a D run has a length.  Zero-length
// runs, clipped bytes and the bytes of SEQ behind the consumed part give nothing.  The SEQ bytes go up in pieces of whole
// alignments of at most `chunk` bytes (one alignment at least) into a buffer of the expansion's pool; where ONE piece
// holds the call it stays there and the pointer is returned for the expansion to read, otherwise NULL.
const unsigned char* dvPresentOfRecords(fg_ctx* c, u64 a0, u64 a1, const uint64_t* runOff, const uint8_t* runOp, const uint32_t* runLen,
										const uint64_t* readOff, const uint8_t* readSeq, u64 chunk, bool* present)
{
	hipStream_t s = c->stream;
	u32 mask[4] = {};
	bool resident = false;
	const unsigned char* dSeq = nullptr;
	std::vector<u32> segStart, segLen;
	for (u64 b0 = a0; b0 < a1;)
	{
		u64 b1 = b0 + 1;
		while (b1 < a1 && readOff[b1 + 1] - readOff[b0] <= chunk) ++b1;
		const u64 rd0 = readOff[b0], nBytes = readOff[b1] - rd0;
		segStart.clear(); segLen.clear();
		for (u64 a = b0; a < b1; ++a)
		{
			u64 qpos = readOff[a] - rd0, open = ~0ULL;		// open: where the piece under way ends
			for (u64 r = runOff[a]; r < runOff[a + 1]; ++r)
			{
				const u64 l = runLen[r];
				const unsigned char o = runOp[r];
				if (l == 0) continue;
				if (o == 'D') present['-'] = true;
				else if (o == 'S') qpos += l;
				else if (o == 'M' || o == 'I')
				{
					if (open == qpos) segLen.back() += (u32)l;
					else { segStart.push_back((u32)qpos); segLen.push_back((u32)l); }
					qpos += l; open = qpos;
				}
			}
		}
		if (nBytes >= (1ULL << 32))
			throw FgError{FG_ERR_NOMEM, "fg_divergence_profile_cigars: an alignment with 2^32 SEQ bytes"};
		const u32 nSeg = (u32)segStart.size();
		if (nSeg)
		{
			DevPool B = cigPool(c, 12);			// behind the buffers of cigExpandOnDevice and its callers
			unsigned char* dBytes = B.get<unsigned char>(nBytes);
			u32* dStart = B.get<u32>(nSeg);
			u32* dLen = B.get<u32>(nSeg);
			u32* dPresent = B.get<u32>(4);
			HIP_CHECK(hipMemcpyAsync(dBytes, readSeq + rd0, nBytes, hipMemcpyHostToDevice, s));
			HIP_CHECK(hipMemcpyAsync(dStart, segStart.data(), (size_t)nSeg * 4, hipMemcpyHostToDevice, s));
			HIP_CHECK(hipMemcpyAsync(dLen, segLen.data(), (size_t)nSeg * 4, hipMemcpyHostToDevice, s));
			HIP_CHECK(hipMemsetAsync(dPresent, 0, 16, s));
			{
				ScopedK t(c->timer, "k_seq_present");
				hipLaunchKernelGGL(k_seq_present, bubWaveGrid(nSeg), BUB_BLOCK, 0, s, dStart, dLen, nSeg, dBytes, dPresent);
			}
			HIP_CHECK(hipGetLastError());
			u32 m[4] = {};
			HIP_CHECK(hipMemcpyAsync(m, dPresent, 16, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipStreamSynchronize(s));		// also keeps segStart / segLen alive until their copies have run
			for (int k = 0; k < 4; ++k) mask[k] |= m[k];
			resident = b0 == a0 && b1 == a1;
			dSeq = dBytes;
		}
		b0 = b1;
	}
	for (int b = 0; b < 128; ++b)
		if ((mask[b >> 5] >> (b & 31)) & 1u) present[b] = true;
	return resident ? dSeq : nullptr;
}

// the finished owner into the caller's struct
void dvHandOver(struct fg_divergence_batch* out, DivergenceOwner* own, uint32_t n_contigs, bool wantProfile)
{
	out->n_contigs = n_contigs;
	out->total_off = own->listOff[0].data(); out->total_pos = own->list[0].data();
	out->sub_off = own->listOff[1].data(); out->sub_pos = own->list[1].data();
	out->del_off = own->listOff[2].data(); out->del_pos = own->list[2].data();
	out->ins_off = own->listOff[3].data(); out->ins_pos = own->list[3].data();
	if (wantProfile)
	{
		out->prof_off = own->profOff.data();
		out->cov = own->cov.data();
		out->nucl = own->nucl.data();
		out->mat_ct = own->matCt.data();
		out->sub_base = own->subBase.data();
		out->sub_ct = own->subCt.data();
		out->del_ct = own->delCt.data();
		out->ins_base = own->insBase.data();
		out->ins_ct = own->insCt.data();
		out->flags = own->flags.data();
	}
	out->owner_ = own;
}

} // namespace

extern "C" {

int fg_divergence_profile(fg_ctx* c, double sub_thresh, double del_thresh, double ins_thresh, uint32_t n_contigs,
						  const int32_t* contig_len, const uint64_t* contig_aln_off, const int32_t* trg_start, const uint64_t* col_off,
						  const uint8_t* trg_cols, const uint8_t* qry_cols, uint8_t want_profile, struct fg_divergence_batch* out)
{
	return stageCall<DivergenceOwner>(c, out, [&](DivergenceOwner*& own)
	{
		const std::string name = "fg_divergence_profile";
		if (!out) throw FgError{FG_ERR_ARG, name + ": null result"};
		const double thresh[3] = {sub_thresh, del_thresh, ins_thresh};
		for (double t : thresh)
			if (!(t >= 0.0)) throw FgError{FG_ERR_ARG, name + ": a threshold that is NaN or negative"};
		stageContigTable(name, n_contigs, contig_len, contig_aln_off);
		const u64 a0 = n_contigs ? contig_aln_off[0] : 0, a1 = n_contigs ? contig_aln_off[n_contigs] : 0;
		if (a1 > a0 && (!trg_start || !col_off)) throw FgError{FG_ERR_ARG, name + ": null trg_start or col_off"};
		stageColOff(name, col_off, a0, a1, trg_cols, qry_cols);
		bool present[128] = {};
		for (u32 i = 0; i < n_contigs; ++i)
			for (u64 a = contig_aln_off[i]; a < contig_aln_off[i + 1]; ++a)
			{
				// the order of the reports is part of the call: the bytes first, then trg_start (fg_make_bubbles: trg_start first)
				const u64 nonGap = stageColumnWalk(name, a, col_off, trg_cols, qry_cols, present);
				stageStartOnContig(name, a, trg_start[a], contig_len[i]);
				stageBasesOnContig(name, a, nonGap, contig_len[i]);
			}
		// the query bytes of the call, ranked in byte order: the width of the count tables
		unsigned char rank[128], byteOf[128];
		const u32 nB = dvRankBytes(present, rank, byteOf);
		// a contig counts its columns and a table row per position
		std::vector<u64> cost(n_contigs, 0);
		for (u32 i = 0; i < n_contigs; ++i)
		{
			cost[i] = (u64)contig_len[i] * nB;
			if (contig_aln_off[i + 1] > contig_aln_off[i]) cost[i] += col_off[contig_aln_off[i + 1]] - col_off[contig_aln_off[i]];
		}
		const u64 budget = stageEnvU64("FG_DIVERGENCE_BATCH_COLS", 1ULL << 27);
		const u64 maxContigs = stageEnvCap("FG_DIVERGENCE_BATCH_CONTIGS");
		stageAllFit(name, "contig", cost, budget, "columns and table cells", "FG_DIVERGENCE_BATCH_COLS");
		own = new DivergenceOwner;
		for (auto& v : own->listOff) v.assign(1, 0);
		if (want_profile) own->profOff.assign(1, 0);
		HIP_CHECK(hipSetDevice(c->device));
		c->timer.reset();
		for (u32 i = 0; i < n_contigs;)
		{
			const u32 j = stageCut(i, n_contigs, cost, budget, maxContigs);
			dvSubBatch(c, i, j, thresh, contig_len, contig_aln_off, trg_start, col_off, trg_cols, qry_cols, rank, byteOf, nB, want_profile != 0, *own);
			i = j;
		}
		c->timer.collect();
		for (auto& v : own->list) stageKeep(v);
		stageKeep(own->cov, own->matCt, own->subCt, own->delCt, own->insCt, own->nucl, own->subBase, own->insBase, own->flags);
		dvHandOver(out, own, n_contigs, want_profile != 0);
	});
}

int fg_divergence_profile_cigars(fg_ctx* c, double sub_thresh, double del_thresh, double ins_thresh, uint32_t n_contigs,
								 const uint64_t* contig_off, const uint8_t* contig_seq, const uint64_t* contig_aln_off,
								 const int32_t* ctg_pos, const uint64_t* run_off, const uint8_t* run_op, const uint32_t* run_len,
								 const uint64_t* read_off, const uint8_t* read_seq, uint8_t want_profile, struct fg_divergence_batch* out)
{
	return stageCall<DivergenceOwner>(c, out, [&](DivergenceOwner*& own)
	{
		const std::string name = "fg_divergence_profile_cigars";
		if (!out) throw FgError{FG_ERR_ARG, name + ": null result"};
		if (n_contigs && !contig_aln_off) throw FgError{FG_ERR_ARG, name + ": null contig_aln_off"};
		stageOffsets(name, "contig_aln_off", "contig ", contig_aln_off, 0, n_contigs);
		const u64 a0 = n_contigs ? contig_aln_off[0] : 0, a1 = n_contigs ? contig_aln_off[n_contigs] : 0;
		std::vector<uint32_t> alnContig((size_t)a1, 0);
		for (u32 i = 0; i < n_contigs; ++i)
			for (u64 a = contig_aln_off[i]; a < contig_aln_off[i + 1]; ++a) alnContig[a] = i;
		// every check of fg_expand_cigars, then those fg_divergence_profile makes on what the expansion would hand it
		CigPlan plan;
		cigCheckRecords(name, n_contigs, contig_off, contig_seq, a0, a1, alnContig.data(), !ctg_pos || !run_off || !read_off,
						"null ctg_pos, run_off or read_off", ctg_pos, run_off, run_op, run_len, read_off, read_seq, plan);
		const double thresh[3] = {sub_thresh, del_thresh, ins_thresh};
		for (double t : thresh)
			if (!(t >= 0.0)) throw FgError{FG_ERR_ARG, name + ": a threshold that is NaN or negative"};
		// No walk over columns on the host.  What fg_divergence_profile reads from them holds by construction after
		// cigCheckRecords: every contig and SEQ byte is below 128, so every column is; the non-gap target columns of an
		// alignment are the contig bytes its runs consume, which end on the contig.  trg_start does not: an alignment of
		// insertions alone may stand behind the last base.
		std::vector<int32_t> contigLen(n_contigs, 0);
		for (u32 i = 0; i < n_contigs; ++i)
		{
			if (contig_off[i + 1] - contig_off[i] > CIG_I32) throw FgError{FG_ERR_ARG, name + ": contig " + std::to_string(i) + " has 2^31 bytes"};
			contigLen[i] = (int32_t)(contig_off[i + 1] - contig_off[i]);
			for (u64 a = contig_aln_off[i]; a < contig_aln_off[i + 1]; ++a) stageStartOnContig(name, a, plan.trgStart[a], contigLen[i]);
		}
		const u64 budget = stageEnvU64("FG_DIVERGENCE_BATCH_COLS", 1ULL << 27);
		const u64 maxContigs = stageEnvCap("FG_DIVERGENCE_BATCH_CONTIGS");
		HIP_CHECK(hipSetDevice(c->device));
		c->timer.reset();
		// the query bytes of the call decide every contig's cost, so they are found from the records, before the cut
		bool present[128] = {};
		const unsigned char* dSeq = a1 > a0 ? dvPresentOfRecords(c, a0, a1, run_off, run_op, run_len, read_off, read_seq,
																 std::max<u64>(1, std::min<u64>(budget, CIG_I32)), present) : nullptr;
		unsigned char rank[128], byteOf[128];
		const u32 nB = dvRankBytes(present, rank, byteOf);
		// a contig counts its columns and a table row per position
		std::vector<u64> cost(n_contigs, 0);
		for (u32 i = 0; i < n_contigs; ++i)
			cost[i] = (u64)contigLen[i] * nB + (plan.colOff[contig_aln_off[i + 1]] - plan.colOff[contig_aln_off[i]]);
		stageAllFit(name, "contig", cost, budget, "columns and table cells", "FG_DIVERGENCE_BATCH_COLS");
		own = new DivergenceOwner;
		for (auto& v : own->listOff) v.assign(1, 0);
		if (want_profile) own->profOff.assign(1, 0);
		// the contig bytes go up once per call; a sub-batch expands its own alignments.  The SEQ bytes k_seq_present has read
		// serve the expansion where one sub-batch holds every alignment of the call.
		CigSource src{&plan, a1 > a0 ? cigUploadContigs(c, plan, contig_seq) : nullptr, run_off, run_op, run_len, read_off, read_seq, cigTile()};
		for (u32 i = 0; i < n_contigs;)
		{
			const u32 j = cigCutContigs(name, "FG_DIVERGENCE_BATCH_COLS", i, n_contigs, cost, budget, maxContigs, contig_aln_off, run_off, read_off);
			if (dSeq && contig_aln_off[i] == a0 && contig_aln_off[j] == a1) { src.dSeq = dSeq; src.seq0 = read_off[a0]; }
			else src.dSeq = nullptr;
			dvSubBatch(c, i, j, thresh, contigLen.data(), contig_aln_off, plan.trgStart.data(), plan.colOff.data(), nullptr, nullptr, rank, byteOf,
					   nB, want_profile != 0, *own, &src);
			i = j;
		}
		c->timer.collect();
		for (auto& v : own->list) stageKeep(v);
		stageKeep(own->cov, own->matCt, own->subCt, own->delCt, own->insCt, own->nucl, own->subBase, own->insBase, own->flags);
		dvHandOver(out, own, n_contigs, want_profile != 0);
	});
}

void fg_release_divergence(struct fg_divergence_batch* b) { stageRelease<DivergenceOwner>(b); }

} // extern "C"
