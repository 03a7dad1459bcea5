// fg_uniform_alignments and fg_contig_consensus: the reference's consensus stage (flye/polishing/consensus.py:108-181,
// _contig_profile and _flatten_profile) and the coverage cap in front of it (flye/polishing/alignment.py:95-153,
// get_uniform_alignments) on the device.  Integers and exact compares only: a non-negative double orders as its bit
// pattern, so the error rates travel and sort as 64-bit words.
//
// fg_uniform_alignments, per sub-batch of whole contigs (FG_UNIFORM_BATCH_PAIRS); windows are numbered over the sub-batch:
//   k_uni_emit      one thread per (alignment, window) pair: the pair (err_rate bits, window); the first pair of an
//                   alignment also adds +1 / -1 to the difference arrays of all and of primary alignments.
//   (scan)          inclusive sums of the difference arrays = entries and primary coverage per window; exclusive sums of
//                   the entries = where a window's list starts.
//   (sort)          two stable radix sorts, by the bits and then by the window: every window's list ascending, in place.
//   k_uni_medkeys   one thread per window: (contig << 32 | primary coverage); a third sort leaves every contig's
//                   coverages ascending.
//   k_uni_median    one thread per contig: m2 = twice the median, cov_threshold = max(5 * m2 / 8, 10).  The reference's
//                   int(1.25 * median) is exact in double: median = m2 / 2 and 1.25 * median = 5 * m2 / 8 have at most
//                   three fractional bits below 2^35, so the product is not rounded and int() is the floor.
//   k_uni_thresh    one thread per window: element cov_threshold of its list, or 1.0.
//   k_uni_keep      one thread per alignment: good windows against floor(total / 2).
//
// fg_contig_consensus, per sub-batch of whole contigs (FG_CONSENSUS_BATCH_COLS):
//   k_bub_shift     (fg_gapshift.h) both shift_gaps passes, alignments in use only.
//   k_cc_count      one wave per alignment: its insertion columns (target gap, query base); a scan numbers the records.
//   k_cc_profile    one wave per alignment: positions by ballot prefix counts as in k_bub_profile.  An insertion column
//                   writes the record (position << 32 | read, byte) into its slot: slots run in (alignment, column) order.
//                   Every other column adds to matches[position][rank of the query byte] (a dense table over the bytes
//                   present in the sub-batch, ranked on the host in byte order) and takes nucl by an atomic max of
//                   (alignment + 1) << 40 | column << 8 | target byte: the last writer in list order, then column order.
//   (sort)          one stable radix sort by (position, read): with the slot order that is (position, read, alignment,
//                   column), so the bytes of one read at one position stand together as its insertion string.
//   k_cc_heads      one thread per record: first / last record of every position, and the list of positions with records.
//   k_cc_vote       one wave per listed position: the starts of the strings by ballots, then lane j counts the strings
//                   equal to string j (strings of any length: a lane walks the bytes), and a butterfly over (count, string)
//                   leaves the most frequent one, ties to the smallest in byte order with a proper prefix first.
//   k_cc_flatten    one thread per position: match_total, max_match (the first rank of the largest count), the accepted
//                   flag and the bytes the position gives; a scan places them; k_cc_write writes them.
// The host does work proportional to contigs, alignments and (for the byte check) columns.
//
// fg_contig_consensus_cigars takes SAM records where fg_contig_consensus takes columns: a sub-batch expands its own
// alignments (fg_cigexpand.h) on the context's stream straight into the two column buffers, so no column crosses the bus.
// The one thing the host read from the columns besides checks, the set of query bytes present, comes from
//   k_col_present   one wave per alignment in use: a 128-bit mask of its query bytes, ORed over the wave, one atomic per
//                   wave and word onto four words that the host reads before it sizes the match table.
#include "fg_ctx.h"
#include "fg_stage.h"
#include "fg_devprim.h"
#include "fg_gapshift.h"
#include "fg_cigexpand.h"
#include <cmath>

namespace {

struct UniAln { u32 w0; u32 nW; i32 total; u32 primary; };
struct CcContig { u64 posOff; i32 len; u32 pad; };

// the last i in [0, n) with off[i] <= x (off ascending, off[0] <= x)
template <class T>
__device__ __forceinline__ u32 cc_find(const T* __restrict__ off, u32 n, u64 x)
{
	u32 lo = 0, hi = n;
	while (hi - lo > 1)
	{
		const u32 mid = (lo + hi) >> 1;
		if ((u64)off[mid] <= x) lo = mid; else hi = mid;
	}
	return lo;
}

// ---- fg_uniform_alignments --------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BUB_BLOCK)
k_uni_emit(u64 nPairs, const UniAln* __restrict__ alns, const u32* __restrict__ pairOff, u32 nAln, const u64* __restrict__ errBits,
		   u64* __restrict__ keys, u64* __restrict__ vals, u32* diffAll, u32* diffPrim)
{
	const u64 g = (u64)blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (g >= nPairs) return;
	const u32 a = cc_find(pairOff, nAln, g);
	const UniAln al = alns[a];
	const u32 j = (u32)(g - pairOff[a]);
	keys[g] = errBits[a];
	vals[g] = (u64)al.w0 + j;
	if (j == 0)
	{
		atomicAdd(&diffAll[al.w0], 1u);
		atomicAdd(&diffAll[al.w0 + al.nW], 0xffffffffu);
		if (al.primary)
		{
			atomicAdd(&diffPrim[al.w0], 1u);
			atomicAdd(&diffPrim[al.w0 + al.nW], 0xffffffffu);
		}
	}
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_uni_medkeys(u32 nWin, const u32* __restrict__ winBase, u32 nC, const u32* __restrict__ prim, u64* __restrict__ keys, u64* __restrict__ vals)
{
	const u32 w = blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (w >= nWin) return;
	const u32 c = cc_find(winBase, nC, w);
	keys[w] = ((u64)c << 32) | prim[w];
	vals[w] = w;
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_uni_median(u32 nC, const u32* __restrict__ winBase, const u64* __restrict__ sorted, i32* __restrict__ covThr)
{
	const u32 c = blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (c >= nC) return;
	const u32 b = winBase[c], n = winBase[c + 1] - b;		// n >= 1
	const long long lo = (long long)(u32)sorted[b + (n & 1 ? n / 2 : n / 2 - 1)], hi = (long long)(u32)sorted[b + n / 2];
	const long long t = 5 * (lo + hi) / 8;
	covThr[c] = (i32)(t > 10 ? t : 10);
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_uni_thresh(u32 nWin, const u32* __restrict__ winBase, u32 nC, const i32* __restrict__ covThr, const u32* __restrict__ cnt,
			 const u32* __restrict__ listOff, const u64* __restrict__ sortedBits, u64 one, u64* __restrict__ thr)
{
	const u32 w = blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (w >= nWin) return;
	const u32 T = (u32)covThr[cc_find(winBase, nC, w)];
	thr[w] = cnt[w] > T ? sortedBits[(u64)listOff[w] + T] : one;
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_uni_keep(u32 nAln, const UniAln* __restrict__ alns, const u64* __restrict__ errBits, const u64* __restrict__ thr,
		   unsigned char* __restrict__ keep)
{
	const u32 a = blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (a >= nAln) return;
	const UniAln al = alns[a];
	const u64 e = errBits[a];
	i32 good = 0;
	for (u32 j = 0; j < al.nW; ++j) good += e <= thr[al.w0 + j] ? 1 : 0;
	// Python's floor division: a negative total (trg_end before trg_start) makes total // 2 negative, and 0 > that
	keep[a] = al.total < 0 || good > al.total / 2;
}

// ---- fg_contig_consensus ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BUB_BLOCK)
k_cc_count(const BubAln* __restrict__ alns, u32 nAln, const unsigned char* __restrict__ trg, const unsigned char* __restrict__ qry,
		   u32* __restrict__ nIns)
{
	const int lane = threadIdx.x & 63;
	const u32 a = blockIdx.x * BUB_WAVES + (threadIdx.x >> 6);
	if (a >= nAln) return;
	const BubAln al = alns[a];
	u32 cnt = 0;
	if (al.inProfile)
	{
		const unsigned char* t = trg + al.colOff;
		const unsigned char* q = qry + al.colOff;
		for (long long c0 = 0; c0 < (long long)al.nCols; c0 += 64)
		{
			const long long i = c0 + lane;
			cnt += (u32)__popcll(__ballot(i < (long long)al.nCols && t[i] == '-' && q[i] != '-'));
		}
	}
	if (lane == 0) nIns[a] = cnt;
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_cc_profile(const BubAln* __restrict__ alns, u32 nAln, const CcContig* __restrict__ contigs, const unsigned char* __restrict__ trg,
			 const unsigned char* __restrict__ qry, const u32* __restrict__ qid, const u32* __restrict__ recOff,
			 const unsigned char* __restrict__ rank, u32 nB, u32* matches, unsigned long long* tag, u64* __restrict__ keys,
			 u64* __restrict__ vals)
{
	const int lane = threadIdx.x & 63;
	const u32 a = blockIdx.x * BUB_WAVES + (threadIdx.x >> 6);
	if (a >= nAln) return;
	const BubAln al = alns[a];
	if (!al.inProfile) return;
	const CcContig ct = contigs[al.contig];
	const long long n = al.nCols, len = ct.len;
	const unsigned char* t = trg + al.colOff;
	const unsigned char* q = qry + al.colOff;
	const u64 below = bub_below(lane);
	const u64 read = qid[a];
	long long base = 0;
	u32 slot = recOff[a];
	for (long long c0 = 0; c0 < n; c0 += 64)
	{
		const long long i = c0 + lane;
		const bool valid = i < n;
		const unsigned char tb = valid ? t[i] : (unsigned char)'-', qb = valid ? q[i] : (unsigned char)'-';
		const bool ng = valid && tb != '-';
		const bool isIns = valid && tb == '-' && qb != '-';
		const u64 m = __ballot(ng), mi = __ballot(isIns);
		const long long c = base + __popcll(m & below);
		// a target gap stands at the position before it; index -1 is Python's last element
		long long pos = ng ? al.trgStart + c : al.trgStart + c - 1;
		if (pos >= len) pos -= len;
		if (pos < 0) pos = len - 1;
		if (valid && pos >= 0 && pos < len)
		{
			const u64 at = ct.posOff + (u64)pos;
			if (isIns)
			{
				const u32 sl = slot + (u32)__popcll(mi & below);
				keys[sl] = (at << 32) | read;
				vals[sl] = qb;
			}
			else
			{
				atomicAdd(&matches[at * nB + rank[qb & 127]], 1u);
				atomicMax(&tag[at], ((unsigned long long)(a + 1u) << 40) | ((unsigned long long)i << 8) | tb);
			}
		}
		base += __popcll(m);
		slot += (u32)__popcll(mi);
	}
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_cc_heads(u32 nRec, const u64* __restrict__ keys, u32* __restrict__ posStart, u32* __restrict__ posEnd, u32* __restrict__ list, u32* nList)
{
	const u32 i = blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (i >= nRec) return;
	const u32 pos = (u32)(keys[i] >> 32);
	if (i == 0 || (u32)(keys[i - 1] >> 32) != pos)
	{
		posStart[pos] = i;
		list[atomicAdd(nList, 1u)] = pos;
	}
	if (i + 1 == nRec || (u32)(keys[i + 1] >> 32) != pos) posEnd[pos] = i + 1;
}

// string x before string y in Python's order of byte strings (a proper prefix first); the bytes are the low bytes of vals
__device__ __forceinline__ bool cc_less(const u64* __restrict__ vals, u32 xs, u32 xl, u32 ys, u32 yl)
{
	const u32 l = xl < yl ? xl : yl;
	for (u32 k = 0; k < l; ++k)
	{
		const u32 bx = (u32)vals[xs + k], by = (u32)vals[ys + k];
		if (bx != by) return bx < by;
	}
	return xl < yl;
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_cc_vote(u32 nList, const u32* __restrict__ list, const u32* __restrict__ posStart, const u32* __restrict__ posEnd,
		  const u64* __restrict__ keys, const u64* __restrict__ vals, u32* strStart, i32* __restrict__ numIns, u32* __restrict__ insStart,
		  u32* __restrict__ insLen)
{
	const int lane = threadIdx.x & 63;
	const u32 w = blockIdx.x * BUB_WAVES + (threadIdx.x >> 6);
	if (w >= nList) return;
	const u32 pos = list[w];
	const u32 s = posStart[pos], e = posEnd[pos];
	const u64 below = bub_below(lane);
	// the strings: maximal runs of one read; string j starts at strStart[s + j]
	u32 R = 0;
	for (u32 i0 = s; i0 < e; i0 += 64)
	{
		const u32 i = i0 + lane;
		const bool head = i < e && (i == s || keys[i] != keys[i - 1]);
		const u64 m = __ballot(head);
		if (head) strStart[s + R + (u32)__popcll(m & below)] = i;
		R += (u32)__popcll(m);
	}
	bub_fence();
	u32 bestCnt = 0, bestS = 0, bestL = 0;
	for (u32 j = lane; j < R; j += 64)
	{
		const u32 js = strStart[s + j], jl = (j + 1 < R ? strStart[s + j + 1] : e) - js;
		u32 cnt = 0;
		for (u32 k = 0; k < R; ++k)
		{
			const u32 ks = strStart[s + k], kl = (k + 1 < R ? strStart[s + k + 1] : e) - ks;
			if (kl != jl) continue;
			bool eq = true;
			for (u32 b = 0; eq && b < jl; ++b) eq = (u32)vals[js + b] == (u32)vals[ks + b];
			cnt += eq ? 1u : 0u;
		}
		if (cnt > bestCnt || (cnt == bestCnt && cc_less(vals, js, jl, bestS, bestL))) { bestCnt = cnt; bestS = js; bestL = jl; }
	}
	for (int sh = 32; sh > 0; sh >>= 1)
	{
		const u32 oc = __shfl_xor(bestCnt, sh), os = __shfl_xor(bestS, sh), ol = __shfl_xor(bestL, sh);
		if (oc > bestCnt || (oc == bestCnt && oc > 0 && cc_less(vals, os, ol, bestS, bestL))) { bestCnt = oc; bestS = os; bestL = ol; }
	}
	if (lane == 0) { numIns[pos] = (i32)R; insStart[pos] = bestS; insLen[pos] = bestL; }
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_cc_flatten(u32 nPos, const u32* __restrict__ matches, u32 nB, const unsigned char* __restrict__ byteOf, const unsigned long long* __restrict__ tag,
			 const i32* __restrict__ numIns, const u32* __restrict__ insLen, unsigned char* __restrict__ nucl, i32* __restrict__ matchTotal,
			 unsigned char* __restrict__ maxMatch, unsigned char* __restrict__ accepted, u32* __restrict__ outLen)
{
	const u32 g = blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (g > nPos) return;
	if (g == nPos) { outLen[g] = 0; return; }
	const u32* row = matches + (u64)g * nB;
	u32 total = 0, top = 0, topRank = 0;
	for (u32 r = 0; r < nB; ++r)
	{
		const u32 v = row[r];
		total += v;
		if (v > top) { top = v; topRank = r; }		// ranks are in byte order: the first of the largest is the smallest byte
	}
	const unsigned long long tg = tag[g];
	const unsigned char nu = tg ? (unsigned char)(tg & 0xffu) : (unsigned char)'-';
	const unsigned char mm = total ? byteOf[topRank] : nu;
	const i32 ni = numIns[g];
	const bool acc = ni > 0 && (u32)ni > total / 2;
	nucl[g] = nu; matchTotal[g] = (i32)total; maxMatch[g] = mm; accepted[g] = acc;
	outLen[g] = (mm != '-' ? 1u : 0u) + (acc ? insLen[g] : 0u);
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_cc_write(u32 nPos, const u32* __restrict__ outOff, const unsigned char* __restrict__ maxMatch, const unsigned char* __restrict__ accepted,
		   const u32* __restrict__ insStart, const u32* __restrict__ insLen, const u64* __restrict__ vals, unsigned char* __restrict__ seq)
{
	const u32 g = blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (g >= nPos) return;
	u32 at = outOff[g];
	if (maxMatch[g] != '-') seq[at++] = maxMatch[g];
	if (accepted[g])
	{
		const u32 s = insStart[g], l = insLen[g];
		for (u32 k = 0; k < l; ++k) seq[at + k] = (unsigned char)vals[s + k];
	}
}

// the chosen insertion string of every position, accepted or not (want_profile)
__global__ void __launch_bounds__(BUB_BLOCK)
k_cc_inswrite(u32 nPos, const u32* __restrict__ insOff, const u32* __restrict__ insStart, const u32* __restrict__ insLen,
			  const u64* __restrict__ vals, unsigned char* __restrict__ ins)
{
	const u32 g = blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (g >= nPos) return;
	const u32 at = insOff[g], s = insStart[g], l = insLen[g];
	for (u32 k = 0; k < l; ++k) ins[at + k] = (unsigned char)vals[s + k];
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_cc_pick(u32 n, const u64* __restrict__ at, const u32* __restrict__ off, u32* __restrict__ out)
{
	const u32 i = blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (i < n) out[i] = off[at[i]];
}

// present[0 .. 4) |= the set of bytes (below 128) among the query columns of the alignments with inProfile set: bit b of
// the 128 stands for byte b.  One wave per alignment.  A lane takes whole 8-byte words where the address allows (the
// alignment's first bytes up to the next word boundary and its last bytes go one per lane), ORs into four registers, the
// wave folds them by a butterfly and lane 0 issues one atomic per word that has a bit.
__global__ void __launch_bounds__(BUB_BLOCK)
k_col_present(const BubAln* __restrict__ alns, u32 nAln, const unsigned char* __restrict__ qry, u32* present)
{
	const int lane = threadIdx.x & 63;
	const u32 a = blockIdx.x * BUB_WAVES + (threadIdx.x >> 6);
	if (a >= nAln) return;
	const BubAln al = alns[a];
	if (!al.inProfile) return;
	const unsigned char* q = qry + al.colOff;
	const u64 n = al.nCols;
	u32 m[4] = {0u, 0u, 0u, 0u};
	const auto mark = [&m](u32 b)
	{
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

struct UniformOwner {
	std::vector<uint8_t> keep;
	std::vector<int32_t> covThr;
	std::vector<uint64_t> wndOff;
	std::vector<double> wndThr;
};

struct ConsensusOwner {
	std::vector<uint64_t> seqOff, profOff, insOff;
	std::vector<uint8_t> seq, nucl, maxMatch, accepted, ins;
	std::vector<int32_t> matchTotal, numIns;
};

inline u64 bitsOf(double x) { u64 b; memcpy(&b, &x, 8); return b; }
inline int bitsFor(u64 n) { int b = 1; while (b < 64 && (1ULL << b) < n) ++b; return b; }

void uniSubBatch(fg_ctx* c, u32 c0, u32 c1, const int32_t* contigLen, const uint64_t* contigAlnOff, const int32_t* trgStart,
				 const int32_t* trgEnd, const double* errRate, const uint8_t* isSecondary, u64 aln00, bool wantThr, UniformOwner& own)
{
	hipStream_t s = c->stream;
	const u32 nC = c1 - c0;
	const u64 a0 = contigAlnOff[c0], a1 = contigAlnOff[c1];
	const u32 nAln = (u32)(a1 - a0);
	std::vector<u32> winBase((size_t)nC + 1, 0), pairOff((size_t)nAln + 1, 0);
	std::vector<UniAln> alns(nAln);
	std::vector<u64> errBits(nAln);
	u64 nPairs = 0;
	for (u32 i = 0; i < nC; ++i)
	{
		winBase[i + 1] = winBase[i] + (u32)(contigLen[c0 + i] / 100 + 1);
		for (u64 a = contigAlnOff[c0 + i]; a < contigAlnOff[c0 + i + 1]; ++a)
		{
			UniAln& al = alns[a - a0];
			const i32 first = trgStart[a] / 100, last = trgEnd[a] / 100;
			al.w0 = winBase[i] + (u32)first; al.total = last - first; al.nW = last > first ? (u32)(last - first) : 0u;
			al.primary = isSecondary && isSecondary[a] ? 0u : 1u;
			errBits[a - a0] = errRate[a] == 0.0 ? 0ULL : bitsOf(errRate[a]);		// -0.0 orders as 0.0
			pairOff[a - a0] = (u32)nPairs;
			nPairs += al.nW;
		}
	}
	pairOff[nAln] = (u32)nPairs;
	const u32 nWin = winBase[nC];

	DevPool B{c->dCc, "fg_contigcons"};
	UniAln* dAln = B.get<UniAln>(nAln);
	u32* dPairOff = B.get<u32>((size_t)nAln + 1);
	u64* dErr = B.get<u64>(nAln);
	u32* dWinBase = B.get<u32>((size_t)nC + 1);
	u32* dDiff = B.get<u32>(2 * ((size_t)nWin + 1));		// all, primary: differences, then counts
	u32* dListOff = B.get<u32>((size_t)nWin + 1);
	const u64 nSort = std::max<u64>(nPairs, nWin);
	u64* dK0 = B.get<u64>(nSort);
	u64* dV0 = B.get<u64>(nSort);
	u64* dK1 = B.get<u64>(nSort);
	u64* dV1 = B.get<u64>(nSort);
	u64* dBits = B.get<u64>(nPairs);						// the windows' lists, ascending
	char* dSortScratch = B.get<char>(fgprim::radixSortScratchBytes(nSort));
	u32* dScan = B.get<u32>(fgprim::scanScratchElems((u64)nWin + 1) + 8);
	i32* dCovThr = B.get<i32>(nC);
	u64* dThr = B.get<u64>(nWin);
	unsigned char* dKeep = B.get<unsigned char>(nAln);
	u32 *dAll = dDiff, *dPrim = dDiff + nWin + 1;

	HIP_CHECK(hipMemcpyAsync(dAln, alns.data(), (size_t)nAln * sizeof(UniAln), hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dPairOff, pairOff.data(), ((size_t)nAln + 1) * 4, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dErr, errBits.data(), (size_t)nAln * 8, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dWinBase, winBase.data(), ((size_t)nC + 1) * 4, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemsetAsync(dDiff, 0, 2 * ((size_t)nWin + 1) * 4, s));
	if (nPairs)
	{
		ScopedK t(c->timer, "k_uni_emit");
		hipLaunchKernelGGL(k_uni_emit, bubGrid(nPairs), BUB_BLOCK, 0, s, nPairs, dAln, dPairOff, nAln, dErr, dK0, dV0, dAll, dPrim);
	}
	{
		ScopedK t(c->timer, "k_uni_scan");
		fgprim::scan<u32>(s, dAll, dAll, (u64)nWin + 1, true, dScan);
		fgprim::scan<u32>(s, dPrim, dPrim, (u64)nWin + 1, true, dScan);
		fgprim::scan<u32>(s, dAll, dListOff, (u64)nWin + 1, false, dScan);
	}
	if (nPairs)
	{
		ScopedK t(c->timer, "k_uni_sort");
		// by the bits, then (keys and values change places) by the window: both stable
		const int w1 = fgprim::radixSortPairs(s, dK0, dV0, dK1, dV1, nPairs, 0, 64, dSortScratch);
		u64 *bits = w1 ? dK1 : dK0, *wins = w1 ? dV1 : dV0, *bitsAlt = w1 ? dK0 : dK1, *winsAlt = w1 ? dV0 : dV1;
		const int w2 = fgprim::radixSortPairs(s, wins, bits, winsAlt, bitsAlt, nPairs, 0, bitsFor(nWin), dSortScratch);
		HIP_CHECK(hipMemcpyAsync(dBits, w2 ? bitsAlt : bits, nPairs * 8, hipMemcpyDeviceToDevice, s));
	}
	{
		ScopedK t(c->timer, "k_uni_median");
		hipLaunchKernelGGL(k_uni_medkeys, bubGrid(nWin), BUB_BLOCK, 0, s, nWin, dWinBase, nC, dPrim, dK0, dV0);
		const int w3 = fgprim::radixSortPairs(s, dK0, dV0, dK1, dV1, nWin, 0, 32 + bitsFor(nC), dSortScratch);
		hipLaunchKernelGGL(k_uni_median, bubGrid(nC), BUB_BLOCK, 0, s, nC, dWinBase, w3 ? dK1 : dK0, dCovThr);
	}
	{
		ScopedK t(c->timer, "k_uni_thresh");
		hipLaunchKernelGGL(k_uni_thresh, bubGrid(nWin), BUB_BLOCK, 0, s, nWin, dWinBase, nC, dCovThr, dAll, dListOff, dBits, bitsOf(1.0), dThr);
	}
	if (nAln)
	{
		ScopedK t(c->timer, "k_uni_keep");
		hipLaunchKernelGGL(k_uni_keep, bubGrid(nAln), BUB_BLOCK, 0, s, nAln, dAln, dErr, dThr, dKeep);
	}
	HIP_CHECK(hipGetLastError());
	const size_t cAt = own.covThr.size();
	own.covThr.resize(cAt + nC);
	HIP_CHECK(hipMemcpyAsync(own.covThr.data() + cAt, dCovThr, (size_t)nC * 4, hipMemcpyDeviceToHost, s));
	if (nAln) HIP_CHECK(hipMemcpyAsync(own.keep.data() + (a0 - aln00), dKeep, nAln, hipMemcpyDeviceToHost, s));
	if (wantThr)
	{
		const size_t wAt = own.wndThr.size();
		own.wndThr.resize(wAt + nWin);
		HIP_CHECK(hipMemcpyAsync(own.wndThr.data() + wAt, dThr, (size_t)nWin * 8, hipMemcpyDeviceToHost, s));
		for (u32 i = 0; i < nC; ++i) own.wndOff.push_back(wAt + winBase[i + 1]);
	}
	HIP_CHECK(hipStreamSynchronize(s));
}

void ccSubBatch(fg_ctx* c, u32 c0, u32 c1, const int32_t* contigLen, const uint64_t* contigAlnOff, const int32_t* trgStart,
				const int32_t* qryId, const uint8_t* use, const uint64_t* colOff, const uint8_t* trgCols, const uint8_t* qryCols,
				bool wantProfile, ConsensusOwner& own, const CigSource* cig = nullptr /* the columns are expanded here, not read from the host */)
{
	hipStream_t s = c->stream;
	const u32 nC = c1 - c0;
	const u64 a0 = contigAlnOff[c0], a1 = contigAlnOff[c1];
	const u32 nAln = (u32)(a1 - a0);
	const u64 col0 = nAln ? colOff[a0] : 0, nCols = nAln ? colOff[a1] - col0 : 0;

	std::vector<CcContig> ctg(nC);
	std::vector<BubAln> alns(nAln);
	std::vector<u32> qid(nAln);
	std::vector<u64> ctgAt((size_t)nC + 1);
	bool present[128] = {};
	u64 nPos = 0;
	for (u32 i = 0; i < nC; ++i)
	{
		ctg[i] = CcContig{nPos, contigLen[c0 + i], 0};
		ctgAt[i] = nPos;
		nPos += (u64)contigLen[c0 + i];
		for (u64 a = contigAlnOff[c0 + i]; a < contigAlnOff[c0 + i + 1]; ++a)
		{
			BubAln& al = alns[a - a0];
			al.colOff = colOff[a] - col0; al.nCols = (u32)(colOff[a + 1] - colOff[a]);
			al.trgStart = trgStart[a]; al.trgEnd = 0; al.contig = i; al.inProfile = !use || use[a] ? 1u : 0u; al.pad = 0;
			qid[a - a0] = (u32)qryId[a];
			if (al.inProfile && !cig)
				for (u64 k = colOff[a]; k < colOff[a + 1]; ++k) present[qryCols[k]] = true;
		}
	}
	ctgAt[nC] = nPos;
	if (nPos >= (1ULL << 31) || nAln >= (1u << 23) || nCols >= (1ULL << 31))
		throw FgError{FG_ERR_NOMEM, "fg_contig_consensus: a sub-batch of 2^31 positions or columns or 2^23 alignments; lower FG_CONSENSUS_BATCH_COLS"};
	DevPool B{c->dCc, "fg_contigcons"};
	BubAln* dAln = B.get<BubAln>(nAln);
	CcContig* dCtg = B.get<CcContig>(nC);
	u32* dQid = B.get<u32>(nAln);
	// k_cig_expand stores whole words past the last column
	unsigned char* dTrg = B.get<unsigned char>(nCols + (cig ? CIG_LANE_COLS : 0));
	unsigned char* dQry = B.get<unsigned char>(nCols + (cig ? CIG_LANE_COLS : 0));
	unsigned char* dTrgS = B.get<unsigned char>(nCols);
	unsigned char* dQryS = B.get<unsigned char>(nCols);
	unsigned char* dTab = B.get<unsigned char>(256);
	CigStaged staged;
	if (cig && nAln)
	{
		HIP_CHECK(hipMemcpyAsync(dAln, alns.data(), (size_t)nAln * sizeof(BubAln), hipMemcpyHostToDevice, s));
		DevPool CB = cigExpandSource(c, *cig, staged, a0, a1, dTrg, dQry);
		u32* dPresent = CB.get<u32>(4);
		HIP_CHECK(hipMemsetAsync(dPresent, 0, 16, s));
		{
			ScopedK t(c->timer, "k_col_present");
			hipLaunchKernelGGL(k_col_present, bubWaveGrid(nAln), BUB_BLOCK, 0, s, dAln, nAln, dQry, dPresent);
		}
		HIP_CHECK(hipGetLastError());
		u32 mask[4] = {};
		HIP_CHECK(hipMemcpyAsync(mask, dPresent, 16, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		for (int b = 0; b < 128; ++b) present[b] = (mask[b >> 5] >> (b & 31)) & 1u;
	}
	// the bytes present, ranked in byte order
	unsigned char rank[128] = {}, byteOf[128] = {};
	u32 nB = 0;
	for (int b = 0; b < 128; ++b)
		if (present[b]) { rank[b] = (unsigned char)nB; byteOf[nB++] = (unsigned char)b; }
	if (nB == 0) { byteOf[0] = '-'; nB = 1; }
	if (nPos * nB >= (1ULL << 32))
		throw FgError{FG_ERR_NOMEM, "fg_contig_consensus: the match table of a sub-batch has 2^32 cells (" + std::to_string(nB) +
										" distinct bytes); lower FG_CONSENSUS_BATCH_COLS"};

	u32* dMatches = B.get<u32>(nPos * nB);
	unsigned long long* dTag = B.get<unsigned long long>(nPos);
	u32* dRecOff = B.get<u32>((size_t)nAln + 1);
	u32* dScan = B.get<u32>(fgprim::scanScratchElems(std::max<u64>(nPos + 1, (u64)nAln + 1)) + 8);
	u32* dPos32 = B.get<u32>(5 * nPos + 1);			// first / last record, num_ins, chosen string start / length
	i32* dTotal = B.get<i32>(nPos);
	unsigned char* dBytes = B.get<unsigned char>(3 * nPos);	// nucl, max_match, accepted
	u32* dOutLen = B.get<u32>(nPos + 1);
	u32* dOutOff = B.get<u32>(nPos + 1);
	u64* dCtgAt = B.get<u64>((size_t)nC + 1);
	u32* dSeqAt = B.get<u32>((size_t)nC + 1);
	u32 *dPosStart = dPos32, *dPosEnd = dPos32 + nPos, *dInsStart = dPos32 + 3 * nPos, *dInsLen = dPos32 + 4 * nPos, *dNList = dPos32 + 5 * nPos;
	i32* dNumIns = (i32*)(dPos32 + 2 * nPos);
	unsigned char *dNucl = dBytes, *dMaxMatch = dBytes + nPos, *dAccepted = dBytes + 2 * nPos;

	if (!cig) HIP_CHECK(hipMemcpyAsync(dAln, alns.data(), (size_t)nAln * sizeof(BubAln), hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dCtg, ctg.data(), (size_t)nC * sizeof(CcContig), hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dQid, qid.data(), (size_t)nAln * 4, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dCtgAt, ctgAt.data(), ((size_t)nC + 1) * 8, hipMemcpyHostToDevice, s));
	if (nCols && !cig)
	{
		HIP_CHECK(hipMemcpyAsync(dTrg, trgCols + col0, nCols, hipMemcpyHostToDevice, s));
		HIP_CHECK(hipMemcpyAsync(dQry, qryCols + col0, nCols, hipMemcpyHostToDevice, s));
	}
	HIP_CHECK(hipMemcpyAsync(dTab, rank, 128, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dTab + 128, byteOf, 128, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemsetAsync(dMatches, 0, nPos * nB * 4 + 4, s));
	HIP_CHECK(hipMemsetAsync(dTag, 0, nPos * 8 + 8, s));
	HIP_CHECK(hipMemsetAsync(dPos32, 0, (5 * nPos + 1) * 4, s));
	HIP_CHECK(hipMemsetAsync(dRecOff, 0, ((size_t)nAln + 1) * 4, s));

	u32 nRec = 0;
	if (nAln)
	{
		{
			ScopedK t(c->timer, "k_bub_shift");
			hipLaunchKernelGGL(k_bub_shift, bubWaveGrid(nAln), BUB_BLOCK, 0, s, dAln, nAln, dTrg, dQry, dQryS);
			hipLaunchKernelGGL(k_bub_shift, bubWaveGrid(nAln), BUB_BLOCK, 0, s, dAln, nAln, dQryS, dTrg, dTrgS);
		}
		{
			ScopedK t(c->timer, "k_cc_count");
			hipLaunchKernelGGL(k_cc_count, bubWaveGrid(nAln), BUB_BLOCK, 0, s, dAln, nAln, dTrgS, dQryS, dRecOff);
		}
		{
			ScopedK t(c->timer, "k_cc_scan");
			fgprim::scan<u32>(s, dRecOff, dRecOff, (u64)nAln + 1, false, dScan);
		}
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipMemcpyAsync(&nRec, dRecOff + nAln, 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
	}
	u64* dK0 = B.get<u64>(nRec);
	u64* dV0 = B.get<u64>(nRec);
	u64* dK1 = B.get<u64>(nRec);
	u64* dV1 = B.get<u64>(nRec);
	char* dSortScratch = B.get<char>(fgprim::radixSortScratchBytes(nRec));
	u32* dList = B.get<u32>(nRec);
	u32* dStrStart = B.get<u32>(nRec);
	const u64 *dKeys = dK0, *dVals = dV0;
	u32 nList = 0;
	if (nAln)
	{
		ScopedK t(c->timer, "k_cc_profile");
		hipLaunchKernelGGL(k_cc_profile, bubWaveGrid(nAln), BUB_BLOCK, 0, s, dAln, nAln, dCtg, dTrgS, dQryS, dQid, dRecOff, dTab, nB,
						   dMatches, dTag, dK0, dV0);
	}
	if (nRec)
	{
		{
			ScopedK t(c->timer, "k_cc_sort");
			const int where = fgprim::radixSortPairs(s, dK0, dV0, dK1, dV1, nRec, 0, 32 + bitsFor(nPos), dSortScratch);
			dKeys = where ? dK1 : dK0; dVals = where ? dV1 : dV0;
		}
		{
			ScopedK t(c->timer, "k_cc_heads");
			hipLaunchKernelGGL(k_cc_heads, bubGrid(nRec), BUB_BLOCK, 0, s, nRec, dKeys, dPosStart, dPosEnd, dList, dNList);
		}
		HIP_CHECK(hipGetLastError());
		HIP_CHECK(hipMemcpyAsync(&nList, dNList, 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		ScopedK t(c->timer, "k_cc_vote");
		hipLaunchKernelGGL(k_cc_vote, bubWaveGrid(nList), BUB_BLOCK, 0, s, nList, dList, dPosStart, dPosEnd, dKeys, dVals, dStrStart, dNumIns,
						   dInsStart, dInsLen);
	}
	{
		ScopedK t(c->timer, "k_cc_flatten");
		hipLaunchKernelGGL(k_cc_flatten, bubGrid(nPos + 1), BUB_BLOCK, 0, s, (u32)nPos, dMatches, nB, dTab + 128, dTag, dNumIns, dInsLen, dNucl,
						   dTotal, dMaxMatch, dAccepted, dOutLen);
	}
	{
		ScopedK t(c->timer, "k_cc_scan");
		fgprim::scan<u32>(s, dOutLen, dOutOff, nPos + 1, false, dScan);
		hipLaunchKernelGGL(k_cc_pick, bubGrid((u64)nC + 1), BUB_BLOCK, 0, s, nC + 1, dCtgAt, dOutOff, dSeqAt);
	}
	HIP_CHECK(hipGetLastError());
	std::vector<u32> seqAt((size_t)nC + 1);
	HIP_CHECK(hipMemcpyAsync(seqAt.data(), dSeqAt, ((size_t)nC + 1) * 4, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	const u32 nSeq = seqAt[nC];
	unsigned char* dSeq = B.get<unsigned char>(nSeq);
	if (nPos)
	{
		ScopedK t(c->timer, "k_cc_write");
		hipLaunchKernelGGL(k_cc_write, bubGrid(nPos), BUB_BLOCK, 0, s, (u32)nPos, dOutOff, dMaxMatch, dAccepted, dInsStart, dInsLen, dVals, dSeq);
	}
	HIP_CHECK(hipGetLastError());
	const size_t seqBase = own.seq.size();
	own.seq.resize(seqBase + nSeq);
	if (nSeq) HIP_CHECK(hipMemcpyAsync(own.seq.data() + seqBase, dSeq, nSeq, hipMemcpyDeviceToHost, s));
	for (u32 i = 0; i < nC; ++i) own.seqOff.push_back(seqBase + seqAt[i + 1]);
	if (wantProfile)
	{
		const size_t at = own.nucl.size();
		for (u32 i = 0; i < nC; ++i) own.profOff.push_back(at + ctgAt[i + 1]);
		own.nucl.resize(at + nPos); own.maxMatch.resize(at + nPos); own.accepted.resize(at + nPos);
		own.matchTotal.resize(at + nPos); own.numIns.resize(at + nPos);
		// the output lengths are no longer needed: their buffers take the lengths and offsets of the chosen strings
		HIP_CHECK(hipMemcpyAsync(dOutLen, dInsLen, nPos * 4, hipMemcpyDeviceToDevice, s));
		HIP_CHECK(hipMemsetAsync(dOutLen + nPos, 0, 4, s));
		fgprim::scan<u32>(s, dOutLen, dOutOff, nPos + 1, false, dScan);
		std::vector<u32> insOff(nPos + 1);
		HIP_CHECK(hipMemcpyAsync(insOff.data(), dOutOff, (nPos + 1) * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		const u32 nInsBytes = insOff[nPos];
		unsigned char* dIns = B.get<unsigned char>(nInsBytes);
		if (nPos) hipLaunchKernelGGL(k_cc_inswrite, bubGrid(nPos), BUB_BLOCK, 0, s, (u32)nPos, dOutOff, dInsStart, dInsLen, dVals, dIns);
		HIP_CHECK(hipGetLastError());
		const size_t insBase = own.ins.size();
		own.ins.resize(insBase + nInsBytes);
		for (u64 p = 0; p < nPos; ++p) own.insOff.push_back(insBase + insOff[p + 1]);
		if (nPos)
		{
			HIP_CHECK(hipMemcpyAsync(own.nucl.data() + at, dNucl, nPos, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipMemcpyAsync(own.maxMatch.data() + at, dMaxMatch, nPos, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipMemcpyAsync(own.accepted.data() + at, dAccepted, nPos, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipMemcpyAsync(own.matchTotal.data() + at, dTotal, nPos * 4, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipMemcpyAsync(own.numIns.data() + at, dNumIns, nPos * 4, hipMemcpyDeviceToHost, s));
		}
		if (nInsBytes) HIP_CHECK(hipMemcpyAsync(own.ins.data() + insBase, dIns, nInsBytes, hipMemcpyDeviceToHost, s));
	}
	HIP_CHECK(hipStreamSynchronize(s));
}

// the finished owner into the caller's struct
void ccHandOver(struct fg_consensus_batch* out, ConsensusOwner* own, uint32_t n_contigs, bool wantProfile)
{
	out->n_contigs = n_contigs;
	out->seq_off = own->seqOff.data();
	out->seq = own->seq.data();
	if (wantProfile)
	{
		out->prof_off = own->profOff.data();
		out->nucl = own->nucl.data();
		out->match_total = own->matchTotal.data();
		out->num_ins = own->numIns.data();
		out->max_match = own->maxMatch.data();
		out->accepted = own->accepted.data();
		out->ins_off = own->insOff.data();
		out->ins = own->ins.data();
	}
	out->owner_ = own;
}

} // namespace

extern "C" {

int fg_uniform_alignments(fg_ctx* c, uint32_t n_contigs, const int32_t* contig_len, const uint64_t* contig_aln_off,
						  const int32_t* trg_start, const int32_t* trg_end, const double* err_rate, const uint8_t* is_secondary,
						  uint8_t want_thresholds, struct fg_uniform_result* out)
{
	return stageCall<UniformOwner>(c, out, [&](UniformOwner*& own)
	{
		const std::string name = "fg_uniform_alignments";
		if (!out) throw FgError{FG_ERR_ARG, name + ": null result"};
		stageContigTable(name, n_contigs, contig_len, contig_aln_off);
		const u64 a0 = n_contigs ? contig_aln_off[0] : 0, a1 = n_contigs ? contig_aln_off[n_contigs] : 0;
		if (a1 > a0 && (!trg_start || !trg_end || !err_rate)) throw FgError{FG_ERR_ARG, name + ": null trg_start, trg_end or err_rate"};
		std::vector<u64> cost(n_contigs, 0);
		for (u32 i = 0; i < n_contigs; ++i)
			for (u64 a = contig_aln_off[i]; a < contig_aln_off[i + 1]; ++a)
			{
				if (trg_start[a] < 0 || trg_end[a] < 0)
					throw FgError{FG_ERR_ARG, name + ": trg_start or trg_end < 0 at alignment " + std::to_string(a)};
				if (std::max(trg_start[a], trg_end[a]) / 100 > contig_len[i] / 100)
					throw FgError{FG_ERR_ARG, name + ": alignment " + std::to_string(a) + " ends beyond the last window of its contig"};
				if (!(err_rate[a] >= 0.0)) throw FgError{FG_ERR_ARG, name + ": err_rate NaN or negative at alignment " + std::to_string(a)};
				if (trg_end[a] / 100 > trg_start[a] / 100) cost[i] += (u64)(trg_end[a] / 100 - trg_start[a] / 100);
			}
		const u64 budget = std::min<u64>(stageEnvU64("FG_UNIFORM_BATCH_PAIRS", 1ULL << 26), fgprim::RS_MAX_N);
		stageAllFit(name, "contig", cost, budget, "(alignment, window) pairs", "FG_UNIFORM_BATCH_PAIRS");
		own = new UniformOwner;
		own->keep.assign((size_t)(a1 - a0), 0);
		if (want_thresholds) own->wndOff.assign(1, 0);
		HIP_CHECK(hipSetDevice(c->device));
		c->timer.reset();
		u32 i = 0;
		while (i < n_contigs)
		{
			u32 j = i;
			u64 used = 0, wins = 0, alns = 0;
			// windows and alignments of a sub-batch are numbered in 32 bits
			while (j < n_contigs && (j == i || (used + cost[j] <= budget && wins + (u64)contig_len[j] / 100 + 1 < (1ULL << 27) &&
											   alns + (contig_aln_off[j + 1] - contig_aln_off[j]) < (1ULL << 27))))
			{
				used += cost[j]; wins += (u64)contig_len[j] / 100 + 1; alns += contig_aln_off[j + 1] - contig_aln_off[j];
				++j;
			}
			if (alns >= (1ULL << 31)) throw FgError{FG_ERR_NOMEM, name + ": a contig with 2^31 alignments"};
			uniSubBatch(c, i, j, contig_len, contig_aln_off, trg_start, trg_end, err_rate, is_secondary, a0, want_thresholds != 0, *own);
			i = j;
		}
		c->timer.collect();
		stageKeep(own->keep, own->covThr, own->wndThr);
		out->n_contigs = n_contigs;
		out->n_alignments = (uint64_t)own->keep.size();
		out->keep = own->keep.data();
		out->cov_threshold = own->covThr.data();
		if (want_thresholds)
		{
			out->wnd_off = own->wndOff.data();
			out->wnd_threshold = own->wndThr.data();
		}
		out->owner_ = own;
	});
}

void fg_release_uniform(struct fg_uniform_result* r) { stageRelease<UniformOwner>(r); }

int fg_contig_consensus(fg_ctx* c, uint32_t n_contigs, const int32_t* contig_len, const uint64_t* contig_aln_off,
						const int32_t* trg_start, const int32_t* qry_id, const uint8_t* use, const uint64_t* col_off,
						const uint8_t* trg_cols, const uint8_t* qry_cols, uint8_t want_profile, struct fg_consensus_batch* out)
{
	return stageCall<ConsensusOwner>(c, out, [&](ConsensusOwner*& own)
	{
		const std::string name = "fg_contig_consensus";
		if (!out) throw FgError{FG_ERR_ARG, name + ": null result"};
		stageContigTable(name, n_contigs, contig_len, contig_aln_off);
		const u64 a0 = n_contigs ? contig_aln_off[0] : 0, a1 = n_contigs ? contig_aln_off[n_contigs] : 0;
		if (a1 > a0 && (!trg_start || !qry_id || !col_off)) throw FgError{FG_ERR_ARG, name + ": null trg_start, qry_id or col_off"};
		stageColOff(name, col_off, a0, a1, trg_cols, qry_cols);
		std::vector<u64> cost(n_contigs, 0);
		for (u32 i = 0; i < n_contigs; ++i)
		{
			for (u64 a = contig_aln_off[i]; a < contig_aln_off[i + 1]; ++a)
			{
				// the order of the reports is part of the call: the bytes of every alignment first, then, for those in use,
				// trg_start (fg_make_bubbles: trg_start first)
				const u64 nonGap = stageColumnWalk(name, a, col_off, trg_cols, qry_cols);
				if (use && !use[a]) continue;		// the positions of an alignment that takes no part are not looked at
				if (contig_len[i] == 0)
					throw FgError{FG_ERR_ARG, name + ": alignment " + std::to_string(a) + " is in use on a contig of length 0"};
				stageStartOnContig(name, a, trg_start[a], contig_len[i]);
				stageBasesOnContig(name, a, nonGap, contig_len[i]);
			}
			// a contig counts its columns and its positions
			cost[i] = (u64)contig_len[i];
			if (contig_aln_off[i + 1] > contig_aln_off[i]) cost[i] += col_off[contig_aln_off[i + 1]] - col_off[contig_aln_off[i]];
		}
		const u64 budget = stageEnvU64("FG_CONSENSUS_BATCH_COLS", 1ULL << 27);
		const u64 maxContigs = stageEnvCap("FG_CONSENSUS_BATCH_CONTIGS");		// a switch for tests: contigs per sub-batch
		stageAllFit(name, "contig", cost, budget, "columns and positions", "FG_CONSENSUS_BATCH_COLS");
		own = new ConsensusOwner;
		own->seqOff.assign(1, 0);
		if (want_profile) { own->profOff.assign(1, 0); own->insOff.assign(1, 0); }
		HIP_CHECK(hipSetDevice(c->device));
		c->timer.reset();
		for (u32 i = 0; i < n_contigs;)
		{
			const u32 j = stageCut(i, n_contigs, cost, budget, maxContigs);
			ccSubBatch(c, i, j, contig_len, contig_aln_off, trg_start, qry_id, use, col_off, trg_cols, qry_cols, want_profile != 0, *own);
			i = j;
		}
		c->timer.collect();
		stageKeep(own->seq, own->nucl, own->maxMatch, own->accepted, own->ins, own->matchTotal, own->numIns);
		ccHandOver(out, own, n_contigs, want_profile != 0);
	});
}

int fg_contig_consensus_cigars(fg_ctx* c, uint32_t n_contigs, const uint64_t* contig_off, const uint8_t* contig_seq,
							   const uint64_t* contig_aln_off, const int32_t* ctg_pos, const uint64_t* run_off, const uint8_t* run_op,
							   const uint32_t* run_len, const uint64_t* read_off, const uint8_t* read_seq, const int32_t* qry_id,
							   const uint8_t* use, uint8_t want_profile, struct fg_consensus_batch* out)
{
	return stageCall<ConsensusOwner>(c, out, [&](ConsensusOwner*& own)
	{
		const std::string name = "fg_contig_consensus_cigars";
		if (!out) throw FgError{FG_ERR_ARG, name + ": null result"};
		if (n_contigs && !contig_aln_off) throw FgError{FG_ERR_ARG, name + ": null contig_aln_off"};
		stageOffsets(name, "contig_aln_off", "contig ", contig_aln_off, 0, n_contigs);
		const u64 a0 = n_contigs ? contig_aln_off[0] : 0, a1 = n_contigs ? contig_aln_off[n_contigs] : 0;
		std::vector<uint32_t> alnContig((size_t)a1, 0);
		for (u32 i = 0; i < n_contigs; ++i)
			for (u64 a = contig_aln_off[i]; a < contig_aln_off[i + 1]; ++a) alnContig[a] = i;
		// every check of fg_expand_cigars, then those fg_contig_consensus makes on what the expansion would hand it
		CigPlan plan;
		cigCheckRecords(name, n_contigs, contig_off, contig_seq, a0, a1, alnContig.data(), !ctg_pos || !run_off || !read_off || !qry_id,
						"null ctg_pos, run_off, read_off or qry_id", ctg_pos, run_off, run_op, run_len, read_off, read_seq, plan);
		std::vector<int32_t> contigLen(n_contigs, 0);
		std::vector<u64> cost(n_contigs, 0);
		for (u32 i = 0; i < n_contigs; ++i)
		{
			if (contig_off[i + 1] - contig_off[i] > CIG_I32) throw FgError{FG_ERR_ARG, name + ": contig " + std::to_string(i) + " has 2^31 bytes"};
			contigLen[i] = (int32_t)(contig_off[i + 1] - contig_off[i]);
			for (u64 a = contig_aln_off[i]; a < contig_aln_off[i + 1]; ++a)
			{
				if (use && !use[a]) continue;		// the positions of an alignment that takes no part are not looked at
				if (contigLen[i] == 0)
					throw FgError{FG_ERR_ARG, name + ": alignment " + std::to_string(a) + " is in use on a contig of length 0"};
				// an alignment of insertions alone may stand behind the last base
				stageStartOnContig(name, a, plan.trgStart[a], contigLen[i]);
			}
			// a contig counts its columns and its positions
			cost[i] = (u64)contigLen[i] + (plan.colOff[contig_aln_off[i + 1]] - plan.colOff[contig_aln_off[i]]);
		}
		const u64 budget = stageEnvU64("FG_CONSENSUS_BATCH_COLS", 1ULL << 27);
		const u64 maxContigs = stageEnvCap("FG_CONSENSUS_BATCH_CONTIGS");		// a switch for tests: contigs per sub-batch
		stageAllFit(name, "contig", cost, budget, "columns and positions", "FG_CONSENSUS_BATCH_COLS");
		own = new ConsensusOwner;
		own->seqOff.assign(1, 0);
		if (want_profile) { own->profOff.assign(1, 0); own->insOff.assign(1, 0); }
		HIP_CHECK(hipSetDevice(c->device));
		c->timer.reset();
		// the contig bytes go up once per call; a sub-batch expands its own alignments
		const CigSource src{&plan, a1 > a0 ? cigUploadContigs(c, plan, contig_seq) : nullptr, run_off, run_op, run_len, read_off, read_seq, cigTile()};
		u32 i = 0;
		while (i < n_contigs)
		{
			const u32 j = cigCutContigs(name, "FG_CONSENSUS_BATCH_COLS", i, n_contigs, cost, budget, maxContigs, contig_aln_off, run_off, read_off);
			ccSubBatch(c, i, j, contigLen.data(), contig_aln_off, plan.trgStart.data(), qry_id, use, plan.colOff.data(), nullptr, nullptr,
					   want_profile != 0, *own, &src);
			i = j;
		}
		c->timer.collect();
		stageKeep(own->seq, own->nucl, own->maxMatch, own->accepted, own->ins, own->matchTotal, own->numIns);
		ccHandOver(out, own, n_contigs, want_profile != 0);
	});
}

void fg_release_consensus(struct fg_consensus_batch* b) { stageRelease<ConsensusOwner>(b); }

} // extern "C"
