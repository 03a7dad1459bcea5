// fg_make_bubbles: the bubble partition of the reference's polisher (flye/polishing/bubbles.py: _compute_profile with
// both shift_gaps passes of alignment.py:68-92, _get_partition, _get_bubble_seqs, _postprocess_bubbles) on the device.
// Integers only on the device: the two rate tests of _is_solid_kmer are made against a host table that holds, per
// coverage value, the largest numerator that still passes Python's double division.
//
// A sub-batch of whole contigs (FG_BUBBLE_BATCH_COLS) goes through these launches:
//   k_bub_shift     (fg_gapshift.h) one wave per profiled alignment, twice (query against target, then target against
//                   the shifted query).  The wave copies the string, finds gap runs by ballots over 64 columns, and closes them left
//                   to right: the compare of one run is parallel, a ballot finds the first mismatch, the block of m
//                   bases moves in parallel (source and destination never overlap: m <= run length).
//   k_bub_profile   one wave per profiled alignment over the shifted strings: the position of a column is trg_start +
//                   the ballot prefix count of non-gap target columns; integer atomics on the four counters and an
//                   atomic max of (alignment + 1) << 8 | byte for nucl (the last alignment in list order wins).
//   k_bub_good      one thread per position: the solid test against the table, as a 0 / 1 "bad" word.
//   (scan)          exclusive sums of the bad words; k_bub_badpos lists the bad positions.
//   k_bub_solid     one thread per position: the first loop of _get_partition in closed form.  In a maximal run of good
//                   positions [s, e] the greedy walk marks k-mers at s, s + SOLID, ... while they fit in the run and
//                   start below len - SOLID: min(floor((e - s + 1) / SOLID), floor((len - SOLID - 1 - s) / SOLID) + 1)
//                   of them (none when s >= len - SOLID).
//   k_bub_landmark  one thread per position: all(solid[p : p + SIMPLE]) and _is_simple_kmer(p + SIMPLE / 2).
//   k_bub_walk      one wave per contig: the second loop, a true chain.  The next event after prof_pos is the first
//                   landmark (64 positions per ballot) or prev_partition + max_bubble_length + 1, whichever is first.
//   k_bub_cuts      one wave per alignment (all of them, original strings), first counting, then writing branch records.
//                   A cut is a non-gap target column at position 0 or at a partition point, except the alignment's
//                   first non-gap column unless it is position 0: the reference's "trg_pos >= next_bubble_start" can
//                   only become true AT a partition point because positions rise by one.
//   (sort)          stable radix sort of (bubble, slot): slots are numbered in (alignment, cut) order.
//   k_bub_post      one wave per bubble: _postprocess_bubbles.  The median is element n / 2 of the order (length, index),
//                   found by rank counting.  incons_rate < 0.5 is 2 |d| < med: |d| / med <= 1/2 - 1/(2 med) is further
//                   from 0.5 than a double's rounding error for med < 2^31.  len > max_bubble_length * 1.5 is
//                   2 len > 3 max_bubble_length: 1.5 * an int32 is exact in double.
//   k_bub_fill      one wave per kept bubble: the consensus, the branch offsets and the branch bytes (gaps dropped by
//                   ballot compaction, to_acgt by table).
// The host does work proportional to contigs, alignments and bubbles (checks, offsets, the rate table).
//
// fg_make_bubbles_cigars takes SAM records where fg_make_bubbles takes columns: a sub-batch expands its own alignments
// (fg_cigexpand.h) on the context's stream straight into the two column buffers, so no column crosses the bus.
#include "fg_ctx.h"
#include "fg_stage.h"
#include "fg_devprim.h"
#include "fg_gapshift.h"
#include "fg_cigexpand.h"
#include <cmath>

namespace {

struct BubContig { u64 posOff; u64 partBase; u64 bubBase; i32 len; u32 circular; u32 nPart; u32 pad; };
struct BubPost { u64 keptBytes; u32 keep, nKept, consLen, medIdx, mode, consFromMed; };
struct BubOut { u64 candOff, slotBase, byteBase; };

// the segment i with off[i] <= x < off[i + 1] (off ascending, n segments; empty segments are skipped)
template <class F>
__device__ __forceinline__ u32 bub_find(u32 n, u64 x, F off)
{
	u32 lo = 0, hi = n;
	while (hi - lo > 1)
	{
		const u32 mid = (lo + hi) >> 1;
		if (off(mid) <= x) lo = mid; else hi = mid;
	}
	return lo;
}

// bisect_right(partition, p)
__device__ __forceinline__ u32 bub_bisect(const i32* __restrict__ part, u32 n, i32 p)
{
	u32 lo = 0, hi = n;
	while (lo < hi)
	{
		const u32 mid = (lo + hi) >> 1;
		if (part[mid] <= p) lo = mid + 1; else hi = mid;
	}
	return lo;
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_bub_profile(const BubAln* __restrict__ alns, u32 nAln, const BubContig* __restrict__ contigs, const unsigned char* __restrict__ trg,
			  const unsigned char* __restrict__ qry, i32* cov, i32* ins, i32* del, i32* mis, u32* tag)
{
	const int lane = threadIdx.x & 63;
	const u32 a = blockIdx.x * BUB_WAVES + (threadIdx.x >> 6);
	if (a >= nAln) return;
	const BubAln al = alns[a];
	if (!al.inProfile) return;
	const BubContig ct = contigs[al.contig];
	const long long n = al.nCols, len = ct.len;
	const unsigned char* t = trg + al.colOff;
	const unsigned char* q = qry + al.colOff;
	const u64 below = bub_below(lane);
	long long base = 0;
	for (long long c0 = 0; c0 < n; c0 += 64)
	{
		const long long i = c0 + lane;
		const bool valid = i < n;
		const unsigned char tb = valid ? t[i] : (unsigned char)'-', qb = valid ? q[i] : (unsigned char)'-';
		const bool ng = valid && tb != '-';
		const u64 m = __ballot(ng);
		const long long c = base + __popcll(m & below);
		if (ng)
		{
			long long pos = al.trgStart + c;
			if (pos >= len) pos -= len;
			if (pos >= 0 && pos < len)
			{
				const u64 at = ct.posOff + (u64)pos;
				atomicAdd(&cov[at], 1);
				if (qb == '-') atomicAdd(&del[at], 1);
				else if (qb != tb) atomicAdd(&mis[at], 1);
				atomicMax(&tag[at], ((a + 1u) << 8) | tb);
			}
		}
		else if (valid)
		{
			// an insertion counts at the position before it; index -1 is Python's last element
			long long pos = al.trgStart + c - 1;
			if (pos >= len) pos -= len;
			if (pos < 0) pos = len - 1;
			if (pos >= 0 && pos < len) atomicAdd(&ins[ct.posOff + (u64)pos], 1);
		}
		base += __popcll(m);
	}
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_bub_good(u64 nPos, const i32* __restrict__ cov, const i32* __restrict__ ins, const i32* __restrict__ del, const i32* __restrict__ mis,
		   const i32* __restrict__ tabMis, const i32* __restrict__ tabIns, u32 tabN, u32* __restrict__ bad)
{
	const u64 g = (u64)blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (g > nPos) return;
	if (g == nPos) { bad[g] = 0; return; }
	const i32 cv = cov[g];
	const bool good = cv > 0 && (u32)cv < tabN && mis[g] + del[g] <= tabMis[cv] && ins[g] <= tabIns[cv];
	bad[g] = good ? 0u : 1u;
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_bub_badpos(u64 nPos, const u32* __restrict__ bad, const u32* __restrict__ B, u32* __restrict__ badPos)
{
	const u64 g = (u64)blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (g < nPos && bad[g]) badPos[B[g]] = (u32)g;
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_bub_solid(u64 nPos, const BubContig* __restrict__ contigs, u32 nContigs, const u32* __restrict__ bad, const u32* __restrict__ B,
			const u32* __restrict__ badPos, i32 SOLID, unsigned char* __restrict__ solid)
{
	const u64 g = (u64)blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (g >= nPos) return;
	unsigned char r = 0;
	if (!bad[g])
	{
		const u32 c = bub_find(nContigs, g, [&](u32 i) { return contigs[i].posOff; });
		const BubContig ct = contigs[c];
		const u64 P0 = ct.posOff, P1 = ct.posOff + (u64)ct.len;
		const u32 k = B[g];
		const long long s = k == B[P0] ? (long long)P0 : (long long)badPos[k - 1] + 1;
		const long long e = k == B[P1] ? (long long)P1 - 1 : (long long)badPos[k] - 1;
		const long long sl = s - (long long)P0, len = ct.len;
		long long nk = (e - s + 1) / SOLID;
		if (sl > len - SOLID - 1) nk = 0;
		else
		{
			const long long byBound = (len - SOLID - 1 - sl) / SOLID + 1;
			if (byBound < nk) nk = byBound;
		}
		r = ((long long)g - s) < nk * SOLID;
	}
	solid[g] = r;
}

// has-base and byte in one word: two positions without a base compare equal, as two empty strings do
__device__ __forceinline__ u32 bub_code(u32 tag) { return tag ? (0x100u | (tag & 0xffu)) : 0u; }

__global__ void __launch_bounds__(BUB_BLOCK)
k_bub_landmark(u64 nPos, const BubContig* __restrict__ contigs, u32 nContigs, const unsigned char* __restrict__ solid,
			   const u32* __restrict__ tag, i32 SOLID, i32 SIMPLE, unsigned char* __restrict__ lm)
{
	const u64 g = (u64)blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (g >= nPos) return;
	const u32 c = bub_find(nContigs, g, [&](u32 i) { return contigs[i].posOff; });
	const BubContig ct = contigs[c];
	const long long p = (long long)(g - ct.posOff), len = ct.len;
	unsigned char r = 0;
	if (p >= SOLID && p < len - SOLID)
	{
		bool ok = true;
		for (int i = 0; i < SIMPLE; ++i) ok = ok && solid[g + i];
		if (ok)
		{
			// N[i] = nucl[p + SIMPLE / 2 - SIMPLE + i], i in [0, 2 SIMPLE)
			const u32* N = tag + (g + SIMPLE / 2 - SIMPLE);
			for (int i = SIMPLE - SIMPLE / 2; ok && i < SIMPLE + SIMPLE / 2 - 1; ++i)
				if (bub_code(N[i]) == bub_code(N[i + 1])) ok = false;
			for (int shift = 0; ok && shift < 2; ++shift)
				for (int i = 0; ok && i < SIMPLE - shift - 1; ++i)
				{
					const int q = shift + 2 * i;
					if (bub_code(N[q]) == bub_code(N[q + 2]) && bub_code(N[q + 1]) == bub_code(N[q + 3])) ok = false;
				}
		}
		r = ok;
	}
	lm[g] = r;
}

__global__ void __launch_bounds__(64)
k_bub_walk(BubContig* contigs, const unsigned char* __restrict__ lm, unsigned char* __restrict__ isPart, i32* __restrict__ partition,
		   i32* __restrict__ nLong, i32 SOLID, i32 SIMPLE, i32 MAXB)
{
	const int lane = threadIdx.x;
	const BubContig ct = contigs[blockIdx.x];
	const long long end = (long long)ct.len - SOLID;
	long long pos = SOLID, prev = SOLID;
	u32 cnt = 0;
	i32 lg = 0;
	while (pos < end)
	{
		const long long reach = prev + (long long)MAXB + 1;
		const long long forcedAt = pos > reach ? pos : reach;
		const long long lim = forcedAt < end ? forcedAt : end;
		long long q = -1;
		for (long long s = pos; s < lim; s += 64)
		{
			const long long i = s + lane;
			const u64 m = __ballot(i < lim && lm[ct.posOff + (u64)i]);
			if (m) { q = s + (__ffsll((unsigned long long)m) - 1); break; }
		}
		if (q < 0)
		{
			if (forcedAt >= end) break;
			q = forcedAt;
		}
		if (q - prev > MAXB) ++lg;
		const long long cur = q + SIMPLE / 2;
		if (lane == 0)
		{
			partition[ct.partBase + cnt] = (i32)cur;
			isPart[ct.posOff + (u64)cur] = 1;
		}
		++cnt;
		prev = cur;
		pos = q + SOLID;
	}
	if (lane == 0)
	{
		contigs[blockIdx.x].nPart = cnt;
		nLong[blockIdx.x] = lg;
	}
}

// COUNT: nEmit[a] = branches the alignment gives.  Otherwise: their records, slot = slotBase[a] + order of emission.
template <bool COUNT>
__global__ void __launch_bounds__(BUB_BLOCK)
k_bub_cuts(const BubAln* __restrict__ alns, u32 nAln, const BubContig* __restrict__ contigs, const unsigned char* __restrict__ trg,
		   const unsigned char* __restrict__ qry, const unsigned char* __restrict__ isPart, const i32* __restrict__ partition,
		   u32* __restrict__ nEmit, const u32* __restrict__ slotBase, u64* __restrict__ keys, u64* __restrict__ vals,
		   u64* __restrict__ segCol, u32* __restrict__ segCols, u32* __restrict__ segLen, u32* __restrict__ rawCnt)
{
	const int lane = threadIdx.x & 63;
	const u32 a = blockIdx.x * BUB_WAVES + (threadIdx.x >> 6);
	if (a >= nAln) return;
	const BubAln al = alns[a];
	const BubContig ct = contigs[al.contig];
	if (ct.nPart == 0) { if (COUNT && lane == 0) nEmit[a] = 0; return; }
	const i32* part = partition + ct.partBase;
	const long long n = al.nCols, len = ct.len;
	const unsigned char* t = trg + al.colOff;
	const unsigned char* q = qry + al.colOff;
	const u64 below = bub_below(lane);
	const bool linear = !ct.circular;
	u32 curBub = bub_bisect(part, ct.nPart, al.trgStart);
	const bool chromStart = curBub == 0 && linear;
	const bool chromEnd = al.trgEnd > part[ct.nPart - 1] && linear;
	const u32 sb = COUNT ? 0u : slotBase[a];
	long long base = 0, qbase = 0, lastCutCol = 0, lastCutQ = 0;
	u32 nCuts = 0;
	for (long long c0 = 0; c0 < n; c0 += 64)
	{
		const long long i = c0 + lane;
		const bool valid = i < n;
		const bool ng = valid && t[i] != '-';
		const bool qn = valid && q[i] != '-';
		const u64 mT = __ballot(ng), mQ = __ballot(qn);
		const long long j = base + __popcll(mT & below);
		long long p = al.trgStart + j;
		if (p >= len) p -= len;
		const bool inRange = p >= 0 && p < len;
		const bool isCut = ng && inRange && (p == 0 || (j > 0 && isPart[ct.posOff + (u64)p]));
		const u64 mC = __ballot(isCut);
		if (!COUNT && mC)
		{
			const long long qAt = qbase + __popcll(mQ & below);
			const u32 bubAfter = isCut ? bub_bisect(part, ct.nPart, (i32)p) : 0u;
			const u64 before = mC & below;
			const int pl = before ? 63 - __clzll((long long)before) : 0;
			const long long pQ = __shfl(qAt, pl);
			const u32 pB = __shfl(bubAfter, pl);
			const long long prevCol = before ? c0 + pl : lastCutCol;
			const long long prevQ = before ? pQ : lastCutQ;
			const u32 prevBub = before ? pB : curBub;
			const u32 tIdx = nCuts + (u32)__popcll(before);
			if (isCut && (tIdx > 0 || chromStart))
			{
				const u32 slot = sb + (chromStart ? tIdx : tIdx - 1);
				const u64 bub = ct.bubBase + prevBub;
				keys[slot] = bub;
				vals[slot] = slot;
				segCol[slot] = al.colOff + (u64)prevCol;
				segCols[slot] = (u32)(i - prevCol);
				segLen[slot] = (u32)(qAt - prevQ);
				atomicAdd(&rawCnt[bub], 1u);
			}
			const int hl = 63 - __clzll((long long)mC);
			lastCutCol = c0 + hl;
			lastCutQ = __shfl(qAt, hl);
			curBub = __shfl(bubAfter, hl);
		}
		nCuts += (u32)__popcll(mC);
		base += __popcll(mT);
		qbase += __popcll(mQ);
	}
	const u32 atCuts = nCuts ? (chromStart ? nCuts : nCuts - 1) : 0u;
	if (COUNT) { if (lane == 0) nEmit[a] = atCuts + (chromEnd ? 1u : 0u); return; }
	if (chromEnd && lane == 0)
	{
		// qry[branch_start:] to the LAST bubble; branch_start is None (the whole string) without a cut
		const u32 slot = sb + atCuts;
		const u64 bub = ct.bubBase + ct.nPart;
		keys[slot] = bub;
		vals[slot] = slot;
		segCol[slot] = al.colOff + (u64)lastCutCol;
		segCols[slot] = (u32)(n - lastCutCol);
		segLen[slot] = (u32)(qbase - lastCutQ);
		atomicAdd(&rawCnt[bub], 1u);
	}
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_bub_gather(u64 nSlots, const u64* __restrict__ vals, const u32* __restrict__ segLen, u32* __restrict__ sortedLen)
{
	const u64 g = (u64)blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (g < nSlots) sortedLen[g] = segLen[vals[g]];
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_bub_post(u32 nBub, const BubContig* __restrict__ contigs, u32 nContigs, const i32* __restrict__ partition, const u32* __restrict__ tag,
		   const u32* __restrict__ rawOff, const u32* __restrict__ sortedLen, i32 MAXB, i32 MAXBR, unsigned char* __restrict__ keptFlag,
		   BubPost* __restrict__ post, i32* __restrict__ nEmpty, i32* __restrict__ nLongBranch)
{
	const int lane = threadIdx.x & 63;
	const u32 b = blockIdx.x * BUB_WAVES + (threadIdx.x >> 6);
	if (b >= nBub) return;
	const u32 c = bub_find(nContigs, b, [&](u32 i) { return contigs[i].bubBase; });
	const BubContig ct = contigs[c];
	const u32 k = b - (u32)ct.bubBase;
	const u32 r0 = rawOff[b], n = rawOff[b + 1] - r0;
	const u32* L = sortedLen + r0;
	unsigned char* kf = keptFlag + r0;
	BubPost o;
	o.keptBytes = 0; o.keep = 0; o.nKept = 0; o.consLen = 0; o.medIdx = 0; o.mode = 0; o.consFromMed = 0;
	if (n == 0)
	{
		if (lane == 0) { atomicAdd(&nEmpty[c], 1); post[b] = o; }
		return;
	}
	// element n / 2 of the stable sort by length
	u32 medIdx = 0xffffffffu;
	for (u32 i0 = 0; i0 < n; i0 += 64)
	{
		const u32 i = i0 + lane;
		const u32 li = i < n ? L[i] : 0u;
		u32 rank = 0;
		for (u32 j = 0; j < n; ++j)
		{
			const u32 lj = L[j];
			rank += (lj < li || (lj == li && j < i)) ? 1u : 0u;
		}
		const u64 hit = __ballot(i < n && rank == n / 2);
		if (hit) { medIdx = i0 + (u32)(__ffsll((unsigned long long)hit) - 1); break; }
	}
	const long long med = L[medIdx];
	if (med == 0) { if (lane == 0) post[b] = o; return; }
	o.keep = 1; o.medIdx = medIdx;
	const u64 below = bub_below(lane);
	if (2 * med > 3 * (long long)MAXB)
	{
		o.mode = 1; o.nKept = 1; o.keptBytes = (u64)med;
		for (u32 i = lane; i < n; i += 64) kf[i] = i == medIdx;
		if (lane == 0) atomicAdd(&nLongBranch[c], 1);
	}
	else
	{
		u32 run = 0;
		u64 bytes = 0;
		for (u32 i0 = 0; i0 < n; i0 += 64)
		{
			const u32 i = i0 + lane;
			const long long li = i < n ? (long long)L[i] : 0;
			const long long d = li > med ? li - med : med - li;
			const bool cons = i < n && 2 * d < med;
			const u64 m = __ballot(cons);
			const bool kept = cons && run + (u32)__popcll(m & below) < (u32)MAXBR;
			if (i < n) kf[i] = kept;
			u64 mine = kept ? (u64)(li == 0 ? 1 : li) : 0ULL;
			for (int s = 32; s > 0; s >>= 1)
			{
				const u32 lo = __shfl_xor((u32)mine, s), hi = __shfl_xor((u32)(mine >> 32), s);
				mine += ((u64)hi << 32) | lo;
			}
			bytes += mine;
			run += (u32)__popcll(m);
		}
		o.nKept = run < (u32)MAXBR ? run : (u32)MAXBR;
		o.keptBytes = bytes;
	}
	// the consensus: the bases of the span
	const long long pl = k == 0 ? 0 : partition[ct.partBase + k - 1];
	const long long pr = k == ct.nPart ? (long long)ct.len : partition[ct.partBase + k];
	u32 cl = 0;
	for (long long p0 = pl; p0 < pr; p0 += 64)
	{
		const long long p = p0 + lane;
		cl += (u32)__popcll(__ballot(p < pr && tag[ct.posOff + (u64)p] != 0));
	}
	const long long dc = med > (long long)cl ? med - cl : (long long)cl - med;
	if (dc > med / 2) { o.consFromMed = 1; o.consLen = (u32)med; } else o.consLen = cl;
	if (lane == 0) post[b] = o;
}

// the non-gap bytes of src[0 .. nCols) through the table to dst; returns their number
__device__ __forceinline__ u32 bub_degap(const unsigned char* __restrict__ src, u32 nCols, unsigned char* __restrict__ dst,
										 const unsigned char* __restrict__ tab, int lane, u64 below)
{
	u32 w = 0;
	for (u32 c0 = 0; c0 < nCols; c0 += 64)
	{
		const u32 i = c0 + lane;
		const unsigned char ch = i < nCols ? src[i] : (unsigned char)'-';
		const bool keep = i < nCols && ch != '-';
		const u64 m = __ballot(keep);
		if (keep) dst[w + (u32)__popcll(m & below)] = tab[ch & 127];
		w += (u32)__popcll(m);
	}
	return w;
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_bub_fill(u32 nBub, const BubContig* __restrict__ contigs, u32 nContigs, const i32* __restrict__ partition, const u32* __restrict__ tag,
		   const u32* __restrict__ rawOff, const u64* __restrict__ vals, const u64* __restrict__ segCol, const u32* __restrict__ segCols,
		   const u32* __restrict__ sortedLen, const unsigned char* __restrict__ keptFlag, const BubPost* __restrict__ post,
		   const BubOut* __restrict__ outs, const unsigned char* __restrict__ qry, const unsigned char* __restrict__ tab,
		   unsigned char* __restrict__ cand, u64 candBase, unsigned char* __restrict__ brBytes, u64 byteBase0, u64* __restrict__ brOff,
		   u64 slotBase0)
{
	const int lane = threadIdx.x & 63;
	const u32 b = blockIdx.x * BUB_WAVES + (threadIdx.x >> 6);
	if (b >= nBub) return;
	const BubPost po = post[b];
	if (!po.keep) return;
	const BubOut ou = outs[b];
	const u32 c = bub_find(nContigs, b, [&](u32 i) { return contigs[i].bubBase; });
	const BubContig ct = contigs[c];
	const u32 k = b - (u32)ct.bubBase;
	const u32 r0 = rawOff[b], n = rawOff[b + 1] - r0;
	const u64 below = bub_below(lane);
	unsigned char* cd = cand + (ou.candOff - candBase);
	if (po.consFromMed)
	{
		const u64 slot = vals[r0 + po.medIdx];
		(void)bub_degap(qry + segCol[slot], segCols[slot], cd, tab, lane, below);
	}
	else
	{
		const long long pl = k == 0 ? 0 : partition[ct.partBase + k - 1];
		const long long pr = k == ct.nPart ? (long long)ct.len : partition[ct.partBase + k];
		u32 w = 0;
		for (long long p0 = pl; p0 < pr; p0 += 64)
		{
			const long long p = p0 + lane;
			const u32 tg = p < pr ? tag[ct.posOff + (u64)p] : 0u;
			const u64 m = __ballot(tg != 0);
			if (tg) cd[w + (u32)__popcll(m & below)] = (unsigned char)(tg & 0xffu);
			w += (u32)__popcll(m);
		}
	}
	u64 at = ou.byteBase;
	u32 r = 0;
	for (u32 i = 0; i < n; ++i)
	{
		if (!keptFlag[r0 + i]) continue;
		const u64 slot = vals[r0 + i];
		const u32 len = sortedLen[r0 + i];
		if (lane == 0) brOff[ou.slotBase - slotBase0 + r] = at;
		unsigned char* dst = brBytes + (at - byteBase0);
		if (len == 0) { if (lane == 0) dst[0] = 'A'; at += 1; }
		else { (void)bub_degap(qry + segCol[slot], segCols[slot], dst, tab, lane, below); at += len; }
		++r;
	}
}

__global__ void __launch_bounds__(BUB_BLOCK)
k_bub_nucl(u64 nPos, const u32* __restrict__ tag, unsigned char* __restrict__ nucl)
{
	const u64 g = (u64)blockIdx.x * BUB_BLOCK + threadIdx.x;
	if (g < nPos) nucl[g] = (unsigned char)(tag[g] & 0xffu);
}

struct BubbleOwner {
	std::vector<uint64_t> bubbleOff, candOff, branchOff, bubbleBranchOff, partOff, profOff;
	std::vector<int32_t> position, nLongBubbles, nEmpty, nLongBranch, nPartition, partition, coverage, numInserts, numDeletions,
		numMissmatch;
	std::vector<int64_t> meanCov;
	std::vector<uint8_t> cand, branches, inProfile, nucl;
};

// the largest integer n with (double)n / cov <= rate, Python's true division
i32 bubMaxNumerator(double rate, u32 cov)
{
	const double x = rate * (double)cov;
	if (!(x < 2147483000.0)) return 0x7fffffff;
	long long n = (long long)std::floor(x);
	while ((double)(n + 1) / (double)cov <= rate) ++n;
	while (n > 0 && (double)n / (double)cov > rate) --n;
	return (i32)n;
}

void bubSubBatch(fg_ctx* c, const fg_bubble_params& P, u32 c0, u32 c1, const int32_t* contigLen, const uint8_t* contigCirc,
				 const uint64_t* contigAlnOff, const int32_t* trgStart, const int32_t* trgEnd, const uint64_t* colOff,
				 const uint8_t* trgCols, const uint8_t* qryCols, const uint8_t* inProf /* by absolute alignment - first */, u64 aln00,
				 bool wantProfile, BubbleOwner& own, const CigSource* cig = nullptr /* the columns are expanded here, not read from the host */)
{
	hipStream_t s = c->stream;
	const u32 nC = c1 - c0;
	const u64 a0 = contigAlnOff[c0], a1 = contigAlnOff[c1];
	const u32 nAln = (u32)(a1 - a0);
	const u64 col0 = nAln ? colOff[a0] : 0, nCols = nAln ? colOff[a1] - col0 : 0;
	const i32 SOLID = P.solid_kmer_length, SIMPLE = P.simple_kmer_length;

	std::vector<BubContig> ctg(nC);
	std::vector<BubAln> alns(nAln);
	u64 nPos = 0, partCap = 0;
	u32 maxProf = 0;
	for (u32 i = 0; i < nC; ++i)
	{
		BubContig& ct = ctg[i];
		ct.posOff = nPos; ct.partBase = partCap; ct.bubBase = 0; ct.len = contigLen[c0 + i];
		ct.circular = contigCirc && contigCirc[c0 + i] ? 1u : 0u; ct.nPart = 0; ct.pad = 0;
		nPos += (u64)ct.len;
		partCap += (u64)ct.len / (u64)SOLID + 2;
		u32 prof = 0;
		for (u64 a = contigAlnOff[c0 + i]; a < contigAlnOff[c0 + i + 1]; ++a)
		{
			BubAln& al = alns[a - a0];
			al.colOff = colOff[a] - col0; al.nCols = (u32)(colOff[a + 1] - colOff[a]);
			al.trgStart = trgStart[a]; al.trgEnd = trgEnd[a]; al.contig = i; al.inProfile = inProf[a - aln00]; al.pad = 0;
			prof += al.inProfile;
		}
		maxProf = std::max(maxProf, prof);
	}
	if (nPos >= (1ULL << 31) || nAln >= (1u << 24) - 1)
		throw FgError{FG_ERR_NOMEM, "fg_make_bubbles: a sub-batch of 2^31 positions or 2^24 alignments; lower FG_BUBBLE_BATCH_COLS"};
	const u32 tabN = maxProf + 1;
	std::vector<i32> tabMis(tabN, 0), tabIns(tabN, 0);
	for (u32 v = 1; v < tabN; ++v) { tabMis[v] = bubMaxNumerator(P.solid_missmatch, v); tabIns[v] = bubMaxNumerator(P.solid_indel, v); }
	unsigned char acgt[128];
	for (int i = 0; i < 128; ++i) acgt[i] = (unsigned char)i;
	{
		const char* from = "URYKMSWBVDHNXurykmswbvdhnx";
		const char* to = "ACGTACGTACGTAacgtacgtacgta";
		for (int i = 0; from[i]; ++i) acgt[(int)from[i]] = (unsigned char)to[i];
	}

	DevPool B{c->dBub, "fg_make_bubbles"};
	BubAln* dAln = B.get<BubAln>(nAln);
	BubContig* dCtg = B.get<BubContig>(nC);
	// k_cig_expand stores whole words past the last column
	unsigned char* dTrg = B.get<unsigned char>(nCols + (cig ? CIG_LANE_COLS : 0));
	unsigned char* dQry = B.get<unsigned char>(nCols + (cig ? CIG_LANE_COLS : 0));
	unsigned char* dTrgS = B.get<unsigned char>(nCols);
	unsigned char* dQryS = B.get<unsigned char>(nCols);
	i32* dCnt = B.get<i32>(4 * nPos);			// coverage, inserts, deletions, mismatches
	u32* dTag = B.get<u32>(nPos);
	u32* dBad = B.get<u32>(nPos + 1);
	u32* dB = B.get<u32>(nPos + 1);
	u32* dBadPos = B.get<u32>(nPos + 1);
	unsigned char* dFlags = B.get<unsigned char>(3 * nPos);		// solid, landmark, partition point
	i32* dPart = B.get<i32>(partCap);
	i32* dPerC = B.get<i32>(3 * (size_t)nC);	// long bubbles, empty, long branches
	i32* dTab = B.get<i32>(2 * (size_t)tabN);
	unsigned char* dAcgt = B.get<unsigned char>(128);
	u32* dScan = B.get<u32>(fgprim::scanScratchElems(std::max<u64>(nPos + 1, (u64)nAln + 1)) + 8);
	u32* dEmit = B.get<u32>((size_t)nAln + 1);
	i32 *dCov = dCnt, *dIns = dCnt + nPos, *dDel = dCnt + 2 * nPos, *dMis = dCnt + 3 * nPos;
	unsigned char *dSolid = dFlags, *dLm = dFlags + nPos, *dIsPart = dFlags + 2 * nPos;

	HIP_CHECK(hipMemcpyAsync(dAln, alns.data(), (size_t)nAln * sizeof(BubAln), hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dCtg, ctg.data(), (size_t)nC * sizeof(BubContig), hipMemcpyHostToDevice, s));
	CigStaged staged;		// read by the stream until the first wait below
	if (cig && nAln) (void)cigExpandSource(c, *cig, staged, a0, a1, dTrg, dQry);
	else if (nCols)
	{
		HIP_CHECK(hipMemcpyAsync(dTrg, trgCols + col0, nCols, hipMemcpyHostToDevice, s));
		HIP_CHECK(hipMemcpyAsync(dQry, qryCols + col0, nCols, hipMemcpyHostToDevice, s));
	}
	HIP_CHECK(hipMemcpyAsync(dTab, tabMis.data(), (size_t)tabN * 4, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dTab + tabN, tabIns.data(), (size_t)tabN * 4, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dAcgt, acgt, 128, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemsetAsync(dCnt, 0, 4 * nPos * 4 + 4, s));
	HIP_CHECK(hipMemsetAsync(dTag, 0, nPos * 4 + 4, s));
	HIP_CHECK(hipMemsetAsync(dFlags, 0, 3 * nPos + 1, s));
	HIP_CHECK(hipMemsetAsync(dPerC, 0, 3 * (size_t)nC * 4, s));

	if (nAln)
	{
		{
			ScopedK t(c->timer, "k_bub_shift");
			hipLaunchKernelGGL(k_bub_shift, bubWaveGrid(nAln), BUB_BLOCK, 0, s, dAln, nAln, dTrg, dQry, dQryS);
			hipLaunchKernelGGL(k_bub_shift, bubWaveGrid(nAln), BUB_BLOCK, 0, s, dAln, nAln, dQryS, dTrg, dTrgS);
		}
		ScopedK t(c->timer, "k_bub_profile");
		hipLaunchKernelGGL(k_bub_profile, bubWaveGrid(nAln), BUB_BLOCK, 0, s, dAln, nAln, dCtg, dTrgS, dQryS, dCov, dIns, dDel, dMis, dTag);
	}
	{
		ScopedK t(c->timer, "k_bub_good");
		hipLaunchKernelGGL(k_bub_good, bubGrid(nPos + 1), BUB_BLOCK, 0, s, nPos, dCov, dIns, dDel, dMis, dTab, dTab + tabN, tabN, dBad);
	}
	{
		ScopedK t(c->timer, "k_bub_scan");
		fgprim::scan<u32>(s, dBad, dB, nPos + 1, false, dScan);
		if (nPos) hipLaunchKernelGGL(k_bub_badpos, bubGrid(nPos), BUB_BLOCK, 0, s, nPos, dBad, dB, dBadPos);
	}
	if (nPos)
	{
		{
			ScopedK t(c->timer, "k_bub_solid");
			hipLaunchKernelGGL(k_bub_solid, bubGrid(nPos), BUB_BLOCK, 0, s, nPos, dCtg, nC, dBad, dB, dBadPos, SOLID, dSolid);
		}
		ScopedK t(c->timer, "k_bub_landmark");
		hipLaunchKernelGGL(k_bub_landmark, bubGrid(nPos), BUB_BLOCK, 0, s, nPos, dCtg, nC, dSolid, dTag, SOLID, SIMPLE, dLm);
	}
	{
		ScopedK t(c->timer, "k_bub_walk");
		hipLaunchKernelGGL(k_bub_walk, nC, 64, 0, s, dCtg, dLm, dIsPart, dPart, dPerC, SOLID, SIMPLE, P.max_bubble_length);
	}
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipMemcpyAsync(ctg.data(), dCtg, (size_t)nC * sizeof(BubContig), hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	u64 nBubRaw = 0;
	for (u32 i = 0; i < nC; ++i)
	{
		ctg[i].bubBase = nBubRaw;
		nBubRaw += ctg[i].nPart ? (u64)ctg[i].nPart + 1 : 0;
	}
	if (nBubRaw >= (1ULL << 31)) throw FgError{FG_ERR_NOMEM, "fg_make_bubbles: 2^31 bubbles in a sub-batch; lower FG_BUBBLE_BATCH_COLS"};
	const u32 nBub = (u32)nBubRaw;
	HIP_CHECK(hipMemcpyAsync(dCtg, ctg.data(), (size_t)nC * sizeof(BubContig), hipMemcpyHostToDevice, s));

	// branches: count, number the slots, write the records
	std::vector<u32> slotBase((size_t)nAln + 1, 0);
	u64 nSlots = 0;
	u32* dRawCnt = B.get<u32>((size_t)nBub + 1);
	u32* dRawOff = B.get<u32>((size_t)nBub + 1);
	HIP_CHECK(hipMemsetAsync(dRawCnt, 0, ((size_t)nBub + 1) * 4, s));
	if (nAln && nBub)
	{
		{
			ScopedK t(c->timer, "k_bub_cuts");
			hipLaunchKernelGGL(k_bub_cuts<true>, bubWaveGrid(nAln), BUB_BLOCK, 0, s, dAln, nAln, dCtg, dTrg, dQry, dIsPart, dPart, dEmit,
							   (const u32*)nullptr, (u64*)nullptr, (u64*)nullptr, (u64*)nullptr, (u32*)nullptr, (u32*)nullptr, (u32*)nullptr);
		}
		HIP_CHECK(hipMemsetAsync(dEmit + nAln, 0, 4, s));
		{
			ScopedK t(c->timer, "k_bub_scan");
			fgprim::scan<u32>(s, dEmit, dEmit, (u64)nAln + 1, false, dScan);
		}
		HIP_CHECK(hipMemcpyAsync(slotBase.data(), dEmit, ((size_t)nAln + 1) * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		nSlots = slotBase[nAln];
	}
	if (nSlots > fgprim::RS_MAX_N) throw FgError{FG_ERR_NOMEM, "fg_make_bubbles: 2^30 branches in a sub-batch; lower FG_BUBBLE_BATCH_COLS"};
	u64* dKeys0 = B.get<u64>(nSlots);
	u64* dVals0 = B.get<u64>(nSlots);
	u64* dKeys1 = B.get<u64>(nSlots);
	u64* dVals1 = B.get<u64>(nSlots);
	u64* dSegCol = B.get<u64>(nSlots);
	u32* dSeg32 = B.get<u32>(3 * nSlots);		// columns, length, length in sorted order
	char* dSortScratch = B.get<char>(fgprim::radixSortScratchBytes(nSlots));
	unsigned char* dKept = B.get<unsigned char>(nSlots);
	BubPost* dPost = B.get<BubPost>(nBub);
	BubOut* dOuts = B.get<BubOut>(nBub);
	u32 *dSegCols = dSeg32, *dSegLen = dSeg32 + nSlots, *dSortedLen = dSeg32 + 2 * nSlots;
	const u64* dVals = dVals0;
	if (nSlots)
	{
		{
			ScopedK t(c->timer, "k_bub_cuts");
			hipLaunchKernelGGL(k_bub_cuts<false>, bubWaveGrid(nAln), BUB_BLOCK, 0, s, dAln, nAln, dCtg, dTrg, dQry, dIsPart, dPart,
							   (u32*)nullptr, dEmit, dKeys0, dVals0, dSegCol, dSegCols, dSegLen, dRawCnt);
		}
		int bits = 1;
		while ((1ULL << bits) < nBubRaw) ++bits;
		ScopedK t(c->timer, "k_bub_sort");
		const int where = fgprim::radixSortPairs(s, dKeys0, dVals0, dKeys1, dVals1, nSlots, 0, bits, dSortScratch);
		dVals = where ? dVals1 : dVals0;
	}
	{
		ScopedK t(c->timer, "k_bub_scan");
		fgprim::scan<u32>(s, dRawCnt, dRawOff, (u64)nBub + 1, false, dScan);
	}
	std::vector<BubPost> post(nBub);
	std::vector<u32> rawOff((size_t)nBub + 1, 0);
	if (nBub)
	{
		ScopedK t(c->timer, "k_bub_post");
		if (nSlots) hipLaunchKernelGGL(k_bub_gather, bubGrid(nSlots), BUB_BLOCK, 0, s, nSlots, dVals, dSegLen, dSortedLen);
		hipLaunchKernelGGL(k_bub_post, bubWaveGrid(nBub), BUB_BLOCK, 0, s, nBub, dCtg, nC, dPart, dTag, dRawOff, dSortedLen,
						   P.max_bubble_length, P.max_bubble_branches, dKept, dPost, dPerC + nC, dPerC + 2 * (size_t)nC);
	}
	HIP_CHECK(hipGetLastError());
	if (nBub) HIP_CHECK(hipMemcpyAsync(post.data(), dPost, (size_t)nBub * sizeof(BubPost), hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipMemcpyAsync(rawOff.data(), dRawOff, ((size_t)nBub + 1) * 4, hipMemcpyDeviceToHost, s));
	std::vector<i32> perC(3 * (size_t)nC);
	HIP_CHECK(hipMemcpyAsync(perC.data(), dPerC, perC.size() * 4, hipMemcpyDeviceToHost, s));
	std::vector<i32> part(partCap);
	HIP_CHECK(hipMemcpyAsync(part.data(), dPart, partCap * 4, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));

	// offsets of the kept bubbles, in the call's arrays
	const u64 candBase = own.cand.size(), byteBase0 = own.branches.size(), slotBase0 = own.branchOff.size();
	u64 candAt = candBase, byteAt = byteBase0, slotAt = slotBase0;
	std::vector<BubOut> outs(nBub);
	for (u32 i = 0; i < nC; ++i)
	{
		const BubContig& ct = ctg[i];
		const u32 nb = ct.nPart ? ct.nPart + 1 : 0;
		for (u32 k = 0; k < nb; ++k)
		{
			const u32 b = (u32)ct.bubBase + k;
			outs[b] = BubOut{candAt, slotAt, byteAt};
			if (!post[b].keep) continue;
			own.position.push_back(k == 0 ? 0 : part[ct.partBase + k - 1]);
			own.candOff.push_back(candAt);
			own.bubbleBranchOff.push_back(slotAt);
			candAt += post[b].consLen; slotAt += post[b].nKept; byteAt += post[b].keptBytes;
		}
		own.bubbleOff.push_back(own.position.size());
		own.nLongBubbles.push_back(perC[i]);
		own.nEmpty.push_back(perC[nC + i]);
		own.nLongBranch.push_back(perC[2 * (size_t)nC + i]);
		own.nPartition.push_back((i32)ct.nPart);
		const u64 rawBr = nb ? (u64)rawOff[ct.bubBase + nb] - rawOff[ct.bubBase] : 0;
		own.meanCov.push_back((int64_t)(rawBr / ((u64)nb + 1)));
		if (wantProfile)
		{
			own.partition.insert(own.partition.end(), part.begin() + ct.partBase, part.begin() + ct.partBase + ct.nPart);
			own.partOff.push_back(own.partition.size());
			own.profOff.push_back(own.profOff.back() + (u64)ct.len);
		}
	}
	unsigned char* dCand = B.get<unsigned char>(candAt - candBase);
	unsigned char* dBr = B.get<unsigned char>(byteAt - byteBase0);
	u64* dBrOff = B.get<u64>(slotAt - slotBase0);
	if (nBub)
	{
		HIP_CHECK(hipMemcpyAsync(dOuts, outs.data(), (size_t)nBub * sizeof(BubOut), hipMemcpyHostToDevice, s));
		ScopedK t(c->timer, "k_bub_fill");
		hipLaunchKernelGGL(k_bub_fill, bubWaveGrid(nBub), BUB_BLOCK, 0, s, nBub, dCtg, nC, dPart, dTag, dRawOff, dVals, dSegCol, dSegCols,
						   dSortedLen, dKept, dPost, dOuts, dQry, dAcgt, dCand, candBase, dBr, byteBase0, dBrOff, slotBase0);
	}
	HIP_CHECK(hipGetLastError());
	own.cand.resize(candAt);
	own.branches.resize(byteAt);
	own.branchOff.resize(slotAt);
	if (candAt > candBase) HIP_CHECK(hipMemcpyAsync(own.cand.data() + candBase, dCand, candAt - candBase, hipMemcpyDeviceToHost, s));
	if (byteAt > byteBase0) HIP_CHECK(hipMemcpyAsync(own.branches.data() + byteBase0, dBr, byteAt - byteBase0, hipMemcpyDeviceToHost, s));
	if (slotAt > slotBase0) HIP_CHECK(hipMemcpyAsync(own.branchOff.data() + slotBase0, dBrOff, (slotAt - slotBase0) * 8, hipMemcpyDeviceToHost, s));
	if (wantProfile && nPos)
	{
		const size_t at = own.coverage.size();
		own.coverage.resize(at + nPos); own.numInserts.resize(at + nPos); own.numDeletions.resize(at + nPos);
		own.numMissmatch.resize(at + nPos); own.nucl.resize(at + nPos);
		// the bad words are no longer needed: their buffer takes the bytes
		unsigned char* dNucl = (unsigned char*)dBad;
		hipLaunchKernelGGL(k_bub_nucl, bubGrid(nPos), BUB_BLOCK, 0, s, nPos, dTag, dNucl);
		HIP_CHECK(hipMemcpyAsync(own.coverage.data() + at, dCov, nPos * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipMemcpyAsync(own.numInserts.data() + at, dIns, nPos * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipMemcpyAsync(own.numDeletions.data() + at, dDel, nPos * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipMemcpyAsync(own.numMissmatch.data() + at, dMis, nPos * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipMemcpyAsync(own.nucl.data() + at, dNucl, nPos, hipMemcpyDeviceToHost, s));
	}
	HIP_CHECK(hipStreamSynchronize(s));
}

// the finished owner into the caller's struct
void bubHandOver(struct fg_bubble_batch* out, BubbleOwner* own, uint32_t n_contigs, bool want_profile)
{
	out->n_contigs = n_contigs;
	out->n_bubbles = (uint32_t)own->position.size();
	out->n_alignments = (uint64_t)own->inProfile.size();
	out->bubble_off = own->bubbleOff.data();
	out->position = own->position.data();
	out->cand = own->cand.data();
	out->cand_off = own->candOff.data();
	out->branches = own->branches.data();
	out->branch_off = own->branchOff.data();
	out->bubble_branch_off = own->bubbleBranchOff.data();
	out->n_long_bubbles = own->nLongBubbles.data();
	out->n_empty = own->nEmpty.data();
	out->n_long_branch = own->nLongBranch.data();
	out->mean_cov = own->meanCov.data();
	out->n_partition = own->nPartition.data();
	out->in_profile = own->inProfile.data();
	if (want_profile)
	{
		out->part_off = own->partOff.data();
		out->partition = own->partition.data();
		out->prof_off = own->profOff.data();
		out->coverage = own->coverage.data();
		out->num_inserts = own->numInserts.data();
		out->num_deletions = own->numDeletions.data();
		out->num_missmatch = own->numMissmatch.data();
		out->nucl = own->nucl.data();
	}
	out->owner_ = own;
}

// what both calls check of the parameters
void bubCheckParams(const std::string& name, const fg_bubble_params& P)
{
	if (P.solid_kmer_length <= 0 || P.simple_kmer_length <= 0 || P.max_bubble_length <= 0 || P.max_bubble_branches <= 0 ||
		P.min_polish_aln_len <= 0)
		throw FgError{FG_ERR_ARG, name + ": a length or cap <= 0"};
	for (double r : {P.solid_missmatch, P.solid_indel, P.max_aln_error})
		if (!(r >= 0.0)) throw FgError{FG_ERR_ARG, name + ": a rate that is NaN or negative"};
	const long long S = P.simple_kmer_length, K = P.solid_kmer_length;
	if (S % 2 || S < 2 || S > 2 * K || 3 * S / 2 > K + 1)
		throw FgError{FG_ERR_UNSUPPORTED, name + ": simple_kmer_length " + std::to_string(S) + " with solid_kmer_length " +
											  std::to_string(K) + " would slice outside the profile"};
}

// the call's last offsets and non-null pointers for empty arrays
void bubClose(BubbleOwner* own)
{
	own->candOff.push_back(own->cand.size());
	own->bubbleBranchOff.push_back(own->branchOff.size());
	own->branchOff.push_back(own->branches.size());
	stageKeep(own->cand, own->branches, own->inProfile, own->nucl, own->position, own->nLongBubbles, own->nEmpty, own->nLongBranch,
			  own->nPartition, own->partition, own->coverage, own->numInserts, own->numDeletions, own->numMissmatch, own->meanCov);
}

} // namespace

extern "C" {

int fg_make_bubbles(fg_ctx* c, const struct fg_bubble_params* params, uint32_t n_contigs, const int32_t* contig_len,
					const uint8_t* contig_circular, const uint64_t* contig_aln_off, const int32_t* trg_start, const int32_t* trg_end,
					const double* err_rate, const uint64_t* col_off, const uint8_t* trg_cols, const uint8_t* qry_cols,
					uint8_t want_profile, struct fg_bubble_batch* out)
{
	return stageCall<BubbleOwner>(c, out, [&](BubbleOwner*& own)
	{
		const std::string name = "fg_make_bubbles";
		if (!params || !out) throw FgError{FG_ERR_ARG, name + ": null params or result"};
		const fg_bubble_params& P = *params;
		bubCheckParams(name, P);
		stageContigTable(name, n_contigs, contig_len, contig_aln_off);
		const u64 a0 = n_contigs ? contig_aln_off[0] : 0, a1 = n_contigs ? contig_aln_off[n_contigs] : 0;
		if (a1 > a0 && (!trg_start || !trg_end || !err_rate || !col_off))
			throw FgError{FG_ERR_ARG, name + ": null trg_start, trg_end, err_rate or col_off"};
		stageColOff(name, col_off, a0, a1, trg_cols, qry_cols, [&](u64 a)
		{
			if (!(err_rate[a] >= 0.0)) throw FgError{FG_ERR_ARG, name + ": err_rate NaN or negative at alignment " + std::to_string(a)};
		});
		own = new BubbleOwner;
		own->inProfile.assign((size_t)(a1 - a0), 0);
		std::vector<u64> cost(n_contigs, 0);
		for (u32 i = 0; i < n_contigs; ++i)
		{
			for (u64 a = contig_aln_off[i]; a < contig_aln_off[i + 1]; ++a)
			{
				// the order of the reports is part of the call: trg_start first, then the bytes (fg_contig_consensus and
				// fg_divergence_profile: the bytes first)
				stageStartOnContig(name, a, trg_start[a], contig_len[i]);
				stageBasesOnContig(name, a, stageColumnWalk(name, a, col_off, trg_cols, qry_cols), contig_len[i]);
				const u64 nCols = col_off[a + 1] - col_off[a];
				own->inProfile[a - a0] = !(err_rate[a] > P.max_aln_error) && nCols >= (u64)P.min_polish_aln_len;
			}
			// a contig counts its columns and its positions
			cost[i] = (u64)contig_len[i];
			if (contig_aln_off[i + 1] > contig_aln_off[i]) cost[i] += col_off[contig_aln_off[i + 1]] - col_off[contig_aln_off[i]];
		}
		const u64 budget = stageEnvU64("FG_BUBBLE_BATCH_COLS", 1ULL << 27);
		const u64 maxContigs = stageEnvCap("FG_BUBBLE_BATCH_CONTIGS");		// a switch for tests: contigs per sub-batch
		own->bubbleOff.assign(1, 0);
		if (want_profile) { own->partOff.assign(1, 0); own->profOff.assign(1, 0); }
		HIP_CHECK(hipSetDevice(c->device));
		c->timer.reset();
		stageAllFit(name, "contig", cost, budget, "columns and positions", "FG_BUBBLE_BATCH_COLS");
		for (u32 i = 0; i < n_contigs;)
		{
			const u32 j = stageCut(i, n_contigs, cost, budget, maxContigs);
			bubSubBatch(c, P, i, j, contig_len, contig_circular, contig_aln_off, trg_start, trg_end, col_off, trg_cols, qry_cols,
						own->inProfile.data(), a0, want_profile != 0, *own);
			i = j;
		}
		c->timer.collect();
		bubClose(own);
		bubHandOver(out, own, n_contigs, want_profile != 0);
	});
}

int fg_make_bubbles_cigars(fg_ctx* c, const struct fg_bubble_params* params, uint32_t n_contigs, const uint64_t* contig_off,
						   const uint8_t* contig_seq, const uint8_t* contig_circular, const uint64_t* contig_aln_off, const int32_t* ctg_pos,
						   const uint64_t* run_off, const uint8_t* run_op, const uint32_t* run_len, const uint64_t* read_off,
						   const uint8_t* read_seq, const double* err_rate, uint8_t want_profile, struct fg_bubble_batch* out)
{
	return stageCall<BubbleOwner>(c, out, [&](BubbleOwner*& own)
	{
		const std::string name = "fg_make_bubbles_cigars";
		if (!params || !out) throw FgError{FG_ERR_ARG, name + ": null params or result"};
		const fg_bubble_params& P = *params;
		bubCheckParams(name, P);
		if (n_contigs && !contig_aln_off) throw FgError{FG_ERR_ARG, name + ": null contig_aln_off"};
		stageOffsets(name, "contig_aln_off", "contig ", contig_aln_off, 0, n_contigs);
		const u64 a0 = n_contigs ? contig_aln_off[0] : 0, a1 = n_contigs ? contig_aln_off[n_contigs] : 0;
		std::vector<uint32_t> alnContig((size_t)a1, 0);
		for (u32 i = 0; i < n_contigs; ++i)
			for (u64 a = contig_aln_off[i]; a < contig_aln_off[i + 1]; ++a) alnContig[a] = i;
		// every check of fg_expand_cigars, then those fg_make_bubbles makes on what the expansion would hand it
		CigPlan plan;
		cigCheckRecords(name, n_contigs, contig_off, contig_seq, a0, a1, alnContig.data(), !ctg_pos || !run_off || !read_off || !err_rate,
						"null ctg_pos, run_off, read_off or err_rate", ctg_pos, run_off, run_op, run_len, read_off, read_seq, plan);
		for (u64 a = a0; a < a1; ++a)
			if (!(err_rate[a] >= 0.0)) throw FgError{FG_ERR_ARG, name + ": err_rate NaN or negative at alignment " + std::to_string(a)};
		own = new BubbleOwner;
		own->inProfile.assign((size_t)(a1 - a0), 0);
		std::vector<int32_t> contigLen(n_contigs, 0);
		std::vector<u64> cost(n_contigs, 0);
		for (u32 i = 0; i < n_contigs; ++i)
		{
			if (contig_off[i + 1] - contig_off[i] > CIG_I32) throw FgError{FG_ERR_ARG, name + ": contig " + std::to_string(i) + " has 2^31 bytes"};
			contigLen[i] = (int32_t)(contig_off[i + 1] - contig_off[i]);
			for (u64 a = contig_aln_off[i]; a < contig_aln_off[i + 1]; ++a)
			{
				// an alignment of insertions alone may stand behind the last base
				stageStartOnContig(name, a, plan.trgStart[a], contigLen[i]);
				own->inProfile[a - a0] = !(err_rate[a] > P.max_aln_error) && plan.tot[a].cols >= (u64)P.min_polish_aln_len;
			}
			// a contig counts its columns and its positions
			cost[i] = (u64)contigLen[i] + (plan.colOff[contig_aln_off[i + 1]] - plan.colOff[contig_aln_off[i]]);
		}
		const u64 budget = stageEnvU64("FG_BUBBLE_BATCH_COLS", 1ULL << 27);
		const u64 maxContigs = stageEnvCap("FG_BUBBLE_BATCH_CONTIGS");		// a switch for tests: contigs per sub-batch
		own->bubbleOff.assign(1, 0);
		if (want_profile) { own->partOff.assign(1, 0); own->profOff.assign(1, 0); }
		HIP_CHECK(hipSetDevice(c->device));
		c->timer.reset();
		stageAllFit(name, "contig", cost, budget, "columns and positions", "FG_BUBBLE_BATCH_COLS");
		// the contig bytes go up once per call; a sub-batch expands its own alignments
		const CigSource src{&plan, a1 > a0 ? cigUploadContigs(c, plan, contig_seq) : nullptr, run_off, run_op, run_len, read_off, read_seq, cigTile()};
		for (u32 i = 0; i < n_contigs;)
		{
			const u32 j = cigCutContigs(name, "FG_BUBBLE_BATCH_COLS", i, n_contigs, cost, budget, maxContigs, contig_aln_off, run_off, read_off);
			bubSubBatch(c, P, i, j, contigLen.data(), contig_circular, contig_aln_off, plan.trgStart.data(), plan.trgEnd.data(),
						plan.colOff.data(), nullptr, nullptr, own->inProfile.data(), a0, want_profile != 0, *own, &src);
			i = j;
		}
		c->timer.collect();
		bubClose(own);
		bubHandOver(out, own, n_contigs, want_profile != 0);
	});
}

void fg_release_bubbles(struct fg_bubble_batch* b) { stageRelease<BubbleOwner>(b); }

} // extern "C"
