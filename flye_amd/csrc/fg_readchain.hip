// fg_chain_alignments: the edge-chain step of ReadAligner::alignReads (reference src/repeat_graph/read_aligner.cpp:212-262)
// for a batch of reads: the lambda's filter (:224-226), its std::sort by curBegin (:233-235), chainReadAlignments
// (:24-154) with its std::sort by score (:119-123) and the greedy selection (:126-151).  Integers only.
//
//   k_rc_filter<false>  kept records per query (:224-226)
//   k_rc_filter<true>   the same walk once more: key = curBegin, value = rank among the kept ones, and the kept record's
//                       position in the query's list, in input order at the query's segment
//   (fgSortSegments)    std::sort's permutation per query (:233-235)
//   k_rc_gather         the sorted alignments with what the DP reads of each: spans, the two graph gaps, the two nodes
//   k_rc_chain          :32-117, one wave per query.  Every alignment creates exactly one chain whose last alignment is
//                       the alignment itself, so a chain is (predecessor, score, first alignment, depth) under the
//                       alignment's index and the two deques are lists of indices.  The outer loop is serial; the lanes
//                       stride over the active list: candidate test, wave reduction to (best score, earliest position),
//                       ballot count of the outdated chains, ballot-ranked compaction for the cleanup (:96-116)
//   (fgSortSegments)    std::sort by score, descending, of "active then frozen" (:119-123): key = 2^31 - score
//   k_rc_select         :126-151, one wave per query, lanes over the accepted spans
//   k_rc_write          each accepted chain from front to back as indices into the caller's records, and its score
//
// All per-query state lives in global scratch at the query's segment of the sub-batch (one element per kept record in
// every array).  A block is one wave; the lists a wave's lanes hand to one another go through that scratch with a
// workgroup barrier between the store and the loads that follow.  Every loop is bounded by the query's record count.
#include "fg_ctx.h"
#include "fg_stage.h"
#include "fg_devprim.h"

namespace {

#define RC_BLOCK 256
#define RC_MAX_WAVES 16384u		// waves of the per-query kernels; the rest of a sub-batch by grid stride
#define RC_NONE 0xFFFFFFFFu

// one sorted alignment as the DP reads it
struct RcAln {
	i32 curBegin, curEnd, extBegin, rightGap, score;	// rightGap = extLen - extEnd
	u32 nodeLeft, nodeRight;
	u32 rec;											// position in the query's input list
};

// the arrays of a sub-batch, one element per kept record unless noted (the query's part at seg[q])
struct RcState {
	const u64* qOff;		// nq + 1: the records of query q in the side table
	const u64* seg;			// nq + 1: the kept records of query q
	RcAln* aln;
	i32* score;				// Chain::score of the chain that ends in alignment i
	u32* pred;				// its alignment before the last one, RC_NONE for a chain of one
	u32* first;				// its first alignment
	u32* depth;				// its number of alignments
	u32* active;			// the two deques; after the DP: active = "active then frozen"
	u32* frozen;
	u32* accChain;			// accepted chains in order, their spans and where each one's alignments start in the query's output
	i32* accBegin;
	i32* accEnd;
	u32* accAlnAt;
	u32* accCnt;			// nq
	u32* accAlns;			// nq
};

__device__ __forceinline__ u32 lane_rank(u64 m)
{
	return __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0));
}

__device__ __forceinline__ bool rc_keep(const FgChainAln& a, i32 longEdge, i32 bigAlignment)
{
	const i32 cr = a.curEnd - a.curBegin, er = a.extEnd - a.extBegin;
	return a.extLen < longEdge || (cr < er ? cr : er) > bigAlignment;
}

template <bool EMIT>
__global__ void __launch_bounds__(64)
k_rc_filter(const FgChainAln* __restrict__ tab, const u64* __restrict__ qOff, u32 nq, i32 longEdge, i32 bigAlignment,
			u64* __restrict__ cnt, const u64* __restrict__ seg, u64* __restrict__ keys, u32* __restrict__ vals, u32* __restrict__ ord)
{
	const int lane = threadIdx.x;
	for (u32 q = blockIdx.x; q < nq; q += gridDim.x)
	{
		const u64 a = fg_uni(qOff[q]), b = fg_uni(qOff[q + 1]);
		const u64 dst = EMIT ? fg_uni(seg[q]) : 0;
		const u64 room = EMIT ? fg_uni(seg[q + 1]) - dst : 0;
		u64 w = 0;
		for (u64 k0 = a; k0 < b; k0 += 64)
		{
			const u64 k = k0 + lane;
			FgChainAln r{};
			bool keep = false;
			if (k < b) { r = tab[k]; keep = rc_keep(r, longEdge, bigAlignment); }
			const u64 m = __builtin_amdgcn_ballot_w64(keep);
			if (EMIT && keep)
			{
				const u64 at = w + lane_rank(m);
				if (at < room)
				{
					keys[dst + at] = (u64)(u32)r.curBegin;
					vals[dst + at] = (u32)at;
					ord[dst + at] = (u32)(k - a);
				}
			}
			w += (u64)__popcll(m);
		}
		if (!EMIT && lane == 0) cnt[q] = w;
	}
}

// the p < n with off[p] <= g < off[p + 1]
__device__ __forceinline__ u32 rc_seg_of(const u64* __restrict__ off, u32 n, u64 g)
{
	u32 lo = 0, hi = n;
	while (hi - lo > 1)
	{
		const u32 mid = (lo + hi) >> 1;
		if (off[mid] <= g) lo = mid; else hi = mid;
	}
	return lo;
}

// aln[g] = the alignment std::sort left at position g of its query's list
__global__ void __launch_bounds__(RC_BLOCK)
k_rc_gather(const FgChainAln* __restrict__ tab, const u64* __restrict__ qOff, const u64* __restrict__ seg, u32 nq, u64 nKept,
			const u32* __restrict__ vals, const u32* __restrict__ ord, const u32* __restrict__ nodeLeft,
			const u32* __restrict__ nodeRight, u32 nExt, RcAln* __restrict__ aln)
{
	for (u64 g = (u64)blockIdx.x * RC_BLOCK + threadIdx.x; g < nKept; g += (u64)gridDim.x * RC_BLOCK)
	{
		const u32 q = rc_seg_of(seg, nq, g);
		const u64 base = seg[q], m = seg[q + 1] - base;
		u32 v = vals[g];
		if (v >= m) v = 0;			// never: the sort permutes 0 .. m - 1
		const u32 at = ord[base + v];
		const FgChainAln r = tab[qOff[q] + at];
		const u32 e = r.ext < nExt ? r.ext : 0u;	// checked by the caller
		RcAln o;
		o.curBegin = r.curBegin; o.curEnd = r.curEnd; o.extBegin = r.extBegin; o.rightGap = r.extLen - r.extEnd;
		o.score = r.score; o.nodeLeft = nodeLeft[e]; o.nodeRight = nodeRight[e]; o.rec = at;
		aln[g] = o;
	}
}

__device__ __forceinline__ u64 wave_max(u64 v)
{
	for (int o = 32; o > 0; o >>= 1)
	{
		const u32 lo = __shfl_xor((u32)v, o), hi = __shfl_xor((u32)(v >> 32), o);
		const u64 t = ((u64)hi << 32) | lo;
		if (t > v) v = t;
	}
	return v;
}

__global__ void __launch_bounds__(64)
k_rc_chain(RcState S, u32 nq, i32 maxJump, i32 maxReadOverlap, u64* __restrict__ keys, u32* __restrict__ vals)
{
	const int lane = threadIdx.x;
	for (u32 q = blockIdx.x; q < nq; q += gridDim.x)
	{
		const u64 base = fg_uni(S.seg[q]);
		const u32 m = (u32)(fg_uni(S.seg[q + 1]) - base);
		const RcAln* A = S.aln + base;
		i32* score = S.score + base;
		u32* pred = S.pred + base;
		u32* first = S.first + base;
		u32* depth = S.depth + base;
		u32* act = S.active + base;
		u32* frz = S.frozen + base;
		u32 nAct = 0, nFrz = 0;
		for (u32 i = 0; i < m; ++i)
		{
			const RcAln nx = A[i];			// the same address in every lane
			const bool canExtend = nx.extBegin < maxJump;
			const bool canBeExtended = nx.rightGap < maxJump;
			u64 best = 0;					// score << 32 | ~position: the largest score, the earliest position among equals
			u32 numOutdated = 0;
			if (canExtend)
			{
				for (u32 t0 = 0; t0 < nAct; t0 += 64)
				{
					const u32 t = t0 + lane;
					bool outdated = false;
					if (t < nAct)
					{
						const u32 j = act[t];
						const RcAln pv = A[j];
						const i32 readDiff = nx.curBegin - pv.curEnd;
						const i32 graphDiff = nx.extBegin + pv.rightGap;
						if (pv.nodeRight == nx.nodeLeft && maxJump > readDiff && readDiff > -maxReadOverlap && graphDiff < maxJump)
						{
							i32 jumpDiv = readDiff - graphDiff;
							if (jumpDiv < 0) jumpDiv = -jumpDiv;
							const i32 gapCost = jumpDiv > 100 ? jumpDiv / 50 : 0;
							const i32 sc = (i32)((u32)score[j] + (u32)nx.score - (u32)gapCost);
							if (sc > 0)
							{
								const u64 cand = ((u64)(u32)sc << 32) | (u64)(0xFFFFFFFFu - t);
								if (cand > best) best = cand;
							}
						}
						outdated = readDiff > maxJump;
					}
					numOutdated += (u32)__popcll(__builtin_amdgcn_ballot_w64(outdated));
				}
				best = wave_max(best);
			}
			if (lane == 0)
			{
				if (best)
				{
					const u32 j = act[0xFFFFFFFFu - (u32)best];
					score[i] = (i32)(u32)(best >> 32); pred[i] = j; first[i] = first[j]; depth[i] = depth[j] + 1;
					act[nAct] = i;
				}
				else
				{
					score[i] = nx.score; pred[i] = RC_NONE; first[i] = i; depth[i] = 1;
					if (canBeExtended) act[nAct] = i; else frz[nFrz] = i;
				}
			}
			if (best || canBeExtended) ++nAct; else ++nFrz;
			__syncthreads();		// one wave: the stores above before the loads of the cleanup and of the next alignment
			if (numOutdated > nAct / 2)
			{
				u32 w = 0;
				for (u32 t0 = 0; t0 < nAct; t0 += 64)
				{
					const u32 t = t0 + lane;
					u32 j = 0;
					bool live = false, old = false;
					if (t < nAct)
					{
						j = act[t];
						old = nx.curBegin - A[j].curEnd > maxJump;
						live = !old;
					}
					const u64 mo = __builtin_amdgcn_ballot_w64(old), ml = __builtin_amdgcn_ballot_w64(live);
					// w + rank <= t: a slot is written only after the step that read it
					if (old && nFrz + lane_rank(mo) < m) frz[nFrz + lane_rank(mo)] = j;
					if (live) act[w + lane_rank(ml)] = j;
					nFrz += (u32)__popcll(mo);
					w += (u32)__popcll(ml);
					__syncthreads();
				}
				nAct = w;
			}
		}
		// active then frozen (:119-120), with the keys of the sort by score
		for (u32 t = lane; t < nFrz && nAct + t < m; t += 64) act[nAct + t] = frz[t];
		__syncthreads();
		for (u32 t = lane; t < m; t += 64)
		{
			const u32 ch = act[t] < m ? act[t] : 0u;		// always: every alignment's chain is in exactly one of the lists
			keys[base + t] = (u64)((long long)(1LL << 31) - (long long)score[ch]);
			vals[base + t] = t;
		}
		__syncthreads();
	}
}

__global__ void __launch_bounds__(64)
k_rc_select(RcState S, u32 nq, i32 minAlignment, i32 maxSeparation, const u32* __restrict__ vals)
{
	const int lane = threadIdx.x;
	for (u32 q = blockIdx.x; q < nq; q += gridDim.x)
	{
		const u64 base = fg_uni(S.seg[q]);
		const u32 m = (u32)(fg_uni(S.seg[q + 1]) - base);
		const RcAln* A = S.aln + base;
		u32 nAcc = 0, nAlns = 0;
		for (u32 t = 0; t < m; ++t)
		{
			u32 v = fg_uni(vals[base + t]);
			if (v >= m) v = 0;			// never
			u32 ch = fg_uni(S.active[base + v]);
			if (ch >= m) ch = 0;		// never
			const i32 curStart = fg_uni(A[S.first[base + ch]].curBegin), curEnd = fg_uni(A[ch].curEnd);
			if (curEnd - curStart < minAlignment) continue;
			bool overlaps = false;
			for (u32 k = lane; k < nAcc; k += 64)
			{
				const i32 es = S.accBegin[base + k], ee = S.accEnd[base + k];
				overlaps |= (curEnd < ee ? curEnd : ee) - (curStart > es ? curStart : es) > maxSeparation;
			}
			if (__builtin_amdgcn_ballot_w64(overlaps)) continue;
			const u32 d = fg_uni(S.depth[base + ch]);
			if (lane == 0)
			{
				S.accChain[base + nAcc] = ch; S.accBegin[base + nAcc] = curStart; S.accEnd[base + nAcc] = curEnd;
				S.accAlnAt[base + nAcc] = nAlns;
			}
			++nAcc; nAlns += d;
			__syncthreads();		// the span is read by the lanes of the next candidates
		}
		if (lane == 0) { S.accCnt[q] = nAcc; S.accAlns[q] = nAlns; }
	}
}

// chainAt / alnAt: nq + 1 offsets of the queries' chains / alignments in the sub-batch's output.  outOff[c] = where
// chain c's alignments start (the caller adds the last entry); the alignments themselves as recBase + qOff[q] + position
__global__ void __launch_bounds__(64)
k_rc_write(RcState S, u32 nq, const u64* __restrict__ chainAt, const u64* __restrict__ alnAt, u64 recBase,
		   u64* __restrict__ outOff, u64* __restrict__ outAln, i32* __restrict__ outScore)
{
	const int lane = threadIdx.x;
	for (u32 q = blockIdx.x; q < nq; q += gridDim.x)
	{
		const u64 base = fg_uni(S.seg[q]);
		const u32 m = (u32)(fg_uni(S.seg[q + 1]) - base);
		const u64 c0 = fg_uni(chainAt[q]), a0 = fg_uni(alnAt[q]), a1 = fg_uni(alnAt[q + 1]);
		const u32 nAcc = (u32)(fg_uni(chainAt[q + 1]) - c0);
		const u64 rec0 = recBase + fg_uni(S.qOff[q]);
		for (u32 k = lane; k < nAcc; k += 64)
		{
			const u32 ch = S.accChain[base + k];
			const u64 at = a0 + S.accAlnAt[base + k];
			const u32 d = S.depth[base + ch];
			outOff[c0 + k] = at;
			outScore[c0 + k] = S.score[base + ch];
			u32 j = ch;
			for (u32 s = d; s > 0 && j < m; --s)		// back to front
			{
				if (at + s - 1 < a1) outAln[at + s - 1] = rec0 + S.aln[base + j].rec;
				j = S.pred[base + j];
			}
		}
	}
}

} // namespace

// fg_chain_alignments behind its argument checks.  tab: the side table of all records, qOff: nq + 1 offsets into it;
// recBase: what the caller's query_off[0] is (the output names records of the caller's array).  chainOff (nq + 1),
// alnOff (chains + 1), aln, score as fg_chain_batch describes them.
void fgChainAlignments(fg_ctx* c, const fg_chain_params& p, const std::vector<FgChainAln>& tab, const std::vector<u64>& qOff,
					   u64 recBase, const u32* nodeLeft, const u32* nodeRight, u32 nExt, std::vector<u64>& chainOff,
					   std::vector<u64>& alnOff, std::vector<u64>& aln, std::vector<i32>& score)
{
	const u32 nq = (u32)(qOff.size() - 1);
	chainOff.assign((size_t)nq + 1, 0);
	alnOff.assign(1, 0);
	aln.clear(); score.clear();
	if (!nq || tab.empty()) return;
	hipStream_t s = c->stream;
	u64 batch = stageEnvU64("FG_READCHAIN_BATCH_RECS", 1ULL << 20);
	batch = std::min<u64>(std::max<u64>(batch, 1), 1ULL << 28);
	c->timer.reset();
	c->dRcNodes.reserve(2 * (size_t)nExt);
	u32* dNodeL = c->dRcNodes.p;
	u32* dNodeR = dNodeL + nExt;
	HIP_CHECK(hipMemcpyAsync(dNodeL, nodeLeft, (size_t)nExt * 4, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dNodeR, nodeRight, (size_t)nExt * 4, hipMemcpyHostToDevice, s));
	std::vector<u64> localOff, at;
	std::vector<u32> hCnt;
	std::vector<u64> hOutOff, hOutAln;
	std::vector<i32> hOutScore;
	u32 qa = 0;
	while (qa < nq)
	{
		// queries [qa, qb): as many as fit the record bound (a query beyond it runs alone)
		u32 qb = qa + 1;
		while (qb < nq && qOff[qb + 1] - qOff[qa] <= batch) ++qb;
		const u32 n = qb - qa;
		const u64 r0 = qOff[qa], nRec = qOff[qb] - r0;
		if (!nRec) { for (u32 q = qa; q < qb; ++q) chainOff[q + 1] = chainOff[qa]; qa = qb; continue; }
		localOff.resize((size_t)n + 1);
		for (u32 i = 0; i <= n; ++i) localOff[i] = qOff[qa + i] - r0;
		const unsigned waves = std::min<unsigned>(n, RC_MAX_WAVES);
		c->dRcTab.reserve(nRec * sizeof(FgChainAln));
		c->dRcOff.reserve(5 * ((size_t)n + 1) + fgprim::scanScratchElems((u64)n + 1));
		u64* dQOff = c->dRcOff.p;
		u64* dCnt = dQOff + (n + 1);
		u64* dSeg = dCnt + (n + 1);
		u64* dChainAt = dSeg + (n + 1);
		u64* dAlnAt = dChainAt + (n + 1);
		u64* dScan = dAlnAt + (n + 1);
		const FgChainAln* dTab = (const FgChainAln*)c->dRcTab.p;
		HIP_CHECK(hipMemcpyAsync(c->dRcTab.p, tab.data() + r0, nRec * sizeof(FgChainAln), hipMemcpyHostToDevice, s));
		HIP_CHECK(hipMemcpyAsync(dQOff, localOff.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
		HIP_CHECK(hipMemsetAsync(dCnt + n, 0, 8, s));
		{
			ScopedK t(c->timer, "k_rc_filter");
			hipLaunchKernelGGL(k_rc_filter<false>, waves, 64, 0, s, dTab, dQOff, n, p.long_edge, p.big_alignment, dCnt,
							   (const u64*)nullptr, (u64*)nullptr, (u32*)nullptr, (u32*)nullptr);
			fgprim::scan<u64>(s, dCnt, dSeg, (u64)n + 1, false, dScan);
		}
		c->hScalar.reserve(8);
		HIP_CHECK(hipMemcpyAsync(c->hScalar.p, dSeg + n, 8, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		const u64 nKept = c->hScalar.p[0];
		if (nKept > nRec) throw FgError{FG_ERR_HIP, "internal: fg_chain_alignments kept more records than it was given"};
		if (!nKept) { for (u32 q = qa; q < qb; ++q) chainOff[q + 1] = chainOff[qa]; qa = qb; continue; }
		c->dRcKeys.reserve(nKept); c->dRcVals.reserve(nKept);
		c->dRcAln.reserve(nKept * sizeof(RcAln));
		c->dRcU32.reserve(11 * nKept + 2 * (size_t)n);
		RcState S{};
		S.qOff = dQOff; S.seg = dSeg; S.aln = (RcAln*)c->dRcAln.p;
		u32* u = c->dRcU32.p;
		u32* dOrd = u;							u += nKept;
		S.score = (i32*)u;						u += nKept;
		S.pred = u;								u += nKept;
		S.first = u;							u += nKept;
		S.depth = u;							u += nKept;
		S.active = u;							u += nKept;
		S.frozen = u;							u += nKept;
		S.accChain = u;							u += nKept;
		S.accBegin = (i32*)u;					u += nKept;
		S.accEnd = (i32*)u;						u += nKept;
		S.accAlnAt = u;							u += nKept;
		S.accCnt = u;							u += n;
		S.accAlns = u;
		{
			ScopedK t(c->timer, "k_rc_filter");
			hipLaunchKernelGGL(k_rc_filter<true>, waves, 64, 0, s, dTab, dQOff, n, p.long_edge, p.big_alignment, (u64*)nullptr,
							   dSeg, c->dRcKeys.p, c->dRcVals.p, dOrd);
		}
		fgSortSegments(c, dSeg, n, c->dRcKeys.p, c->dRcVals.p, nKept);
		{
			ScopedK t(c->timer, "k_rc_gather");
			hipLaunchKernelGGL(k_rc_gather, (unsigned)std::min<u64>((nKept + RC_BLOCK - 1) / RC_BLOCK, 4096), RC_BLOCK, 0, s, dTab, dQOff,
							   dSeg, n, nKept, c->dRcVals.p, dOrd, dNodeL, dNodeR, nExt, S.aln);
		}
		{
			ScopedK t(c->timer, "k_rc_chain");
			hipLaunchKernelGGL(k_rc_chain, waves, 64, 0, s, S, n, p.max_jump, p.max_read_overlap, c->dRcKeys.p, c->dRcVals.p);
		}
		fgSortSegments(c, dSeg, n, c->dRcKeys.p, c->dRcVals.p, nKept);
		{
			ScopedK t(c->timer, "k_rc_select");
			hipLaunchKernelGGL(k_rc_select, waves, 64, 0, s, S, n, p.min_alignment, p.max_separation, c->dRcVals.p);
		}
		HIP_CHECK(hipGetLastError());
		hCnt.resize(2 * (size_t)n);
		HIP_CHECK(hipMemcpyAsync(hCnt.data(), S.accCnt, 2 * (size_t)n * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		at.assign(2 * ((size_t)n + 1), 0);
		u64* chainAt = at.data();
		u64* alnAt = chainAt + (n + 1);
		for (u32 i = 0; i < n; ++i)
		{
			chainAt[i + 1] = chainAt[i] + hCnt[i];
			alnAt[i + 1] = alnAt[i] + hCnt[n + i];
		}
		const u64 nChains = chainAt[n], nAlns = alnAt[n];
		if (nAlns > nKept || nChains > nAlns) throw FgError{FG_ERR_HIP, "internal: fg_chain_alignments accepted more than it kept"};
		const u64 chain0 = chainOff[qa], aln0 = aln.size();
		for (u32 i = 0; i < n; ++i) chainOff[qa + i + 1] = chain0 + chainAt[i + 1];
		if (nChains)
		{
			c->dRcOut.reserve(nChains + nAlns);
			c->dRcOutScore.reserve(nChains);
			HIP_CHECK(hipMemcpyAsync(dChainAt, at.data(), at.size() * 8, hipMemcpyHostToDevice, s));	// dAlnAt follows it
			{
				ScopedK t(c->timer, "k_rc_write");
				hipLaunchKernelGGL(k_rc_write, waves, 64, 0, s, S, n, dChainAt, dAlnAt, recBase + r0, c->dRcOut.p, c->dRcOut.p + nChains,
								   c->dRcOutScore.p);
			}
			HIP_CHECK(hipGetLastError());
			hOutOff.resize(nChains); hOutAln.resize(nAlns); hOutScore.resize(nChains);
			HIP_CHECK(hipMemcpyAsync(hOutOff.data(), c->dRcOut.p, nChains * 8, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipMemcpyAsync(hOutAln.data(), c->dRcOut.p + nChains, nAlns * 8, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipMemcpyAsync(hOutScore.data(), c->dRcOutScore.p, nChains * 4, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipStreamSynchronize(s));
			alnOff.pop_back();
			for (u64 k = 0; k < nChains; ++k) alnOff.push_back(aln0 + hOutOff[k]);
			alnOff.push_back(aln0 + nAlns);
			aln.insert(aln.end(), hOutAln.begin(), hOutAln.end());
			score.insert(score.end(), hOutScore.begin(), hOutScore.end());
		}
		qa = qb;
	}
	c->timer.collect();
}
