// The second half of checkIdyAndTrim (reference src/sequence/alignment.cpp:330-457) on the device, for the runs
// fg_align_ranges' decode step leaves there: prefix sums over a pair's runs, the search for the intervals of runs
// that begin and end on a '=' run and pass the divergence gate, their std::sort by realLen, the greedy selection of
// a non-intersecting set, the mapping back through the homopolymer offset table and the minOverlap filter.
//
//   k_trim_prefix    sumCurLen / sumExtLen / sumErrors (:330-354) and the number of '=' runs before each run
//   k_trim_count     good intervals per (pair, interval length): one wave per row of the enumeration of :366-385
//   k_trim_emit      the same walk once more, writing (key, rank, interval) at the row's offset in enumeration order
//   (fgSortSegments) std::sort's permutation per pair (:389; the comparator looks at realLen alone)
//   k_trim_select    :393-409, 64 sorted candidates at a time against a bitmap of the covered runs
//   k_trim_map       :414-446 for one (accepted interval, side): positions from the prefix sums, the offset table
//                    entry by a rank-select over the range
//   k_trim_compact   :451-456, per pair, in order
//
// Floats: the gate float(rangeErr) / rangeLen < maxDivergence is evaluated here with a correctly rounded division
// of the two converted integers (what the host's division gives); the float a record carries is made by the host
// shim from the two integers.
#include "fg_ctx.h"
#include "fg_stage.h"
#include "fg_devprim.h"

namespace {

// runs a pair may have: one bit per run in one wave's LDS (k_trim_select)
#define TRIM_BM_WORDS 2048
#define TRIM_MAX_RUNS (TRIM_BM_WORDS * 64)
// device bytes a good interval costs while its sub-batch is worked on: key 8 + rank 4 + interval 8 + the sort's
// scratch (8) and task lists
#define TRIM_BYTES_PER_INTERVAL 32ULL

struct TrimRuns {
	const u64* off;			// count + 1 run offsets of the ksw sub-batch
	u32 count;
	const uint8_t* ops;
	const i32* lens;
	const i32* pre;			// four arrays of preStride entries: cur, ext, err, '=' runs; pair p's at off[p] + p
	u64 preStride;
};

__device__ __forceinline__ i32 wave_incl(i32 v, int lane)
{
	for (int o = 1; o < 64; o <<= 1)
	{
		const i32 t = __shfl_up(v, o);
		if (lane >= o) v += t;
	}
	return v;
}

// the p < n with off[p] <= g < off[p + 1] (off[0] = 0 <= g < off[n])
__device__ __forceinline__ u32 seg_of(const u64* __restrict__ off, u32 n, u64 g)
{
	u32 lo = 0, hi = n;
	while (hi - lo > 1)
	{
		const u32 mid = (lo + hi) >> 1;
		if (off[mid] <= g) lo = mid; else hi = mid;
	}
	return lo;
}

__global__ void __launch_bounds__(64)
k_trim_prefix(TrimRuns T, i32* __restrict__ pre)
{
	const int lane = threadIdx.x;
	for (u32 p = blockIdx.x; p < T.count; p += gridDim.x)
	{
		const u64 base = fg_uni(T.off[p]);
		const i32 n = (i32)(fg_uni(T.off[p + 1]) - base);
		i32* sc = pre + base + p;
		i32* se = sc + T.preStride;
		i32* sr = se + T.preStride;
		i32* sq = sr + T.preStride;
		if (lane == 0) { sc[0] = 0; se[0] = 0; sr[0] = 0; sq[0] = 0; }
		i32 cc = 0, ce = 0, cr = 0, cq = 0;
		for (i32 k0 = 0; k0 < n; k0 += 64)
		{
			const i32 k = k0 + lane;
			const bool valid = k < n;
			const uint8_t op = valid ? T.ops[base + k] : (uint8_t)'=';
			const i32 len = valid ? T.lens[base + k] : 0;
			const i32 vc = wave_incl(op == 'I' ? 0 : len, lane) + cc;
			const i32 ve = wave_incl(op == 'D' ? 0 : len, lane) + ce;
			const i32 vr = wave_incl(op != '=' ? len : 0, lane) + cr;
			const i32 vq = wave_incl(valid && op == '=' ? 1 : 0, lane) + cq;
			if (valid) { sc[k + 1] = vc; se[k + 1] = ve; sr[k + 1] = vr; sq[k + 1] = vq; }
			cc = __shfl(vc, 63); ce = __shfl(ve, 63); cr = __shfl(vr, 63); cq = __shfl(vq, 63);
		}
	}
}

// One wave per row g of [g0, g1): row r of pair p holds the intervals of n - r runs (the enumeration of :366-385
// takes the lengths in descending order), starts 0 .. r.  EMIT = false: rowCnt[g] = its good intervals, added to
// pairCnt[p].  EMIT = true: the good intervals at rowOff[g - g0] (+ their rank in the row, from the ballots) of the
// sub-batch's arrays: key = 2^32 - realLen (ascending = realLen descending), val = the position in the pair's list,
// ivl = start | end << 32.
template <bool EMIT>
__global__ void __launch_bounds__(64)
k_trim_rows(TrimRuns T, u64 g0, u64 g1, float maxDivergence, u64* __restrict__ rowCnt, unsigned long long* __restrict__ pairCnt,
			const u64* __restrict__ rowOff, const u64* __restrict__ seg, u32 pairFirst, u64 nGood, u64* __restrict__ keys,
			u32* __restrict__ vals, u64* __restrict__ ivl)
{
	const int lane = threadIdx.x;
	for (u64 g = g0 + blockIdx.x; g < g1; g += gridDim.x)
	{
		const u32 p = fg_uni(seg_of(T.off, T.count, g));
		const u64 base = fg_uni(T.off[p]);
		const i32 n = (i32)(fg_uni(T.off[p + 1]) - base);
		const i32 r = (i32)(g - base);
		const i32 L = n - r;
		const i32* sc = T.pre + base + p;
		const i32* se = sc + T.preStride;
		const i32* sr = se + T.preStride;
		const uint8_t* ops = T.ops + base;
		u64 cnt = 0;
		u64 dst = 0, segAt = 0;
		if (EMIT) { dst = fg_uni(rowOff[g - g0]); segAt = fg_uni(seg[p - pairFirst]); }
		for (i32 s0 = 0; s0 <= r; s0 += 64)
		{
			const i32 i = s0 + lane, j = i + L - 1;
			bool ok = i <= r && ops[i] == '=' && ops[j] == '=';
			i32 realLen = 1;
			if (ok)
			{
				const i32 lc = sc[j + 1] - sc[i], le = se[j + 1] - se[i];
				realLen = lc > le ? lc : le;
				const i32 err = sr[j + 1] - sr[i];
				ok = __fdiv_rn((float)err, (float)realLen) < maxDivergence;
			}
			const u64 m = __builtin_amdgcn_ballot_w64(ok);
			if (EMIT && ok)
			{
				const u64 idx = dst + cnt + (u64)__builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0));
				if (idx < nGood)
				{
					keys[idx] = (1ULL << 32) - (u64)(u32)realLen;
					vals[idx] = (u32)(idx - segAt);
					ivl[idx] = (u64)(u32)i | ((u64)(u32)j << 32);
				}
			}
			cnt += (u64)__popcll(m);
		}
		if (!EMIT && lane == 0)
		{
			rowCnt[g] = cnt;
			if (cnt) atomicAdd(&pairCnt[p], (unsigned long long)cnt);
		}
	}
}

// The greedy pass over a pair's sorted list (:393-409), one wave per pair of [pairFirst, pairEnd).  The accepted
// intervals are disjoint, so "intersects an accepted one" = "covers a run that is covered": a bitmap of the covered
// runs in LDS.  64 candidates are screened against it; the first survivor is accepted, the later survivors of the
// block are screened against that one interval, and so on.  Every interval begins on a '=' run: once all of them are
// covered nothing more can be accepted.  acc[off[p] + k] = the k-th accepted interval, accCnt[p] their number.
__global__ void __launch_bounds__(64)
k_trim_select(TrimRuns T, u32 pairFirst, u32 pairEnd, const u64* __restrict__ seg, u64 nGood, const u32* __restrict__ vals,
			  const u64* __restrict__ ivl, u64* __restrict__ acc, u32* __restrict__ accCnt)
{
	__shared__ u64 bm[TRIM_BM_WORDS];
	const int lane = threadIdx.x;
	for (u32 p = pairFirst + blockIdx.x; p < pairEnd; p += gridDim.x)
	{
		const u64 base = fg_uni(T.off[p]);
		const i32 n = (i32)(fg_uni(T.off[p + 1]) - base);
		const u64 a = fg_uni(seg[p - pairFirst]), b = fg_uni(seg[p - pairFirst + 1]);
		u32 nAcc = 0;
		if (n > 0 && n <= TRIM_MAX_RUNS && b > a)
		{
			const i32* sq = T.pre + base + p + 3 * T.preStride;
			const i32 nEq = fg_uni(sq[n]);
			for (i32 w = lane; w < (n + 63) / 64; w += 64) bm[w] = 0;
			__syncthreads();
			i32 covered = 0;
			for (u64 c0 = a; c0 < b && covered < nEq; c0 += 64)
			{
				const u64 cIdx = c0 + lane;
				bool valid = cIdx < b && cIdx < nGood;
				i32 s = 0, e = 0;
				if (valid)
				{
					const u64 at = a + vals[cIdx];
					valid = at < b && at < nGood;
					if (valid) { const u64 iv = ivl[at]; s = (i32)(u32)iv; e = (i32)(iv >> 32); }
					valid = valid && s >= 0 && e >= s && e < n;
				}
				bool hit = false;
				if (valid)
					for (i32 w = s >> 6; w <= (e >> 6) && !hit; ++w)
					{
						u64 mask = ~0ULL;
						if (w == (s >> 6)) mask &= ~0ULL << (s & 63);
						if (w == (e >> 6)) mask &= ~0ULL >> (63 - (e & 63));
						hit = (bm[w] & mask) != 0;
					}
				u64 surv = __builtin_amdgcn_ballot_w64(valid && !hit);
				while (surv)
				{
					const int f = __builtin_ctzll(surv);
					const i32 as = __shfl(s, f), ae = __shfl(e, f);
					if (lane == 0 && nAcc < (u32)n) acc[base + nAcc] = (u64)(u32)as | ((u64)(u32)ae << 32);
					++nAcc;
					covered += sq[ae + 1] - sq[as];
					for (i32 w = (as >> 6) + lane; w <= (ae >> 6); w += 64)
					{
						u64 mask = ~0ULL;
						if (w == (as >> 6)) mask &= ~0ULL << (as & 63);
						if (w == (ae >> 6)) mask &= ~0ULL >> (63 - (ae & 63));
						bm[w] |= mask;
					}
					const bool later = ((surv >> lane) & 1ULL) && lane > f;
					const bool ov = (e < ae ? e : ae) - (s > as ? s : as) >= 0;
					surv = __builtin_amdgcn_ballot_w64(later && !ov);
					__syncthreads();	// one wave: keeps the bitmap's stores ahead of the loads that follow
				}
			}
		}
		const u32 room = n > 0 ? (u32)n : 0u;
		if (lane == 0) accCnt[p] = nAcc < room ? nAcc : room;
		__syncthreads();
	}
}

struct TrimSeqs {
	const u64* qWords; const u64* qWordOff; const i32* qLen;
	const u64* words; const u64* wordOff; const i32* len;
};

// One wave per (record, side): record t >> 1 is accepted interval k of pair p (accOff: count + 1 offsets), side 0 =
// cur, 1 = ext.  posTrg / posQry at the interval's first run and behind its last one come from the prefix sums
// (:418-446); the offset table entry of kept base number x is the position of the x-th kept base of the range, found
// by walking the range 64 bases per step and ranking the ballot of the kept ones.
__global__ void __launch_bounds__(64)
k_trim_map(TrimRuns T, const u64* __restrict__ accOff, const u64* __restrict__ acc, const FgRangeSide* __restrict__ sides,
		   TrimSeqs S, int hpc, fg_trim_rec* __restrict__ raw)
{
	const int lane = threadIdx.x;
	const u64 nTasks = 2 * fg_uni(accOff[T.count]);
	for (u64 t = blockIdx.x; t < nTasks; t += gridDim.x)
	{
		const u64 rec = t >> 1;
		const u32 side = (u32)(t & 1);
		const u32 p = fg_uni(seg_of(accOff, T.count, rec));
		const u64 base = fg_uni(T.off[p]);
		const u64 iv = fg_uni(acc[base + (rec - fg_uni(accOff[p]))]);
		const i32 s = (i32)(u32)iv, e = (i32)(iv >> 32);
		const i32* sc = T.pre + base + p;
		const i32* se = sc + T.preStride;
		const i32* sr = se + T.preStride;
		const i32* sp = side ? se : sc;
		const i32 posB = fg_uni(sp[s]), posE = fg_uni(sp[e + 1]) - 1;
		const FgRangeSide R = sides[2 * (size_t)p + side];
		i32 offB = posB, offE = posE;
		if (hpc)
		{
			const bool q = R.flags & 2u;
			const u64* w = (q ? S.qWords : S.words) + (q ? S.qWordOff : S.wordOff)[R.rec];
			const i32 L = (q ? S.qLen : S.len)[R.rec];
			u32 carry = 4;
			i32 at = 0;
			offB = offE = 0;
			for (i32 t0 = 0; t0 < R.len && at <= posE; t0 += 64)
			{
				u32 b; bool keep;
				const u64 m = fg_range_step(w, L, R.flags & 1u, R.start, R.len, true, t0, carry, b, keep);
				const i32 rank = at + (i32)__builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0));
				const u64 mb = __builtin_amdgcn_ballot_w64(keep && rank == posB);
				const u64 me = __builtin_amdgcn_ballot_w64(keep && rank == posE);
				if (mb) offB = t0 + __builtin_ctzll(mb);
				if (me) offE = t0 + __builtin_ctzll(me);
				at += __popcll(m);
			}
		}
		if (lane == 0)
		{
			fg_trim_rec& o = raw[rec];
			if (side == 0)
			{
				o.cur_begin = R.start + offB; o.cur_end = R.start + offE;
				o.run_start = s; o.run_end = e;
				const i32 lc = sc[e + 1] - sc[s], le = se[e + 1] - se[s];
				o.range_len = lc > le ? lc : le;
				o.range_err = sr[e + 1] - sr[s];
				o.seq_divergence = 0.0f;
			}
			else { o.ext_begin = R.start + offB; o.ext_end = R.start + offE; }
		}
	}
}

// the minOverlap test (:451-452, both ranges strictly greater) and the compaction of each pair's records, in order:
// kept[p] records at out[accOff[p] ..)
__global__ void __launch_bounds__(64)
k_trim_compact(const u64* __restrict__ accOff, u32 count, i32 minOverlap, const fg_trim_rec* __restrict__ raw,
			   fg_trim_rec* __restrict__ out, u32* __restrict__ kept)
{
	const int lane = threadIdx.x;
	for (u32 p = blockIdx.x; p < count; p += gridDim.x)
	{
		const u64 a = fg_uni(accOff[p]), b = fg_uni(accOff[p + 1]);
		u32 w = 0;
		for (u64 k0 = a; k0 < b; k0 += 64)
		{
			const u64 k = k0 + lane;
			fg_trim_rec r{};
			bool keep = false;
			if (k < b)
			{
				r = raw[k];
				keep = r.cur_end - r.cur_begin > minOverlap && r.ext_end - r.ext_begin > minOverlap;
			}
			const u64 m = __builtin_amdgcn_ballot_w64(keep);
			if (keep) out[a + w + __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0))] = r;
			w += (u32)__popcll(m);
		}
		if (lane == 0) kept[p] = w;
	}
}

} // namespace

void fgTrimRanges(fg_ctx* c, const std::vector<FgRangeSide>& sides, bool useHpc, float maxDivergence, i32 minOverlap,
				  std::vector<u64>& recOff, std::vector<fg_trim_rec>& recs)
{
	hipStream_t s = c->stream;
	const u32 nPairs = (u32)(sides.size() / 2);
	recOff.assign(nPairs + 1, 0);
	recs.clear();
	if (!nPairs) return;
	c->timer.reset();
	const u64 budget = stageEnvU64("FG_TRIM_SCRATCH_BYTES", 1ULL << 30);
	const bool trace = getenv("FG_TRIM_TRACE") != nullptr;
	const TrimSeqs S{c->dQWords.p, c->dQWordOff.p, c->dQLen.p, c->dWords.p, c->dWordOff.p, c->dLen.p};
	std::vector<u32> keptAll(nPairs, 0);
	std::vector<u64> runOff;
	std::vector<u32> errBases;
	std::vector<i32> lenCur, lenExt;
	fgAlignRangesDevice(c, sides, useHpc, runOff, errBases, lenCur, lenExt, [&](const FgDecodedRuns& D)
	{
		const u32 n = D.count;
		const u64 nOut = D.nOut, nPre = nOut + n;
		for (u32 i = 0; i < n; ++i)
			if (D.off[i + 1] - D.off[i] > (u64)TRIM_MAX_RUNS)
				throw FgError{FG_ERR_NOMEM, "fg_trim_ranges: pair " + std::to_string(D.first + i) + " has " + std::to_string(D.off[i + 1] - D.off[i]) +
											" runs, more than the " + std::to_string(TRIM_MAX_RUNS) + " the selection pass holds a bit for"};
		c->dTrimPre.reserve(4 * nPre); c->dTrimRowCnt.reserve(nOut); c->dTrimRowOff.reserve(nOut);
		c->dTrimPairCnt.reserve(n); c->dTrimAcc.reserve(nOut); c->dTrimAccCnt.reserve(n);
		c->dTrimSeg.reserve((size_t)n + 1); c->dTrimAccOff.reserve((size_t)n + 1); c->dTrimKept.reserve(n);
		HIP_CHECK(hipMemsetAsync(c->dTrimPairCnt.p, 0, (size_t)n * 8, s));
		const TrimRuns T{c->dDecOff.p, n, c->dDecOps.p, c->dDecLens.p, c->dTrimPre.p, nPre};
		{
			ScopedK t(c->timer, "k_trim_prefix");
			hipLaunchKernelGGL(k_trim_prefix, std::min<unsigned>(n, 8192u), 64, 0, s, T, c->dTrimPre.p);
		}
		{
			ScopedK t(c->timer, "k_trim_count");
			hipLaunchKernelGGL(k_trim_rows<false>, (unsigned)std::min<u64>(nOut, 1u << 18), 64, 0, s, T, (u64)0, nOut, maxDivergence,
							   c->dTrimRowCnt.p, c->dTrimPairCnt.p, (const u64*)nullptr, (const u64*)nullptr, 0u, (u64)0, (u64*)nullptr,
							   (u32*)nullptr, (u64*)nullptr);
		}
		std::vector<unsigned long long> hCnt(n);
		HIP_CHECK(hipMemcpyAsync(hCnt.data(), c->dTrimPairCnt.p, (size_t)n * 8, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		// steps 2 to 4 in sub-batches of pairs whose good intervals fit the budget (a pair beyond it runs alone)
		u32 a = 0;
		while (a < n)
		{
			u32 b = a;
			u64 nGood = 0;
			while (b < n && (b == a || (nGood + hCnt[b]) * TRIM_BYTES_PER_INTERVAL <= budget))
			{
				if (hCnt[b] > 0xFFFFFFFFULL)
					throw FgError{FG_ERR_NOMEM, "fg_trim_ranges: pair " + std::to_string(D.first + b) + " has more than 2^32 - 1 intervals below the gate"};
				nGood += hCnt[b]; ++b;
			}
			std::vector<u64> seg(b - a + 1, 0);
			for (u32 i = a; i < b; ++i) seg[i - a + 1] = seg[i - a] + hCnt[i];
			HIP_CHECK(hipMemcpyAsync(c->dTrimSeg.p, seg.data(), seg.size() * 8, hipMemcpyHostToDevice, s));
			const u64 g0 = D.off[a], g1 = D.off[b];
			if (nGood)
			{
				c->dTrimKeys.reserve(nGood); c->dTrimVals.reserve(nGood); c->dTrimIvl.reserve(nGood);
				c->dTrimScan.reserve(fgprim::scanScratchElems(g1 - g0));
				{
					ScopedK t(c->timer, "k_trim_emit");
					fgprim::scan<u64>(s, c->dTrimRowCnt.p + g0, c->dTrimRowOff.p, g1 - g0, false, c->dTrimScan.p);
					hipLaunchKernelGGL(k_trim_rows<true>, (unsigned)std::min<u64>(g1 - g0, 1u << 18), 64, 0, s, T, g0, g1, maxDivergence,
									   (u64*)nullptr, (unsigned long long*)nullptr, c->dTrimRowOff.p, c->dTrimSeg.p, a, nGood, c->dTrimKeys.p,
									   c->dTrimVals.p, c->dTrimIvl.p);
				}
				fgSortSegments(c, c->dTrimSeg.p, b - a, c->dTrimKeys.p, c->dTrimVals.p, nGood);
			}
			{
				ScopedK t(c->timer, "k_trim_select");
				hipLaunchKernelGGL(k_trim_select, std::min<unsigned>(b - a, 8192u), 64, 0, s, T, a, b, c->dTrimSeg.p, nGood, c->dTrimVals.p,
								   c->dTrimIvl.p, c->dTrimAcc.p, c->dTrimAccCnt.p);
			}
			HIP_CHECK(hipStreamSynchronize(s));		// seg goes out of scope; the next sub-batch reuses the arrays
			if (trace) fprintf(stderr, "[trim] pairs %u..%u of the ksw sub-batch: %llu good intervals\n", a, b, (unsigned long long)nGood);
			a = b;
		}
		std::vector<u32> hAcc(n);
		HIP_CHECK(hipMemcpyAsync(hAcc.data(), c->dTrimAccCnt.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		std::vector<u64> accOff(n + 1, 0);
		for (u32 i = 0; i < n; ++i) accOff[i + 1] = accOff[i] + hAcc[i];
		const u64 nRec = accOff[n];
		if (!nRec) return;
		c->dTrimRaw.reserve(nRec * sizeof(fg_trim_rec)); c->dTrimOut.reserve(nRec * sizeof(fg_trim_rec));
		HIP_CHECK(hipMemcpyAsync(c->dTrimAccOff.p, accOff.data(), accOff.size() * 8, hipMemcpyHostToDevice, s));
		{
			ScopedK t(c->timer, "k_trim_map");
			hipLaunchKernelGGL(k_trim_map, (unsigned)std::min<u64>(2 * nRec, 1u << 18), 64, 0, s, T, c->dTrimAccOff.p, c->dTrimAcc.p,
							   (const FgRangeSide*)c->dRangeSides.p + 2 * (size_t)D.first, S, useHpc ? 1 : 0, (fg_trim_rec*)c->dTrimRaw.p);
		}
		{
			ScopedK t(c->timer, "k_trim_compact");
			hipLaunchKernelGGL(k_trim_compact, std::min<unsigned>(n, 8192u), 64, 0, s, c->dTrimAccOff.p, n, minOverlap,
							   (const fg_trim_rec*)c->dTrimRaw.p, (fg_trim_rec*)c->dTrimOut.p, c->dTrimKept.p);
		}
		std::vector<fg_trim_rec> hOut(nRec);
		HIP_CHECK(hipMemcpyAsync(keptAll.data() + D.first, c->dTrimKept.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipMemcpyAsync(hOut.data(), c->dTrimOut.p, nRec * sizeof(fg_trim_rec), hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		for (u32 i = 0; i < n; ++i)
			recs.insert(recs.end(), hOut.begin() + accOff[i], hOut.begin() + accOff[i] + keptAll[D.first + i]);
	});
	for (u32 i = 0; i < nPairs; ++i) recOff[i + 1] = recOff[i] + keptAll[i];
	c->timer.collect();
}
