// shift_gaps of the reference (flye/polishing/alignment.py:68-92) on the device, shared by fg_make_bubbles
// (fg_bubbles.hip) and fg_contig_consensus (fg_contigcons.hip): one wave per alignment copies the second string, finds
// its gap runs by ballots over 64 columns and closes them left to right against the first string.
#pragma once
#include "fg_ctx.h"

namespace {		// kernels of a header shared by several translation units: one internal copy each

#define BUB_BLOCK 256
#define BUB_WAVES (BUB_BLOCK / 64)

// inProfile: the alignment takes part in the profile (only those are shifted)
struct BubAln { u64 colOff; u32 nCols; i32 trgStart; i32 trgEnd; u32 contig; u32 inProfile; u32 pad; };

__device__ __forceinline__ void bub_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }
__device__ __forceinline__ u64 bub_below(int lane) { return lane == 0 ? 0ULL : (~0ULL >> (64 - lane)); }

// close the gap run [a, b) of `out` against `first` (alignment.py:78-86)
__device__ __forceinline__ void bub_close_run(const unsigned char* __restrict__ first, unsigned char* out, long long a, long long b, int lane)
{
	const long long lim = (b - a) < a ? (b - a) : a;
	long long m = lim;
	for (long long k0 = 0; k0 < lim; k0 += 64)
	{
		const long long k = k0 + lane;
		const bool neq = k < lim && out[a - 1 - k] != first[b - 1 - k];
		const u64 bal = __ballot(neq);
		if (bal) { m = k0 + (__ffsll((unsigned long long)bal) - 1); break; }
	}
	if (m == 0) return;
	for (long long k = lane; k < m; k += 64)
	{
		const unsigned char ch = out[a - 1 - k];
		out[b - 1 - k] = ch;
		out[a - 1 - k] = '-';
	}
	bub_fence();
}

// out = shift_gaps(first, second); only profiled alignments are shifted
__global__ void __launch_bounds__(BUB_BLOCK)
k_bub_shift(const BubAln* __restrict__ alns, u32 nAln, const unsigned char* first, const unsigned char* second, unsigned char* out)
{
	const int lane = threadIdx.x & 63;
	const u32 a = blockIdx.x * BUB_WAVES + (threadIdx.x >> 6);
	if (a >= nAln) return;
	const BubAln al = alns[a];
	if (!al.inProfile) return;
	const long long n = al.nCols;
	const unsigned char* f = first + al.colOff;
	const unsigned char* sIn = second + al.colOff;
	unsigned char* o = out + al.colOff;
	for (long long i = lane; i < n; i += 64) o[i] = sIn[i];
	bub_fence();
	bool inGap = false;
	long long gapStart = 0;
	for (long long c0 = 0; c0 < n; c0 += 64)
	{
		const long long i = c0 + lane;
		// bytes at or behind the scan point are never moved by an earlier run, so the input tells the gaps
		const bool valid = i < n;
		const u64 vm = __ballot(valid);
		const u64 gm = __ballot(valid && sIn[i] == '-');
		int p = 0;
		while (p < 64)
		{
			const u64 from = ~0ULL << p;
			if (inGap)
			{
				const u64 nz = ~gm & vm & from;
				if (!nz) break;
				const int bit = __ffsll((unsigned long long)nz) - 1;
				bub_close_run(f, o, gapStart, c0 + bit, lane);
				inGap = false;
				p = bit + 1;
			}
			else
			{
				const u64 g = gm & from;
				if (!g) break;
				const int bit = __ffsll((unsigned long long)g) - 1;
				gapStart = c0 + bit;
				inGap = true;
				p = bit + 1;
			}
		}
	}
	// the right sentinel closes a run that reaches the end
	if (inGap) bub_close_run(f, o, gapStart, n, lane);
}

inline unsigned bubGrid(u64 n) { return (unsigned)((n + BUB_BLOCK - 1) / BUB_BLOCK); }
inline unsigned bubWaveGrid(u64 n) { return (unsigned)((n + BUB_WAVES - 1) / BUB_WAVES); }

} // namespace
