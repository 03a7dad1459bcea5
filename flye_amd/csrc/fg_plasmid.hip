// fg_paf_groups / fg_paf_circular / fg_components / fg_paf_parse: the passes of the short-plasmid rescue
// (reference flye/short_plasmids/, called from flye/main.py after the contigger) over the hits of a PAF file.
//   groups     read_paf_grouped (flye/utils/sam_parser.py:102-120): the hits of one (run, target), runs in file order,
//              targets ascending inside a run, and per group what unite_mapping_segments / calc_mapping_rate
//              (unmapped_reads.py:27-48) sum on either side before the division
//   circular   extract_circular_reads (circular_sequences.py:17-44) and the per-group search of extract_circular_pairs
//              (:87-111)
//   components find_connected_components (utils.py:7-29) as labels
// Integers only; every float, the greedy used_reads filter and the FASTA slices stay with the caller.
//
//   k_paf_run_flag   one thread per hit: 1 where the query differs from the hit before; (scan) -> the hit's run
//   k_paf_keys       one thread per hit: key = run << bits(target) | target, value = hit index
//   (fgprim::radixSortPairs over the bits in use: stable, so a group keeps file order)
//   k_paf_group_flag one thread per sorted hit: 1 where the key differs from the one before; (scan) -> the hit's group
//   k_paf_group_out  order, group_off, group_query, group_target
//   k_paf_cover      one block per group, 64 threads up to FG_PAF_WAVE_MAX hits, 256 up to FG_PAF_WG_MAX: both sides'
//                    (start, end) in LDS; thread i takes M_i = the largest end among the segments that sort before
//                    segment i by (start, position) straight from LDS (every lane reads the same word: a broadcast),
//                    adds max(0, end_i - max(M_i, start_i - 1)); block sum.  s^2 / threads steps and no sort: a group
//                    of the bulk (a read on a contig: 1 - 3 hits) costs a few steps.
//   flat route, groups above FG_PAF_WG_MAX, per side:
//   k_paf_flat_fill  key = group << 31 | start, value = end, the groups side by side
//   (fgprim::radixSortPairs by (group, start))
//   k_paf_flat_scan  one block per tile of FG_PAF_TILE sorted segments: the running maximum of the ends inside the
//                    tile, restarted where the group changes (Hillis-Steele steps in LDS; the groups ascend, so
//                    "same group d places back" covers the whole stretch), and the tile's first group, last group
//                    and the maximum of its last group
//   k_paf_flat_carry one thread, tile after tile: the maximum a tile's first group brings in from the tiles before (a
//                    tile of one group hands its own carry on: the carry crosses whole tiles)
//   k_paf_flat_sum   one thread per segment: M_i from the running maximum before it and the carry, the segment's
//                    bases; a wave that lies inside one group adds them up first, then one 64-bit integer atomic
//   k_paf_circ_*     per query id, over the file: an atomic maximum of (length << 32 | ~hit index) keeps the first
//                    longest circular hit, an atomic minimum the first circular hit; flag + scan lists the queries by it
//   k_paf_pair_*     per group: atomic minima of the sorted position of the first hit with A, then of the first other
//                    hit with B; then the intersection test
//   k_cc_hook / k_cc_jump   fg_components, see include/flye_gpu.h
// Every atomic is an integer minimum, maximum or sum: the results do not depend on the order of arrival.
#include "fg_ctx.h"
#include "fg_stage.h"
#include "fg_devprim.h"

namespace {

#define PAF_BLOCK 256
#define PAF_WAVE_CAP 64			// hits of a group of the 64-thread class (4 arrays of 256 B)
#define PAF_WG_CAP 1024			// ... of the 256-thread class (4 arrays of 4 KiB)
#define PAF_TILE_CAP 1024		// segments of a tile of the flat route
#define PAF_MAX_BLOCKS 16384u
#define PAF_NONE 0xFFFFFFFFu
#define PAF_START_BITS 31		// 0 <= start < 2^31

unsigned pafGrid(u64 n) { return (unsigned)std::min<u64>(std::max<u64>((n + PAF_BLOCK - 1) / PAF_BLOCK, 1), 4096); }

int pafBits(u64 maxValue)
{
	int b = 0;
	while (b < 64 && (maxValue >> b)) ++b;
	return b;
}

__global__ void __launch_bounds__(PAF_BLOCK) k_paf_run_flag(const fg_paf_hit* __restrict__ hits, u64 n, u32* __restrict__ flag)
{
	for (u64 i = (u64)blockIdx.x * PAF_BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * PAF_BLOCK)
		flag[i] = i > 0 && hits[i].query != hits[i - 1].query ? 1u : 0u;
}

__global__ void __launch_bounds__(PAF_BLOCK)
k_paf_keys(const fg_paf_hit* __restrict__ hits, const u32* __restrict__ run, u64 n, int targetBits, u64* __restrict__ keys,
		   u64* __restrict__ vals)
{
	for (u64 i = (u64)blockIdx.x * PAF_BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * PAF_BLOCK)
	{
		keys[i] = ((u64)run[i] << targetBits) | hits[i].target;
		vals[i] = i;
	}
}

__global__ void __launch_bounds__(PAF_BLOCK) k_paf_group_flag(const u64* __restrict__ keys, u64 n, u32* __restrict__ flag)
{
	for (u64 j = (u64)blockIdx.x * PAF_BLOCK + threadIdx.x; j < n; j += (u64)gridDim.x * PAF_BLOCK)
		flag[j] = j > 0 && keys[j] != keys[j - 1] ? 1u : 0u;
}

// gid: the group of every sorted hit; groupOff has one entry more than there are groups
__global__ void __launch_bounds__(PAF_BLOCK)
k_paf_group_out(const fg_paf_hit* __restrict__ hits, const u64* __restrict__ vals, const u32* __restrict__ gid, u64 n,
				u32* __restrict__ order, u64* __restrict__ groupOff, u32* __restrict__ groupQuery, u32* __restrict__ groupTarget)
{
	for (u64 j = (u64)blockIdx.x * PAF_BLOCK + threadIdx.x; j < n; j += (u64)gridDim.x * PAF_BLOCK)
	{
		const u32 h = (u32)vals[j], g = gid[j];
		order[j] = h;
		if (j == 0 || gid[j - 1] != g)
		{
			groupOff[g] = j;
			groupQuery[g] = hits[h].query;
			groupTarget[g] = hits[h].target;
		}
		if (j == n - 1) groupOff[(u64)g + 1] = n;
	}
}

__device__ __forceinline__ long long paf_shfl_xor(long long v, int o)
{
	const u32 lo = __shfl_xor((u32)v, o), hi = __shfl_xor((u32)((u64)v >> 32), o);
	return (long long)(((u64)hi << 32) | lo);
}

// the sum over the block, to every thread; sh: NT / 64 entries, reused after the barrier
template <int NT>
__device__ __forceinline__ long long paf_block_sum(long long v, long long* sh)
{
	for (int o = 32; o > 0; o >>= 1) v += paf_shfl_xor(v, o);
	if (NT == 64) return v;
	if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
	__syncthreads();
	long long r = 0;
	for (int w = 0; w < NT / 64; ++w) r += sh[w];
	__syncthreads();
	return r;
}

// list: the groups of this launch, each of at most CAP hits
template <int NT, int CAP>
__global__ void __launch_bounds__(NT)
k_paf_cover(const u32* __restrict__ list, u32 nList, const u64* __restrict__ groupOff, const u32* __restrict__ order,
			const fg_paf_hit* __restrict__ hits, long long* __restrict__ queryCover, long long* __restrict__ targetCover)
{
	__shared__ i32 sStart[2][CAP], sEnd[2][CAP];
	__shared__ long long sh[NT / 64];
	const int tid = threadIdx.x;
	for (u32 li = blockIdx.x; li < nList; li += gridDim.x)
	{
		const u32 g = fg_uni(list[li]);
		const u64 a = fg_uni(groupOff[g]);
		int s = (int)(fg_uni(groupOff[g + 1]) - a);
		if (s > CAP) s = CAP;						// the host lists no such group
		for (int i = tid; i < s; i += NT)
		{
			const fg_paf_hit h = hits[order[a + i]];
			sStart[0][i] = h.query_start; sEnd[0][i] = h.query_end;
			sStart[1][i] = h.target_start; sEnd[1][i] = h.target_end;
		}
		__syncthreads();
		long long mine[2] = {0, 0};
		for (int i = tid; i < s; i += NT)
			for (int side = 0; side < 2; ++side)
			{
				const i32 st = sStart[side][i], en = sEnd[side][i];
				i32 m = st - 1;						// start >= 0: "no end before" and "every end before below start" read alike
				for (int j = 0; j < s; ++j)
				{
					const i32 sj = sStart[side][j], ej = sEnd[side][j];
					if ((sj < st || (sj == st && j < i)) && ej > m) m = ej;
				}
				if (en > m) mine[side] += (long long)en - m;
			}
		const long long q = paf_block_sum<NT>(mine[0], sh);
		const long long t = paf_block_sum<NT>(mine[1], sh);
		if (tid == 0) { queryCover[g] = q; targetCover[g] = t; }
		__syncthreads();							// the arrays are read above and filled by the next group
	}
}

// list: the groups of the flat route; flatOff[li]: where the segments of list[li] start among them
__global__ void __launch_bounds__(PAF_BLOCK)
k_paf_flat_fill(const u32* __restrict__ list, u32 nList, const u64* __restrict__ flatOff, const u64* __restrict__ groupOff,
				const u32* __restrict__ order, const fg_paf_hit* __restrict__ hits, int side, u64* __restrict__ keys, u64* __restrict__ vals)
{
	for (u32 li = blockIdx.x; li < nList; li += gridDim.x)
	{
		const u32 g = fg_uni(list[li]);
		const u64 a = fg_uni(groupOff[g]), s = fg_uni(groupOff[g + 1]) - a, at = fg_uni(flatOff[li]);
		for (u64 i = threadIdx.x; i < s; i += PAF_BLOCK)
		{
			const fg_paf_hit h = hits[order[a + i]];
			keys[at + i] = ((u64)g << PAF_START_BITS) | (u32)(side ? h.target_start : h.query_start);
			vals[at + i] = (u32)(side ? h.target_end : h.query_end);
		}
	}
}

struct PafTile { u32 firstGroup, lastGroup; i32 lastMax, pad; };

// incl[i]: the largest end among the segments of i's group from the tile's begin up to i
__global__ void __launch_bounds__(PAF_BLOCK)
k_paf_flat_scan(const u64* __restrict__ keys, const u64* __restrict__ vals, u64 m, int tile, i32* __restrict__ incl,
				PafTile* __restrict__ tiles)
{
	__shared__ u32 sGroup[PAF_TILE_CAP];
	__shared__ i32 sMax[2][PAF_TILE_CAP];
	const u64 base = (u64)blockIdx.x * tile;
	const int len = (int)(m - base < (u64)tile ? m - base : (u64)tile);
	for (int i = threadIdx.x; i < len; i += PAF_BLOCK)
	{
		sGroup[i] = (u32)(keys[base + i] >> PAF_START_BITS);
		sMax[0][i] = (i32)vals[base + i];
	}
	__syncthreads();
	int cur = 0;
	for (int d = 1; d < len; d <<= 1)
	{
		for (int i = threadIdx.x; i < len; i += PAF_BLOCK)
		{
			i32 v = sMax[cur][i];
			if (i >= d && sGroup[i - d] == sGroup[i] && sMax[cur][i - d] > v) v = sMax[cur][i - d];
			sMax[cur ^ 1][i] = v;
		}
		__syncthreads();
		cur ^= 1;
	}
	for (int i = threadIdx.x; i < len; i += PAF_BLOCK) incl[base + i] = sMax[cur][i];
	if (threadIdx.x == 0) tiles[blockIdx.x] = PafTile{sGroup[0], sGroup[len - 1], sMax[cur][len - 1], 0};
}

// carry[t]: the largest end of tile t's first group in the tiles before t; -1: none
__global__ void k_paf_flat_carry(const PafTile* __restrict__ tiles, u64 nTiles, i32* __restrict__ carry)
{
	if (blockIdx.x || threadIdx.x) return;
	i32 c = -1;
	carry[0] = c;
	for (u64 t = 1; t < nTiles; ++t)
	{
		const PafTile p = tiles[t - 1];
		if (p.lastGroup != tiles[t].firstGroup) c = -1;
		else if (p.firstGroup != p.lastGroup) c = p.lastMax;
		else c = p.lastMax > c ? p.lastMax : c;			// a tile of one group hands its own carry on
		carry[t] = c;
	}
}

__global__ void __launch_bounds__(PAF_BLOCK)
k_paf_flat_sum(const u64* __restrict__ keys, const u64* __restrict__ vals, const i32* __restrict__ incl, const i32* __restrict__ carry,
			   u64 m, int tile, unsigned long long* __restrict__ cover)
{
	for (u64 base = (u64)blockIdx.x * PAF_BLOCK; base < m; base += (u64)gridDim.x * PAF_BLOCK)		// whole waves take every turn
	{
		const u64 i = base + threadIdx.x;
		const bool valid = i < m;
		const u64 k = keys[valid ? i : m - 1];
		const u32 g = (u32)(k >> PAF_START_BITS);
		long long d = 0;
		if (valid)
		{
			const i32 st = (i32)(k & ((1ULL << PAF_START_BITS) - 1)), en = (i32)vals[i];
			const u64 t = i / (u64)tile;
			i32 mx = st - 1;
			if (i % (u64)tile != 0 && (u32)(keys[i - 1] >> PAF_START_BITS) == g && incl[i - 1] > mx) mx = incl[i - 1];
			if ((u32)(keys[t * (u64)tile] >> PAF_START_BITS) == g && carry[t] > mx) mx = carry[t];
			if (en > mx) d = (long long)en - mx;
		}
		const u32 g0 = fg_uni(g);
		if (__all(g == g0))
		{
			for (int o = 32; o > 0; o >>= 1) d += paf_shfl_xor(d, o);
			if ((threadIdx.x & 63) == 0 && d) atomicAdd(&cover[g0], (unsigned long long)d);
		}
		else if (d) atomicAdd(&cover[g], (unsigned long long)d);
	}
}

// ---- circular reads -------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool paf_is_circular(const fg_paf_hit& h, i32 maxOverhang)
{
	return h.query == h.target && h.query_start < h.query_end && h.query_end < h.target_start && h.target_start < h.target_end &&
		   h.query_start < maxOverhang && (long long)h.target_len - h.target_end + 1 < (long long)maxOverhang;
}

// best[q]: length << 32 | ~index of the first longest circular hit of query q (0: none); first[q]: its first circular hit
__global__ void __launch_bounds__(PAF_BLOCK)
k_paf_circ_mark(const fg_paf_hit* __restrict__ hits, u64 n, i32 maxOverhang, unsigned long long* __restrict__ best, u32* __restrict__ first)
{
	for (u64 i = (u64)blockIdx.x * PAF_BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * PAF_BLOCK)
	{
		const fg_paf_hit h = hits[i];
		if (!paf_is_circular(h, maxOverhang)) continue;
		const u64 len = (u64)((long long)h.query_end - h.query_start + 1);
		atomicMax(&best[h.query], (unsigned long long)((len << 32) | (u64)(PAF_NONE - (u32)i)));
		atomicMin(&first[h.query], (u32)i);
	}
}

__global__ void __launch_bounds__(PAF_BLOCK)
k_paf_circ_flag(const fg_paf_hit* __restrict__ hits, u64 n, const u32* __restrict__ first, u32* __restrict__ flag)
{
	for (u64 i = (u64)blockIdx.x * PAF_BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * PAF_BLOCK)
		flag[i] = first[hits[i].query] == (u32)i ? 1u : 0u;
}

// rank: the inclusive sums of the flags
__global__ void __launch_bounds__(PAF_BLOCK)
k_paf_circ_out(const fg_paf_hit* __restrict__ hits, u64 n, const u32* __restrict__ first, const unsigned long long* __restrict__ best,
			   const u32* __restrict__ rank, u32* __restrict__ circQuery, u32* __restrict__ circHit)
{
	for (u64 i = (u64)blockIdx.x * PAF_BLOCK + threadIdx.x; i < n; i += (u64)gridDim.x * PAF_BLOCK)
	{
		const u32 q = hits[i].query;
		if (first[q] != (u32)i) continue;
		circQuery[rank[i] - 1] = q;
		circHit[rank[i] - 1] = PAF_NONE - (u32)best[q];
	}
}

// ---- circular pairs -------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool paf_pair_a(const fg_paf_hit& h, i32 ov)
{
	return (long long)h.query_len - h.query_end + 1 < (long long)ov && h.target_start < ov;
}

__device__ __forceinline__ bool paf_pair_b(const fg_paf_hit& h, i32 ov)
{
	return h.query_start < ov && (long long)h.target_len - h.target_end + 1 < (long long)ov;
}

// second == 0: posA[g] = the first sorted position of group g with A; second == 1: posB[g] = the first other one with B
__global__ void __launch_bounds__(PAF_BLOCK)
k_paf_pair_pos(const fg_paf_hit* __restrict__ hits, const u32* __restrict__ order, const u32* __restrict__ gid, u64 n, i32 ov, int second,
			   u32* __restrict__ posA, u32* __restrict__ posB)
{
	for (u64 j = (u64)blockIdx.x * PAF_BLOCK + threadIdx.x; j < n; j += (u64)gridDim.x * PAF_BLOCK)
	{
		const fg_paf_hit h = hits[order[j]];
		if (h.query == h.target) continue;
		const u32 g = gid[j];
		if (!second) { if (paf_pair_a(h, ov)) atomicMin(&posA[g], (u32)j); }
		else if (paf_pair_b(h, ov) && posA[g] != (u32)j) atomicMin(&posB[g], (u32)j);
	}
}

__global__ void __launch_bounds__(PAF_BLOCK)
k_paf_pair_out(const fg_paf_hit* __restrict__ hits, const u32* __restrict__ order, const u32* __restrict__ posA,
			   const u32* __restrict__ posB, u32 nGroups, i32* __restrict__ pairFirst, i32* __restrict__ pairSecond, uint8_t* __restrict__ pairOk)
{
	for (u64 g = (u64)blockIdx.x * PAF_BLOCK + threadIdx.x; g < nGroups; g += (u64)gridDim.x * PAF_BLOCK)
	{
		const u32 a = posA[g], b = posB[g];
		const i32 f = a == PAF_NONE ? -1 : (i32)order[a], s = b == PAF_NONE ? -1 : (i32)order[b];
		uint8_t ok = 0;
		if (f >= 0 && s >= 0)
		{
			const fg_paf_hit p0 = hits[f], p1 = hits[s];
			// mapping_segments_without_intersection (circular_sequences.py:70-79)
			ok = p1.query_start < p1.query_end && p1.query_end < p0.query_start && p0.query_start < p0.query_end &&
				 p0.target_start < p0.target_end && p0.target_end < p1.target_start && p1.target_start < p1.target_end;
		}
		pairFirst[g] = f; pairSecond[g] = s; pairOk[g] = ok;
	}
}

// ---- components -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PAF_BLOCK) k_cc_init(u32* __restrict__ parent, u32 n)
{
	for (u64 v = (u64)blockIdx.x * PAF_BLOCK + threadIdx.x; v < n; v += (u64)gridDim.x * PAF_BLOCK) parent[v] = (u32)v;
}

// parent[x] <= x throughout: the larger label goes under the smaller
__global__ void __launch_bounds__(PAF_BLOCK)
k_cc_hook(const u32* __restrict__ edgeU, const u32* __restrict__ edgeV, u64 m, u32* parent, u32* changed)
{
	for (u64 e = (u64)blockIdx.x * PAF_BLOCK + threadIdx.x; e < m; e += (u64)gridDim.x * PAF_BLOCK)
	{
		const u32 pu = __hip_atomic_load(parent + edgeU[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		const u32 pv = __hip_atomic_load(parent + edgeV[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		if (pu == pv) continue;
		atomicMin(parent + (pu > pv ? pu : pv), pu > pv ? pv : pu);
		__hip_atomic_store(changed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

// every vertex to the root of its chain; a root (parent[r] == r) is left alone, other threads' stores only shorten chains
__global__ void __launch_bounds__(PAF_BLOCK) k_cc_jump(u32* parent, u32 n)
{
	for (u64 v = (u64)blockIdx.x * PAF_BLOCK + threadIdx.x; v < n; v += (u64)gridDim.x * PAF_BLOCK)
	{
		u32 p = __hip_atomic_load(parent + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		while (true)
		{
			const u32 q = __hip_atomic_load(parent + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			if (q == p) break;
			p = q;
		}
		__hip_atomic_store(parent + v, p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	}
}

// ---- host -----------------------------------------------------------------------------------------------------------
struct PafSwitches { u32 waveMax, wgMax; int tile; };

PafSwitches pafSwitches()
{
	PafSwitches s;
	s.waveMax = (u32)std::min<u64>(stageEnvU64("FG_PAF_WAVE_MAX", PAF_WAVE_CAP), PAF_WAVE_CAP);
	s.wgMax = (u32)std::min<u64>(stageEnvU64("FG_PAF_WG_MAX", PAF_WG_CAP), PAF_WG_CAP);
	s.tile = (int)std::min<u64>(std::max<u64>(stageEnvU64("FG_PAF_TILE", PAF_TILE_CAP), 64), PAF_TILE_CAP);
	return s;
}

struct PafShape { u32 maxId; u64 nRuns; };

// the preconditions of a hit array; the largest name id and the number of runs
PafShape pafCheck(const std::string& name, const fg_paf_hit* hits, u64 n)
{
	if (n > 0x7fffffffULL) throw FgError{FG_ERR_ARG, name + ": more than 2^31 - 1 hits"};
	if (n && !hits) throw FgError{FG_ERR_ARG, name + ": null hits"};
	PafShape sh{0, 0};
	for (u64 i = 0; i < n; ++i)
	{
		const fg_paf_hit& h = hits[i];
		if (h.query_start < 0 || h.query_end < h.query_start || h.target_start < 0 || h.target_end < h.target_start)
			throw FgError{FG_ERR_ARG, name + ": hit " + std::to_string(i) + " is without 0 <= start <= end"};
		sh.maxId = std::max(sh.maxId, std::max(h.query, h.target));
		sh.nRuns += i == 0 || hits[i - 1].query != h.query;
	}
	if (n > fgprim::RS_MAX_N) throw FgError{FG_ERR_NOMEM, name + ": more than 2^30 - 1 hits in one call"};
	return sh;
}

// what the grouping leaves on the device
struct PafGroups {
	const fg_paf_hit* hits;
	u32* gid;				// the group of every sorted hit
	u32* order;
	u64* groupOff;
	u32 *groupQuery, *groupTarget;
	u32 nGroups;
	u64 *k0, *v0, *k1, *v1;	// the sort's buffers, free again
	char* sortScratch;
	u32* scanScratch;
};

PafGroups pafGroupOnDevice(fg_ctx* c, DevPool& B, const fg_paf_hit* hits, u64 n, const PafShape& shape)
{
	hipStream_t s = c->stream;
	PafGroups G{};
	fg_paf_hit* dHits = B.get<fg_paf_hit>(n);
	u32* dRun = B.get<u32>(n);
	G.gid = B.get<u32>(n);
	G.scanScratch = B.get<u32>(fgprim::scanScratchElems(n));
	G.k0 = B.get<u64>(n); G.v0 = B.get<u64>(n); G.k1 = B.get<u64>(n); G.v1 = B.get<u64>(n);
	G.sortScratch = B.get<char>(fgprim::radixSortScratchBytes(n));
	G.order = B.get<u32>(n);
	G.hits = dHits;
	HIP_CHECK(hipMemcpyAsync(dHits, hits, n * sizeof(fg_paf_hit), hipMemcpyHostToDevice, s));
	const int targetBits = pafBits(shape.maxId), runBits = pafBits(shape.nRuns - 1);
	{
		ScopedK t(c->timer, "k_paf_group");
		hipLaunchKernelGGL(k_paf_run_flag, pafGrid(n), PAF_BLOCK, 0, s, (const fg_paf_hit*)dHits, n, dRun);
		fgprim::scan<u32>(s, dRun, dRun, n, true, G.scanScratch);
		hipLaunchKernelGGL(k_paf_keys, pafGrid(n), PAF_BLOCK, 0, s, (const fg_paf_hit*)dHits, (const u32*)dRun, n, targetBits, G.k0, G.v0);
	}
	int at;
	{
		ScopedK t(c->timer, "k_paf_sort");
		at = fgprim::radixSortPairs(s, G.k0, G.v0, G.k1, G.v1, n, 0, targetBits + runBits, G.sortScratch);
	}
	const u64* keys = at ? G.k1 : G.k0;
	const u64* vals = at ? G.v1 : G.v0;
	u32 last = 0;
	{
		ScopedK t(c->timer, "k_paf_group");
		hipLaunchKernelGGL(k_paf_group_flag, pafGrid(n), PAF_BLOCK, 0, s, keys, n, G.gid);
		fgprim::scan<u32>(s, G.gid, G.gid, n, true, G.scanScratch);
	}
	HIP_CHECK(hipMemcpyAsync(&last, G.gid + (n - 1), 4, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	G.nGroups = last + 1;
	G.groupOff = B.get<u64>((size_t)G.nGroups + 1);
	G.groupQuery = B.get<u32>(G.nGroups);
	G.groupTarget = B.get<u32>(G.nGroups);
	{
		ScopedK t(c->timer, "k_paf_group");
		hipLaunchKernelGGL(k_paf_group_out, pafGrid(n), PAF_BLOCK, 0, s, (const fg_paf_hit*)dHits, vals, (const u32*)G.gid, n, G.order,
						   G.groupOff, G.groupQuery, G.groupTarget);
	}
	HIP_CHECK(hipGetLastError());
	return G;
}

// the covers of the groups above FG_PAF_WG_MAX (list, nFlat of them with m segments, flatOff on the host) for one side
void pafFlatSide(fg_ctx* c, const PafGroups& G, const PafSwitches& sw, const u32* dList, u32 nFlat, const u64* dFlatOff, u64 m,
				 int side, i32* dIncl, PafTile* dTiles, i32* dCarry, long long* dCover)
{
	hipStream_t s = c->stream;
	const u64 nTiles = (m + sw.tile - 1) / sw.tile;
	ScopedK t(c->timer, "k_paf_cover_flat");
	hipLaunchKernelGGL(k_paf_flat_fill, std::min(nFlat, PAF_MAX_BLOCKS), PAF_BLOCK, 0, s, dList, nFlat, dFlatOff, (const u64*)G.groupOff,
					   (const u32*)G.order, G.hits, side, G.k0, G.v0);
	const int at = fgprim::radixSortPairs(s, G.k0, G.v0, G.k1, G.v1, m, 0, PAF_START_BITS + pafBits(G.nGroups - 1), G.sortScratch);
	const u64* keys = at ? G.k1 : G.k0;
	const u64* vals = at ? G.v1 : G.v0;
	hipLaunchKernelGGL(k_paf_flat_scan, (unsigned)nTiles, PAF_BLOCK, 0, s, keys, vals, m, sw.tile, dIncl, dTiles);
	hipLaunchKernelGGL(k_paf_flat_carry, 1, 64, 0, s, (const PafTile*)dTiles, nTiles, dCarry);
	hipLaunchKernelGGL(k_paf_flat_sum, pafGrid(m), PAF_BLOCK, 0, s, keys, vals, (const i32*)dIncl, (const i32*)dCarry, m, sw.tile,
					   (unsigned long long*)dCover);
	HIP_CHECK(hipGetLastError());
}

struct GroupsOwner {
	std::vector<uint32_t> order, groupQuery, groupTarget;
	std::vector<uint64_t> groupOff;
	std::vector<int64_t> queryCover, targetCover;
};

struct CircularOwner {
	std::vector<uint32_t> circQuery, circHit, groupQuery, groupTarget;
	std::vector<int32_t> pairFirst, pairSecond;
	std::vector<uint8_t> pairOk;
};

struct PafTextOwner {
	std::vector<uint64_t> nameOff[2];
	std::vector<uint32_t> nameLen[2];
	std::vector<int32_t> num[6];
};

bool pafIsSpace(unsigned char b) { return b == ' ' || (b >= '\t' && b <= '\r'); }		// \t \n \v \f \r

} // namespace

extern "C" {

int fg_paf_groups(fg_ctx* c, const struct fg_paf_hit* hits, uint64_t n_hits, struct fg_paf_group_batch* out)
{
	return stageCall<GroupsOwner>(c, out, [&](GroupsOwner*& own)
	{
		const std::string name = "fg_paf_groups";
		if (!out) throw FgError{FG_ERR_ARG, name + ": null result"};
		const PafShape shape = pafCheck(name, hits, n_hits);
		const u64 n = n_hits;
		own = new GroupsOwner;
		own->order.resize((size_t)n);
		own->groupOff.assign(1, 0);
		u32 nGroups = 0;
		HIP_CHECK(hipSetDevice(c->device));
		c->timer.reset();
		if (n)
		{
			hipStream_t s = c->stream;
			const PafSwitches sw = pafSwitches();
			DevPool B(c->dPaf, "paf");
			const PafGroups G = pafGroupOnDevice(c, B, hits, n, shape);
			nGroups = G.nGroups;
			own->groupOff.resize((size_t)nGroups + 1);
			own->groupQuery.resize(nGroups); own->groupTarget.resize(nGroups);
			own->queryCover.resize(nGroups); own->targetCover.resize(nGroups);
			HIP_CHECK(hipMemcpyAsync(own->order.data(), G.order, (size_t)n * 4, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipMemcpyAsync(own->groupOff.data(), G.groupOff, ((size_t)nGroups + 1) * 8, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipMemcpyAsync(own->groupQuery.data(), G.groupQuery, (size_t)nGroups * 4, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipMemcpyAsync(own->groupTarget.data(), G.groupTarget, (size_t)nGroups * 4, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipStreamSynchronize(s));
			// the class of a group follows its size: the wave's groups, then the workgroup's, then the flat route's
			const std::vector<uint64_t>& off = own->groupOff;
			std::vector<u32> list(nGroups);
			std::vector<u64> flatOff;
			u32 nWave = 0, nWg = 0, nFlat = 0;
			for (u32 g = 0; g < nGroups; ++g)
				if (off[g + 1] - off[g] <= sw.waveMax) list[nWave++] = g;
			for (u32 g = 0; g < nGroups; ++g)
				if (off[g + 1] - off[g] > sw.waveMax && off[g + 1] - off[g] <= sw.wgMax) list[nWave + nWg++] = g;
			u64 m = 0;
			for (u32 g = 0; g < nGroups; ++g)
				if (off[g + 1] - off[g] > sw.waveMax && off[g + 1] - off[g] > sw.wgMax)
				{
					list[nWave + nWg + nFlat++] = g;
					flatOff.push_back(m);
					m += off[g + 1] - off[g];
				}
			flatOff.push_back(m);
			u32* dList = B.get<u32>(nGroups);
			long long* dCover = B.get<long long>(2 * (size_t)nGroups);
			u64* dFlatOff = B.get<u64>(flatOff.size());
			const u64 nTiles = (m + sw.tile - 1) / sw.tile;
			i32* dIncl = B.get<i32>(m);
			PafTile* dTiles = B.get<PafTile>(nTiles);
			i32* dCarry = B.get<i32>(nTiles);
			HIP_CHECK(hipMemcpyAsync(dList, list.data(), (size_t)nGroups * 4, hipMemcpyHostToDevice, s));
			HIP_CHECK(hipMemcpyAsync(dFlatOff, flatOff.data(), flatOff.size() * 8, hipMemcpyHostToDevice, s));
			HIP_CHECK(hipMemsetAsync(dCover, 0, 2 * (size_t)nGroups * 8, s));
			if (nWave)
			{
				ScopedK t(c->timer, "k_paf_cover_wave");
				hipLaunchKernelGGL((k_paf_cover<64, PAF_WAVE_CAP>), std::min(nWave, 4 * PAF_MAX_BLOCKS), 64, 0, s, (const u32*)dList, nWave,
								   (const u64*)G.groupOff, (const u32*)G.order, G.hits, dCover, dCover + nGroups);
			}
			if (nWg)
			{
				ScopedK t(c->timer, "k_paf_cover_wg");
				hipLaunchKernelGGL((k_paf_cover<PAF_BLOCK, PAF_WG_CAP>), std::min(nWg, PAF_MAX_BLOCKS), PAF_BLOCK, 0, s,
								   (const u32*)(dList + nWave), nWg, (const u64*)G.groupOff, (const u32*)G.order, G.hits, dCover,
								   dCover + nGroups);
			}
			HIP_CHECK(hipGetLastError());
			if (nFlat)
				for (int side = 0; side < 2; ++side)
					pafFlatSide(c, G, sw, dList + nWave + nWg, nFlat, dFlatOff, m, side, dIncl, dTiles, dCarry, dCover + (size_t)side * nGroups);
			HIP_CHECK(hipMemcpyAsync(own->queryCover.data(), dCover, (size_t)nGroups * 8, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipMemcpyAsync(own->targetCover.data(), dCover + nGroups, (size_t)nGroups * 8, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipStreamSynchronize(s));		// `list` and `flatOff` live until their copies have run
		}
		c->timer.collect();
		stageKeep(own->order, own->groupQuery, own->groupTarget, own->queryCover, own->targetCover);
		out->n_hits = n;
		out->n_groups = nGroups;
		out->order = own->order.data();
		out->group_off = own->groupOff.data();
		out->group_query = own->groupQuery.data();
		out->group_target = own->groupTarget.data();
		out->query_cover = own->queryCover.data();
		out->target_cover = own->targetCover.data();
		out->owner_ = own;
	});
}

void fg_release_paf_groups(struct fg_paf_group_batch* b) { stageRelease<GroupsOwner>(b); }

int fg_paf_circular(fg_ctx* c, const struct fg_paf_hit* hits, uint64_t n_hits, int32_t max_overhang_read, int32_t max_overhang_pair,
					struct fg_paf_circular_batch* out)
{
	return stageCall<CircularOwner>(c, out, [&](CircularOwner*& own)
	{
		const std::string name = "fg_paf_circular";
		if (!out) throw FgError{FG_ERR_ARG, name + ": null result"};
		const PafShape shape = pafCheck(name, hits, n_hits);
		const u64 n = n_hits;
		own = new CircularOwner;
		u32 nGroups = 0, nCirc = 0;
		HIP_CHECK(hipSetDevice(c->device));
		c->timer.reset();
		if (n)
		{
			hipStream_t s = c->stream;
			DevPool B(c->dPaf, "paf");
			const PafGroups G = pafGroupOnDevice(c, B, hits, n, shape);
			nGroups = G.nGroups;
			const size_t nNames = (size_t)shape.maxId + 1;
			unsigned long long* dBest = B.get<unsigned long long>(nNames);
			u32* dFirst = B.get<u32>(nNames);
			u32* dRank = B.get<u32>(n);
			u32* dPos = B.get<u32>(2 * (size_t)nGroups);
			i32* dPair = B.get<i32>(2 * (size_t)nGroups);
			uint8_t* dOk = B.get<uint8_t>(nGroups);
			HIP_CHECK(hipMemsetAsync(dBest, 0, nNames * 8, s));
			HIP_CHECK(hipMemsetAsync(dFirst, 0xFF, nNames * 4, s));
			HIP_CHECK(hipMemsetAsync(dPos, 0xFF, 2 * (size_t)nGroups * 4, s));
			{
				ScopedK t(c->timer, "k_paf_circular");
				hipLaunchKernelGGL(k_paf_circ_mark, pafGrid(n), PAF_BLOCK, 0, s, G.hits, n, max_overhang_read, dBest, dFirst);
				hipLaunchKernelGGL(k_paf_circ_flag, pafGrid(n), PAF_BLOCK, 0, s, G.hits, n, (const u32*)dFirst, dRank);
				fgprim::scan<u32>(s, dRank, dRank, n, true, G.scanScratch);
			}
			HIP_CHECK(hipMemcpyAsync(&nCirc, dRank + (n - 1), 4, hipMemcpyDeviceToHost, s));
			{
				ScopedK t(c->timer, "k_paf_pairs");
				hipLaunchKernelGGL(k_paf_pair_pos, pafGrid(n), PAF_BLOCK, 0, s, G.hits, (const u32*)G.order, (const u32*)G.gid, n,
								   max_overhang_pair, 0, dPos, dPos + nGroups);
				hipLaunchKernelGGL(k_paf_pair_pos, pafGrid(n), PAF_BLOCK, 0, s, G.hits, (const u32*)G.order, (const u32*)G.gid, n,
								   max_overhang_pair, 1, dPos, dPos + nGroups);
				hipLaunchKernelGGL(k_paf_pair_out, pafGrid(nGroups), PAF_BLOCK, 0, s, G.hits, (const u32*)G.order, (const u32*)dPos,
								   (const u32*)(dPos + nGroups), nGroups, dPair, dPair + nGroups, dOk);
			}
			HIP_CHECK(hipGetLastError());
			HIP_CHECK(hipStreamSynchronize(s));
			u32* dCirc = B.get<u32>(2 * (size_t)nCirc);
			if (nCirc)
			{
				ScopedK t(c->timer, "k_paf_circular");
				hipLaunchKernelGGL(k_paf_circ_out, pafGrid(n), PAF_BLOCK, 0, s, G.hits, n, (const u32*)dFirst, (const unsigned long long*)dBest,
								   (const u32*)dRank, dCirc, dCirc + nCirc);
			}
			HIP_CHECK(hipGetLastError());
			own->circQuery.resize(nCirc); own->circHit.resize(nCirc);
			own->groupQuery.resize(nGroups); own->groupTarget.resize(nGroups);
			own->pairFirst.resize(nGroups); own->pairSecond.resize(nGroups); own->pairOk.resize(nGroups);
			if (nCirc)
			{
				HIP_CHECK(hipMemcpyAsync(own->circQuery.data(), dCirc, (size_t)nCirc * 4, hipMemcpyDeviceToHost, s));
				HIP_CHECK(hipMemcpyAsync(own->circHit.data(), dCirc + nCirc, (size_t)nCirc * 4, hipMemcpyDeviceToHost, s));
			}
			HIP_CHECK(hipMemcpyAsync(own->groupQuery.data(), G.groupQuery, (size_t)nGroups * 4, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipMemcpyAsync(own->groupTarget.data(), G.groupTarget, (size_t)nGroups * 4, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipMemcpyAsync(own->pairFirst.data(), dPair, (size_t)nGroups * 4, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipMemcpyAsync(own->pairSecond.data(), dPair + nGroups, (size_t)nGroups * 4, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipMemcpyAsync(own->pairOk.data(), dOk, (size_t)nGroups, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipStreamSynchronize(s));
		}
		c->timer.collect();
		stageKeep(own->circQuery, own->circHit, own->groupQuery, own->groupTarget, own->pairFirst, own->pairSecond, own->pairOk);
		out->n_hits = n;
		out->n_circular = nCirc;
		out->circ_query = own->circQuery.data();
		out->circ_hit = own->circHit.data();
		out->n_groups = nGroups;
		out->group_query = own->groupQuery.data();
		out->group_target = own->groupTarget.data();
		out->pair_first = own->pairFirst.data();
		out->pair_second = own->pairSecond.data();
		out->pair_ok = own->pairOk.data();
		out->owner_ = own;
	});
}

void fg_release_paf_circular(struct fg_paf_circular_batch* b) { stageRelease<CircularOwner>(b); }

int fg_components(fg_ctx* c, uint32_t n_vertices, uint64_t n_edges, const uint32_t* edge_u, const uint32_t* edge_v, uint32_t* labels)
{
	if (!c) return FG_ERR_ARG;
	const int rc = guarded(c, [&]
	{
		const std::string name = "fg_components";
		if (n_vertices && !labels) throw FgError{FG_ERR_ARG, name + ": null labels"};
		if (n_edges && (!edge_u || !edge_v)) throw FgError{FG_ERR_ARG, name + ": null edge_u or edge_v"};
		for (u64 e = 0; e < n_edges; ++e)
			if (edge_u[e] >= n_vertices || edge_v[e] >= n_vertices)
				throw FgError{FG_ERR_ARG, name + ": edge " + std::to_string(e) + " has a vertex index >= n_vertices"};
		HIP_CHECK(hipSetDevice(c->device));
		c->timer.reset();
		if (n_vertices)
		{
			hipStream_t s = c->stream;
			DevPool B(c->dPaf, "paf");
			u32* dParent = B.get<u32>(n_vertices);
			u32* dU = B.get<u32>(n_edges);
			u32* dV = B.get<u32>(n_edges);
			u32* dChanged = B.get<u32>(1);
			if (n_edges)
			{
				HIP_CHECK(hipMemcpyAsync(dU, edge_u, n_edges * 4, hipMemcpyHostToDevice, s));
				HIP_CHECK(hipMemcpyAsync(dV, edge_v, n_edges * 4, hipMemcpyHostToDevice, s));
			}
			hipLaunchKernelGGL(k_cc_init, pafGrid(n_vertices), PAF_BLOCK, 0, s, dParent, n_vertices);
			while (n_edges)
			{
				u32 changed = 0;
				HIP_CHECK(hipMemsetAsync(dChanged, 0, 4, s));
				{
					ScopedK t(c->timer, "k_cc_hook");
					hipLaunchKernelGGL(k_cc_hook, pafGrid(n_edges), PAF_BLOCK, 0, s, (const u32*)dU, (const u32*)dV, (u64)n_edges, dParent, dChanged);
				}
				HIP_CHECK(hipMemcpyAsync(&changed, dChanged, 4, hipMemcpyDeviceToHost, s));
				HIP_CHECK(hipStreamSynchronize(s));
				if (!changed) break;
				ScopedK t(c->timer, "k_cc_jump");
				hipLaunchKernelGGL(k_cc_jump, pafGrid(n_vertices), PAF_BLOCK, 0, s, dParent, n_vertices);
			}
			HIP_CHECK(hipGetLastError());
			HIP_CHECK(hipMemcpyAsync(labels, dParent, (size_t)n_vertices * 4, hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipStreamSynchronize(s));
		}
		c->timer.collect();
	});
	if (rc != FG_OK) c->timer.reset();
	return rc;
}

int fg_paf_parse(const char* text, uint64_t n_bytes, struct fg_paf_text* out)
{
	if (out) memset(out, 0, sizeof(*out));
	std::string& err = fgHostError();
	err.clear();
	if (!out || (n_bytes && !text)) { err = "fg_paf_parse: null argument"; return FG_ERR_ARG; }
	PafTextOwner* own = nullptr;
	try
	{
		own = new PafTextOwner;
		const unsigned char* p = (const unsigned char*)text;
		u64 line = 0, at = 0;
		while (at < n_bytes)
		{
			++line;
			u64 end = at;
			while (end < n_bytes && p[end] != '\n') ++end;
			int field = 0;
			u64 i = at;
			while (field < 9)
			{
				while (i < end && pafIsSpace(p[i])) ++i;
				if (i == end) break;
				u64 j = i;
				while (j < end && !pafIsSpace(p[j])) ++j;
				if (field == 0 || field == 5)
				{
					own->nameOff[field == 5].push_back(i);
					own->nameLen[field == 5].push_back((u32)std::min<u64>(j - i, 0xffffffffULL));
				}
				else if (field != 4)
				{
					// int() of the field: an optionally signed decimal number
					u64 k = i;
					const bool neg = p[k] == '-';
					if (p[k] == '-' || p[k] == '+') ++k;
					bool good = k < j;
					long long v = 0;
					for (; k < j && good; ++k)
					{
						if (p[k] < '0' || p[k] > '9') { good = false; break; }
						v = v * 10 + (p[k] - '0');
						if (v > 0x80000000LL) v = 0x80000001LL;			// stays out of range, cannot overflow
					}
					if (!good)
						throw FgError{FG_ERR_ARG, "fg_paf_parse: line " + std::to_string(line) + ": field " + std::to_string(field + 1) + " is no decimal number"};
					if (neg) v = -v;
					if (v < -0x80000000LL || v > 0x7fffffffLL)
						throw FgError{FG_ERR_ARG, "fg_paf_parse: line " + std::to_string(line) + ": field " + std::to_string(field + 1) + " is outside int32"};
					own->num[field < 4 ? field - 1 : field - 3].push_back((int32_t)v);
				}
				++field;
				i = j;
			}
			if (field < 9)
				throw FgError{FG_ERR_ARG, "fg_paf_parse: line " + std::to_string(line) + " has " + std::to_string(field) + " fields, 9 are needed"};
			at = end + 1;
		}
		out->n_hits = own->num[0].size();
		stageKeep(own->nameOff[0], own->nameOff[1], own->nameLen[0], own->nameLen[1], own->num[0], own->num[1], own->num[2], own->num[3],
				  own->num[4], own->num[5]);
		out->query_name_off = own->nameOff[0].data(); out->query_name_len = own->nameLen[0].data();
		out->target_name_off = own->nameOff[1].data(); out->target_name_len = own->nameLen[1].data();
		out->query_len = own->num[0].data(); out->query_start = own->num[1].data(); out->query_end = own->num[2].data();
		out->target_len = own->num[3].data(); out->target_start = own->num[4].data(); out->target_end = own->num[5].data();
		out->owner_ = own;
		return FG_OK;
	}
	catch (const FgError& e) { err = e.msg; delete own; memset(out, 0, sizeof(*out)); return e.code; }
	catch (const std::bad_alloc&) { err = "fg_paf_parse: host allocation failed"; delete own; memset(out, 0, sizeof(*out)); return FG_ERR_NOMEM; }
}

void fg_release_paf_text(struct fg_paf_text* b) { stageRelease<PafTextOwner>(b); }

} // extern "C"
