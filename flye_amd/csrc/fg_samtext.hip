// fg_sam_parse: the tokeniser in front of the SAM paths (reference flye/utils/sam_parser.py: _read_file_chunk :168-213,
// the per-line part of get_chunk :355-377, the expression of :140), a flat pass over the bytes of a sub-batch of whole
// lines.  A line is 10 - 40 kB with everything of interest in its first hundred bytes, yet every byte has to be seen
// once to find the next line and to count tokens up to the eleventh: so bytes, not lines, are spread over the lanes.
//   tile walk      a workgroup takes one tile of FG_SAM_TILE bytes in rounds of 4096; a lane loads 16 bytes and makes 16-bit
//                  masks of them: newline, tab, token start (a non-space byte after a space byte or at the text's begin),
//                  token end, and "one of MIDNSHP=X after a digit".  An exclusive scan over the block of the packed counts
//                  gives every lane the counts before its bytes inside the tile.
//   k_sam_classify the tile's counts of newlines, tabs and token starts            (scans of fg_devprim.h over the tiles)
//   k_sam_lines    the walk again: each newline writes where the next line starts and the tabs / token starts before it
//   k_sam_scatter  the walk again: count before the byte - count at the line's first byte = the rank of a tab or token
//                  in its line; tabs 0 - 2 and the starts and ends of tokens 0 - 10 write their position into the line's
//                  table of 27 words.  A run end inside token 5 is listed per tile (at most tile / 2 of them), and the
//                  start and the end of token 5 note how many the tile has listed by then     (scan of the tile's run ends)
//   k_sam_record   one lane per line: header prefix, three tabs, eleven tokens, the runs of the line from the two notes
//                  (scans: the records before a line, the runs before a line)
//   k_sam_fields   one lane per line, records only: every per-record field, FLAG and POS, the '*' test
//   k_sam_chunk    one lane per record: tab RNAME against the record before (the first record of a sub-batch is the host's:
//                  it carries the RNAME before the cut as offsets into the text)
//   k_sam_runs     one lane per listed run end: its tile and line by binary search, the digit run before it in 64 bits
//   k_sam_span     the four sums of _parse_cigar :316-320 over a record's runs: a lane sums a record of up to 32 runs
//                  (the clips and short alignments of a file), k_sam_span_wave a wave one of more, with a reduction
// No atomics: every word has one writer.
#include "fg_ctx.h"
#include "fg_stage.h"
#include "fg_devprim.h"

namespace {

#define SAM_BLOCK 256
#define SAM_PIECE 16							// bytes of a lane
#define SAM_ROUND (SAM_BLOCK * SAM_PIECE)
#define SAM_NONE 0xFFFFFFFFu
#define SAM_TOKENS 11
#define SAM_TAB 0								// the line's table: tabs 0 - 2
#define SAM_TS 3								// token starts 0 - 10
#define SAM_TE 14								// token ends (one past the last byte) 0 - 10
#define SAM_R0 25								// run ends the tile has listed before token 5's first byte
#define SAM_R1 26								// ... up to token 5's last byte
#define SAM_WORDS 27
#define SAM_SPAN_CUT 32							// runs of a record that one lane sums
#define SAM_MAX_BATCH (1ULL << 30)

unsigned samGrid(u64 n) { return (unsigned)std::min<u64>(std::max<u64>((n + SAM_BLOCK - 1) / SAM_BLOCK, 1), 16384); }

__device__ __forceinline__ bool sam_space(u32 b) { return b == 32u || (b >= 9u && b <= 13u); }
__device__ __forceinline__ bool sam_digit(u32 b) { return b - 48u <= 9u; }
__device__ __forceinline__ bool sam_op(u32 b)
{
	return b == 'M' || b == 'I' || b == 'D' || b == 'N' || b == 'S' || b == 'H' || b == 'P' || b == '=' || b == 'X';
}
__device__ __forceinline__ u32 sam_below(int i) { return (1u << i) - 1u; }

struct SamPiece { u32 nl, tab, ts, te, cand; };

// the masks of the 16 bytes behind p0 (p0 < n, a multiple of 16; the buffer is readable 16 bytes past n)
__device__ __forceinline__ SamPiece sam_piece(const uint8_t* __restrict__ text, u32 n, u32 p0)
{
	const uint4 q = *(const uint4*)(text + p0);
	const u32 w[4] = {q.x, q.y, q.z, q.w};
	const u32 prev = p0 ? text[p0 - 1] : 10u, next = p0 + SAM_PIECE < n ? text[p0 + SAM_PIECE] : 10u;
	u32 nl = 0, tab = 0, ws = 0, dg = 0, op = 0;
#pragma unroll
	for (int i = 0; i < SAM_PIECE; ++i)
	{
		const u32 b = (w[i >> 2] >> (8 * (i & 3))) & 255u;
		nl |= (u32)(b == 10u) << i;
		tab |= (u32)(b == 9u) << i;
		ws |= (u32)sam_space(b) << i;
		dg |= (u32)sam_digit(b) << i;
		op |= (u32)sam_op(b) << i;
	}
	const u32 valid = n - p0 >= SAM_PIECE ? 0xFFFFu : sam_below((int)(n - p0));
	ws = (ws | ~valid) & 0xFFFFu;				// past the text: space
	const u32 nonws = ~ws & 0xFFFFu;
	SamPiece pc;
	pc.nl = nl & valid;
	pc.tab = tab & valid;
	pc.ts = nonws & ((ws << 1) | (u32)sam_space(prev));
	pc.te = nonws & ((ws >> 1) | ((u32)sam_space(next) << 15));
	pc.cand = op & valid & ((dg << 1) | (u32)sam_digit(prev));
	return pc;
}

// newlines, tabs and token starts in 21 bits each
__device__ __forceinline__ u64 sam_pack(const SamPiece& pc)
{
	return (u64)__popc(pc.nl) | ((u64)__popc(pc.tab) << 21) | ((u64)__popc(pc.ts) << 42);
}
__device__ __forceinline__ u32 sam_nl(u64 v) { return (u32)v & 0x1FFFFFu; }
__device__ __forceinline__ u32 sam_tab(u64 v) { return (u32)(v >> 21) & 0x1FFFFFu; }
__device__ __forceinline__ u32 sam_tok(u64 v) { return (u32)(v >> 42) & 0x1FFFFFu; }

__global__ void __launch_bounds__(SAM_BLOCK)
k_sam_classify(const uint8_t* __restrict__ text, u32 n, u32 tile, u32* __restrict__ tileNl, u32* __restrict__ tileTab, u32* __restrict__ tileTok)
{
	__shared__ u64 sh[SAM_BLOCK / 64];
	const u32 tileBase = blockIdx.x * tile, tileEnd = min(tileBase + tile, n);
	u64 carry = 0;
	for (u32 rb = tileBase; rb < tileEnd; rb += SAM_ROUND)
	{
		const u32 p0 = rb + threadIdx.x * SAM_PIECE;
		u64 mine = 0;
		if (p0 < tileEnd) mine = sam_pack(sam_piece(text, n, p0));
		u64 tot;
		(void)fgprim::block_exscan_256<u64>(mine, sh, &tot);
		carry += tot;
	}
	if (threadIdx.x == 0)
	{
		tileNl[blockIdx.x] = sam_nl(carry);
		tileTab[blockIdx.x] = sam_tab(carry);
		tileTok[blockIdx.x] = sam_tok(carry);
	}
}

// tileNl / tileTab / tileTok: the exclusive sums.  lineStart has nLines + 1 entries: a line ends one byte before the next starts.
__global__ void __launch_bounds__(SAM_BLOCK)
k_sam_lines(const uint8_t* __restrict__ text, u32 n, u32 tile, const u32* __restrict__ tileNl, const u32* __restrict__ tileTab,
			const u32* __restrict__ tileTok, u32 nLines, int lastIsNl, u32* __restrict__ lineStart, u32* __restrict__ lineTab0,
			u32* __restrict__ lineTok0)
{
	__shared__ u64 sh[SAM_BLOCK / 64];
	const u32 tileBase = blockIdx.x * tile, tileEnd = min(tileBase + tile, n);
	const u32 nl0 = tileNl[blockIdx.x], tab0 = tileTab[blockIdx.x], tok0 = tileTok[blockIdx.x];
	if (blockIdx.x == 0 && threadIdx.x == 0)
	{
		lineStart[0] = 0; lineTab0[0] = 0; lineTok0[0] = 0;
		if (!lastIsNl) lineStart[nLines] = n + 1;			// as if the text ended in a newline
	}
	u64 carry = 0;
	for (u32 rb = tileBase; rb < tileEnd; rb += SAM_ROUND)
	{
		const u32 p0 = rb + threadIdx.x * SAM_PIECE;
		SamPiece pc{};
		if (p0 < tileEnd) pc = sam_piece(text, n, p0);
		u64 tot;
		const u64 ex = fgprim::block_exscan_256<u64>(sam_pack(pc), sh, &tot) + carry;
		carry += tot;
		u32 m = pc.nl;
		while (m)
		{
			const int i = __ffs((int)m) - 1;
			m &= m - 1;
			const u32 line = nl0 + sam_nl(ex) + (u32)__popc(pc.nl & sam_below(i)) + 1;
			if (line > nLines) continue;					// cannot be: nLines counts every newline
			lineStart[line] = p0 + i + 1;
			lineTab0[line] = tab0 + sam_tab(ex) + (u32)__popc(pc.tab & sam_below(i));
			lineTok0[line] = tok0 + sam_tok(ex) + (u32)__popc(pc.ts & sam_below(i));
		}
	}
}

// table: SAM_WORDS per line, all ones before; runPos: tile / 2 slots per tile; tileRun: the tile's run ends
__global__ void __launch_bounds__(SAM_BLOCK)
k_sam_scatter(const uint8_t* __restrict__ text, u32 n, u32 tile, const u32* __restrict__ tileNl, const u32* __restrict__ tileTab,
			  const u32* __restrict__ tileTok, u32 nLines, const u32* __restrict__ lineTab0, const u32* __restrict__ lineTok0,
			  u32* __restrict__ table, u32* __restrict__ runPos, u32* __restrict__ tileRun)
{
	__shared__ u64 sh[SAM_BLOCK / 64];
	__shared__ u32 shRun[SAM_BLOCK / 64];
	const u32 tileBase = blockIdx.x * tile, tileEnd = min(tileBase + tile, n);
	const u32 nl0 = tileNl[blockIdx.x], tab0 = tileTab[blockIdx.x], tok0 = tileTok[blockIdx.x];
	u32* const myRuns = runPos + (u64)blockIdx.x * (tile / 2);
	u64 carry = 0;
	u32 runCarry = 0;
	for (u32 rb = tileBase; rb < tileEnd; rb += SAM_ROUND)
	{
		const u32 p0 = rb + threadIdx.x * SAM_PIECE;
		SamPiece pc{};
		if (p0 < tileEnd) pc = sam_piece(text, n, p0);
		u64 tot;
		const u64 ex = fgprim::block_exscan_256<u64>(sam_pack(pc), sh, &tot) + carry;
		carry += tot;
		const u32 nlB = nl0 + sam_nl(ex), tabB = tab0 + sam_tab(ex), tokB = tok0 + sam_tok(ex);
		// the candidates that lie in token 5 of their line
		u32 conf = 0, m = pc.cand;
		while (m)
		{
			const int i = __ffs((int)m) - 1;
			m &= m - 1;
			const u32 line = nlB + (u32)__popc(pc.nl & sam_below(i));
			if (line >= nLines) continue;
			if (tokB + (u32)__popc(pc.ts & sam_below(i + 1)) - 1 - lineTok0[line] == 5u) conf |= 1u << i;
		}
		u32 runTot;
		const u32 runEx = fgprim::block_exscan_256<u32>((u32)__popc(conf), shRun, &runTot) + runCarry;
		runCarry += runTot;
		m = pc.tab | pc.ts | pc.te;
		while (m)
		{
			const int i = __ffs((int)m) - 1;
			m &= m - 1;
			const u32 line = nlB + (u32)__popc(pc.nl & sam_below(i));
			if (line >= nLines) continue;
			u32* const row = table + (u64)line * SAM_WORDS;
			const u32 p = p0 + i;
			if ((pc.tab >> i) & 1u)
			{
				const u32 rank = tabB + (u32)__popc(pc.tab & sam_below(i)) - lineTab0[line];
				if (rank < 3u) row[SAM_TAB + rank] = p;
				continue;
			}
			const u32 base = lineTok0[line];
			if ((pc.ts >> i) & 1u)
			{
				const u32 rank = tokB + (u32)__popc(pc.ts & sam_below(i)) - base;
				if (rank < SAM_TOKENS) row[SAM_TS + rank] = p;
				if (rank == 5u) row[SAM_R0] = runEx + (u32)__popc(conf & sam_below(i));
			}
			if ((pc.te >> i) & 1u)
			{
				const u32 rank = tokB + (u32)__popc(pc.ts & sam_below(i + 1)) - 1 - base;
				if (rank < SAM_TOKENS) row[SAM_TE + rank] = p + 1;
				if (rank == 5u) row[SAM_R1] = runEx + (u32)__popc(conf & sam_below(i + 1));
			}
		}
		m = conf;
		while (m)
		{
			const int i = __ffs((int)m) - 1;
			m &= m - 1;
			const u32 slot = runEx + (u32)__popc(conf & sam_below(i));
			if (slot < tile / 2) myRuns[slot] = p0 + i;		// a run end follows a digit: no two are neighbours
		}
	}
	if (threadIdx.x == 0) tileRun[blockIdx.x] = runCarry;
}

// per line (and one entry past the last, zero, for the sums): is it a record, the runs of its CIGAR and where the tiles list
// the first of them (SAM_NONE: the line has no runs to report)
__global__ void __launch_bounds__(SAM_BLOCK)
k_sam_record(const uint8_t* __restrict__ text, u32 nLines, u32 tile, const u32* __restrict__ lineStart, const u32* __restrict__ table,
			 const u32* __restrict__ tileRunOff, u32* __restrict__ isRec, u32* __restrict__ lineRuns, u32* __restrict__ lineR0)
{
	for (u64 l = (u64)blockIdx.x * SAM_BLOCK + threadIdx.x; l <= nLines; l += (u64)gridDim.x * SAM_BLOCK)
	{
		u32 rec = 0, runs = 0, r0 = SAM_NONE;
		if (l < nLines)
		{
			const u32 s = lineStart[l], len = lineStart[l + 1] - 1 - s;
			const u32* const row = table + l * SAM_WORDS;
			bool header = false;
			if (len >= 3 && text[s] == '@')
			{
				const u32 a = text[s + 1], b = text[s + 2];
				header = (a == 'P' && b == 'G') || (a == 'H' && b == 'D') || (a == 'S' && b == 'Q') || (a == 'R' && b == 'G') ||
						 (a == 'C' && b == 'O');
			}
			rec = !header && row[SAM_TAB + 2] != SAM_NONE;
			if (rec && row[SAM_TS + SAM_TOKENS - 1] != SAM_NONE)
			{
				r0 = tileRunOff[row[SAM_TS + 5] / tile] + row[SAM_R0];
				runs = tileRunOff[(row[SAM_TE + 5] - 1) / tile] + row[SAM_R1] - r0;
			}
		}
		isRec[l] = rec; lineRuns[l] = runs; lineR0[l] = r0;
	}
}

struct SamOut {
	u64 *lineNo, *lineOff; u32* lineLen;
	uint8_t* status;
	u64* tabOff; u32* tabLen;
	u64* tokOff[4]; u32* tokLen[4];			// tokens 0, 2, 5, 9
	i32 *flag, *pos;
	long long *qryStart, *qryEnd;
	u64* runOff;
	uint8_t* runOp; u32* runLen; uint8_t* runOvf;
	uint8_t* chunkFlag;
};

// the token text[a .. b) as [+-]?[0-9]+ within int32
__device__ __forceinline__ bool sam_int32(const uint8_t* __restrict__ text, u32 a, u32 b, i32* out)
{
	const bool neg = text[a] == '-';
	if (text[a] == '-' || text[a] == '+') ++a;
	if (a >= b) return false;
	long long v = 0;
	for (; a < b; ++a)
	{
		if (!sam_digit(text[a])) return false;
		v = v * 10 + (text[a] - 48);
		if (v > 0x80000000LL) v = 0x80000001LL;			// stays out of range, cannot overflow
	}
	if (neg) v = -v;
	if (v < -0x80000000LL || v > 0x7fffffffLL) return false;
	*out = (i32)v;
	return true;
}

// recIdx / runOffLine: the exclusive sums of isRec / lineRuns, nLines + 1 entries
__global__ void __launch_bounds__(SAM_BLOCK)
k_sam_fields(const uint8_t* __restrict__ text, u32 nLines, u64 textBase, u64 lineBase, u64 runBase, const u32* __restrict__ lineStart,
			 const u32* __restrict__ table, const u32* __restrict__ recIdx, const u32* __restrict__ runOffLine, SamOut o)
{
	for (u64 l = (u64)blockIdx.x * SAM_BLOCK + threadIdx.x; l <= nLines; l += (u64)gridDim.x * SAM_BLOCK)
	{
		const u32 r = recIdx[l];
		if (l == nLines) { o.runOff[r] = runBase + runOffLine[l]; continue; }
		if (recIdx[l + 1] == r) continue;
		const u32 s = lineStart[l];
		const u32* const row = table + l * SAM_WORDS;
		o.lineNo[r] = lineBase + l + 1;
		o.lineOff[r] = textBase + s;
		o.lineLen[r] = lineStart[l + 1] - 1 - s;
		o.tabOff[r] = textBase + row[SAM_TAB + 1] + 1;
		o.tabLen[r] = row[SAM_TAB + 2] - row[SAM_TAB + 1] - 1;
		o.runOff[r] = runBase + runOffLine[l];
		const bool full = row[SAM_TS + SAM_TOKENS - 1] != SAM_NONE;
		u32 st = full ? 0u : 1u;
		i32 flag = 0, pos = 0;
		const int which[4] = {0, 2, 5, 9};
#pragma unroll
		for (int k = 0; k < 4; ++k)
		{
			o.tokOff[k][r] = full ? textBase + row[SAM_TS + which[k]] : 0;
			o.tokLen[k][r] = full ? row[SAM_TE + which[k]] - row[SAM_TS + which[k]] : 0;
		}
		if (full)
		{
			if (!sam_int32(text, row[SAM_TS + 1], row[SAM_TE + 1], &flag)) { st |= 2u; flag = 0; }
			if (!sam_int32(text, row[SAM_TS + 3], row[SAM_TE + 3], &pos)) { st |= 4u; pos = 0; }
			if (row[SAM_TE + 9] - row[SAM_TS + 9] == 1 && text[row[SAM_TS + 9]] == '*') st |= 8u;
		}
		o.status[r] = (uint8_t)st;
		o.flag[r] = flag; o.pos[r] = pos;
	}
}

// chunkFlag[r] = 1 where record r's tab RNAME differs from that of record r - 1; r = 0 is the host's
__global__ void __launch_bounds__(SAM_BLOCK)
k_sam_chunk(const uint8_t* __restrict__ text, u32 nRec, u64 textBase, SamOut o)
{
	for (u64 r = (u64)blockIdx.x * SAM_BLOCK + threadIdx.x; r < nRec; r += (u64)gridDim.x * SAM_BLOCK)
	{
		uint8_t differs = 1;
		if (r > 0 && o.tabLen[r] == o.tabLen[r - 1])
		{
			const uint8_t* const a = text + (o.tabOff[r] - textBase);
			const uint8_t* const b = text + (o.tabOff[r - 1] - textBase);
			const u32 len = o.tabLen[r];
			u32 k = 0;
			while (k < len && a[k] == b[k]) ++k;
			differs = k < len;
		}
		o.chunkFlag[r] = differs;
	}
}

// the largest i in [0, n) with a[i] <= v (a ascends, a[0] <= v)
__device__ __forceinline__ u32 sam_find(const u32* __restrict__ a, u32 n, u32 v)
{
	u32 lo = 0, hi = n;
	while (hi - lo > 1)
	{
		const u32 mid = lo + (hi - lo) / 2;
		if (a[mid] <= v) lo = mid; else hi = mid;
	}
	return lo;
}

__global__ void __launch_bounds__(SAM_BLOCK)
k_sam_runs(const uint8_t* __restrict__ text, u32 nListed, u32 nTiles, u32 tile, const u32* __restrict__ tileRunOff,
		   const u32* __restrict__ runPos, u32 nLines, const u32* __restrict__ lineStart, const u32* __restrict__ lineR0,
		   const u32* __restrict__ runOffLine, u32 nRuns, SamOut o)
{
	for (u64 j = (u64)blockIdx.x * SAM_BLOCK + threadIdx.x; j < nListed; j += (u64)gridDim.x * SAM_BLOCK)
	{
		const u32 t = sam_find(tileRunOff, nTiles, (u32)j);
		const u32 p = runPos[(u64)t * (tile / 2) + ((u32)j - tileRunOff[t])];
		const u32 line = sam_find(lineStart, nLines, p);
		const u32 r0 = lineR0[line];
		if (r0 == SAM_NONE) continue;						// token 5 of a dropped line, or of a record without eleven tokens
		const u32 at = runOffLine[line] + ((u32)j - r0);
		if (at >= nRuns) continue;
		u32 a = p;
		while (a > 0 && sam_digit(text[a - 1])) --a;
		u64 v = 0;
		bool ovf = false;
		for (; a < p; ++a)
		{
			v = v * 10 + (text[a] - 48);
			if (v > 0xFFFFFFFFULL) { ovf = true; v = 0x100000000ULL; }
		}
		o.runOp[at] = text[p];
		o.runLen[at] = ovf ? 0u : (u32)v;
		o.runOvf[at] = ovf;
	}
}

__device__ __forceinline__ long long sam_shfl_xor(long long v, int off)
{
	const u32 lo = __shfl_xor((u32)v, off), hi = __shfl_xor((u32)((u64)v >> 32), off);
	return (long long)(((u64)hi << 32) | lo);
}

struct SamSums { long long mis, s; u32 firstOther, ovf; };		// firstOther: the first run that is not H

__device__ __forceinline__ void sam_add(SamSums& x, const SamOut& o, u32 k)
{
	const u32 op = o.runOp[k];
	const long long len = o.runLen[k];
	if (op == 'M' || op == 'I' || op == 'S') x.mis += len;
	if (op == 'S') x.s += len;
	if (op != 'H' && k < x.firstOther) x.firstOther = k;
	x.ovf |= o.runOvf[k];
}

// runs [a, b) of record r
__device__ __forceinline__ void sam_span_out(const SamSums& x, const SamOut& o, u32 r, u32 a, u32 b)
{
	const long long hardLeft = b > a && o.runOp[a] == 'H' ? (long long)o.runLen[a] : 0;
	const long long softLeft = x.firstOther < b && o.runOp[x.firstOther] == 'S' ? (long long)o.runLen[x.firstOther] : 0;
	o.qryStart[r] = hardLeft + softLeft;
	o.qryEnd[r] = x.mis + hardLeft - (x.s - softLeft);
	if (x.ovf) o.status[r] |= 16u;
}

// a lane per record of up to SAM_SPAN_CUT runs
__global__ void __launch_bounds__(SAM_BLOCK) k_sam_span(u32 nRec, u64 runBase, SamOut o)
{
	for (u64 r = (u64)blockIdx.x * SAM_BLOCK + threadIdx.x; r < nRec; r += (u64)gridDim.x * SAM_BLOCK)
	{
		const u32 a = (u32)(o.runOff[r] - runBase), b = (u32)(o.runOff[r + 1] - runBase);
		if (b - a > SAM_SPAN_CUT) continue;
		SamSums x{0, 0, SAM_NONE, 0};
		for (u32 k = a; k < b; ++k) sam_add(x, o, k);
		sam_span_out(x, o, (u32)r, a, b);
	}
}

// a wave per record of more runs: strided partial sums, then a reduction over the lanes
__global__ void __launch_bounds__(SAM_BLOCK) k_sam_span_wave(u32 nRec, u64 runBase, SamOut o)
{
	const int lane = threadIdx.x & 63;
	const u64 nWaves = (u64)gridDim.x * (SAM_BLOCK / 64);
	for (u64 r = (u64)blockIdx.x * (SAM_BLOCK / 64) + (threadIdx.x >> 6); r < nRec; r += nWaves)
	{
		const u32 a = fg_uni((u32)(o.runOff[r] - runBase)), b = fg_uni((u32)(o.runOff[r + 1] - runBase));
		if (b - a <= SAM_SPAN_CUT) continue;
		SamSums x{0, 0, SAM_NONE, 0};
		for (u32 k = a + lane; k < b; k += 64) sam_add(x, o, k);
		for (int off = 32; off > 0; off >>= 1)
		{
			x.mis += sam_shfl_xor(x.mis, off);
			x.s += sam_shfl_xor(x.s, off);
			x.firstOther = min(x.firstOther, (u32)__shfl_xor(x.firstOther, off));
			x.ovf |= (u32)__shfl_xor(x.ovf, off);
		}
		if (lane == 0) sam_span_out(x, o, (u32)r, a, b);
	}
}

// ---- host -----------------------------------------------------------------------------------------------------------
struct SamOwner {
	std::vector<uint64_t> chunkOff, lineNo, lineOff, tabOff, tokOff[4], runOff;
	std::vector<uint32_t> lineLen, tabLen, tokLen[4], runLen;
	std::vector<uint8_t> status, runOp;
	std::vector<int32_t> flag, pos;
	std::vector<int64_t> qryStart, qryEnd;
};

u32 samTile()
{
	const u64 t = std::min<u64>(std::max<u64>(stageEnvU64("FG_SAM_TILE", 4096), 256), 16384);
	u32 p = 256;
	while ((u64)p * 2 <= t) p *= 2;
	return p;
}

template <class T>
void samFetch(std::vector<T>& to, size_t at, const void* from, size_t count, hipStream_t s)
{
	if (count) HIP_CHECK(hipMemcpyAsync(to.data() + at, from, count * sizeof(T), hipMemcpyDeviceToHost, s));
}

struct SamCarry { bool have = false; u64 off = 0; u32 len = 0; };	// the tab RNAME of the last record so far

// one sub-batch of whole lines: text[at .. at + n), 0 < n <= 2^30
void samBatch(fg_ctx* c, SamOwner& own, const char* text, u64 at, u32 n, u32 tile, u64& nLinesAll, SamCarry& carry)
{
	hipStream_t s = c->stream;
	DevPool B(c->dSam, "sam");
	const u32 nTiles = (n + tile - 1) / tile;
	uint8_t* dText = B.get<uint8_t>((size_t)n + 2 * SAM_PIECE);
	u32* dTile = B.get<u32>(4 * ((size_t)nTiles + 1));			// newlines, tabs, token starts, run ends: + 1 for the totals
	u32 *dTileNl = dTile, *dTileTab = dTile + (nTiles + 1), *dTileTok = dTile + 2 * ((size_t)nTiles + 1), *dTileRun = dTile + 3 * ((size_t)nTiles + 1);
	u32* dRunPos = B.get<u32>((size_t)nTiles * (tile / 2));
	HIP_CHECK(hipMemcpyAsync(dText, text + at, n, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemsetAsync(dTile, 0, 4 * ((size_t)nTiles + 1) * 4, s));
	{
		ScopedK t(c->timer, "k_sam_classify");
		hipLaunchKernelGGL(k_sam_classify, nTiles, SAM_BLOCK, 0, s, (const uint8_t*)dText, n, tile, dTileNl, dTileTab, dTileTok);
	}
	u32* dScan = B.get<u32>(fgprim::scanScratchElems((u64)n + 1));	// every scan below is shorter
	{
		ScopedK t(c->timer, "k_sam_scan");
		fgprim::scan<u32>(s, dTileNl, dTileNl, (u64)nTiles + 1, false, dScan);
		fgprim::scan<u32>(s, dTileTab, dTileTab, (u64)nTiles + 1, false, dScan);
		fgprim::scan<u32>(s, dTileTok, dTileTok, (u64)nTiles + 1, false, dScan);
	}
	u32 nNl = 0;
	HIP_CHECK(hipMemcpyAsync(&nNl, dTileNl + nTiles, 4, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	const int lastIsNl = text[at + n - 1] == '\n';
	const u32 nLines = nNl + (lastIsNl ? 0 : 1);
	u32* dLine = B.get<u32>(6 * ((size_t)nLines + 1));			// start, tabs before, token starts before, record, runs, first run
	const size_t L1 = (size_t)nLines + 1;
	u32 *dLineStart = dLine, *dLineTab0 = dLine + L1, *dLineTok0 = dLine + 2 * L1, *dIsRec = dLine + 3 * L1, *dLineRuns = dLine + 4 * L1,
		*dLineR0 = dLine + 5 * L1;
	u32* dTable = B.get<u32>((size_t)nLines * SAM_WORDS);
	HIP_CHECK(hipMemsetAsync(dTable, 0xFF, (size_t)nLines * SAM_WORDS * 4, s));
	{
		ScopedK t(c->timer, "k_sam_lines");
		hipLaunchKernelGGL(k_sam_lines, nTiles, SAM_BLOCK, 0, s, (const uint8_t*)dText, n, tile, (const u32*)dTileNl, (const u32*)dTileTab,
						   (const u32*)dTileTok, nLines, lastIsNl, dLineStart, dLineTab0, dLineTok0);
	}
	{
		ScopedK t(c->timer, "k_sam_scatter");
		hipLaunchKernelGGL(k_sam_scatter, nTiles, SAM_BLOCK, 0, s, (const uint8_t*)dText, n, tile, (const u32*)dTileNl, (const u32*)dTileTab,
						   (const u32*)dTileTok, nLines, (const u32*)dLineTab0, (const u32*)dLineTok0, dTable, dRunPos, dTileRun);
	}
	{
		ScopedK t(c->timer, "k_sam_scan");
		fgprim::scan<u32>(s, dTileRun, dTileRun, (u64)nTiles + 1, false, dScan);
	}
	{
		ScopedK t(c->timer, "k_sam_record");
		hipLaunchKernelGGL(k_sam_record, samGrid(L1), SAM_BLOCK, 0, s, (const uint8_t*)dText, nLines, tile, (const u32*)dLineStart,
						   (const u32*)dTable, (const u32*)dTileRun, dIsRec, dLineRuns, dLineR0);
	}
	{
		ScopedK t(c->timer, "k_sam_scan");
		fgprim::scan<u32>(s, dIsRec, dIsRec, L1, false, dScan);
		fgprim::scan<u32>(s, dLineRuns, dLineRuns, L1, false, dScan);
	}
	u32 counts[3] = {0, 0, 0};									// listed run ends, records, runs
	HIP_CHECK(hipMemcpyAsync(&counts[0], dTileRun + nTiles, 4, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipMemcpyAsync(&counts[1], dIsRec + nLines, 4, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipMemcpyAsync(&counts[2], dLineRuns + nLines, 4, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipStreamSynchronize(s));
	const u32 nListed = counts[0], nRec = counts[1], nRuns = counts[2];
	const size_t recBase = own.lineNo.size(), runBase = own.runOp.size();

	SamOut o;
	u64* d64 = B.get<u64>(8 * (size_t)nRec + 1);				// line_no, line_off, tab_rname_off, four token offsets, run_off (+ 1)
	o.lineNo = d64; o.lineOff = d64 + nRec; o.tabOff = d64 + 2 * (size_t)nRec;
	for (int k = 0; k < 4; ++k) o.tokOff[k] = d64 + (3 + k) * (size_t)nRec;
	o.runOff = d64 + 7 * (size_t)nRec;
	long long* dSpan = B.get<long long>(2 * (size_t)nRec);
	o.qryStart = dSpan; o.qryEnd = dSpan + nRec;
	u32* d32 = B.get<u32>(8 * (size_t)nRec);					// line_len, tab_rname_len, four token lengths, flag, pos
	o.lineLen = d32; o.tabLen = d32 + nRec;
	for (int k = 0; k < 4; ++k) o.tokLen[k] = d32 + (2 + k) * (size_t)nRec;
	o.flag = (i32*)(d32 + 6 * (size_t)nRec); o.pos = (i32*)(d32 + 7 * (size_t)nRec);
	uint8_t* d8 = B.get<uint8_t>(2 * (size_t)nRec);
	o.status = d8; o.chunkFlag = d8 + nRec;
	o.runLen = B.get<u32>(nRuns);
	uint8_t* dRun8 = B.get<uint8_t>(2 * (size_t)nRuns);
	o.runOp = dRun8; o.runOvf = dRun8 + nRuns;
	{
		ScopedK t(c->timer, "k_sam_record");
		hipLaunchKernelGGL(k_sam_fields, samGrid(L1), SAM_BLOCK, 0, s, (const uint8_t*)dText, nLines, at, nLinesAll, (u64)runBase,
						   (const u32*)dLineStart, (const u32*)dTable, (const u32*)dIsRec, (const u32*)dLineRuns, o);
		if (nRec) hipLaunchKernelGGL(k_sam_chunk, samGrid(nRec), SAM_BLOCK, 0, s, (const uint8_t*)dText, nRec, at, o);
	}
	if (nListed)
	{
		ScopedK t(c->timer, "k_sam_runs");
		hipLaunchKernelGGL(k_sam_runs, samGrid(nListed), SAM_BLOCK, 0, s, (const uint8_t*)dText, nListed, nTiles, tile, (const u32*)dTileRun,
						   (const u32*)dRunPos, nLines, (const u32*)dLineStart, (const u32*)dLineR0, (const u32*)dLineRuns, nRuns, o);
	}
	if (nRec)
	{
		ScopedK t(c->timer, "k_sam_span");
		hipLaunchKernelGGL(k_sam_span, samGrid(nRec), SAM_BLOCK, 0, s, nRec, (u64)runBase, o);
		hipLaunchKernelGGL(k_sam_span_wave, samGrid((u64)nRec * 64), SAM_BLOCK, 0, s, nRec, (u64)runBase, o);
	}
	HIP_CHECK(hipGetLastError());

	const size_t nr = recBase + nRec;
	own.lineNo.resize(nr); own.lineOff.resize(nr); own.lineLen.resize(nr); own.status.resize(nr);
	own.tabOff.resize(nr); own.tabLen.resize(nr);
	for (int k = 0; k < 4; ++k) { own.tokOff[k].resize(nr); own.tokLen[k].resize(nr); }
	own.flag.resize(nr); own.pos.resize(nr); own.qryStart.resize(nr); own.qryEnd.resize(nr);
	own.runOff.resize(nr + 1);
	own.runOp.resize(runBase + nRuns); own.runLen.resize(runBase + nRuns);
	std::vector<uint8_t> chunkFlag(nRec);
	samFetch(own.lineNo, recBase, o.lineNo, nRec, s);
	samFetch(own.lineOff, recBase, o.lineOff, nRec, s);
	samFetch(own.lineLen, recBase, o.lineLen, nRec, s);
	samFetch(own.status, recBase, o.status, nRec, s);
	samFetch(own.tabOff, recBase, o.tabOff, nRec, s);
	samFetch(own.tabLen, recBase, o.tabLen, nRec, s);
	for (int k = 0; k < 4; ++k)
	{
		samFetch(own.tokOff[k], recBase, o.tokOff[k], nRec, s);
		samFetch(own.tokLen[k], recBase, o.tokLen[k], nRec, s);
	}
	samFetch(own.flag, recBase, o.flag, nRec, s);
	samFetch(own.pos, recBase, o.pos, nRec, s);
	samFetch(own.qryStart, recBase, o.qryStart, nRec, s);
	samFetch(own.qryEnd, recBase, o.qryEnd, nRec, s);
	samFetch(own.runOff, recBase, o.runOff, (size_t)nRec + 1, s);
	samFetch(own.runOp, runBase, o.runOp, nRuns, s);
	samFetch(own.runLen, runBase, o.runLen, nRuns, s);
	samFetch(chunkFlag, 0, o.chunkFlag, nRec, s);
	HIP_CHECK(hipStreamSynchronize(s));

	for (u32 r = 0; r < nRec; ++r)
	{
		bool opens = chunkFlag[r] != 0;
		if (r == 0)												// against the record before the cut: two short names, by offsets into the text
			opens = !carry.have || carry.len != own.tabLen[recBase] ||
					memcmp(text + carry.off, text + own.tabOff[recBase], carry.len) != 0;
		if (opens) own.chunkOff.push_back(recBase + r);
	}
	if (nRec) carry = SamCarry{true, own.tabOff[nr - 1], own.tabLen[nr - 1]};
	nLinesAll += nLines;
}

} // namespace

extern "C" {

int fg_sam_parse(fg_ctx* c, const char* text, uint64_t n_bytes, struct fg_sam_text* out)
{
	return stageCall<SamOwner>(c, out, [&](SamOwner*& own)
	{
		const std::string name = "fg_sam_parse";
		if (!out) throw FgError{FG_ERR_ARG, name + ": null result"};
		if (n_bytes && !text) throw FgError{FG_ERR_ARG, name + ": null text"};
		const u64 budget = std::min<u64>(std::max<u64>(stageEnvU64("FG_SAM_BATCH_BYTES", SAM_MAX_BATCH), 1), SAM_MAX_BATCH);
		const u32 tile = samTile();
		own = new SamOwner;
		own->runOff.assign(1, 0);
		u64 nLines = 0;
		SamCarry carry;
		HIP_CHECK(hipSetDevice(c->device));
		c->timer.reset();
		for (u64 at = 0; at < n_bytes;)
		{
			u64 n = n_bytes - at;
			if (n > budget)
			{
				// whole lines: the last newline inside the budget, one backward search
				const void* nl = memrchr(text + at, '\n', (size_t)budget);
				if (!nl)
					throw FgError{FG_ERR_NOMEM, name + ": the line at byte " + std::to_string(at) + " alone has more than " +
													std::to_string(budget) + " bytes, FG_SAM_BATCH_BYTES is " + std::to_string(budget)};
				n = (u64)((const char*)nl - (text + at)) + 1;
			}
			samBatch(c, *own, text, at, (u32)n, tile, nLines, carry);
			at += n;
		}
		c->timer.collect();
		const size_t nRec = own->lineNo.size();
		own->chunkOff.push_back(nRec);
		stageKeep(own->lineNo, own->lineOff, own->lineLen, own->status, own->tabOff, own->tabLen, own->flag, own->pos, own->qryStart,
				  own->qryEnd, own->runOp, own->runLen);
		for (int k = 0; k < 4; ++k) stageKeep(own->tokOff[k], own->tokLen[k]);
		out->n_lines = nLines;
		out->n_records = nRec;
		out->n_chunks = own->chunkOff.size() - 1;
		out->n_runs = own->runOp.size();
		out->chunk_off = own->chunkOff.data();
		out->line_no = own->lineNo.data(); out->line_off = own->lineOff.data(); out->line_len = own->lineLen.data();
		out->status = own->status.data();
		out->tab_rname_off = own->tabOff.data(); out->tab_rname_len = own->tabLen.data();
		out->qname_off = own->tokOff[0].data(); out->qname_len = own->tokLen[0].data();
		out->rname_off = own->tokOff[1].data(); out->rname_len = own->tokLen[1].data();
		out->cigar_off = own->tokOff[2].data(); out->cigar_len = own->tokLen[2].data();
		out->seq_off = own->tokOff[3].data(); out->seq_len = own->tokLen[3].data();
		out->flag = own->flag.data(); out->pos = own->pos.data();
		out->qry_start = own->qryStart.data(); out->qry_end = own->qryEnd.data();
		out->run_off = own->runOff.data(); out->run_op = own->runOp.data(); out->run_len = own->runLen.data();
		out->owner_ = own;
	});
}

void fg_release_sam_text(struct fg_sam_text* b) { stageRelease<SamOwner>(b); }

} // extern "C"
