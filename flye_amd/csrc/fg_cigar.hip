// fg_expand_cigars: what SynchronizedSamReader._parse_cigar (flye/utils/sam_parser.py:260-323) does to one SAM record,
// for a batch of records on the device: CIGAR runs, the SEQ bytes and the contig bytes go up; the gapped strings (one
// byte per column, the layout fg_make_bubbles / fg_contig_consensus read) and the number of equal columns come back.
// fg_cigar_parse is the tokeniser in front of it (host only).
//
// An alignment has 10^3 - 10^5 columns in runs of a few columns each, so the work is cut by OUTPUT COLUMNS, not by
// alignment or run.  Per sub-batch of whole alignments (FG_CIGAR_BATCH_COLS, FG_CIGAR_BATCH_ALNS):
//   k_cig_advance   one thread per run: the columns, read bytes and contig bytes the run advances by (M 1 1 1, I 1 1 0,
//                   D 1 0 1, S 0 1 0, H 0 0 0, each times the length) and the flag "has columns".
//   (scan)          four exclusive sums over the flattened run array: where every run starts in the sub-batch's columns,
//                   read bytes and contig bytes, and its number among the runs that have columns.
//   k_cig_place     one thread per run with columns: its record (first column, first read byte in the sub-batch's SEQ
//                   bytes, first contig byte relative to the alignment's first, alignment | kind << 30) at that number.
//                   Runs without columns (S, H, length 0) are gone from here on: the first columns of the records
//                   ascend strictly, which is what the searches below need.
//   k_cig_expand    one workgroup per tile of FG_CIGAR_TILE consecutive columns of the sub-batch: the last record that
//                   starts at or before the tile by binary search; the first columns of the (at most tile) records that
//                   reach into it staged in LDS; a lane takes 8 consecutive columns, finds its first record in LDS, walks
//                   on from there, forms both bytes of every column (contig byte or '-', read byte or '-', a-z
//                   upper-cased) and stores them as one 8-byte word per string, consecutive lanes consecutive words.
//                   Equal columns: a lane counts per alignment; an alignment that begins and ends inside one lane is
//                   added by that lane; the counts of a lane's first and last alignment are summed over the wave per
//                   alignment (lanes ascend in alignment, so the smallest pending number is taken in turn), one integer
//                   atomic per (wave, alignment).  Integer sums do not depend on the order of arrival.
// The host validates every run once (the totals it needs for col_off anyway) and computes err_rate in double.
#include "fg_ctx.h"
#include "fg_devprim.h"

namespace {

constexpr int CIG_BLOCK = 256;
constexpr int CIG_LANE_COLS = 8;
constexpr int CIG_MAX_TILE = 4096;
constexpr int CIG_DEFAULT_TILE = CIG_BLOCK * CIG_LANE_COLS;		// one pass of a full block
constexpr u32 CIG_ALN_MASK = (1u << 30) - 1u;
constexpr u32 CIG_NONE = 0xffffffffu;
enum { CIG_M = 0, CIG_I = 1, CIG_D = 2 };

// a run that has columns; col ascends strictly over the array
struct CigRun { u32 col; u32 read; u32 trg; u32 alnKind; };

inline unsigned cigGrid(u64 n) { return (unsigned)((n + CIG_BLOCK - 1) / CIG_BLOCK); }

__global__ void __launch_bounds__(CIG_BLOCK)
k_cig_advance(u32 nRuns, const unsigned char* __restrict__ op, const u32* __restrict__ len, u32* __restrict__ advCol,
			  u32* __restrict__ advRead, u32* __restrict__ advTrg, u32* __restrict__ flag)
{
	const u32 r = blockIdx.x * CIG_BLOCK + threadIdx.x;
	if (r > nRuns) return;
	u32 c = 0, q = 0, t = 0;
	if (r < nRuns)
	{
		const unsigned char o = op[r];
		const u32 l = len[r];
		c = o == 'M' || o == 'I' || o == 'D' ? l : 0u;
		q = o == 'M' || o == 'I' || o == 'S' ? l : 0u;
		t = o == 'M' || o == 'D' ? l : 0u;
	}
	advCol[r] = c; advRead[r] = q; advTrg[r] = t; flag[r] = c ? 1u : 0u;
}

__global__ void __launch_bounds__(CIG_BLOCK)
k_cig_place(u32 nRuns, const unsigned char* __restrict__ op, const u32* __restrict__ col, const u32* __restrict__ read,
			const u32* __restrict__ trg, const u32* __restrict__ slot, const u32* __restrict__ runBegin, u32 nAln,
			const u32* __restrict__ alnRead, CigRun* __restrict__ out)
{
	const u32 r = blockIdx.x * CIG_BLOCK + threadIdx.x;
	if (r >= nRuns || slot[r + 1] == slot[r]) return;
	// the last alignment that begins at or before this run
	u32 lo = 0, hi = nAln;
	while (hi - lo > 1)
	{
		const u32 mid = (lo + hi) >> 1;
		if (runBegin[mid] <= r) lo = mid; else hi = mid;
	}
	const u32 first = runBegin[lo];
	const unsigned char o = op[r];
	const u32 kind = o == 'M' ? CIG_M : o == 'I' ? CIG_I : CIG_D;
	out[slot[r]] = CigRun{col[r], alnRead[lo] + (read[r] - read[first]), trg[r] - trg[first], lo | (kind << 30)};
}

__device__ __forceinline__ unsigned char cig_upper(unsigned char b) { return b >= 'a' && b <= 'z' ? (unsigned char)(b - 32) : b; }

__global__ void __launch_bounds__(CIG_BLOCK)
k_cig_expand(u32 nCols, u32 tile, const CigRun* __restrict__ runs, u32 nRec, const u64* __restrict__ alnTrg,
			 const unsigned char* __restrict__ contig, const unsigned char* __restrict__ reads, unsigned char* __restrict__ trgOut,
			 unsigned char* __restrict__ qryOut, u32* matches)
{
	__shared__ u32 sCol[CIG_MAX_TILE];
	const int lane = threadIdx.x & 63;
	const u32 t0 = blockIdx.x * tile;
	// the last record that starts at or before the tile (record 0 starts at column 0)
	u32 j0 = 0;
	{
		u32 hi = nRec;
		while (hi - j0 > 1)
		{
			const u32 mid = (j0 + hi) >> 1;
			if (runs[mid].col <= t0) j0 = mid; else hi = mid;
		}
	}
	// every record has a column, so at most `tile` of them reach into the tile
	const u32 cnt = nRec - j0 < tile ? nRec - j0 : tile;
	for (u32 i = threadIdx.x; i < cnt; i += blockDim.x) sCol[i] = runs[j0 + i].col;
	__syncthreads();

	for (u32 pass = 0; pass * blockDim.x * CIG_LANE_COLS < tile; ++pass)
	{
		const u32 base = (pass * blockDim.x + threadIdx.x) * CIG_LANE_COLS;
		const u32 c0 = t0 + base;
		// the lane's first and last alignment and their equal columns, for the wave's sums
		u32 a0 = CIG_NONE, m0 = 0, a1 = CIG_NONE, m1 = 0;
		if (base < tile && c0 < nCols)
		{
			u32 k = 0;
			{
				u32 hi = cnt;
				while (hi - k > 1)
				{
					const u32 mid = (k + hi) >> 1;
					if (sCol[mid] <= c0) k = mid; else hi = mid;
				}
			}
			CigRun d = runs[j0 + k];
			u32 a = d.alnKind & CIG_ALN_MASK, m = 0;
			u64 tb = alnTrg[a];
			a0 = a;
			bool first = true;			// still in the lane's first alignment
			u64 tw = 0, qw = 0;
#pragma unroll
			for (int i = 0; i < CIG_LANE_COLS; ++i)
			{
				const u32 c = c0 + (u32)i;
				unsigned char t = '-', q = '-';
				if (c < nCols)
				{
					while (k + 1 < cnt && sCol[k + 1] <= c)
					{
						d = runs[j0 + ++k];
						const u32 na = d.alnKind & CIG_ALN_MASK;
						if (na != a)
						{
							if (first) { m0 = m; first = false; }
							else if (m) atomicAdd(&matches[a], m);		// begins and ends inside this lane
							a = na; m = 0; tb = alnTrg[a];
						}
					}
					const u32 off = c - d.col, kind = d.alnKind >> 30;
					if (kind != CIG_I) t = cig_upper(contig[tb + d.trg + off]);
					if (kind != CIG_D) q = cig_upper(reads[d.read + off]);
					m += t == q ? 1u : 0u;
				}
				tw |= (u64)t << (8 * i);
				qw |= (u64)q << (8 * i);
			}
			if (first) m0 = m;
			else { a1 = a; m1 = m; }
			if (trgOut)
			{
				// the buffers are padded to a whole word past the last column
				*(u64*)(trgOut + c0) = tw;
				*(u64*)(qryOut + c0) = qw;
			}
		}
		// lanes ascend in alignment: the smallest pending number in turn, one atomic per (wave, alignment)
		while (__ballot(a0 != CIG_NONE || a1 != CIG_NONE))
		{
			u32 mn = a0 < a1 ? a0 : a1;
#pragma unroll
			for (int sh = 32; sh > 0; sh >>= 1) { const u32 o = __shfl_xor(mn, sh); mn = o < mn ? o : mn; }
			u32 s = (a0 == mn ? m0 : 0u) + (a1 == mn ? m1 : 0u);
#pragma unroll
			for (int sh = 32; sh > 0; sh >>= 1) s += __shfl_xor(s, sh);
			if (lane == 0 && s) atomicAdd(&matches[mn], s);
			if (a0 == mn) a0 = CIG_NONE;
			if (a1 == mn) a1 = CIG_NONE;
		}
	}
}

struct CigBufs {
	fg_ctx* c;
	int next;
	template <class T> T* get(size_t count)
	{
		if (next >= (int)(sizeof(c->dCig) / sizeof(c->dCig[0]))) throw FgError{FG_ERR_HIP, "internal: fg_cigar buffer pool too small"};
		DevBuf<char>& b = c->dCig[next++];
		b.reserve(count * sizeof(T) + 16);
		return (T*)b.p;
	}
};

struct ExpandOwner {
	std::vector<uint64_t> colOff;
	std::vector<uint8_t> trgCols, qryCols;
	std::vector<int32_t> trgStart, trgEnd, qryStart, qryEnd, qryLen;
	std::vector<int64_t> matches;
	std::vector<double> errRate;
};

u64 cigEnv(const char* name, u64 dflt)
{
	const char* e = getenv(name);
	return e ? strtoull(e, nullptr, 10) : dflt;
}

// FG_CIGAR_TILE: a power of two in 64 .. 4096 (other values: the power of two below, inside that range)
u32 cigTile()
{
	u64 t = cigEnv("FG_CIGAR_TILE", CIG_DEFAULT_TILE);
	t = std::min<u64>(std::max<u64>(t, 64), CIG_MAX_TILE);
	u32 p = 64;
	while ((u64)p * 2 <= t) p *= 2;
	return p;
}

struct CigTotals { u64 cols, withCols; };		// columns; runs that have columns

void cigSubBatch(fg_ctx* c, u64 a0, u64 a1, const std::vector<CigTotals>& tot, const std::vector<u64>& trgBase,
				 const unsigned char* dContig, const uint64_t* runOff, const uint8_t* runOp, const uint32_t* runLen,
				 const uint64_t* readOff, const uint8_t* readSeq, bool wantCols, u32 tile, ExpandOwner& own)
{
	hipStream_t s = c->stream;
	const u32 nAln = (u32)(a1 - a0);
	const u64 r0 = runOff[a0], rd0 = readOff[a0];
	const u32 nRuns = (u32)(runOff[a1] - r0);
	const u64 nReadBytes = readOff[a1] - rd0;
	std::vector<u32> runBegin((size_t)nAln + 1), alnRead(nAln);
	std::vector<u64> alnTrg(nAln);
	u64 nCols = 0, nRec = 0;
	for (u64 a = a0; a < a1; ++a)
	{
		runBegin[a - a0] = (u32)(runOff[a] - r0);
		alnRead[a - a0] = (u32)(readOff[a] - rd0);
		alnTrg[a - a0] = trgBase[a];
		nCols += tot[a].cols;
		nRec += tot[a].withCols;
	}
	runBegin[nAln] = nRuns;

	CigBufs B{c, 1};
	unsigned char* dOp = B.get<unsigned char>(nRuns);
	u32* dLen = B.get<u32>(nRuns);
	u32* dAdv = B.get<u32>(4 * ((size_t)nRuns + 1));
	u32* dScan = B.get<u32>(fgprim::scanScratchElems((u64)nRuns + 1) + 8);
	u32* dRunBegin = B.get<u32>((size_t)nAln + 1);
	u32* dAlnRead = B.get<u32>(nAln);
	u64* dAlnTrg = B.get<u64>(nAln);
	CigRun* dRec = B.get<CigRun>(nRec);
	unsigned char* dReads = B.get<unsigned char>(nReadBytes);
	u32* dMatches = B.get<u32>(nAln);
	// whole words: the lane that holds the last column stores all of its 8
	unsigned char* dTrgOut = wantCols ? B.get<unsigned char>(nCols + CIG_LANE_COLS) : nullptr;
	unsigned char* dQryOut = wantCols ? B.get<unsigned char>(nCols + CIG_LANE_COLS) : nullptr;
	u32 *dCol = dAdv, *dRead = dAdv + (nRuns + 1), *dTrg = dAdv + 2 * ((size_t)nRuns + 1), *dSlot = dAdv + 3 * ((size_t)nRuns + 1);

	HIP_CHECK(hipMemcpyAsync(dOp, runOp + r0, nRuns, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dLen, runLen + r0, (size_t)nRuns * 4, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dRunBegin, runBegin.data(), ((size_t)nAln + 1) * 4, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dAlnRead, alnRead.data(), (size_t)nAln * 4, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dAlnTrg, alnTrg.data(), (size_t)nAln * 8, hipMemcpyHostToDevice, s));
	if (nReadBytes) HIP_CHECK(hipMemcpyAsync(dReads, readSeq + rd0, nReadBytes, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemsetAsync(dMatches, 0, (size_t)nAln * 4, s));
	{
		ScopedK t(c->timer, "k_cig_advance");
		hipLaunchKernelGGL(k_cig_advance, cigGrid((u64)nRuns + 1), CIG_BLOCK, 0, s, nRuns, dOp, dLen, dCol, dRead, dTrg, dSlot);
	}
	{
		ScopedK t(c->timer, "k_cig_scan");
		for (u32* p : {dCol, dRead, dTrg, dSlot}) fgprim::scan<u32>(s, p, p, (u64)nRuns + 1, false, dScan);
	}
	{
		ScopedK t(c->timer, "k_cig_place");
		hipLaunchKernelGGL(k_cig_place, cigGrid(nRuns), CIG_BLOCK, 0, s, nRuns, dOp, dCol, dRead, dTrg, dSlot, dRunBegin, nAln, dAlnRead, dRec);
	}
	{
		ScopedK t(c->timer, "k_cig_expand");
		const unsigned block = (unsigned)std::min<u32>(CIG_BLOCK, std::max<u32>(64, tile / CIG_LANE_COLS));
		hipLaunchKernelGGL(k_cig_expand, (unsigned)((nCols + tile - 1) / tile), block, 0, s, (u32)nCols, tile, dRec, (u32)nRec, dAlnTrg, dContig,
						   dReads, dTrgOut, dQryOut, dMatches);
	}
	HIP_CHECK(hipGetLastError());
	std::vector<u32> m(nAln);
	HIP_CHECK(hipMemcpyAsync(m.data(), dMatches, (size_t)nAln * 4, hipMemcpyDeviceToHost, s));
	if (wantCols)
	{
		const u64 at = own.colOff[a0];
		HIP_CHECK(hipMemcpyAsync(own.trgCols.data() + at, dTrgOut, nCols, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipMemcpyAsync(own.qryCols.data() + at, dQryOut, nCols, hipMemcpyDeviceToHost, s));
	}
	HIP_CHECK(hipStreamSynchronize(s));
	for (u32 i = 0; i < nAln; ++i) own.matches[a0 + i] = (int64_t)m[i];
}

bool cigIsOp(unsigned char b) { return b == 'M' || b == 'I' || b == 'D' || b == 'N' || b == 'S' || b == 'H' || b == 'P' || b == '=' || b == 'X'; }

} // namespace

extern "C" {

int fg_cigar_parse(const char* cigar, uint64_t n_bytes, uint8_t* ops, uint32_t* lens, uint64_t cap, uint64_t* n_runs)
{
	if (n_runs) *n_runs = 0;
	if (!n_runs || (n_bytes && !cigar) || (cap && (!ops || !lens))) return FG_ERR_ARG;
	const unsigned char* p = (const unsigned char*)cigar;
	u64 n = 0, i = 0;
	bool tooLong = false;
	while (i < n_bytes)
	{
		if (p[i] < '0' || p[i] > '9') { ++i; continue; }
		u64 v = 0;
		bool big = false;
		u64 j = i;
		for (; j < n_bytes && p[j] >= '0' && p[j] <= '9'; ++j)
		{
			v = v * 10 + (u64)(p[j] - '0');
			if (v > 0xffffffffULL) { big = true; v = 0xffffffffULL; }
		}
		// digits that no operation follows match nothing; the byte behind them is looked at again
		if (j < n_bytes && cigIsOp(p[j]))
		{
			if (big) tooLong = true;
			if (n < cap) { ops[n] = p[j]; lens[n] = (u32)v; }
			++n;
			++j;
		}
		i = j;
	}
	*n_runs = n;
	return n > cap || tooLong ? FG_ERR_ARG : FG_OK;
}

int fg_expand_cigars(fg_ctx* c, uint32_t n_contigs, const uint64_t* contig_off, const uint8_t* contig_seq, uint64_t n_alignments,
					 const uint32_t* aln_contig, const int32_t* ctg_pos, const uint64_t* run_off, const uint8_t* run_op,
					 const uint32_t* run_len, const uint64_t* read_off, const uint8_t* read_seq, uint8_t want_cols,
					 struct fg_expand_batch* out)
{
	if (!c) return FG_ERR_ARG;
	if (out) memset(out, 0, sizeof(*out));
	ExpandOwner* own = nullptr;
	int rc = FG_OK;
	try
	{
		const std::string name = "fg_expand_cigars";
		const u64 nA = n_alignments;
		if (!out) throw FgError{FG_ERR_ARG, name + ": null result"};
		if (n_contigs && !contig_off) throw FgError{FG_ERR_ARG, name + ": null contig_off"};
		for (u32 i = 0; i < n_contigs; ++i)
			if (contig_off[i + 1] < contig_off[i]) throw FgError{FG_ERR_ARG, name + ": contig_off decreases at contig " + std::to_string(i)};
		const u64 ctg0 = n_contigs ? contig_off[0] : 0, nCtgBytes = n_contigs ? contig_off[n_contigs] - ctg0 : 0;
		if (nCtgBytes && !contig_seq) throw FgError{FG_ERR_ARG, name + ": null contig_seq"};
		if (nA && (!aln_contig || !ctg_pos || !run_off || !read_off)) throw FgError{FG_ERR_ARG, name + ": null aln_contig, ctg_pos, run_off or read_off"};
		for (u64 a = 0; a < nA; ++a)
		{
			if (run_off[a + 1] < run_off[a]) throw FgError{FG_ERR_ARG, name + ": run_off decreases at alignment " + std::to_string(a)};
			if (read_off[a + 1] < read_off[a]) throw FgError{FG_ERR_ARG, name + ": read_off decreases at alignment " + std::to_string(a)};
		}
		if (nA && run_off[nA] > run_off[0] && (!run_op || !run_len)) throw FgError{FG_ERR_ARG, name + ": null run_op or run_len"};
		if (nA && read_off[nA] > read_off[0] && !read_seq) throw FgError{FG_ERR_ARG, name + ": null read_seq"};
		for (u64 k = 0; k < nCtgBytes; ++k)
			if (contig_seq[ctg0 + k] >= 128) throw FgError{FG_ERR_ARG, name + ": a byte >= 128 in the contigs"};
		if (nA)
			for (u64 k = read_off[0]; k < read_off[nA]; ++k)
				if (read_seq[k] >= 128) throw FgError{FG_ERR_ARG, name + ": a byte >= 128 in the reads"};

		own = new ExpandOwner;
		own->colOff.assign((size_t)nA + 1, 0);
		for (auto* v : {&own->trgStart, &own->trgEnd, &own->qryStart, &own->qryEnd, &own->qryLen}) v->assign((size_t)nA, 0);
		own->matches.assign((size_t)nA, 0);
		own->errRate.assign((size_t)nA, 0.0);
		std::vector<CigTotals> tot((size_t)nA);
		std::vector<u64> trgBase((size_t)nA);
		const u64 I32 = 0x7fffffffULL;
		for (u64 a = 0; a < nA; ++a)
		{
			const auto at = [a] { return " at alignment " + std::to_string(a); };
			if (aln_contig[a] >= n_contigs) throw FgError{FG_ERR_ARG, name + ": aln_contig outside the contigs" + at()};
			if (ctg_pos[a] < 1) throw FgError{FG_ERR_ARG, name + ": ctg_pos < 1" + at()};
			const u64 ctgLen = contig_off[aln_contig[a] + 1] - contig_off[aln_contig[a]];
			if (run_off[a + 1] - run_off[a] > I32) throw FgError{FG_ERR_ARG, name + ": 2^31 runs" + at()};
			// _parse_cigar's walk (sam_parser.py:269-306)
			bool leftHard = true, leftSoft = true;
			u64 hardL = 0, hardR = 0, softL = 0, softR = 0, cols = 0, qpos = 0, tadv = 0, withCols = 0;
			for (u64 r = run_off[a]; r < run_off[a + 1]; ++r)
			{
				const u64 l = run_len[r];
				switch (run_op[r])
				{
				case 'H': (leftHard ? hardL : hardR) += l; break;
				case 'S': qpos += l; (leftSoft ? softL : softR) += l; break;
				case 'M': cols += l; qpos += l; tadv += l; withCols += l != 0; break;
				case 'I': cols += l; qpos += l; withCols += l != 0; break;
				case 'D': cols += l; tadv += l; withCols += l != 0; break;
				case 'N': case 'P': case '=': case 'X':
					throw FgError{FG_ERR_UNSUPPORTED, name + ": CIGAR operation " + std::string(1, (char)run_op[r]) + at()};
				default:
					throw FgError{FG_ERR_ARG, name + ": byte " + std::to_string((int)run_op[r]) + " is no CIGAR operation" + at()};
				}
				leftHard = false;
				if (run_op[r] != 'H') leftSoft = false;
			}
			const u64 trgStart = (u64)ctg_pos[a] - 1;
			if (cols > I32 || qpos + hardL + hardR > I32 || trgStart + tadv > I32)
				throw FgError{FG_ERR_ARG, name + ": totals beyond int32" + at()};
			if (qpos > read_off[a + 1] - read_off[a])
				throw FgError{FG_ERR_ARG, name + ": the runs consume " + std::to_string(qpos) + " read bytes, SEQ holds " +
											  std::to_string(read_off[a + 1] - read_off[a]) + at()};
			if (trgStart + tadv > ctgLen) throw FgError{FG_ERR_ARG, name + ": the runs walk past the end of the contig" + at()};
			if (cols == 0) throw FgError{FG_ERR_ARG, name + ": no columns" + at()};
			tot[a] = CigTotals{cols, withCols};
			trgBase[a] = contig_off[aln_contig[a]] - ctg0 + trgStart;
			own->colOff[a + 1] = own->colOff[a] + cols;
			own->trgStart[a] = (int32_t)trgStart;
			own->trgEnd[a] = (int32_t)(trgStart + tadv);
			// :316-320
			own->qryStart[a] = (int32_t)(hardL + softL);
			own->qryEnd[a] = (int32_t)((long long)(qpos + hardL) - (long long)softR);
			own->qryLen[a] = (int32_t)(qpos + hardL + hardR);
		}
		const u64 budget = std::min<u64>(cigEnv("FG_CIGAR_BATCH_COLS", 1ULL << 27), I32);
		u64 maxAlns = CIG_ALN_MASK;			// a record carries the alignment's number in 30 bits
		if (getenv("FG_CIGAR_BATCH_ALNS")) maxAlns = std::min<u64>(maxAlns, std::max<u64>(1, cigEnv("FG_CIGAR_BATCH_ALNS", 1)));
		for (u64 a = 0; a < nA; ++a)
			if (tot[a].cols > budget)
				throw FgError{FG_ERR_NOMEM, name + ": alignment " + std::to_string(a) + " alone has " + std::to_string(tot[a].cols) +
												" columns, FG_CIGAR_BATCH_COLS is " + std::to_string(budget)};
		if (want_cols)
		{
			own->trgCols.resize((size_t)own->colOff[nA]);
			own->qryCols.resize((size_t)own->colOff[nA]);
		}
		const u32 tile = cigTile();
		HIP_CHECK(hipSetDevice(c->device));
		c->timer.reset();
		if (nA)
		{
			// the contig bytes go up once per call
			CigBufs B{c, 0};
			unsigned char* dContig = B.get<unsigned char>(nCtgBytes);
			if (nCtgBytes) HIP_CHECK(hipMemcpyAsync(dContig, contig_seq + ctg0, nCtgBytes, hipMemcpyHostToDevice, c->stream));
			u64 i = 0;
			while (i < nA)
			{
				u64 j = i, cols = 0;
				// columns, runs and read bytes of a sub-batch are numbered in 32 bits
				while (j < nA && (j == i || (cols + tot[j].cols <= budget && j - i < maxAlns && run_off[j + 1] - run_off[i] <= I32 &&
											 read_off[j + 1] - read_off[i] <= I32)))
					cols += tot[j++].cols;
				if (read_off[j] - read_off[i] > I32) throw FgError{FG_ERR_ARG, name + ": a SEQ of 2^31 bytes at alignment " + std::to_string(i)};
				cigSubBatch(c, i, j, tot, trgBase, dContig, run_off, run_op, run_len, read_off, read_seq, want_cols != 0, tile, *own);
				i = j;
			}
		}
		c->timer.collect();
		for (u64 a = 0; a < nA; ++a) own->errRate[a] = 1.0 - (double)own->matches[a] / (double)tot[a].cols;
		for (auto* v : {&own->trgCols, &own->qryCols})
			if (v->empty()) v->reserve(1);
		for (auto* v : {&own->trgStart, &own->trgEnd, &own->qryStart, &own->qryEnd, &own->qryLen})
			if (v->empty()) v->reserve(1);
		if (own->matches.empty()) own->matches.reserve(1);
		if (own->errRate.empty()) own->errRate.reserve(1);
	}
	catch (const FgError& e) { c->lastError = e.msg; rc = e.code; }
	catch (const std::bad_alloc&) { c->lastError = "host allocation failed"; rc = FG_ERR_NOMEM; }
	catch (const std::exception& e) { c->lastError = e.what(); rc = FG_ERR_HIP; }
	if (rc != FG_OK)
	{
		// launches of a call that failed half way drain before the context's scratch is used again
		if (c->stream) (void)hipStreamSynchronize(c->stream);
		c->timer.reset();
		delete own;
		return rc;
	}
	out->n_alignments = n_alignments;
	out->col_off = own->colOff.data();
	if (want_cols)
	{
		out->trg_cols = own->trgCols.data();
		out->qry_cols = own->qryCols.data();
	}
	out->trg_start = own->trgStart.data();
	out->trg_end = own->trgEnd.data();
	out->qry_start = own->qryStart.data();
	out->qry_end = own->qryEnd.data();
	out->qry_len = own->qryLen.data();
	out->matches = own->matches.data();
	out->err_rate = own->errRate.data();
	out->owner_ = own;
	return FG_OK;
}

void fg_release_expand(struct fg_expand_batch* b)
{
	if (!b) return;
	delete (ExpandOwner*)b->owner_;
	memset(b, 0, sizeof(*b));
}

} // extern "C"
