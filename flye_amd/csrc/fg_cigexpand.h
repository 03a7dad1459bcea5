// The expansion of SAM CIGAR runs into gapped columns (what fg_cigar.hip describes at its head), shared by
// fg_expand_cigars (fg_cigar.hip), which copies the columns down, and by fg_contig_consensus_cigars (fg_contigcons.hip),
// fg_make_bubbles_cigars (fg_bubbles.hip), fg_divergence_profile_cigars (fg_divergence.hip) and fg_classify_reads_cigars
// (fg_partition.hip), which expand straight into the buffers their own kernels read:
//   cigCheckRecords     the host walk over every run: argument errors, column totals, trg_start / trg_end, the query span.
//   cigExpandOnDevice   the device part of one sub-batch of whole alignments: k_cig_advance, the four scans, k_cig_place
//                       and k_cig_expand into destination pointers the caller gives.
//   cigCutContigs       where a sub-batch of whole contigs (or jobs) ends for a caller that expands per sub-batch.
#pragma once
#include "fg_ctx.h"
#include "fg_stage.h"
#include "fg_devprim.h"

namespace {		// kernels of a header shared by several translation units: one internal copy each

constexpr int CIG_BLOCK = 256;
constexpr int CIG_LANE_COLS = 8;
constexpr int CIG_MAX_TILE = 4096;
constexpr int CIG_DEFAULT_TILE = CIG_BLOCK * CIG_LANE_COLS;		// one pass of a full block
constexpr u32 CIG_ALN_MASK = (1u << 30) - 1u;
constexpr u32 CIG_NONE = 0xffffffffu;
constexpr u64 CIG_I32 = 0x7fffffffULL;
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

// the scratch of the expansion: the call's contig bytes in the pool's first buffer, then the buffers of one sub-batch
inline DevPool cigPool(fg_ctx* c, int start) { return DevPool{c->dCig, "fg_cigar", start}; }

// FG_CIGAR_TILE: a power of two in 64 .. 4096 (other values: the power of two below, inside that range)
inline u32 cigTile()
{
	u64 t = stageEnvU64("FG_CIGAR_TILE", CIG_DEFAULT_TILE);
	t = std::min<u64>(std::max<u64>(t, 64), CIG_MAX_TILE);
	u32 p = 64;
	while ((u64)p * 2 <= t) p *= 2;
	return p;
}

struct CigTotals { u64 cols, withCols; };		// columns; runs that have columns

// what the host walk finds per alignment; every array is indexed by the caller's alignment number (entries below the
// first alignment of the call stay zero), colOff has one more and starts at 0 at the first alignment
struct CigPlan {
	std::vector<CigTotals> tot;
	std::vector<u64> trgBase;				// first contig byte, in the call's contig bytes on the device
	std::vector<uint64_t> colOff;
	std::vector<int32_t> trgStart, trgEnd, qryStart, qryEnd, qryLen;
	u64 ctg0 = 0, nCtgBytes = 0;			// the call's contig bytes: contig_seq[ctg0 .. ctg0 + nCtgBytes)
};

// Every argument check of the expansion and _parse_cigar's walk (sam_parser.py:269-306, :316-320) for the alignments
// aFirst .. aEnd, alignment a on contig alnContig[a].  perAlnNull: one of the caller's per-alignment arrays is NULL
// (nullMsg names them).  Throws FgError; fills plan.
inline void cigCheckRecords(const std::string& name, u32 n_contigs, const uint64_t* contig_off, const uint8_t* contig_seq, u64 aFirst,
							u64 aEnd, const uint32_t* alnContig, bool perAlnNull, const char* nullMsg, const int32_t* ctg_pos,
							const uint64_t* run_off, const uint8_t* run_op, const uint32_t* run_len, const uint64_t* read_off,
							const uint8_t* read_seq, CigPlan& plan)
{
	const u64 nA = aEnd - aFirst;
	if (n_contigs && !contig_off) throw FgError{FG_ERR_ARG, name + ": null contig_off"};
	stageOffsets(name, "contig_off", "contig ", contig_off, 0, n_contigs);
	const u64 ctg0 = n_contigs ? contig_off[0] : 0, nCtgBytes = n_contigs ? contig_off[n_contigs] - ctg0 : 0;
	if (nCtgBytes && !contig_seq) throw FgError{FG_ERR_ARG, name + ": null contig_seq"};
	if (nA && perAlnNull) throw FgError{FG_ERR_ARG, name + ": " + nullMsg};
	for (u64 a = aFirst; a < aEnd; ++a)
	{
		if (run_off[a + 1] < run_off[a]) throw FgError{FG_ERR_ARG, name + ": run_off decreases at alignment " + std::to_string(a)};
		if (read_off[a + 1] < read_off[a]) throw FgError{FG_ERR_ARG, name + ": read_off decreases at alignment " + std::to_string(a)};
	}
	if (nA && run_off[aEnd] > run_off[aFirst] && (!run_op || !run_len)) throw FgError{FG_ERR_ARG, name + ": null run_op or run_len"};
	if (nA && read_off[aEnd] > read_off[aFirst] && !read_seq) throw FgError{FG_ERR_ARG, name + ": null read_seq"};
	for (u64 k = 0; k < nCtgBytes; ++k)
		if (contig_seq[ctg0 + k] >= 128) throw FgError{FG_ERR_ARG, name + ": a byte >= 128 in the contigs"};
	if (nA)
		for (u64 k = read_off[aFirst]; k < read_off[aEnd]; ++k)
			if (read_seq[k] >= 128) throw FgError{FG_ERR_ARG, name + ": a byte >= 128 in the reads"};

	plan.ctg0 = ctg0; plan.nCtgBytes = nCtgBytes;
	plan.colOff.assign((size_t)aEnd + 1, 0);
	for (auto* v : {&plan.trgStart, &plan.trgEnd, &plan.qryStart, &plan.qryEnd, &plan.qryLen}) v->assign((size_t)aEnd, 0);
	plan.tot.assign((size_t)aEnd, CigTotals{0, 0});
	plan.trgBase.assign((size_t)aEnd, 0);
	const u64 I32 = CIG_I32;
	for (u64 a = aFirst; a < aEnd; ++a)
	{
		const auto at = [a] { return " at alignment " + std::to_string(a); };
		if (alnContig[a] >= n_contigs) throw FgError{FG_ERR_ARG, name + ": aln_contig outside the contigs" + at()};
		if (ctg_pos[a] < 1) throw FgError{FG_ERR_ARG, name + ": ctg_pos < 1" + at()};
		const u64 ctgLen = contig_off[alnContig[a] + 1] - contig_off[alnContig[a]];
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
		plan.tot[a] = CigTotals{cols, withCols};
		plan.trgBase[a] = contig_off[alnContig[a]] - ctg0 + trgStart;
		plan.colOff[a + 1] = plan.colOff[a] + cols;
		plan.trgStart[a] = (int32_t)trgStart;
		plan.trgEnd[a] = (int32_t)(trgStart + tadv);
		// :316-320
		plan.qryStart[a] = (int32_t)(hardL + softL);
		plan.qryEnd[a] = (int32_t)((long long)(qpos + hardL) - (long long)softR);
		plan.qryLen[a] = (int32_t)(qpos + hardL + hardR);
	}
}

// the host arrays that the uploads of one expansion read
struct CigStaged { std::vector<u32> runBegin, alnRead; std::vector<u64> alnTrg; };

// The device part of one sub-batch of whole alignments a0 .. a1 (at most CIG_ALN_MASK of them, at most 2^31 - 1 columns,
// runs and read bytes): the runs and the SEQ bytes go up, the four kernels are queued on the context's stream.  The
// columns of the sub-batch go to dTrgOut / dQryOut from byte 0 on, whole 8-column words: both hold at least columns +
// CIG_LANE_COLS bytes (both NULL: the equal columns are counted and nothing is stored).  trgBase[a] is the alignment's
// first contig byte in dContig.  Returns the equal columns per alignment, on the device; nothing is waited for, so
// `staged` stays alive until the caller has synchronised the stream.  dReadsResident, where given, holds the SEQ bytes
// from readOff[a0] on already: nothing of readSeq goes up.
inline u32* cigExpandOnDevice(fg_ctx* c, DevPool& B, CigStaged& staged, u64 a0, u64 a1, const std::vector<CigTotals>& tot, const std::vector<u64>& trgBase,
							  const unsigned char* dContig, const uint64_t* runOff, const uint8_t* runOp, const uint32_t* runLen,
							  const uint64_t* readOff, const uint8_t* readSeq, u32 tile, unsigned char* dTrgOut, unsigned char* dQryOut,
							  const unsigned char* dReadsResident = nullptr)
{
	hipStream_t s = c->stream;
	const u32 nAln = (u32)(a1 - a0);
	const u64 r0 = runOff[a0], rd0 = readOff[a0];
	const u32 nRuns = (u32)(runOff[a1] - r0);
	const u64 nReadBytes = readOff[a1] - rd0;
	std::vector<u32>&runBegin = staged.runBegin, &alnRead = staged.alnRead;
	std::vector<u64>& alnTrg = staged.alnTrg;
	runBegin.assign((size_t)nAln + 1, 0); alnRead.assign(nAln, 0); alnTrg.assign(nAln, 0);
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

	unsigned char* dOp = B.get<unsigned char>(nRuns);
	u32* dLen = B.get<u32>(nRuns);
	u32* dAdv = B.get<u32>(4 * ((size_t)nRuns + 1));
	u32* dScan = B.get<u32>(fgprim::scanScratchElems((u64)nRuns + 1) + 8);
	u32* dRunBegin = B.get<u32>((size_t)nAln + 1);
	u32* dAlnRead = B.get<u32>(nAln);
	u64* dAlnTrg = B.get<u64>(nAln);
	CigRun* dRec = B.get<CigRun>(nRec);
	const unsigned char* dReads = dReadsResident ? (B.get<unsigned char>(0), dReadsResident) : B.get<unsigned char>(nReadBytes);
	u32* dMatches = B.get<u32>(nAln);
	u32 *dCol = dAdv, *dRead = dAdv + (nRuns + 1), *dTrg = dAdv + 2 * ((size_t)nRuns + 1), *dSlot = dAdv + 3 * ((size_t)nRuns + 1);

	HIP_CHECK(hipMemcpyAsync(dOp, runOp + r0, nRuns, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dLen, runLen + r0, (size_t)nRuns * 4, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dRunBegin, runBegin.data(), ((size_t)nAln + 1) * 4, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dAlnRead, alnRead.data(), (size_t)nAln * 4, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(dAlnTrg, alnTrg.data(), (size_t)nAln * 8, hipMemcpyHostToDevice, s));
	if (nReadBytes && !dReadsResident) HIP_CHECK(hipMemcpyAsync((void*)dReads, readSeq + rd0, nReadBytes, hipMemcpyHostToDevice, s));
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
	return dMatches;
}

// where a fused call's columns come from: the checked records of the call and its contig bytes on the device
struct CigSource {
	const CigPlan* plan;
	const unsigned char* dContig;
	const uint64_t* runOff; const uint8_t* runOp; const uint32_t* runLen;
	const uint64_t* readOff; const uint8_t* readSeq;
	u32 tile;
	const unsigned char* dSeq = nullptr;	// the call's SEQ bytes from read_seq[seq0] on, where they are on the device already
	u64 seq0 = 0;
};

// the contig bytes of a fused call go up once, into the first buffer of the expansion's pool
inline const unsigned char* cigUploadContigs(fg_ctx* c, const CigPlan& plan, const uint8_t* contigSeq)
{
	DevPool B = cigPool(c, 0);
	unsigned char* dContig = B.get<unsigned char>(plan.nCtgBytes);
	if (plan.nCtgBytes) HIP_CHECK(hipMemcpyAsync(dContig, contigSeq + plan.ctg0, plan.nCtgBytes, hipMemcpyHostToDevice, c->stream));
	return dContig;
}

// the columns of the alignments a0 .. a1 (a0 < a1) into dTrg / dQry (columns + CIG_LANE_COLS bytes each); the returned
// DevPool hands out the pool's buffers behind those the expansion uses
inline DevPool cigExpandSource(fg_ctx* c, const CigSource& src, CigStaged& staged, u64 a0, u64 a1, unsigned char* dTrg, unsigned char* dQry)
{
	DevPool B = cigPool(c, 1);
	(void)cigExpandOnDevice(c, B, staged, a0, a1, src.plan->tot, src.plan->trgBase, src.dContig, src.runOff, src.runOp, src.runLen, src.readOff,
							src.readSeq, src.tile, dTrg, dQry, src.dSeq ? src.dSeq + (src.readOff[a0] - src.seq0) : nullptr);
	return B;
}

// The end of the sub-batch of whole contigs that begins at contig i, for a call that expands each sub-batch itself: the
// consumer's budget (cost per contig, at most maxContigs contigs) and the expansion's numbering: the runs and read bytes
// of a sub-batch in 32 bits, an alignment's number in 30.  A contig that alone exceeds the numbering cannot be cut.
// fg_classify_reads_cigars cuts between jobs: `item` is "job" and contigAlnOff[j] the first alignment of job j's edges.
inline u32 cigCutContigs(const std::string& name, const char* budgetSwitch, u32 i, u32 n_contigs, const std::vector<u64>& cost, u64 budget,
						 u64 maxContigs, const uint64_t* contigAlnOff, const uint64_t* runOff, const uint64_t* readOff,
						 const char* item = "contig")
{
	const u64 aI = contigAlnOff[i];
	const auto fits = [&](u32 j)		// the contigs i .. j together
	{
		const u64 aJ = contigAlnOff[j + 1];
		return aJ == aI || (aJ - aI <= CIG_ALN_MASK && runOff[aJ] - runOff[aI] <= CIG_I32 && readOff[aJ] - readOff[aI] <= CIG_I32);
	};
	if (!fits(i) || cost[i] > CIG_I32)
		throw FgError{FG_ERR_NOMEM, name + ": " + item + " " + std::to_string(i) + " alone has 2^30 alignments or 2^31 columns, runs or SEQ bytes, " +
										"more than the expansion numbers in one sub-batch; " + budgetSwitch + " cuts between " + item + "s only"};
	const u64 most = std::min<u64>(budget, CIG_I32);		// the columns of a sub-batch are numbered in 32 bits too
	u32 j = i;
	u64 used = 0;
	while (j < n_contigs && (j == i || (used + cost[j] <= most && j - i < maxContigs && fits(j)))) used += cost[j++];
	return j;
}

} // namespace
