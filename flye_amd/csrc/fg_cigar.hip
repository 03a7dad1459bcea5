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
// The kernels, the host walk and the device part of a sub-batch live in fg_cigexpand.h: fg_contig_consensus_cigars and
// fg_make_bubbles_cigars expand with them straight into the buffers of their own kernels.
#include "fg_ctx.h"
#include "fg_devprim.h"
#include "fg_cigexpand.h"		// the kernels, the host walk and the device part of a sub-batch, shared with the fused calls

namespace {

struct ExpandOwner {
	std::vector<uint64_t> colOff;
	std::vector<uint8_t> trgCols, qryCols;
	std::vector<int32_t> trgStart, trgEnd, qryStart, qryEnd, qryLen;
	std::vector<int64_t> matches;
	std::vector<double> errRate;
};

void cigSubBatch(fg_ctx* c, u64 a0, u64 a1, const std::vector<CigTotals>& tot, const std::vector<u64>& trgBase,
				 const unsigned char* dContig, const uint64_t* runOff, const uint8_t* runOp, const uint32_t* runLen,
				 const uint64_t* readOff, const uint8_t* readSeq, bool wantCols, u32 tile, ExpandOwner& own)
{
	hipStream_t s = c->stream;
	const u32 nAln = (u32)(a1 - a0);
	u64 nCols = 0;
	for (u64 a = a0; a < a1; ++a) nCols += tot[a].cols;
	DevPool B = cigPool(c, 1);
	// whole words: the lane that holds the last column stores all of its 8
	unsigned char* dTrgOut = wantCols ? B.get<unsigned char>(nCols + CIG_LANE_COLS) : nullptr;
	unsigned char* dQryOut = wantCols ? B.get<unsigned char>(nCols + CIG_LANE_COLS) : nullptr;
	CigStaged staged;
	const u32* dMatches = cigExpandOnDevice(c, B, staged, a0, a1, tot, trgBase, dContig, runOff, runOp, runLen, readOff, readSeq, tile,
											dTrgOut, dQryOut);
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
	return stageCall<ExpandOwner>(c, out, [&](ExpandOwner*& own)
	{
		const std::string name = "fg_expand_cigars";
		const u64 nA = n_alignments;
		if (!out) throw FgError{FG_ERR_ARG, name + ": null result"};
		CigPlan plan;
		cigCheckRecords(name, n_contigs, contig_off, contig_seq, 0, nA, aln_contig, !aln_contig || !ctg_pos || !run_off || !read_off,
						"null aln_contig, ctg_pos, run_off or read_off", ctg_pos, run_off, run_op, run_len, read_off, read_seq, plan);
		const u64 ctg0 = plan.ctg0, nCtgBytes = plan.nCtgBytes, I32 = CIG_I32;
		const std::vector<CigTotals>& tot = plan.tot;
		const std::vector<u64>& trgBase = plan.trgBase;
		own = new ExpandOwner;
		own->colOff = std::move(plan.colOff);
		own->trgStart = std::move(plan.trgStart); own->trgEnd = std::move(plan.trgEnd);
		own->qryStart = std::move(plan.qryStart); own->qryEnd = std::move(plan.qryEnd); own->qryLen = std::move(plan.qryLen);
		own->matches.assign((size_t)nA, 0);
		own->errRate.assign((size_t)nA, 0.0);
		const u64 budget = std::min<u64>(stageEnvU64("FG_CIGAR_BATCH_COLS", 1ULL << 27), I32);
		const u64 maxAlns = std::min<u64>(CIG_ALN_MASK, stageEnvCap("FG_CIGAR_BATCH_ALNS"));		// a record carries the alignment's number in 30 bits
		for (u64 a = 0; a < nA; ++a) stageFits(name, "alignment", a, tot[a].cols, budget, "columns", "FG_CIGAR_BATCH_COLS");
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
			DevPool B = cigPool(c, 0);
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
		stageKeep(own->trgCols, own->qryCols, own->trgStart, own->trgEnd, own->qryStart, own->qryEnd, own->qryLen, own->matches, own->errRate);

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
	});
}

void fg_release_expand(struct fg_expand_batch* b) { stageRelease<ExpandOwner>(b); }

} // extern "C"
