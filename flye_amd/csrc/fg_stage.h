// What the stage calls of the C ABI share on the host (fg_uniform_alignments, fg_contig_consensus[_cigars],
// fg_make_bubbles[_cigars], fg_expand_cigars, fg_divergence_profile[_cigars], fg_confirm_positions,
// fg_classify_reads[_cigars], fg_paf_groups, fg_paf_circular, fg_sam_parse):
//   host part (no HIP: fg_error.h and include/flye_gpu.h alone; tests/stage_host_check.cpp builds it with g++)
//     stageEnvU64 / stageEnvCap             the u64 switches of the environment
//     stageOffsets .. stageColumnWalk       the argument checks; each takes the call's name, so a message reads the same
//                                           from every call
//     stageFits / stageAllFit / stageCut    whole items per sub-batch under a budget
//     stageKeep                             non-null pointers for empty result arrays
//   device part (hipcc only)
//     guarded                               the library's one catch ladder
//     stageCall / stageRelease              the frame of a stage call around its body, and its release
//     DevPool                               the buffers of one of the context's per-stage arrays, handed out in order
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../include/flye_gpu.h"
#include "fg_error.h"

// ---- switches ---------------------------------------------------------------------------------------------------
// base 10; something that is no number reads as 0
inline uint64_t stageEnvU64(const char* name, uint64_t dflt)
{
	const char* e = getenv(name);
	return e ? strtoull(e, nullptr, 10) : dflt;
}

// a switch for tests, items per sub-batch: present: max(1, value), absent: unlimited
inline uint64_t stageEnvCap(const char* name)
{
	const char* e = getenv(name);
	return e ? std::max<uint64_t>(1, strtoull(e, nullptr, 10)) : ~0ULL;
}

// ---- argument checks --------------------------------------------------------------------------------------------
// off[lo .. hi] does not decrease; item ("contig ", "alignment " or "") stands before the number in the text
inline void stageOffsets(const std::string& name, const char* what, const char* item, const uint64_t* off, uint64_t lo, uint64_t hi)
{
	for (uint64_t i = lo; i < hi; ++i)
		if (off[i + 1] < off[i]) throw FgError{FG_ERR_ARG, name + ": " + what + " decreases at " + item + std::to_string(i)};
}

// the contig table: per contig its length, then its offsets
inline void stageContigTable(const std::string& name, uint32_t nContigs, const int32_t* contigLen, const uint64_t* contigAlnOff)
{
	if (nContigs && (!contigLen || !contigAlnOff)) throw FgError{FG_ERR_ARG, name + ": null contig_len or contig_aln_off"};
	for (uint32_t i = 0; i < nContigs; ++i)
	{
		if (contigLen[i] < 0) throw FgError{FG_ERR_ARG, name + ": contig_len < 0 at contig " + std::to_string(i)};
		stageOffsets(name, "contig_aln_off", "contig ", contigAlnOff, i, (uint64_t)i + 1);
	}
}

// the kernels number an alignment's columns in 31 bits
inline void stageColWidth(const std::string& name, const uint64_t* colOff, uint64_t a)
{
	if (colOff[a + 1] - colOff[a] >= (1ULL << 31)) throw FgError{FG_ERR_ARG, name + ": an alignment of 2^31 columns"};
}

// alignments that have columns need both column arrays
inline void stageColsGiven(const std::string& name, const uint64_t* colOff, uint64_t lo, uint64_t hi, const uint8_t* trgCols, const uint8_t* qryCols)
{
	if (hi > lo && colOff[hi] > colOff[lo] && (!trgCols || !qryCols)) throw FgError{FG_ERR_ARG, name + ": null trg_cols or qry_cols"};
}

// col_off over the alignments lo .. hi: per alignment its offsets, its width and what the call adds (each(a)), then
// the column arrays
template <class Each>
inline void stageColOff(const std::string& name, const uint64_t* colOff, uint64_t lo, uint64_t hi, const uint8_t* trgCols, const uint8_t* qryCols,
						Each each)
{
	for (uint64_t a = lo; a < hi; ++a)
	{
		stageOffsets(name, "col_off", "alignment ", colOff, a, a + 1);
		stageColWidth(name, colOff, a);
		each(a);
	}
	stageColsGiven(name, colOff, lo, hi, trgCols, qryCols);
}

inline void stageColOff(const std::string& name, const uint64_t* colOff, uint64_t lo, uint64_t hi, const uint8_t* trgCols, const uint8_t* qryCols)
{
	stageColOff(name, colOff, lo, hi, trgCols, qryCols, [](uint64_t) {});
}

// one alignment's columns: every byte below 128; returns the non-gap target columns.  present[b], where given, marks
// the query bytes seen.
inline uint64_t stageColumnWalk(const std::string& name, uint64_t a, const uint64_t* colOff, const uint8_t* trgCols, const uint8_t* qryCols,
								bool* present = nullptr)
{
	uint64_t nonGap = 0;
	for (uint64_t k = colOff[a]; k < colOff[a + 1]; ++k)
	{
		if ((trgCols[k] | qryCols[k]) >= 128) throw FgError{FG_ERR_ARG, name + ": a byte >= 128 in alignment " + std::to_string(a)};
		nonGap += trgCols[k] != '-';
		if (present) present[qryCols[k]] = true;
	}
	return nonGap;
}

// trg_start lies on the contig
inline void stageStartOnContig(const std::string& name, uint64_t a, int32_t trgStart, int32_t contigLen)
{
	if (trgStart < 0 || trgStart >= contigLen) throw FgError{FG_ERR_ARG, name + ": trg_start outside the contig at alignment " + std::to_string(a)};
}

inline void stageBasesOnContig(const std::string& name, uint64_t a, uint64_t nonGap, int32_t contigLen)
{
	if (nonGap > (uint64_t)contigLen) throw FgError{FG_ERR_ARG, name + ": alignment " + std::to_string(a) + " has more target bases than its contig"};
}

// ---- sub-batches ------------------------------------------------------------------------------------------------
// a sub-batch holds whole items ("contig", "job", "alignment"), so one item's cost (in `unit`) has to fit the budget
inline void stageFits(const std::string& name, const char* item, uint64_t i, uint64_t cost, uint64_t budget, const char* unit, const char* budgetSwitch)
{
	if (cost > budget)
		throw FgError{FG_ERR_NOMEM, name + ": " + item + " " + std::to_string(i) + " alone has " + std::to_string(cost) + " " + unit + ", " +
										budgetSwitch + " is " + std::to_string(budget)};
}

inline void stageAllFit(const std::string& name, const char* item, const std::vector<uint64_t>& cost, uint64_t budget, const char* unit,
						const char* budgetSwitch)
{
	for (size_t i = 0; i < cost.size(); ++i) stageFits(name, item, i, cost[i], budget, unit, budgetSwitch);
}

// the end of the sub-batch that begins at item i: the longest run of whole items with a total cost of at most the
// budget and at most maxItems items; always at least one
inline uint32_t stageCut(uint32_t i, uint32_t n, const std::vector<uint64_t>& cost, uint64_t budget, uint64_t maxItems)
{
	uint32_t j = i;
	uint64_t used = 0;
	while (j < n && (j == i || (used + cost[j] <= budget && j - i < maxItems))) used += cost[j++];
	return j;
}

// ---- results ----------------------------------------------------------------------------------------------------
// an empty result array still hands the caller a non-null pointer
template <class... V>
inline void stageKeep(V&... v)
{
	((v.empty() ? v.reserve(1) : void()), ...);
}

#ifdef __HIPCC__
#include "fg_ctx.h"

// The catch ladder of every call of the C ABI: f's exception becomes lastError and a code.  Launches of a call that
// failed half way may be left behind on any stream: nothing of the context's scratch is reused before they have drained.
template <class F>
inline int guarded(fg_ctx* c, F f)
{
	int rc = FG_OK;
	try { f(); return FG_OK; }
	catch (const FgError& e) { if (c) c->lastError = e.msg; rc = e.code; }
	catch (const std::bad_alloc&) { if (c) c->lastError = "host allocation failed"; rc = FG_ERR_NOMEM; }
	catch (const std::exception& e) { if (c) c->lastError = e.what(); rc = FG_ERR_HIP; }
	for (fg_ctx* x : {c, c ? c->lane2.get() : (fg_ctx*)nullptr})		// the second lane of fg_overlaps has streams of its own
	{
		if (x && x->stream2) (void)hipStreamSynchronize(x->stream2);
		if (x && x->stream3) (void)hipStreamSynchronize(x->stream3);
		if (x && x->stream) (void)hipStreamSynchronize(x->stream);
	}
	return rc;
}

// The frame of a stage call: *out is zero unless the call succeeds.  body(own) checks the arguments (the null result
// among them, so the text carries the call's name), allocates the owner, runs the sub-batches and, as its last step,
// hands the owner's arrays over into *out.  After a failure the streams have drained, the timer is reset and the owner
// is gone.
template <class Owner, class Out, class Body>
inline int stageCall(fg_ctx* c, Out* out, Body body)
{
	if (!c) return FG_ERR_ARG;
	if (out) memset(out, 0, sizeof(*out));
	Owner* own = nullptr;
	const int rc = guarded(c, [&] { body(own); });
	if (rc != FG_OK)
	{
		c->timer.reset();
		delete own;
	}
	return rc;
}

template <class Owner, class Out>
inline void stageRelease(Out* b)
{
	if (!b) return;
	delete (Owner*)b->owner_;
	memset(b, 0, sizeof(*b));
}

// One of the context's per-stage buffer arrays (fg_ctx: dBub, dCc, dCig, dDv, dPt, dPaf, dSam), handed out in order from slot
// `start`; a buffer keeps its size between calls and only grows.
struct DevPool {
	DevBuf<char>* bufs;
	int n;
	const char* name;		// in the text of the internal error
	int next;
	template <size_t N>
	DevPool(DevBuf<char> (&a)[N], const char* name, int start = 0) : bufs(a), n((int)N), name(name), next(start) {}
	template <class T> T* get(size_t count)
	{
		if (next >= n) throw FgError{FG_ERR_HIP, std::string("internal: ") + name + " buffer pool too small"};
		DevBuf<char>& b = bufs[next++];
		b.reserve(count * sizeof(T) + 16);
		return (T*)b.p;
	}
};
#endif
