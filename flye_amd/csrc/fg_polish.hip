// fg_polish_bubbles: the bubble polishing of flye-modules polisher (reference src/polishing: BubbleProcessor::
// parallelWorker, GeneralPolisher::polishBubble / makeStep, Alignment, DinucleotideFixer::fixBubble) on the device.
// Integers only: scores are the int64 of the substitution matrix, and every sum and maximum is exact.
//
// The host drives the step loop.  A round takes every bubble that is still at work: a bubble inside optimize() gives
// one item (its current candidate against the branch list of its phase: the sorted middle five, or all), a bubble at
// the dinucleotide decision gives three score-only items (candidate, increased, decreased).  The items of a round are
// cut into chunks under the scratch budget; per chunk three launches:
//   k_pol_fill    one wave per (item, branch, direction): F (and R, on the reversed strings) row by row.  Lanes own
//                 the columns of a piece of 64; the horizontal move of a row is a max-plus prefix scan: with P[j] the
//                 border row F[0][j] and T[j] the maximum of the vertical and diagonal terms, F[i][j] = P[j] +
//                 max_{k <= j} (T[k] - P[k]) -- one wave scan per piece and a carry between pieces.  A lane reads
//                 back only cells it wrote itself; the diagonal neighbour comes by shuffle.
//   k_pol_edits   one wave per (item, position p): for every branch the nine maxima over the columns (deletion of
//                 v[p], four insertions before p, four substitutions of v[p]) out of F[p], R[L - p] and R[L - 1 - p],
//                 summed over the branches in list order by one lane.  No atomics.
//   k_pol_select  one wave per item: A(v) = sum of F[L][Lb] (0 where L or Lb is 0), then makeStep's choice: the first
//                 maximum above A among the deletions, else among the insertions (p, then A C G T), else among the
//                 substitutions, as (kind, position, letter, score).
// The host applies the edit to its copy of the candidate, records the step and decides how optimize() goes on.  Nothing
// stays on the device between rounds but the branches, so the result cannot depend on how the rounds were cut.
// Scratch per item: 8 bytes per cell of F and of R, (L + 1) * (Lb + 1) cells per branch each, plus 72 (L + 1) for the
// edit sums.
#include "fg_ctx.h"
#include "fg_stage.h"
#include "../../include/introsort_emul.h"

namespace {

#define POL_BLOCK 256
#define POL_WAVES (POL_BLOCK / 64)
#define POL_MIN ((long long)0x8000000000000000LL)

typedef long long i64;

// mode 0: a makeStep item (F, R, edits, selection); 1: score only (F and A)
struct PolItem { u64 candOff; u64 taskOff; u64 edOff; u32 L, nb, mode, pad; };
struct PolTask { u64 cellOff; u32 item, branch; };
struct PolRes { i64 score; i32 kind, pos, letter, pad; };

__device__ __forceinline__ int pol_cls(unsigned char b)
{
	return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : b == '-' ? 5 : 4;
}

__device__ __forceinline__ i64 pol_shfl(i64 v, int lane)
{
	const u32 lo = __shfl((u32)v, lane), hi = __shfl((u32)((u64)v >> 32), lane);
	return (i64)(((u64)hi << 32) | lo);
}
__device__ __forceinline__ i64 pol_shfl_up(i64 v, int d)
{
	const u32 lo = __shfl_up((u32)v, d), hi = __shfl_up((u32)((u64)v >> 32), d);
	return (i64)(((u64)hi << 32) | lo);
}
__device__ __forceinline__ i64 pol_shfl_xor(i64 v, int d)
{
	const u32 lo = __shfl_xor((u32)v, d), hi = __shfl_xor((u32)((u64)v >> 32), d);
	return (i64)(((u64)hi << 32) | lo);
}
__device__ __forceinline__ i64 pol_max(i64 a, i64 b) { return a > b ? a : b; }

__device__ __forceinline__ void pol_load_scores(i64* sS, const i64* __restrict__ score)
{
	if (threadIdx.x < 36) sS[threadIdx.x] = score[threadIdx.x];
	__syncthreads();
}

__global__ void __launch_bounds__(POL_BLOCK)
k_pol_fill(const i64* __restrict__ score, const PolItem* __restrict__ items, const PolTask* __restrict__ tasks, u64 nTasks,
		   const unsigned char* __restrict__ cand, const unsigned char* __restrict__ br, const u64* __restrict__ brOff, i64* cells)
{
	__shared__ i64 sS[36];
	pol_load_scores(sS, score);
	const int lane = threadIdx.x & 63;
	const u64 unit = (u64)blockIdx.x * POL_WAVES + (threadIdx.x >> 6);
	const u64 t = unit >> 1;
	const bool rev = unit & 1;
	if (t >= nTasks) return;
	const PolTask tk = tasks[t];
	const PolItem it = items[tk.item];
	if (rev && it.mode) return;
	const long long L = it.L;
	const u64 w0 = brOff[tk.branch];
	const long long Lb = (long long)(brOff[tk.branch + 1] - w0);
	const long long stride = Lb + 1;
	const unsigned char* v = cand + it.candOff;
	const unsigned char* w = br + w0;
	i64* out = cells + tk.cellOff + (rev ? (u64)(L + 1) * (u64)stride : 0);
	// row 0: the running sum of s(gap, w[j - 1])
	i64 carry = 0;
	for (long long c0 = 0; c0 <= Lb; c0 += 64)
	{
		const long long j = c0 + lane;
		const bool valid = j <= Lb;
		i64 g = 0;
		if (valid && j >= 1) g = sS[5 * 6 + pol_cls(rev ? w[Lb - j] : w[j - 1])];
		for (int d = 1; d < 64; d <<= 1)
		{
			const i64 o = pol_shfl_up(g, d);
			if (lane >= d) g += o;
		}
		g += carry;
		if (valid) out[j] = g;
		carry = pol_shfl(g, 63);
	}
	for (long long i = 1; i <= L; ++i)
	{
		const int vc = pol_cls(rev ? v[L - i] : v[i - 1]);
		const i64 sDel = sS[vc * 6 + 5];
		i64* prevRow = out + (u64)(i - 1) * (u64)stride;
		i64* curRow = out + (u64)i * (u64)stride;
		i64 diagCarry = 0, runMax = POL_MIN;
		for (long long c0 = 0; c0 <= Lb; c0 += 64)
		{
			const long long j = c0 + lane;
			const bool valid = j <= Lb;
			const i64 up = valid ? prevRow[j] : 0;
			const i64 P = valid ? out[j] : 0;
			i64 dg = pol_shfl_up(up, 1);
			if (lane == 0) dg = diagCarry;
			diagCarry = pol_shfl(up, 63);
			i64 x = POL_MIN;
			if (valid)
			{
				i64 T = up + sDel;
				if (j >= 1) T = pol_max(T, dg + sS[vc * 6 + pol_cls(rev ? w[Lb - j] : w[j - 1])]);
				x = T - P;
			}
			for (int d = 1; d < 64; d <<= 1)
			{
				const i64 o = pol_shfl_up(x, d);
				if (lane >= d) x = pol_max(x, o);
			}
			x = pol_max(x, runMax);
			if (valid) curRow[j] = P + x;
			runMax = pol_shfl(x, 63);
		}
	}
}

// edOffs: nItems + 1 offsets into ed, 9 per position of a mode-0 item, none for a score-only item
__global__ void __launch_bounds__(POL_BLOCK)
k_pol_edits(const i64* __restrict__ score, const PolItem* __restrict__ items, u32 nItems, const u64* __restrict__ edOffs,
			const PolTask* __restrict__ tasks, const unsigned char* __restrict__ br, const u64* __restrict__ brOff,
			const i64* __restrict__ cells, i64* __restrict__ ed)
{
	__shared__ i64 sS[36];
	pol_load_scores(sS, score);
	const int lane = threadIdx.x & 63;
	const u64 unit = (u64)blockIdx.x * POL_WAVES + (threadIdx.x >> 6);
	if (unit * 9 >= edOffs[nItems]) return;
	// the last item whose offset is <= 9 * unit (an item without positions shares its offset with the next one)
	u32 lo = 0, hi = nItems;
	while (hi - lo > 1)
	{
		const u32 mid = (lo + hi) >> 1;
		if (edOffs[mid] <= unit * 9) lo = mid; else hi = mid;
	}
	const PolItem it = items[lo];
	const long long L = it.L;
	const long long p = (long long)(unit - it.edOff / 9);
	if (it.mode || p > L) return;
	i64 acc[9];
	for (int e = 0; e < 9; ++e) acc[e] = 0;
	for (u32 k = 0; k < it.nb; ++k)
	{
		const PolTask tk = tasks[it.taskOff + k];
		const u64 w0 = brOff[tk.branch];
		const long long Lb = (long long)(brOff[tk.branch + 1] - w0);
		const long long stride = Lb + 1;
		const unsigned char* w = br + w0;
		const i64* F = cells + tk.cellOff + (u64)p * (u64)stride;
		const i64* R = cells + tk.cellOff + (u64)(L + 1) * (u64)stride;
		const i64* rIns = R + (u64)(L - p) * (u64)stride;
		const i64* rSub = R + (u64)(p < L ? L - 1 - p : 0) * (u64)stride;
		i64 m[9];
		for (int e = 0; e < 9; ++e) m[e] = POL_MIN;
		for (long long j = lane; j <= Lb; j += 64)
		{
			const i64 f0 = F[j];
			const i64 rI = rIns[Lb - j], rS = rSub[Lb - j];
			const i64 fm1 = j ? F[j - 1] : 0;
			const int wc = j ? pol_cls(w[j - 1]) : 0;
			m[0] = pol_max(m[0], f0 + rS);
			for (int b = 0; b < 4; ++b)
			{
				i64 sub = f0 + sS[b * 6 + 5];
				if (j) sub = pol_max(sub, fm1 + sS[b * 6 + wc]);
				m[1 + b] = pol_max(m[1 + b], sub + rI);
				m[5 + b] = pol_max(m[5 + b], sub + rS);
			}
		}
		for (int e = 0; e < 9; ++e)
		{
			i64 x = m[e];
			for (int d = 32; d > 0; d >>= 1) x = pol_max(x, pol_shfl_xor(x, d));
			acc[e] += x;
		}
	}
	if (lane == 0)
	{
		i64* o = ed + it.edOff + 9 * (u64)p;
		for (int e = 0; e < 9; ++e) o[e] = (p == L && (e == 0 || e >= 5)) ? POL_MIN : acc[e];
	}
}

// (score, index): the greater score, at equal scores the smaller index
__device__ __forceinline__ void pol_first_max(i64& s, long long& idx)
{
	for (int d = 32; d > 0; d >>= 1)
	{
		const i64 os = pol_shfl_xor(s, d);
		const long long oi = pol_shfl_xor((i64)idx, d);
		if (os > s || (os == s && oi < idx)) { s = os; idx = oi; }
	}
}

__global__ void __launch_bounds__(64)
k_pol_select(const PolItem* __restrict__ items, const PolTask* __restrict__ tasks, const unsigned char* __restrict__ cand,
			 const u64* __restrict__ brOff, const i64* __restrict__ cells, const i64* __restrict__ ed, PolRes* __restrict__ res)
{
	const int lane = threadIdx.x;
	const PolItem it = items[blockIdx.x];
	const long long L = it.L;
	i64 A = 0;
	for (u32 k = lane; k < it.nb; k += 64)
	{
		const PolTask tk = tasks[it.taskOff + k];
		const long long Lb = (long long)(brOff[tk.branch + 1] - brOff[tk.branch]);
		// getScoringMatrix returns its untouched 0 when either string is empty
		if (L > 0 && Lb > 0) A += cells[tk.cellOff + (u64)L * (u64)(Lb + 1) + (u64)Lb];
	}
	for (int d = 32; d > 0; d >>= 1) A += pol_shfl_xor(A, d);
	PolRes r;
	r.score = A; r.kind = 0; r.pos = 0; r.letter = 0; r.pad = 0;
	if (!it.mode)
	{
		const i64* e = ed + it.edOff;
		const unsigned char* v = cand + it.candOff;
		const long long NONE = 0x7FFFFFFFFFFFFFFFLL;
		i64 s = POL_MIN; long long idx = NONE;
		for (long long p = lane; p < L; p += 64)
		{
			const i64 x = e[9 * p];
			if (x > s) { s = x; idx = p; }
		}
		pol_first_max(s, idx);
		if (idx != NONE && s > A) { r.score = s; r.kind = 1; r.pos = (i32)idx; }
		else
		{
			s = POL_MIN; idx = NONE;
			for (long long q = lane; q < 4 * (L + 1); q += 64)
			{
				const i64 x = e[9 * (q >> 2) + 1 + (q & 3)];
				if (x > s) { s = x; idx = q; }
			}
			pol_first_max(s, idx);
			if (idx != NONE && s > A) { r.score = s; r.kind = 2; r.pos = (i32)(idx >> 2); r.letter = (i32)(idx & 3); }
			else
			{
				s = POL_MIN; idx = NONE;
				for (long long q = lane; q < 4 * L; q += 64)
				{
					if (pol_cls(v[q >> 2]) == (int)(q & 3)) continue;		// the letter the candidate already has
					const i64 x = e[9 * (q >> 2) + 5 + (q & 3)];
					if (x > s) { s = x; idx = q; }
				}
				pol_first_max(s, idx);
				if (idx != NONE && s > A) { r.score = s; r.kind = 3; r.pos = (i32)(idx >> 2); r.letter = (i32)(idx & 3); }
			}
		}
	}
	if (lane == 0) res[blockIdx.x] = r;
}

// DinucleotideFixer::getDinucleotideRuns: (position, run) of the longest run of a pair of two different bases that a
// different pair ends
std::pair<long long, long long> polDinucleotideRun(const std::string& s)
{
	long long maxRun = 0, maxPos = 0;
	if (s.size() < 2) return {0, 0};
	for (size_t shift = 0; shift < 2; ++shift)
	{
		char p0 = '-', p1 = '-';
		long long run = 0;
		for (size_t pos = 0; pos < (s.size() - shift) / 2; ++pos)
		{
			const char c0 = s[pos * 2 + shift], c1 = s[pos * 2 + shift + 1];
			if (c0 != p0 || c1 != p1)
			{
				if (run > maxRun && p0 != p1) { maxRun = run; maxPos = (long long)(pos * 2 + shift) - run * 2; }
				run = 1; p0 = c0; p1 = c1;
			}
			else ++run;
		}
	}
	return {maxPos, maxRun};
}

struct PolLenSort {
	typedef u32 T;
	std::vector<u32>& ids;
	const u64* off;
	T load(int i) const { return ids[i]; }
	void store(int i, const T& x) { ids[i] = x; }
	bool less(const T& a, const T& b) const { return off[a + 1] - off[a] < off[b + 1] - off[b]; }
};

struct PolBubble {
	std::string cand, inc, dec;
	std::vector<u32> mid;		// the pre-polish branches
	u64 sumAll = 0, sumMid = 0;	// sums of Lb + 1 over the branch lists
	int phase = 3;				// 0: pre-polish, 1: all branches, 2: the dinucleotide decision, 3: done
	size_t iter = 0, len0 = 0;
};

struct PolWork { u32 bubble; u32 mode; const std::string* cand; };

} // namespace

void fgPolishBubbles(fg_ctx* c, const int64_t* score36, const uint8_t* cand, const uint64_t* candOff, const uint8_t* branches,
					 const uint64_t* branchOff, const uint64_t* bubbleBranchOff, u32 nBubbles, bool fixDinucleotides, bool wantSteps,
					 std::vector<std::string>& outCand, std::vector<uint32_t>& nSteps, std::vector<uint8_t>& status,
					 std::vector<std::vector<std::pair<std::string, int64_t>>>& steps)
{
	outCand.resize(nBubbles); nSteps.assign(nBubbles, 0); status.assign(nBubbles, 0);
	steps.clear(); steps.resize(wantSteps ? nBubbles : 0);
	if (!nBubbles) return;
	hipStream_t s = c->stream;
	const u64 budget = stageEnvU64("FG_POLISH_SCRATCH_BYTES", 8ULL << 30);
	const u64 maxItems = stageEnvCap("FG_POLISH_BATCH_BUBBLES");		// a switch for tests: bubbles at work per chunk
	const u64 br0 = bubbleBranchOff[0], nBr = bubbleBranchOff[nBubbles] - br0;
	const u64 byte0 = nBr ? branchOff[br0] : 0, nBytes = nBr ? branchOff[br0 + nBr] - byte0 : 0;
	if (nBr >= (1ULL << 32)) throw FgError{FG_ERR_ARG, "fg_polish_bubbles: more than 2^32 - 1 branches in one call"};

	std::vector<PolBubble> B(nBubbles);
	std::vector<u64> localOff(nBr + 1);
	for (u64 r = 0; r <= nBr; ++r) localOff[r] = branchOff[br0 + r] - byte0;
	std::vector<int> stack(fgsort::STACK_INTS);
	for (u32 i = 0; i < nBubbles; ++i)
	{
		PolBubble& b = B[i];
		b.cand.assign((const char*)cand + candOff[i], (size_t)(candOff[i + 1] - candOff[i]));
		const u64 r0 = bubbleBranchOff[i] - br0, nb = bubbleBranchOff[i + 1] - bubbleBranchOff[i];
		// parallelWorker's rule
		if (!(b.cand.size() < 5000 && nb > 1)) { status[i] = 1; continue; }
		for (u64 r = r0; r < r0 + nb; ++r) b.sumAll += localOff[r + 1] - localOff[r] + 1;
		b.phase = 1;
		if (nb > 10)
		{
			// std::sort by length with libstdc++'s permutation, then the five around the middle
			std::vector<u32> ids(nb);
			for (u64 k = 0; k < nb; ++k) ids[k] = (u32)(r0 + k);
			PolLenSort acc{ids, localOff.data()};
			fgsort::sort(acc, 0, (int)nb, stack.data());
			const size_t left = nb / 2 - 2;
			b.mid.assign(ids.begin() + left, ids.begin() + left + 5);
			for (u32 r : b.mid) b.sumMid += localOff[r + 1] - localOff[r] + 1;
			b.phase = 0;
		}
		b.len0 = b.cand.size();
	}

	c->timer.reset();
	c->dPolBytes.reserve(nBytes);
	c->dPolOff.reserve(nBr + 1);
	c->dPolScore.reserve(36);
	if (nBytes) HIP_CHECK(hipMemcpyAsync(c->dPolBytes.p, branches + byte0, nBytes, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(c->dPolOff.p, localOff.data(), (nBr + 1) * 8, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(c->dPolScore.p, score36, 36 * 8, hipMemcpyHostToDevice, s));

	auto finishOptimize = [&](u32 i)
	{
		PolBubble& b = B[i];
		if (b.phase == 0) { b.phase = 1; b.iter = 0; b.len0 = b.cand.size(); return; }
		b.phase = 3;
		if (!fixDinucleotides) return;
		const auto run = polDinucleotideRun(b.cand);
		if (run.second < 3) return;
		b.inc = b.cand; b.inc.insert((size_t)run.first, b.cand.substr((size_t)run.first, 2));
		b.dec = b.cand; b.dec.erase((size_t)run.first, 2);
		b.phase = 2;
	};
	auto record = [&](u32 i, const std::string& seq, int64_t sc)
	{
		++nSteps[i];
		if (wantSteps) steps[i].emplace_back(seq, sc);
	};

	std::vector<PolWork> work;
	std::vector<PolItem> items;
	std::vector<PolTask> tasks;
	std::vector<u64> edOffs;
	std::vector<PolRes> res;
	std::string bytes;
	const char LETTERS[4] = {'A', 'C', 'G', 'T'};
	for (;;)
	{
		work.clear();
		for (u32 i = 0; i < nBubbles; ++i)
		{
			const PolBubble& b = B[i];
			if (b.phase == 0 || b.phase == 1) work.push_back(PolWork{i, 0, &b.cand});
			else if (b.phase == 2)
				for (const std::string* q : {&b.cand, &b.inc, &b.dec}) work.push_back(PolWork{i, 1, q});
		}
		if (work.empty()) break;
		size_t wa = 0;
		while (wa < work.size())
		{
			// a chunk: whole bubbles (the three items of a decision stay together) under the budget
			items.clear(); tasks.clear(); edOffs.clear(); bytes.clear();
			u64 cellsUsed = 0, edUsed = 0, nChunkBubbles = 0;
			size_t wb = wa;
			while (wb < work.size())
			{
				const u32 i = work[wb].bubble;
				size_t we = wb;
				u64 cellsNeed = 0, edNeed = 0;
				while (we < work.size() && work[we].bubble == i)
				{
					const PolBubble& b = B[i];
					const u64 L1 = work[we].cand->size() + 1;
					cellsNeed += L1 * (b.phase == 0 ? b.sumMid : b.sumAll) * (work[we].mode ? 1 : 2);
					if (!work[we].mode) edNeed += 9 * L1;
					++we;
				}
				if (wb > wa && ((cellsUsed + cellsNeed + edUsed + edNeed) * 8 > budget || nChunkBubbles >= maxItems)) break;
				if ((cellsNeed + edNeed) * 8 > budget)
					throw FgError{FG_ERR_NOMEM, "fg_polish_bubbles: bubble " + std::to_string(i) + " alone needs " +
												std::to_string((cellsNeed + edNeed) * 8) + " bytes of scratch, FG_POLISH_SCRATCH_BYTES is " +
												std::to_string(budget)};
				for (; wb < we; ++wb)
				{
					const PolBubble& b = B[i];
					const std::string& v = *work[wb].cand;
					PolItem it;
					it.candOff = bytes.size(); it.taskOff = tasks.size(); it.edOff = edUsed;
					it.L = (u32)v.size(); it.mode = work[wb].mode; it.pad = 0;
					bytes += v;
					const u64 L1 = v.size() + 1;
					const u32 item = (u32)items.size();
					auto addTask = [&](u32 r)
					{
						tasks.push_back(PolTask{cellsUsed, item, r});
						cellsUsed += L1 * (localOff[r + 1] - localOff[r] + 1) * (it.mode ? 1 : 2);
					};
					if (b.phase == 0) for (u32 r : b.mid) addTask(r);
					else
						for (u64 r = bubbleBranchOff[i] - br0; r < bubbleBranchOff[i + 1] - br0; ++r) addTask((u32)r);
					it.nb = (u32)(tasks.size() - it.taskOff);
					edOffs.push_back(edUsed);
					if (!it.mode) edUsed += 9 * L1;
					items.push_back(it);
				}
				++nChunkBubbles;
			}
			edOffs.push_back(edUsed);
			const u32 nItems = (u32)items.size();
			const u64 nTasks = tasks.size();
			if (nTasks >= (1ULL << 31)) throw FgError{FG_ERR_ARG, "fg_polish_bubbles: more than 2^31 - 1 branch alignments in one chunk"};
			c->dPolCand.reserve(bytes.size());
			c->dPolItems.reserve((size_t)nItems * sizeof(PolItem));
			c->dPolTasks.reserve((size_t)nTasks * sizeof(PolTask));
			c->dPolEdOff.reserve(edOffs.size());
			c->dPolCells.reserve(cellsUsed);
			c->dPolEdits.reserve(edUsed);
			c->dPolRes.reserve((size_t)nItems * sizeof(PolRes));
			if (!bytes.empty()) HIP_CHECK(hipMemcpyAsync(c->dPolCand.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice, s));
			HIP_CHECK(hipMemcpyAsync(c->dPolItems.p, items.data(), (size_t)nItems * sizeof(PolItem), hipMemcpyHostToDevice, s));
			HIP_CHECK(hipMemcpyAsync(c->dPolTasks.p, tasks.data(), (size_t)nTasks * sizeof(PolTask), hipMemcpyHostToDevice, s));
			HIP_CHECK(hipMemcpyAsync(c->dPolEdOff.p, edOffs.data(), edOffs.size() * 8, hipMemcpyHostToDevice, s));
			const PolItem* dItems = (const PolItem*)c->dPolItems.p;
			const PolTask* dTasks = (const PolTask*)c->dPolTasks.p;
			const unsigned char* dCand = (const unsigned char*)c->dPolCand.p;
			const unsigned char* dBr = (const unsigned char*)c->dPolBytes.p;
			{
				ScopedK t(c->timer, "k_pol_fill");
				hipLaunchKernelGGL(k_pol_fill, (unsigned)((2 * nTasks + POL_WAVES - 1) / POL_WAVES), POL_BLOCK, 0, s,
								   (const i64*)c->dPolScore.p, dItems, dTasks, nTasks, dCand, dBr, (const u64*)c->dPolOff.p,
								   (i64*)c->dPolCells.p);
			}
			if (edUsed)
			{
				ScopedK t(c->timer, "k_pol_edits");
				hipLaunchKernelGGL(k_pol_edits, (unsigned)((edUsed / 9 + POL_WAVES - 1) / POL_WAVES), POL_BLOCK, 0, s,
								   (const i64*)c->dPolScore.p, dItems, nItems, (const u64*)c->dPolEdOff.p, dTasks, dBr,
								   (const u64*)c->dPolOff.p, (const i64*)c->dPolCells.p, (i64*)c->dPolEdits.p);
			}
			{
				ScopedK t(c->timer, "k_pol_select");
				hipLaunchKernelGGL(k_pol_select, nItems, 64, 0, s, dItems, dTasks, dCand, (const u64*)c->dPolOff.p,
								   (const i64*)c->dPolCells.p, (const i64*)c->dPolEdits.p, (PolRes*)c->dPolRes.p);
			}
			HIP_CHECK(hipGetLastError());
			res.resize(nItems);
			HIP_CHECK(hipMemcpyAsync(res.data(), c->dPolRes.p, (size_t)nItems * sizeof(PolRes), hipMemcpyDeviceToHost, s));
			HIP_CHECK(hipStreamSynchronize(s));

			for (size_t k = 0; k < nItems; )
			{
				const u32 i = work[wa + k].bubble;
				PolBubble& b = B[i];
				if (work[wa + k].mode)
				{
					// fixBubble: the longer form first
					const i64 normal = res[k].score, increased = res[k + 1].score, decreased = res[k + 2].score;
					if (increased > normal) { b.cand = b.inc; status[i] |= 8; record(i, b.cand, 0); }
					else if (decreased > normal) { b.cand = b.dec; status[i] |= 8; record(i, b.cand, 0); }
					b.phase = 3;
					k += 3;
					continue;
				}
				const PolRes& r = res[k];
				std::string seq = b.cand;
				if (r.kind == 1) seq.erase((size_t)r.pos, 1);
				else if (r.kind == 2) seq.insert((size_t)r.pos, 1, LETTERS[r.letter]);
				else if (r.kind == 3) seq[(size_t)r.pos] = LETTERS[r.letter];
				record(i, seq, r.score);
				if (r.kind == 0) finishOptimize(i);
				else if (r.score > 0) { status[i] |= 2; finishOptimize(i); }
				else if (b.iter++ > 10 * b.len0) { status[i] |= 4; finishOptimize(i); }
				else b.cand.swap(seq);
				++k;
			}
			wa = wb;
		}
	}
	c->timer.collect();
	for (u32 i = 0; i < nBubbles; ++i) outCand[i].swap(B[i].cand);
}
