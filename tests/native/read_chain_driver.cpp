// The edge-chain step of a read aligner, stated literally on the host: the yardstick of tests/test_read_chains.py and
// the host side of tools/read_chain_bench.py.  Chains are objects that hold vectors of alignment pointers, they live in
// two std::deques and are copied wherever the behaviour fg_chain_alignments documents copies them; both orderings are
// the real std::sort on those objects.
//
//   read_chain_driver IN OUT [threads] [repeats]
//
// IN : int32 params[6] (max_jump, max_read_overlap, min_alignment, max_separation, long_edge, big_alignment),
//      uint32 first_ext_id, n_ext_ids, n_queries, 0, uint64 n_recs, uint32 node_left[n_ext_ids], node_right[n_ext_ids],
//      uint64 query_off[n_queries + 1] (from 0), int32 recs[n_recs][7] (cur_begin, cur_end, ext_begin, ext_end, ext_len,
//      score, ext_id)
// OUT: uint64 n_chains, n_alns, cleanups, first sorts of more than 16 elements with a tied key, second sorts likewise,
//      chains rejected for overlapping an accepted one; uint64 chain_off[n_queries + 1], aln_off[n_chains + 1],
//      aln[n_alns]; int32 score[n_chains]
// stdout: "seconds <best wall time of the repeats>"
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <set>
#include <thread>
#include <vector>

namespace {

struct Params { int32_t maxJump, maxReadOverlap, minAlignment, maxSeparation, longEdge, bigAlignment; };

struct Rec { int32_t curBegin, curEnd, extBegin, extEnd, extLen, score; uint32_t extId; };

struct EdgeAln {
	Rec o;
	uint32_t nodeLeft, nodeRight;
	uint64_t index;		// in the caller's array
};

struct Chain {
	std::vector<const EdgeAln*> aln;
	int32_t score;
};

struct Counters { uint64_t cleanups = 0, tiedFirst = 0, tiedSecond = 0, rejected = 0; };

struct QueryResult {
	std::vector<std::vector<uint64_t>> chains;
	std::vector<int32_t> scores;
};

template <class It, class Key>
bool hasTie(It b, It e, Key key)
{
	std::multiset<int64_t> seen;
	for (It i = b; i != e; ++i) seen.insert(key(*i));
	for (auto it = seen.begin(); it != seen.end(); ++it)
		if (seen.count(*it) > 1) return true;
	return false;
}

int32_t addWrapped(int32_t a, int32_t b, int32_t c)		// a + b - c as 32-bit two's complement
{
	return (int32_t)((uint32_t)a + (uint32_t)b - (uint32_t)c);
}

std::vector<Chain> chainOneRead(const std::vector<EdgeAln>& sorted, const Params& P, Counters& cnt)
{
	std::deque<Chain> active, frozen;
	for (const EdgeAln& cur : sorted)
	{
		int32_t bestScore = 0;
		Chain* bestChain = nullptr;
		int outdatedSeen = 0;
		const bool mayExtend = cur.o.extBegin < P.maxJump;
		const bool mayBeExtended = cur.o.extLen - cur.o.extEnd < P.maxJump;
		if (mayExtend)
		{
			for (Chain& ch : active)
			{
				const EdgeAln& last = *ch.aln.back();
				const int32_t readGap = cur.o.curBegin - last.o.curEnd;
				const int32_t leftGap = cur.o.extBegin;
				const int32_t rightGap = last.o.extLen - last.o.extEnd;
				const bool joined = last.nodeRight == cur.nodeLeft;
				if (joined && P.maxJump > readGap && readGap > -P.maxReadOverlap && leftGap + rightGap < P.maxJump)
				{
					const int32_t disagreement = std::abs(readGap - (leftGap + rightGap));
					const int32_t penalty = disagreement > 100 ? disagreement / 50 : 0;
					const int32_t total = addWrapped(ch.score, cur.o.score, penalty);
					if (total > bestScore) { bestScore = total; bestChain = &ch; }
				}
				if (readGap > P.maxJump) ++outdatedSeen;
			}
		}
		if (bestChain)
		{
			active.push_back(*bestChain);		// a copy: the chain that was extended stays where it is
			active.back().aln.push_back(&cur);
			active.back().score = bestScore;
		}
		else
		{
			Chain fresh{{&cur}, cur.o.score};
			if (mayBeExtended) active.push_back(fresh); else frozen.push_back(fresh);
		}
		if (outdatedSeen > (int)active.size() / 2)
		{
			++cnt.cleanups;
			auto keepAt = active.begin();
			for (auto it = active.begin(); it != active.end(); ++it)
			{
				if (cur.o.curBegin - it->aln.back()->o.curEnd > P.maxJump) frozen.push_back(*it);
				else
				{
					if (keepAt != it) *keepAt = *it;
					++keepAt;
				}
			}
			active.erase(keepAt, active.end());
		}
	}
	active.insert(active.end(), frozen.begin(), frozen.end());
	if (active.size() > 16 && hasTie(active.begin(), active.end(), [](const Chain& c) { return (int64_t)c.score; })) ++cnt.tiedSecond;
	std::sort(active.begin(), active.end(), [](const Chain& a, const Chain& b) { return a.score > b.score; });

	std::vector<Chain> accepted;
	for (const Chain& ch : active)
	{
		const int32_t begin = ch.aln.front()->o.curBegin, end = ch.aln.back()->o.curEnd;
		if (end - begin < P.minAlignment) continue;
		bool clash = false;
		for (const Chain& have : accepted)
		{
			const int32_t hb = have.aln.front()->o.curBegin, he = have.aln.back()->o.curEnd;
			if (std::min(end, he) - std::max(begin, hb) > P.maxSeparation) clash = true;
		}
		if (clash) { ++cnt.rejected; continue; }
		accepted.push_back(ch);
	}
	return accepted;
}

struct Input {
	Params P;
	uint32_t firstExt = 0, nExt = 0, nq = 0;
	uint64_t nRecs = 0;
	std::vector<uint32_t> nodeLeft, nodeRight;
	std::vector<uint64_t> queryOff;
	std::vector<Rec> recs;
};

void runQuery(const Input& in, uint32_t q, QueryResult& out, Counters& cnt)
{
	std::vector<EdgeAln> alns;
	for (uint64_t i = in.queryOff[q]; i < in.queryOff[q + 1]; ++i)
	{
		const Rec& r = in.recs[i];
		if (r.extLen < in.P.longEdge || std::min(r.curEnd - r.curBegin, r.extEnd - r.extBegin) > in.P.bigAlignment)
			alns.push_back(EdgeAln{r, in.nodeLeft[r.extId - in.firstExt], in.nodeRight[r.extId - in.firstExt], i});
	}
	if (alns.size() > 16 && hasTie(alns.begin(), alns.end(), [](const EdgeAln& a) { return (int64_t)a.o.curBegin; })) ++cnt.tiedFirst;
	std::sort(alns.begin(), alns.end(), [](const EdgeAln& a, const EdgeAln& b) { return a.o.curBegin < b.o.curBegin; });
	out.chains.clear(); out.scores.clear();
	for (const Chain& ch : chainOneRead(alns, in.P, cnt))
	{
		out.chains.emplace_back();
		for (const EdgeAln* a : ch.aln) out.chains.back().push_back(a->index);
		out.scores.push_back(ch.score);
	}
}

template <class T>
bool readAll(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

} // namespace

int main(int argc, char** argv)
{
	if (argc < 3) { fprintf(stderr, "usage: read_chain_driver IN OUT [threads] [repeats]\n"); return 2; }
	const unsigned threads = argc > 3 ? std::max(1, atoi(argv[3])) : 1;
	const int repeats = argc > 4 ? std::max(1, atoi(argv[4])) : 1;
	Input in;
	FILE* f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	uint32_t head[4];
	bool ok = readAll(f, (int32_t*)&in.P, 6) && readAll(f, head, 4) && readAll(f, &in.nRecs, 1);
	if (ok)
	{
		in.firstExt = head[0]; in.nExt = head[1]; in.nq = head[2];
		in.nodeLeft.resize(in.nExt); in.nodeRight.resize(in.nExt); in.queryOff.resize((size_t)in.nq + 1); in.recs.resize(in.nRecs);
		ok = readAll(f, in.nodeLeft.data(), in.nExt) && readAll(f, in.nodeRight.data(), in.nExt) &&
			 readAll(f, in.queryOff.data(), (size_t)in.nq + 1) && readAll(f, (int32_t*)in.recs.data(), 7 * (size_t)in.nRecs);
	}
	fclose(f);
	if (!ok || in.queryOff[in.nq] != in.nRecs) { fprintf(stderr, "malformed input\n"); return 2; }
	for (const Rec& r : in.recs)
		if (r.extId < in.firstExt || r.extId - in.firstExt >= in.nExt) { fprintf(stderr, "ext id outside the node tables\n"); return 2; }

	std::vector<QueryResult> results(in.nq);
	Counters total;
	double best = 1e30;
	for (int rep = 0; rep < repeats; ++rep)
	{
		std::vector<Counters> cnts(threads);
		const auto t0 = std::chrono::steady_clock::now();
		auto work = [&](unsigned t)
		{
			const uint64_t a = (uint64_t)in.nq * t / threads, b = (uint64_t)in.nq * (t + 1) / threads;
			for (uint64_t q = a; q < b; ++q) runQuery(in, (uint32_t)q, results[q], cnts[t]);
		};
		std::vector<std::thread> pool;
		for (unsigned t = 1; t < threads; ++t) pool.emplace_back(work, t);
		work(0);
		for (auto& th : pool) th.join();
		best = std::min(best, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
		total = Counters();
		for (const Counters& c : cnts)
		{
			total.cleanups += c.cleanups; total.tiedFirst += c.tiedFirst; total.tiedSecond += c.tiedSecond; total.rejected += c.rejected;
		}
	}

	std::vector<uint64_t> chainOff{0}, alnOff{0}, aln;
	std::vector<int32_t> score;
	for (const QueryResult& r : results)
	{
		for (size_t k = 0; k < r.chains.size(); ++k)
		{
			aln.insert(aln.end(), r.chains[k].begin(), r.chains[k].end());
			alnOff.push_back(aln.size());
			score.push_back(r.scores[k]);
		}
		chainOff.push_back(score.size());
	}
	f = fopen(argv[2], "wb");
	if (!f) { perror(argv[2]); return 2; }
	const uint64_t headOut[6] = {score.size(), aln.size(), total.cleanups, total.tiedFirst, total.tiedSecond, total.rejected};
	fwrite(headOut, 8, 6, f);
	fwrite(chainOff.data(), 8, chainOff.size(), f);
	fwrite(alnOff.data(), 8, alnOff.size(), f);
	if (!aln.empty()) fwrite(aln.data(), 8, aln.size(), f);
	if (!score.empty()) fwrite(score.data(), 4, score.size(), f);
	if (fclose(f) != 0) return 2;
	printf("seconds %.6f\n", best);
	return 0;
}
