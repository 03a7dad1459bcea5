// The literal form of the coverage yardstick (tests/coverage_restate.py): ChimeraDetector::getReadCoverage,
// getCachedCoverage and testReadByCoverage (reference src/assemble/chimera.cpp:106-202, :280-343) and the first half of
// MultiplicityInferer::estimateCoverage (src/repeat_graph/multiplicity_inferer.cpp:14-41, :63) restated statement by
// statement on plain integers: std::vector::at, std::sort for the median (src/common/utils.h:31-51), std::ceil on
// float, std::lround.  Shares no code with the library.
//
//   coverage_driver in.bin out.bin [threads [repeats]]
// prints the best wall time of the computation (without reading and writing the files) as its last word.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <thread>
#include <vector>

struct Ovlp { int32_t curId, extId, curBegin, curEnd, curLen, extBegin, extEnd, extLen; };

static int32_t lrOverhang(const Ovlp& o)		// overlap.h:195-199
{
	return std::max(std::min(o.curBegin, o.extBegin), std::min(o.curLen - o.curEnd, o.extLen - o.extEnd));
}

template <typename T>
static T quantile(const std::vector<T>& vec, int percent)	// utils.h:31-45
{
	if (vec.empty()) return 0;
	auto sortedVec = vec;
	std::sort(sortedVec.begin(), sortedVec.end());
	size_t targetId = std::min(vec.size() * (size_t)percent / 100, vec.size() - 1);
	return sortedVec[targetId];
}
template <typename T>
static T median(const std::vector<T>& vec) { return quantile(vec, 50); }

struct ReadParams { int32_t window, maxOverhang, overlapCoverage, uneven; float maxDropRate; };

struct ReadResult {
	std::vector<int32_t> full, junction;
	int64_t sum = 0;
	int32_t max = 0, median = 0, minGood = INT_MAX, threshold = 0;
	uint8_t chimeric = 0, degenerate = 0;
};

static void readCoverage(const ReadParams& P, int32_t seqLen, const Ovlp* ovlps, size_t nOvlps, ReadResult& R)
{
	const int WINDOW = P.window;
	const int MAX_OVERHANG = P.maxOverhang;
	const int FLANK = 1;
	const float MAX_DROP_RATE = P.maxDropRate;

	// chimera.cpp:114-117 / :298-303
	int numWindows = std::ceil((float)seqLen / WINDOW) + 1;
	int vecSize = numWindows - 2 * FLANK;
	std::vector<int32_t> coverage, junctions;
	if (vecSize <= 0)
	{
		R.degenerate = 1;
		coverage = {0};
		junctions = {0};
	}
	else
	{
		coverage.assign(vecSize, 0);
		junctions.assign(vecSize, 0);
		for (size_t k = 0; k < nOvlps; ++k)
		{
			const Ovlp& ovlp = ovlps[k];
			if (ovlp.curId == (ovlp.extId ^ 1) || ovlp.curId == ovlp.extId) continue;
			for (int pos = ovlp.curBegin / WINDOW + FLANK; pos <= ovlp.curEnd / WINDOW - FLANK; ++pos)
			{
				if (lrOverhang(ovlp) > MAX_OVERHANG) ++junctions.at(pos - FLANK);
				else ++coverage.at(pos - FLANK);
			}
		}
	}

	// :145-153
	int32_t maxCov = 0;
	int64_t sumCov = 0;
	for (auto cov : coverage)
	{
		maxCov = std::max(maxCov, cov);
		sumCov += cov;
	}
	int32_t medianCoverage = median(coverage);
	R.sum = sumCov; R.max = maxCov; R.median = medianCoverage;

	// :166-171
	const int MAX_FLANK = (int)MAX_OVERHANG / (float)WINDOW;
	int32_t goodStart = MAX_FLANK;
	int32_t goodEnd = coverage.size() - MAX_FLANK - 1;
	for (int32_t i = goodStart; i <= goodEnd; ++i) R.minGood = std::min(R.minGood, coverage.at(i));

	if (sumCov == 0) R.chimeric = 1;
	else
	{
		// :155-164
		int threshold = 0;
		if (!P.uneven) threshold = std::max(1L, std::lround((float)P.overlapCoverage / MAX_DROP_RATE));
		else threshold = std::max(1L, std::lround(medianCoverage / MAX_DROP_RATE));
		// :173-182
		bool lowCoverage = false;
		if (goodEnd <= goodStart) lowCoverage = true;
		for (int32_t i = goodStart; i <= goodEnd; ++i)
		{
			if (coverage.at(i) < threshold)
			{
				lowCoverage = true;
				break;
			}
		}
		R.threshold = threshold;
		R.chimeric = lowCoverage;
	}
	R.full.swap(coverage);
	R.junction.swap(junctions);
}

template <class T>
static std::vector<T> readVec(FILE* f, size_t n)
{
	std::vector<T> v(n);
	if (n && fread(v.data(), sizeof(T), n, f) != n) throw std::runtime_error("short input");
	return v;
}
template <class T>
static void writeVec(FILE* f, const std::vector<T>& v) { if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f); }

static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static int runReads(FILE* in, FILE* out, int threads, int repeats)
{
	const auto head = readVec<int32_t>(in, 4);
	const auto rate = readVec<float>(in, 1);
	const ReadParams P{head[0], head[1], head[2], head[3], rate[0]};
	const uint32_t nq = readVec<uint32_t>(in, 1)[0];
	const uint64_t nRec = readVec<uint64_t>(in, 1)[0];
	const auto len = readVec<int32_t>(in, nq);
	const auto off = readVec<uint64_t>(in, (size_t)nq + 1);
	const auto tab = readVec<Ovlp>(in, nRec);
	std::vector<ReadResult> res;
	double best = 1e30;
	for (int rep = 0; rep < repeats; ++rep)
	{
		res.assign(nq, ReadResult());
		const double t0 = now();
		std::vector<std::thread> pool;
		for (int t = 0; t < threads; ++t)
			pool.emplace_back([&, t]
			{
				for (uint32_t q = t; q < nq; q += threads) readCoverage(P, len[q], tab.data() + off[q], off[q + 1] - off[q], res[q]);
			});
		for (auto& th : pool) th.join();
		best = std::min(best, now() - t0);
	}
	std::vector<uint64_t> winOff(1, 0);
	std::vector<int32_t> full, junction, mx, med, mn, thr;
	std::vector<int64_t> sum;
	std::vector<uint8_t> chim, deg;
	for (auto& r : res)
	{
		winOff.push_back(winOff.back() + r.full.size());
		full.insert(full.end(), r.full.begin(), r.full.end());
		junction.insert(junction.end(), r.junction.begin(), r.junction.end());
		sum.push_back(r.sum); mx.push_back(r.max); med.push_back(r.median); mn.push_back(r.minGood); thr.push_back(r.threshold);
		chim.push_back(r.chimeric); deg.push_back(r.degenerate);
	}
	writeVec(out, winOff); writeVec(out, full); writeVec(out, junction); writeVec(out, sum); writeVec(out, mx); writeVec(out, med);
	writeVec(out, mn); writeVec(out, thr); writeVec(out, chim); writeVec(out, deg);
	printf("reads %u records %llu seconds %.6f\n", nq, (unsigned long long)nRec, best);
	return 0;
}

struct EdgeAln { int32_t extId, extBegin, extEnd; };

static int runEdges(FILE* in, FILE* out)
{
	const int WINDOW = readVec<int32_t>(in, 1)[0];
	const auto h = readVec<uint32_t>(in, 3);
	const uint32_t nEdges = h[0], nExt = h[1], firstExt = h[2];
	const auto n = readVec<uint64_t>(in, 3);
	const auto edgeLen = readVec<int32_t>(in, nEdges);
	const auto edgeOf = readVec<uint32_t>(in, nExt);
	const auto recs = readVec<EdgeAln>(in, n[0]);
	const auto alnOff = readVec<uint64_t>(in, n[1] + 1);
	const auto aln = readVec<uint64_t>(in, n[2]);
	const double t0 = now();
	// multiplicity_inferer.cpp:19-25
	std::vector<std::vector<int32_t>> wndCoverage(nEdges);
	for (uint32_t e = 0; e < nEdges; ++e)
	{
		size_t numWindows = edgeLen[e] / WINDOW;
		wndCoverage[e].assign(numWindows, 0);
	}
	// :27-41
	for (uint64_t p = 0; p < n[1]; ++p)
	{
		std::vector<EdgeAln> path;
		for (uint64_t i = alnOff[p]; i < alnOff[p + 1]; ++i) path.push_back(recs.at(aln.at(i)));
		for (size_t pathId = 0; pathId < path.size(); ++pathId)
		{
			auto& edgeCov = wndCoverage.at(edgeOf.at(path[pathId].extId - firstExt));
			int covFrom = std::max(0, path[pathId].extBegin / WINDOW + 1);
			int covTo = std::min((int)edgeCov.size(), path[pathId].extEnd / WINDOW);
			if (pathId > 0) covFrom = 0;
			if (pathId < path.size() - 1) covTo = edgeCov.size();
			for (int i = covFrom; i < covTo; ++i) ++edgeCov.at(i);
		}
	}
	std::vector<uint64_t> winOff(1, 0);
	std::vector<int32_t> cov, mx, med;
	std::vector<int64_t> sum;
	for (auto& v : wndCoverage)
	{
		winOff.push_back(winOff.back() + v.size());
		cov.insert(cov.end(), v.begin(), v.end());
		int64_t s = 0;
		int32_t m = 0;
		for (auto c : v) { s += (int64_t)c; m = std::max(m, c); }
		sum.push_back(s); mx.push_back(m); med.push_back(median(v));
	}
	const double dt = now() - t0;
	writeVec(out, winOff); writeVec(out, cov); writeVec(out, sum); writeVec(out, mx); writeVec(out, med);
	printf("edges %u paths %llu seconds %.6f\n", nEdges, (unsigned long long)n[1], dt);
	return 0;
}

int main(int argc, char** argv)
{
	if (argc < 3) { fprintf(stderr, "usage: coverage_driver in.bin out.bin [threads [repeats]]\n"); return 2; }
	const int threads = argc > 3 ? std::max(1, atoi(argv[3])) : 1;
	const int repeats = argc > 4 ? std::max(1, atoi(argv[4])) : 1;
	FILE* in = fopen(argv[1], "rb");
	FILE* out = fopen(argv[2], "wb");
	if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
	int rc = 1;
	try
	{
		const int32_t mode = readVec<int32_t>(in, 1)[0];
		rc = mode == 0 ? runReads(in, out, threads, repeats) : runEdges(in, out);
	}
	catch (const std::exception& e) { fprintf(stderr, "coverage_driver: %s\n", e.what()); }
	fclose(in); fclose(out);
	return rc;
}
