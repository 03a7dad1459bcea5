// The host part of flye_amd/csrc/fg_stage.h on its own: no HIP, g++ -std=c++17 (tests/test_stage_errors.py builds and
// runs it; exit code 0 and "stage_host_check ok" when every check holds).
#include "../flye_amd/csrc/fg_stage.h"
#include <cstdio>
#include <cstring>
#include <functional>
#include <random>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++failures; printf("line %d: %s\n", __LINE__, #cond); } } while (0)

// f throws FgError{code, text}
static bool throws(const std::function<void()>& f, int code, const std::string& text)
{
	try { f(); }
	catch (const FgError& e)
	{
		if (e.code == code && e.msg == text) return true;
		printf("got %d \"%s\", want %d \"%s\"\n", e.code, e.msg.c_str(), code, text.c_str());
		return false;
	}
	printf("nothing thrown, want %d \"%s\"\n", code, text.c_str());
	return false;
}

static bool quiet(const std::function<void()>& f)
{
	try { f(); return true; }
	catch (const FgError& e) { printf("thrown: %d \"%s\"\n", e.code, e.msg.c_str()); return false; }
}

// the rule of the cut, stated directly: the longest run of whole items from i with a total cost of at most the budget
// and at most maxItems items; at least one item
static uint32_t cutByRule(uint32_t i, uint32_t n, const std::vector<uint64_t>& cost, uint64_t budget, uint64_t maxItems)
{
	uint32_t best = i + 1;
	for (uint32_t end = i + 1; end <= n; ++end)
	{
		uint64_t total = 0;
		for (uint32_t k = i; k < end; ++k) total += cost[k];
		if (total <= budget && (uint64_t)(end - i) <= maxItems) best = end;
		else break;				// costs are not negative: a longer run costs no less
	}
	return best;
}

static void checkCut()
{
	std::mt19937_64 rng(12345);
	int edge[5] = {};
	for (int round = 0; round < 400; ++round)
	{
		const uint32_t n = 1 + rng() % 12;
		std::vector<uint64_t> cost(n);
		const int kind = round % 5;		// 0: budget 0; 1: an item equal to the budget; 2: one above it; 3: zero costs; 4: maxItems 1
		for (auto& c : cost) c = kind == 3 && rng() % 2 ? 0 : rng() % 50;
		uint64_t budget = rng() % 120, maxItems = rng() % 3 ? ~0ULL : 1 + rng() % 4;
		if (kind == 0) budget = 0;
		if (kind == 1) cost[rng() % n] = budget;
		if (kind == 2) cost[rng() % n] = budget + 1;
		if (kind == 4) maxItems = 1;
		++edge[kind];
		uint32_t i = 0, batches = 0;
		while (i < n)
		{
			const uint32_t j = stageCut(i, n, cost, budget, maxItems);
			CHECK(j == cutByRule(i, n, cost, budget, maxItems));
			CHECK(j > i && j <= n);
			if (kind == 4) CHECK(j == i + 1);
			i = j;
			++batches;
		}
		CHECK(batches >= 1 && batches <= n);
	}
	for (int k : edge) CHECK(k == 80);
	// an item above the budget still goes, alone: the refusal in front of the cut is stageFits'
	CHECK(stageCut(0, 3, {5, 9, 1}, 4, ~0ULL) == 1);
	CHECK(stageCut(1, 3, {5, 9, 1}, 9, ~0ULL) == 2);
	CHECK(stageCut(1, 3, {5, 9, 1}, 10, ~0ULL) == 3);
}

static void checkChecks()
{
	const std::string name = "fg_some_call";
	const int32_t contigLen[3] = {6, 0, 4};
	const uint64_t alnOff[4] = {0, 2, 2, 3}, colOff[4] = {0, 5, 8, 12};
	//                          alignment 0     1        2
	const uint8_t trg[] = "AC-GT" "A-C" "GGTA", qry[] = "ACTG-" "AAC" "G-TA";
	CHECK(quiet([&] { stageContigTable(name, 3, contigLen, alnOff); }));
	CHECK(quiet([&] { stageContigTable(name, 0, nullptr, nullptr); }));
	CHECK(quiet([&] { stageColOff(name, colOff, 0, 3, trg, qry); }));
	CHECK(quiet([&] { stageColOff(name, colOff, 0, 0, nullptr, nullptr); }));
	CHECK(quiet([&] { stageOffsets(name, "x_off", "", colOff, 0, 3); }));
	uint64_t ng[3];
	bool present[128] = {};
	CHECK(quiet([&] { for (uint64_t a = 0; a < 3; ++a) ng[a] = stageColumnWalk(name, a, colOff, trg, qry, a == 1 ? present : nullptr); }));
	CHECK(ng[0] == 4 && ng[1] == 2 && ng[2] == 4);
	for (int b = 0; b < 128; ++b) CHECK(present[b] == (b == 'A' || b == 'C'));
	CHECK(quiet([&] { stageStartOnContig(name, 0, 5, 6); stageBasesOnContig(name, 0, 6, 6); }));
	CHECK(quiet([&] { stageFits(name, "contig", 0, 7, 7, "columns", "FG_X"); stageAllFit(name, "job", {1, 2, 3}, 3, "columns", "FG_X"); }));

	CHECK(throws([&] { stageContigTable(name, 3, nullptr, alnOff); }, FG_ERR_ARG, "fg_some_call: null contig_len or contig_aln_off"));
	const int32_t negLen[3] = {6, -1, 4};
	CHECK(throws([&] { stageContigTable(name, 3, negLen, alnOff); }, FG_ERR_ARG, "fg_some_call: contig_len < 0 at contig 1"));
	const uint64_t badAlnOff[4] = {0, 2, 1, 3};
	CHECK(throws([&] { stageContigTable(name, 3, contigLen, badAlnOff); }, FG_ERR_ARG, "fg_some_call: contig_aln_off decreases at contig 1"));
	// the length of a contig stands before its offsets, and an earlier contig before a later one
	CHECK(throws([&] { stageContigTable(name, 3, negLen, badAlnOff); }, FG_ERR_ARG, "fg_some_call: contig_len < 0 at contig 1"));
	CHECK(throws([&] { stageOffsets(name, "job_edge_off", "", badAlnOff, 0, 3); }, FG_ERR_ARG, "fg_some_call: job_edge_off decreases at 1"));
	const uint64_t badColOff[4] = {0, 8, 5, 12}, wide[2] = {3, 3 + (1ULL << 31)};
	CHECK(throws([&] { stageColOff(name, badColOff, 0, 3, trg, qry); }, FG_ERR_ARG, "fg_some_call: col_off decreases at alignment 1"));
	CHECK(throws([&] { stageColOff(name, wide, 0, 1, trg, qry); }, FG_ERR_ARG, "fg_some_call: an alignment of 2^31 columns"));
	CHECK(throws([&] { stageColWidth(name, wide, 0); }, FG_ERR_ARG, "fg_some_call: an alignment of 2^31 columns"));
	CHECK(throws([&] { stageColOff(name, colOff, 0, 3, trg, nullptr); }, FG_ERR_ARG, "fg_some_call: null trg_cols or qry_cols"));
	// what a call adds per alignment comes behind that alignment's own checks and before the next alignment's
	CHECK(throws([&] { stageColOff(name, badColOff, 0, 3, trg, qry, [&](uint64_t a) { if (a == 0) throw FgError{FG_ERR_ARG, "mine"}; }); },
				 FG_ERR_ARG, "mine"));
	uint8_t high[13];
	memcpy(high, qry, 13);
	high[6] = 128;
	CHECK(throws([&] { stageColumnWalk(name, 1, colOff, trg, high); }, FG_ERR_ARG, "fg_some_call: a byte >= 128 in alignment 1"));
	CHECK(throws([&] { stageColumnWalk(name, 1, colOff, high, qry); }, FG_ERR_ARG, "fg_some_call: a byte >= 128 in alignment 1"));
	CHECK(quiet([&] { stageColumnWalk(name, 0, colOff, trg, high); }));
	CHECK(throws([&] { stageStartOnContig(name, 7, -1, 6); }, FG_ERR_ARG, "fg_some_call: trg_start outside the contig at alignment 7"));
	CHECK(throws([&] { stageStartOnContig(name, 7, 6, 6); }, FG_ERR_ARG, "fg_some_call: trg_start outside the contig at alignment 7"));
	CHECK(throws([&] { stageBasesOnContig(name, 2, 7, 6); }, FG_ERR_ARG, "fg_some_call: alignment 2 has more target bases than its contig"));
	CHECK(throws([&] { stageFits(name, "contig", 4, 8, 7, "columns and positions", "FG_X_BATCH_COLS"); }, FG_ERR_NOMEM,
				 "fg_some_call: contig 4 alone has 8 columns and positions, FG_X_BATCH_COLS is 7"));
	CHECK(throws([&] { stageAllFit(name, "job", {1, 9, 12}, 8, "columns and table cells", "FG_Y"); }, FG_ERR_NOMEM,
				 "fg_some_call: job 1 alone has 9 columns and table cells, FG_Y is 8"));
}

static void checkSwitches()
{
	const char* name = "FG_STAGE_HOST_CHECK_SWITCH";
	unsetenv(name);
	CHECK(stageEnvU64(name, 42) == 42 && stageEnvCap(name) == ~0ULL);
	setenv(name, "0", 1);
	CHECK(stageEnvU64(name, 42) == 0 && stageEnvCap(name) == 1);
	setenv(name, "17", 1);
	CHECK(stageEnvU64(name, 42) == 17 && stageEnvCap(name) == 17);
	setenv(name, "many", 1);		// no number: 0, as strtoull gives
	CHECK(stageEnvU64(name, 42) == 0 && stageEnvCap(name) == 1);
	unsetenv(name);
}

static void checkKeep()
{
	std::vector<int32_t> a, b{1, 2};
	std::vector<uint8_t> c;
	const int32_t* was = b.data();
	stageKeep(a, b, c);
	CHECK(a.data() != nullptr && c.data() != nullptr && a.empty() && c.empty() && b.data() == was && b.size() == 2);
}

int main()
{
	checkCut();
	checkChecks();
	checkSwitches();
	checkKeep();
	if (failures) { printf("stage_host_check: %d failures\n", failures); return 1; }
	printf("stage_host_check ok\n");
	return 0;
}
