// Driver of tests/test_task_chain.py: the ordered task pass of fg_taskchain.h under several threads (built with
// -fsanitize=thread where the toolchain has it).  Prints "ok" and returns 0 when every check holds.
#include "fg_taskchain.h"

#include <cstdio>
#include <stdexcept>
#include <thread>
#include <vector>

static int failures = 0;
#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); ++failures; } } while (0)

static uint64_t cntA(uint32_t t) { return (t * 2654435761u >> 7) % 9; }		// some tasks count nothing
static uint64_t cntB(uint32_t t) { return t % 3; }

template <class Body>
static void runThreads(unsigned n, Body body)
{
	std::vector<std::thread> th;
	for (unsigned i = 1; i < n; ++i) th.emplace_back(body);
	body();
	for (auto& t : th) t.join();
}

// every task gets the sums of the tasks before it and writes its own stretch: the output is gap-free and in task order
static void ordered(uint32_t nTasks, unsigned nThreads)
{
	std::vector<uint64_t> wantA(nTasks + 1, 0), wantB(nTasks + 1, 0);
	for (uint32_t t = 0; t < nTasks; ++t) { wantA[t + 1] = wantA[t] + cntA(t); wantB[t + 1] = wantB[t] + cntB(t); }
	std::vector<uint32_t> outA(wantA[nTasks], 0xFFFFFFFFu), outB(wantB[nTasks], 0xFFFFFFFFu);
	std::vector<uint8_t> counted(nTasks, 0), written(nTasks, 0);
	FgTaskChain<2> chain(nTasks);
	runThreads(nThreads, [&]
	{
		chain.work(
			[&](uint32_t t, uint64_t* mine) { mine[0] = cntA(t); mine[1] = cntB(t); counted[t] = 1; },
			[&](uint32_t t, const uint64_t* base)
			{
				if (base[0] != wantA[t] || base[1] != wantB[t]) throw std::runtime_error("wrong base");
				for (uint64_t i = 0; i < cntA(t); ++i) outA[base[0] + i] = t;
				for (uint64_t i = 0; i < cntB(t); ++i) outB[base[1] + i] = t;
				written[t] = counted[t];		// count and write of a task run on one thread
			});
	});
	chain.rethrow();
	CHECK(chain.total(0) == wantA[nTasks] && chain.total(1) == wantB[nTasks]);
	for (uint32_t t = 0; t < nTasks; ++t)
	{
		CHECK(written[t] == 1);
		for (uint64_t i = wantA[t]; i < wantA[t + 1]; ++i) CHECK(outA[i] == t);
		for (uint64_t i = wantB[t]; i < wantB[t + 1]; ++i) CHECK(outB[i] == t);
	}
}

// a task that throws -- in its count or in its write -- ends the pass with that exception on the caller, not with a hang
static void failing(bool inCount, unsigned nThreads)
{
	const uint32_t nTasks = 4000, bad = 1777;
	std::vector<uint8_t> wrote(nTasks, 0);
	FgTaskChain<1> chain(nTasks);
	runThreads(nThreads, [&]
	{
		chain.work(
			[&](uint32_t t, uint64_t* mine) { if (inCount && t == bad) throw std::runtime_error("count failed"); mine[0] = 1; },
			[&](uint32_t t, const uint64_t*) { if (!inCount && t == bad) throw std::runtime_error("write failed"); wrote[t] = 1; });
	});
	bool thrown = false;
	try { chain.rethrow(); }
	catch (const std::runtime_error& e) { thrown = std::string(e.what()) == (inCount ? "count failed" : "write failed"); }
	CHECK(thrown);
	CHECK(wrote[bad] == 0);
	CHECK(chain.next.load() >= nTasks);		// every task was claimed and published: nobody is left waiting
}

int main()
{
	FgTaskChain<3> none(0);
	none.work([](uint32_t, uint64_t*) {}, [](uint32_t, const uint64_t*) {});
	none.rethrow();
	CHECK(none.total(0) == 0);
	ordered(1, 1);
	ordered(1, 4);
	ordered(3000, 1);
	for (unsigned n : {2u, 5u, 16u}) ordered(20000, n);
	for (unsigned n : {1u, 8u}) { failing(true, n); failing(false, n); }
	if (failures) return 1;
	puts("ok");
	return 0;
}
