// Ordered tasks with a chained prefix (host only, no HIP): the record pass of fg_overlaps.
//
// Tasks 0 .. nTasks-1 are claimed in order by any number of worker threads.  A task first COUNTS what it will
// write (N running sums: records, statistics, match pairs), then takes its output bases from the sums its
// predecessor published, publishes its own (predecessor + mine) and only then WRITES -- so task t + 1 never waits
// for task t's writing, only for its counting.  There is no pass over all tasks and no join between counting and
// writing.
//
// Every wait ends: tasks are claimed in ascending order from one counter, so the predecessor of a claimed task
// has been claimed before it by a thread that is running (or done), and a task publishes whatever happens in it --
// a failed count publishes its predecessor's sums unchanged.  The first exception of any task is kept and
// rethrown by rethrow() on the calling thread; once one task has failed the others skip their work.
#pragma once
#include <atomic>
#include <cstdint>
#include <exception>
#include <memory>
#include <mutex>
#include <thread>

template <int N>
struct FgTaskChain {
	struct alignas(64) Slot {
		std::atomic<uint32_t> ready{0};
		uint64_t sum[N];		// running sums up to and including this task
	};
	std::unique_ptr<Slot[]> slots;
	uint32_t nTasks = 0;
	std::atomic<uint32_t> next{0};
	std::atomic<bool> failed{false};
	std::mutex errMu;
	std::exception_ptr err;

	explicit FgTaskChain(uint32_t n) : slots(n ? new Slot[n] : nullptr), nTasks(n) {}

	void fail(std::exception_ptr e)
	{
		std::lock_guard<std::mutex> g(errMu);
		if (!err) err = e;
		failed.store(true, std::memory_order_release);
	}

	// One worker; call it from as many threads as wanted.  count(task, mine[N]) fills the task's own counts,
	// write(task, base[N]) gets the sums of all tasks before it.  Both run on the same thread, count first.
	template <class Count, class Write>
	void work(Count&& count, Write&& write)
	{
		while (true)
		{
			const uint32_t t = next.fetch_add(1, std::memory_order_relaxed);
			if (t >= nTasks) return;
			uint64_t mine[N] = {}, base[N] = {};
			bool counted = false;
			if (!failed.load(std::memory_order_acquire))
			{
				try { count(t, mine); counted = true; }
				catch (...) { for (int i = 0; i < N; ++i) mine[i] = 0; fail(std::current_exception()); }
			}
			if (t)
			{
				const Slot& prev = slots[t - 1];
				for (unsigned spins = 0; !prev.ready.load(std::memory_order_acquire); ++spins)
				{
					if (spins < 64) __builtin_ia32_pause();
					else std::this_thread::yield();
				}
				for (int i = 0; i < N; ++i) base[i] = prev.sum[i];
			}
			Slot& me = slots[t];
			for (int i = 0; i < N; ++i) me.sum[i] = base[i] + mine[i];
			me.ready.store(1, std::memory_order_release);
			if (counted && !failed.load(std::memory_order_acquire))
			{
				try { write(t, base); }
				catch (...) { fail(std::current_exception()); }
			}
		}
	}

	// after all workers have returned
	uint64_t total(int i) const { return nTasks ? slots[nTasks - 1].sum[i] : 0; }
	void rethrow() { if (err) std::rethrow_exception(err); }
};
