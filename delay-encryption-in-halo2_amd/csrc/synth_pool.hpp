// synth_pool.hpp -- the host threads that write a proving call's independent regions (synth_chips.hpp BigIntChip::pow_mod): how many, and the pool that
// keeps them between calls.  Host only, no HIP include.
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <functional>
#include <mutex>
#include <pthread.h>
#include <thread>

namespace synth { namespace {

inline unsigned synth_threads() {
    static const unsigned n = [] {
        const char* e = getenv("DEHALO_SYNTH_THREADS");
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        return e ? (unsigned)std::max(1, atoi(e)) : std::min(8u, hw);
    }();
    return n;
}

// Worker threads kept for the life of the process (starting seven threads costs more than the regions they would write: 25 us each against 34 us per
// region): they sleep on a condition variable between calls.  One job at a time -- a second caller that finds the pool busy writes its regions itself.
struct SynthPool {
    std::mutex job_mu, mu;
    std::condition_variable cv, done_cv;
    const std::function<void()>* fn = nullptr;
    uint64_t gen = 0;
    unsigned pending = 0, workers = 0;
    explicit SynthPool(unsigned n) : workers(n) {
        for (unsigned i = 0; i < n; i++)
            std::thread([this] {
                uint64_t seen = 0;
                for (;;) {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return gen != seen; });
                    seen = gen;
                    const std::function<void()>* f = fn;
                    lk.unlock();
                    (*f)();
                    lk.lock();
                    if (--pending == 0) done_cv.notify_one();
                }
            }).detach();
    }
    void run(const std::function<void()>& f) {      // f on every worker and on the caller; returns when all are back
        { std::lock_guard<std::mutex> lk(mu); fn = &f; pending = workers; gen++; }
        cv.notify_all();
        f();
        std::unique_lock<std::mutex> lk(mu);
        done_cv.wait(lk, [&] { return pending == 0; });
    }
    void run_or_alone(const std::function<void()>& f) {      // (a second caller that finds the pool busy runs f itself)
        if (job_mu.try_lock()) {
            run(f);
            job_mu.unlock();
        } else f();
    }
};
// (never destroyed: its threads sleep until the process ends.  A forked child has none of them: it starts with no pool and makes its own.)
inline std::atomic<SynthPool*> g_synth_pool{nullptr};
inline SynthPool* synth_pool() {
    static const int registered = pthread_atfork(nullptr, nullptr, [] { g_synth_pool.store(nullptr); });
    (void)registered;
    SynthPool* p = g_synth_pool.load();
    if (!p) {
        SynthPool* fresh = new SynthPool(synth_threads() - 1);
        if (g_synth_pool.compare_exchange_strong(p, fresh)) p = fresh;      // (lost the race: `fresh` stays behind, asleep)
    }
    return p;
}

} }   // namespace synth
