// worker_pool_throw.cpp -- TEST: an exception thrown by fn(0) on the calling thread (an SDF's sample() is the caller's code)
// must leave WorkerPool::run (sdf-viewer_amd/host/worker_pool.hpp) only after every background worker of that run is done: the
// workers run *fn over the caller's stack frame.  Afterwards the same pool keeps serving sessions and runs, and shuts down.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <stdexcept>
#include <thread>
#include <vector>

#include "worker_pool.hpp"

static int check_runs(sdfviewer::WorkerPool& pool, unsigned max_workers) {
    std::vector<std::atomic<unsigned>> hits(max_workers);
    for (int session = 0; session < 20; ++session) {
        const unsigned n = 1 + (unsigned)session % max_workers;
        pool.begin(n);
        for (int r = 0; r < 25; ++r) {
            const unsigned m = 1 + (unsigned)(r * 7 + session) % n;
            for (auto& h : hits) h.store(0);
            std::function<void(unsigned)> fn = [&](unsigned t) { hits[t].fetch_add(1); };
            pool.run(m, fn);
            for (unsigned t = 0; t < max_workers; ++t)
                if (hits[t].load() != (t < m ? 1u : 0u)) {
                    fprintf(stderr, "after the throw: session %d run %d: worker %u ran %u times (m = %u)\n", session, r, t,
                            hits[t].load(), m);
                    return 1;
                }
        }
        pool.end();
    }
    return 0;
}

int main() {
    for (unsigned n : {2u, 5u}) {
        sdfviewer::WorkerPool pool;
        std::atomic<unsigned> finished{0};
        pool.begin(n);
        bool caught = false;
        try {
            std::function<void(unsigned)> fn = [&](unsigned t) {
                if (t == 0) throw std::runtime_error("sample() failed");
                std::this_thread::sleep_for(std::chrono::milliseconds(20));
                finished.fetch_add(1);
            };
            pool.run(n, fn);
        } catch (const std::runtime_error&) {
            caught = true;
            const unsigned seen = finished.load();
            if (seen != n - 1) {
                fprintf(stderr, "n = %u: run() unwound with %u of %u workers finished\n", n, seen, n - 1);
                return 1;
            }
        }
        pool.end();
        if (!caught) {
            fprintf(stderr, "n = %u: the exception did not reach the caller\n", n);
            return 1;
        }
        if (check_runs(pool, 6) != 0) return 1;
    }  // (the pool's destructor joins its threads: a clean shutdown)
    printf("ok\n");
    return 0;
}
