// The speculative batch loop of the iterative solves (A2 value iteration, A4/A5 EGM, the A10
// histogram fixed point): steps are enqueued a batch at a time between two reads of the stopping
// distance, two batches in flight, so the device never waits for a read.  Host code only, no HIP:
// the caller's callables make the launches, copies and waits.  Steps are deterministic and each
// depends only on its predecessor, so the steps up to the stopping one are exactly those of a
// read-per-step loop; the speculative ones past it are discarded by the caller.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace aiy {

struct SpecResult {
    int64_t g = 0;     // the final step: the first that met the predicate, else the last enqueued
    int64_t stop = 0;  // the first step that met the predicate, 0 = none did
    int64_t enq = 0;   // steps enqueued
    bool any = false;  // a distance was read
    double d = NAN;    // the last distance read
};

// Runs steps 1, 2, ... (at most max_iter) in batches of at most M until a step's distance meets
// `stops`.  A batch is sized by the geometric decay of the last two distances read: the steps
// still needed to reach tol, less those already in flight, where that is fewer than M.
//   int step(int64_t g)                   enqueue step g
//   int flush(int hb)                     end of a batch: copy its distances to host half hb, record
//   int wait(int hb)                      until half hb's copy has landed
//   int read(int64_t g, int hb, double*)  step g's distance from half hb (may fail)
//   bool stops(double d)                  the solver's stopping test
// A non-zero return of a callable ends the loop with that code (*R then holds the counts so far).
template <class Step, class Flush, class Wait, class Read, class Stops>
int spec_loop(int64_t M, int64_t max_iter, double tol, SpecResult* R, Step&& step, Flush&& flush,
              Wait&& wait, Read&& read, Stops&& stops) {
    struct Batch {
        int64_t s0, m;  // steps s0 + 1 .. s0 + m
        int hb;         // host half holding its distances
    };
    Batch q[2];
    int nq = 0, hb_next = 0;
    double d_prev = NAN, d_last = NAN;
    *R = SpecResult{};
    int64_t& enq = R->enq;
    auto enqueue = [&]() -> int {
        int64_t m = M;
        if (d_last == d_last && d_prev == d_prev && d_last < d_prev && d_last > 0) {
            // steps the observed decay still needs, counted from the last read (tol <= 0 or NaN:
            // +inf or NaN, neither shortens the batch)
            const double need = std::ceil(std::log(tol / d_last) / std::log(d_last / d_prev));
            int64_t ahead = 0;  // steps in flight, not yet read
            for (int b = 0; b < nq; ++b) ahead += q[b].m;
            if (need >= 1 && need - (double)ahead < (double)m)
                m = (int64_t)std::max(1.0, need - (double)ahead);
        }
        m = std::min<int64_t>(std::max<int64_t>(m, 1), max_iter - enq);
        for (int64_t g = enq + 1; g <= enq + m; ++g)
            if (const int rc = step(g)) return rc;
        if (const int rc = flush(hb_next)) return rc;
        q[nq++] = Batch{enq, m, hb_next};
        hb_next ^= 1;
        enq += m;
        return 0;
    };
    int rc = max_iter > 0 ? enqueue() : 0;
    while (rc == 0 && nq > 0) {
        if (nq < 2 && enq < max_iter && (rc = enqueue())) break;  // the device runs while we read
        const Batch b = q[0];
        if ((rc = wait(b.hb))) break;
        for (int64_t g = b.s0 + 1; g <= b.s0 + b.m; ++g) {
            double d = NAN;
            if ((rc = read(g, b.hb, &d))) break;
            d_prev = d_last;
            d_last = d;
            R->any = true;
            R->d = d;
            if (stops(d)) {
                R->stop = g;
                break;
            }
        }
        q[0] = q[1];
        --nq;
        if (rc || R->stop) break;
    }
    R->g = R->stop ? R->stop : enq;
    return rc;
}

}  // namespace aiy
