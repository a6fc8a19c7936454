// Stand-alone host program around csrc/spec_loop.hpp (tests/test_host_layer_cpu.py builds it with
// -fsanitize=address,undefined).  stdin: the number of cases, then per case
//   M max_iter tol pred step_err read_err nd   followed by nd distances (step g's is the g-th)
// pred 0: stop on d < tol, 1: on !(d > tol); step_err / read_err: the step at which the fake
// step / read fails (0: never; codes 7 / 9).  stdout per case: the calls in order — S<g> step,
// F<hb> flush, W<hb> wait, R<g> read — then `= rc g stop enq any d`.  The fakes keep the two host
// halves as a real caller's would be: a flush into a half not yet read, a wait on a half not
// flushed (or waited for before) and a read of a step its half does not hold end the program
// with FAILED.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "spec_loop.hpp"

struct Half {
    bool full = false, waited = false;  // holds a batch; the loop has waited for it
    long long first = 0, last = 0;      // the steps whose distances it holds
};

static void failed(const char* what) {
    printf("\nFAILED %s\n", what);
    exit(3);
}

int main() {
    int ncase = 0;
    if (scanf("%d", &ncase) != 1) return 2;
    for (int c = 0; c < ncase; ++c) {
        long long M, max_iter, step_err, read_err;
        int pred, nd;
        double tol;
        if (scanf("%lld %lld %lf %d %lld %lld %d", &M, &max_iter, &tol, &pred, &step_err, &read_err,
                  &nd) != 7)
            return 2;
        std::vector<double> ds((size_t)nd);
        for (double& v : ds)
            if (scanf("%lf", &v) != 1) return 2;
        Half half[2];
        long long issued = 0, flushed = 0;
        int waited = -1;
        auto step = [&](int64_t g) -> int {
            if (g != issued + 1) failed("steps out of order");
            if (g > max_iter) failed("a step beyond max_iter");
            if ((size_t)g > ds.size()) failed("no distance for the step");
            issued = g;
            printf("S%lld ", (long long)g);
            return g == step_err ? 7 : 0;
        };
        auto flush = [&](int hb) -> int {
            if (hb < 0 || hb > 1 || (half[hb].full && !half[hb].waited))
                failed("flush into a half still unread");
            if (issued == flushed) failed("flush of an empty batch");
            half[hb] = Half{true, false, flushed + 1, issued};
            flushed = issued;
            printf("F%d ", hb);
            return 0;
        };
        auto wait = [&](int hb) -> int {
            if (hb < 0 || hb > 1 || !half[hb].full || half[hb].waited)
                failed("wait on a half not flushed");
            half[hb].waited = true;
            waited = hb;
            printf("W%d ", hb);
            return 0;
        };
        auto read = [&](int64_t g, int hb, double* d) -> int {
            if (hb != waited || g < half[hb].first || g > half[hb].last)
                failed("read of a step its half does not hold");
            printf("R%lld ", (long long)g);
            if (g == read_err) return 9;
            *d = ds[(size_t)g - 1];
            return 0;
        };
        aiy::SpecResult R;
        const int rc = pred ? aiy::spec_loop(M, max_iter, tol, &R, step, flush, wait, read,
                                             [tol](double d) { return !(d > tol); })
                            : aiy::spec_loop(M, max_iter, tol, &R, step, flush, wait, read,
                                             [tol](double d) { return d < tol; });
        printf("= %d %lld %lld %lld %d %.17g\n", rc, (long long)R.g, (long long)R.stop,
               (long long)R.enq, (int)R.any, R.d);
    }
    return 0;
}
