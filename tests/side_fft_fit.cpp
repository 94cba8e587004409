// Drives fit_batch and the plan cache of csrc/tomo_side_fft.h on the host with a fake plan source: no device, no hipFFT call.  Built and
// run by tests/test_side_fft_fit.py; exits 0 if every check holds, else prints the ones that do not and exits 1.  The program is not
// linked against hipFFT or the HIP runtime, so it may use nothing of the header that calls them: its forget action erases the entry
// itself where the libraries call FftPlans::drop, and drop, destroy_all, release and the makers are run by the GPU tests only.
#include <hip/hip_runtime.h>
#include <hipfft/hipfft.h>

#include <cstdio>
#include <functional>

namespace {
constexpr int SIDE_ERR_ARG = 1, SIDE_ERR_HIP = 2, SIDE_ERR_NODEV = 3, SIDE_ERR_FFT = 4;
}
#include "../tomography_alignment_amd/csrc/tomo_side_host.h"
#include "../tomography_alignment_amd/csrc/tomo_side_fft.h"

namespace {

int failures = 0;

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond); \
            ++failures;                                                 \
        }                                                               \
    } while (0)

// Plans that are nothing but a work size, work(b), in a real FftPlans; makes and drops are counted per batch size.
struct Fake {
    int rows, cols;
    std::function<size_t(int)> work;
    FftPlans<std::tuple<int, int, int>> cache;
    std::map<int, int> made, dropped;

    int total(const std::map<int, int> &m) const {
        int t = 0;
        for (auto &kv : m) t += kv.second;
        return t;
    }

    int fit(int n, size_t budget, BatchFit *out) {
        return fit_batch(
            cache.lowered, rows, cols, n, budget,
            [&](int b, FftPlan **p) {
                return cache.get(std::make_tuple(rows, cols, b), [&](FftPlan &q) {
                    const auto t0 = std::chrono::steady_clock::now();
                    while (std::chrono::steady_clock::now() == t0) {}      // a make takes time the stopwatch can see
                    q.work_bytes = work(b);
                    ++made[b];
                    return 0;
                }, p);
            },
            [&](int b) {
                ++dropped[b];
                cache.plans.erase(std::make_tuple(rows, cols, b));
            },
            out);
    }
};

void check_tail(const Fake &f, const BatchFit &fit, int n) {
    const int rest = n % fit.b;
    CHECK((fit.tail != nullptr) == (rest != 0));
    CHECK(fit.plan != nullptr && fit.plan == &f.cache.plans.at(std::make_tuple(f.rows, f.cols, fit.b)));
    if (rest && fit.tail) CHECK(fit.tail == &f.cache.plans.at(std::make_tuple(f.rows, f.cols, rest)));
}

void run(int rows, int cols, int n) {
    const size_t fb = frame_bytes(rows, cols);
    CHECK(fb == (size_t)4 * rows * 2 * (cols / 2 + 1));
    const long long cap = std::min<long long>(std::min<long long>(n, 65535), (1LL << 31) / (long long)(fb / 4));
    BatchFit fit;

    {   // no budget
        Fake f{rows, cols, [&](int b) { return 3 * (size_t)b * fb; }};
        CHECK(f.fit(n, 0, &fit) == 0);
        CHECK(fit.b == cap);
        CHECK(f.total(f.dropped) == 0 && f.cache.lowered.empty());
        check_tail(f, fit, n);
    }
    {   // the work area is what the first batch assumes: one spectrum a frame
        Fake f{rows, cols, [&](int b) { return (size_t)b * fb; }};
        const size_t budgets[5] = {1, 2 * fb, 4 * fb, 6 * fb + 5, 8 * fb};
        const int want[5] = {1, 1, 2, 3, 4};
        for (int i = 0; i < 5; ++i) {
            CHECK(f.fit(n, budgets[i], &fit) == 0);
            CHECK(fit.b == std::min(n, want[i]));
            CHECK(fit.b == batch_for(n, fb, budgets[i], fb));
            check_tail(f, fit, n);
        }
        CHECK(f.total(f.dropped) == 0 && f.cache.lowered.empty());
    }
    {   // three times that, eight frames of budget: 4 is lowered to min(3, 8 fb / (fb + 3 fb)) = 2
        Fake f{rows, cols, [&](int b) { return 3 * (size_t)b * fb; }};
        const size_t budget = 8 * fb;
        CHECK(batch_for(n, fb, budget, fb) == 4);
        CHECK(f.fit(n, budget, &fit) == 0);
        CHECK(fit.b == 2);
        CHECK(f.made[4] == 1 && f.dropped[4] == 1 && f.total(f.dropped) == 1);
        CHECK(f.cache.plans.count(std::make_tuple(rows, cols, 4)) == 0);
        CHECK((size_t)fit.b * fb + fit.plan->work_bytes <= budget);
        check_tail(f, fit, n);
        CHECK(fit.max_work() == 3 * (size_t)fit.b * fb);
        const int makes = f.total(f.made);
        CHECK(makes == (n % 2 ? 3 : 2));
        const double seconds = f.cache.seconds;
        CHECK(seconds > 0.0);                        // the stopwatch ran on the misses
        BatchFit again;
        CHECK(f.fit(n, budget, &again) == 0);        // the remembered batch, and every plan from the cache
        CHECK(again.b == 2 && again.plan == fit.plan && again.tail == fit.tail);
        CHECK(f.total(f.made) == makes && f.total(f.dropped) == 1);
        CHECK(f.cache.seconds == seconds);           // and stood still on the hits
    }
    {   // the same work and one byte: a batch is never fewer than one frame, and one frame is not lowered
        Fake f{rows, cols, [&](int b) { return 3 * (size_t)b * fb; }};
        CHECK(f.fit(n, 1, &fit) == 0);
        CHECK(fit.b == 1 && fit.tail == nullptr);
        CHECK(f.total(f.dropped) == 0 && f.cache.lowered.empty() && f.total(f.made) == 1);
    }
    {   // a miss that fails is handed on, is not cached and costs the stopwatch nothing
        FftPlans<std::tuple<int, int, int>> cache;
        FftPlan *p = nullptr;
        CHECK(cache.get(std::make_tuple(rows, cols, 1), [](FftPlan &) { return SIDE_ERR_FFT; }, &p) == SIDE_ERR_FFT);
        CHECK(p == nullptr && cache.plans.empty() && cache.seconds == 0.0);
    }
}

}  // namespace

int main() {
    run(64, 50, 5);
    run(2, 2, 70000);                                // MAX_BATCH binds
    CHECK(batch_for(70000, frame_bytes(2, 2), 0, frame_bytes(2, 2)) == 65535);
    CHECK(batch_for(5, frame_bytes(8192, 8192), 0, 0) == 5 && batch_for(64, frame_bytes(8192, 8192), 0, 0) == 31);   // MAX_BATCH_FLOATS binds
    if (failures) std::printf("%d checks failed\n", failures);
    return failures ? 1 : 0;
}
