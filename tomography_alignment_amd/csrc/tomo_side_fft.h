// What the side libraries that transform with hipFFT share on the host: FFTCHK, a cache of plans with its planning stopwatch, the maker
// of the common plan (batched in-place 2-D R2C, with its C2R twin if asked for), the stream / work area / execute triple, the rule that
// fits a batch of frames and hipFFT's work area into a scratch budget, and the events that time the passes of a batch.  Internal, as
// tomo_side_host.h is, and with its conventions: included after <hipfft/hipfft.h> and tomo_side_host.h, it names no error code of its
// own (SIDE_ERR_FFT, SIDE_ERR_HIP) and takes the handle as a template parameter where it needs fail().
// libtomo_xcorr.so uses FFTCHK only: its Z2Z plans allocate their own work areas, are bound to the handle's stream when they are made
// and are documented not to count in its device_bytes, so moving them here would change what it holds.
#pragma once

#include <algorithm>
#include <chrono>
#include <map>
#include <tuple>

namespace {
#define FFTCHK(h, call)                                                                                                             \
    do {                                                                                                                            \
        hipfftResult r_ = (call);                                                                                                   \
        if (r_ != HIPFFT_SUCCESS) return fail(h, SIDE_ERR_FFT, std::string(#call) + ": hipfft error " + std::to_string((int)r_));   \
    } while (0)
constexpr int MAX_BATCH = 65535;                   // frames of one batch: the y extent of a grid
constexpr long long MAX_BATCH_FLOATS = 1LL << 31;  // floats of one batch's buffer

struct FftPlan {
    hipfftHandle fwd = 0, inv = 0;   // R2C, and C2R where the library transforms back
    size_t work_bytes = 0;           // the larger of the two
};
inline void release(FftPlan &p) {
    if (p.fwd) hipfftDestroy(p.fwd);
    if (p.inv) hipfftDestroy(p.inv);
}

// The plans of a handle.  Entries stay where they are while others come and go, so a caller may keep the pointers get() gives.
template <class Key>
struct FftPlans {
    std::map<Key, FftPlan> plans;
    std::map<std::tuple<int, int, int>, int> lowered;   // fit_batch's memory, whatever Key is: (rows, cols, first batch) -> lowered batch
    double seconds = 0.0;            // spent making plans
    // The plan of key; a miss calls make(FftPlan &), which returns 0 or what fail() gave it after releasing what it had made.
    template <class Make>
    int get(const Key &key, Make make, FftPlan **out) {
        auto it = plans.find(key);
        if (it == plans.end()) {
            const auto t0 = std::chrono::steady_clock::now();
            FftPlan p;
            CHK(make(p));
            seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            it = plans.emplace(key, p).first;
        }
        *out = &it->second;
        return 0;
    }
    void drop(const Key &key) {
        auto it = plans.find(key);
        if (it != plans.end()) release(it->second), plans.erase(it);
    }
    void destroy_all() {
        for (auto &kv : plans) release(kv.second);
        plans.clear();
    }
};

// A plan without a work area of hipFFT's own: make(plan, &work_bytes) is the hipfftMakePlan* call.  Nothing is left behind on failure.
template <class Make>
hipfftResult new_plan(hipfftHandle *plan, size_t *work_bytes, Make make) {
    hipfftResult r = hipfftCreate(plan);
    if (r == HIPFFT_SUCCESS) r = hipfftSetAutoAllocation(*plan, 0);
    if (r == HIPFFT_SUCCESS) r = make(*plan, work_bytes);
    if (r != HIPFFT_SUCCESS && *plan) hipfftDestroy(*plan), *plan = 0;
    return r;
}

// `batch` in-place 2-D R2C transforms of rows x cols reals, and the C2R back if `inverse`.
template <class H>
int make_r2c_2d(H *h, int rows, int cols, int batch, bool inverse, FftPlan &p) {
    int n[2] = {rows, cols};
    hipfftHandle *hs[2] = {&p.fwd, &p.inv};
    const hipfftType types[2] = {HIPFFT_R2C, HIPFFT_C2R};
    for (int i = 0; i < (inverse ? 2 : 1); ++i) {
        size_t ws = 0;
        const hipfftResult r = new_plan(hs[i], &ws, [&](hipfftHandle f, size_t *w) {
            return hipfftMakePlanMany(f, 2, n, nullptr, 1, 0, nullptr, 1, 0, types[i], batch, w);
        });
        if (r != HIPFFT_SUCCESS) {
            release(p);
            return fail(h, SIDE_ERR_FFT, "hipfft plan (" + std::to_string(rows) + " x " + std::to_string(cols) + ", batch " + std::to_string(batch) +
                                             "): hipfft error " + std::to_string((int)r));
        }
        p.work_bytes = std::max(p.work_bytes, ws);
    }
    return 0;
}

// The R2C, and the C2R, in place in buf on st; work: the area the plan uses if it needs one.
template <class H>
int exec_forward(H *h, const FftPlan &p, hipStream_t st, void *work, void *buf) {
    FFTCHK(h, hipfftSetStream(p.fwd, st));
    if (p.work_bytes) FFTCHK(h, hipfftSetWorkArea(p.fwd, work));
    FFTCHK(h, hipfftExecR2C(p.fwd, (hipfftReal *)buf, (hipfftComplex *)buf));
    return 0;
}
template <class H>
int exec_inverse(H *h, const FftPlan &p, hipStream_t st, void *work, void *buf) {
    FFTCHK(h, hipfftSetStream(p.inv, st));
    if (p.work_bytes) FFTCHK(h, hipfftSetWorkArea(p.inv, work));
    FFTCHK(h, hipfftExecC2R(p.inv, (hipfftComplex *)buf, (hipfftReal *)buf));
    return 0;
}

// The bytes of one frame of an in-place R2C buffer: rows of 2 (cols/2 + 1) floats.
inline size_t frame_bytes(int rows, int cols) { return sizeof(float) * (size_t)rows * (size_t)(2 * (cols / 2 + 1)); }
// The frames of a batch, out of n of fb bytes each, when the work area is work_per_frame bytes a frame; budget 0: no limit.
inline int batch_for(int n, size_t fb, size_t budget, size_t work_per_frame) {
    long long b = n;
    if (budget) b = std::min<long long>(b, (long long)(budget / (fb + work_per_frame)));
    b = std::min<long long>(b, MAX_BATCH);
    b = std::min<long long>(b, MAX_BATCH_FLOATS / (long long)(fb / sizeof(float)));
    return (int)std::max<long long>(b, 1);
}

struct BatchFit {                    // b frames a batch, their plan, and the plan of the last n % b frames if there are any
    int b = 0;
    FftPlan *plan = nullptr, *tail = nullptr;
    size_t max_work() const { return std::max(plan->work_bytes, tail ? tail->work_bytes : (size_t)0); }
};
// The batch for n frames of rows x cols within budget: first with the work area taken to be one spectrum a frame, then, once, with what
// the plan asks for; the large plan is forgotten and the decision remembered in `lowered`, so that the next call does not make it again.
// get(b, FftPlan **) gives the plan of a batch of b (0, or what fail() gave it), forget(b) drops it: neither has to be hipFFT's.  The
// caller grows its work area (to max_work()) and its buffers afterwards.
template <class Get, class Forget>
int fit_batch(std::map<std::tuple<int, int, int>, int> &lowered, int rows, int cols, int n, size_t budget, Get get, Forget forget, BatchFit *out) {
    const size_t fb = frame_bytes(rows, cols);
    int b = batch_for(n, fb, budget, fb);
    const auto first = std::make_tuple(rows, cols, b);
    const auto low = lowered.find(first);
    if (budget && low != lowered.end() && (size_t)low->second * fb < budget) b = low->second;     // decided by an earlier call
    FftPlan *plan = nullptr, *tail = nullptr;
    CHK(get(b, &plan));
    if (budget && b > 1 && (size_t)b * fb + plan->work_bytes > budget) {
        const size_t per = (plan->work_bytes + b - 1) / b;
        const int b2 = std::min(b - 1, batch_for(n, fb, budget, per));
        forget(b);
        lowered[first] = b2;
        b = b2;
        CHK(get(b, &plan));
    }
    if (n % b) CHK(get(n % b, &tail));
    out->b = b, out->plan = plan, out->tail = tail;
    return 0;
}

// fit_batch over the R2C plans of c.
template <class H>
int fit_r2c_2d(H *h, FftPlans<std::tuple<int, int, int>> &c, int rows, int cols, int n, size_t budget, bool inverse, BatchFit *out) {
    const auto get = [&](int b, FftPlan **p) {
        return c.get(std::make_tuple(rows, cols, b), [&](FftPlan &q) { return make_r2c_2d(h, rows, cols, b, inverse, q); }, p);
    };
    return fit_batch(c.lowered, rows, cols, n, budget, get, [&](int b) { c.drop(std::make_tuple(rows, cols, b)); }, out);
}

// Device times of up to N passes: mark i before pass i, mark n after the last, add_elapsed.  A failed create() leaves nothing behind.
template <int N>
struct PassTimer {
    hipEvent_t ev[N + 1] = {};
    bool create() {
        for (hipEvent_t &e : ev)
            if (hipEventCreate(&e) != hipSuccess) {
                destroy();
                return false;
            }
        return true;
    }
    void destroy() {
        for (hipEvent_t &e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    template <class H>
    int mark(H *h, hipStream_t st, int i) {
        HIPCHK(h, hipEventRecord(ev[i], st));
        return 0;
    }
    // Waits for mark n and adds the ms between marks p and p + 1 to ms[p], p < n.
    template <class H>
    int add_elapsed(H *h, float *ms, int n) {
        HIPCHK(h, hipEventSynchronize(ev[n]));
        for (int p = 0; p < n; ++p) {
            float t = 0.f;
            HIPCHK(h, hipEventElapsedTime(&t, ev[p], ev[p + 1]));
            ms[p] += t;
        }
        return 0;
    }
};

}  // namespace
