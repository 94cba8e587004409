// The host-side scaffolding every side library (csrc/<name>/tomo_<name>.hip) shares: the last-error string, fail() and the check macros,
// the common bodies of <prefix>_last_error and of <prefix>_create (its first half, or the whole of a plain one), a device buffer grown
// on demand with the two things done to a handle's list of them, and the alignment test.  Internal: it is not part of the projector's
// sources (KERNEL_SOURCE_FILES), and each library is one translation unit, so everything has internal linkage.
//
// The libraries number their errors differently (include/tomo_*.h), so this header names no code of its own.  Before including it a
// .hip defines, in an anonymous namespace,
//     constexpr int SIDE_ERR_ARG = ..., SIDE_ERR_HIP = ..., SIDE_ERR_NODEV = ...;     and, with hipFFT,  SIDE_ERR_FFT = ...;
// 0 is success in all of them.  The handle struct of a library has the members `std::string err` and `int device` and, if it owns
// device buffers, `bufs()`: pointers to all of them, e.g. `auto bufs() { return std::array{&part, &stats}; }`.  That is the one list of
// them outside the struct: <prefix>_destroy frees it (free_bufs) and <prefix>_device_bytes adds it up (buf_bytes).  After this header
// come, where a library needs them, tomo_side_fft.h (FFTCHK, the plan cache, the batch rule, the pass timer), tomo_side_zgroups.h (a
// volume as groups of four z) and tomo_side_reduce.h (the block sum, the soft mask's edge).
#pragma once

#include <hip/hip_runtime.h>

#include <array>
#include <cstddef>
#include <cstdint>
#include <string>

namespace {

thread_local std::string g_err;      // the last error of the calls of this thread that had no handle to keep it on

// Keep msg on the handle (without one: for the calling thread) and return code.
template <class H>
int fail(H *h, int code, const std::string &msg) {
    if (h) h->err = msg; else g_err = msg;
    return code;
}

inline int fail(std::nullptr_t, int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define HIPCHK(h, call)                                                                                      \
    do {                                                                                                     \
        hipError_t e_ = (call);                                                                              \
        if (e_ != hipSuccess) return fail(h, SIDE_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)
#define CHK(expr)                \
    do {                         \
        int rc_ = (expr);        \
        if (rc_ != 0) return rc_; \
    } while (0)

// The body of <prefix>_last_error.
template <class H>
const char *last_error(const H *h) { return h ? h->err.c_str() : g_err.c_str(); }

// The first half of <prefix>_create: `out` is there and cleared, a device is visible, `device` is one of them.  Whether and when the
// rest of a create makes the device current is the library's own business.
template <class H>
int check_create(int device, H **out) {
    if (!out) return fail(nullptr, SIDE_ERR_ARG, "NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1) return fail(nullptr, SIDE_ERR_NODEV, "no HIP device");
    if (device < 0 || device >= n) return fail(nullptr, SIDE_ERR_ARG, "device out of range");
    return 0;
}

// The whole of a <prefix>_create that makes nothing but the handle; `current`: it makes the device current, as the first call of the
// library that does.  A create that goes on (a timer) undoes *out itself if that fails.
template <class H>
int create_plain(int device, bool current, H **out) {
    CHK(check_create(device, out));
    if (current && hipSetDevice(device) != hipSuccess) return fail(nullptr, SIDE_ERR_HIP, "hipSetDevice failed");
    H *h = new H();
    h->device = device;
    *out = h;
    return 0;
}

inline bool aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }      // a: a power of two

// A device buffer of at least n bytes, grown (never shrunk) on demand.  A grow frees the old block, so the caller makes sure that
// nothing in flight still uses it.
struct Buf {
    void *p = nullptr;
    size_t n = 0;
};

template <class H>
int grow(H *h, Buf &b, size_t bytes) {
    if (b.n >= bytes) return 0;
    if (b.p) {
        HIPCHK(h, hipFree(b.p));
        b.p = nullptr;
        b.n = 0;
    }
    HIPCHK(h, hipMalloc(&b.p, bytes));
    b.n = bytes;
    return 0;
}

// Over h->bufs(): what <prefix>_destroy frees (the device is current) and what <prefix>_device_bytes reports.
template <class List>
void free_bufs(const List &bufs) {
    for (Buf *b : bufs)
        if (b->p) (void)hipFree(b->p);
}

template <class List>
size_t buf_bytes(const List &bufs) {
    size_t t = 0;
    for (const Buf *b : bufs) t += b->n;
    return t;
}

}  // namespace
