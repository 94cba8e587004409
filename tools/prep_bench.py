#!/usr/bin/env python3
"""Development tool (not the benchmark contract; bench.py is): times preprocess.py on the GPU -- the fused normalisation of uint16 frames
the three passes of the stripe removal, and the zinger removal -- with device events on a warmed handle.

    python tools/prep_bench.py                          # 1024 x 1024^2 and 1800 x 2048^2 (n_proj x rows x cols)
    python tools/prep_bench.py --cases 256x512x512 --reps 3

One JSON line per case on stdout.  Normalisation: the minimal traffic is 2 B read + 4 B written per pixel (uint16 in, float32 out; the
flat and dark tiles are read once per 16 frames); the rate is also given as a fraction of a device-to-device copy of the output's bytes
timed in the same process (a copy moves 2 x its bytes).  Stripe removal (size 21): per sinogram value the sort pass reads 4 B and writes
6 B (value + uint16 rank), the median pass reads 4 B (plus the halo) and writes 4 B, the scatter pass reads 6 B and writes 4 B; the sort
does Np log2(Np) (log2(Np) + 1) / 4 compare-exchanges per column (Np: n_proj rounded up to a power of two), each two 8-byte LDS reads and
up to two 8-byte LDS writes.  The large-, dead- and all-stripe passes (cases `large`, `dead`, `all`; snr 3, windows 51, 51 and 61 / --size)
are timed whole, in place, on the same sinogram: each adds its statistics, the detector and a correction to the sort and median passes
above (dead with norm and all run the large pass too).

The outlier leg (--legs outlier; one more JSON line per case) times preprocess.remove_outlier (one-sided, dif 3000) on n x rows x cols
frames of noisy counts, uint16 and float32, windows 3, 5 and 7, out of place and in place (default scratch budget): milliseconds, the
GB/s of the minimal traffic (each pixel read once and written once) and that rate as a fraction of a device-to-device copy of the same
buffer timed in the same process -- the yardstick of normalize_vs_copy."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def _emit(**kw):
    print(json.dumps(kw), flush=True)


def case(n, rows, cols, reps, size, passes_wanted=("large", "dead", "all")):
    from tomography_alignment_amd import _lib, preprocess

    ctx = _lib.Context()
    pre = preprocess.Preprocessor(ctx)
    d_raw = ctx.zeros((n, rows, cols), np.uint16)               # the kernels' work does not depend on the values
    flats = np.full((1, rows, cols), 1000, np.uint16)
    darks = np.full((1, rows, cols), 100, np.uint16)
    d_flats, d_darks = ctx.to_device(flats, np.uint16), ctx.to_device(darks, np.uint16)
    sino = ctx.empty((n, cols, rows), np.float32)
    la = cols if cols % 2 else cols - 1                            # the widest odd window the detector allows
    copy_dst = ctx.empty((n, cols, rows), np.float32)

    def timed(fn):
        fn()                                                     # warm-up
        ctx.sync()
        out = []
        for _ in range(reps):
            ctx.timer_start()
            fn()
            out.append(ctx.timer_stop())
        return float(np.median(out)), float(np.min(out))

    npix = n * rows * cols
    norm_ms, norm_min = timed(lambda: pre.normalize(d_raw, d_flats, d_darks, out=sino))
    copy_ms, _ = timed(lambda: copy_dst.copy_from(sino))
    norm_gbs = 6.0 * npix / (norm_ms * 1e-3) / 1e9
    copy_gbs = 2.0 * sino.nbytes / (copy_ms * 1e-3) / 1e9
    copy_dst.free()

    pre.remove_stripe_sorting(sino, size=size, out=sino)         # warm-up (scratch allocation, LDS attributes)
    ctx.sync()
    passes = []
    for _ in range(reps):
        _, ms = pre.remove_stripe_sorting(sino, size=size, out=sino, timed=True)
        passes.append(ms)
    passes = np.median(np.asarray(passes), axis=0)
    whole_ms, _ = timed(lambda: pre.remove_stripe_sorting(sino, size=size, out=sino))
    extra = {}
    runs = {"large": lambda: pre.remove_large_stripe(sino, size=min(51, la), out=sino),
            "dead": lambda: pre.remove_dead_stripe(sino, size=min(51, la), out=sino),
            "all": lambda: pre.remove_all_stripe(sino, la_size=min(61, la), sm_size=size, out=sino)}
    for name in passes_wanted:
        ms, ms_min = timed(runs[name])
        extra[name + "_ms"] = round(ms, 2)
        extra[name + "_min_ms"] = round(ms_min, 2)
    if passes_wanted:
        extra["stripe_all_chunk_z"] = preprocess._prep_lib.stripe_all_chunk(n, cols, rows, preprocess.DEFAULT_SCRATCH_BYTES)
    np2 = 1 << max(0, math.ceil(math.log2(n)))
    lg = int(math.log2(np2))
    cols_z = cols * rows                                         # sinogram columns (x, z)
    cex = cols_z * np2 * lg * (lg + 1) // 4
    moved = {"sort": 10.0 * npix, "median": 8.0 * npix, "scatter": 10.0 * npix}
    _emit(case="%dx%dx%d" % (n, rows, cols), reps=reps, device=ctx.device_name(),
          normalize_ms=round(norm_ms, 3), normalize_min_ms=round(norm_min, 3), normalize_GBps=round(norm_gbs, 1),
          d2d_copy_GBps=round(copy_gbs, 1), normalize_vs_copy=round(norm_gbs / copy_gbs, 3),
          stripe_size=size, stripe_chunk_z=preprocess._prep_lib.stripe_chunk(n, cols, rows, preprocess.DEFAULT_SCRATCH_BYTES),
          stripe_ms=round(whole_ms, 2),
          sort_ms=round(float(passes[0]), 2), sort_GBps=round(moved["sort"] / (passes[0] * 1e-3) / 1e9, 1),
          sort_compare_exchanges=cex, sort_lds_GBps=round(32.0 * cex / (passes[0] * 1e-3) / 1e9, 1),
          median_ms=round(float(passes[1]), 2), median_GBps=round(moved["median"] / (passes[1] * 1e-3) / 1e9, 1),
          scatter_ms=round(float(passes[2]), 2), scatter_GBps=round(moved["scatter"] / (passes[2] * 1e-3) / 1e9, 1), **extra)
    pre.close()
    ctx.close()


def outlier_case(n, rows, cols, reps):
    from tomography_alignment_amd import _lib, preprocess

    ctx = _lib.Context()
    pre = preprocess.Preprocessor(ctx)
    rng = np.random.default_rng(0)
    block = min(n, 16)                                           # noisy counts, not zeros: 16 random frames, repeated
    base = np.clip(rng.poisson(2e4, (block, rows, cols)) + 100, 0, 65535).astype(np.uint16)
    base.reshape(-1)[rng.choice(base.size, size=4 * block, replace=False)] += 9000       # a few zingers
    frames = np.concatenate([base] * ((n + block - 1) // block))[:n]
    res = dict(case="%dx%dx%d" % (n, rows, cols), leg="outlier", reps=reps, device=ctx.device_name(), dif=3000.0)

    def timed(fn):
        fn()                                                     # warm-up
        ctx.sync()
        out = []
        for _ in range(reps):
            ctx.timer_start()
            fn()
            out.append(ctx.timer_stop())
        return float(np.median(out)), float(np.min(out))

    for dtype, name in ((np.uint16, "u16"), (np.float32, "f32")):
        d_in = ctx.to_device(frames.astype(dtype), dtype)
        d_out = ctx.empty(frames.shape, dtype)
        moved = 2.0 * d_in.nbytes                                # read once, written once: what a copy of the buffer moves too
        copy_ms, _ = timed(lambda: d_out.copy_from(d_in))
        res["%s_copy_ms" % name] = round(copy_ms, 3)
        res["%s_copy_GBps" % name] = round(moved / (copy_ms * 1e-3) / 1e9, 1)
        code = preprocess._prep_lib.U16 if dtype == np.uint16 else preprocess._prep_lib.F32
        res["%s_in_place_batch" % name] = preprocess._prep_lib.outlier_batch(rows, cols, code, n, preprocess.DEFAULT_SCRATCH_BYTES)
        for size in (3, 5, 7):
            for where, out in (("out", d_out), ("in_place", d_in)):
                ms, ms_min = timed(lambda: pre.remove_outlier(d_in, 3000.0, size=size, out=out))
                key = "%s_size%d_%s" % (name, size, where)
                res[key + "_ms"] = round(ms, 3)
                res[key + "_min_ms"] = round(ms_min, 3)
                res[key + "_GBps"] = round(moved / (ms * 1e-3) / 1e9, 1)
                res[key + "_vs_copy"] = round(copy_ms / ms, 3)
            d_in.upload(frames.astype(dtype))                    # the in-place runs removed the zingers: put them back
        d_in.free()
        d_out.free()
    _emit(**res)
    pre.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=["1024x1024x1024", "1800x2048x2048"], help="n_proj x rows x cols")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=21)
    ap.add_argument("--passes", nargs="*", default=["large", "dead", "all"], choices=["large", "dead", "all"],
                    help="the large- / dead- / all-stripe passes to time after the sorting pass (none: --passes with no value)")
    ap.add_argument("--legs", nargs="+", default=["prep", "outlier"], choices=["prep", "outlier"],
                    help="prep: normalisation and stripe removal; outlier: remove_outlier, both dtypes, windows 3, 5 and 7")
    a = ap.parse_args()
    for c in a.cases:
        n, rows, cols = (int(v) for v in c.split("x"))
        if "prep" in a.legs:
            case(n, rows, cols, a.reps, a.size, tuple(a.passes))
        if "outlier" in a.legs:
            outlier_case(n, rows, cols, a.reps)


if __name__ == "__main__":
    main()
