#!/usr/bin/env python3
"""Development tool (not the benchmark contract; bench.py is): times align/align_cc.py's two chains on the GPU at sizes users run,
the throughput of phase_cross_correlation_batch, and the reference's CPU path on a few steps of the same data, extrapolated.

    python tools/xcorr_bench.py                                   # 1024 x 1024^2 and 720 x 512^2
    python tools/xcorr_bench.py --cases 720x512 --cpu-steps 2

One JSON line per measurement on stdout.  Per chain: plan creation (host seconds, first call on a fresh handle: includes any JIT
compile of hipFFT kernels), then, on the warmed handle, the device-event times of upload, the n-1 enqueued steps and download, and
per step the bytes a minimal implementation moves (the model below) with the fraction of HBM peak (8.0 TB/s spec) they imply."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

HBM_PEAK = 8.0e12


def _emit(**kw):
    print(json.dumps(kw), flush=True)


def step_bytes(N, path, esz=4, region=150, nx=1024, nz=1024):
    """Bytes per chain step of the kernels and FFTs, each counted once (FFT: one read and one write of the complex plane)."""
    c = 16 * N
    if path == "numpy":
        # reference mean (read) + window (read plane, W; write complex) + FFT + cross power (2 spectra, K; write) + iFFT + |.| argmax
        # (read) + roll (read, write)
        return esz * N + (esz * N + 8 * N + c) + 2 * c + (2 * c + 8 * N + c) + 2 * c + c + 2 * esz * N
    # reference load + FFT + cross power + iFFT + argmax + upsampled DFT (read P, E1; write T; read E0, T) + spline (2 passes r/w
    # of float64 coefficients, input read) + interpolation (read coefficients, write plane)
    updft = c + 16 * region * nz + 16 * region * nx * 2 + 16 * region * nx
    return (esz * N + c) + 2 * c + 3 * c + 2 * c + c + updft + (esz * N + 8 * N * 4) + (8 * N + esz * N)


def series(n, size, seed=0):
    rng = np.random.default_rng(seed)
    f = np.fft.rfft2(rng.standard_normal((size, size)))
    f *= np.exp(-60 * (np.fft.fftfreq(size)[:, None] ** 2 + np.fft.rfftfreq(size)[None] ** 2))
    base = np.fft.irfft2(f, s=(size, size)).astype(np.float32)
    drift = np.clip(np.cumsum(rng.integers(-2, 3, (n, 2)), axis=0), -20, 20)
    return np.stack([np.roll(base, tuple(d), axis=(0, 1)) for d in drift])


def bench_case(n, size, cpu_steps, batch):
    from tomography_alignment_amd.align import align_cc
    from tomography_alignment_amd._xcorr_lib import XcorrHandle
    import xcorr_model

    proj = series(n, size)
    N = size * size
    for path in ("numpy", "skimage"):
        fn = align_cc.cross_correlation_numpy if path == "numpy" else align_cc.cross_correlation_skimage
        with XcorrHandle() as h:
            t0 = time.perf_counter()
            fn(proj[:3], handle=h)                         # plans for batch 1, 2 (and the chunk) + first-launch code loads
            first = time.perf_counter() - t0
            plan_first = h.last_timing()["plan_s"]
            reps = []
            for _ in range(3):
                t0 = time.perf_counter()
                fn(proj, handle=h)
                wall = time.perf_counter() - t0
                reps.append((h.last_timing(), wall))
            plan_full = reps[0][0]["plan_s"]
            best = min(reps, key=lambda r: r[0]["steps_ms"])
            t = best[0]
        per_step_s = t["steps_ms"] / 1e3 / (n - 1)
        b = step_bytes(N, path, nx=size, nz=size)
        cpu = None
        if cpu_steps > 0:
            sub = proj[:cpu_steps + 1]
            t0 = time.perf_counter()
            (xcorr_model.chain_numpy if path == "numpy" else xcorr_model.chain_skimage)(sub)
            cpu = (time.perf_counter() - t0) / cpu_steps
        _emit(case="%dx%d^2" % (n, size), path=path, plan_create_s_first_call=round(plan_first, 4),
              plan_create_s_chunk_plan=round(plan_full, 4), first_call_wall_s=round(first, 3),
              upload_ms=round(t["upload_ms"], 2), steps_ms=round(t["steps_ms"], 2), download_ms=round(t["download_ms"], 2),
              steps_ms_all_reps=[round(r[0]["steps_ms"], 2) for r in reps], wall_s=round(best[1], 3),
              us_per_step=round(per_step_s * 1e6, 1), model_bytes_per_step=b, hbm_frac=round(b / per_step_s / HBM_PEAK, 3),
              cpu_s_per_step=None if cpu is None else round(cpu, 4),
              cpu_chain_s_extrapolated=None if cpu is None else round(cpu * (n - 1), 1),
              speedup_vs_cpu=None if cpu is None else round(cpu * (n - 1) / (t["steps_ms"] / 1e3), 1))
    # batch throughput: B independent pairs, upsample 100
    B = min(batch, n - 1)
    refs = proj[:B].astype(np.float64)
    movs = proj[1:B + 1].astype(np.float64)
    with XcorrHandle() as h:
        align_cc.phase_cross_correlation_batch(refs[:2], movs[:2], upsample_factor=100, handle=h)
        align_cc.phase_cross_correlation_batch(refs, movs, upsample_factor=100, handle=h)
        ms = []
        for _ in range(3):
            align_cc.phase_cross_correlation_batch(refs, movs, upsample_factor=100, handle=h)
            ms.append(h.last_timing()["steps_ms"])
    _emit(case="%dx%d^2" % (n, size), path="pcc_batch", pairs=B, upsample=100, ms_incl_upload=[round(m, 2) for m in ms],
          pairs_per_s=round(B / (min(ms) / 1e3), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1024x1024,720x512")
    ap.add_argument("--cpu-steps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64)
    a = ap.parse_args()
    for c in a.cases.split(","):
        n, size = (int(v) for v in c.split("x"))
        bench_case(n, size, a.cpu_steps, a.batch)


if __name__ == "__main__":
    main()
