#!/usr/bin/env python3
"""Development tool (not the benchmark contract; bench.py is): times recon/fbp.py on the GPU -- the ramp filter (libtomo_fbp.so), the
back-projection (tomo_adjoint), the whole FBP -- and one SIRT iteration in the same run, with the tomo context's events after warm-up.

    python tools/fbp_bench.py                       # 1024^3 x 1024 angles and 512^3 x 720
    python tools/fbp_bench.py --cases 512x720 --reps 3

One JSON line per case on stdout.  The filter moves n_proj * ndx * ndz * 4 bytes in and as many out (the kernel reads each value once
and writes it once); GB/s is reported against the 8.0 TB/s HBM peak and the 6.29 TB/s the copy kernel reaches (round 6)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

HBM_PEAK = 8.0e12
COPY_RATE = 6.29e12


def _emit(**kw):
    print(json.dumps(kw), flush=True)


def case(N, n_proj, reps, sirt_reps, filt):
    from tomography_alignment_amd.backend import HipBackend
    from tomography_alignment_amd.recon import fbp, sirt
    from tomography_alignment_amd.utilities.geometry import Geometry

    geo = Geometry(n_proj, np.array([N, N, N]), np.ones(3), np.array([N, N]), np.ones(2))
    be = HipBackend(geo)
    ctx = be.ctx
    phi = np.linspace(0, np.pi, n_proj, endpoint=False)
    angles = np.array([phi, 0 * phi, 0 * phi]).T
    xyz = np.zeros((n_proj, 3))
    d_p = be.empty(n_proj * N * N)
    be.fill(d_p, 1.0)
    d_q = be.empty(n_proj * N * N)
    f = fbp.FBP(geo, d_p, angles, xyz, options={"_backend": be, "filter": filt})
    f.d_rec = be.empty(be.n_vox)
    stream = ctx.stream()

    def timed(fn, n):
        fn()                                   # warm-up
        ctx.sync()
        out = []
        for _ in range(n):
            ctx.timer_start()
            fn()
            out.append(ctx.timer_stop())
        return float(np.median(out)), float(np.min(out))

    flt = lambda: f.handle.filter(stream, d_p.ptr, d_q.ptr, n_proj, N, N, f.scales)      # noqa: E731 (the input stays as it is)
    adj = lambda: f.proj_mat.T.apply(d_q, f.d_rec)                                       # noqa: E731

    def fbp_device():                          # FBP.run without the download of the volume
        f.proj_mat.T.apply(f.filtered(), f.d_rec)
    filt_ms, filt_min = timed(flt, reps)
    adj_ms, adj_min = timed(adj, reps)
    tot_ms, _ = timed(fbp_device, max(1, reps // 2))
    moved = 2.0 * n_proj * N * N * 4
    gbs = moved / (filt_ms * 1e-3)
    # one SIRT iteration on the same geometry, in the same process (its buffers are allocated after the FBP's are freed)
    f = d_q = None
    s = sirt.SIRT(geo, d_p, angles, xyz, options={"_backend": be})
    s.iterate_device(niter=1)
    ctx.sync()
    it = []
    for _ in range(sirt_reps):
        t0 = time.perf_counter()
        ctx.timer_start()
        s.iterate_device(niter=1)
        it.append((ctx.timer_stop(), time.perf_counter() - t0))
    sirt_ms = float(np.median([a for a, _ in it]))
    _emit(case="%d^3 x %d" % (N, n_proj), filter=filt, filter_ms=round(filt_ms, 3), filter_min_ms=round(filt_min, 3),
          filter_GBps=round(gbs / 1e9, 1), filter_of_peak=round(gbs / HBM_PEAK, 3), filter_of_copy=round(gbs / COPY_RATE, 3),
          adjoint_ms=round(adj_ms, 2), filter_over_adjoint=round(filt_ms / adj_ms, 4), fbp_total_s=round(tot_ms / 1e3, 4),
          sirt_iteration_s=round(sirt_ms / 1e3, 4), fbp_over_sirt_iteration=round(tot_ms / sirt_ms, 3),
          lib=os.path.basename(os.environ.get("TOMO_FBP_LIB", "libtomo_fbp.so")))
    s = None
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1024x1024,512x720", help="comma-separated NxANGLES (N^3 volume, N x N detector)")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sirt-reps", type=int, default=3)
    ap.add_argument("--filter", default="ramp")
    a = ap.parse_args()
    for c in a.cases.split(","):
        N, n = (int(v) for v in c.split("x"))
        case(N, n, a.reps, a.sirt_reps, a.filter)


if __name__ == "__main__":
    main()
