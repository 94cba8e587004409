#!/usr/bin/env python3
"""Development tool (not the benchmark contract; bench.py is): seconds per iteration of RegularizedRecon's four methods and the
bandwidth of its fused vector passes (csrc/tomo_reg.hip) at N^3 x n_proj, untilted Shepp-Logan data generated on the device.

    python tools/regularized_bench.py --N 512 --n-proj 512 [--iters 2] [--methods fista,tikh,ista,acc]
    python tools/regularized_bench.py --N 512 --n-proj 512 --rocprof OUTDIR     # the same run under rocprofv3 --kernel-trace --stats,
                                                                                # then the per-kernel split from its kernel_stats.csv

One JSON line per measurement on stdout.  Per method: wall seconds per iteration (after one warm-up iteration) and the split the context's
own kernel timer sees (the new passes, the TV prox, the rest = projectors).  Per fused pass: GB/s over the bytes it must move."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

REG_KERNELS = ("k_reg_fista_momentum", "k_reg_tikh_grad", "k_reg_trial", "k_reg_clamp_err", "k_reg_prox_l1_trial", "k_reg_prox_l1_momentum",
               "k_reg_residual", "k_reg_final")
TV_KERNELS = ("k_tv_error", "k_tv_update", "k_tv_gap_det", "k_tv_iso_det")


def _emit(**kw):
    print(json.dumps(kw), flush=True)


def vector_passes(be, ctx, n, reps=5):
    """GB/s of each fused pass over n float32 elements (bytes = what the pass must read and write)."""
    bufs = [be.empty(n) for _ in range(5)]
    for b_ in bufs:
        be.fill(b_, 0.5)
    a, b, c, d, o = bufs
    passes = [
        ("fista_momentum+gt", 16, lambda: be.fista_momentum(o, a, b, 0.3, gt=c, slot=0)),
        ("tikh_grad", 12, lambda: be.tikh_grad(o, a, 0.1, slot=0)),
        ("trial", 12, lambda: be.trial(o, a, b, -0.01, slot=0)),
        ("clamp_err+gt", 12, lambda: be.clamp_err(o, True, c, slot=0)),
        ("prox_l1_trial", 12, lambda: be.prox_l1_trial(o, a, b, 0.01, 0.001, slot=0)),
        ("prox_l1_momentum+gt", 20, lambda: be.prox_l1_momentum(o, a, b, c, 0.2, 0.01, 0.001, gt=d, slot=0)),
        ("residual_acc", 12, lambda: be.residual_acc(o, a, b, slot=0)),
    ]
    for name, bpe, fn in passes:
        be.acc_zero(0, 4)
        fn()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        ctx.sync()
        dt = (time.perf_counter() - t0) / reps
        _emit(kind="vector_pass", pass_=name, n=n, ms=1e3 * dt, GBps=bpe * n / dt / 1e9)


def solver_iterations(N, n_proj, iters, methods):
    from tomography_alignment_amd.backend import HipBackend
    from tomography_alignment_amd.recon.regularized import RegularizedRecon
    from tomography_alignment_amd.utilities.generate_phantom import SHEPP_LOGAN
    from tomography_alignment_amd.utilities.geometry import Geometry
    from tomography_alignment_amd.utilities.projection_operators import ProjectionMatrix
    phi = np.linspace(0., np.pi, n_proj, endpoint=False)
    z, xyz = np.zeros(n_proj), np.zeros((n_proj, 3))
    geo = Geometry(n_proj, np.array([N, N, N]), np.ones(3), np.array([N, N]), np.ones(2))
    be = HipBackend(geo)
    ctx = be.ctx
    d_gt = be.phantom(be.empty(N ** 3), (N, N, N), SHEPP_LOGAN)
    d_b = ProjectionMatrix(geo, backend=be).projection_matrix(alpha=z, beta=z, phi=phi, xyz_shift=xyz).apply(d_gt)
    lip = float(n_proj * N)                      # ~ the largest eigenvalue of A^T A for this geometry (constant vector)
    runs = {"fista": ("run_fista", dict(hyper=2.0 * lip, beta_tv=0.1, niter_tv=20)),
            "tikh": ("run_tikhonov_gd", dict(reg_param=0.1, positivity=True)),
            "ista": ("run_lasso_ista", dict(reg_param=1.0, alpha0=2.0 / lip, beta=0.5)),
            "acc": ("run_lasso_accelerated", dict(reg_param=1.0, alpha0=2.0 / lip, beta=0.5))}
    for m in methods:
        meth, kw = runs[m]
        r = RegularizedRecon(geo, d_b, np.array([phi, z, z]).T, xyz, options={"ground_truth": d_gt, "_backend": be})
        getattr(r, meth)(niter=1, **kw)                                      # warm-up: workspaces, code objects
        ctx.sync()
        ctx.profile_reset()
        ctx.profile_enable(True)
        t0 = time.perf_counter()
        _, rms = getattr(r, meth)(niter=iters, **kw)
        ctx.sync()
        dt = time.perf_counter() - t0
        ctx.profile_enable(False)
        k = len(rms)
        reg = {nm: ctx.profile_get(nm)[1] / k for nm in REG_KERNELS if ctx.profile_get(nm)[0]}
        tv = sum(ctx.profile_get(nm)[1] for nm in TV_KERNELS) / k
        _emit(kind="iteration", method=m, N=N, n_proj=n_proj, iters=k, s_per_iter=dt / k, fused_ms=sum(reg.values()), tv_prox_ms=tv,
              fused_split_ms=reg, n_feval=[int(v) for v in (r.n_feval if r.n_feval is not None else [])],
              rms_last=float(rms[-1]))
        del r
    vector_passes(be, ctx, N ** 3)


def rocprof_split(outdir, argv):
    """Run this tool under rocprofv3 --kernel-trace --stats (a child process) and print the per-kernel totals."""
    os.makedirs(outdir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "-o", "run", "--", sys.executable, os.path.abspath(__file__)] + argv
    rc = subprocess.call(cmd)
    if rc != 0:
        raise SystemExit(rc)
    files = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("no kernel_stats.csv under %s" % outdir)
    rows = list(csv.DictReader(open(files[0])))
    tot = sum(float(r_["TotalDurationNs"]) for r_ in rows)
    for r_ in sorted(rows, key=lambda r_: -float(r_["TotalDurationNs"]))[:25]:
        _emit(kind="rocprof_kernel", name=r_["Name"][:80], calls=int(r_["Calls"]), total_ms=float(r_["TotalDurationNs"]) / 1e6,
              avg_us=float(r_["AverageNs"]) / 1e3, share=float(r_["TotalDurationNs"]) / tot)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=512)
    ap.add_argument("--n-proj", type=int, default=None)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--methods", default="fista,tikh,ista,acc")
    ap.add_argument("--rocprof", default=None, help="output directory: run under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    if a.rocprof:
        args = sys.argv[1:]
        argv = [x for i, x in enumerate(args) if x != "--rocprof" and (i == 0 or args[i - 1] != "--rocprof")]
        rocprof_split(a.rocprof, argv)
        return
    solver_iterations(a.N, a.n_proj or a.N, a.iters, [m for m in a.methods.split(",") if m])


if __name__ == "__main__":
    main()
