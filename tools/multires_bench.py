#!/usr/bin/env python3
"""Development tool (not the benchmark contract; bench.py is): the resolution pyramid on the GPU.

    python tools/multires_bench.py kernels                       # the three kernels of libtomo_pyr.so at 1024 x 1024^2 / 1024^3
    python tools/multires_bench.py align --size 512 --angles 720 --outer 12 --sirt-iters 60

kernels: device events on a warmed handle; bytes moved (every input read once, every output written once) per second, next to a
device-to-device copy timed in the same process (a copy moves 2 x its bytes).  align: on generate_data.make's data, wall time and pose
errors per outer iteration of examples/align_rigid.run_multires(levels=3) against `run` with the same sirt_iters, so that the time to reach
a given tilt and shift error can be read off both.  One JSON line per measurement on stdout."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def _emit(**kw):
    print(json.dumps(kw), flush=True)


def kernels(n, reps):
    from tomography_alignment_amd import _lib, multires

    ctx = _lib.Context()
    pyr = multires.Pyramid(ctx)

    def timed(fn):
        fn()                                                     # warm-up
        ctx.sync()
        out = []
        for _ in range(reps):
            ctx.timer_start()
            fn()
            out.append(ctx.timer_stop())
        return float(np.median(out)), float(np.min(out))

    src = ctx.zeros((n, n, n), np.float32)                       # the kernels' work does not depend on the values
    dst = ctx.empty((n, n, n), np.float32)
    copy_ms, _ = timed(lambda: dst.copy_from(src))
    copy_gbs = 2.0 * src.nbytes / (copy_ms * 1e-3) / 1e9
    dst.free()
    _emit(what="d2d_copy", size=n, ms=round(copy_ms, 3), GBps=round(copy_gbs, 1), device=ctx.device_name())
    for f in (2, 4, 8):
        for name, call, n_out in (("bin_projections", pyr.bin_projections, n ** 3 // f ** 2), ("bin_volume", pyr.bin_volume, n ** 3 // f ** 3)):
            out = ctx.empty((n_out,), np.float32)
            ms, mn = timed(lambda: call(src, f, out=out))
            gbs = 4.0 * (n ** 3 + n_out) / (ms * 1e-3) / 1e9
            _emit(what=name, shape=[n, n, n], f=f, ms=round(ms, 3), min_ms=round(mn, 3), GBps=round(gbs, 1), vs_copy=round(gbs / copy_gbs, 3))
            out.free()
    src.free()
    h = n // 2
    coarse, fine = ctx.zeros((h, h, h), np.float32), ctx.empty((n, n, n), np.float32)
    ms, mn = timed(lambda: pyr.prolong_volume(coarse, out=fine))
    gbs = 4.0 * (h ** 3 + n ** 3) / (ms * 1e-3) / 1e9
    _emit(what="prolong_volume", coarse=[h, h, h], fine=[n, n, n], ms=round(ms, 3), min_ms=round(mn, 3), GBps=round(gbs, 1),
          vs_copy=round(gbs / copy_gbs, 3))
    pyr.close()
    ctx.close()


def align(size, angles, outer, sirt_iters, n_outer_levels, seed):
    from tomography_alignment_amd.examples import align_rigid, generate_data

    t0 = time.perf_counter()
    data = generate_data.make(size, angles, seed=seed)
    _emit(what="data", size=size, angles=angles, seconds=round(time.perf_counter() - t0, 1))
    for name, fn in (("run_multires", lambda: align_rigid.run_multires(dict(data), levels=3, n_outer=n_outer_levels, sirt_iters=sirt_iters,
                                                                       verbose=False, download=False)),
                     ("run", lambda: align_rigid.run(dict(data), n_outer=outer, sirt_iters=sirt_iters, verbose=False, download=False))):
        t0 = time.perf_counter()
        hist = fn()[4]
        wall = time.perf_counter() - t0
        t = 0.0
        for h in hist:
            t += h["sirt_wall_s"] + h["align_wall_s"]
            _emit(what=name, outer=h["outer"], factor=h.get("factor", 1), cumulative_s=round(t, 2), sirt_s=h["sirt_wall_s"], align_s=h["align_wall_s"],
                  rmse=round(h["rmse"], 4), shift_err_px=round(h["shift_err_px"], 4), tilt_err_deg=round(h["tilt_err_deg"], 4))
        _emit(what=name + "_total", wall_s=round(wall, 2), sirt_iters=sirt_iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("kernels", "align"))
    ap.add_argument("--n", type=int, default=1024, help="kernels: the cube edge")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--angles", type=int, default=720)
    ap.add_argument("--outer", type=int, default=12, help="outer iterations of the plain `run`")
    ap.add_argument("--levels-outer", type=int, nargs=3, default=[3, 3, 2], help="outer iterations per level, coarsest first")
    ap.add_argument("--sirt-iters", type=int, default=60)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if a.mode == "kernels":
        kernels(a.n, a.reps)
    else:
        align(a.size, a.angles, a.outer, a.sirt_iters, tuple(a.levels_outer), a.seed)


if __name__ == "__main__":
    main()
