#!/usr/bin/env python3
"""Development tool (not the benchmark contract; bench.py is): the rotation-axis search of libtomo_cor.so on the GPU.

    python tools/cor_bench.py                       # 1800 x 2048 (one row and 16 rows) and 720 x 512
    python tools/cor_bench.py --case 720 512 1

Device events (the library's own, around each pass) on a warmed handle, the median of --reps (7) runs: gather and prefilter of one
load, and build, R2C and reduce of the coarse list of the default search (201 candidates per row), each hand-written kernel's bytes set
against a device-to-device copy timed in the same process (a copy moves 2 x its bytes).  Also the time to make the hipFFT plans, the
device bytes the handle holds, the wall time of the whole find_center call on a device-resident sinogram, and -- for sinograms of at
most --model-max values -- the numpy model of tests/cor_model.py on one host core.  One JSON line per measurement on stdout."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

NZ = 64         # detector rows of the device sinogram p[n][nx][nz]: z is the fastest axis, so one row is read with a stride of nz floats


def _emit(**kw):
    print(json.dumps(kw), flush=True)


def run(n, nx, nrows, reps, model_max):
    import cor_model as cm
    from tomography_alignment_amd import _cor_lib, _lib, rotation_axis

    ctx = _lib.Context()
    case = "%d x %d, %d row%s" % (n, nx, nrows, "" if nrows == 1 else "s")

    def timed(fn):
        fn()                                                     # warm-up
        ctx.sync()
        out = []
        for _ in range(reps):
            ctx.timer_start()
            fn()
            out.append(ctx.timer_stop())
        return float(np.median(out))

    S = cm.ellipse_sinogram(n, nx, 7.25, seed=0, noise=0.02)
    d_p = ctx.to_device(np.ascontiguousarray(np.broadcast_to(S[:, :, None], (n, nx, NZ))))
    d_q = ctx.empty(d_p.shape, np.float32)
    copy_ms = timed(lambda: d_q.copy_from(d_p))
    copy_gbs = 2.0 * d_p.nbytes / (copy_ms * 1e-3) / 1e9
    d_q.free()
    _emit(what="d2d_copy", case=case, ms=round(copy_ms, 3), GBps=round(copy_gbs, 1), device=ctx.device_name())

    def at_copy_rate(nbytes):
        return nbytes / (copy_gbs * 1e9) * 1e3

    axis = rotation_axis.RotationAxis(ctx)
    rows = rotation_axis.spread_rows(NZ, nrows)
    assert rows.size == nrows
    tc = rotation_axis.coarse_list(-50, 50)
    slices, ts = np.repeat(np.arange(nrows), tc.size), np.tile(tc, nrows)
    half = 0.5 + tc                                              # the same count of candidates, all on the spline path

    t0 = time.perf_counter()
    axis.load(d_p, rows=rows)
    axis.metric(slices, ts)
    first_wall = time.perf_counter() - t0
    h = axis.handle
    _emit(what="first_call", case=case, wall_s=round(first_wall, 3), plan_s=round(h.plan_seconds(), 3), handle_GB=round(h.device_bytes() / 1e9, 3),
          batch=_cor_lib.batch(slices.size, n, nx, rotation_axis.DEFAULT_SCRATCH))

    loads = np.array([axis.load(d_p, rows=rows, timed=True)[3] for _ in range(reps + 1)][1:])
    g_ms, p_ms = (float(v) for v in np.median(loads, axis=0))
    elems = float(nrows) * n * nx
    g_bytes = 8.0 * elems                                        # the values read and written; every value read pulls a line of its own
    p_bytes = 28.0 * elems                                       # S read, the coefficients written, read and written again
    _emit(what="gather", case=case, ms=round(g_ms, 4), bytes_at_copy_rate_ms=round(at_copy_rate(g_bytes), 4), ratio=round(g_ms / at_copy_rate(g_bytes), 2),
          lines_touched_at_copy_rate_ms=round(at_copy_rate(elems * (min(128.0, 4.0 * NZ) + 4.0)), 4))
    _emit(what="prefilter", case=case, ms=round(p_ms, 4), bytes_at_copy_rate_ms=round(at_copy_rate(p_bytes), 4), ratio=round(p_ms / at_copy_rate(p_bytes), 2))

    R, H = 2 * n, nx // 2 + 1
    hi = _cor_lib.wedge(n, nx)
    masked = float(np.sum(np.maximum(np.minimum(hi, H - 1) - 1, 0)))      # complex values of one spectrum that count
    for name, tt, src_bytes in (("integer", ts, 4.0), ("spline", np.tile(half, nrows), 8.0)):
        runs = np.array([axis.metric(slices, tt, timed=True)[1] for _ in range(reps + 1)][1:])
        b_ms, f_ms, r_ms = (float(v) for v in np.median(runs, axis=0))
        pairs = float(tt.size)
        b_bytes = pairs * (4.0 * R * 2 * H + 4.0 * n * nx + src_bytes * n * nx)     # the buffer written, S read, the B half's source read
        r_bytes = pairs * 8.0 * masked
        _emit(what="metric_" + name, case=case, pairs=int(pairs), build_ms=round(b_ms, 3), r2c_ms=round(f_ms, 3), reduce_ms=round(r_ms, 3),
              build_bytes_at_copy_rate_ms=round(at_copy_rate(b_bytes), 3), build_ratio=round(b_ms / at_copy_rate(b_bytes), 2),
              reduce_bytes_at_copy_rate_ms=round(at_copy_rate(r_bytes), 3), reduce_ratio=round(r_ms / at_copy_rate(r_bytes), 2),
              masked_fraction=round(masked / (R * H), 3), r2c_GFLOPs=round(pairs * 2.5 * R * nx * np.log2(float(R) * nx) / (f_ms * 1e-3) / 1e9, 1))

    walls = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        found = axis.find_center(d_p, rows=rows)
        walls.append(time.perf_counter() - t0)
    _emit(what="find_center", case=case, wall_ms=round(float(np.median(walls[1:])) * 1e3, 3), offset=found.offset, candidates=int(nrows * (tc.size + 49)))
    axis.close()
    d_p.free()
    ctx.close()
    if n * nx <= model_max:
        t0 = time.perf_counter()
        r = cm.find_center(S)
        _emit(what="numpy_model_one_core", case="%d x %d, 1 row" % (n, nx), wall_s=round(time.perf_counter() - t0, 3), offset=r.offset)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", type=int, nargs=3, action="append", metavar=("N", "NX", "ROWS"), help="angles, columns, detector rows searched")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--model-max", type=int, default=720 * 512, help="time the numpy model for sinograms of at most this many values")
    a = ap.parse_args()
    for n, nx, nrows in (a.case or [(1800, 2048, 1), (1800, 2048, 16), (720, 512, 1)]):
        run(n, nx, nrows, a.reps, a.model_max)


if __name__ == "__main__":
    main()
