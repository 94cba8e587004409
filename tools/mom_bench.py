#!/usr/bin/env python3
"""Development tool (not the benchmark contract; bench.py is): the marginals pass of libtomo_mom.so on the GPU.

    python tools/mom_bench.py                       # 1024 x 1024 x 1024 and 720 x 512 x 512
    python tools/mom_bench.py --case 720 512 512

Device events (the context's, around the enqueue-only call) on a warmed handle, the median of --reps (7) runs, set against the time the
pass's bytes take at the rate of a device-to-device copy timed in the same process (a copy moves 2 x its bytes).  The bytes: p read once,
plus the partial sums written and read (per projection 8 nz ceil(nx / 128) + 8 nx ceil(nz / 1024) + 4 per work-group) and the tables
written.  Also the wall time of the whole marginals() call on a device-resident stack (with the tables handed to the host) and of the
numpy estimator that follows, both vertical modes.  One JSON line per measurement on stdout."""
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


def run(n, nx, nz, reps):
    from tomography_alignment_amd import _lib, _mom_lib
    from tomography_alignment_amd.align import consistency

    ctx = _lib.Context()
    case = "%d x %d x %d" % (n, nx, nz)

    def timed(fn):
        fn()                                                     # warm-up
        ctx.sync()
        out = []
        for _ in range(reps):
            ctx.timer_start()
            fn()
            out.append(ctx.timer_stop())
        return float(np.median(out))

    d_p = ctx.empty((n, nx, nz), np.float32)
    d_q = ctx.empty((n, nx, nz), np.float32)
    block = np.random.default_rng(0).uniform(0.0, 1.0, (1, nx, nz)).astype(np.float32)
    for i in range(n):                                           # the same frame in every projection: the content does not matter here
        d_p.view(i * nx * nz, nx * nz).upload(block)
    copy_ms = timed(lambda: d_q.copy_from(d_p))
    copy_gbs = 2.0 * d_p.nbytes / (copy_ms * 1e-3) / 1e9
    d_q.free()
    _emit(what="d2d_copy", case=case, ms=round(copy_ms, 3), GBps=round(copy_gbs, 1), device=ctx.device_name())

    cons = consistency.Consistency(ctx)
    cons._ready(d_p)
    h = cons.handle
    for budget, name in ((0, "no limit"), (consistency.DEFAULT_SCRATCH, "default 2 GiB"), (_mom_lib.scratch_bytes(nx, nz), "one projection")):
        h.set_max_scratch(budget)
        ms = timed(lambda: h.marginals(ctx.stream(), d_p.ptr, n, nx, nz, fetch=False))
        partial = float(n) * _mom_lib.scratch_bytes(nx, nz)
        nbytes = d_p.nbytes + 2.0 * partial + 8.0 * n * (nx + nz) + 4.0 * n
        at_copy = nbytes / (copy_gbs * 1e9) * 1e3
        _emit(what="marginals", case=case, scratch=name, batch=_mom_lib.batch(n, nx, nz, budget), ms=round(ms, 3), GBps_of_p=round(d_p.nbytes / ms / 1e6, 1),
              bytes_at_copy_rate_ms=round(at_copy, 3), ratio=round(ms / at_copy, 2), partials_MB=round(partial / 1e6, 1),
              handle_MB=round(h.device_bytes() / 1e6, 1))
    h.set_max_scratch(consistency.DEFAULT_SCRATCH)
    ms_w = timed(lambda: h.marginals(ctx.stream(), d_p.ptr, n, nx, nz, z0=nz // 4, z1=3 * nz // 4, fetch=False))
    _emit(what="marginals_half_window", case=case, ms=round(ms_w, 3))

    walls = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        m = cons.marginals(d_p)
        walls.append(time.perf_counter() - t0)
    _emit(what="marginals_call", case=case, wall_ms=round(float(np.median(walls[1:])) * 1e3, 3))
    phi = np.arange(n) * np.pi / n
    for vertical in ("moment", "profile"):
        t0 = time.perf_counter()
        consistency.shifts_from_marginals(m, phi, vertical=vertical)
        _emit(what="estimator_numpy", case=case, vertical=vertical, wall_ms=round((time.perf_counter() - t0) * 1e3, 3))
    cons.close()
    d_p.free()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", type=int, nargs=3, action="append", metavar=("N", "NX", "NZ"), help="projections, detector columns, detector rows")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    for n, nx, nz in (a.case or [(1024, 1024, 1024), (720, 512, 512)]):
        run(n, nx, nz, a.reps)


if __name__ == "__main__":
    main()
