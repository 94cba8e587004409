#!/usr/bin/env python3
"""Development tool (not the benchmark contract; bench.py is): the search and the stitch of libtomo_half.so on the GPU.

    python tools/half_bench.py                                   # search at 1800 x 2048, 16 rows; stitch at 1800 x 2048 x 2048
    python tools/half_bench.py --search 900 2048 16 256 --stitch 900 1024 1024

Device events (the context's, around enqueue-only calls) on a warmed handle, the median of --reps (7) runs.  The search: the gather of the
detector rows and the three kernels of tomo_half_search (column sums, band sums of the Gram, fold), window max(8, nx // 8) unless given.
The stitch: its time, the bytes it must move (p read once, the stitched series written once) per second, and that set against the rate
of a device-to-device copy timed in the same process (a copy moves 2 x its bytes).  One JSON line per measurement on stdout."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def _emit(**kw):
    print(json.dumps(kw), flush=True)


def _timed(ctx, fn, reps):
    fn()                                                         # warm-up
    ctx.sync()
    out = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        out.append(ctx.timer_stop())
    return float(np.median(out))


def _fill(d, frame, count):
    for i in range(count):                                       # the same frame in every projection: the content does not matter here
        d.view(i * frame.size, frame.size).upload(frame)


def search(ctx, n, nx, nrows, w, reps):
    from tomography_alignment_amd import _half_lib, half_acquisition
    w = half_acquisition.default_window(nx) if w is None else w
    nz = max(nrows, 16)
    case = "%d x %d, %d rows of %d, window %d" % (n, nx, nrows, nz, w)
    d_p = ctx.empty((n, nx, nz), np.float32)
    _fill(d_p, np.random.default_rng(0).uniform(0.0, 1.0, (nx, nz)).astype(np.float32), n)
    rows = np.unique(np.linspace(0, nz - 1, nrows).astype(np.int64))
    owner = half_acquisition.HalfAcquisition(ctx)
    owner._ready(d_p)
    h = owner.handle
    gather_ms = _timed(ctx, lambda: h.load_rows(ctx.stream(), d_p.ptr, n, nx, nz, n, rows), reps)
    search_ms = _timed(ctx, lambda: h.search(ctx.stream(), w, fetch=False), reps)
    fma = 2.0 * rows.size * (n // 2) * w * nx                    # float64 multiply-adds of the band sums, both sides
    _emit(what="search", case=case, gather_ms=round(gather_ms, 3), search_ms=round(search_ms, 3), band_GFMA_per_s=round(fma / search_ms / 1e6, 1),
          partials_MB=round(rows.size * _half_lib.scratch_bytes(nx, w) / 1e6, 1), handle_MB=round(h.device_bytes() / 1e6, 1), device=ctx.device_name())
    owner.close()
    d_p.free()


def stitch(ctx, n, nx, nz, reps):
    from tomography_alignment_amd import half_acquisition
    case = "%d x %d x %d" % (n, nx, nz)
    d_p = ctx.empty((n, nx, nz), np.float32)
    _fill(d_p, np.random.default_rng(1).uniform(0.0, 1.0, (nx, nz)).astype(np.float32), n)
    d_q = ctx.empty((n, nx, nz), np.float32)
    copy_ms = _timed(ctx, lambda: d_q.copy_from(d_p), reps)
    copy_gbs = 2.0 * d_p.nbytes / (copy_ms * 1e-3) / 1e9
    d_q.free()
    _emit(what="d2d_copy", case=case, ms=round(copy_ms, 3), GBps=round(copy_gbs, 1), device=ctx.device_name())
    owner = half_acquisition.HalfAcquisition(ctx)
    owner._ready(d_p)
    h = owner.handle
    for c, name in ((nx - 1 - 0.0625 * nx, "2c integer"), (nx - 1 - 0.0625 * nx + 0.3, "fractional")):
        hh, W, _ = half_acquisition.stitched_shape(n, nx, c)
        d_out = ctx.empty((hh, W, nz), np.float32)
        ms = _timed(ctx, lambda: h.stitch(ctx.stream(), d_p.ptr, n, nx, nz, c, d_out.ptr), reps)
        nbytes = float(d_p.nbytes + d_out.nbytes)
        _emit(what="stitch", case=case, axis=name, center=c, W=W, ms=round(ms, 3), GBps=round(nbytes / ms / 1e6, 1),
              of_copy_rate=round(nbytes / ms / 1e6 / copy_gbs, 3))
        d_out.free()
    owner.close()
    d_p.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--search", type=int, nargs="+", action="append", metavar="N NX ROWS [W]", help="projections, detector columns, detector rows, window")
    ap.add_argument("--stitch", type=int, nargs=3, action="append", metavar=("N", "NX", "NZ"), help="projections, detector columns, detector rows")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    from tomography_alignment_amd import _lib
    ctx = _lib.Context()
    default = not (a.search or a.stitch)
    for s in (a.search or ([[1800, 2048, 16]] if default else [])):
        if len(s) not in (3, 4):
            ap.error("--search takes N NX ROWS [W]")
        search(ctx, s[0], s[1], s[2], s[3] if len(s) == 4 else None, a.reps)
    for n, nx, nz in (a.stitch or ([(1800, 2048, 2048)] if default else [])):
        stitch(ctx, n, nx, nz, a.reps)
    ctx.close()


if __name__ == "__main__":
    main()
