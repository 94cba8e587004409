#!/usr/bin/env python3
"""Development tool (not the benchmark contract; bench.py is): the passes of libtomo_vol.so (postprocess) on the GPU.

    python tools/vol_bench.py                       # 1024^3 and 512^3
    python tools/vol_bench.py --case 512

Device events (the context's, around the enqueue-only call) on a warmed handle, the median of --reps (7) runs, set against the time the
pass's bytes take at the rate of a device-to-device copy timed in the same process (a copy moves 2 x its bytes).  The bytes of a pass:
the volume read once (for the cylinder mask: the pi / 4 of it inside) plus what it writes.  The volume is a Shepp-Logan phantom (256^3,
every voxel repeated along the three axes: piecewise constant, the worst case of the histogram's LDS atomics); the histogram is also
timed on uniform random data.  Then, at wall-clock time (the median of the second and third run), export_stack to uint8 without the file
writes against DeviceArray.download() of the float32 volume into a new and into a reused array, and the parts of the export on their
own.  One JSON line per measurement on stdout."""
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


def _fill(d, n, slab_of):
    """Upload slab_of(x0, x1) -> float32 [x1 - x0][n][n] in slabs of 32 planes."""
    for x0 in range(0, n, 32):
        x1 = min(n, x0 + 32)
        d.view(x0 * n * n, (x1 - x0) * n * n).upload(slab_of(x0, x1))


def run(n, reps, end_to_end):
    from tomography_alignment_amd import _lib, postprocess
    from tomography_alignment_amd.utilities import generate_phantom

    ctx = _lib.Context()
    case = "%d^3" % n
    nvox = float(n) ** 3

    def timed(fn):
        fn()                                                     # warm-up
        ctx.sync()
        out = []
        for _ in range(reps):
            ctx.timer_start()
            fn()
            out.append(ctx.timer_stop())
        return float(np.median(out))

    d_v = ctx.empty((n, n, n), np.float32)
    d_w = ctx.empty((n, n, n), np.float32)
    base = min(n, 256)
    rep = n // base
    small = np.asarray(generate_phantom.shepp3d(base), np.float32)
    _fill(d_v, n, lambda x0, x1: np.repeat(np.repeat(small[np.arange(x0, x1) // rep], rep, axis=1), rep, axis=2))
    copy_ms = timed(lambda: d_w.copy_from(d_v))
    copy_gbs = 2.0 * d_v.nbytes / (copy_ms * 1e-3) / 1e9
    _emit(what="d2d_copy", case=case, ms=round(copy_ms, 3), GBps=round(copy_gbs, 1), device=ctx.device_name())

    pp = postprocess.PostProcessor(ctx)
    pp._ready(d_v)
    h, st = pp.handle, ctx.stream()
    r4 = postprocess.region_r4("cylinder", n, n)

    def report(what, ms, nbytes, **kw):
        at_copy = nbytes / (copy_gbs * 1e9) * 1e3
        _emit(what=what, case=case, ms=round(ms, 3), GBps=round(nbytes / ms / 1e6, 1), bytes_at_copy_rate_ms=round(at_copy, 3),
              ratio=round(ms / at_copy, 2), **kw)

    stats = pp.statistics(d_v)
    lo, hi = float(stats.min), float(stats.max)
    report("statistics", timed(lambda: h.stats(st, d_v.ptr, n, n, n, -1, fetch=False)), 4 * nvox)
    report("statistics_cylinder", timed(lambda: h.stats(st, d_v.ptr, n, n, n, r4, fetch=False)), 4 * nvox * np.pi / 4)
    report("histogram_4096", timed(lambda: h.histogram(st, d_v.ptr, n, n, n, -1, lo, hi, 4096, fetch=False)), 4 * nvox, data="shepp-logan")
    report("histogram_256", timed(lambda: h.histogram(st, d_v.ptr, n, n, n, -1, lo, hi, 256, fetch=False)), 4 * nvox, data="shepp-logan")
    rng = np.random.default_rng(0)
    _fill(d_w, n, lambda x0, x1: rng.uniform(lo, hi, (x1 - x0, n, n)).astype(np.float32))
    report("histogram_4096", timed(lambda: h.histogram(st, d_w.ptr, n, n, n, -1, lo, hi, 4096, fetch=False)), 4 * nvox, data="uniform random")
    report("histogram_256", timed(lambda: h.histogram(st, d_w.ptr, n, n, n, -1, lo, hi, 256, fetch=False)), 4 * nvox, data="uniform random")
    report("histogram_16384", timed(lambda: h.histogram(st, d_w.ptr, n, n, n, -1, lo, hi, 16384, fetch=False)), 4 * nvox, data="uniform random")
    report("mask_cylinder", timed(lambda: h.mask(st, d_v.ptr, n, n, n, r4, 0.0, d_w.ptr)), 4 * nvox * (np.pi / 4 + 1))
    for bits in (8, 16):                                         # d_w is scratch from here on: the codes go there
        for order in ("xyz", "zyx"):
            report("quantize_uint%d_%s" % (bits, order),
                   timed(lambda: h.quantize(st, d_v.ptr, n, n, n, -1, lo, hi, bits, postprocess._ORDERS[order], 0, d_w.ptr)), (4 + bits / 8) * nvox)
    for axis in range(3):
        report("project_max_axis%d" % axis, timed(lambda: h.project(st, d_v.ptr, n, n, n, axis, 0, d_w.ptr)), 4 * nvox + 4.0 * n * n)
    d_w.free()

    if end_to_end:
        host = np.empty((n, n, n), np.float32)
        codes = np.empty((n, n, n), np.uint8)

        def wall(fn):
            out = []
            for _ in range(3):
                t0 = time.perf_counter()
                fn()
                out.append(time.perf_counter() - t0)
            return float(np.median(out[1:])) * 1e3

        def quantize_download():
            d_c = pp.quantize(d_v, (lo, hi), np.uint8, "zyx", "cylinder")
            d_c.download(codes)
            d_c.free()

        def previews():
            for a in range(3):
                pp.slice(d_v, a, n // 2).free()
                pp.project(d_v, a).free()
            ctx.sync()

        t = {"export_stack_uint8_no_files": wall(lambda: pp.export_stack(d_v, None, write=False)),
             "download_float32_new_array": wall(lambda: d_v.download()),              # what DeviceArray.download() does by default
             "download_float32_reused_array": wall(lambda: d_v.download(host)),
             "statistics_and_histogram": wall(lambda: pp.histogram(d_v, 4096, None, "cylinder")),
             "quantize_and_download_reused_array": wall(quantize_download),
             "previews": wall(previews),
             "new_uint8_array_first_touch": wall(lambda: np.empty((n, n, n), np.uint8).fill(0))}
        _emit(what="end_to_end", case=case, download_new_over_export=round(t["download_float32_new_array"] / t["export_stack_uint8_no_files"], 2),
              download_reused_over_export=round(t["download_float32_reused_array"] / t["export_stack_uint8_no_files"], 2),
              **{k + "_ms": round(v, 1) for k, v in t.items()})
    pp.close()
    d_v.free()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", type=int, action="append", metavar="N", help="the edge of the cubic volume (a multiple of 256, or below it)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-end-to-end", action="store_true")
    a = ap.parse_args()
    for n in (a.case or [1024, 512]):
        run(n, a.reps, not a.no_end_to_end)


if __name__ == "__main__":
    main()
