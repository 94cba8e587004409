#!/usr/bin/env python3
"""Development tool (not the benchmark contract; bench.py is): the passes of libtomo_seg.so (segment) on the GPU.

    python tools/seg_bench.py                       # 1024^3 and 512^3
    python tools/seg_bench.py --case 512

Device events (the context's) around each call on a warmed handle, the median of --reps (5) runs, set against the time the pass's
compulsory bytes take at the rate of a device-to-device copy timed in the same process (a copy moves 2 x its bytes).  The compulsory
bytes: threshold reads 4 and writes 1 per voxel; label reads the mask (1) and writes the labels (4); measure reads the labels (4, with
the volume 8); remove_small reads and writes the labels (8).  label, measure and remove_small hand a number or a table to the host, so
their times include that wait.  The masks: the Shepp-Logan phantom (256^3, every voxel repeated) thresholded at Otsu's threshold, and
Bernoulli masks of density 0.1, 0.3116 (the site-percolation threshold of the cubic lattice) and 0.6.  For the 512^3 masks
scipy.ndimage.label on the host is timed too where scipy can be imported.  One JSON line per measurement on stdout."""
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


def _fill(d, n, slab_of, dtype):
    """Upload slab_of(x0, x1) -> [x1 - x0][n][n] in slabs of 32 planes."""
    for x0 in range(0, n, 32):
        x1 = min(n, x0 + 32)
        d.view(x0 * n * n, (x1 - x0) * n * n).upload(np.ascontiguousarray(slab_of(x0, x1), dtype))


def run(n, reps, host_scipy):
    from tomography_alignment_amd import _lib, _seg_lib, segment
    from tomography_alignment_amd.utilities import generate_phantom

    ctx = _lib.Context()
    case = "%d^3" % n
    nvox = float(n) ** 3

    def timed(fn, reps=reps):
        fn()                                                     # warm-up
        ctx.sync()
        out = []
        for _ in range(reps):
            ctx.timer_start()
            fn()
            out.append(ctx.timer_stop())
        return float(np.median(out))

    d_v = ctx.empty((n, n, n), np.float32)
    d_l = ctx.empty((n, n, n), np.int32)
    d_l2 = ctx.empty((n, n, n), np.int32)
    d_m = ctx.empty((n, n, n), np.uint8)
    base = min(n, 256)
    rep = n // base
    small = np.asarray(generate_phantom.shepp3d(base), np.float32)
    _fill(d_v, n, lambda x0, x1: np.repeat(np.repeat(small[np.arange(x0, x1) // rep], rep, axis=1), rep, axis=2), np.float32)
    copy_ms = timed(lambda: d_l.copy_from(d_v), 7)
    copy_gbs = 2.0 * d_v.nbytes / (copy_ms * 1e-3) / 1e9
    _emit(what="d2d_copy", case=case, ms=round(copy_ms, 3), GBps=round(copy_gbs, 1), device=ctx.device_name())

    seg = segment.Segmenter(ctx)
    seg._ready(d_v)
    h, st = seg.handle, ctx.stream()

    def report(what, ms, nbytes, **kw):
        at_copy = nbytes / (copy_gbs * 1e9) * 1e3
        _emit(what=what, case=case, ms=round(ms, 3), bytes_at_copy_rate_ms=round(at_copy, 3), ratio=round(ms / at_copy, 2), **kw)

    t_otsu, = seg.otsu(d_v, region="cylinder")
    report("threshold", timed(lambda: h.threshold(st, d_v.ptr, n, n, n, -1, t_otsu, None, d_m.ptr)), 5 * nvox, data="shepp-logan")
    rng = np.random.default_rng(0)
    masks = [("shepp-logan >= otsu", None)] + [("bernoulli %g" % p, p) for p in (0.1, 0.3116, 0.6)]
    for name, p in masks:
        if p is not None:
            _fill(d_m, n, lambda x0, x1: rng.random((x1 - x0, n, n), np.float32) < p, np.uint8)
        host_mask = d_m.download() if (host_scipy and n <= 512) else None
        for c in (1, 2, 3):
            count = [0]

            def lab():
                count[0] = h.label(st, d_m.ptr, n, n, n, c, d_l.ptr)
            report("label_c%d" % c, timed(lab), 5 * nvox, data=name, n=count[0])
            if host_mask is not None:
                try:
                    from scipy import ndimage
                except ImportError:
                    ndimage = None
                if ndimage is not None:
                    t0 = time.perf_counter()
                    _, n_ref = ndimage.label(host_mask, ndimage.generate_binary_structure(3, c))
                    _emit(what="scipy_label_c%d" % c, case=case, data=name, ms=round((time.perf_counter() - t0) * 1e3, 1), n=int(n_ref),
                          same_n=bool(n_ref == count[0]))
        nc = h.label(st, d_m.ptr, n, n, n, 1, d_l.ptr)
        report("measure", timed(lambda: h.measure(st, d_l.ptr, None, n, n, n, nc), 3), 4 * nvox, data=name, n=nc, passes=_seg_lib.measure_passes(nc, False))
        report("measure_vol", timed(lambda: h.measure(st, d_l.ptr, d_v.ptr, n, n, n, nc), 3), 8 * nvox, data=name, n=nc,
               passes=_seg_lib.measure_passes(nc, True))
        kept = [0]

        def small_out():
            kept[0] = h.remove_small(st, d_l.ptr, n, n, n, nc, 8, d_l2.ptr)
        report("remove_small_8", timed(small_out, 3), 8 * nvox, data=name, n=nc, kept=kept[0])
    seg.close()
    for a in (d_v, d_l, d_l2, d_m):
        a.free()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", type=int, action="append", metavar="N", help="the edge of the cubic volume (a multiple of 256, or below it)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-scipy", action="store_true", help="skip scipy.ndimage.label on the host (512^3 and below)")
    a = ap.parse_args()
    for n in (a.case or [1024, 512]):
        run(n, a.reps, not a.no_scipy)


if __name__ == "__main__":
    main()
