#!/usr/bin/env python3
"""Development tool (not the benchmark contract; bench.py is): the passes of libtomo_morph.so (morphology) on the GPU.

    python tools/morph_bench.py                       # 1024^3 and 512^3
    python tools/morph_bench.py --case 512
    python tools/morph_bench.py --scipy 256           # only scipy.ndimage on the host, one core

Device events (the context's) around each call on a warmed handle, the median of --reps (5) runs, set against the time the call's
compulsory bytes take at the rate of a device-to-device copy timed in the same process (a copy moves 2 x its bytes).  The compulsory
bytes per voxel: distance_sq reads the mask (1) and writes int32 (4); its passes alone (line_pass, each into a buffer of its own):
z 1 + 4, y and x 4 + 4 each; erode reads 1 and writes 1; open twice that; fill_holes reads 1 and writes 1 (its labelling inside is segment's, and its time includes the wait for the
component table).  The masks: the Shepp-Logan phantom (256^3, every voxel repeated) at Otsu's threshold, a Bernoulli mask of density
0.6, and the worst case of the line routine, one background voxel in a full volume, where every lane walks to the end of its line.
r2 = 9 for erode and open.  One JSON line per measurement on stdout."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

R2 = 9


def _emit(**kw):
    print(json.dumps(kw), flush=True)


def _fill(d, n, slab_of, dtype):
    """Upload slab_of(x0, x1) -> [x1 - x0][n][n] in slabs of 32 planes."""
    for x0 in range(0, n, 32):
        x1 = min(n, x0 + 32)
        d.view(x0 * n * n, (x1 - x0) * n * n).upload(np.ascontiguousarray(slab_of(x0, x1), dtype))


def _phantom_mask(n):
    from tomography_alignment_amd import segment, postprocess
    from tomography_alignment_amd.utilities import generate_phantom
    base = min(n, 256)
    rep = n // base
    small = np.asarray(generate_phantom.shepp3d(base), np.float32)
    counts, edges = np.histogram(small, 4096)
    t, = segment.otsu_threshold(postprocess.Histogram(counts.astype(np.uint64), 0, 0, 0, float(edges[0]), float(edges[-1])))
    m = (small >= t).astype(np.uint8)
    return lambda x0, x1: np.repeat(np.repeat(m[np.arange(x0, x1) // rep], rep, axis=1), rep, axis=2)


def _masks(n):
    rng = np.random.default_rng(0)

    def worst(x0, x1):
        s = np.ones((x1 - x0, n, n), np.uint8)
        if x0 <= n // 2 < x1:
            s[n // 2 - x0, n // 2, n // 2] = 0
        return s
    return [("shepp-logan >= otsu", _phantom_mask(n)), ("bernoulli 0.6", lambda x0, x1: rng.random((x1 - x0, n, n), np.float32) < 0.6),
            ("one background voxel", worst)]


def run(n, reps):
    from tomography_alignment_amd import _lib, morphology

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

    d_a = ctx.empty((n, n, n), np.int32)
    d_b = ctx.empty((n, n, n), np.int32)
    d_c = ctx.empty((n, n, n), np.int32)
    d_m = ctx.empty((n, n, n), np.uint8)
    d_o = ctx.empty((n, n, n), np.uint8)
    copy_ms = timed(lambda: d_b.copy_from(d_a), 7)
    copy_gbs = 2.0 * d_a.nbytes / (copy_ms * 1e-3) / 1e9
    _emit(what="d2d_copy", case=case, ms=round(copy_ms, 3), GBps=round(copy_gbs, 1), device=ctx.device_name())

    mo = morphology.Morphology(ctx)
    mo._ready(d_m)
    h, st = mo.handle, ctx.stream()

    def report(what, ms, nbytes, **kw):
        at_copy = nbytes / (copy_gbs * 1e9) * 1e3
        _emit(what=what, case=case, ms=round(ms, 3), bytes_at_copy_rate_ms=round(at_copy, 3), ratio=round(ms / at_copy, 2), **kw)

    for name, slab in _masks(n):
        _fill(d_m, n, slab, np.uint8)
        for border in (0, 1):
            report("distance_sq border %d" % border, timed(lambda: h.distance_sq(st, d_m.ptr, n, n, n, border, d_a.ptr)), 5 * nvox, data=name)
        report("pass z", timed(lambda: h.line_pass(st, d_m.ptr, n, n, n, 2, 0, d_a.ptr)), 5 * nvox, data=name)
        report("pass y", timed(lambda: h.line_pass(st, d_a.ptr, n, n, n, 1, 0, d_b.ptr)), 8 * nvox, data=name)
        report("pass x", timed(lambda: h.line_pass(st, d_b.ptr, n, n, n, 0, 0, d_c.ptr)), 8 * nvox, data=name)
        report("distance", timed(lambda: h.distance(st, d_m.ptr, n, n, n, 1, d_a.ptr)), 5 * nvox, data=name)
        for bv in (0, 1):
            report("erode r2 %d border_value %d" % (R2, bv), timed(lambda: h.erode(st, d_m.ptr, n, n, n, R2, bv, d_o.ptr)), 2 * nvox, data=name)
        report("dilate r2 %d" % R2, timed(lambda: h.dilate(st, d_m.ptr, n, n, n, R2, d_o.ptr)), 2 * nvox, data=name)
        report("open r2 %d" % R2, timed(lambda: h.open(st, d_m.ptr, n, n, n, R2, 0, d_o.ptr)), 4 * nvox, data=name)
        filled = [0]

        def fill():
            filled[0] = mo.fill_holes(d_m, out=d_o, return_count=True)[1]
        report("fill_holes", timed(fill, 3), 2 * nvox, data=name, filled=filled[0])
    mo.close()
    for a in (d_a, d_b, d_c, d_m, d_o):
        a.free()
    ctx.close()


def host(n):
    """scipy.ndimage on one host core on the same three masks."""
    from scipy import ndimage
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import morph_model as mm
    ball = mm.ball(R2)
    for name, slab in _masks(n):
        m = np.ascontiguousarray(slab(0, n), np.uint8)
        for what, fn in (("scipy distance_transform_edt", lambda: ndimage.distance_transform_edt(m)),
                         ("scipy binary_erosion r2 %d" % R2, lambda: ndimage.binary_erosion(m, ball)),
                         ("scipy binary_opening r2 %d" % R2, lambda: ndimage.binary_opening(m, ball)),
                         ("scipy binary_fill_holes", lambda: ndimage.binary_fill_holes(m))):
            t0 = time.perf_counter()
            fn()
            _emit(what=what, case="%d^3" % n, data=name, ms=round((time.perf_counter() - t0) * 1e3, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", type=int, action="append", metavar="N", help="the edge of the cubic volume (a multiple of 256, or below it)")
    ap.add_argument("--scipy", type=int, action="append", metavar="N", help="time scipy.ndimage on the host at this edge instead (256, 512)")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if a.scipy:
        for n in a.scipy:
            host(n)
        return
    for n in (a.case or [1024, 512]):
        run(n, a.reps)


if __name__ == "__main__":
    main()
