#!/usr/bin/env python3
"""Development tool (not the benchmark contract; bench.py is): the passes of libtomo_vreg.so (registration) on the GPU.

    python tools/vreg_bench.py                       # 512^3 and 1024^3
    python tools/vreg_bench.py --case 512

Device events (the context's, around the enqueue-only calls) on a warmed handle, the median of --reps (7) runs, with the
device-to-device copy timed in the same process.  The reference is a Shepp-Logan phantom (256^3, every voxel repeated along the three
axes), the moving volume its Fourier shift by (2.3, -1.7, 0.4) made on the device.  Per case: prepare (both volumes), correlate (two
R2C, the cross-power pass, one C2R, the coarse argmax; timed as prepare + correlate minus prepare, because correlate consumes what
prepare wrote), refine at upsample 10 and 100 with its share of the whole register call, the Fourier shift and the integer roll.
refine's float64 rate is the flops of its three contractions over its time; the rate given for k_up_z alone, 8 nx ny (nz/2 + 1) U
flops over the time of ALL of refine, is a lower bound of what that kernel reaches.  One JSON line per measurement on stdout."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

FP64_VECTOR_PEAK_TFLOPS = 78.6


def _emit(**kw):
    print(json.dumps(kw), flush=True)


def run(n, reps):
    from tomography_alignment_amd import _lib, _vreg_lib, registration
    from tomography_alignment_amd.utilities import generate_phantom

    ctx = _lib.Context()
    case = "%d^3" % n

    def timed(fn):
        fn()                                                     # warm-up
        ctx.sync()
        out = []
        for _ in range(reps):
            ctx.timer_start()
            fn()
            out.append(ctx.timer_stop())
        return float(np.median(out))

    d_ref = ctx.empty((n, n, n), np.float32)
    d_mov = ctx.empty((n, n, n), np.float32)
    base = min(n, 256)
    rep = n // base
    small = np.asarray(generate_phantom.shepp3d(base), np.float32)
    for x0 in range(0, n, 32):
        x1 = min(n, x0 + 32)
        d_ref.view(x0 * n * n, (x1 - x0) * n * n).upload(np.repeat(np.repeat(small[np.arange(x0, x1) // rep], rep, axis=1), rep, axis=2))
    copy_ms = timed(lambda: d_mov.copy_from(d_ref))
    _emit(what="d2d_copy", case=case, ms=round(copy_ms, 3), GBps=round(2.0 * d_ref.nbytes / (copy_ms * 1e-3) / 1e9, 1), device=ctx.device_name())

    rg = registration.Registrar(ctx)
    planted = (2.3, -1.7, 0.4)
    rg.shift_volume(d_ref, [-s for s in planted], out=d_mov)
    h, st = rg.handle, ctx.stream()
    radius, edge = n / 2.0 - 6.0, 6.0

    def prepare():
        h.prepare(st, 0, d_ref.ptr, _vreg_lib.MASK_SPHERE, None, radius, edge, True)
        h.prepare(st, 1, d_mov.ptr, _vreg_lib.MASK_SPHERE, None, radius, edge, True)

    def prepare_correlate():
        prepare()
        h.correlate(st)

    t_prep = timed(prepare)
    t_corr = timed(prepare_correlate) - t_prep
    _emit(what="prepare_both", case=case, ms=round(t_prep, 3), copies=round(t_prep / copy_ms, 2))
    _emit(what="correlate", case=case, ms=round(t_corr, 3), copies=round(t_corr / copy_ms, 2), plan_seconds=round(h.plan_seconds(), 2))
    nzh = n // 2 + 1
    for u in (10, 100):
        U = (3 * u + 1) // 2
        t_ref = timed(lambda: h.refine(st, u))
        out = h.fetch(st)
        fz, fy, fx = 8.0 * n * n * nzh * U, 8.0 * n * n * U * U, 4.0 * n * U ** 3
        whole = t_prep + t_corr + t_ref
        _emit(what="refine", case=case, upsample=u, U=U, ms=round(t_ref, 3), share_of_register=round(t_ref / whole, 3),
              register_ms=round(whole, 3), shift=[round(float(v), 4) for v in out[:3]], planted=planted,
              contraction_gflop=round((fz + fy + fx) / 1e9, 1), refine_fp64_tflops=round((fz + fy + fx) / t_ref / 1e9, 2),
              k_up_z_fp64_tflops_at_least=round(fz / t_ref / 1e9, 2), fraction_of_vector_peak_at_least=round(fz / t_ref / 1e9 / FP64_VECTOR_PEAK_TFLOPS, 3),
              device_bytes=h.device_bytes())
    d_out = ctx.empty((n, n, n), np.float32)
    t_shift = timed(lambda: h.shift(st, d_mov.ptr, planted, d_out.ptr))
    t_roll = timed(lambda: h.shift(st, d_mov.ptr, (2, -1, 3), d_out.ptr))
    _emit(what="shift_fractional", case=case, ms=round(t_shift, 3), copies=round(t_shift / copy_ms, 2))
    _emit(what="shift_integer", case=case, ms=round(t_roll, 3), copies=round(t_roll / copy_ms, 2))
    d_out.free()
    rg.close()
    d_ref.free()
    d_mov.free()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", type=int, action="append", metavar="N", help="the edge of the cubic volume (a multiple of 256, or below it)")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    for n in (a.case or [512, 1024]):
        run(n, a.reps)


if __name__ == "__main__":
    main()
