#!/usr/bin/env python3
"""Development tool (not the benchmark contract; bench.py is): the Paganin phase retrieval of libtomo_phase.so on the GPU.

    python tools/phase_bench.py                              # 1024 x 1024^2 and 1800 x 2048^2, a = 400 and a = 1558
    python tools/phase_bench.py --sizes 256x512 --strengths 25

Device events (the library's own, around each pass, summed over the batches) on a warmed handle, the median of --reps (7) runs: the pad
kernel, the batched R2C, the filter kernel, the batched C2R and the crop kernel, then their total and the device time of an untimed
call.  Each hand-written kernel's bytes (pad: the frames read, the padded buffer written; filter: the half-spectrum read and written;
crop: the window read, the frames written) are set against a device-to-device copy timed in the same process (a copy moves 2 x its
bytes).  Also the time to make the hipFFT plans (the first call) and the device bytes the handle keeps.  One JSON line per measurement."""
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


def run(n, size, strengths, reps, budget):
    from tomography_alignment_amd import _lib, _phase_lib, preprocess

    ctx = _lib.Context()

    def timed(fn):
        fn()                                                     # warm-up
        ctx.sync()
        out = []
        for _ in range(reps):
            ctx.timer_start()
            fn()
            out.append(ctx.timer_stop())
        return float(np.median(out)), float(np.min(out))

    shape = (n, size, size)
    src = ctx.zeros(shape, np.float32)                           # the passes' work does not depend on the values
    dst = ctx.empty(shape, np.float32)
    copy_ms, _ = timed(lambda: dst.copy_from(src))
    copy_gbs = 2.0 * src.nbytes / (copy_ms * 1e-3) / 1e9
    _emit(what="d2d_copy", frames=n, size=size, ms=round(copy_ms, 3), GBps=round(copy_gbs, 1), device=ctx.device_name())
    pre = preprocess.Preprocessor(ctx)
    for a in strengths:
        (mx, px), (mz, pz) = preprocess.phase_padding(size, a), preprocess.phase_padding(size, a)
        t0 = time.perf_counter()
        pre.retrieve_phase(src, a, out=dst, max_scratch_bytes=budget)                  # makes the plans
        _emit(what="first_call", frames=n, size=size, strength=a, pad=mx, padded=[px, pz], wall_s=round(time.perf_counter() - t0, 3),
              plan_s=round(pre._phase.plan_seconds(), 3), handle_GB=round(pre._phase.device_bytes() / 1e9, 3),
              batch=_phase_lib.batch(n, px, pz, preprocess.DEFAULT_SCRATCH_BYTES if budget is None else budget))
        runs = []
        for _ in range(reps):
            runs.append(pre.retrieve_phase(src, a, out=dst, max_scratch_bytes=budget, timed=True)[1])
        ms = np.median(np.asarray(runs, np.float64), axis=0)
        frames_b = 4.0 * n * size * size
        padded_b = 4.0 * n * px * (pz + 2)
        moved = dict(pad=frames_b + padded_b, filter=2.0 * padded_b, crop=2.0 * frames_b)
        row = dict(what="passes", frames=n, size=size, strength=a, padded=[px, pz], total_ms=round(float(ms.sum()), 3))
        for name, t in zip(_phase_lib.PASSES, ms):
            row[name + "_ms"] = round(float(t), 3)
        for name, nbytes in moved.items():
            t = float(ms[_phase_lib.PASSES.index(name)])
            at_copy = nbytes / (copy_gbs * 1e9) * 1e3
            row[name + "_GBps"] = round(nbytes / (t * 1e-3) / 1e9, 1)
            row[name + "_bytes_at_copy_rate_ms"] = round(at_copy, 3)
            row[name + "_over_copy"] = round(t / at_copy, 2)
        _emit(**row)
        whole, whole_min = timed(lambda: pre.retrieve_phase(src, a, out=dst, max_scratch_bytes=budget))
        _emit(what="whole_call", frames=n, size=size, strength=a, ms=round(whole, 3), min_ms=round(whole_min, 3),
              ms_per_frame=round(whole / n, 4))
    log_ms, _ = timed(lambda: pre.minus_log(src, out=dst))
    _emit(what="minus_log", frames=n, size=size, ms=round(log_ms, 3), over_copy=round(log_ms / copy_ms, 2))
    pre.close()
    src.free()
    dst.free()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["1024x1024", "1800x2048"], help="FRAMESxEDGE: stacks of FRAMES frames of EDGE^2")
    ap.add_argument("--strengths", type=float, nargs="+", default=[400.0, 1558.0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--max-scratch-bytes", type=int, default=None, help="default: preprocess.DEFAULT_SCRATCH_BYTES (2 GiB)")
    a = ap.parse_args()
    if a.reps < 7:
        ap.error("--reps must be at least 7")
    for s in a.sizes:
        n, size = (int(v) for v in s.lower().split("x"))
        run(n, size, a.strengths, a.reps, a.max_scratch_bytes)


if __name__ == "__main__":
    main()
