#!/usr/bin/env python3
"""Development tool (not the benchmark contract; bench.py is): the dynamic flat-field correction of libtomo_dff.so on the GPU.

    python tools/dff_bench.py                       # 1024 frames of 1024 x 1024 and 720 of 512 x 512; K = 20 flats, m = 3, bin 2
    python tools/dff_bench.py --case 720 512 512

uint16 frames of a smooth object under a beam whose centre jitters by +-cols / 8 px (16 distinct frames, repeated), 20 flats under the
same beam.  Device events (the context's) on a warmed handle, the median of --reps (5) runs, each leg set against the time its bytes take at
the rate of a device-to-device copy timed in the same process (a copy moves 2 x its bytes):
    gram       the flats and fbar read once                                      (the K x K result comes back to the host inside the timing)
    eff        the flats and fbar read, m fields written
    bin        every frame read, its binned counts written
    cost       one evaluation of all projections: the binned counts read once (the binned flat and fields stay in L2); the weights go up
               and f, g come back inside the timing
    apply      every frame read, fbar, dark and m fields read, the sinogram written -- beside preprocess.normalize at the same size
and the wall time of the whole estimation (binning, every L-BFGS-B step on the host, every launch) with its evaluation count, the
number of launches and the time the helper thread spent inside them; beside it the wall time of the same driver
(_lbfgsb_batch.minimize_many, as many problems and weights, the same bounds and ftol) on a quartic evaluated in numpy, i.e. what the host
side alone costs per evaluation on the machine that ran the tool.
One JSON line per measurement on stdout."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

K, M, BIN, DISTINCT = 20, 3, 2, 16


def _emit(**kw):
    print(json.dumps(kw), flush=True)


def frames_under_a_drifting_beam(n, rows, cols, rng):
    z, x = np.arange(rows, dtype=np.float64)[None, :, None], np.arange(cols, dtype=np.float64)[None, None, :]

    def beam(k):
        cx, cz = (cols - 1) / 2.0 + rng.uniform(-cols / 8.0, cols / 8.0, k), (rows - 1) / 2.0 + rng.uniform(-cols / 8.0, cols / 8.0, k)
        return 0.6 + 0.4 * np.exp(-((x - cx[:, None, None]) ** 2 + (z - cz[:, None, None]) ** 2) / (2.0 * (0.6 * cols) ** 2))

    gain = 1.0 + 0.02 * rng.standard_normal((rows, cols))
    r2 = ((x - cols / 2.0) / (0.3 * cols)) ** 2 + ((z - rows / 2.0) / (0.35 * rows)) ** 2
    att = np.exp(-1.5 * np.sqrt(np.clip(1.0 - r2, 0.0, None)))
    flats = np.clip(rng.poisson(2e4 * gain * beam(K)) + 100, 0, 65535).astype(np.uint16)
    frames = np.clip(rng.poisson(2e4 * gain * att * beam(n)) + 100, 0, 65535).astype(np.uint16)
    darks = np.clip(rng.poisson(np.full((5, rows, cols), 100.0)), 0, 65535).astype(np.uint16)
    return frames, flats, darks


def run(n, rows, cols, reps):
    from tomography_alignment_amd import _dff_lib, _lib, preprocess

    ctx = _lib.Context()
    case = "%d x %d x %d" % (n, rows, cols)
    P = rows * cols
    zb, xb = rows // BIN, cols // BIN

    def timed(fn):
        fn()                                                     # warm-up
        ctx.sync()
        out = []
        for _ in range(reps):
            ctx.timer_start()
            fn()
            out.append(ctx.timer_stop())
        return float(np.median(out))

    frames, flats, darks = frames_under_a_drifting_beam(DISTINCT, rows, cols, np.random.default_rng(0))
    d_raw = ctx.empty((n, rows, cols), np.uint16)
    for i in range(n):
        d_raw.view(i * P, P).upload(frames[i % DISTINCT])
    d_out = ctx.empty((n, cols, rows), np.float32)
    d_tmp = ctx.empty((n, cols, rows), np.float32)
    copy_ms = timed(lambda: d_tmp.copy_from(d_out))
    copy_gbs = 2.0 * d_out.nbytes / (copy_ms * 1e-3) / 1e9
    d_tmp.free()
    _emit(what="d2d_copy", case=case, ms=round(copy_ms, 3), GBps=round(copy_gbs, 1), device=ctx.device_name())

    def leg(what, ms, nbytes, **kw):
        at_copy = nbytes / (copy_gbs * 1e9) * 1e3
        _emit(what=what, case=case, ms=round(ms, 3), bytes_at_copy_rate_ms=round(at_copy, 4), ratio=round(ms / at_copy, 2), **kw)

    pre = preprocess.Preprocessor(ctx)
    d_flats, d_darks = ctx.to_device(flats, np.uint16), ctx.to_device(darks, np.uint16)
    ef = pre.eigen_flats(d_flats, d_darks, n_eff=M)
    h, st = pre._dff, ctx.stream()
    lam, V = preprocess.eigen_decomposition(h.gram(st, d_flats.ptr, _dff_lib.U16, K, rows, cols, ef.flat.ptr))
    _emit(what="eigenvalues_over_median", case=case, values=np.round(lam[:6] / np.median(lam), 2).tolist(), auto_m=preprocess.count_eigen_flats(lam))
    leg("gram", timed(lambda: h.gram(st, d_flats.ptr, _dff_lib.U16, K, rows, cols, ef.flat.ptr)), 2.0 * K * P + 4.0 * P, K=K)
    leg("eff", timed(lambda: h.eff(st, d_flats.ptr, _dff_lib.U16, K, rows, cols, ef.flat.ptr, V[:, :M], ef.eff.ptr)), 2.0 * K * P + 4.0 * P + 4.0 * M * P, m=M)
    h.set_max_scratch(0)
    leg("bin", timed(lambda: h.load_projections(st, d_raw.ptr, _dff_lib.U16, 0, n, rows, cols, BIN, ef.dark.ptr)), 2.0 * n * P + 4.0 * P + 4.0 * n * zb * xb,
        bin=BIN)
    Fb, Eb = ctx.empty((zb, xb), np.float32), ctx.empty((M, zb, xb), np.float32)
    h.bin(st, ef.flat.ptr, _dff_lib.F32, 1, rows, cols, BIN, ef.dark.ptr, Fb.ptr)
    h.bin(st, ef.eff.ptr, _dff_lib.F32, M, rows, cols, BIN, None, Eb.ptr)
    a = np.array([Fb.download().astype(np.float64).mean()] + [e.astype(np.float64).mean() for e in Eb.download()])
    ids, W = np.arange(n), np.zeros((n, M))
    leg("cost", timed(lambda: h.cost(st, ids, W, np.full(n, a[0]), a, 1e-3, Fb.ptr, Eb.ptr)), 4.0 * n * zb * xb + 4.0 * (1 + M) * zb * xb, projections=n)
    Fb.free()
    Eb.free()

    inside = {"s": 0.0, "launches": 0, "listed": 0}
    cost = h.cost

    def counted(stream, ids, *args):
        t0 = time.perf_counter()
        try:
            return cost(stream, ids, *args)
        finally:
            inside["s"] += time.perf_counter() - t0
            inside["launches"] += 1
            inside["listed"] += len(ids)

    h.cost = counted
    runs = []
    for _ in range(3):
        ctx.sync()
        inside.update(s=0.0, launches=0, listed=0)
        t0 = time.perf_counter()
        Wt, nfev = pre._estimate_weights(d_raw, np.dtype(np.uint16), n, rows, cols, ef, M, BIN, 1e-3, 10.0, 0)
        runs.append((time.perf_counter() - t0, dict(inside)))
    del h.cost
    wall, part = min(runs, key=lambda r: r[0])
    assert part["listed"] == nfev                                        # every evaluation the optimisers count went through a launch
    _emit(what="estimation", case=case, wall_ms=round(wall * 1e3, 1), all_runs_ms=[round(r[0] * 1e3, 1) for r in runs], evaluations=int(nfev),
          per_projection=round(nfev / float(n), 1), launches=part["launches"], inside_launches_ms=round(part["s"] * 1e3, 1),
          us_per_evaluation=round(wall * 1e6 / nfev, 2), largest_weight=round(float(np.abs(Wt).max()), 2), handle_MB=round(h.device_bytes() / 1e6, 1))

    from concurrent.futures import ThreadPoolExecutor
    from tomography_alignment_amd import _lbfgsb_batch
    target = np.random.default_rng(1).uniform(-1, 1, (n, M))

    def quartic(ids, X):
        d = X - target[ids]
        return (d * d).sum(axis=1) + (d ** 4).sum(axis=1), 2 * d + 4 * d ** 3

    host = []
    for _ in range(3):
        with ThreadPoolExecutor(max_workers=1) as pool:
            t0 = time.perf_counter()
            _, _, nf, _ = _lbfgsb_batch.minimize_many(quartic, np.zeros((n, M)), bounds=[(-10.0, 10.0)] * M, options=preprocess.TV_OPTIONS, overlap=pool.submit)
            host.append(time.perf_counter() - t0)
    _emit(what="driver_alone_numpy_quartic", case=case, wall_ms=round(min(host) * 1e3, 1), evaluations=int(nf.sum()),
          us_per_evaluation=round(min(host) * 1e6 / int(nf.sum()), 2))

    crop = ((0, rows), (0, cols))
    w32 = Wt.astype(np.float32)
    ms_apply = timed(lambda: h.apply(st, d_raw.ptr, _dff_lib.U16, n, rows, cols, ef.flat.ptr, ef.dark.ptr, ef.eff.ptr, w32, crop, None, True, 1e-6, d_out.ptr))
    leg("apply", ms_apply, 2.0 * n * P + 4.0 * n * P + 4.0 * (2 + M) * P, m=M)
    pre._ready(d_raw)
    ms_norm = timed(lambda: pre.handle.normalize(st, d_raw.ptr, preprocess._DTYPES[np.dtype(np.uint16)], n, rows, cols, ef.flat.ptr, ef.dark.ptr, crop, None,
                                                 True, 1e-6, d_out.ptr))
    leg("normalize", ms_norm, 2.0 * n * P + 4.0 * n * P + 8.0 * P, apply_over_normalize=round(ms_apply / ms_norm, 2))
    ef.free()
    for d in (d_raw, d_out, d_flats, d_darks):
        d.free()
    pre.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", type=int, nargs=3, action="append", metavar=("N", "ROWS", "COLS"), help="projections, detector rows, detector columns")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for n, rows, cols in (a.case or [(1024, 1024, 1024), (720, 512, 512)]):
        run(n, rows, cols, a.reps)


if __name__ == "__main__":
    main()
