"""The definitions of include/tomo_vol.h / tomography_alignment_amd/postprocess.py in numpy: float32 arithmetic where the definition says
float32, integers for the region, math.fsum (correctly rounded) for the sums.  v[nx][ny][nz], z fastest."""
import math

import numpy as np

# one partly filled wave (3, 5, 7); the 4-byte load path with a z tail past a wave (2, 33, 65); an x tail past a 64-wide transpose tile
# and a z tail past two of them (70, 5, 130); the 16-byte load path and aligned 16-byte stores for both dtypes (64, 4, 256); several x
# tiles and an odd nx, so that the rows of the "zyx" output are unaligned (129, 3, 64); ny = 1 and 17 * 241 = 4097 groups of four z, one
# past the 4096 a work-group owns (17, 1, 964); the cylinder at odd and even width.
GPU_SHAPES = [(3, 5, 7), (2, 33, 65), (70, 5, 130), (64, 4, 256), (129, 3, 64), (17, 1, 964), (31, 31, 8), (32, 32, 8)]

QMAX = {np.dtype(np.uint8): 255, np.dtype(np.uint16): 65535}


def r4_of(ratio, nx, ny):
    """What the host passes for the cylinder of `ratio`: floor((ratio min(nx, ny))^2)."""
    return int(math.floor((float(ratio) * min(nx, ny)) ** 2))


def region(nx, ny, R4=-1):
    """bool [nx][ny]: (2x - nx + 1)^2 + (2y - ny + 1)^2 <= R4 in integers; everything for R4 < 0."""
    if R4 < 0:
        return np.ones((nx, ny), bool)
    a = 2 * np.arange(nx, dtype=np.int64) - nx + 1
    b = 2 * np.arange(ny, dtype=np.int64) - ny + 1
    return a[:, None] ** 2 + b[None, :] ** 2 <= np.int64(R4)


def _inside(v, R4):
    v = np.asarray(v, np.float32)
    return v[region(v.shape[0], v.shape[1], R4)].ravel()          # [rows inside][nz] flattened


def statistics(v, R4=-1):
    w = _inside(v, R4)
    fin = np.isfinite(w)
    f = w[fin].astype(np.float64)
    return {"n_finite": int(f.size), "n_nonfinite": int(w.size - f.size),
            "min": np.float32(f.min()) if f.size else np.float32(np.nan), "max": np.float32(f.max()) if f.size else np.float32(np.nan),
            "sum": math.fsum(f), "sumsq": math.fsum(f * f),               # a float32 squared is exact in float64
            "sumabs": math.fsum(np.abs(f))}


def histogram(v, lo, hi, nbins, R4=-1):
    """-> (counts uint64 [nbins], under, over, nonfinite)."""
    lo, hi = np.float32(lo), np.float32(hi)
    assert np.isfinite(lo) and np.isfinite(hi) and lo < hi and nbins >= 1
    w = _inside(v, R4)
    fin = np.isfinite(w)
    f = w[fin]
    scale = np.float32(nbins) / (hi - lo)
    assert scale.dtype == np.float32
    mid = f[(f >= lo) & (f <= hi)]
    t = (mid - lo) * scale
    assert t.dtype == np.float32
    b = np.minimum(np.floor(t).astype(np.int64), nbins - 1)
    counts = np.bincount(b, minlength=nbins).astype(np.uint64)
    return counts, int(np.count_nonzero(f < lo)), int(np.count_nonzero(f > hi)), int(w.size - f.size)


def codes(v, lo, hi, dtype):
    """clamp(rint((v - lo) * s), 0, qmax) in float32, half to even; NaN -> 0, +inf -> qmax, -inf -> 0."""
    v = np.asarray(v, np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    qmax = QMAX[np.dtype(dtype)]
    s = np.float32(qmax) / (hi - lo)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint((v - lo) * s)
    assert r.dtype == np.float32
    r = np.where(np.isnan(r), np.float32(0), r)
    return np.clip(r, 0, qmax).astype(dtype)


def quantize(v, lo, hi, dtype, order="xyz", R4=-1, fill=0):
    v = np.asarray(v, np.float32)
    c = codes(v, lo, hi, dtype)
    c[~region(v.shape[0], v.shape[1], R4)] = fill
    if order == "xyz":
        return c
    out = np.empty(v.shape[::-1], dtype)                             # out[z][y][x], element by element
    for x in range(v.shape[0]):
        out[:, :, x] = c[x].T
    return out


def circular_mask(v, R4, value=0.0):
    out = np.array(v, np.float32)
    out[~region(v.shape[0], v.shape[1], R4)] = np.float32(value)
    return out


def project(v, axis, op="max"):
    v = np.asarray(v, np.float32)
    fin = np.isfinite(v)
    if op == "max":
        r = np.where(fin, v, -np.inf).max(axis=axis)
    else:
        r = np.where(fin, v, np.inf).min(axis=axis)
    return np.where(fin.any(axis=axis), r, np.nan).astype(np.float32)


def plane(v, axis, index):
    return np.ascontiguousarray(np.take(np.asarray(v, np.float32), index, axis=axis))
