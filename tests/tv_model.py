"""A stepwise numpy model of the 3-D TV proximal step (utilities/tv_denoise.py:98-170 denoise_fista) in ONE working precision, and the
case table the CPU and GPU tests of that step share.

oracle.tv_denoise_fista is the reference's text: on float32 input its `(1 + t_factor)` is a numpy float64 scalar, which (numpy >= 2)
promotes the whole dual field to float64 from the first iteration on -- so it says nothing about what float32 arithmetic costs.  Here
every array, and every scalar that meets an array, is cast to `dtype`, and every product is rounded on its own: with dtype=float32 this
is operation for operation what csrc/tomo_reg.hip's k_tv_error / k_tv_update / k_tv_new / k_tv_norm<1> state (same order of the adds
in div, same three-term norm (a0 a0 + a1 a1) + a2 a2, t / t_new / t_factor as host doubles, the dual gap from float64 sums of the
float32 values); with dtype=float64 it is the oracle."""
import functools

import numpy as np

from oracle.oracle import tv_div, tv_gradient


def _iso(x):
    """sqrt((gx gx + gy gy) + gz gz) of the forward differences of x, in x's dtype."""
    g = tv_gradient(x)
    return np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])


def _sum64(a):
    return float(np.sum(a.astype(np.float64)))


def _sumsq64(a):
    a = a.astype(np.float64)
    return float(np.sum(a * a))


def denoise_fista(im, weight, niter, eps, check_gap_frequency, dtype):
    """-> (new, iters, gap, gaps_at_every_check, largest_pre_projection_norm, TV_of_new).  `new` is the iterate of the last dual-gap
    check (im itself if none ran), TV_of_new = sum sqrt(|grad new|^2) in float64, largest_pre_projection_norm the largest
    sqrt(a0^2 + a1^2 + a2^2) any iteration met before projecting on the unit ball."""
    im = np.asarray(im).astype(dtype)
    assert im.ndim == 3 and min(im.shape) >= 2
    w, c = dtype(weight), dtype(1.0 / (12.0 * weight))
    aux = np.zeros((3,) + im.shape, dtype)
    p_old = np.zeros((3,) + im.shape, dtype)
    new = im.copy()
    im_norm = _sumsq64(im)
    t, i, dgap, gaps, worst = 1.0, 0, 0.0, [], 0.0
    while i < niter:
        err = w * tv_div(aux) - im
        a = aux + tv_gradient(err) * c
        nrm = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
        worst = max(worst, float(nrm.max()))
        p = a / np.maximum(nrm, dtype(1))
        t_new = 0.5 * (1.0 + np.sqrt(1.0 + 4.0 * t * t))
        t_factor = float((t - 1.0) / t_new)
        aux = dtype(1.0 + t_factor) * p - dtype(t_factor) * p_old
        p_old = p
        t = float(t_new)
        if i % check_gap_frequency == 0:
            gap = w * tv_div(p)
            new = im - gap
            tv_new = 2.0 * weight * _sum64(_iso(new))
            dgap = 0.5 / im_norm * (_sumsq64(gap) + tv_new - im_norm + _sumsq64(new)) if im_norm > 0.0 else 0.0
            gaps.append(dgap)
            if dgap < eps:
                break
        i += 1
    assert new.dtype == dtype and aux.dtype == dtype
    return new, i, float(dgap), gaps, worst, _sum64(_iso(new))


# ---- the case table
def block(shape):
    nx, ny, nz = shape
    v = np.zeros(shape)
    v[nx // 4:max(nx // 4 + 1, 3 * nx // 4), :, nz // 5:4 * nz // 5] = 1.0
    return (v + 0.2 * np.random.default_rng(nx + ny + nz).standard_normal(shape)).astype(np.float32)


def flat(shape):
    return np.random.default_rng(1).uniform(0.0, 1.0, shape).astype(np.float32)


BIG = (2, 2, 131080)       # 524 320 voxels: 513 z chunks per row, 32 voxels past one sweep of the fixed 2048 x 256 grid
SHAPES = [(2, 2, 2), (2, 3, 257), (3, 2, 256), (5, 4, 255), (7, 2, 513), (16, 12, 20), BIG]
SETTINGS = {      # tag: (input, exact regime, parameters)
    "A": (block, False, dict(weight=0.3, niter=12, eps=0.0, check_gap_frequency=1)),
    "B": (block, False, dict(weight=0.1, niter=60, eps=2e-3, check_gap_frequency=3)),
    "C": (block, False, dict(weight=0.1, niter=60, eps=1e-4, check_gap_frequency=3)),
    "E": (flat, True, dict(weight=2.0, niter=6, eps=0.0, check_gap_frequency=1)),
}
CASES = [(tag, shape) for shape in SHAPES for tag in (("B", "E") if shape == BIG else ("A", "B", "C", "E"))]
CASE_IDS = ["%s-%dx%dx%d" % ((tag,) + shape) for tag, shape in CASES]
INEXACT = [c for c in CASES if not SETTINGS[c[0]][1]]
EXACT = [c for c in CASES if SETTINGS[c[0]][1]]


def case_id(case):
    return CASE_IDS[CASES.index(case)]


def params(case):
    return SETTINGS[case[0]][2]


@functools.lru_cache(maxsize=None)
def case_input(case):
    im = SETTINGS[case[0]][0](case[1])
    im.setflags(write=False)
    return im


@functools.lru_cache(maxsize=None)
def case_model(case, dtype):
    """The model's result on a case of the table, computed once per process and shared (read-only)."""
    r = denoise_fista(case_input(case), dtype=dtype, **params(case))
    r[0].setflags(write=False)
    return r
