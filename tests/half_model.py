"""
The numpy / float64 definition of tomography_alignment_amd.half_acquisition (include/tomo_half.h states the same): the rotation axis of
a half-acquisition (offset-axis) scan over 2 pi by the fixed-window overlap search of Vo et al., and the stitch of the 2 pi series to
the pi series of double width.  It is the specification the library is tested against; no equality with other packages is claimed.

S[n][nx] is one detector row of p[n][nx][nz] (float32, z fastest), n even, row i taken at phi0 + i 2 pi / n.  h = n / 2,
A[i][x] = S[i][x], M[i][x] = S[h + i][nx - 1 - x] for i < h.  With the axis at column c (centre convention (nx - 1) / 2),
A[i][x] = M[i][x + t], t = nx - 1 - 2 c.
"""
import numpy as np

SIDES = ("right", "left")          # the order of the curves of one row


def angle_span(angles, n):
    """How many rows of a series of n cover [0, 2 pi): n for None or n d = 2 pi, n - 1 for (n - 1) d = 2 pi (the endpoint repeats the
    first row and is dropped).  ValueError for anything else, and for an odd count after the drop."""
    n = int(n)
    if angles is None:
        used = n
    else:
        a = np.asarray(angles, np.float64).ravel()
        if a.size != n:
            raise ValueError("half acquisition: %d angles for %d projections" % (a.size, n))
        if n < 2:
            raise ValueError("half acquisition: needs at least two angles")
        d = (a[-1] - a[0]) / (n - 1)
        if not (np.isfinite(d) and d != 0.0) or np.max(np.abs(np.diff(a) - d)) > 1e-6 * abs(d):
            raise ValueError("half acquisition: the angles must be uniformly spaced")
        tol = 1e-6 * abs(d)
        if abs(n * abs(d) - 2 * np.pi) <= tol:
            used = n
        elif abs((n - 1) * abs(d) - 2 * np.pi) <= tol:
            used = n - 1
        else:
            raise ValueError("half acquisition: the angles must span 2 pi (n d = 2 pi, or (n - 1) d = 2 pi with the endpoint), got a "
                             "spacing of %g rad over %d angles" % (d, n))
    if used < 2 or used % 2:
        raise ValueError("half acquisition: needs an even number of projections over 2 pi, got %d" % used)
    return used


# ------------------------------------------------------------------------------------------------------------------------ search

def metric_from_sums(N, sa, saa, sb, sbb, sab):
    """m = 1 - r from the five sums of two blocks of N values each (arrays broadcast); 1 where either variance is 0."""
    N = np.float64(N)
    va, vb = N * saa - sa * sa, N * sbb - sb * sb
    ok = (va > 0) & (vb > 0)
    den = np.sqrt(np.where(ok, va, 1.0) * np.where(ok, vb, 1.0))
    return np.where(ok, 1.0 - (N * sab - sa * sb) / den, 1.0)


def curve(S, w, side):
    """m(p), p = 0 ... nx - w, of one sinogram S (n, nx) for one side: float64 (nx - w + 1,)."""
    S = np.asarray(S, np.float32).astype(np.float64)           # float32 values, multiplied and added in float64
    n, nx = S.shape
    h = n // 2
    A, M = S[:h], S[h:2 * h, ::-1]
    ref = A[:, nx - w:] if side == "right" else A[:, :w]
    sa, saa = ref.sum(), (ref * ref).sum()
    m = np.empty(nx - w + 1)
    for p in range(nx - w + 1):
        b = M[:, p:p + w]
        m[p] = metric_from_sums(h * w, sa, saa, b.sum(), (b * b).sum(), (ref * b).sum())
    return m


def refine(m):
    """(k, delta): the first index of the minimum of m and the parabola's step, clipped to +-1/2; 0 at an end or without curvature."""
    k = int(np.argmin(m))
    delta = 0.0
    if 0 < k < m.size - 1:
        den = m[k - 1] - 2.0 * m[k] + m[k + 1]
        if den > 0:
            delta = float(np.clip(0.5 * (m[k - 1] - m[k + 1]) / den, -0.5, 0.5))
    return k, delta


def center_from_curves(m_right, m_left, nx, w, side=None):
    """(c, side, k, minimum) of one row from its two curves (the one of a side that is not asked for may be None)."""
    best = None
    for s, m in (("right", m_right), ("left", m_left)):
        if side not in (None, s):
            continue
        k, delta = refine(m)
        if best is None or m[k] < best[3]:                      # right first: it wins a tie
            p = k + delta
            t = p - (nx - w) if s == "right" else p
            best = (0.5 * (nx - 1 - t), s, k, float(m[k]))
    return best


def find_center_row(S, w, side=None):
    nx = np.shape(S)[1]
    return center_from_curves(curve(S, w, "right") if side in (None, "right") else None,
                              curve(S, w, "left") if side in (None, "left") else None, nx, w, side)


def find_center_360(p, angles=None, rows=None, win_width=None, side=None):
    """(center, centers, sides, ks, curves) of p (n, nx, nz): the median of c over the detector rows `rows` (default the middle one)."""
    p = np.asarray(p)
    n = angle_span(angles, p.shape[0])
    nx, nz = p.shape[1:]
    w = max(8, nx // 8) if win_width is None else win_width
    rows = np.array([nz // 2] if rows is None else rows, np.int64).ravel()
    res, curves = [], []
    for z in rows:
        S = p[:n, :, z]
        mr, ml = curve(S, w, "right"), curve(S, w, "left")
        curves.append((mr, ml))
        res.append(center_from_curves(mr, ml, nx, w, side))
    centers = np.array([r[0] for r in res])
    return float(np.median(centers)), centers, [r[1] for r in res], [r[2] for r in res], curves


# ------------------------------------------------------------------------------------------------------------------------ stitch

def stitched_shape(n, nx, center):
    """(h, W, j0): rows and columns of the stitched series and the output column of input column 0 of the first half."""
    c = float(center)
    if not 0.0 <= c <= nx - 1:
        raise ValueError("half acquisition: the axis must lie on the detector, 0 <= center <= %d, got %r" % (nx - 1, center))
    W = int(np.floor(2.0 * max(c, nx - 1 - c))) + 1
    return int(n) // 2, W, (0 if c >= nx - 1 - c else W - nx)


def column_table(nx, center):
    """The per-column table of the stitch: dict of a_valid, b_valid (bool), ja (column of the first half), i0, i1 (columns of the second
    half's row; i1 = i0 where the neighbour is not needed), f, wA (float64), W, j0, c_out, side."""
    c = float(center)
    _, W, j0 = stitched_shape(2, nx, c)
    right = c >= nx - 1 - c
    g = nx - 1 - c if right else c
    c_out = c + j0
    j = np.arange(W)
    ja = j - j0
    a_valid = (ja >= 0) & (ja <= nx - 1)
    xb = 2.0 * c - ja
    b_valid = (xb >= 0) & (xb <= nx - 1)
    i0 = np.floor(xb).astype(np.int64)
    f = xb - i0
    i0 = np.clip(i0, 0, nx - 1)
    i1 = np.where(f > 0, np.minimum(i0 + 1, nx - 1), i0)
    u = j - c_out
    if g > 0:
        wA = np.clip((g - u) / (2.0 * g) if right else (g + u) / (2.0 * g), 0.0, 1.0)
    else:
        wA = np.ones(W)
    assert np.all(a_valid | b_valid), "a stitched column without a source"
    return dict(a_valid=a_valid, b_valid=b_valid, ja=np.clip(ja, 0, nx - 1), i0=i0, i1=i1, f=f, wA=wA, W=W, j0=j0, c_out=c_out,
                side="right" if right else "left")


def stitch(p, center, angles=None):
    """The stitched series of p (n, nx, nz) or of one sinogram (n, nx): float64 (h, W[, nz]), and the table."""
    p = np.asarray(p)
    flat = p.ndim == 2
    if flat:
        p = p[:, :, None]
    n = angle_span(angles, p.shape[0])
    nx = p.shape[1]
    h = n // 2
    T = column_table(nx, center)
    q = p.astype(np.float64)                                   # the values as they are: float32 data are exact in float64
    a = q[:h, T["ja"], :]
    f = T["f"][None, :, None]
    b = (1.0 - f) * q[h:2 * h, T["i0"], :] + f * q[h:2 * h, T["i1"], :]
    wA = T["wA"][None, :, None]
    av, bv = T["a_valid"][None, :, None], T["b_valid"][None, :, None]
    out = np.where(av & bv, wA * a + (1.0 - wA) * b, np.where(av, a, b))
    return (out[:, :, 0] if flat else out), T


# ------------------------------------------------------------------------------------------------------- analytic sinograms

OBJECTS = ((6, 4, 14, "d", 1.0), (-18, 10, 6, "d", 1.5), (0, -22, 8, "g", 1.2), (25, -5, 5, "g", 2.0), (-30, -20, 4, "d", 1.0))
CASES = ((120, 64, 52.3, 12), (120, 64, 55.75, 12), (120, 64, 10.2, 12), (90, 48, 40.5, 8), (240, 128, 101.37, 24), (240, 128, 120.0, 6))


def profile(s, r, kind, amp):
    """The parallel projection of a disc (2 sqrt(r^2 - s^2)) or of a Gaussian (r sqrt(2 pi) exp(-s^2 / 2 r^2)) at distance s."""
    if kind == "d":
        return amp * 2.0 * np.sqrt(np.maximum(r * r - s * s, 0.0))
    return amp * r * np.sqrt(2.0 * np.pi) * np.exp(-s * s / (2.0 * r * r))


def analytic(n_rows, step, nx, c, objects=OBJECTS, second_half=False):
    """n_rows rows at phi = i step (second_half: at pi + i step) on a detector of nx columns with the axis at column c, float64.  An
    object projects to the column c + cx cos phi + cy sin phi; the second half uses cos(phi + pi) = -cos phi, so that the two halves
    are mirror images of each other about c to the last bit wherever the column arithmetic is exact."""
    phi = np.arange(n_rows) * step
    x = np.arange(nx, dtype=np.float64)[None, :]
    S = np.zeros((n_rows, nx))
    for cx, cy, r, kind, amp in objects:
        q = (cx * np.cos(phi) + cy * np.sin(phi))[:, None]
        S += profile((x - c) + q if second_half else (x - c) - q, r, kind, amp)
    return S


def sinogram_360(n, nx, c, objects=OBJECTS, noise=0.0, seed=0, dtype=np.float32):
    """The 2 pi series of n rows; noise: Gaussian, this fraction of the maximum, from a fixed seed.  float32, what a stack holds, unless
    dtype says float64."""
    h = n // 2
    step = 2.0 * np.pi / n
    S = np.concatenate([analytic(h, step, nx, c, objects), analytic(h, step, nx, c, objects, second_half=True)])
    if noise:
        S = S + noise * S.max() * np.random.default_rng(seed).standard_normal(S.shape)
    return S.astype(dtype)


def sinogram_180(n, nx, c, objects=OBJECTS):
    """What the stitch of sinogram_360(n, nx, c) stands for: (the h rows over [0, pi) on W columns about c_out, float64; c_out)."""
    h, W, j0 = stitched_shape(n, nx, c)
    return analytic(h, 2.0 * np.pi / n, W, c + j0, objects), c + j0
