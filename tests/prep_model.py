"""numpy models of tomography_alignment_amd/preprocess.py (the formulas of its module docstring), for the CPU and GPU tests."""
import numpy as np
from scipy import ndimage


def reference_mean(frames):
    """float32(sum_j double(f_j) / n), summed in frame order."""
    f = np.asarray(frames)
    f = f[None] if f.ndim == 2 else f
    acc = np.zeros(f.shape[1:], np.float64)
    for j in range(f.shape[0]):
        acc += f[j].astype(np.float64)
    return (acc / f.shape[0]).astype(np.float32)


def reference_median(frames):
    """Exact per-pixel median; for even n float32(0.5 * (double(a) + double(b))) of the two middle values.  As in the kernel's key, -0 is
    read as +0 (the median of zeros is +0 whichever zero the sort leaves in the middle) and every NaN sorts above +inf."""
    f = np.asarray(frames)
    f = f[None] if f.ndim == 2 else f
    f = f.astype(np.float32)
    s = np.sort(np.where(f == 0, np.float32(0), f), axis=0)
    n = s.shape[0]
    a, b = s[(n - 1) // 2], s[n // 2]
    if n % 2:
        return a.copy()
    return (0.5 * (a.astype(np.float64) + b.astype(np.float64))).astype(np.float32)


def reference(frames, method):
    return reference_mean(frames) if method == "mean" else reference_median(frames)


def normalize(frames, flats, darks, cutoff=None, minus_log=True, min_ratio=1e-6, method="mean", crop=None):
    """The float32 sinogram (n, nx, nz), in the order of operations of the kernel."""
    flat, dark = reference(flats, method), reference(darks, method)
    raw = np.asarray(frames)
    (z0, z1), (x0, x1) = crop if crop is not None else ((0, raw.shape[1]), (0, raw.shape[2]))
    raw = raw[:, z0:z1, x0:x1].astype(np.float32)
    flat, dark = flat[z0:z1, x0:x1], dark[z0:z1, x0:x1]
    den = (flat - dark).astype(np.float32)
    den = np.where(den < np.float32(1e-6), np.float32(1e-6), den).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = ((raw - dark) / den).astype(np.float32)
        if cutoff is not None:
            r = np.fmin(r, np.float32(cutoff))
        out = -np.log(np.fmax(r, np.float32(min_ratio))) if minus_log else r
    return np.ascontiguousarray(out.astype(np.float32).transpose(0, 2, 1))


def stripe_keys(p):
    """The sort keys of the stripe removal as signed-orderable int64 values: -0 -> +0, every NaN one value above +inf."""
    v = np.where(p == 0, np.float32(0), p).astype(np.float32)       # canonicalises -0.0
    u = v.view(np.uint32).astype(np.int64)
    o = np.where(u & 0x80000000, (~u) & 0xffffffff, u | 0x80000000)
    return np.where(np.isnan(v), 0xffffffff, o)


def remove_stripe_sorting(p, size=21):
    """Vo et al. algorithm 3 on p[n_proj][nx][nz]: stable argsort along the angles of the canonicalised keys, scipy's median filter along
    x (mode='reflect') at equal rank, the inverse permutation."""
    p = np.asarray(p, np.float32)
    order = np.argsort(stripe_keys(p), axis=0, kind="stable")
    s = np.take_along_axis(np.where(p == 0, np.float32(0), p), order, axis=0)
    m = ndimage.median_filter(s, size=(1, size, 1), mode="reflect")
    out = np.empty_like(p)
    np.put_along_axis(out, order, m, axis=0)
    return out


def remove_stripe_sorting_vo(sino, size=21):
    """A direct restatement of Vo's algorithm 3 for one 2-D sinogram [n_proj][nx] (tie-free data): stack the column index with the data,
    sort each column, filter the sorted data, sort back by the index."""
    n, nx = sino.shape
    index = np.tile(np.arange(n), (nx, 1))                                  # [nx][n]
    mat = np.stack([index, sino.T], axis=2)                                  # [nx][n][2]
    mat = np.asarray([col[col[:, 1].argsort()] for col in mat])             # sort by value
    mat[:, :, 1] = ndimage.median_filter(mat[:, :, 1], (size, 1), mode="reflect")
    mat = np.asarray([col[col[:, 0].argsort()] for col in mat])             # back to the angles
    return mat[:, :, 1].T.astype(np.float32)


def stripe_amplitude(p):
    """Stripe amplitude of a sinogram [n_proj][nx] or [n_proj][nx][nz]: the std over x of the angle-mean minus its 9-px median."""
    m = np.asarray(p, np.float64).mean(axis=0)
    sm = ndimage.median_filter(m, size=(9,) + (1,) * (m.ndim - 1), mode="reflect")
    return float(np.mean(np.std(m - sm, axis=0)))
