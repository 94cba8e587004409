"""
Coarse pre-alignment of a projection series by FFT cross-correlation, on the GPU -- the device twin of the reference's
align/align_cc.py, with its four functions under their names, signatures and return values, plus the function the reference imports
from scikit-image (`phase_cross_correlation`) and a batched form of it, so that no scikit-image is needed.

Every call runs through libtomo_xcorr.so (include/tomo_xcorr.h): hipFFT Z2Z transforms and hand-written HIP kernels for the rest.
A chain (`cross_correlation_numpy`, `cross_correlation_skimage`) is one upload, n-1 steps enqueued on one stream -- the peak and
shift of step i stay in device memory, where step i's roll or spline shift and step i+1's reference read them -- and one download.
The moving images' spectra do not depend on the chain and are computed ahead in batched plans.  There is no CPU path: without a
device or hipFFT every function raises.

Each function takes an optional keyword `handle` (an `XcorrHandle`, reused between calls: its plans and buffers are kept); without
one, the call opens a handle and closes it before it returns.

Decisions (the reference's behaviour, pinned):
  * Arithmetic is float64 throughout the correlation and the spline, whatever the input dtype: the means (a deterministic float64
    sum), the windows and filters, the FFTs, the upsampled DFT and the B-spline.  This matches the reference's numpy arithmetic on
    float64 data and scikit-image's numpy-era float64 path; it is at least as accurate as scikit-image >= 0.19, which transforms
    float32 input in complex64.  (On float32 input numpy's np.mean is a float32 mean: this module's mean is float64.)
  * `aligned_proj` keeps the input dtype (float32 or float64; other dtypes raise TypeError).  Each aligned image is rounded to
    that dtype before it becomes the next step's reference, exactly as the reference stores it in `aligned_proj` first.
  * `phase_cross_correlation` is scikit-image's algorithm: normalization "phase" divides the cross-power spectrum by
    max(|F_ref conj(F_mov)|, 100 eps), None leaves it plain; the coarse peak (first index of equal maxima, as numpy's argmax) is
    wrapped by shifts[shifts > fix(n/2)] -= n; for upsample_factor u > 1 the shift is rounded to 1/u, the product is transformed by
    the matrix-multiply upsampled DFT over a region of ceil(1.5 u) samples centred at fix(region / 2) and the refined peak added.
    The shift along an axis of length 1 is 0.  error = sqrt(|1 - |CCmax|^2 / (src_amp target_amp)|) with amp = sum |F|^2 (divided
    by the image size for u = 1, as scikit-image does), phasediff = atan2(Im CCmax, Re CCmax).  No reference caller reads these
    two; they are kept for API compatibility.
  * The spline shift is scipy.ndimage.shift(x, s, order=3, mode='constant', cval=0.0, prefilter=True) of scipy 1.15: the cubic
    B-spline prefilter with its mirror boundary along axis 0 then axis 1, and an output point whose source coordinate lies outside
    [0, n-1] on either axis set to 0.
  * Non-square input: the reference's numpy path only runs on square images (filters of shape (nz, nx) multiply images of shape
    (nx, nz)).  Here the filters are built in image-axis order, and offsets[:, 0] wraps by the length of axis 0, offsets[:, 1] by
    that of axis 1.  For square input this is the reference exactly.
  * With 0 or 1 projections the offsets are zeros and `aligned_proj` is a copy.  `sinogram_order` is accepted and ignored, as in
    the reference.
"""
import numpy as np

from .._xcorr_lib import DTYPES, XcorrHandle

__all__ = ["cor_flipping", "cross_correlation_skimage", "cross_correlation_numpy", "crossCorrelationAlign",
           "phase_cross_correlation", "phase_cross_correlation_batch", "cc_filters", "XcorrHandle"]


class _Use(object):
    """The caller's handle, or one opened for this call and closed when it returns."""

    def __init__(self, handle):
        self.own = handle is None
        self.h = handle

    def __enter__(self):
        if self.own:
            self.h = XcorrHandle()
        return self.h

    def __exit__(self, *exc):
        if self.own:
            self.h.close()


def _stack(projections):
    p = np.asarray(projections)
    if p.ndim != 3:
        raise ValueError("projections must be (n_proj, nx, nz), got shape %s" % (p.shape,))
    if p.dtype not in DTYPES:
        raise TypeError("projections must be float32 or float64, got %s" % p.dtype)
    return np.ascontiguousarray(p)


def cc_filters(nx, nz):
    """The numpy path's (real-space window, k-space band filter), both (nx, nz) float64, in image-axis order.  For nx == nz they
    equal the reference's filter_r and filter_k exactly (those are symmetric in their two axes)."""
    kx = np.fft.fftfreq(nx)[:, None]
    kz = np.fft.fftfreq(nz)[None, :]
    abs_k = np.sqrt(kx ** 2 + kz ** 2)
    cutoff = 4
    filter_k = (abs_k <= (0.5 / cutoff)) * np.sin(2 * np.pi * cutoff * abs_k) ** 2
    x = np.linspace(1, nx, nx)[:, None]
    z = np.linspace(1, nz, nz)[None, :]
    filter_r = (np.sin(np.pi * x / nx) * np.sin(np.pi * z / nz)) ** 2
    return np.ascontiguousarray(filter_r), np.ascontiguousarray(filter_k)


def phase_cross_correlation_batch(refs, movings, upsample_factor=1, normalization="phase", *, handle=None):
    """B independent phase cross-correlations: refs, movings (B, nx, nz).  Returns (shifts (B, 2), error (B,), phasediff (B,))."""
    r = np.ascontiguousarray(refs, dtype=np.float64)
    m = np.ascontiguousarray(movings, dtype=np.float64)
    if r.ndim != 3 or r.shape != m.shape:
        raise ValueError("refs and movings must both be (B, nx, nz) of one shape, got %s and %s" % (r.shape, m.shape))
    if normalization not in ("phase", None):
        raise ValueError("normalization must be either phase or None")
    u = int(upsample_factor)
    if u != upsample_factor or u < 1:
        raise ValueError("upsample_factor must be an integer >= 1")
    if r.shape[0] == 0:
        return np.zeros((0, 2)), np.zeros(0), np.zeros(0)
    with _Use(handle) as h:
        return h.pcc_batch(r, m, u, normalization == "phase")


def phase_cross_correlation(reference_image, moving_image, upsample_factor=1, normalization="phase", *, handle=None):
    """scikit-image's phase_cross_correlation of two 2-D images: (shifts (2,), error, phasediff)."""
    r = np.asarray(reference_image)
    m = np.asarray(moving_image)
    if r.ndim != 2 or r.shape != m.shape:
        raise ValueError("images must be 2-D and of the same shape, got %s and %s" % (r.shape, m.shape))
    s, e, p = phase_cross_correlation_batch(r[None], m[None], upsample_factor, normalization, handle=handle)
    return s[0], float(e[0]), float(p[0])


def cor_flipping(proj_0, proj_180, *, handle=None):
    """Column shift of proj_0 against fliplr(proj_180) (phase correlation, upsample_factor 16): the centre-of-rotation offset."""
    out = phase_cross_correlation(proj_0, np.fliplr(np.asarray(proj_180)), upsample_factor=16, handle=handle)
    return out[0][1]


def cross_correlation_skimage(projections, sinogram_order='True', *, handle=None):
    """Chain i = 1..n-1: shifts = pcc(aligned[i-1], aligned[i], upsample_factor=100); aligned[i] = ndimage.shift(aligned[i], shifts).
    Returns (offsets (n, 2), aligned_proj)."""
    p = _stack(projections)
    if p.shape[0] < 2:
        return np.zeros((p.shape[0], 2)), p.copy()
    with _Use(handle) as h:
        return h.chain_skimage(p, 100)


def cross_correlation_numpy(projections, *, handle=None):
    """Chain i = 1..n-1: crossCorrelationAlign(aligned[i], aligned[i-1]) with the reference's window and band filter, offsets past
    half the image wrapped to negative.  Returns (offsets (n, 2), aligned_proj)."""
    p = _stack(projections)
    n, nx, nz = p.shape
    if n < 2:
        return np.zeros((n, 2)), p.copy()
    filter_r, filter_k = cc_filters(nx, nz)
    with _Use(handle) as h:
        offsets, aligned = h.chain_numpy(p, filter_r, filter_k)
    offsets[offsets[:, 0] > nx / 2, 0] -= nx
    offsets[offsets[:, 1] > nz / 2, 1] -= nz
    return offsets, aligned


def crossCorrelationAlign(image, reference, rFilter, kFilter, *, handle=None):
    """Align image to reference by cross-correlation with the caller's real-space and k-space filters (real, broadcastable to the
    image).  Returns (shifts (2 ints), output_image: image rolled by shifts, in image's dtype)."""
    img = np.asarray(image)
    ref = np.asarray(reference)
    if img.ndim != 2 or img.shape != ref.shape:
        raise ValueError("image and reference must be 2-D and of the same shape, got %s and %s" % (img.shape, ref.shape))
    if img.dtype not in DTYPES:
        raise TypeError("image must be float32 or float64, got %s" % img.dtype)
    dt = np.result_type(img.dtype, ref.dtype)
    if dt not in DTYPES:
        raise TypeError("reference must be a float array, got %s" % ref.dtype)
    if np.iscomplexobj(rFilter) or np.iscomplexobj(kFilter):
        raise TypeError("rFilter and kFilter must be real")
    fr = np.ascontiguousarray(np.broadcast_to(np.asarray(rFilter, np.float64), img.shape))
    fk = np.ascontiguousarray(np.broadcast_to(np.asarray(kFilter, np.float64), img.shape))
    pair = np.ascontiguousarray(np.stack([ref, img]).astype(dt, copy=False))
    with _Use(handle) as h:
        off, out = h.chain_numpy(pair, fr, fk)
    shifts = (np.intp(off[1, 0]), np.intp(off[1, 1]))
    return shifts, out[1].astype(img.dtype, copy=False)
