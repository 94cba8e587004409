"""
Preprocessing of raw projections on the GPU (libtomo_prep.so, include/tomo_prep.h): reference frames, flat-field normalisation with the
transpose into the package's sinogram layout, and stripe removal (sorting-based, large stripes, dead stripes, and the three combined).
The first step of the pipeline

    raw counts --remove_outlier--> --normalize--> sinogram --remove_stripe_sorting / remove_all_stripe--> align.align_cc / recon.fbp / examples.align_rigid

Layouts.  Raw frames, flats and darks are [n][rows = z][cols = x] (x fastest), uint16 or float32, uploaded in their own dtype.  The
sinogram is float32 p[n_proj][nx][nz] with z, the rotation axis, fastest -- what FBP, SIRT and OuterLoop read (OuterLoop takes the
device buffer as it is, with projections_shape).

Reference frames (reference_frames): each of the flat and dark stacks becomes one float32 frame.
    mean     float32(sum_j double(f_j) / n): the float64 sum runs in frame order, with no atomics, so the result is deterministic.
    median   n <= 64: exact selection per pixel; for an even n, float32(0.5 * (double(a) + double(b))) of the two middle values.

Normalisation (normalize), per pixel of the crop window z0:z1, x0:x1 (default the whole frame), all in float32 in this order:
    den = flat - dark;  den = den < 1e-6 ? 1e-6 : den
    r   = (float(raw) - dark) / den            IEEE division (the library is built without fast-math reciprocals)
    r   = fmin(r, cutoff)                      if a cutoff is given
    out = -log(fmax(r, min_ratio))             if minus_log (the default); else r
min_ratio (default 1e-6) keeps the output finite for zero, below-dark and dead-pixel counts: -log(1e-6) = 13.8.  The frame is written
transposed, out[i][x - x0][z - z0], through LDS tiles, so frame rows and sinogram rows are both read and written coalesced.

Stripe removal (remove_stripe_sorting): Vo, Atwood & Drakopoulos, Opt. Express 26 (2018), algorithm 3.  For every detector row z:
    1. sort each column (x, z) along the angle axis;
    2. median-filter the sorted array along x, at equal rank, with an odd window `size` and scipy.ndimage's mode='reflect'
       (half-sample symmetric: d c b a | a b c d | d c b a);
    3. put every filtered value back at the angle it came from.
The order is defined exactly, so the GPU matches a numpy model bit for bit:
    - the sort key is (orderable bits of v, angle index): every key is unique, and the order is numpy's argsort(kind='stable');
    - -0.0 is canonicalised to +0.0 before the key is built.  -log(1.0f) is -0.0f, so air pixels produce it; kept apart from +0.0 the two
      zeros would order differently from numpy's comparison, and the tie order decides which angle receives which filtered value;
    - every NaN maps to one key above +inf;
    - the median is an exact selection: the output is always one of the window's input values.
Limits: n_proj <= 8192 (one 64-bit key per angle in LDS; more raises PrepUnsupported before any launch), size odd with
3 <= size <= min(nx, 63).  z is processed in chunks whose scratch (10 bytes per sinogram value: sorted values, filtered values, uint16
permutation) fits max_scratch_bytes (default 2 GiB); the result does not depend on the chunking.  The removal needs every angle of a
column, so it runs on the full stack on one GPU; ranks that each hold a block of angles can still call normalize on their own frames.

Large, dead and all stripes (remove_large_stripe, remove_dead_stripe, remove_all_stripe): algorithms 5 and 6 of the same paper and their
combination, for what the sorting pass leaves: columns whose gain is wrong over the whole scan, and columns that are stuck or fluctuate.
Both build a float32 factor per column (x, z) and share one detector, which works on one z row at a time in float64:
    detector   factors f[x] (NaN and +inf read as FLT_MAX, -inf as -FLT_MAX) sorted descending into d; nd = nx // 4; a least-squares line
               through (i, d[i]), nd <= i < nx - nd - 1 (closed form, centred abscissae, sums in ascending i): intercept c, slope m;
               t1 = c + m (nx - 1), noise = max(|t1 - c|, 1e-6), v1 = |d[0] - c| / noise, v2 = |d[nx-1] - t1| / noise.  If v1 >= snr every
               x with f[x] > c + 0.5 snr noise is masked; if v2 >= snr every x with f[x] <= t1 - 0.5 snr noise; the mask is dilated by
               one column on each side.  snr is used as a float32.
    large      sort and median-filter (window `size`) as in the sorting pass; nd = int(0.5 clip(drop_ratio, 0, 0.8) n_proj); l1, l2 =
               float64 means, in rank order, of the sorted and of the smoothed values over the ranks nd <= r < n_proj - nd;
               f = l2 != 0 ? float32(l1 / l2) : 1.  With norm every value is divided by its column's f (IEEE float32); a masked column
               takes the smoothed value at the rank its angle had in the sort.  (The paper sorts the normalised column again; the ranks
               are the same whenever f > 0 and the division merges no two distinct values.)
    dead       n_proj >= 10.  u[a] = float32(sum_{k=a-5..a+4} double(s[k]) / 10) (reflected at the ends), diff[x] = float32(sum_a
               double(|s[a] - u[a]|)), bck = reflected median of diff along x (window `size`), f = bck != 0 ? diff / bck : 1.  After
               the detector the first and last two columns are unmasked; a masked column is interpolated along x, at the same angle,
               between the nearest unmasked columns xl < x < xr: s[xl] + (s[xr] - s[xl]) * (float(x - xl) / float(xr - xl)) in float32,
               every operation rounded on its own.  With norm the large pass (same snr and size, drop_ratio 0.1, norm) follows.
    all        dead (la_size, norm) then the sorting pass (sm_size).
Limits: those of the sorting pass, and 8 <= nx <= 8192 (the detector sorts one row of factors in LDS; more raises PrepUnsupported before
anything is uploaded).  The scratch is 10 bytes per value plus 13 per column (x, z) of a chunk; the result does not depend on the chunking.
return_mask=True also returns the detector's dilated mask(s) as boolean (nx, nz) arrays.

Zinger removal and the 2-D median filter (remove_outlier, median_filter): the first step of the chain, applied to the raw counts and to
the flats before anything else sees them (a zinger is a pixel, or a cluster of two or three, that a scattered photon or a cosmic ray
drives far above its neighbours in one frame).  frames is a stack [n][rows][cols] or one image [rows][cols], uint16 or float32 -- raw
frames [n][z][x] and the sinogram (n, nx, nz) alike; the output has the input's dtype.  size is 3, 5 or 7 (rows, cols >= size).  Per pixel v:
    window   the size x size values around it in its own frame, scipy.ndimage's mode='reflect' at the edges;
    med      the window's value of rank (size^2 - 1) / 2: uint16 ordered by value, float32 by the stripe sort's key (-0 read as +0, every
             NaN above +inf), decoded from the key -- a median of -0 is +0, a NaN median is the quiet NaN 0x7fc00000;
    remove_outlier   d = float32(v) - float32(med) (exact for uint16), |d| if two_sided; v becomes med if d >= dif or if v is not finite,
             else it keeps its bits.  dif >= 0 (as a float32), +inf only repairs non-finite pixels.  This is tomopy's remove_outlier
             with the exact median; one-sided is the default because zingers are bright.
    median_filter    every pixel becomes med.
return_count=True also gives, per frame, the number of pixels the test replaced (whether or not med differs from v), as int64.  `out`
may be the input: frames then go through the handle's scratch in batches bounded by max_scratch_bytes (default 2 GiB; 0: no limit; never
fewer than one frame), and the result does not depend on the batch.  The work is per frame: a rank that holds a block of angles filters
its own block.

Phase retrieval (retrieve_phase; libtomo_phase.so, include/tomo_phase.h): Paganin's single-distance filter, the step between the
flat-field division and the -log for data recorded with a propagation distance:
    normalize(minus_log=False) --retrieve_phase--> line integrals --remove_stripe_sorting--> ...
One parameter, the strength a = pi lambda z (delta/beta) / pixel_size^2 in pixels^2 (paganin_strength).  Per projection: pad by edge
replication to (Px, Pz), P the smallest even 2^i 3^j 5^k >= n_axis + 2 m with the data at offset (P - n_axis) // 2, m = pad if given,
else min(n_axis, ceil(8 sqrt(a) / (2 pi))); multiply the 2-D spectrum by H = 1 / (1 + a ((kx/Px)^2 + (kz/Pz)^2)); transform back, crop,
and out = -log(fmax(r, min_ratio)) if minus_log (the default), else r.  a = 0 is the identity, applied as such: retrieve_phase(p, 0) is
bit for bit minus_log(p).  Limits: a padded axis of at most 8192 values where a > 0 (PrepUnsupported before any launch otherwise), 0 <= a <= 1e12,
float32 transforms.  Frames are filtered in batches whose spectra and hipFFT work area fit max_scratch_bytes (default 2 GiB; 0: no limit;
never fewer than one frame); every frame is transformed on its own, so the result does not depend on the batch.  The work is per
projection: a rank that holds a block of angles filters its own block.

Dynamic flat-field correction (eigen_flats, normalize_dynamic; libtomo_dff.so, include/tomo_dff.h, whose comment defines the arithmetic):
Van Nieuwenhove et al., Opt. Express 23, 27975 (2015), for a beam that moves or changes shape between the flats and the projections.
    eigen_flats        fbar, dark = the float32 means of the stacks; G = the float64 Gram matrix of the K flats' deviations from fbar;
                       numpy.linalg.eigh(G), eigenvalues descending, every eigenvector's largest component positive; the eigen flat
                       fields e_j = float32(sum_k V[k][j] (F_k - fbar) / sqrt(K)), j < m.  n_eff=None keeps every leading eigenvalue
                       above eig_ratio x the median eigenvalue, at most MAX_EFF, possibly none.
    normalize_dynamic  projection i is divided by a flat of its own, fbar + sum_j w_ij e_j.  The m weights minimise the total variation
                       of s_i (raw_i - dark) / (flat_i - dark) on frames binned by `bin`, s_i the mean of the binned flat_i - dark
                       (without it a brighter flat would always lower the cost); L-BFGS-B from zero within +-w_max, every projection's
                       optimiser advanced side by side and all pending costs and gradients evaluated in one launch.  The apply step is
                       normalize's arithmetic with flat_i: with n_eff=0 or zero weights the result is normalize(method="mean") bit for bit.
A weight is in standard deviations of the flats' own variation along e_j.  A beam whose total intensity changes by a constant factor is
not recovered: s_i makes the cost blind to it, by design.  Limits (DffUnsupported before anything is uploaded): 2 <= K <= 128 flats,
m <= 8 and m <= K - 1, bin in 1 ... 8 with at least 2 x 2 binned pixels.  The binned counts live in the handle's scratch, in batches of
projections bounded by max_scratch_bytes (default 2 GiB; 0: no limit; never fewer than one); the result does not depend on the batch.
Every rank computes the same eigen flat fields from the same flats and normalises its own block of angles, on its own or with weights=.

The kernels live in their own library, like libtomo_fbp.so and libtomo_xcorr.so, so that the projector's sources and the kernel-source
hash that keys the committed PMC counters do not change.  Host arrays and _lib.DeviceArrays are both accepted; a device input gives a
device output, with no host round trip, and every temporary buffer is freed before a call returns.  Arguments are checked (ValueError)
before anything is uploaded or launched.
"""
import math

import numpy as np

from . import _dff_lib, _lbfgsb_batch, _phase_lib, _prep_lib
from ._dff_lib import DffUnsupported  # noqa: F401  (re-exported)
from ._ops import HandleOwner, Staging, _is_dev
from ._prep_lib import PrepUnsupported  # noqa: F401  (re-exported)

DEFAULT_SCRATCH_BYTES = 2 << 30
METHODS = {"mean": _prep_lib.MEAN, "median": _prep_lib.MEDIAN}
_DTYPES = {np.dtype(np.uint16): _prep_lib.U16, np.dtype(np.float32): _prep_lib.F32}
_DFF_DTYPES = {np.dtype(np.uint16): _dff_lib.U16, np.dtype(np.float32): _dff_lib.F32}
MAX_EFF = _dff_lib.MAX_EFF
# L-BFGS-B options of normalize_dynamic's minimisation (scipy's names).  ftol: the device evaluates the cost in float32 with float64 sums
# and agrees with float64 arithmetic to 1e-7 of the cost; scipy's default 2.2e-9 asks the line search for decreases
# below that noise, which cost five times the evaluations on the test data and moved no weight by more than 0.006.
TV_OPTIONS = {"ftol": 1e-7}


def _shape_dtype(a, what, ndims):
    shape = tuple(a.shape) if _is_dev(a) else np.shape(a)
    dtype = a.dtype if _is_dev(a) else np.asarray(a).dtype
    if len(shape) not in ndims:
        raise ValueError("%s must have %s dimensions, got shape %s" % (what, " or ".join(str(d) for d in ndims), shape))
    if np.dtype(dtype) not in _DTYPES:
        raise ValueError("%s must be uint16 or float32, got %s" % (what, dtype))
    if any(s < 1 for s in shape):
        raise ValueError("%s must not be empty, got shape %s" % (what, shape))
    return shape, np.dtype(dtype)


def _crop(crop, rows, cols):
    if crop is None:
        return (0, rows), (0, cols)
    try:
        cz, cx = crop
    except (TypeError, ValueError):
        raise ValueError("crop must be ((z0, z1), (x0, x1)) or (slice, slice)")
    out = []
    for c, n, name in ((cz, rows, "z"), (cx, cols, "x")):
        if isinstance(c, slice):
            if c.step not in (None, 1):
                raise ValueError("crop: slices must have step 1")
            c = (0 if c.start is None else c.start, n if c.stop is None else c.stop)
        a, b = (int(v) for v in c)
        if not (0 <= a < b <= n):
            raise ValueError("crop %s window %d:%d lies outside the frame (0:%d) or is empty" % (name, a, b, n))
        out.append((a, b))
    return tuple(out)


WAVELENGTH_KEV_M = 1.2398419843320026e-9      # h c in keV m: lambda = WAVELENGTH_KEV_M / E_keV


def paganin_strength(pixel_size, dist, energy=None, wavelength=None, delta_beta=1000.0):
    """The dimensionless strength a = pi lambda z (delta/beta) / pixel_size^2 (pixels^2) of retrieve_phase.  pixel_size and dist (the
    propagation distance z) in metres; give exactly one of energy (keV) and wavelength (metres)."""
    if (energy is None) == (wavelength is None):
        raise ValueError("give exactly one of energy (keV) and wavelength (m)")
    vals = dict(pixel_size=pixel_size, dist=dist, delta_beta=delta_beta)
    vals["wavelength" if energy is None else "energy"] = wavelength if energy is None else energy
    for k, v in vals.items():
        v = vals[k] = float(v)
        positive = k not in ("dist", "delta_beta")
        if not math.isfinite(v) or v < 0 or (positive and v == 0):
            raise ValueError("%s must be finite and %s, got %r" % (k, "> 0" if positive else ">= 0", v))
    lam = WAVELENGTH_KEV_M / vals["energy"] if wavelength is None else vals["wavelength"]
    return math.pi * lam * vals["dist"] * vals["delta_beta"] / vals["pixel_size"] ** 2


def _fast_even(want):
    """The smallest even 2^i 3^j 5^k >= want."""
    p = max(2, int(want) + (int(want) & 1))
    while True:
        q = p
        for f in (2, 3, 5):
            while q % f == 0:
                q //= f
        if q == 1:
            return p
        p += 2


def phase_padding(n_axis, strength, pad=None):
    """(m, P): the padding on each side and the padded length of an axis of n_axis values (module docstring)."""
    m = int(pad) if pad is not None else min(int(n_axis), int(math.ceil(8.0 * math.sqrt(strength) / (2.0 * math.pi))))
    return m, _fast_even(int(n_axis) + 2 * m)


def _check_out(proj, out, size):
    if out is None:
        return
    if not (_is_dev(out) and out.dtype == np.float32 and out.size == size):
        raise ValueError("out must be a float32 DeviceArray of %d values" % size)
    if not _is_dev(proj):
        raise ValueError("out needs a DeviceArray input (a host input gives a host result)")
    if out.ptr.value != proj.ptr.value:
        a0, b0 = proj.ptr.value, out.ptr.value
        if a0 < b0 + out.nbytes and b0 < a0 + proj.nbytes:
            raise ValueError("out must be proj itself or not overlap it")


def _check_min_ratio(min_ratio):
    try:
        ok = bool(np.isfinite(min_ratio) and min_ratio > 0 and np.float32(min_ratio) > 0)
    except TypeError:
        ok = False
    if not ok:
        raise ValueError("min_ratio must be finite and > 0 (in float32), got %r" % (min_ratio,))


def _float32_stack(proj):
    shape, dtype = _shape_dtype(proj, "proj", (3,))
    if dtype != np.float32:
        raise ValueError("proj must be float32, got %s" % dtype)
    return shape


def _check_window(size, nx, name="size"):
    if isinstance(size, (bool, np.bool_)) or int(size) != size:
        raise ValueError("%s must be an odd integer, got %r" % (name, size))
    size = int(size)
    if size % 2 == 0 or size < 3 or size > min(nx, _prep_lib.MAX_STRIPE_SIZE):
        raise ValueError("%s must be odd with 3 <= %s <= min(nx, 63) = %d, got %d" % (name, name, min(nx, _prep_lib.MAX_STRIPE_SIZE), size))
    return size


def _check_stripe_args(proj, snr, out, max_scratch_bytes, min_nproj, what):
    """(shape, float32 snr, budget) of a large / dead / all call, or ValueError / PrepUnsupported: nothing is uploaded before this."""
    shape = _float32_stack(proj)
    n, nx, nz = shape
    if n < min_nproj:
        raise ValueError("%s needs n_proj >= %d, got %d" % (what, min_nproj, n))
    if nx < _prep_lib.MIN_STRIPE_NDX:
        raise ValueError("%s needs nx >= %d, got %d" % (what, _prep_lib.MIN_STRIPE_NDX, nx))
    if n > _prep_lib.MAX_NPROJ or nx > _prep_lib.MAX_STRIPE_NDX:
        raise PrepUnsupported("%s: n_proj %d, nx %d exceed the %d angles / %d columns one work-group sorts in LDS; nothing was written"
                              % (what, n, nx, _prep_lib.MAX_NPROJ, _prep_lib.MAX_STRIPE_NDX))
    try:
        snr32 = np.float32(snr)
        ok = not isinstance(snr, (bool, np.bool_)) and bool(np.isfinite(snr32) and snr32 > 0)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("snr must be finite and > 0 (in float32), got %r" % (snr,))
    budget = DEFAULT_SCRATCH_BYTES if max_scratch_bytes is None else int(max_scratch_bytes)
    if budget < 0:
        raise ValueError("max_scratch_bytes must be >= 0 (0: no limit)")
    if out is not None:
        if not (_is_dev(out) and out.dtype == np.float32 and out.size == n * nx * nz):
            raise ValueError("out must be a float32 DeviceArray of %d values" % (n * nx * nz))
        if _is_dev(proj) and out.ptr.value != proj.ptr.value:
            a0, b0 = proj.ptr.value, out.ptr.value
            if a0 < b0 + out.nbytes and b0 < a0 + proj.nbytes:
                raise ValueError("out must be proj itself or not overlap it")
    return shape, float(snr32), budget


def _check_outlier_args(frames, size, out, max_scratch_bytes):
    """((n, rows, cols), dtype, size, budget) of a remove_outlier / median_filter call, or ValueError: nothing is uploaded before this."""
    shape, dtype = _shape_dtype(frames, "frames", (2, 3))
    n, rows, cols = (1,) + shape if len(shape) == 2 else shape
    if isinstance(size, (bool, np.bool_)) or not isinstance(size, (int, np.integer)) or int(size) not in _prep_lib.OUTLIER_SIZES:
        raise ValueError("size must be 3, 5 or 7, got %r" % (size,))
    size = int(size)
    if rows < size or cols < size:
        raise ValueError("frames of %d x %d are smaller than the window: rows and cols must be >= size = %d" % (rows, cols, size))
    if rows * cols >= 2 ** 31:
        raise ValueError("frames must have fewer than 2^31 pixels each, got %d x %d" % (rows, cols))
    budget = DEFAULT_SCRATCH_BYTES if max_scratch_bytes is None else int(max_scratch_bytes)
    if budget < 0:
        raise ValueError("max_scratch_bytes must be >= 0 (0: no limit)")
    if out is not None:
        if not (_is_dev(out) and out.dtype == dtype and out.size == n * rows * cols):
            raise ValueError("out must be a %s DeviceArray of %d values" % (dtype, n * rows * cols))
        if not _is_dev(frames):
            raise ValueError("out needs a DeviceArray input (a host input gives a host result)")
        if out.ptr.value != frames.ptr.value:
            a0, b0 = frames.ptr.value, out.ptr.value
            if a0 < b0 + out.nbytes and b0 < a0 + frames.nbytes:
                raise ValueError("out must be frames itself or not overlap it")
    return (n, rows, cols), dtype, size, budget


def _check_dif(dif):
    """dif as the float32 the kernel compares with, or ValueError."""
    try:
        dif32 = np.float32(dif)
        ok = not isinstance(dif, (bool, np.bool_)) and bool(dif32 >= 0)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("dif must be a number >= 0 (in float32; inf is allowed, NaN is not), got %r" % (dif,))
    return float(dif32)


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _positive(v, name):
    try:
        ok = not isinstance(v, (bool, np.bool_)) and math.isfinite(float(v)) and float(v) > 0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("%s must be finite and > 0, got %r" % (name, v))
    return float(v)


def eigen_decomposition(G):
    """(eigenvalues descending, V): numpy.linalg.eigh of the Gram matrix G, every eigenvector V[:, j] signed so that its component of
    largest magnitude -- the lowest index on a tie -- is positive."""
    lam, V = np.linalg.eigh(np.asarray(G, np.float64))
    lam, V = lam[::-1].copy(), V[:, ::-1].copy()
    for j in range(V.shape[1]):
        if V[np.argmax(np.abs(V[:, j])), j] < 0:
            V[:, j] = -V[:, j]
    return lam, V


def count_eigen_flats(eigenvalues, eig_ratio=2.0):
    """How many leading eigenvalues exceed eig_ratio x the median eigenvalue, at most MAX_EFF (and possibly none)."""
    med = float(np.median(eigenvalues))
    m = 0
    while m < min(len(eigenvalues), MAX_EFF) and eigenvalues[m] > eig_ratio * med:
        m += 1
    return m


class EigenFlats(object):
    """What eigen_flats returns, on the device: `flat` and `dark`, float32 [z][x]; `eff`, the eigen flat fields, float32 [m][z][x] (None
    where n_eff = 0); and on the host `eigenvalues` (K,) of the flats' Gram matrix, descending, and `n_eff` = m.  free() releases the
    device buffers; a context manager."""

    def __init__(self, flat, dark, eff, eigenvalues, n_eff):
        self.flat, self.dark, self.eff = flat, dark, eff
        self.eigenvalues, self.n_eff = np.asarray(eigenvalues, np.float64), int(n_eff)
        self.shape = tuple(flat.shape)

    def free(self):
        for d in (self.flat, self.dark, self.eff):
            if d is not None:
                d.free()
        self.flat = self.dark = self.eff = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def _check_n_eff(n_eff):
    if n_eff is not None and (not _is_int(n_eff) or n_eff < 0):
        raise ValueError("n_eff must be None or an integer >= 0, got %r" % (n_eff,))
    return None if n_eff is None else int(n_eff)


class Preprocessor(HandleOwner):
    """One libtomo_prep handle and its scratch, reused across calls.  ctx: the _lib.Context whose device and stream the work uses (work
    is enqueued on ctx.stream(), in order with the projector work that follows); default the context of the first DeviceArray passed in,
    or a context of the handle's own.  Arguments are checked before the context or the handle is made."""

    def __init__(self, ctx=None):
        HandleOwner.__init__(self, ctx)
        self._phase = None
        self._dff = None

    def _new_handle(self):
        return _prep_lib.PrepHandle(self.ctx.device)

    def close(self):
        if self._phase is not None:
            self._phase.close()
            self._phase = None
        if self._dff is not None:
            self._dff.close()
            self._dff = None
        HandleOwner.close(self)

    def _reference(self, st, d, shape, dtype, method):
        """The reference frame of the stack d, an array of the staging st."""
        n = 1 if len(shape) == 2 else shape[0]
        rows, cols = shape[-2:]
        out = st.scratch((rows, cols))
        self.handle.reference(self.ctx.stream(), d.ptr, _DTYPES[dtype], n, rows, cols, METHODS[method], out.ptr)
        return out

    def _check_reference_args(self, stacks, method):
        if method not in METHODS:
            raise ValueError("method must be 'mean' or 'median', got %r" % (method,))
        infos = []
        for a, what in stacks:
            shape, dtype = _shape_dtype(a, what, (2, 3))
            n = 1 if len(shape) == 2 else shape[0]
            if method == "median" and n > _prep_lib.MAX_MEDIAN_FRAMES:
                raise PrepUnsupported("%s: the median supports at most %d frames, got %d" % (what, _prep_lib.MAX_MEDIAN_FRAMES, n))
            infos.append((shape, dtype))
        if infos[0][0][-2:] != infos[1][0][-2:]:
            raise ValueError("flats and darks must have the same frame shape, got %s and %s" % (infos[0][0][-2:], infos[1][0][-2:]))
        return infos

    def reference_frames(self, flats, darks, method="mean"):
        """(flat, dark): float32 [rows][cols] frames reduced from the stacks flats, darks ([n][rows][cols] or one [rows][cols] frame).
        DeviceArrays when flats is one, ndarrays otherwise."""
        infos = self._check_reference_args(((flats, "flats"), (darks, "darks")), method)
        self._ready(flats)
        with self._staging(flats) as st:
            res = [self._reference(st, st.source(a, None), shape, dtype, method) for a, (shape, dtype) in zip((flats, darks), infos)]
            return tuple(st.result(r) for r in res)

    def normalize(self, frames, flats, darks, cutoff=None, minus_log=True, min_ratio=1e-6, method="mean", crop=None, out=None):
        """The (n_proj, nx, nz) float32 sinogram of raw frames [n_proj][rows][cols] (module docstring): an ndarray for host frames, a
        DeviceArray for device frames (`out`, a float32 DeviceArray of that shape, if given)."""
        shape, dtype = _shape_dtype(frames, "frames", (3,))
        n, rows, cols = shape
        infos = self._check_reference_args(((flats, "flats"), (darks, "darks")), method)
        if infos[0][0][-2:] != (rows, cols):
            raise ValueError("flats and darks must have the frames' shape %s, got %s" % ((rows, cols), infos[0][0][-2:]))
        (z0, z1), (x0, x1) = _crop(crop, rows, cols)
        if not (np.isfinite(min_ratio) and min_ratio > 0):
            raise ValueError("min_ratio must be finite and > 0, got %r" % (min_ratio,))
        if cutoff is not None and not np.isfinite(cutoff):
            raise ValueError("cutoff must be finite or None, got %r" % (cutoff,))
        oshape = (n, x1 - x0, z1 - z0)
        if out is not None and not (_is_dev(out) and out.dtype == np.float32 and out.size == int(np.prod(oshape))):
            raise ValueError("out must be a float32 DeviceArray of %d values %s" % (int(np.prod(oshape)), oshape))
        self._ready(frames)
        with self._staging(frames) as st:
            d_raw = st.source(frames, None)
            d_flat, d_dark = [self._reference(st, st.source(a, None), s, dt, method) for a, (s, dt) in zip((flats, darks), infos)]
            res = st.dest(oshape, np.float32, out)
            self.handle.normalize(self.ctx.stream(), d_raw.ptr, _DTYPES[dtype], n, rows, cols, d_flat.ptr, d_dark.ptr,
                                  ((z0, z1), (x0, x1)), cutoff, minus_log, min_ratio, res.ptr)
            return st.result(res)

    def _ready_dff(self, like):
        self._ready(like)
        if self._dff is None:
            self._dff = _dff_lib.DffHandle(self.ctx.device)

    def _check_eigen_args(self, flats, darks, n_eff, eig_ratio, bin=1):
        """((flats' shape, dtype), (darks' shape, dtype), n_eff) or ValueError / DffUnsupported: nothing is uploaded before this."""
        infos = self._check_reference_args(((flats, "flats"), (darks, "darks")), "mean")
        n_eff = _check_n_eff(n_eff)
        _positive(eig_ratio, "eig_ratio")
        shape = infos[0][0]
        K = 1 if len(shape) == 2 else shape[0]
        _dff_lib.check(K, 0 if n_eff is None else n_eff, shape[-2], shape[-1], bin)
        return infos[0], infos[1], n_eff

    def _eigen_flats(self, keep, flats, darks, infos, n_eff, eig_ratio):
        """The EigenFlats, its three arrays made in the staging `keep` of the caller; the uploads go when they are made."""
        (fshape, fdtype), (dshape, ddtype) = infos
        K, rows, cols = fshape
        stream = self.ctx.stream()
        with self._staging(flats) as st:
            d_flats = st.source(flats, None)
            flat = self._reference(keep, d_flats, fshape, fdtype, "mean")
            dark = self._reference(keep, st.source(darks, None), dshape, ddtype, "mean")
            lam, V = eigen_decomposition(self._dff.gram(stream, d_flats.ptr, _DFF_DTYPES[fdtype], K, rows, cols, flat.ptr))
            m = count_eigen_flats(lam, eig_ratio) if n_eff is None else n_eff
            eff = None
            if m:
                eff = keep.scratch((m, rows, cols))
                self._dff.eff(stream, d_flats.ptr, _DFF_DTYPES[fdtype], K, rows, cols, flat.ptr, V[:, :m], eff.ptr)
            return EigenFlats(flat, dark, eff, lam, m)

    def eigen_flats(self, flats, darks, n_eff=None, eig_ratio=2.0):
        """The EigenFlats (module docstring) of the stacks flats [K][rows][cols] and darks, uint16 or float32, host or device: the mean
        flat, the mean dark and the n_eff leading eigen flat fields, all on the device.  n_eff=None: as many as have an eigenvalue above
        eig_ratio x the median eigenvalue (at most MAX_EFF, possibly 0)."""
        f, d, n_eff = self._check_eigen_args(flats, darks, n_eff, eig_ratio)
        self._ready_dff(flats)
        with Staging(self.ctx, True) as keep:                    # the fields stay on the device whatever the flats are
            ef = self._eigen_flats(keep, flats, darks, (f, d), n_eff, eig_ratio)
            for a in (ef.flat, ef.dark, ef.eff):
                keep.result(a)
            return ef

    def _estimate_weights(self, d_raw, dtype, n, rows, cols, ef, m, bin, tv_eps, w_max, budget):
        """((n, m) float64 weights, evaluations): the total-variation minimisation of normalize_dynamic."""
        from . import alignment
        h, st = self._dff, self.ctx.stream()
        zb, xb = rows // bin, cols // bin
        W, nfev = np.zeros((n, m), np.float64), 0
        h.set_max_scratch(budget)
        with self._staging(d_raw) as scratch:
            Fb, Eb = scratch.scratch((zb, xb)), scratch.scratch((m, zb, xb))
            h.bin(st, ef.flat.ptr, _dff_lib.F32, 1, rows, cols, bin, ef.dark.ptr, Fb.ptr)
            h.bin(st, ef.eff.ptr, _dff_lib.F32, m, rows, cols, bin, None, Eb.ptr)
            a = np.array([np.mean(Fb.download().astype(np.float64))] + [np.mean(e.astype(np.float64)) for e in Eb.download()], np.float64)
            bounds = [(-w_max, w_max)] * m
            nb = min(_dff_lib.batch(n, rows, cols, bin, budget), _dff_lib.MAX_IDS)      # one launch lists at most MAX_IDS projections
            batched = alignment.batch_driver_available()
            from concurrent.futures import ThreadPoolExecutor
            for i0 in range(0, n, nb):
                cnt = min(nb, n - i0)
                h.load_projections(st, d_raw.ptr, _DFF_DTYPES[dtype], i0, cnt, rows, cols, bin, ef.dark.ptr)

                def fun_batch(ids, X, i0=i0):
                    w = np.asarray(X, np.float64).reshape(len(ids), m).astype(np.float32)
                    s = a[0] + w.astype(np.float64) @ a[1:]              # float64; the library takes it rounded
                    return h.cost(st, i0 + np.asarray(ids, np.int64), w, s, a, tv_eps, Fb.ptr, Eb.ptr)

                # the helper thread is the only one that touches the GPU while the pass runs (alignment.align_projections)
                with ThreadPoolExecutor(max_workers=1, initializer=self.ctx.make_current) as pool:
                    if batched:
                        x, _, nf, _ = _lbfgsb_batch.minimize_many(fun_batch, np.zeros((cnt, m)), bounds=bounds, options=TV_OPTIONS, overlap=pool.submit)
                    else:                                                # this scipy's core is laid out differently: one problem at a time
                        from scipy import optimize
                        x, nf = np.zeros((cnt, m)), np.zeros(cnt, np.int64)
                        for i in range(cnt):
                            def fun(p, i=i):
                                f, g = pool.submit(fun_batch, [i], p[None]).result()
                                return f[0], g[0]
                            res = optimize.minimize(fun, np.zeros(m), jac=True, method="L-BFGS-B", bounds=bounds, options=dict(TV_OPTIONS))
                            x[i], nf[i] = res.x, res.nfev
                W[i0:i0 + cnt], nfev = x, nfev + int(np.sum(nf))
        return W, nfev

    def normalize_dynamic(self, frames, flats, darks=None, n_eff=None, eig_ratio=2.0, bin=2, tv_eps=1e-3, w_max=10.0, weights=None,
                          cutoff=None, minus_log=True, min_ratio=1e-6, crop=None, out=None, max_scratch_bytes=None, return_weights=False):
        """normalize with a flat per projection (module docstring): the (n_proj, nx, nz) float32 sinogram of raw frames
        [n_proj][rows][cols], an ndarray for host frames, a DeviceArray for device frames (`out`, a float32 DeviceArray of that shape,
        if given).  flats: the stack of flats (with darks), or an EigenFlats (darks must then be None; n_eff may select fewer of its
        fields).  weights: an (n_proj, m) array skips the estimation and only applies -- a rank that holds a block of angles passes
        its rows.  return_weights=True: (result, (n_proj, m) float64 weights, number of cost evaluations)."""
        shape, dtype = _shape_dtype(frames, "frames", (3,))
        n, rows, cols = shape
        given = isinstance(flats, EigenFlats)
        if not _is_int(bin):
            raise ValueError("bin must be an integer in 1 ... %d, got %r" % (_dff_lib.MAX_BIN, bin))
        n_eff = _check_n_eff(n_eff)
        if weights is not None:
            weights = np.asarray(weights)
            if weights.ndim != 2 or weights.shape[0] != n or not np.issubdtype(weights.dtype, np.number) or not np.all(np.isfinite(weights)):
                raise ValueError("weights must be a finite (%d, m) array, got shape %s" % (n, weights.shape))
            weights = weights.astype(np.float64)
            if n_eff is None:
                n_eff = weights.shape[1]
            if weights.shape[1] != n_eff:
                raise ValueError("weights has %d columns for n_eff = %d" % (weights.shape[1], n_eff))
        if given:
            if darks is not None:
                raise ValueError("darks must be None where flats is an EigenFlats (it holds the dark)")
            if flats.flat is None:
                raise ValueError("the EigenFlats has been freed")
            _positive(eig_ratio, "eig_ratio")
            if flats.shape != (rows, cols):
                raise ValueError("the EigenFlats must have the frames' shape %s, got %s" % ((rows, cols), flats.shape))
            if n_eff is not None and n_eff > flats.n_eff:
                raise ValueError("n_eff = %d exceeds the %d fields of the EigenFlats" % (n_eff, flats.n_eff))
            infos = None
        else:
            if darks is None:
                raise ValueError("darks must be given with a stack of flats")
            f, d, n_eff = self._check_eigen_args(flats, darks, n_eff, eig_ratio, bin)
            infos = (f, d)
            if f[0][-2:] != (rows, cols):
                raise ValueError("flats and darks must have the frames' shape %s, got %s" % ((rows, cols), f[0][-2:]))
        tv_eps, w_max = _positive(tv_eps, "tv_eps"), _positive(w_max, "w_max")
        (z0, z1), (x0, x1) = _crop(crop, rows, cols)
        _check_min_ratio(min_ratio)
        if cutoff is not None and not np.isfinite(cutoff):
            raise ValueError("cutoff must be finite or None, got %r" % (cutoff,))
        budget = DEFAULT_SCRATCH_BYTES if max_scratch_bytes is None else int(max_scratch_bytes)
        if budget < 0:
            raise ValueError("max_scratch_bytes must be >= 0 (0: no limit)")
        oshape = (n, x1 - x0, z1 - z0)
        if out is not None and not (_is_dev(out) and out.dtype == np.float32 and out.size == int(np.prod(oshape))):
            raise ValueError("out must be a float32 DeviceArray of %d values %s" % (int(np.prod(oshape)), oshape))
        if out is not None and not _is_dev(frames):
            raise ValueError("out needs a DeviceArray input (a host input gives a host result)")
        if given:
            _dff_lib.check(max(2, flats.n_eff + 1), flats.n_eff, rows, cols, bin)      # the frame and the bin factor
        self._ready_dff(frames)
        with self._staging(frames) as st:
            d_raw = st.source(frames, None)
            ef = flats if given else self._eigen_flats(st, flats, darks, infos, n_eff, eig_ratio)      # its fields go with this call
            m = ef.n_eff if n_eff is None else n_eff
            nfev = 0
            if weights is None:
                weights = np.zeros((n, m), np.float64)
                if m:
                    weights, nfev = self._estimate_weights(d_raw, dtype, n, rows, cols, ef, m, int(bin), tv_eps, w_max, budget)
            res = st.dest(oshape, np.float32, out)
            self._dff.apply(self.ctx.stream(), d_raw.ptr, _DFF_DTYPES[dtype], n, rows, cols, ef.flat.ptr, ef.dark.ptr,
                            None if not m else ef.eff.ptr, weights.astype(np.float32).reshape(n, m), ((z0, z1), (x0, x1)), cutoff, minus_log,
                            min_ratio, res.ptr)
            result = st.result(res)
        return (result, weights, nfev) if return_weights else result

    def remove_stripe_sorting(self, proj, size=21, out=None, max_scratch_bytes=None, timed=False):
        """Stripe removal of the sinogram proj [n_proj][nx][nz] (float32; module docstring).  Host in: an ndarray out.  Device in: the
        result goes to `out` (a float32 DeviceArray of the same size; `out=proj` works in place) or a new DeviceArray.
        timed=True (benchmarks): returns (result, (sort_ms, median_ms, scatter_ms)) after a synchronisation."""
        shape, dtype = _shape_dtype(proj, "proj", (3,))
        if dtype != np.float32:
            raise ValueError("proj must be float32, got %s" % dtype)
        n, nx, nz = shape
        if isinstance(size, (bool, np.bool_)) or int(size) != size:
            raise ValueError("size must be an odd integer, got %r" % (size,))
        size = int(size)
        if size % 2 == 0 or size < 3 or size > min(nx, _prep_lib.MAX_STRIPE_SIZE):
            raise ValueError("size must be odd with 3 <= size <= min(nx, 63) = %d, got %d" % (min(nx, _prep_lib.MAX_STRIPE_SIZE), size))
        budget = DEFAULT_SCRATCH_BYTES if max_scratch_bytes is None else int(max_scratch_bytes)
        if budget < 0:
            raise ValueError("max_scratch_bytes must be >= 0 (0: no limit)")
        if out is not None:
            if not (_is_dev(out) and out.dtype == np.float32 and out.size == n * nx * nz):
                raise ValueError("out must be a float32 DeviceArray of %d values" % (n * nx * nz))
            if _is_dev(proj) and out.ptr.value != proj.ptr.value:
                a0, b0 = proj.ptr.value, out.ptr.value
                if a0 < b0 + out.nbytes and b0 < a0 + proj.nbytes:
                    raise ValueError("out must be proj itself or not overlap it")
        self._ready(proj)
        with self._staging(proj) as st:
            d_in = st.source(proj)
            res = st.dest(shape, np.float32, out)
            ms = self.handle.stripe_sorting(self.ctx.stream(), d_in.ptr, res.ptr, n, nx, nz, size, budget, timed)
            result = st.result(res)
        return (result, ms) if timed else result

    def _run_stripe(self, proj, shape, out, n_masks, call):
        """Upload / allocate as remove_stripe_sorting does, run call(d_in, d_out, masks) with n_masks zeroed uint8 (nx, nz) device
        buffers, and return (result, mask, ...) with the masks as boolean ndarrays."""
        self._ready(proj)
        with self._staging(proj) as st:
            d_in = st.source(proj)
            res = st.dest(shape, np.float32, out)
            masks = [st.scratch(shape[1:], np.uint8, zero=True) for _ in range(n_masks)]
            call(d_in, res, [m.ptr for m in masks])
            host_masks = tuple(m.download().astype(bool) for m in masks)
            result = st.result(res)
        return (result,) + host_masks if n_masks else result

    def remove_large_stripe(self, proj, snr=3.0, size=51, drop_ratio=0.1, norm=True, out=None, max_scratch_bytes=None, return_mask=False):
        """Large-stripe removal (Vo algorithm 5; module docstring) of the sinogram proj [n_proj][nx][nz] (float32).  Host in: an ndarray
        out.  Device in: the result goes to `out` (`out=proj` works in place) or a new DeviceArray.  return_mask=True: (result, mask)."""
        shape, snr, budget = _check_stripe_args(proj, snr, out, max_scratch_bytes, 1, "remove_large_stripe")
        n, nx, nz = shape
        size = _check_window(size, nx)
        try:
            drop_ratio = float(drop_ratio)
        except (TypeError, ValueError):
            drop_ratio = float("nan")
        if not math.isfinite(drop_ratio):
            raise ValueError("drop_ratio must be a finite number (it is clipped to 0 ... 0.8)")

        def call(d_in, d_out, masks):
            self.handle.stripe_large(self.ctx.stream(), d_in.ptr, d_out.ptr, n, nx, nz, snr, size, drop_ratio, norm, budget,
                                     masks[0] if masks else None)

        return self._run_stripe(proj, shape, out, 1 if return_mask else 0, call)

    def remove_dead_stripe(self, proj, snr=3.0, size=51, norm=True, out=None, max_scratch_bytes=None, return_mask=False):
        """Dead-stripe removal (Vo algorithm 6; module docstring), n_proj >= 10.  Conventions as remove_large_stripe; the mask is that
        of the dead-stripe detector."""
        shape, snr, budget = _check_stripe_args(proj, snr, out, max_scratch_bytes, _prep_lib.MIN_DEAD_NPROJ, "remove_dead_stripe")
        n, nx, nz = shape
        size = _check_window(size, nx)

        def call(d_in, d_out, masks):
            self.handle.stripe_dead(self.ctx.stream(), d_in.ptr, d_out.ptr, n, nx, nz, snr, size, norm, budget, masks[0] if masks else None)

        return self._run_stripe(proj, shape, out, 1 if return_mask else 0, call)

    def remove_all_stripe(self, proj, snr=3.0, la_size=61, sm_size=21, out=None, max_scratch_bytes=None, return_mask=False):
        """Dead stripes, large stripes (window la_size) and the sorting pass (window sm_size) in one call, chunk by chunk on one scratch.
        Conventions as remove_large_stripe; return_mask=True: (result, dead mask, large mask)."""
        shape, snr, budget = _check_stripe_args(proj, snr, out, max_scratch_bytes, _prep_lib.MIN_DEAD_NPROJ, "remove_all_stripe")
        n, nx, nz = shape
        la_size, sm_size = _check_window(la_size, nx, "la_size"), _check_window(sm_size, nx, "sm_size")

        def call(d_in, d_out, masks):
            self.handle.stripe_all(self.ctx.stream(), d_in.ptr, d_out.ptr, n, nx, nz, snr, la_size, sm_size, budget, *masks)

        return self._run_stripe(proj, shape, out, 2 if return_mask else 0, call)

    def _run_outlier(self, frames, out, info, mode, dif, two_sided, return_count):
        """Upload / allocate as the conventions say (a host input's upload is filtered in place), enqueue, download a host input's result."""
        (n, rows, cols), dtype, size, budget = info
        self._ready(frames)
        with self._staging(frames) as st:
            d_in = st.source(frames, dtype)
            res = st.dest(np.shape(frames), dtype, out, inplace=d_in)      # a host input's upload is filtered in place
            d_count = st.scratch((n,), np.uint32) if return_count else None
            self.handle.outlier(self.ctx.stream(), d_in.ptr, res.ptr, _DTYPES[dtype], n, rows, cols, size, mode, dif, two_sided, budget,
                                None if d_count is None else d_count.ptr)
            counts = d_count.download().astype(np.int64) if return_count else None
            result = st.result(res, shape=np.shape(frames))
        return (result, counts) if return_count else result

    def remove_outlier(self, frames, dif, size=3, two_sided=False, out=None, max_scratch_bytes=None, return_count=False):
        """Zinger removal (module docstring) of frames [n][rows][cols] or [rows][cols], uint16 or float32: a pixel that exceeds the
        size x size median of its neighbourhood by dif or more (two_sided: or falls below it by as much) becomes that median.  Host in:
        an ndarray out.  Device in: the result goes to `out` (a DeviceArray of the same dtype and size; `out=frames` works in place) or
        a new DeviceArray.  return_count=True: (result, int64 array of the pixels replaced per frame)."""
        info = _check_outlier_args(frames, size, out, max_scratch_bytes)
        dif = _check_dif(dif)
        return self._run_outlier(frames, out, info, _prep_lib.OUTLIER, dif, bool(two_sided), return_count)

    def median_filter(self, frames, size=3, out=None, max_scratch_bytes=None):
        """The size x size median filter (module docstring; scipy.ndimage.median_filter(mode='reflect') per frame on finite data) of
        frames [n][rows][cols] or [rows][cols], uint16 or float32.  Conventions as remove_outlier."""
        info = _check_outlier_args(frames, size, out, max_scratch_bytes)
        return self._run_outlier(frames, out, info, _prep_lib.MEDIAN2D, 0.0, False, False)

    def _ready_phase(self, like):
        self._ready_ctx(like)
        if self._phase is None:
            self._phase = _phase_lib.PhaseHandle(self.ctx.device)      # made on first use: loads hipFFT

    def _run_phase(self, proj, shape, out, call):
        """Upload / allocate as the conventions say, run call(d_in, d_out), download a host input's result."""
        self._ready_phase(proj)
        with self._staging(proj) as st:
            d_in = st.source(proj)
            res = st.dest(shape, np.float32, out, inplace=d_in)      # a host input's upload is ours: in place
            extra = call(d_in, res)
            return st.result(res), extra

    def retrieve_phase(self, proj, strength=None, *, pixel_size=None, dist=None, energy=None, wavelength=None, delta_beta=None, pad=None,
                       minus_log=True, min_ratio=1e-6, out=None, max_scratch_bytes=None, timed=False):
        """Paganin phase retrieval of the transmission proj [n_proj][nx][nz] (float32; module docstring), what
        normalize(minus_log=False) returns.  Give either `strength` (pixels^2) or the physical quantities of paganin_strength
        (pixel_size, dist, one of energy / wavelength, optionally delta_beta), not both.  pad: values of edge replication on each side
        of both axes (default from the strength).  Host in: an ndarray out.  Device in: the result goes to `out` (a float32 DeviceArray
        of the same size; `out=proj` works in place) or a new DeviceArray.  Limits: a padded axis of at most 8192 values where
        strength > 0 (PrepUnsupported), 0 <= strength <= 1e12.  timed=True (benchmarks): returns (result, (pad_ms, r2c_ms, filter_ms, c2r_ms,
        crop_ms))."""
        shape = _float32_stack(proj)
        n, nx, nz = shape
        physical = dict(pixel_size=pixel_size, dist=dist, energy=energy, wavelength=wavelength, delta_beta=delta_beta)
        given = [k for k, v in physical.items() if v is not None]
        if strength is not None:
            if given:
                raise ValueError("give either strength or the physical quantities (%s), not both" % ", ".join(given))
            try:
                strength = float(strength)
            except (TypeError, ValueError):
                raise ValueError("strength must be a number, got %r" % (strength,))
        else:
            if pixel_size is None or dist is None:
                raise ValueError("give strength, or pixel_size, dist and one of energy / wavelength")
            strength = paganin_strength(pixel_size, dist, energy=energy, wavelength=wavelength,
                                        delta_beta=1000.0 if delta_beta is None else delta_beta)
        if not (math.isfinite(strength) and 0 <= strength <= _phase_lib.MAX_STRENGTH):
            raise ValueError("strength must be in 0 ... 1e12 pixels^2, got %r" % (strength,))
        if pad is not None:
            if isinstance(pad, (bool, np.bool_)) or not isinstance(pad, (int, np.integer)) or pad < 0:
                raise ValueError("pad must be an integer >= 0 or None, got %r" % (pad,))
        _check_min_ratio(min_ratio)
        budget = DEFAULT_SCRATCH_BYTES if max_scratch_bytes is None else int(max_scratch_bytes)
        if budget < 0:
            raise ValueError("max_scratch_bytes must be >= 0 (0: no limit)")
        _check_out(proj, out, n * nx * nz)
        (mx, px), (mz, pz) = phase_padding(nx, strength, pad), phase_padding(nz, strength, pad)
        if strength > 0 and max(px, pz) > _phase_lib.MAX_P:             # a = 0 pads and transforms nothing
            raise PrepUnsupported("retrieve_phase: the padded frame %d x %d (pad %d, %d) exceeds %d values on an axis"
                                  % (px, pz, mx, mz, _phase_lib.MAX_P))

        def call(d_in, d_out):
            return self._phase.retrieve(self.ctx.stream(), d_in.ptr, d_out.ptr, n, nx, nz, strength, mx, mz, minus_log, min_ratio, budget,
                                        timed)

        result, ms = self._run_phase(proj, shape, out, call)
        return (result, ms) if timed else result

    def minus_log(self, proj, min_ratio=1e-6, out=None):
        """-log(fmax(proj, min_ratio)) of a float32 stack [n_proj][nx][nz]: the last step of retrieve_phase alone, for pipelines that
        skip the retrieval.  Host in: an ndarray out; device in: `out` (may be proj) or a new DeviceArray."""
        shape = _float32_stack(proj)
        _check_min_ratio(min_ratio)
        size = int(np.prod(shape))
        _check_out(proj, out, size)

        def call(d_in, d_out):
            self._phase.minus_log(self.ctx.stream(), d_in.ptr, d_out.ptr, size, min_ratio)

        return self._run_phase(proj, shape, out, call)[0]


def reference_frames(flats, darks, method="mean", ctx=None):
    """(flat, dark) float32 reference frames: Preprocessor.reference_frames on a handle of its own."""
    with Preprocessor(ctx) as p:
        return p.reference_frames(flats, darks, method)


def normalize(frames, flats, darks, cutoff=None, minus_log=True, min_ratio=1e-6, method="mean", crop=None, ctx=None, out=None):
    """The (n_proj, nx, nz) sinogram of raw frames: Preprocessor.normalize on a handle of its own."""
    with Preprocessor(ctx) as p:
        return p.normalize(frames, flats, darks, cutoff=cutoff, minus_log=minus_log, min_ratio=min_ratio, method=method, crop=crop, out=out)


def eigen_flats(flats, darks, n_eff=None, eig_ratio=2.0, ctx=None):
    """The EigenFlats of the stacks flats and darks: Preprocessor.eigen_flats on a handle of its own.  Its buffers belong to ctx (without
    one: to the context of device flats), which must outlive them."""
    if ctx is None and not _is_dev(flats):
        raise ValueError("eigen_flats: the EigenFlats lives on the device, so host flats need a ctx that outlives it")
    with Preprocessor(ctx) as p:
        return p.eigen_flats(flats, darks, n_eff=n_eff, eig_ratio=eig_ratio)


def normalize_dynamic(frames, flats, darks=None, n_eff=None, eig_ratio=2.0, bin=2, tv_eps=1e-3, w_max=10.0, weights=None, cutoff=None,
                      minus_log=True, min_ratio=1e-6, crop=None, ctx=None, out=None, max_scratch_bytes=None, return_weights=False):
    """The sinogram of raw frames with a flat per projection: Preprocessor.normalize_dynamic on a handle of its own."""
    if ctx is None and isinstance(flats, EigenFlats) and flats.flat is not None:
        ctx = flats.flat.ctx
    with Preprocessor(ctx) as p:
        return p.normalize_dynamic(frames, flats, darks, n_eff=n_eff, eig_ratio=eig_ratio, bin=bin, tv_eps=tv_eps, w_max=w_max, weights=weights,
                                   cutoff=cutoff, minus_log=minus_log, min_ratio=min_ratio, crop=crop, out=out,
                                   max_scratch_bytes=max_scratch_bytes, return_weights=return_weights)


def remove_outlier(frames, dif, size=3, two_sided=False, ctx=None, out=None, max_scratch_bytes=None, return_count=False):
    """Zinger removal: Preprocessor.remove_outlier on a handle of its own."""
    with Preprocessor(ctx) as p:
        return p.remove_outlier(frames, dif, size=size, two_sided=two_sided, out=out, max_scratch_bytes=max_scratch_bytes,
                                return_count=return_count)


def median_filter(frames, size=3, ctx=None, out=None, max_scratch_bytes=None):
    """The 2-D median filter: Preprocessor.median_filter on a handle of its own."""
    with Preprocessor(ctx) as p:
        return p.median_filter(frames, size=size, out=out, max_scratch_bytes=max_scratch_bytes)


def remove_stripe_sorting(proj, size=21, ctx=None, out=None, max_scratch_bytes=None):
    """Sorting-based stripe removal: Preprocessor.remove_stripe_sorting on a handle of its own."""
    with Preprocessor(ctx) as p:
        return p.remove_stripe_sorting(proj, size=size, out=out, max_scratch_bytes=max_scratch_bytes)


def remove_large_stripe(proj, snr=3.0, size=51, drop_ratio=0.1, norm=True, ctx=None, out=None, max_scratch_bytes=None, return_mask=False):
    """Large-stripe removal: Preprocessor.remove_large_stripe on a handle of its own."""
    with Preprocessor(ctx) as p:
        return p.remove_large_stripe(proj, snr=snr, size=size, drop_ratio=drop_ratio, norm=norm, out=out,
                                     max_scratch_bytes=max_scratch_bytes, return_mask=return_mask)


def remove_dead_stripe(proj, snr=3.0, size=51, norm=True, ctx=None, out=None, max_scratch_bytes=None, return_mask=False):
    """Dead-stripe removal: Preprocessor.remove_dead_stripe on a handle of its own."""
    with Preprocessor(ctx) as p:
        return p.remove_dead_stripe(proj, snr=snr, size=size, norm=norm, out=out, max_scratch_bytes=max_scratch_bytes,
                                    return_mask=return_mask)


def remove_all_stripe(proj, snr=3.0, la_size=61, sm_size=21, ctx=None, out=None, max_scratch_bytes=None, return_mask=False):
    """Dead, large and sorting-based stripe removal: Preprocessor.remove_all_stripe on a handle of its own."""
    with Preprocessor(ctx) as p:
        return p.remove_all_stripe(proj, snr=snr, la_size=la_size, sm_size=sm_size, out=out, max_scratch_bytes=max_scratch_bytes,
                                   return_mask=return_mask)


def retrieve_phase(proj, strength=None, ctx=None, **kwargs):
    """Paganin phase retrieval: Preprocessor.retrieve_phase (same keywords) on a handle of its own."""
    with Preprocessor(ctx) as p:
        return p.retrieve_phase(proj, strength, **kwargs)


def minus_log(proj, min_ratio=1e-6, ctx=None, out=None):
    """-log(fmax(proj, min_ratio)): Preprocessor.minus_log on a handle of its own."""
    with Preprocessor(ctx) as p:
        return p.minus_log(proj, min_ratio=min_ratio, out=out)
