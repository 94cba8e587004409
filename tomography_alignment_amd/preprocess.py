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

The kernels live in their own library, like libtomo_fbp.so and libtomo_xcorr.so, so that the projector's sources and the kernel-source
hash that keys the committed PMC counters do not change.  Host arrays and _lib.DeviceArrays are both accepted; a device input gives a
device output, with no host round trip, and every temporary buffer is freed before a call returns.  Arguments are checked (ValueError)
before anything is uploaded or launched.
"""
import math

import numpy as np

from . import _phase_lib, _prep_lib
from ._ops import HandleOwner, _is_dev
from ._prep_lib import PrepUnsupported  # noqa: F401  (re-exported)

DEFAULT_SCRATCH_BYTES = 2 << 30
METHODS = {"mean": _prep_lib.MEAN, "median": _prep_lib.MEDIAN}
_DTYPES = {np.dtype(np.uint16): _prep_lib.U16, np.dtype(np.float32): _prep_lib.F32}


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


class Preprocessor(HandleOwner):
    """One libtomo_prep handle and its scratch, reused across calls.  ctx: the _lib.Context whose device and stream the work uses (work
    is enqueued on ctx.stream(), in order with the projector work that follows); default the context of the first DeviceArray passed in,
    or a context of the handle's own.  Arguments are checked before the context or the handle is made."""

    def __init__(self, ctx=None):
        HandleOwner.__init__(self, ctx)
        self._phase = None

    def _new_handle(self):
        return _prep_lib.PrepHandle(self.ctx.device)

    def close(self):
        if self._phase is not None:
            self._phase.close()
            self._phase = None
        HandleOwner.close(self)

    def _upload(self, a, temps):
        if _is_dev(a):
            return a
        a = np.ascontiguousarray(a)
        d = self.ctx.to_device(a, a.dtype)
        temps.append(d)
        return d

    @staticmethod
    def _free(temps):
        for t in temps:
            t.free()
        del temps[:]

    def _reference(self, d, shape, dtype, method):
        n = 1 if len(shape) == 2 else shape[0]
        rows, cols = shape[-2:]
        out = self.ctx.empty((rows, cols), np.float32)
        try:
            self.handle.reference(self.ctx.stream(), d.ptr, _DTYPES[dtype], n, rows, cols, METHODS[method], out.ptr)
        except Exception:
            out.free()
            raise
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
        temps, res = [], []
        try:
            for a, (shape, dtype) in zip((flats, darks), infos):
                res.append(self._reference(self._upload(a, temps), shape, dtype, method))
        except Exception:
            self._free(res)
            raise
        finally:
            self._free(temps)
        if _is_dev(flats):
            return tuple(res)
        out = tuple(r.download() for r in res)
        self._free(res)
        return out

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
        temps = []
        try:
            d_raw = self._upload(frames, temps)
            d_flat, d_dark = (self._reference(self._upload(a, temps), s, dt, method) for a, (s, dt) in zip((flats, darks), infos))
            temps += [d_flat, d_dark]
            res = out if out is not None else self.ctx.empty(oshape, np.float32)
            if out is None and not _is_dev(frames):
                temps.append(res)
            self.handle.normalize(self.ctx.stream(), d_raw.ptr, _DTYPES[dtype], n, rows, cols, d_flat.ptr, d_dark.ptr,
                                  ((z0, z1), (x0, x1)), cutoff, minus_log, min_ratio, res.ptr)
            return res if _is_dev(frames) else res.download()
        finally:
            self._free(temps)

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
        temps = []
        try:
            d_in = self._upload(proj, temps)
            res = out
            if res is None:
                res = self.ctx.empty(shape, np.float32)
                if not _is_dev(proj):
                    temps.append(res)
            try:
                ms = self.handle.stripe_sorting(self.ctx.stream(), d_in.ptr, res.ptr, n, nx, nz, size, budget, timed)
            except Exception:
                if out is None:
                    res.free()
                raise
            result = res if _is_dev(proj) else res.download()
        finally:
            self._free(temps)
        return (result, ms) if timed else result

    def _run_stripe(self, proj, shape, out, n_masks, call):
        """Upload / allocate as remove_stripe_sorting does, run call(d_in, d_out, masks) with n_masks zeroed uint8 (nx, nz) device
        buffers, and return (result, mask, ...) with the masks as boolean ndarrays."""
        self._ready(proj)
        temps = []
        try:
            d_in = self._upload(proj, temps)
            res = out
            if res is None:
                res = self.ctx.empty(shape, np.float32)
                if not _is_dev(proj):
                    temps.append(res)
            try:
                masks = []
                for _ in range(n_masks):
                    masks.append(self.ctx.zeros(shape[1:], np.uint8))
                    temps.append(masks[-1])
                call(d_in, res, [m.ptr for m in masks])
                host_masks = tuple(m.download().astype(bool) for m in masks)
            except Exception:
                if out is None and _is_dev(proj):
                    res.free()
                raise
            result = res if _is_dev(proj) else res.download()
        finally:
            self._free(temps)
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
        temps = []
        try:
            d_in = self._upload(frames, temps)
            res = out
            if res is None:
                res = d_in if not _is_dev(frames) else self.ctx.empty(tuple(frames.shape), dtype)
            try:
                d_count = None
                if return_count:
                    d_count = self.ctx.empty((n,), np.uint32)
                    temps.append(d_count)
                self.handle.outlier(self.ctx.stream(), d_in.ptr, res.ptr, _DTYPES[dtype], n, rows, cols, size, mode, dif, two_sided, budget,
                                    None if d_count is None else d_count.ptr)
                counts = d_count.download().astype(np.int64) if return_count else None
            except Exception:
                if out is None and res is not d_in:
                    res.free()
                raise
            result = res if _is_dev(frames) else res.download().reshape(np.shape(frames))
        finally:
            self._free(temps)
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
        temps = []
        try:
            d_in = self._upload(proj, temps)
            res = out
            if res is None:
                res = d_in if not _is_dev(proj) else self.ctx.empty(shape, np.float32)     # a host input's upload is ours: in place
            try:
                extra = call(d_in, res)
            except Exception:
                if out is None and res is not d_in:
                    res.free()
                raise
            return (res if _is_dev(proj) else res.download()), extra
        finally:
            self._free(temps)

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
    p = Preprocessor(ctx)
    try:
        return p.reference_frames(flats, darks, method)
    finally:
        p.close()


def normalize(frames, flats, darks, cutoff=None, minus_log=True, min_ratio=1e-6, method="mean", crop=None, ctx=None, out=None):
    """The (n_proj, nx, nz) sinogram of raw frames: Preprocessor.normalize on a handle of its own."""
    p = Preprocessor(ctx)
    try:
        return p.normalize(frames, flats, darks, cutoff=cutoff, minus_log=minus_log, min_ratio=min_ratio, method=method, crop=crop, out=out)
    finally:
        p.close()


def remove_outlier(frames, dif, size=3, two_sided=False, ctx=None, out=None, max_scratch_bytes=None, return_count=False):
    """Zinger removal: Preprocessor.remove_outlier on a handle of its own."""
    p = Preprocessor(ctx)
    try:
        return p.remove_outlier(frames, dif, size=size, two_sided=two_sided, out=out, max_scratch_bytes=max_scratch_bytes,
                                return_count=return_count)
    finally:
        p.close()


def median_filter(frames, size=3, ctx=None, out=None, max_scratch_bytes=None):
    """The 2-D median filter: Preprocessor.median_filter on a handle of its own."""
    p = Preprocessor(ctx)
    try:
        return p.median_filter(frames, size=size, out=out, max_scratch_bytes=max_scratch_bytes)
    finally:
        p.close()


def remove_stripe_sorting(proj, size=21, ctx=None, out=None, max_scratch_bytes=None):
    """Sorting-based stripe removal: Preprocessor.remove_stripe_sorting on a handle of its own."""
    p = Preprocessor(ctx)
    try:
        return p.remove_stripe_sorting(proj, size=size, out=out, max_scratch_bytes=max_scratch_bytes)
    finally:
        p.close()


def remove_large_stripe(proj, snr=3.0, size=51, drop_ratio=0.1, norm=True, ctx=None, out=None, max_scratch_bytes=None, return_mask=False):
    """Large-stripe removal: Preprocessor.remove_large_stripe on a handle of its own."""
    p = Preprocessor(ctx)
    try:
        return p.remove_large_stripe(proj, snr=snr, size=size, drop_ratio=drop_ratio, norm=norm, out=out,
                                     max_scratch_bytes=max_scratch_bytes, return_mask=return_mask)
    finally:
        p.close()


def remove_dead_stripe(proj, snr=3.0, size=51, norm=True, ctx=None, out=None, max_scratch_bytes=None, return_mask=False):
    """Dead-stripe removal: Preprocessor.remove_dead_stripe on a handle of its own."""
    p = Preprocessor(ctx)
    try:
        return p.remove_dead_stripe(proj, snr=snr, size=size, norm=norm, out=out, max_scratch_bytes=max_scratch_bytes,
                                    return_mask=return_mask)
    finally:
        p.close()


def remove_all_stripe(proj, snr=3.0, la_size=61, sm_size=21, ctx=None, out=None, max_scratch_bytes=None, return_mask=False):
    """Dead, large and sorting-based stripe removal: Preprocessor.remove_all_stripe on a handle of its own."""
    p = Preprocessor(ctx)
    try:
        return p.remove_all_stripe(proj, snr=snr, la_size=la_size, sm_size=sm_size, out=out, max_scratch_bytes=max_scratch_bytes,
                                   return_mask=return_mask)
    finally:
        p.close()


def retrieve_phase(proj, strength=None, ctx=None, **kwargs):
    """Paganin phase retrieval: Preprocessor.retrieve_phase (same keywords) on a handle of its own."""
    p = Preprocessor(ctx)
    try:
        return p.retrieve_phase(proj, strength, **kwargs)
    finally:
        p.close()


def minus_log(proj, min_ratio=1e-6, ctx=None, out=None):
    """-log(fmax(proj, min_ratio)): Preprocessor.minus_log on a handle of its own."""
    p = Preprocessor(ctx)
    try:
        return p.minus_log(proj, min_ratio=min_ratio, out=out)
    finally:
        p.close()
