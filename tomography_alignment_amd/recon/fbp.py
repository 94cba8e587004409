"""
Filtered back-projection (FBP) for the parallel-beam geometry of utilities/geometry.py: one ramp-filter pass over the sinogram
(libtomo_fbp.so, include/tomo_fbp.h) and one back-projection through the exact adjoint of the projector (tomo_adjoint), so every
per-projection pose -- phi, alpha, beta, x/y/z shift, cor_x -- that SIRT and the alignment use is followed as it is.

Filter, per projection and detector row z (sinogram p[ip][ix][iz], iz fastest; the filter runs along ix):

    Npad = max(64, next power of two >= 2 ndx); the column is zero-padded to Npad
    h[k] = 1/4 (m == 0), -1/(pi m)^2 (m odd), 0 (m even),  m = k (k < Npad/2) else k - Npad     Ram-Lak, Kak & Slaney (3.29)
    H[j] = Re(DFT(h))[j] * W(f_j),  f_j = fftfreq(Npad)[j]                                       filter_response()
    q[ip, x, z] = s[ip] * IDFT(H . DFT(pad(p[ip, :, z])))[x],  x < ndx

FBP = A^T q with s[ip] = w[ip] * dz * step^2 / (vx vy vz): w the angle weights (angle_weights()), dz the detector pitch along z,
step the ray sampling step, v the voxel pitches.  Why: the forward sums samples, so p = line integral / step; per angle A^T spreads a
detector value over the voxels at a density of 1 / (dx dz step) samples per unit volume, i.e. A^T ~ interpolation * (vx vy vz) /
(dx dz step); the ramp filter of a sampled projection carries 1 / dx; dx cancels.  For the unit geometry (pitches 1, step 1) s = w.
The scale is folded into the filter's output write, so the adjoint's result is the FBP with no extra pass over the volume.

Tilted poses (alpha, beta != 0) take the adjoint's tilted kernels (about 5x slower than the untilted ones), and a ramp filter along
detector x is then only an approximation of the exact inversion.  Neither is special-cased.
"""
import numpy as np

try:
    from ..utilities import projection_operators
except ImportError:      # imported as top-level `recon` (package directory on sys.path, like the reference tree)
    from utilities import projection_operators

MAX_NDX = 4096           # Npad <= 8192: the largest FFT the kernel holds in LDS (include/tomo_fbp.h)

_WINDOWS = {
    "ramp": lambda f: np.ones_like(f),
    "shepp-logan": lambda f: np.sinc(f),                       # sin(pi f) / (pi f), 1 at 0
    "cosine": lambda f: np.cos(np.pi * f),
    "hamming": lambda f: 0.54 + 0.46 * np.cos(2 * np.pi * f),
    "hann": lambda f: 0.5 + 0.5 * np.cos(2 * np.pi * f),
}
FILTERS = tuple(_WINDOWS)


def padded_length(ndx):
    """Npad = max(64, smallest power of two >= 2 ndx), in integers as the library's log2_npad computes it: the response table handed to
    tomo_fbp_set_response must hold exactly Npad/2 + 1 values."""
    ndx = int(ndx)
    if ndx < 1:
        raise ValueError("padded_length: ndx must be >= 1")
    return max(64, 1 << (2 * ndx - 1).bit_length())


def ramlak_kernel(npad):
    """The spatial Ram-Lak kernel h on the circular grid of npad points (float64)."""
    k = np.arange(npad)
    m = np.where(k < npad // 2, k, k - npad)
    h = np.zeros(npad)
    h[m == 0] = 0.25
    odd = (m % 2) != 0
    h[odd] = -1.0 / (np.pi * m[odd]) ** 2
    return h


def window(filter, f):
    """W(f) of the named window; raises ValueError for an unknown name."""
    if filter not in _WINDOWS:
        raise ValueError("unknown FBP filter %r; choose one of %s" % (filter, ", ".join(FILTERS)))
    return _WINDOWS[filter](np.asarray(f, np.float64))


def filter_response(ndx, filter="ramp"):
    """H[j] for j = 0 .. Npad/2 (float64): the real DFT of the Ram-Lak kernel times the window.  H is even, H[Npad - j] = H[j]."""
    window(filter, 0.0)                 # the name is checked before anything else
    npad = padded_length(ndx)
    H = np.real(np.fft.fft(ramlak_kernel(npad)))[:npad // 2 + 1]
    f = np.fft.fftfreq(npad)[:npad // 2 + 1]
    return H * window(filter, f)


def angle_weights(phi):
    """Weight of each projection angle in the FBP sum (float64, sums to pi): the angles are folded mod pi and stably sorted; each gets
    half the sum of the gaps to its circular neighbours, (theta_next - theta_prev) mod pi / 2.  pi/n each for n equispaced angles over
    [0, pi) or [0, 2 pi); for the endpoint-inclusive linspace(0, pi, n) Delta inside and Delta/2 at each end.  (Computed from the gaps
    themselves, so that one or two angles get pi and pi/2 each, where the difference mod pi would give 0.)"""
    phi = np.atleast_1d(np.asarray(phi, np.float64)).ravel()
    n = phi.size
    if n == 0:
        return np.zeros(0)
    th = np.mod(phi, np.pi)
    order = np.argsort(th, kind="stable")
    ts = th[order]
    gap = np.empty(n)                      # gap[i] = angle from sorted i to sorted i+1 (circularly; the last wraps through pi)
    gap[:-1] = ts[1:] - ts[:-1]
    gap[-1] = ts[0] + np.pi - ts[-1]
    ws = 0.5 * (gap + np.roll(gap, 1))
    w = np.empty(n)
    w[order] = ws
    return w


def projection_scales(geometry, weights):
    """s[ip] = w[ip] * dz * step^2 / (vx vy vz) (module docstring)."""
    dz = float(np.asarray(geometry.det_pix, np.float64).ravel()[1])
    vol = float(np.prod(np.asarray(geometry.vox_pix, np.float64).ravel()[:3]))
    return np.asarray(weights, np.float64) * dz * float(geometry.step_size) ** 2 / vol


def filter_projections(handle, stream, d_in, n_proj, ndx, ndz, scales, d_out=None):
    """q = s * filter(p) on the device: d_in (n_proj * ndx * ndz float32 DeviceArray) filtered into d_out, or in place when d_out is
    None or d_in itself.  `handle`: an _fbp_lib.FbpHandle whose response is set for ndx; `stream`: the tomo context's compute stream
    (_lib.Context.stream()) -- the filter is ordered with everything else the context runs.  Returns the output buffer."""
    out = d_in if d_out is None else d_out
    n = int(n_proj) * int(ndx) * int(ndz)
    if d_in.size != n or out.size != n:
        raise ValueError("filter_projections: buffers must hold n_proj * ndx * ndz = %d values" % n)
    handle.filter(stream, d_in.ptr, out.ptr, int(n_proj), int(ndx), int(ndz), scales)
    return out


class FBP(object):
    """Filtered back-projection with the constructor of recon/sirt.py's SIRT: angles (n_proj, 3) rows phi, alpha, beta; xyz_shifts
    (n_proj, 3); geometry.cor_shift is followed as by every operator of the package.

    options: filter ('ramp' | 'shepp-logan' | 'cosine' | 'hamming' | 'hann'; default 'ramp'), angle_weights (n_proj weights that
    replace angle_weights(phi)), ground_truth (-> self.rms_error = ||gt - rec|| / ||gt||), _backend (a HipBackend) and
    overwrite_projections (filter a device-resident sinogram in place instead of into a buffer of its own: one sinogram less of HBM,
    the caller's projections are then the filtered ones) and download (default True; False: run() leaves the volume in self.d_rec and
    returns None instead of copying it to the host).  Projections and the ground truth may be DeviceArrays."""

    def __init__(self, geometry, projections, angles, xyz_shifts, options={}):
        self.geometry = geometry
        self.projections = projections
        self.angles = np.asarray(angles, np.float64).reshape(-1, 3)
        self.xyz_shifts = xyz_shifts
        self.n_proj = self.angles.shape[0]
        self.filter = options.get('filter', 'ramp')
        self.response = filter_response(int(geometry.det_shape[0]), self.filter)      # raises on a bad name before any launch
        w = options.get('angle_weights')
        self.weights = angle_weights(self.angles[:, 0]) if w is None else np.asarray(w, np.float64).ravel()
        if self.weights.size != self.n_proj:
            raise ValueError("FBP: angle_weights must hold one weight per projection (%d)" % self.n_proj)
        self.ground_truth = options.get('ground_truth')
        self.overwrite_projections = bool(options.get('overwrite_projections', False))
        self.download = bool(options.get('download', True))
        self._backend = options.get('_backend')
        self.rms_error = None
        self.d_rec = None
        self._initialize()

    # ---- hooks the sharded subclass overrides
    def _my_rows(self):
        return np.arange(self.n_proj)

    def _local_geometry(self, rows):
        return self.geometry

    def _allreduce_vol(self, buf):
        return buf

    def _initialize(self):
        from .. import _fbp_lib
        rows = self._rows = self._my_rows()
        self.f_proj_obj = projection_operators.ProjectionMatrix(self._local_geometry(rows), backend=self._backend)
        self.proj_mat = self.f_proj_obj.projection_matrix(phi=self.angles[rows, 0], alpha=self.angles[rows, 1],
                                                          beta=self.angles[rows, 2], xyz_shift=np.asarray(self.xyz_shifts).reshape(-1, 3)[rows])
        self.be = self.f_proj_obj.backend
        self.ctx = self.be.ctx
        self.handle = _fbp_lib.FbpHandle(self.ctx.device)
        self.ndx, self.ndz = (int(v) for v in self.geometry.det_shape)
        self.handle.set_response(self.ndx, self.response)
        self.scales = projection_scales(self.geometry, self.weights)[rows]

    def filtered(self):
        """This rank's rows of the filtered, scaled sinogram (a DeviceArray)."""
        be, rows = self.be, self._rows
        n = rows.size * self.ndx * self.ndz
        if be.is_buffer(self.projections):
            if self.projections.size != n:
                raise ValueError("FBP: the device projections must hold this rank's %d rows" % rows.size)
            d_in = self.projections
            if self.overwrite_projections:
                d_out = d_in
            else:
                if getattr(self, "_d_q", None) is None:
                    self._d_q = be.empty(n)           # kept for the next run()
                d_out = self._d_q
        else:
            d_in = d_out = be.upload(np.asarray(self.projections, np.float32).reshape(self.n_proj, -1)[rows])      # a copy of our own
        return filter_projections(self.handle, self.ctx.stream(), d_in, rows.size, self.ndx, self.ndz, self.scales, d_out)

    def run(self, positivity=False):
        """The FBP volume shaped vox_shape (float32); self.d_rec keeps it in HBM (SIRT(options={'rec': fbp.d_rec}) starts from it)."""
        be = self.be
        if self.d_rec is None:
            self.d_rec = be.empty(be.n_vox)
        if self._rows.size:
            self.proj_mat.T.apply(self.filtered(), self.d_rec)
        else:
            self.d_rec.zero_()                 # a rank that owns no angle (more ranks than projections) adds nothing
        self._allreduce_vol(self.d_rec)
        gt = None
        if self.ground_truth is not None:
            gt = self.ground_truth if be.is_buffer(self.ground_truth) else be.upload(np.asarray(self.ground_truth, np.float32).ravel())
        if positivity or gt is not None:
            be.acc_zero(0)
            be.clamp_err(self.d_rec, positivity, gt, slot=0)
            if gt is not None:
                err = be.acc_fetch(0)[0]
                self.rms_error = float(np.sqrt(err) / np.sqrt(be.dot(gt, gt)))
        if not self.download:
            return None
        rec = be.download(self.d_rec)
        return rec.reshape(tuple(int(v) for v in self.geometry.vox_shape))
