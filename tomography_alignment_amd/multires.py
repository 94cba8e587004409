"""
The device operations of a resolution pyramid (libtomo_pyr.so, include/tomo_pyr.h): binning of a sinogram and of a volume by 2, 4 or 8,
and the prolongation of a coarse reconstruction to twice its size.  examples/align_rigid.run_multires is what they are for: the first
outer iterations of the joint reconstruction and alignment run on binned data, the poses and the reconstruction are handed up.

The level convention.  A level binned by f is described IN ITS OWN UNITS: Geometry(n, [N/f]*3, ones(3), [N/f, N/f], ones(2)) -- unit
pitch, everything in level pixels (level_geometry).  utilities/geometry._cell_centres adds a fixed +0.5 that does not scale with the
pitch, so "N/f cells of pitch f" would put the cell centres 0.5 (f - 1) full-size pixels away from the centres of the bins they stand
for, on the detector and in the volume alike; the unit-pitch level's centres times f are the bin centres exactly
(tests/test_multires.py).  Between levels lengths are rescaled (translations times the ratio of the factors), angles are not.

    bin_projections   [n][nx][nz] -> [n][nx/f][nz/f]: float32(S * scale / f^2), S the float64 sum of the f x f values of a bin.  The
                      default scale is 1/f: a ray's path in level pixels is 1/f of its path in full-size pixels, so with it the level's
                      reconstruction carries the same VALUES as the full-size one -- comparable with bin_volume(ground truth), and carried
                      up by prolong_volume with scale 1.
    bin_volume        [nx][ny][nz] -> [nx/f][ny/f][nz/f]: float32(S * scale / f^3), the mean of the bin times scale.
    prolong_volume    [nx][ny][nz] -> [2nx][2ny][2nz], cell-centred trilinear interpolation: fine index i samples the coarse axis at
                      (i + 0.5) / 2 - 0.5 -- weights 3/4 and 1/4 on the two nearest coarse cells, the index clamped at both ends (the
                      outermost fine cell copies its coarse cell) -- separable, float32, times scale.

The float64 sum makes a binned value independent of the order of summation whenever the sum is exact; the kernels are bound by memory, so
it costs nothing.  Host arrays in give ndarrays out; _lib.DeviceArrays in give DeviceArrays out with no host round trip (a flat device
buffer, such as OuterLoop.d_b, needs `shape`).  Source and destination are distinct buffers.  Extents that f does not divide raise
ValueError before the library is loaded; nothing here synchronises.
"""
import numpy as np

from . import _pyr_lib
from ._ops import HandleOwner, _is_dev, shape_of
from ._pyr_lib import PyrUnsupported  # noqa: F401  (re-exported)

FACTORS = _pyr_lib.FACTORS


def _shape_of(a, shape, what, ndim):
    """The (n, nx, nz) / (nx, ny, nz) of `a`: `shape` if given (it must hold a's number of values), else a's own."""
    return shape_of(a, shape, ndim, what, nonempty=True)


def _check_factor(f, extents, what):
    if isinstance(f, (bool, np.bool_)) or int(f) != f or int(f) not in FACTORS:
        raise ValueError("the binning factor must be 2, 4 or 8, got %r" % (f,))
    f = int(f)
    for e in extents:
        if e % f:
            raise ValueError("%s: the factor %d does not divide the extent %d" % (what, f, e))
    return f


def _check_scale(scale):
    scale = float(scale)
    if not np.isfinite(scale):
        raise ValueError("scale must be finite, got %r" % (scale,))
    return scale


def level_geometry(n_proj, vox_shape, f=1):
    """The unit-pitch geometry of the level binned by f of a full-size (nx, ny, nz) volume and its (nx, nz) detector (module docstring)."""
    from .utilities import geometry
    nx, ny, nz = (int(v) for v in vox_shape)
    if f != 1:
        _check_factor(f, (nx, ny, nz), "level_geometry")
    return geometry.Geometry(int(n_proj), np.array([nx // f, ny // f, nz // f]), np.ones(3), np.array([nx // f, nz // f]), np.ones(2))


class Pyramid(HandleOwner):
    """One libtomo_pyr handle reused across calls.  ctx: the _lib.Context whose device and stream the work uses (work is enqueued on
    ctx.stream(), in order with the projector work around it); default the context of the first DeviceArray passed in, or a context of
    the handle's own.  Arguments are checked before the context or the handle is made."""

    def _new_handle(self):
        return _pyr_lib.PyrHandle(self.ctx.device)

    def _run(self, src, oshape, out, launch):
        """Upload a host source, allocate the destination unless `out` is given, launch; device in -> device out, host in -> host out."""
        n_out = int(np.prod(oshape))
        if out is not None:
            if not (_is_dev(out) and out.dtype == np.float32 and out.size == n_out):
                raise ValueError("out must be a float32 DeviceArray of %d values %s" % (n_out, oshape))
            if _is_dev(src) and src.ptr.value < out.ptr.value + out.nbytes and out.ptr.value < src.ptr.value + src.nbytes:
                raise ValueError("out must not overlap the source")
        self._ready(src)
        with self._staging(src) as st:
            d_src = st.source(src)
            res = st.dest(oshape, np.float32, out)
            launch(self.ctx.stream(), d_src.ptr, res.ptr)
            return st.result(res, shape=oshape)

    def bin_projections(self, proj, f, scale=None, out=None, shape=None):
        """The sinogram proj [n][nx][nz] binned by f within each projection (module docstring); scale None: 1 / f."""
        n, nx, nz = _shape_of(proj, shape, "proj", 3)
        f = _check_factor(f, (nx, nz), "bin_projections")
        scale = 1.0 / f if scale is None else _check_scale(scale)
        return self._run(proj, (n, nx // f, nz // f), out, lambda st, s, d: self.handle.bin_sino(st, s, n, nx, nz, f, scale, d))

    def bin_volume(self, vol, f, shape=None, scale=1.0, out=None):
        """The volume vol [nx][ny][nz] binned by f: the mean of every f x f x f bin, times scale."""
        nx, ny, nz = _shape_of(vol, shape, "vol", 3)
        f = _check_factor(f, (nx, ny, nz), "bin_volume")
        scale = _check_scale(scale)
        return self._run(vol, (nx // f, ny // f, nz // f), out, lambda st, s, d: self.handle.bin_vol(st, s, nx, ny, nz, f, scale, d))

    def prolong_volume(self, vol, shape=None, scale=1.0, out=None):
        """The coarse volume vol (of `shape` = (nx, ny, nz), needed for a flat buffer) interpolated to (2nx, 2ny, 2nz), times scale."""
        nx, ny, nz = _shape_of(vol, shape, "vol", 3)
        scale = _check_scale(scale)
        return self._run(vol, (2 * nx, 2 * ny, 2 * nz), out, lambda st, s, d: self.handle.prolong_vol(st, s, nx, ny, nz, scale, d))


def bin_projections(proj, f, scale=None, ctx=None, out=None, shape=None):
    """Pyramid.bin_projections on a handle of its own."""
    with Pyramid(ctx) as p:
        return p.bin_projections(proj, f, scale=scale, out=out, shape=shape)


def bin_volume(vol, f, shape=None, scale=1.0, ctx=None, out=None):
    """Pyramid.bin_volume on a handle of its own."""
    with Pyramid(ctx) as p:
        return p.bin_volume(vol, f, shape=shape, scale=scale, out=out)


def prolong_volume(vol, shape=None, scale=1.0, ctx=None, out=None):
    """Pyramid.prolong_volume on a handle of its own."""
    with Pyramid(ctx) as p:
        return p.prolong_volume(vol, shape=shape, scale=scale, out=out)
