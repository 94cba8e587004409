"""
The exact Euclidean distance transform of a mask and ball morphology on the GPU (libtomo_morph.so, include/tomo_morph.h): wall and
pore thickness, the largest inscribed sphere, cleaning a mask before it is labelled, closed porosity -- where the mask lies in HBM,
instead of scipy.ndimage.distance_transform_edt on one host core behind a download.

    distance_sq(mask, border, out)                 -> int32: the squared distance to the nearest background voxel, INF without one
    distance(mask, border, out)                    -> float32: its correctly rounded root, +inf without one
    erode(mask, r2, border_value, out)             -> uint8: the voxels whose ball of squared radius r2 lies in the foreground
    dilate(mask, r2, out)                          -> uint8: the voxels within r2 of the foreground
    open(mask, r2, border_value, out), close(...)  -> uint8: dilate(erode) and erode(dilate), one call each
    fill_holes(mask, out, return_count)            -> uint8: the mask and every background component that touches no face
    ball_r2(radius)                                -> floor(radius^2), the r2 of a ball

Volumes are [nx][ny][nz], z fastest.  A mask is uint8 or bool, non-zero is foreground; an array is a numpy array or a _lib.DeviceArray
(a flat one with shape=); device in gives device out.  border: "ignore" (only background inside the volume counts: scipy's
distance_transform_edt) or "background" (everything outside the volume is background).  border_value: what the outside counts as in an
erosion, as scipy.ndimage.binary_erosion's.  Every definition is an exact integer (tests/morph_model.py is the same in numpy).

The module-level functions make a temporary Morphology; keep one to reuse its handle.  No CPU fallback.
"""
import math

import numpy as np

from . import _morph_lib, _ops
from ._morph_lib import MorphUnsupported  # noqa: F401  (part of this module's interface)
from .segment import _check_out, _count

INF = _morph_lib.INF
_MASK = [np.uint8, np.bool_]
_shape3 = _ops.volume_shape


def ball_r2(radius):
    """floor(radius^2): the squared radius erode, dilate, open and close take for a ball of `radius` voxels."""
    r = float(radius)
    if not (math.isfinite(r) and r >= 0):
        raise ValueError("ball_r2: radius must be finite and >= 0, not %r" % (radius,))
    return int(math.floor(r * r))


def _border(border, what):
    if border not in _morph_lib.BORDERS:
        raise ValueError("%s: border must be 'ignore' or 'background', not %r" % (what, border))
    return _morph_lib.BORDERS[border]


def _border_value(v, what):
    if v not in (0, 1):
        raise ValueError("%s: border_value must be 0 or 1, not %r" % (what, v))
    return int(v)


class Morphology(_ops.HandleOwner):
    """The operations of this module on one libtomo_morph handle (made on first use; see _ops.HandleOwner for ctx).  line_limit: the
    longest line staged in LDS (0: the library's default); it changes no bit of any result."""

    def __init__(self, ctx=None, line_limit=0):
        super(Morphology, self).__init__(ctx)
        self.line_limit = _count(line_limit, "Morphology: line_limit")
        self._seg = None

    def _new_handle(self):
        h = _morph_lib.MorphHandle(self.ctx.device)
        if self.line_limit:
            h.set_line_limit(self.line_limit)
        return h

    def set_line_limit(self, n):
        self.line_limit = _count(n, "set_line_limit: n")
        if self.handle is not None:
            self.handle.set_line_limit(self.line_limit)

    def close(self):
        if self._seg is not None:
            self._seg.close()
            self._seg = None
        super(Morphology, self).close()

    def device_bytes(self):
        return 0 if self.handle is None else self.handle.device_bytes()

    # ---- the distance transform
    def _transform(self, what, mask, border, out, shape, dtype, call):
        s = _shape3(mask, shape, _MASK, what)
        b = _border(border, what)
        _check_out(out, mask, dtype, what)
        _morph_lib.check_shape(*s)
        self._ready(mask)
        with self._staging(mask) as st:
            d = st.source(mask, np.uint8)
            d_out = st.dest(s, dtype, out)
            call(self.handle)(self.ctx.stream(), d.ptr, s[0], s[1], s[2], b, d_out.ptr)
            return st.result(d_out, out)

    def distance_sq(self, mask, border="ignore", out=None, shape=None):
        """int32: 0 on the background, else the squared distance to the nearest background voxel; INF where there is none."""
        return self._transform("distance_sq", mask, border, out, shape, np.int32, lambda h: h.distance_sq)

    def distance(self, mask, border="ignore", out=None, shape=None):
        """float32: the correctly rounded root of distance_sq; +inf where there is no background."""
        return self._transform("distance", mask, border, out, shape, np.float32, lambda h: h.distance)

    def root(self, d2, out=None):
        """float32: the correctly rounded root of every int32 >= 0 of d2, INF -> +inf (the last step of distance)."""
        if np.dtype(d2.dtype) != np.int32 or d2.size < 1:
            raise ValueError("root: need a non-empty int32 array, not %s of %d" % (d2.dtype, d2.size))
        _check_out(out, d2, np.float32, "root")
        self._ready(d2)
        with self._staging(d2) as st:
            d = st.source(d2, np.int32)
            d_out = st.dest(tuple(d2.shape), np.float32, out)
            self.handle.root(self.ctx.stream(), d.ptr, d.size, d_out.ptr)
            return st.result(d_out, out)

    # ---- the ball
    def _ball(self, what, mask, r2, border_value, out, shape, call):
        s = _shape3(mask, shape, _MASK, what)
        r2 = _count(r2, what + ": r2")
        bv = _border_value(border_value, what)
        _check_out(out, mask, np.uint8, what)
        _morph_lib.check_shape(*s)
        self._ready(mask)
        with self._staging(mask) as st:
            d = st.source(mask, np.uint8)
            d_out = st.dest(s, np.uint8, out, inplace=d)         # a temporary upload: in place
            call(self.handle, self.ctx.stream(), d.ptr, s[0], s[1], s[2], r2, bv, d_out.ptr)
            return st.result(d_out, out, s)

    def erode(self, mask, r2, border_value=0, out=None, shape=None):
        """uint8: 1 iff every offset o with |o|^2 <= r2 lands on foreground, the outside counting as border_value.  out may be mask."""
        return self._ball("erode", mask, r2, border_value, out, shape, lambda h, *a: h.erode(*a))

    def dilate(self, mask, r2, out=None, shape=None):
        """uint8: 1 iff a foreground voxel lies within squared distance r2.  out may be mask."""
        return self._ball("dilate", mask, r2, 0, out, shape, lambda h, st, p, nx, ny, nz, r, bv, o: h.dilate(st, p, nx, ny, nz, r, o))

    def open(self, mask, r2, border_value=0, out=None, shape=None):
        """dilate(erode(mask, r2, border_value), r2) in one call."""
        return self._ball("open", mask, r2, border_value, out, shape, lambda h, *a: h.open(*a))

    def close_ball(self, mask, r2, border_value=0, out=None, shape=None):
        """erode(dilate(mask, r2), r2, border_value) in one call: the module's close (close() frees the handle)."""
        return self._ball("close", mask, r2, border_value, out, shape, lambda h, *a: h.close_ball(*a))

    # ---- hole filling
    def fill_holes(self, mask, out=None, return_count=False, shape=None):
        """uint8: 1 on the foreground and on every 6-connected component of the background that touches no face of the volume --
        scipy.ndimage.binary_fill_holes.  return_count: -> (filled mask, the number of voxels that were filled).  out may be mask.
        The background is labelled and measured by a segment.Segmenter on the same context; only its table comes to the host."""
        from . import segment
        s = _shape3(mask, shape, _MASK, "fill_holes")
        _check_out(out, mask, np.uint8, "fill_holes")
        _morph_lib.check_shape(*s)
        segment.check_shape(*s)
        self._ready(mask)
        if self._seg is None:
            self._seg = segment.Segmenter(self.ctx)
        nvox = s[0] * s[1] * s[2]
        with self._staging(mask) as st:
            d = st.source(mask, np.uint8)
            d_inv = st.scratch(s, np.uint8)
            stream = self.ctx.stream()
            self.handle.invert(stream, d.ptr, nvox, d_inv.ptr)
            d_labels, n = self._seg.label(d_inv, 1, shape=s)
            st.adopt(d_labels)
            comp = self._seg.measure(d_labels, n, shape=s)
            d_out = st.dest(s, np.uint8, out, inplace=d)
            self.handle.invert(stream, d_inv.ptr, nvox, d_out.ptr)           # the mask as 0 / 1
            inner = np.ones(n, bool)
            for axis in range(3):
                inner &= (comp.bbox[:, 2 * axis] > 0) & (comp.bbox[:, 2 * axis + 1] < s[axis] - 1)
            filled = int(comp.count[inner].sum())
            if filled:
                d_table = st.source(np.concatenate([[0], inner]).astype(np.uint8), np.uint8)
                self.handle.select(stream, d_labels.ptr, nvox, n, d_table.ptr, d_out.ptr)
            self.ctx.sync()                                  # the scope's arrays (inverse, labels, table) are about to be freed
            res = st.result(d_out, out, s)
        return (res, filled) if return_count else res


def check_shape(nx, ny, nz):
    """MorphUnsupported for a volume of more than 2^31 - 1 voxels or an axis above 16384.  Needs no device."""
    _morph_lib.check_shape(nx, ny, nz)


def distance_sq(mask, border="ignore", out=None, ctx=None, shape=None):
    with Morphology(ctx) as m:                               # without a ctx: a device array's (_ops.HandleOwner)
        return m.distance_sq(mask, border, out, shape=shape)


def distance(mask, border="ignore", out=None, ctx=None, shape=None):
    with Morphology(ctx) as m:
        return m.distance(mask, border, out, shape=shape)


def erode(mask, r2, border_value=0, out=None, ctx=None, shape=None):
    with Morphology(ctx) as m:
        return m.erode(mask, r2, border_value, out, shape=shape)


def dilate(mask, r2, out=None, ctx=None, shape=None):
    with Morphology(ctx) as m:
        return m.dilate(mask, r2, out, shape=shape)


def open(mask, r2, border_value=0, out=None, ctx=None, shape=None):      # noqa: A001  (the operation's name)
    with Morphology(ctx) as m:
        return m.open(mask, r2, border_value, out, shape=shape)


def close(mask, r2, border_value=0, out=None, ctx=None, shape=None):
    with Morphology(ctx) as m:
        return m.close_ball(mask, r2, border_value, out, shape=shape)


def fill_holes(mask, out=None, return_count=False, ctx=None, shape=None):
    with Morphology(ctx) as m:
        return m.fill_holes(mask, out, return_count, shape=shape)
