"""
Volume segmentation on the GPU (libtomo_seg.so, include/tomo_seg.h): threshold a reconstruction, split the result into connected
objects, count and measure them -- where the volume lies in HBM, instead of scipy.ndimage.label on one host core behind a
4-bytes-per-voxel download.

    otsu_threshold(hist, classes)                  -> classes - 1 float32 thresholds from a postprocess.Histogram (host, float64)
    threshold(vol, lo, hi, region, out)            -> uint8 mask
    label(mask, connectivity, out)                 -> (int32 labels, n): scipy.ndimage.label's numbering
    measure(labels, n, vol)                        -> Components (count, bbox, coord_sum, centroid; with vol: min, max, sum)
    remove_small(labels, n, min_size, out)         -> (labels, n_kept)
    largest(labels, n)                             -> uint8 mask of the component with the most voxels

Volumes are [nx][ny][nz], z fastest; the linear index of (x, y, z) is (x ny + y) nz + z.  An array is a numpy array or a
_lib.DeviceArray (a flat one with shape=); device in gives device out.  Every definition is exact (tests/seg_model.py is the same in
numpy): component k is the one whose smallest linear index is the k-th smallest, so the labels depend on the mask only.

The module-level functions make a temporary Segmenter; keep one to reuse its handle.  No CPU fallback.
"""
import numpy as np

from . import _ops, _seg_lib, postprocess
from ._seg_lib import SegUnsupported  # noqa: F401  (part of this module's interface)
from .postprocess import region_r4

TILE = (_seg_lib.TILE_X, _seg_lib.TILE_Y, _seg_lib.TILE_Z)


def otsu_threshold(hist, classes=2):
    """Otsu's thresholds of a postprocess.Histogram: the cuts after bins t_1 < ... < t_(classes - 1), each in 0 ... nbins - 2, that
    maximise the between-class variance of the bin index, i.e. J = sum over the classes in order of M_k M_k / W_k, with W_k the count
    and M_k the sum of index times count of the class -- both exact integers -- and the three operations in float64; an empty class
    adds 0.  Ties go to the first maximum in index order (of t_1, then t_2).  classes 2 or 3 (exhaustive over the ordered pairs).
    `under`, `over` and `nonfinite` are ignored.  -> a tuple of float32(edges[t + 1]); threshold(vol, lo=...) puts bin t + 1 above."""
    if classes not in (2, 3):
        raise ValueError("otsu_threshold: classes must be 2 or 3, not %r" % (classes,))
    c = np.asarray(hist.counts).astype(np.int64)
    nb = c.size
    if nb < classes:
        raise ValueError("otsu_threshold: %d classes need at least %d bins, not %d" % (classes, classes, nb))
    if int(c.sum()) == 0:
        raise ValueError("otsu_threshold: the histogram is empty")
    W = np.cumsum(c)                                             # W[t], M[t]: bins 0 ... t
    M = np.cumsum(c * np.arange(nb, dtype=np.int64))

    def term(m, w):
        m, w = m.astype(np.float64), w.astype(np.float64)
        return np.where(w > 0, m * m / np.where(w > 0, w, 1.0), 0.0)

    head = term(M[:nb - 1], W[:nb - 1])                          # class 0 ... t
    tail = term(M[-1] - M[:nb - 1], W[-1] - W[:nb - 1])          # class t + 1 ... nbins - 1
    if classes == 2:
        cuts = (int(np.argmax(head + tail)),)
    else:
        best, cuts = -1.0, None
        for t1 in range(nb - 2):
            j = (head[t1] + term(M[t1 + 1:nb - 1] - M[t1], W[t1 + 1:nb - 1] - W[t1])) + tail[t1 + 1:]
            k = int(np.argmax(j))
            if j[k] > best:
                best, cuts = float(j[k]), (t1, t1 + 1 + k)
    edges = hist.edges
    return tuple(np.float32(edges[t + 1]) for t in cuts)


class Components(object):
    """Tables over the components 1 ... n (entry k - 1 is component k): count int64 (n,); bbox int32 (n, 6) = xmin, xmax, ymin, ymax,
    zmin, zmax, inclusive; coord_sum int64 (n, 3); centroid = coord_sum / count in float64; with a volume min, max (float32, of the
    finite values, NaN without one) and sum (float64, of the finite values), else None."""

    def __init__(self, count, bbox, coord_sum, vmin=None, vmax=None, vsum=None):
        self.count, self.bbox, self.coord_sum = count, bbox, coord_sum
        self.min, self.max, self.sum = vmin, vmax, vsum

    @property
    def n(self):
        return int(self.count.size)

    @property
    def centroid(self):
        return self.coord_sum.astype(np.float64) / self.count.astype(np.float64)[:, None]

    def table(self, limit=None):
        """The components as a list of {"label", "count", "bbox", "centroid"}, largest first (the lower label among equals), at most
        `limit` of them."""
        order = np.argsort(-self.count, kind="stable")[:limit]
        cen = self.centroid
        return [{"label": int(k) + 1, "count": int(self.count[k]), "bbox": [int(b) for b in self.bbox[k]], "centroid": [float(v) for v in cen[k]]}
                for k in order]


_shape3 = _ops.volume_shape


def _count(n, what):
    if isinstance(n, bool) or int(n) != n or n < 0:
        raise ValueError("%s must be an integer >= 0, not %r" % (what, n))
    return int(n)


def _check_out(out, like, dtype, what):
    if out is None:
        return
    dev = _ops._is_dev(like)
    if dev != _ops._is_dev(out) or out.size != like.size or np.dtype(out.dtype) != np.dtype(dtype):
        raise ValueError("%s: out must be a %s array of the input's kind and size" % (what, np.dtype(dtype).name))
    if not dev and not out.flags["C_CONTIGUOUS"]:
        raise ValueError("%s: out must be C-contiguous" % what)


class Segmenter(_ops.HandleOwner):
    """The operations of this module on one libtomo_seg handle (made on first use; see _ops.HandleOwner for ctx).  max_scratch: the
    bytes measure's tables may take on the device (0: the library's default, 256 MiB); with more components than fit, measure makes
    several passes over the volume, with the same integer tables."""

    def __init__(self, ctx=None, max_scratch=0):
        super(Segmenter, self).__init__(ctx)
        self.max_scratch = _count(max_scratch, "Segmenter: max_scratch")
        self._pp = None

    def _new_handle(self):
        h = _seg_lib.SegHandle(self.ctx.device)
        if self.max_scratch:
            h.set_max_scratch(self.max_scratch)
        return h

    def close(self):
        if self._pp is not None:
            self._pp.close()
            self._pp = None
        super(Segmenter, self).close()

    def device_bytes(self):
        return 0 if self.handle is None else self.handle.device_bytes()

    # ---- the operations
    def otsu(self, vol, classes=2, bins=4096, range=None, region=None, shape=None):
        """otsu_threshold of the histogram of `vol` over `region`, taken on the device (postprocess.histogram)."""
        if classes not in (2, 3):
            raise ValueError("otsu: classes must be 2 or 3, not %r" % (classes,))
        _shape3(vol, shape, [np.float32], "otsu")
        self._ready_ctx(vol)
        if self._pp is None:
            self._pp = postprocess.PostProcessor(self.ctx)
        return otsu_threshold(self._pp.histogram(vol, bins, range, region, shape=shape), classes)

    def threshold(self, vol, lo=None, hi=None, region=None, out=None, shape=None):
        """uint8: 1 where the voxel is inside `region` (as in postprocess), is not NaN and lo <= v <= hi in float32, a bound that is
        None not tested; 0 otherwise.  At least one bound; a given bound is finite."""
        s = _shape3(vol, shape, [np.float32], "threshold")
        r4 = region_r4(region, s[0], s[1])
        if lo is None and hi is None:
            raise ValueError("threshold: give at least one of lo and hi")
        for name, b in (("lo", lo), ("hi", hi)):
            if b is not None and not np.isfinite(np.float32(b)):
                raise ValueError("threshold: %s must be finite in float32, not %r" % (name, b))
        _check_out(out, vol, np.uint8, "threshold")
        _seg_lib.check_shape(*s)
        self._ready(vol)
        with self._staging(vol) as st:
            d = st.source(vol)
            d_out = st.dest(s, np.uint8, out)
            self.handle.threshold(self.ctx.stream(), d.ptr, s[0], s[1], s[2], r4, None if lo is None else np.float32(lo),
                                  None if hi is None else np.float32(hi), d_out.ptr)
            return st.result(d_out, out)

    def label(self, mask, connectivity=1, out=None, shape=None):
        """-> (labels int32, n).  mask: uint8 or bool, non-zero is foreground.  connectivity 1, 2, 3: 6, 18, 26 neighbours."""
        s = _shape3(mask, shape, [np.uint8, np.bool_], "label")
        if isinstance(connectivity, bool) or connectivity not in (1, 2, 3):
            raise ValueError("label: connectivity must be 1, 2 or 3, not %r" % (connectivity,))
        _check_out(out, mask, np.int32, "label")
        _seg_lib.check_shape(*s)
        self._ready(mask)
        with self._staging(mask) as st:
            d = st.source(mask, np.uint8)
            d_out = st.dest(s, np.int32, out)
            n = self.handle.label(self.ctx.stream(), d.ptr, s[0], s[1], s[2], int(connectivity), d_out.ptr)
            return st.result(d_out, out), n

    def measure(self, labels, n, vol=None, shape=None):
        """-> Components over 1 ... n.  vol: None, or the float32 volume of the same shape and kind (host or device) as labels."""
        s = _shape3(labels, shape, [np.int32], "measure: labels")
        n = _count(n, "measure: n")
        if vol is not None:
            if _shape3(vol, shape, [np.float32], "measure: vol") != s:
                raise ValueError("measure: labels %r and vol %r differ in shape" % (s, tuple(vol.shape)))
            if _ops._is_dev(vol) != _ops._is_dev(labels):
                raise ValueError("measure: labels and vol must both be numpy arrays or both DeviceArrays")
        _seg_lib.check_shape(*s)
        if n == 0:
            e = np.zeros(0, np.float32)
            return Components(np.zeros(0, np.int64), np.zeros((0, 6), np.int32), np.zeros((0, 3), np.int64),
                              *((e, e.copy(), np.zeros(0, np.float64)) if vol is not None else ()))
        self._ready(labels)
        with self._staging(labels) as st:
            d = st.source(labels, np.int32)
            v_ptr = None if vol is None else st.source(vol).ptr
            return Components(*self.handle.measure(self.ctx.stream(), d.ptr, v_ptr, s[0], s[1], s[2], n))

    def remove_small(self, labels, n, min_size, out=None, shape=None):
        """-> (labels, n_kept): components of fewer than min_size voxels become 0, the others 1 ... n_kept in their order.  out may be
        labels itself (in place)."""
        s = _shape3(labels, shape, [np.int32], "remove_small")
        n, min_size = _count(n, "remove_small: n"), _count(min_size, "remove_small: min_size")
        _check_out(out, labels, np.int32, "remove_small")
        _seg_lib.check_shape(*s)
        self._ready(labels)
        with self._staging(labels) as st:
            d = st.source(labels, np.int32)
            d_out = st.dest(s, np.int32, out, inplace=d)         # a temporary upload: in place
            kept = self.handle.remove_small(self.ctx.stream(), d.ptr, s[0], s[1], s[2], n, min_size, d_out.ptr)
            return st.result(d_out, out, s), kept

    def largest(self, labels, n, shape=None):
        """-> the uint8 mask of the component with the most voxels, the lowest label among equals; all zeros when n = 0."""
        s = _shape3(labels, shape, [np.int32], "largest")
        n = _count(n, "largest: n")
        _seg_lib.check_shape(*s)
        self._ready(labels)
        with self._staging(labels) as st:
            d = st.source(labels, np.int32)
            d_out = st.dest(s, np.uint8)
            self.handle.largest(self.ctx.stream(), d.ptr, s[0], s[1], s[2], n, d_out.ptr)
            return st.result(d_out)


def check_shape(nx, ny, nz):
    """SegUnsupported for a volume of more than 2^31 - 1 voxels or nx, ny > 16384.  Needs no device."""
    _seg_lib.check_shape(nx, ny, nz)


def threshold(vol, lo=None, hi=None, region=None, out=None, ctx=None, shape=None):
    with Segmenter(ctx) as s:                                # without a ctx: a device array's (_ops.HandleOwner)
        return s.threshold(vol, lo, hi, region, out, shape=shape)


def label(mask, connectivity=1, out=None, ctx=None, shape=None):
    with Segmenter(ctx) as s:
        return s.label(mask, connectivity, out, shape=shape)


def measure(labels, n, vol=None, ctx=None, shape=None):
    with Segmenter(ctx) as s:
        return s.measure(labels, n, vol, shape=shape)


def remove_small(labels, n, min_size, out=None, ctx=None, shape=None):
    with Segmenter(ctx) as s:
        return s.remove_small(labels, n, min_size, out, shape=shape)


def largest(labels, n, ctx=None, shape=None):
    with Segmenter(ctx) as s:
        return s.largest(labels, n, shape=shape)
