"""
Volume post-processing on the GPU (libtomo_vol.so, include/tomo_vol.h): what every user does to a reconstruction next, done where it
lies in HBM instead of in numpy behind a 4-bytes-per-voxel download.

    statistics(vol, region)                     -> VolumeStats (counts, min, max, float64 sum and sumsq, mean, std)
    histogram(vol, bins, range, region)         -> Histogram (counts, under, over, nonfinite, edges, window(p_lo, p_hi))
    circular_mask(vol, ratio, value, out)       -> the volume with `value` outside the reconstruction cylinder
    quantize(vol, window, dtype, order, ...)    -> uint8 / uint16 codes, in the volume's layout ("xyz") or as the stack of z slices ("zyx")
    project(vol, axis, op), slice(vol, axis, i) -> maximum / minimum projections and single planes
    export_stack(vol, directory, ...)           -> statistics, histogram, percentile window, transposed quantize, ONE download of the
                                                   codes; slice_%05d.npy, meta.json and float32 previews

vol is v[nx][ny][nz], float32, z fastest (any 3-D float32 array qualifies): a numpy array or a _lib.DeviceArray (a flat one with
shape=).  Device in gives device out.  region: None (everything), "cylinder" or ("cylinder", ratio): voxel (x, y, .) is inside iff
(2x - nx + 1)^2 + (2y - ny + 1)^2 <= floor((ratio min(nx, ny))^2), in integers.  The definitions are exact (tests/vol_model.py is the
same in numpy); the sums of statistics are taken in an order that depends on the shape only, so the same input gives the same bits.

The module-level functions make a temporary PostProcessor; keep one to reuse its handle.  No CPU fallback.
"""
import json
import math
import os

import numpy as np

from . import _lib, _ops, _vol_lib
from ._vol_lib import VolUnsupported  # noqa: F401  (part of this module's interface)

MAX_BINS = _vol_lib.MAX_BINS
_DTYPES = {np.dtype(np.uint8): 8, np.dtype(np.uint16): 16}
_ORDERS = {"xyz": 0, "zyx": 1}
_OPS = {"max": 0, "min": 1}
_STAGE_BYTES = 64 << 20          # of the host array export_stack downloads the codes through


class VolumeStats(object):
    """n_finite, n_nonfinite, min, max (float32; NaN without finite values), sum, sumsq (float64, of the finite values), mean, std."""

    def __init__(self, n_finite, n_nonfinite, vmin, vmax, vsum, sumsq):
        self.n_finite, self.n_nonfinite = int(n_finite), int(n_nonfinite)
        self.min, self.max = np.float32(vmin), np.float32(vmax)
        self.sum, self.sumsq = float(vsum), float(sumsq)

    @property
    def mean(self):
        return self.sum / self.n_finite if self.n_finite else float("nan")

    @property
    def std(self):
        if not self.n_finite:
            return float("nan")
        return math.sqrt(max(self.sumsq / self.n_finite - self.mean ** 2, 0.0))

    def as_dict(self):
        return {"n_finite": self.n_finite, "n_nonfinite": self.n_nonfinite, "min": float(self.min), "max": float(self.max), "sum": self.sum,
                "sumsq": self.sumsq, "mean": self.mean, "std": self.std}

    def __repr__(self):
        return "VolumeStats(%s)" % ", ".join("%s=%r" % kv for kv in self.as_dict().items())


class Histogram(object):
    """counts (nbins,) uint64 over [lo, hi], the finite values `under` lo and `over` hi, the `nonfinite` ones; edges (nbins + 1,)
    float64."""

    def __init__(self, counts, under, over, nonfinite, lo, hi):
        self.counts = np.asarray(counts, np.uint64)
        self.under, self.over, self.nonfinite = int(under), int(over), int(nonfinite)
        self.lo, self.hi = np.float32(lo), np.float32(hi)

    @property
    def edges(self):
        n = self.counts.size
        return float(self.lo) + (float(self.hi) - float(self.lo)) * np.arange(n + 1, dtype=np.float64) / n

    def window(self, p_lo=0.1, p_hi=99.9):
        """The display window between two percentiles of the counted values, host code in float64: from the lower edge of the first bin
        whose cumulative count exceeds p_lo/100 of counts.sum() to the upper edge of the first bin whose cumulative count reaches
        p_hi/100 of it.  (lo, hi) of the histogram when it is empty."""
        if not (0.0 <= p_lo <= p_hi <= 100.0):
            raise ValueError("Histogram.window: need 0 <= p_lo <= p_hi <= 100, not %r, %r" % (p_lo, p_hi))
        cum = np.cumsum(self.counts.astype(np.float64))
        total = cum[-1] if cum.size else 0.0
        if total == 0.0:
            return float(self.lo), float(self.hi)
        edges = self.edges
        j = int(np.argmax(cum >= min(p_hi / 100.0 * total, total)))
        above = cum > p_lo / 100.0 * total
        i = int(np.argmax(above)) if above.any() else j          # p_lo = 100: no bin exceeds the total
        j = max(j, i)
        return float(edges[i]), float(edges[j + 1])


def region_r4(region, nx, ny):
    """The R4 of include/tomo_vol.h for a region: -1 for None, floor((ratio min(nx, ny))^2) for "cylinder" / ("cylinder", ratio)."""
    if region is None:
        return -1
    ratio = 1.0
    if not isinstance(region, str):
        try:
            region, ratio = region
        except (TypeError, ValueError):
            raise ValueError("postprocess: region must be None, 'cylinder' or ('cylinder', ratio), not %r" % (region,))
    if region != "cylinder" or not (np.isfinite(ratio) and ratio >= 0):
        raise ValueError("postprocess: region must be None, 'cylinder' or ('cylinder', ratio >= 0), not %r" % ((region, ratio),))
    return int(math.floor((float(ratio) * min(int(nx), int(ny))) ** 2))


def _window(window, what):
    try:
        lo, hi = window
        lo, hi = np.float32(lo), np.float32(hi)
    except (TypeError, ValueError):
        raise ValueError("%s: need a pair (lo, hi), not %r" % (what, window))
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError("%s: need finite float32 lo < hi, not %r" % (what, window))
    return lo, hi


def _shape3(vol, shape):
    return _ops.volume_shape(vol, shape, [np.float32], "postprocess", "volume")


def _axis(axis):
    if axis not in (0, 1, 2):
        raise ValueError("postprocess: axis must be 0, 1 or 2, not %r" % (axis,))
    return int(axis)


def _plane_shape(s, axis):
    return tuple(n for a, n in enumerate(s) if a != axis)


class PostProcessor(_ops.HandleOwner):
    """The operations of this module on one libtomo_vol handle (made on first use; see _ops.HandleOwner for ctx)."""

    def _new_handle(self):
        return _vol_lib.VolHandle(self.ctx.device)

    def device_bytes(self):
        return 0 if self.handle is None else self.handle.device_bytes()

    # ---- the operations: every check that needs no device comes before _ready
    def statistics(self, vol, region=None, shape=None):
        s = _shape3(vol, shape)
        r4 = region_r4(region, s[0], s[1])
        _vol_lib.check_shape(*s)
        self._ready(vol)
        with self._staging(vol) as st:
            r = self.handle.stats(self.ctx.stream(), st.source(vol).ptr, s[0], s[1], s[2], r4)
        return VolumeStats(r.n_finite, r.n_nonfinite, r.min, r.max, r.sum, r.sumsq)

    def histogram(self, vol, bins=4096, range=None, region=None, shape=None):
        s = _shape3(vol, shape)
        r4 = region_r4(region, s[0], s[1])
        if int(bins) != bins or not (1 <= int(bins) <= MAX_BINS):
            raise ValueError("histogram: bins must be an integer in 1 ... %d, not %r" % (MAX_BINS, bins))
        if range is not None:
            lo, hi = _window(range, "histogram: range")
        _vol_lib.check_shape(*s)
        self._ready(vol)
        with self._staging(vol) as st:
            d = st.source(vol)
            if range is None:
                r = self.handle.stats(self.ctx.stream(), d.ptr, s[0], s[1], s[2], r4)
                if r.n_finite == 0:
                    raise ValueError("histogram: the region holds no finite value to take a range from")
                lo, hi = np.float32(r.min), np.float32(r.max)
                if lo == hi:                                   # one ulp on each side, so that lo < hi
                    lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
            counts, (under, over, nonfinite) = self.handle.histogram(self.ctx.stream(), d.ptr, s[0], s[1], s[2], r4, lo, hi, int(bins))
        return Histogram(counts, under, over, nonfinite, lo, hi)

    def circular_mask(self, vol, ratio=1.0, value=0.0, out=None, shape=None):
        """`out`: None (a new array), or where the result goes -- for a device volume a DeviceArray, which may be `vol` itself (in place)."""
        s = _shape3(vol, shape)
        r4 = region_r4(("cylinder", ratio), s[0], s[1])
        dev = _ops._is_dev(vol)
        if out is not None:
            if dev != _ops._is_dev(out) or out.size != vol.size or np.dtype(out.dtype) != np.float32:
                raise ValueError("circular_mask: out must be a float32 array of the volume's kind and size")
            if not dev and not out.flags["C_CONTIGUOUS"]:
                raise ValueError("circular_mask: out must be C-contiguous")
        _vol_lib.check_shape(*s)
        self._ready(vol)
        with self._staging(vol) as st:
            d = st.source(vol)
            d_out = st.dest(s, np.float32, out, inplace=d)      # a temporary upload is masked in place
            self.handle.mask(self.ctx.stream(), d.ptr, s[0], s[1], s[2], r4, value, d_out.ptr)
            return st.result(d_out, out)

    def quantize(self, vol, window, dtype=np.uint8, order="zyx", region=None, fill=0, out=None, shape=None):
        """-> codes of `dtype`, (nx, ny, nz) for order "xyz", (nz, ny, nx) for "zyx".  `out`: a DeviceArray of that dtype and size for a
        device volume (returned), a C-contiguous numpy array for a host one."""
        s = _shape3(vol, shape)
        r4 = region_r4(region, s[0], s[1])
        lo, hi = _window(window, "quantize: window")
        try:
            bits = _DTYPES[np.dtype(dtype)]
        except (KeyError, TypeError):
            raise ValueError("quantize: dtype must be uint8 or uint16, not %r" % (dtype,))
        if order not in _ORDERS:
            raise ValueError("quantize: order must be 'xyz' or 'zyx', not %r" % (order,))
        if int(fill) != fill or not (0 <= int(fill) < (1 << bits)):
            raise ValueError("quantize: fill must be an integer in 0 ... %d, not %r" % ((1 << bits) - 1, fill))
        oshape = s if order == "xyz" else s[::-1]
        dev = _ops._is_dev(vol)
        if out is not None:
            if dev != _ops._is_dev(out) or out.size != vol.size or np.dtype(out.dtype) != np.dtype(dtype):
                raise ValueError("quantize: out must be a %s array of the volume's kind and size" % np.dtype(dtype).name)
            if not dev and not out.flags["C_CONTIGUOUS"]:
                raise ValueError("quantize: out must be C-contiguous")
        _vol_lib.check_shape(*s)
        self._ready(vol)
        with self._staging(vol) as st:
            d = st.source(vol)
            d_out = st.dest(oshape, dtype, out)
            self.handle.quantize(self.ctx.stream(), d.ptr, s[0], s[1], s[2], r4, lo, hi, bits, _ORDERS[order], int(fill), d_out.ptr)
            return st.result(d_out, out)

    def project(self, vol, axis, op="max", shape=None):
        s = _shape3(vol, shape)
        axis = _axis(axis)
        if op not in _OPS:
            raise ValueError("project: op must be 'max' or 'min', not %r" % (op,))
        _vol_lib.check_shape(*s)
        self._ready(vol)
        with self._staging(vol) as st:
            d = st.source(vol)
            d_out = st.dest(_plane_shape(s, axis), np.float32)
            self.handle.project(self.ctx.stream(), d.ptr, s[0], s[1], s[2], axis, _OPS[op], d_out.ptr)
            return st.result(d_out)

    def slice(self, vol, axis, index, shape=None):
        s = _shape3(vol, shape)
        axis = _axis(axis)
        if int(index) != index or not (0 <= int(index) < s[axis]):
            raise ValueError("slice: index %r is outside 0 ... %d of axis %d" % (index, s[axis] - 1, axis))
        _vol_lib.check_shape(*s)
        self._ready(vol)
        with self._staging(vol) as st:
            d = st.source(vol)
            d_out = st.dest(_plane_shape(s, axis), np.float32)
            self.handle.slice(self.ctx.stream(), d.ptr, s[0], s[1], s[2], axis, int(index), d_out.ptr)
            return st.result(d_out)

    def export_stack(self, vol, directory, dtype=np.uint8, percentiles=(0.1, 99.9), bins=4096, region="cylinder", previews=True, shape=None,
                     write=True):
        """Statistics and histogram of the region, the window between `percentiles` of it, the transposed quantize (fill 0 outside the
        region) and ONE download, of the codes (in runs of whole slices through a staging array of at most 64 MiB, so the host never
        holds the stack).  Writes directory/slice_%05d.npy (nz images of ny rows by nx columns), meta.json (window,
        dtype, shape, region, statistics, the histogram's counters) and, with previews, the three central planes (preview_slice_axis%d.npy)
        and the three maximum projections (preview_max_axis%d.npy) as float32.  write=False: everything but the files (timing).
        -> the meta dictionary."""
        s = _shape3(vol, shape)
        region_r4(region, s[0], s[1])
        if np.dtype(dtype) not in _DTYPES:
            raise ValueError("export_stack: dtype must be uint8 or uint16, not %r" % (dtype,))
        _vol_lib.check_shape(*s)
        self._ready(vol)
        with self._staging(vol) as whole:
            d = whole.source(vol)
            st = self.statistics(d, region, shape=s)
            if st.n_finite == 0:
                raise ValueError("export_stack: the region holds no finite value")
            hist = self.histogram(d, bins, (st.min, st.max) if st.min < st.max else None, region, shape=s)
            lo, hi = hist.window(*percentiles)
            lo, hi = np.float32(lo), np.float32(hi)
            if not lo < hi:
                lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
            if write:
                os.makedirs(directory, exist_ok=True)
            with self._staging(d) as codes:                     # the codes go before the previews are made
                d_codes = self.quantize(d, (lo, hi), dtype, "zyx", region, 0, codes.scratch(s[::-1], dtype), shape=s)
                plane = s[0] * s[1]                             # the one download, through a bounded staging array that is touched once
                step = max(1, min(s[2], _STAGE_BYTES // (plane * np.dtype(dtype).itemsize)))
                stage = np.empty((step, s[1], s[0]), dtype)
                for z0 in range(0, s[2], step):
                    k = min(step, s[2] - z0)
                    d_codes.view(z0 * plane, k * plane).download(stage[:k])
                    if write:
                        for z in range(k):
                            np.save(os.path.join(directory, "slice_%05d.npy" % (z0 + z)), stage[z])
            pre = {}
            if previews:
                for a in range(3):
                    for name, d_p in (("preview_slice_axis%d" % a, self.slice(d, a, s[a] // 2, shape=s)),
                                      ("preview_max_axis%d" % a, self.project(d, a, "max", shape=s))):
                        pre[name] = d_p.download()
                        d_p.free()                              # a plane at a time: slice and project take no `out`
        meta = {"window": [float(lo), float(hi)], "dtype": np.dtype(dtype).name, "shape": list(s), "stack_shape": list(s[::-1]),
                "region": None if region is None else (["cylinder", 1.0] if isinstance(region, str) else [region[0], float(region[1])]),
                "percentiles": [float(p) for p in percentiles], "bins": int(bins), "statistics": st.as_dict(),
                "histogram": {"lo": float(hist.lo), "hi": float(hist.hi), "under": hist.under, "over": hist.over, "nonfinite": hist.nonfinite,
                              "counted": int(hist.counts.sum())},
                "previews": sorted(pre)}
        if write:
            for name, image in pre.items():
                np.save(os.path.join(directory, name + ".npy"), image)
            with open(os.path.join(directory, "meta.json"), "w") as f:
                json.dump(meta, f, indent=1)
        return meta


def statistics(vol, region=None, ctx=None, shape=None):
    with PostProcessor(ctx) as p:                            # without a ctx: a device volume's (_ops.HandleOwner)
        return p.statistics(vol, region, shape=shape)


def histogram(vol, bins=4096, range=None, region=None, ctx=None, shape=None):
    with PostProcessor(ctx) as p:
        return p.histogram(vol, bins, range, region, shape=shape)


def circular_mask(vol, ratio=1.0, value=0.0, out=None, ctx=None, shape=None):
    with PostProcessor(ctx) as p:
        return p.circular_mask(vol, ratio, value, out, shape=shape)


def quantize(vol, window, dtype=np.uint8, order="zyx", region=None, fill=0, out=None, ctx=None, shape=None):
    with PostProcessor(ctx) as p:
        return p.quantize(vol, window, dtype, order, region, fill, out, shape=shape)


def project(vol, axis, op="max", ctx=None, shape=None):
    with PostProcessor(ctx) as p:
        return p.project(vol, axis, op, shape=shape)


def slice(vol, axis, index, ctx=None, shape=None):      # noqa: A001  (the builtin is not used in this module)
    with PostProcessor(ctx) as p:
        return p.slice(vol, axis, index, shape=shape)


def export_stack(vol, directory, dtype=np.uint8, percentiles=(0.1, 99.9), bins=4096, region="cylinder", previews=True, ctx=None, shape=None):
    with PostProcessor(ctx) as p:
        return p.export_stack(vol, directory, dtype, percentiles, bins, region, previews, shape=shape)
