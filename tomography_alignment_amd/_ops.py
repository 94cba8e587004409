"""What the user-facing classes over one side-library handle share -- preprocess.Preprocessor, postprocess.PostProcessor,
segment.Segmenter, registration.Registrar, resolution.Resolution, multires.Pyramid, half_acquisition.HalfAcquisition,
align.consistency.Consistency, rotation_axis.RotationAxis: the handle made on first use (HandleOwner), the device arrays of one call
(Staging) and the three wordings of the shape check."""
import numpy as np

from . import _lib


def _is_dev(a):
    return isinstance(a, _lib.DeviceArray)


class Staging(object):
    """The device arrays of one call: `with owner._staging(like) as st:`.  The scope owns every array it makes until the call hands it
    over, and frees what it still owns on the way out, in reverse order, whether the body returned or raised.  dev: a device call (device
    in, device out) or a host call (host in, host out), decided once."""

    def __init__(self, ctx, dev):
        self.ctx, self.dev, self._owned = ctx, bool(dev), []

    def _own(self, d):
        self._owned.append(d)
        return d

    def adopt(self, d):
        """A device array made elsewhere during the call (by another owner's operation) becomes the scope's to free."""
        return self._own(d)

    def source(self, a, dtype=np.float32):
        """A DeviceArray as it is; a host array uploaded (contiguous, of `dtype`; None: its own) as a temporary of the scope."""
        if _is_dev(a):
            return a
        a = np.ascontiguousarray(a, dtype)
        return self._own(self.ctx.to_device(a, a.dtype))

    def scratch(self, shape, dtype=np.float32, zero=False):
        return self._own((self.ctx.zeros if zero else self.ctx.empty)(shape, dtype))

    def dest(self, shape, dtype=np.float32, out=None, inplace=None):
        """Where the result goes: the caller's device `out` (never freed); for a host call `inplace`, the temporary upload of an
        operation that works in place; else a new array of the scope."""
        if _is_dev(out):
            return out
        if inplace is not None and not self.dev:
            return inplace
        return self._own(self.ctx.empty(shape, dtype))

    def result(self, d, out=None, shape=None):
        """Hand over: a device call's array leaves the scope and is returned; a host call's is downloaded -- into the host `out` if
        given, which is returned, else into a new array (of `shape` if given) -- and stays with the scope."""
        if self.dev:
            self._owned = [a for a in self._owned if a is not d]
            return d
        if out is not None:
            d.download(out)
            return out
        host = d.download()
        return host if shape is None else host.reshape(shape)

    def __enter__(self):
        return self

    def __exit__(self, etype, exc, tb):
        failed = None
        while self._owned:
            try:
                self._owned.pop().free()
            except Exception as e:      # noqa: BLE001  (the rest is still freed)
                failed = failed or e
        if failed is not None and etype is None:      # never in place of the exception already in flight
            raise failed


class HandleOwner(object):
    """A library handle made on first use on a _lib.Context: the one given, else that of the first DeviceArray passed in, else a context
    of the object's own, which close() closes with the handle.  A context manager.  A subclass gives _new_handle()."""

    def __init__(self, ctx=None):
        self.ctx = ctx
        self.handle = None
        self._own_ctx = None

    def _new_handle(self):
        raise NotImplementedError

    def _ready_ctx(self, like):
        if self.ctx is None:
            if _is_dev(like):
                self.ctx = like.ctx
            else:
                self.ctx = self._own_ctx = _lib.Context()

    def _ready(self, like):
        self._ready_ctx(like)
        if self.handle is None:
            self.handle = self._new_handle()

    def _staging(self, like):
        """The Staging of one call (after _ready): a device call iff `like` is a DeviceArray."""
        return Staging(self.ctx, _is_dev(like))

    def close(self):
        if self.handle is not None:
            self.handle.close()
            self.handle = None
        if self._own_ctx is not None:
            self._own_ctx.close()
            self._own_ctx = self.ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _own_shape(a, shape):
    own = tuple(a.shape) if _is_dev(a) else np.shape(a)
    return own, tuple(int(v) for v in (own if shape is None else shape))


def shape_of(a, shape, ndim, what, nonempty=False):
    """`shape` if given (it must hold a's number of values), else a's own, as ints; float32 on the device (resolution, registration,
    multires; nonempty: multires also refuses an empty axis)."""
    own, shape = _own_shape(a, shape)
    if len(shape) != ndim:
        raise ValueError("%s must have %d dimensions (give `shape` for a flat buffer), got shape %s" % (what, ndim, shape))
    if nonempty and any(s < 1 for s in shape):
        raise ValueError("%s must not be empty, got shape %s" % (what, shape))
    if int(np.prod(shape)) != int(np.prod(own)):
        raise ValueError("%s holds %d values, not the %d of shape %s" % (what, int(np.prod(own)), int(np.prod(shape)), shape))
    if _is_dev(a) and np.dtype(a.dtype) != np.float32:
        raise ValueError("%s must be float32 on the device, got %s" % (what, a.dtype))
    return shape


def stack_shape(proj, shape, who):
    """The (n, nx, nz) of a stack of projections (consistency, half_acquisition, rotation_axis)."""
    own, shp = _own_shape(proj, shape)
    if len(shp) != 3:
        raise ValueError("%s: proj must be (n, nx, nz) (give `shape` for a flat device buffer), got shape %s" % (who, shp))
    if int(np.prod(shp)) != int(np.prod(own)):
        raise ValueError("%s: proj holds %d values, not the %d of shape %s" % (who, int(np.prod(own)), int(np.prod(shp)), shp))
    if _is_dev(proj) and np.dtype(proj.dtype) != np.float32:
        raise ValueError("%s: proj must be float32 on the device, got %s" % (who, proj.dtype))
    return shp


def volume_shape(a, shape, dtypes, what, noun="array"):
    """The (nx, ny, nz) of a volume of one of `dtypes` (segment; postprocess, which calls it a volume)."""
    s = tuple(int(n) for n in (shape if shape is not None else a.shape))
    if len(s) != 3:
        raise ValueError("%s: need a 3-D %s [nx][ny][nz], not shape %r (a flat DeviceArray: pass shape=)" % (what, noun, s))
    if int(np.prod(s, dtype=np.int64)) != int(a.size):
        raise ValueError("%s: shape %r does not hold %d elements" % (what, s, a.size))
    if np.dtype(a.dtype) not in [np.dtype(d) for d in dtypes]:
        raise ValueError("%s: need %s, not %s" % (what, " or ".join(np.dtype(d).name for d in dtypes), a.dtype))
    return s
