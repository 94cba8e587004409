"""What the user-facing classes over one side-library handle (preprocess.Preprocessor, multires.Pyramid, resolution.Resolution) share."""
from . import _lib


def _is_dev(a):
    return isinstance(a, _lib.DeviceArray)


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
