"""
What the ctypes bindings of the package's native libraries share: the error class, the loader, and -- for the side libraries
(libtomo_<name>.so, symbols tomo_<name>_*, include/tomo_<name>.h) -- the return-code check and the handle base class.

A binding module (_lib, _xcorr_lib, _fbp_lib, ...) holds what is its own: LIB_PATH, SIGNATURES, its constants, its Unsupported class, a
one-line load() and the entry points of its handle.  There is NO CPU fallback anywhere: a missing library or device raises.
"""
import ctypes
import os
import threading


class TomoError(RuntimeError):
    pass


_loaded = {}                  # name -> CDLL, one per library and process
_lock = threading.Lock()


def load(name, path, signatures, prefix=None, build_dir=None):
    """Load libtomo_<name>.so from `path` and bind every symbol of `signatures` (name -> (restype, argtypes), all starting with
    `prefix`, default tomo_<name>); raises TomoError (never falls back) on failure.  build_dir: where its Makefile is, below the
    package (default csrc/<name>)."""
    prefix = prefix or "tomo_" + name
    with _lock:
        if name not in _loaded:
            if not os.path.exists(path):
                raise TomoError("libtomo_%s.so not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'` or "
                                "`make -C tomography_alignment_amd/%s`; there is no CPU fallback" % (name, path, build_dir or "csrc/" + name))
            try:
                lib = ctypes.CDLL(path)          # OSError here when a library it needs (hipFFT) cannot be found
            except OSError as e:
                raise TomoError("cannot load %s: %s" % (path, e))
            for sym, (res, args) in signatures.items():
                fn = getattr(lib, sym)           # AttributeError if the header and the .so disagree
                fn.restype = res
                fn.argtypes = args
            if getattr(lib, prefix + "_abi_version")() != 1:
                raise TomoError("libtomo_%s.so ABI version mismatch" % name)
            _loaded[name] = lib
    return _loaded[name]


def check(lib, name, rc, h=None, errors={}):
    """Raise for a nonzero return code of libtomo_<name>.so with the text the library kept on the handle h (None: for this thread):
    errors[rc] if the library's binding maps that code to a class of its own, TomoError otherwise."""
    if rc != 0:
        msg = (getattr(lib, "tomo_%s_last_error" % name)(h) or b"").decode(errors="replace")
        raise errors.get(rc, TomoError)("libtomo_%s error %d: %s" % (name, rc, msg))


def _ptr(p):
    """A device pointer or stream argument: a c_void_p as it is, an int as one, 0 / None as NULL."""
    if isinstance(p, ctypes.c_void_p):
        return p
    return ctypes.c_void_p(int(p)) if p else None


class Handle(object):
    """One tomo_<NAME> handle of a side library: tomo_<NAME>_create on construction, tomo_<NAME>_destroy on close().  A context
    manager.  A subclass sets NAME, load (its module's) and, where return codes map to classes of its own, ERRORS.  device_bytes() and
    plan_seconds() are here for the libraries whose header declares them; on another library they raise AttributeError."""
    NAME = None
    load = None
    ERRORS = {}

    def __init__(self, device=0):
        self._h = None
        self.lib = type(self).load()
        h = ctypes.c_void_p()
        self._check(self._fn("create")(int(device), ctypes.byref(h)), None)
        self._h = h
        self.device = int(device)

    def _fn(self, what):
        return getattr(self.lib, "tomo_%s_%s" % (self.NAME, what))

    def _check(self, rc, h="self"):
        check(self.lib, self.NAME, rc, self._h if h == "self" else h, self.ERRORS)

    @property
    def handle(self):
        if self._h is None:
            raise TomoError("%s handle closed" % self.NAME)
        return self._h

    def device_bytes(self):
        """The device bytes the handle holds between calls, where the library's header declares tomo_<NAME>_device_bytes(h, &n)."""
        n = ctypes.c_int64(0)
        self._check(self._fn("device_bytes")(self.handle, ctypes.byref(n)))
        return n.value

    def plan_seconds(self):
        """The seconds the handle has spent making hipFFT plans, where the header declares tomo_<NAME>_plan_seconds(h, &s)."""
        s = ctypes.c_double(0.0)
        self._check(self._fn("plan_seconds")(self.handle, ctypes.byref(s)))
        return s.value

    def close(self):
        if getattr(self, "_h", None) is not None:
            self._fn("destroy")(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:      # noqa: BLE001
            pass
