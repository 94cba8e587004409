"""_ops.Staging against a fake context, no device: a host call and a device call, each on four ways out -- success, an exception in the
body, the k-th allocation raising (every k the body makes), and free() itself raising while an exception is in flight.  Every array the
scope made and did not hand over is freed exactly once, in reverse order; the caller's input and `out` never; a handed-over array
not; and the exception that propagates is the original one.  Then HandleOwner's choice of the context, and the three shape checks'
messages."""
import numpy as np
import pytest

from tomography_alignment_amd import _lib, _ops


class FakeArray(_lib.DeviceArray):
    """A DeviceArray without a device: it records free() and download()."""

    def __init__(self, ctx, shape, dtype, name):
        self.ctx, self.shape, self.dtype, self.name = ctx, tuple(int(s) for s in np.atleast_1d(shape)), np.dtype(dtype), name
        self.frees, self.downloads, self.ptr, self.fail_free = 0, [], name, False

    def free(self):
        self.frees += 1
        self.ctx.freed.append(self.name)
        if self.fail_free:
            raise RuntimeError("free of %s fails" % self.name)

    def download(self, out=None):
        self.downloads.append(out)
        if out is None:
            out = np.zeros(self.shape, self.dtype)
        out.reshape(-1)[:1] = 7
        return out

    def __del__(self):
        pass


class FakeContext(object):
    """empty, zeros and to_device return FakeArrays, named in the order they were made; the `fail`-th call (from 1) raises."""

    def __init__(self, fail=None, fail_free=()):
        self.made, self.freed, self.calls, self.fail, self.fail_free = [], [], 0, fail, fail_free

    def _make(self, kind, shape, dtype):
        self.calls += 1
        if self.calls == self.fail:
            raise _lib.TomoError("allocation %d fails" % self.calls)
        a = FakeArray(self, shape, dtype, "%s%d" % (kind, self.calls))
        a.fail_free = a.name in self.fail_free
        self.made.append(a)
        return a

    def empty(self, shape, dtype=np.float32):
        return self._make("empty", shape, dtype)

    def zeros(self, shape, dtype=np.float32):
        return self._make("zeros", shape, dtype)

    def to_device(self, host, dtype=np.float32):
        assert host.flags["C_CONTIGUOUS"] and host.dtype == np.dtype(dtype)
        return self._make("up", host.shape, dtype)


def _caller_array(name="given"):
    return FakeArray(FakeContext(), (2, 3), np.float32, name)


def body(ctx, dev, boom=False, out=None):
    """An operation with every kind of array: two sources, a zeroed scratch, a destination.  -> (result, the caller's arrays)."""
    a = _caller_array("a") if dev else np.arange(12, dtype=np.float64).reshape(3, 4)[:, ::2]       # not contiguous, not float32
    b = _caller_array("b") if dev else np.ones((2, 3), np.uint16)
    with _ops.Staging(ctx, dev) as st:
        d_a, d_b = st.source(a), st.source(b, None)
        st.scratch((3,), np.uint8, zero=True)
        d_out = st.dest((2, 3), np.float32, out)
        if boom:
            raise KeyError("the body fails")
        return st.result(d_out, out), [x for x in (a, b, out) if isinstance(x, FakeArray)], (d_a, d_b, d_out)


def _once_in_reverse(ctx, kept=()):
    """Everything the context made but `kept` was freed exactly once, last made first."""
    want = [a.name for a in reversed(ctx.made) if a not in kept]
    assert ctx.freed == want
    assert all(a.frees == (0 if a in kept else 1) for a in ctx.made)


def test_a_device_call_hands_its_result_over_and_frees_the_rest():
    ctx = FakeContext()
    res, given, (d_a, d_b, d_out) = body(ctx, True)
    assert res is d_out and [a.name for a in ctx.made] == ["zeros1", "empty2"] and not res.downloads
    assert d_a is given[0] and d_b is given[1]                       # device sources as they are
    _once_in_reverse(ctx, kept=[res])
    assert all(a.frees == 0 for a in given)


def test_a_device_call_writes_to_the_callers_out_and_never_frees_it():
    ctx, out = FakeContext(), _caller_array("out")
    res, given, _ = body(ctx, True, out=out)
    assert res is out and [a.name for a in ctx.made] == ["zeros1"]
    _once_in_reverse(ctx)
    assert all(a.frees == 0 for a in given) and out in given


def test_a_host_call_uploads_downloads_and_frees_everything():
    ctx = FakeContext()
    res, given, (d_a, d_b, d_out) = body(ctx, False)
    assert isinstance(res, np.ndarray) and res.shape == (2, 3) and res.dtype == np.float32 and not given
    assert [a.name for a in ctx.made] == ["up1", "up2", "zeros3", "empty4"]
    assert (d_a.dtype, d_a.shape, d_b.dtype) == (np.float32, (3, 2), np.uint16)    # float32 by default; None: the array's own
    assert d_out.downloads == [None]
    _once_in_reverse(ctx)


def test_a_host_call_downloads_into_a_host_out_and_returns_it():
    ctx, out = FakeContext(), np.zeros(6, np.float32)
    res, _, (_, _, d_out) = body(ctx, False, out=out)
    assert res is out and out[0] == 7 and len(d_out.downloads) == 1 and d_out.downloads[0] is out
    _once_in_reverse(ctx)


def test_a_new_host_result_takes_the_shape_asked_for():
    ctx = FakeContext()
    with _ops.Staging(ctx, False) as st:
        res = st.result(st.dest((6,), np.int32), shape=(3, 2))
    assert res.shape == (3, 2) and res.dtype == np.int32
    _once_in_reverse(ctx)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_in_place_makes_no_second_buffer(dev):
    """A host call works on its upload where the operation is in place; a device call gets a new array, handed over."""
    ctx = FakeContext()
    src = _caller_array("src") if dev else np.zeros((2, 3), np.float32)
    with _ops.Staging(ctx, dev) as st:
        d = st.source(src)
        d_out = st.dest((2, 3), np.float32, None, inplace=d)
        res = st.result(d_out)
    if dev:
        assert d is src and res is d_out and d_out is not src and [a.name for a in ctx.made] == ["empty1"]
        _once_in_reverse(ctx, kept=[res])
        assert src.frees == 0
    else:
        assert d_out is d and [a.name for a in ctx.made] == ["up1"] and isinstance(res, np.ndarray)
        _once_in_reverse(ctx)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_an_exception_in_the_body_frees_everything_and_propagates(dev):
    ctx, out = FakeContext(), _caller_array("out") if dev else None
    with pytest.raises(KeyError, match="the body fails"):
        body(ctx, dev, boom=True, out=out)
    assert len(ctx.made) == (1 if dev else 4)
    _once_in_reverse(ctx)
    assert out is None or out.frees == 0


@pytest.mark.parametrize("dev,n", [(False, 4), (True, 2)], ids=["host", "dev"])
def test_every_allocation_failing_in_turn(dev, n):
    ctx = FakeContext()
    body(ctx, dev)
    assert ctx.calls == n
    for k in range(1, n + 1):
        ctx = FakeContext(fail=k)
        with pytest.raises(_lib.TomoError, match="allocation %d fails" % k):
            body(ctx, dev)
        assert len(ctx.made) == k - 1
        _once_in_reverse(ctx)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
def test_a_failing_free_does_not_replace_the_exception_in_flight(dev):
    bad = "zeros1" if dev else "zeros3"
    ctx = FakeContext(fail_free=(bad,))
    with pytest.raises(KeyError, match="the body fails"):
        body(ctx, dev, boom=True)
    _once_in_reverse(ctx)                                            # the failing free was tried once, the others still ran
    ctx = FakeContext(fail=2 if dev else 4, fail_free=("zeros1", "up1"))
    with pytest.raises(_lib.TomoError, match="allocation"):
        body(ctx, dev)
    _once_in_reverse(ctx)


def test_a_failing_free_on_a_clean_exit_is_reported_after_the_rest_is_freed():
    ctx = FakeContext(fail_free=("zeros3",))
    with pytest.raises(RuntimeError, match="free of zeros3 fails"):
        body(ctx, False)
    _once_in_reverse(ctx)


# ---- HandleOwner

class _Owner(_ops.HandleOwner):
    def _new_handle(self):
        raise AssertionError("no handle is needed here")


def test_the_owner_takes_the_context_of_a_device_argument_and_does_not_close_it():
    """What the one-shot module functions rely on: `with Cls(None) as p: p.op(device array)` works on the array's context."""
    d = _caller_array()
    o = _Owner()
    o._ready_ctx(d)
    assert o.ctx is d.ctx and o._own_ctx is None
    assert o._staging(d).dev and o._staging(d).ctx is d.ctx and not o._staging(np.zeros(3)).dev
    o.close()
    assert o.ctx is d.ctx                                            # not its own: left as it is
    given = FakeContext()
    o = _Owner(given)
    o._ready_ctx(d)
    assert o.ctx is given                                            # a context given wins


# ---- the shape checks

def test_shape_of():
    assert _ops.shape_of(np.zeros((2, 3, 4)), None, 3, "vol") == (2, 3, 4)
    assert _ops.shape_of(np.zeros(24), (2, 3, 4), 3, "vol") == (2, 3, 4)
    with pytest.raises(ValueError, match=r"vol must have 3 dimensions \(give `shape` for a flat buffer\), got shape \(24,\)"):
        _ops.shape_of(np.zeros(24), None, 3, "vol")
    with pytest.raises(ValueError, match=r"vol holds 24 values, not the 12 of shape \(2, 3, 2\)"):
        _ops.shape_of(np.zeros(24), (2, 3, 2), 3, "vol")
    d = FakeArray(None, (24,), np.float64, "d")
    with pytest.raises(ValueError, match="vol must be float32 on the device, got float64"):
        _ops.shape_of(d, (2, 3, 4), 3, "vol")
    assert _ops.shape_of(np.zeros((2, 0, 4)), None, 3, "vol") == (2, 0, 4)
    with pytest.raises(ValueError, match=r"vol must not be empty, got shape \(2, 0, 4\)"):
        _ops.shape_of(np.zeros((2, 0, 4)), None, 3, "vol", nonempty=True)


def test_stack_shape():
    assert _ops.stack_shape(np.zeros((2, 3, 4)), None, "marginals") == (2, 3, 4)
    with pytest.raises(ValueError, match=r"marginals: proj must be \(n, nx, nz\) \(give `shape` for a flat device buffer\), got shape \(24,\)"):
        _ops.stack_shape(np.zeros(24), None, "marginals")
    with pytest.raises(ValueError, match=r"marginals: proj holds 24 values, not the 12 of shape \(2, 3, 2\)"):
        _ops.stack_shape(np.zeros(24), (2, 3, 2), "marginals")
    with pytest.raises(ValueError, match="marginals: proj must be float32 on the device, got int32"):
        _ops.stack_shape(FakeArray(None, (24,), np.int32, "d"), (2, 3, 4), "marginals")


def test_volume_shape():
    assert _ops.volume_shape(np.zeros(24, np.uint8), (2, 3, 4), [np.uint8, np.bool_], "label") == (2, 3, 4)
    with pytest.raises(ValueError, match=r"label: need a 3-D array \[nx\]\[ny\]\[nz\], not shape \(24,\) \(a flat DeviceArray: pass shape=\)"):
        _ops.volume_shape(np.zeros(24, np.uint8), None, [np.uint8], "label")
    with pytest.raises(ValueError, match=r"postprocess: need a 3-D volume \[nx\]\[ny\]\[nz\], not shape \(24,\)"):
        _ops.volume_shape(np.zeros(24, np.float32), None, [np.float32], "postprocess", "volume")
    with pytest.raises(ValueError, match=r"label: shape \(2, 3, 2\) does not hold 24 elements"):
        _ops.volume_shape(np.zeros(24, np.uint8), (2, 3, 2), [np.uint8], "label")
    with pytest.raises(ValueError, match="label: need uint8 or bool, not float32"):
        _ops.volume_shape(np.zeros(24, np.float32), (2, 3, 4), [np.uint8, np.bool_], "label")
