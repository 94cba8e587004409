"""What the front-end classes over a side-library handle do with device memory around one call, on every way out: at least one operation
per class, each with host inputs and with device inputs, on the smallest shapes the libraries take.

(a) a clean run, with the calls to ctx.empty, ctx.zeros and ctx.to_device counted: the arrays alive on the context afterwards, beyond
    those alive before, are exactly the DeviceArrays the call returned (none for a host input, but for Registrar.shift_volume and
    Preprocessor.eigen_flats, whose results are always on the device), and the numbers are those of a run before;
(b) for every k up to that count, a run in which the k-th of those calls raises TomoError: while the exception and its traceback are
    held, every DeviceArray the call made is freed and the caller's arrays are not;
(c) the same with the handle method the operation calls raising TomoError after the staging.

The failures are Python exceptions raised by stubs; no kernel is made to misbehave."""
import numpy as np
import pytest

from tomography_alignment_amd import (_lib, half_acquisition, multires, postprocess, preprocess, registration, resolution, rotation_axis,
                                      segment)
from tomography_alignment_amd.align import consistency

pytestmark = pytest.mark.gpu

RNG = np.random.default_rng(11)
VOL = RNG.uniform(0.5, 1.5, (8, 8, 8)).astype(np.float32)
VOL_B = (np.roll(VOL, 1, 0) + RNG.uniform(0.0, 0.01, (8, 8, 8))).astype(np.float32)
STACK = RNG.uniform(0.5, 1.5, (4, 8, 8)).astype(np.float32)           # a sinogram (n, nx, nz)
STACK16 = RNG.uniform(0.5, 1.5, (4, 16, 8)).astype(np.float32)        # 16 columns: the stripe detector, the half-acquisition window
SINO = RNG.uniform(0.5, 1.5, (8, 16, 8)).astype(np.float32)           # the rotation-axis search: n >= 8, nx >= 16
RAW = RNG.integers(200, 4000, (4, 8, 8)).astype(np.uint16)
FLATS = RNG.integers(4000, 4400, (3, 8, 8)).astype(np.uint16)
DARKS = RNG.integers(90, 110, (2, 8, 8)).astype(np.uint16)
MASK = (VOL > 1.0).astype(np.uint8)
LABELS = np.zeros((8, 8, 8), np.int32)
LABELS[1:3, 1:3, 1:3], LABELS[5:7, 5:7, 5] = 1, 2


class Case(object):
    """make(ctx) -> the front-end object; arrays: the inputs by name (host; uploaded for the device variant); run(obj, **arrays);
    handle(obj) -> the library handle whose `method` the operation calls; host_calls: the allocations of the host variant where the
    operation works in place on its upload; device_result: a host input gives a DeviceArray too."""

    def __init__(self, name, make, arrays, run, handle, method, host_calls=None, device_result=False):
        self.name, self.make, self.arrays, self.run, self.handle, self.method = name, make, arrays, run, handle, method
        self.host_calls, self.device_result = host_calls, device_result


def _h(o):
    return o.handle


CASES = [
    Case("prep.reference_frames", preprocess.Preprocessor, dict(flats=FLATS, darks=DARKS),
         lambda p, flats, darks: p.reference_frames(flats, darks), _h, "reference"),
    Case("prep.normalize", preprocess.Preprocessor, dict(frames=RAW, flats=FLATS, darks=DARKS),
         lambda p, frames, flats, darks: p.normalize(frames, flats, darks), _h, "normalize"),
    Case("prep.eigen_flats", preprocess.Preprocessor, dict(flats=FLATS, darks=DARKS),
         lambda p, flats, darks: p.eigen_flats(flats, darks, n_eff=1), lambda p: p._dff, "eff", device_result=True),
    Case("prep.normalize_dynamic", preprocess.Preprocessor, dict(frames=RAW, flats=FLATS, darks=DARKS),
         lambda p, frames, flats, darks: p.normalize_dynamic(frames, flats, darks, n_eff=1, weights=np.zeros((4, 1))), lambda p: p._dff, "apply"),
    Case("prep.remove_outlier", preprocess.Preprocessor, dict(frames=RAW),
         lambda p, frames: p.remove_outlier(frames, 500.0, return_count=True), _h, "outlier", host_calls=2),
    Case("prep.median_filter", preprocess.Preprocessor, dict(frames=RAW), lambda p, frames: p.median_filter(frames), _h, "outlier", host_calls=1),
    Case("prep.remove_stripe_sorting", preprocess.Preprocessor, dict(proj=STACK),
         lambda p, proj: p.remove_stripe_sorting(proj, size=3), _h, "stripe_sorting"),
    Case("prep.remove_large_stripe", preprocess.Preprocessor, dict(proj=STACK16),
         lambda p, proj: p.remove_large_stripe(proj, size=3, return_mask=True), _h, "stripe_large"),
    Case("prep.minus_log", preprocess.Preprocessor, dict(proj=STACK), lambda p, proj: p.minus_log(proj), lambda p: p._phase, "minus_log",
         host_calls=1),
    Case("post.statistics", postprocess.PostProcessor, dict(vol=VOL), lambda p, vol: p.statistics(vol, "cylinder"), _h, "stats"),
    Case("post.circular_mask", postprocess.PostProcessor, dict(vol=VOL), lambda p, vol: p.circular_mask(vol, 0.9), _h, "mask", host_calls=1),
    Case("post.quantize", postprocess.PostProcessor, dict(vol=VOL), lambda p, vol: p.quantize(vol, (0.5, 1.5)), _h, "quantize"),
    Case("post.project", postprocess.PostProcessor, dict(vol=VOL), lambda p, vol: p.project(vol, 1), _h, "project"),
    Case("post.slice", postprocess.PostProcessor, dict(vol=VOL), lambda p, vol: p.slice(vol, 2, 3), _h, "slice"),
    Case("seg.threshold", segment.Segmenter, dict(vol=VOL), lambda s, vol: s.threshold(vol, lo=1.0), _h, "threshold"),
    Case("seg.label", segment.Segmenter, dict(mask=MASK), lambda s, mask: s.label(mask), _h, "label"),
    Case("seg.measure", segment.Segmenter, dict(labels=LABELS, vol=VOL), lambda s, labels, vol: s.measure(labels, 2, vol), _h, "measure"),
    Case("seg.remove_small", segment.Segmenter, dict(labels=LABELS), lambda s, labels: s.remove_small(labels, 2, 5), _h, "remove_small",
         host_calls=1),
    Case("seg.largest", segment.Segmenter, dict(labels=LABELS), lambda s, labels: s.largest(labels, 2), _h, "largest"),
    Case("reg.register", registration.Registrar, dict(ref=VOL, mov=VOL_B),
         lambda r, ref, mov: r.register(ref, mov, upsample=2, mask=None, passes=2), _h, "correlate"),
    Case("reg.shift_volume", registration.Registrar, dict(vol=VOL), lambda r, vol: r.shift_volume(vol, (0.5, 1.0, 0.0)), _h, "shift",
         device_result=True),
    Case("reg.argmax", registration.Registrar, dict(vol=VOL), lambda r, vol: r.argmax(vol), _h, "argmax"),
    Case("res.fsc", resolution.Resolution, dict(vol_a=VOL, vol_b=VOL_B), lambda r, vol_a, vol_b: r.fsc(vol_a, vol_b, mask=None), _h, "reduce"),
    Case("res.fsc_mask_array", resolution.Resolution, dict(vol_a=VOL, vol_b=VOL_B, mask=VOL),
         lambda r, vol_a, vol_b, mask: r.fsc(vol_a, vol_b, mask=mask), _h, "reduce"),
    Case("res.fsc_register", resolution.Resolution, dict(vol_a=VOL, vol_b=VOL_B),
         lambda r, vol_a, vol_b: r.fsc(vol_a, vol_b, mask=None, register=True, upsample=2), _h, "reduce"),
    Case("pyr.bin_volume", multires.Pyramid, dict(vol=VOL), lambda p, vol: p.bin_volume(vol, 2), _h, "bin_vol"),
    Case("pyr.prolong_volume", multires.Pyramid, dict(vol=VOL), lambda p, vol: p.prolong_volume(vol), _h, "prolong_vol"),
    Case("half.find_center_360", half_acquisition.HalfAcquisition, dict(proj=STACK16),
         lambda a, proj: a.find_center_360(proj, win_width=4, return_curves=True), _h, "search"),
    Case("half.sino_360_to_180", half_acquisition.HalfAcquisition, dict(proj=STACK16), lambda a, proj: a.sino_360_to_180(proj, 11.0), _h,
         "stitch"),
    Case("cons.marginals", consistency.Consistency, dict(proj=STACK), lambda c, proj: c.marginals(proj), _h, "marginals"),
    Case("axis.load", rotation_axis.RotationAxis, dict(proj=SINO), lambda r, proj: r.load(proj), _h, "load_rows"),
]


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context()
    yield c
    c.close()


def _leaves(r):
    """The DeviceArrays, numpy arrays and plain values a result is made of, in a fixed order."""
    if isinstance(r, (tuple, list)):
        for v in r:
            for leaf in _leaves(v):
                yield leaf
    elif isinstance(r, (_lib.DeviceArray, np.ndarray)) or not hasattr(r, "__dict__"):
        yield r
    else:
        for k in sorted(vars(r)):
            for leaf in _leaves(vars(r)[k]):
                yield leaf


def _device_arrays(r):
    return [v for v in _leaves(r) if isinstance(v, _lib.DeviceArray)]


def _numbers(r):
    return [v.download() if isinstance(v, _lib.DeviceArray) else np.asarray(v) for v in _leaves(r)]


def _alive(ctx):
    return {id(a): a for a in list(ctx._arrays) if a.ptr is not None}


class Allocations(object):
    """ctx.empty, ctx.zeros and ctx.to_device counted; the `fail`-th call of them (from 1) raises TomoError instead.  `made` keeps every
    array they returned, so that none is freed by the collector behind the test's back."""

    def __init__(self, monkeypatch, ctx, fail=None):
        self.calls, self.made, self.fail = 0, [], fail
        for name in ("empty", "zeros", "to_device"):
            monkeypatch.setattr(ctx, name, self._wrap(getattr(ctx, name)))

    def _wrap(self, real):
        def call(*args, **kw):
            self.calls += 1
            if self.calls == self.fail:
                raise _lib.TomoError("staging test: allocation %d fails" % self.calls)
            a = real(*args, **kw)
            self.made.append(a)
            return a
        return call


def _raiser(*args, **kw):
    raise _lib.TomoError("staging test: the library call fails")


def _assert_nothing_left(al, given, before, ctx):
    for a in al.made:
        assert a.ptr is None, "an array the call made is still allocated while the exception is held: %s %s" % (a.shape, a.dtype)
    for a in given.values():
        assert not isinstance(a, _lib.DeviceArray) or a.ptr is not None, "the caller's array was freed"
    assert set(_alive(ctx)) == set(before)


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_staging(ctx, case, dev, monkeypatch):
    obj = case.make(ctx)
    try:
        given = {k: (ctx.to_device(v, v.dtype) if dev else v.copy()) for k, v in case.arrays.items()}
        first = case.run(obj, **given)                              # also makes the handle
        want = _numbers(first)
        for a in _device_arrays(first):
            a.free()
        before = _alive(ctx)

        # (a) a clean run
        with monkeypatch.context() as mp:
            al = Allocations(mp, ctx)
            result = case.run(obj, **given)
        n_calls = al.calls
        returned = _device_arrays(result)
        print("%s %s: %d allocations, %d device arrays returned" % (case.name, "dev" if dev else "host", n_calls, len(returned)))
        assert set(_alive(ctx)) - set(before) == {id(a) for a in returned}
        if not dev and not case.device_result:
            assert not returned
        if dev:
            assert all(isinstance(a, _lib.DeviceArray) and a.ptr is not None for a in given.values())
        if not dev and case.host_calls is not None:
            assert n_calls == case.host_calls, "an operation that works in place on its upload made a second buffer"
        got = _numbers(result)
        assert len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))
        for k, v in case.arrays.items():
            if not dev:
                assert np.array_equal(given[k], v), "the host input %s was written to" % k
        for a in returned:
            a.free()
        del result, returned, got
        assert set(_alive(ctx)) == set(before)

        # (b) every allocation fails in turn
        for k in range(1, n_calls + 1):
            with monkeypatch.context() as mp:
                al = Allocations(mp, ctx, fail=k)
                with pytest.raises(_lib.TomoError, match="allocation %d fails" % k) as held:
                    case.run(obj, **given)
                assert held.value is not None
                _assert_nothing_left(al, given, before, ctx)
            del held

        # (c) the library call fails after the staging
        with monkeypatch.context() as mp:
            al = Allocations(mp, ctx)
            mp.setattr(case.handle(obj), case.method, _raiser)
            with pytest.raises(_lib.TomoError, match="the library call fails") as held:
                case.run(obj, **given)
            assert held.value is not None
            _assert_nothing_left(al, given, before, ctx)
        del held
    finally:
        obj.close()
