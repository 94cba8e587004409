"""GPU tests of the volume registration (tomography_alignment_amd/registration.py, libtomo_vreg.so) against the numpy model
tests/vreg_model.py: planted periodic shifts (exact up to upsample 10, within one grid step at 100), phase normalisation on white noise,
masked phantoms with one and two passes, the peak and the energies at the scale float32 transforms allow, shift_volume (integer
shifts bit for bit, nothing written outside the destination), the tie and NaN rules of argmax, bit-identical repeats across handles,
inputs and scratch budgets, the refusals, the handle's lifetime, and the two drivers (resolution.fsc(register=True),
align_rigid.run(register_truth=True)).  Every test prints the figures it measured.

The shapes: odd and even nz (the R2C padding and the Nyquist plane), an x tail and a z tail past a wave, rows shorter than four
elements' alignment, an axis shorter than the U candidates of the refinement."""
import numpy as np
import pytest

import fsc_model as fm
import vreg_model as vm

from tomography_alignment_amd import _lib, _vreg_lib, registration, resolution
from tomography_alignment_amd.examples import align_rigid, generate_data
from tomography_alignment_amd.utilities.generate_phantom import shepp3d

pytestmark = pytest.mark.gpu

SHAPES = [(6, 5, 8), (17, 12, 10), (20, 17, 13), (33, 20, 18), (64, 48, 40)]

# The admissible difference between the GPU (float32 hipFFT) and the float64 model, as in tests/test_gpu_resolution.py: d32 is what
# float32 transforms cost in the MODEL (scipy.fft in complex64 against the float64 run, same inputs), computed by every test for its
# own inputs; hipFFT factors the lengths differently from pocketfft, so the same order is expected, not the same value, and K_D32 times
# d32 is allowed.  For a single number such as the peak, d32 is the largest difference over the whole correlation grid the peak is the
# maximum of (one value's own difference can be small by chance), relative to the peak.
K_D32 = 16.0


@pytest.fixture()
def ctx():
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture()
def reg(ctx):
    r = registration.Registrar(ctx)
    yield r
    r.close()


def _pair(shape, shift, seed=0):
    """(ref, mov) float32: blobs, and the copy moved by -shift in float64 by the model's Fourier shift, so that `shift` brings it back."""
    ref = vm.blobs(shape, seed)
    mov = vm.fourier_shift(ref, [-float(s) for s in shift])
    return ref.astype(np.float32), mov.astype(np.float32)


def _expected_integer(s, shape):
    return np.array([vm.wrap_shift(int(v) % n, n) for v, n in zip(s, shape)], np.float64)


# ------------------------------------------------------------------------------------------------------------------ planted, periodic

@pytest.mark.parametrize("shape", SHAPES)
def test_integer_rolls_are_recovered_exactly(reg, shape):
    nx, ny, nz = shape
    ref = vm.blobs(shape, 1).astype(np.float32)
    for s in ((2, -1, 3), (-2, 1, -1), (nx // 2, -(ny // 2), nz // 2), (-(nx // 2), ny // 2, 0), (0, 0, 0)):
        mov = np.roll(ref, tuple(-v for v in s), (0, 1, 2))
        want = _expected_integer(s, shape)
        for u in (1, 4):
            got = reg.register(ref, mov, upsample=u, mask=None)
            assert np.array_equal(got.shift, want), (s, u, got.shift)
            assert got.coarse == tuple(int(v) for v in want) and got.upsample == u and got.passes == 1
            assert abs(got.coefficient - 1.0) < 1e-5 and got.error < 5e-3


@pytest.mark.parametrize("shape", SHAPES)
def test_planted_multiples_of_the_grid_step_are_recovered_exactly(reg, shape):
    for u, shifts in ((4, ((0.25, -1.5, 0.75), (-1.75, 0.5, 1.0))), (10, ((1.3, -0.7, 2.1), (-0.4, 1.6, 0.5)))):
        for s in shifts:
            ref, mov = _pair(shape, s, seed=2)
            got = reg.register(ref, mov, upsample=u, mask=None)
            assert np.array_equal(got.shift, np.asarray(s, np.float64)), (u, s, got.shift)
            assert np.array_equal(vm.register(ref, mov, upsample=u, mask=None)["shift"], np.asarray(s, np.float64))


def test_upsample_100_is_within_one_grid_step(reg):
    """At u = 100 the winner's margin over the runner-up is 3e-6 ... 1.5e-5 of the peak in the float64 model, and hipFFT's roundings
    differ from pocketfft's: one grid step per axis is allowed, against the planted value and against the model, in at most a quarter of
    the cases.  In the CPU model none uses it."""
    u, step = 100, 1.0 / 100 + 1e-12
    used, cases = 0, 0
    for shape in SHAPES:
        for s in ((0.37, -1.05, 0.5), (-2.41, 0.08, 1.99)):
            ref, mov = _pair(shape, s, seed=3)
            got = reg.register(ref, mov, upsample=u, mask=None)
            model = vm.register(ref, mov, upsample=u, mask=None)
            d_p, d_m = np.abs(got.shift - np.asarray(s)), np.abs(got.shift - model["shift"])
            cases += 1
            used += bool(d_p.max() > 0)
            print("u 100 %s %s: GPU %s model %s" % (shape, s, got.shift, model["shift"]))
            assert np.all(d_p <= step) and np.all(d_m <= step), (shape, s, got.shift, model["shift"])
    print("u = 100: %d of %d cases used the grid step" % (used, cases))
    assert 4 * used <= cases


# ------------------------------------------------------------------------------------------------------------------ "phase"

@pytest.mark.parametrize("shape", SHAPES)
def test_phase_normalisation_on_white_noise(reg, shape):
    rng = np.random.default_rng(7)
    ref = rng.standard_normal(shape).astype(np.float32)
    for s in ((1, -2, 3), (-1, 0, 2)):
        got = reg.register(ref, np.roll(ref, tuple(-v for v in s), (0, 1, 2)), upsample=1, normalization="phase", mask=None)
        assert np.array_equal(got.shift, _expected_integer(s, shape)) and got.coefficient == got.peak
    for s in ((0.5, 0.5, -0.25), (-0.5, 0.25, -0.75)):      # the float64 and the complex64 model find these on every shape, by >= 2e-2 of the peak
        mov = vm.fourier_shift(ref.astype(np.float64), [-v for v in s]).astype(np.float32)
        got = reg.register(ref, mov, upsample=4, normalization="phase", mask=None)
        assert np.array_equal(got.shift, np.asarray(s)), (s, got.shift)
    # every other case against the model only, within one grid step
    s = (0.3, -0.7, 1.1)
    mov = vm.fourier_shift(ref.astype(np.float64), [-v for v in s]).astype(np.float32)
    got = reg.register(ref, mov, upsample=10, normalization="phase", mask=None)
    model = vm.register(ref, mov, upsample=10, normalization="phase", mask=None)
    print("phase %s u 10: GPU %s model %s" % (shape, got.shift, model["shift"]))
    assert np.all(np.abs(got.shift - model["shift"]) <= 0.1 + 1e-12)


# ------------------------------------------------------------------------------------------------------------------ masked

@pytest.mark.parametrize("n,u,s", [(32, 10, (1.3, -0.7, 2.1)), (48, 10, (-3.4, 2.6, 0.5)), (32, 100, (1.37, -2.05, 0.5)),
                                   (48, 100, (1.37, -2.05, 0.5))])
def test_masked_phantom_one_and_two_passes(reg, n, u, s):
    x = shepp3d(n).astype(np.float64)
    ref = x.astype(np.float32)
    mov = vm.fourier_shift(x, [-v for v in s]).astype(np.float32)
    step = 1.0 / u + 1e-12
    for passes in (1, 2):
        got = reg.register(ref, mov, upsample=u, mask="sphere", edge=6, passes=passes)
        model = vm.register(ref, mov, upsample=u, mask="sphere", edge=6.0, passes=passes)
        print("shepp %d u %d passes %d planted %s: GPU %s model %s, coefficient %.6f" % (n, u, passes, s, got.shift, model["shift"],
                                                                                         got.coefficient))
        assert np.all(np.abs(got.shift - model["shift"]) <= step)
        assert got.passes == passes
    assert np.all(np.abs(got.shift - np.asarray(s)) <= step)            # two passes end within one grid step of the planted value


# ------------------------------------------------------------------------------------------------------------------ peak, E, coefficient

def _model_grids(ref, mov, u, dtype, **kw):
    """(the grid the peak is the maximum of, E0, E1) of the model: c for u = 1, c_u otherwise."""
    a, E0 = vm.prepare(ref, kw.get("mask", "sphere"), kw.get("edge", 6.0), None, kw.get("subtract_mean", True))
    b, E1 = vm.prepare(mov, kw.get("mask", "sphere"), kw.get("edge", 6.0), None, kw.get("subtract_mean", True))
    P = vm.cross_power(a, b, None, dtype)
    import scipy.fft
    c = scipy.fft.irfftn(P, s=ref.shape)
    if u == 1:
        return np.asarray(c, np.float64), E0, E1
    s0 = vm.coarse_peak(vm.cross_power(a, b), ref.shape)[2]          # one grid for both runs: about the float64 run's coarse peak
    return vm.upsampled(P, ref.shape, s0, u), E0, E1


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kw", [dict(mask=None, subtract_mean=False), dict(mask=None, subtract_mean=True), dict(mask="sphere", edge=2.0)])
def test_peak_and_energies_against_the_model(reg, shape, kw):
    ref, mov = _pair(shape, (0.6, -1.2, 0.3), seed=4)
    N = ref.size
    for u in (1, 10):
        got = reg.register(ref, mov, upsample=u, **kw)
        g64, E0, E1 = _model_grids(ref, mov, u, np.float64, **kw)
        g32, _, _ = _model_grids(ref, mov, u, np.float32, **kw)
        peak = float(g64.max())
        d32 = float(np.max(np.abs(g32 - g64))) / abs(peak)
        dp = abs(got.peak - peak) / abs(peak)
        for e_g, e_m in ((got.E0, E0), (got.E1, E1)):
            assert abs(e_g - e_m) <= (N - 1) * 2.0 ** -53 * e_m, (e_g, e_m)
        print("%s %s u %d: peak %.9g model %.9g, d32 %.2e, GPU - model %.2e (%.3f of the bound); E0 %.17g E1 %.17g" % (
            shape, kw, u, got.peak, peak, d32, dp, dp / (K_D32 * d32), got.E0, got.E1))
        assert dp <= K_D32 * d32
        assert got.coefficient == registration.coefficient_of(got.peak, got.E0, got.E1)
        assert 0.0 <= got.error <= 1.0


# ------------------------------------------------------------------------------------------------------------------ shift_volume

@pytest.mark.parametrize("shape", SHAPES)
def test_integer_shifts_are_rolls_bit_for_bit(reg, ctx, shape):
    rng = np.random.default_rng(8)
    v = rng.standard_normal(shape).astype(np.float32)
    N = v.size
    d_v = ctx.to_device(v)
    for s in ((1, 0, 0), (0, 0, 1), (2, -1, 3), (-5, 7, -9), (0, 0, 0), (shape[0], -shape[1], 2 * shape[2] + 1)):
        want = np.roll(v, s, (0, 1, 2))
        out = reg.shift_volume(d_v, s)
        assert out.shape == shape and np.array_equal(out.download(), want), s
        out.free()
        # an output one element off a 16-byte boundary, with guards on both sides
        buf = ctx.to_device(np.full(N + 8, -7.0, np.float32))
        assert reg.shift_volume(d_v, s, out=buf.view(1, N)) is not None
        got = buf.download()
        assert np.array_equal(got[1:N + 1], want.ravel()) and np.all(got[:1] == -7.0) and np.all(got[N + 1:] == -7.0), s
        # in place, aligned and not
        buf.upload(np.concatenate([np.full(1, -7.0, np.float32), v.ravel(), np.full(7, -7.0, np.float32)]))
        w = buf.view(1, N)
        reg.shift_volume(w, s, out=w, shape=shape)
        got = buf.download()
        assert np.array_equal(got[1:N + 1], want.ravel()) and np.all(got[:1] == -7.0) and np.all(got[N + 1:] == -7.0), s
        buf.free()
        d_w = ctx.to_device(v)
        reg.shift_volume(d_w, s, out=d_w)
        assert np.array_equal(d_w.download(), want)
        d_w.free()
    assert np.array_equal(d_v.download(), v)
    with pytest.raises(_lib.TomoError, match="overlap"):
        big = ctx.zeros((N + 4,))
        reg.shift_volume(big.view(0, N), (1, 0, 0), out=big.view(4, N), shape=shape)
    assert np.array_equal(registration.shift_volume(v, (2, -1, 3)), np.roll(v, (2, -1, 3), (0, 1, 2)))      # host in, own context: host out


@pytest.mark.parametrize("shape", SHAPES)
def test_fractional_shifts_against_the_model(reg, ctx, shape):
    v64 = vm.blobs(shape, 5)
    # no Nyquist content, so that a shift and its negative are the identity (the real cos(pi s) at the Nyquist frequency of an even axis
    # is not undone by the shift back)
    import scipy.fft
    V = scipy.fft.rfftn(v64)
    for ax, n in enumerate(shape):
        if n % 2 == 0:
            sl = [slice(None)] * 3
            sl[ax] = n // 2
            V[tuple(sl)] = 0.0
    v = scipy.fft.irfftn(V, s=shape).astype(np.float32)
    vmax = float(np.abs(v).max())
    N = v.size
    worst = 0.0
    for s in ((0.5, 0.0, 0.0), (0.0, 0.0, 0.25), (0.3, -1.2, 0.45), (-7.75, 2.5, 13.125)):
        m64 = vm.fourier_shift(v.astype(np.float64), s)
        m32 = vm.fourier_shift(v, s, np.float32)
        d32 = float(np.max(np.abs(m32 - m64))) / vmax
        buf = ctx.to_device(np.full(N + 8, -7.0, np.float32))
        reg.shift_volume(v, s, out=buf.view(1, N))
        got = buf.download()
        assert np.all(got[:1] == -7.0) and np.all(got[N + 1:] == -7.0)
        d = float(np.max(np.abs(got[1:N + 1].reshape(shape) - m64))) / vmax
        back = reg.shift_volume(buf.view(1, N), [-x for x in s], shape=shape)
        db = float(np.max(np.abs(back.download() - v))) / vmax
        back.free()
        buf.free()
        worst = max(worst, d / (K_D32 * d32))
        print("%s shift %s: d32 %.2e, GPU - model %.2e (%.3f of the bound), there and back %.2e" % (shape, s, d32, d, d / (K_D32 * d32), db))
        assert d <= K_D32 * d32
        assert db <= 2 * K_D32 * d32                         # two shifts, each within the bound
    # the sign: shift_volume(mov, register(ref, mov).shift) is ref
    ref, mov = _pair(shape, (0.5, -0.25, 1.0), seed=6)
    found = reg.register(ref, mov, upsample=4, mask=None)
    moved = reg.shift_volume(mov, found.shift)
    e_moved, e_raw = np.max(np.abs(moved.download() - ref)), np.max(np.abs(mov - ref))
    moved.free()
    wrong = reg.shift_volume(mov, -found.shift)
    e_wrong = np.max(np.abs(wrong.download() - ref))
    wrong.free()
    print("%s: max |shift_volume(mov, s) - ref| %.2e, unshifted %.2e, shifted the wrong way %.2e" % (shape, e_moved, e_raw, e_wrong))
    assert np.array_equal(found.shift, [0.5, -0.25, 1.0]) and e_moved < 0.2 * e_raw and e_moved < 0.2 * e_wrong


# ------------------------------------------------------------------------------------------------------------------ argmax

def test_argmax_ties_and_nan(reg, ctx):
    shape = (64, 48, 40)                      # 30720 groups of four: 120 work-groups of 1024 elements each; rows of 40 take the 16-byte loads
    rng = np.random.default_rng(9)
    base = rng.random(shape).astype(np.float32)
    N = base.size

    def both(v):
        """argmax through the aligned (16-byte loads) and the unaligned (4-byte loads) path: the same answer."""
        flat = v.ravel()
        a = reg.argmax(v)
        buf = ctx.to_device(np.concatenate([np.zeros(1, np.float32), flat, np.zeros(3, np.float32)]))
        b = reg.argmax(buf.view(1, N), shape=shape)
        buf.free()
        assert a[0] == b[0] and (a[1] == b[1] or (np.isnan(a[1]) and np.isnan(b[1])))
        return int(np.ravel_multi_index(a[0], shape)), a[1]

    for idx in ([100000, 5000], [5004, 5000], [5000, 5001, 5002, 5003], [5063, 5000 + 64], list(range(N - 1, 0, -997)), [N - 1, 0]):
        v = base.copy().ravel()
        v[idx] = 2.0
        assert both(v.reshape(shape)) == (min(idx), np.float32(2.0)), idx
    v = base.copy().ravel()
    v[7000] = 2.0
    v[[6999, 7001, 0, N - 1]] = np.nan                    # a NaN beside the maximum, and at both ends, never wins
    assert both(v.reshape(shape)) == (7000, np.float32(2.0))
    v[:] = np.nan
    i, val = both(v.reshape(shape))
    assert i == 0 and np.isnan(val)
    v[12345] = -np.inf                                    # anything that is not NaN beats NaN
    assert both(v.reshape(shape)) == (12345, np.float32(-np.inf))
    assert both(base)[0] == int(np.argmax(base))
    # the maximum in the last element of an odd row, and in the last element of the volume
    odd = (20, 17, 13)
    w = rng.random(odd).astype(np.float32)
    w[3, 5, 12] = 3.0
    assert reg.argmax(w) == ((3, 5, 12), np.float32(3.0)) == vm_argmax3(w)
    w[19, 16, 12] = 4.0
    assert reg.argmax(w) == ((19, 16, 12), np.float32(4.0))
    assert registration.argmax(w) == ((19, 16, 12), np.float32(4.0))


def vm_argmax3(v):
    i, val = vm.argmax(v)
    return tuple(int(j) for j in np.unravel_index(i, v.shape)), val


# ------------------------------------------------------------------------------------------------------------------ determinism

def _bits(r):
    return (r.shift.tobytes(), r.peak, r.E0, r.E1, r.coarse, r.upsample)


def test_results_are_deterministic(reg, ctx):
    shape = (20, 17, 13)
    ref, mov = _pair(shape, (1.3, -0.7, 2.1), seed=10)
    d_ref, d_mov = ctx.to_device(ref), ctx.to_device(mov)
    other = ctx.to_device(np.random.default_rng(1).standard_normal((33, 20, 18)).astype(np.float32))
    for kw in (dict(upsample=10), dict(upsample=100, mask=None), dict(upsample=1), dict(upsample=10, normalization="phase", passes=2)):
        r0 = _bits(reg.register(d_ref, d_mov, **kw))
        assert _bits(reg.register(d_ref, d_mov, **kw)) == r0
        reg.register(other, other, upsample=4)                       # another shape and other data between: stale scratch would show
        assert _bits(reg.register(ref, mov, **kw)) == r0             # host input
        with registration.Registrar(ctx) as fresh:                   # a handle that has seen nothing else
            assert _bits(fresh.register(d_ref, d_mov, **kw)) == r0
        U = vm.grid(kw["upsample"])[0]
        plane = 16 * shape[1] * U                                    # T1 of one kx plane
        for budget in (1, 3 * plane, 0):                             # one plane, three planes, the default
            with registration.Registrar(ctx) as other_budget:
                other_budget._ready(None)
                other_budget.handle.set_scratch_bytes(budget)
                assert _bits(other_budget.register(d_ref, d_mov, **kw)) == r0, (kw, budget)
    assert np.array_equal(d_ref.download(), ref) and np.array_equal(d_mov.download(), mov)        # the inputs are not written
    flat = ctx.to_device(mov.ravel())
    assert _bits(reg.register(d_ref, flat, shape=shape, upsample=10)) == _bits(reg.register(d_ref, d_mov, upsample=10))
    with pytest.raises(ValueError):
        reg.register(d_ref, flat)


def test_a_non_finite_volume_raises(reg):
    ref, mov = _pair((17, 12, 10), (1, 0, 0))
    mov[3, 4, 5] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        reg.register(ref, mov, mask=None)


# ------------------------------------------------------------------------------------------------------------------ refusals, lifetime

def test_refusals_come_before_any_launch(ctx):
    r = registration.Registrar(ctx)
    before = len(ctx._arrays)
    a = np.zeros((8, 8, 8), np.float32)
    for bad in ((8, 1, 8), (2049, 2, 2)):
        z = np.zeros(bad, np.float32)
        with pytest.raises(registration.VregUnsupported):
            r.register(z, z)
        with pytest.raises(registration.VregUnsupported):
            r.shift_volume(z, (0.5, 0, 0))
        with pytest.raises(registration.VregUnsupported):
            r.argmax(z)
    for u in (0, 101):
        with pytest.raises(registration.VregUnsupported):
            r.register(a, a, upsample=u)
    with pytest.raises(ValueError):
        r.register(a, np.zeros((8, 8, 6), np.float32))
    assert r.handle is None and len(ctx._arrays) == before            # refused before a handle was made or anything uploaded
    with _vreg_lib.VregHandle(ctx.device) as h:
        st = ctx.stream()
        d = ctx.zeros((8, 8, 8))
        for call in (lambda: h.prepare(st, 0, d.ptr), lambda: h.correlate(st), lambda: h.refine(st, 4), lambda: h.fetch(st),
                     lambda: h.shift(st, d.ptr, (1, 0, 0), d.ptr), lambda: h.argmax(st, d.ptr)):
            with pytest.raises(_lib.TomoError, match="call tomo_vreg_set_shape first"):
                call()
        with pytest.raises(registration.VregUnsupported):
            h.set_shape(8, 8, 1)
        with pytest.raises(registration.VregUnsupported):
            h.set_shape(2048, 2048, 1024)
        assert h.device_bytes() == 0
        h.set_shape(8, 8, 8)
        bytes_one = h.device_bytes()
        assert bytes_one >= 3 * 8 * 8 * 8 * 5 and h.plan_seconds() > 0.0
        for u in (0, 101):
            with pytest.raises(registration.VregUnsupported):
                h.refine(st, u)
        with pytest.raises(_lib.TomoError, match="slot"):
            h.prepare(st, 2, d.ptr)
        with pytest.raises(_lib.TomoError, match="NULL"):
            h.prepare(st, 0, None)
        planned = h.plan_seconds()
        h.set_shape(8, 8, 8)
        assert h.device_bytes() == bytes_one and h.plan_seconds() == planned          # the plans and the buffers are reused
        d.free()
    r.close()


def test_handle_lifetime():
    h = _vreg_lib.VregHandle(0)
    assert h.handle and h.device == 0
    h.close()
    h.close()
    with pytest.raises(_lib.TomoError, match="^vreg handle closed$"):
        h.handle
    with pytest.raises(_lib.TomoError, match="device out of range"):
        _vreg_lib.VregHandle(10**6)
    live = len(_lib.LIVE_CONTEXTS)
    p = registration.Registrar()
    p._ready(None)
    c, hh = p.ctx, p.handle
    assert isinstance(hh, _vreg_lib.VregHandle) and hh.handle and c.handle and len(_lib.LIVE_CONTEXTS) == live + 1
    p.close()
    assert p.ctx is None and p.handle is None and len(_lib.LIVE_CONTEXTS) == live
    with pytest.raises(_lib.TomoError, match="handle closed"):
        hh.handle
    p.close()
    given = _lib.Context(0)
    with registration.Registrar(given) as q:
        q._ready(None)
        assert q.ctx is given and q.handle.device == given.device
    assert given.handle and q.handle is None                          # a given context is left open
    given.close()


# ------------------------------------------------------------------------------------------------------------------ drivers

def test_fsc_of_a_rolled_pair_with_and_without_registration(ctx):
    N, sigma = 48, 0.02
    rng = np.random.default_rng(11)
    x = shepp3d(N).astype(np.float64)
    a = (x + sigma * rng.standard_normal(x.shape)).astype(np.float32)
    b = (x + sigma * rng.standard_normal(x.shape)).astype(np.float32)
    rolled = np.roll(b, (2, -1, 3), (0, 1, 2))
    with resolution.Resolution(ctx) as res:
        before = len(ctx._arrays)
        c_pair = res.fsc(a, b)
        c_reg = res.fsc(a, rolled, register=True)
        c_raw = res.fsc(a, rolled, register=False)
        assert len(ctx._arrays) == before
    assert c_reg.shift == (-2.0, 1.0, -3.0) and c_pair.shift is None and c_raw.shift is None
    # the d32 scale of tests/test_gpu_resolution.py for these inputs
    C, PA, PB, n = fm.sums(a, b)
    C32, PA32, PB32, _ = fm.sums(a, b, dtype=np.float32)
    live = PA * PB > 0
    live[0] = False
    d32 = float(np.max(np.abs(fm.curve(C32, PA32, PB32) - fm.curve(C, PA, PB))[live]))
    tol = K_D32 * d32 + 4e-6 / np.sqrt(np.maximum(n, 1.0))
    d = np.abs(c_reg.fsc - c_pair.fsc)
    print("fsc(register=True) of the rolled pair against fsc of the pair: %.2e (d32 %.2e, largest fraction of the bound %.3f)" % (
        d[live].max(), d32, (d / tol)[live].max()))
    assert np.array_equal(c_reg.count, c_pair.count) and np.all(d[live] <= tol[live])
    s_reg, st_reg = c_reg.crossing("half-bit")
    s_raw, st_raw = c_raw.crossing("half-bit")
    print("half-bit crossing: registered %s (%s), unregistered %s (%s)" % (s_reg, st_reg, s_raw, st_raw))
    assert st_raw == "crossed" and (st_reg != "crossed" or s_raw < s_reg)
    assert resolution.fsc(a, rolled, register=True, ctx=ctx).shift == (-2.0, 1.0, -3.0)


WALLS = ("sirt_wall_s", "align_wall_s")


def test_align_rigid_reports_the_registered_rmse():
    data = generate_data.make(32, 24, seed=1)
    kw = dict(n_outer=1, sirt_iters=5, verbose=False)       # one outer iteration: the run tests/test_gpu_postprocess.py repeats bit for bit
    plain = align_rigid.run(dict(data), **kw)
    out = align_rigid.run(dict(data), register_truth=True, **kw)
    for p, q in zip(plain[:4], out[:4]):
        assert np.array_equal(p, q)                                   # d_rec was not modified: the run is the same run
    assert len(out[4]) == len(plain[4]) == 1
    for hp, hq in zip(plain[4], out[4]):
        assert set(hq) == set(hp) | {"truth_shift", "rmse_registered"}
        for k in hp:
            if k in WALLS:
                continue
            if isinstance(hp[k], float):
                # the solver's float64 sums (rmse, residual) are added by atomics in no fixed order: two runs of the SAME command differ
                # in the last bits, by at most N 2^-53 of a sum of N = 32^3 terms
                assert abs(hp[k] - hq[k]) <= 32 ** 3 * 2.0 ** -53 * abs(hp[k]), k
            else:
                assert np.array_equal(hp[k], hq[k]), k
        print("align_rigid 32^3: rmse %.6f, registered %.6f, truth_shift %s" % (hq["rmse"], hq["rmse_registered"], hq["truth_shift"]))
        assert len(hq["truth_shift"]) == 3 and np.all(np.isfinite(hq["truth_shift"]))
        assert 0.0 < hq["rmse_registered"] <= hq["rmse"] * (1 + 1e-6)
    no_phantom = {"projections": data["projections"], "phi": data["phi"]}
    quiet = align_rigid.run(no_phantom, register_truth=True, n_outer=1, sirt_iters=5, verbose=False)
    assert "rmse_registered" not in quiet[4][0]
