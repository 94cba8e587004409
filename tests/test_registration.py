"""Volume registration without a GPU: the numpy model tests/vreg_model.py against a brute-force evaluation of the upsampled sum, against
planted shifts and against np.roll; the wrap and Nyquist rules; the arithmetic of registration.Registration; the argument checks of
registration.py that need no device; and the refusals of libtomo_vreg.so's handle-less calls."""
import numpy as np
import pytest

import vreg_model as vm

from tomography_alignment_amd import _lib, _vreg_lib, registration, resolution

SHAPES = [(6, 5, 8), (17, 12, 10), (20, 17, 13), (33, 20, 18)]


def _pair(shape, shift, seed=0):
    ref = vm.blobs(shape, seed)
    mov = vm.fourier_shift(ref, [-s for s in shift])            # moved by -shift, so that `shift` brings it back onto ref
    return ref.astype(np.float32), mov.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ the model

def test_the_upsampled_grid_is_the_sum_it_stands_for():
    shape, u = (6, 5, 8), 4
    ref, mov = _pair(shape, (1.25, -0.5, 0.75))
    a, b = vm.prepare(ref, None)[0], vm.prepare(mov, None)[0]
    P = vm.cross_power(a, b)
    _, peak, s0 = vm.coarse_peak(P, shape)
    cu = vm.upsampled(P, shape, s0, u)
    U, h = vm.grid(u)
    assert cu.shape == (U, U, U) and (U, h) == (6, 3)
    worst = 0.0
    for jx in range(U):
        for jy in range(U):
            for jz in range(U):
                d = [s0[0] + (jx - h) / u, s0[1] + (jy - h) / u, s0[2] + (jz - h) / u]
                worst = max(worst, abs(cu[jx, jy, jz] - vm.brute_force(P, shape, d)))
    assert worst <= 1e-12 * abs(cu.max())
    # the centre of the grid is the coarse peak itself: C2R sums the same terms
    assert abs(cu[h, h, h] - peak) <= 1e-12 * abs(peak)


@pytest.mark.parametrize("shape", SHAPES)
def test_planted_shifts_are_recovered_exactly(shape):
    for u, shift in ((1, (2, -1, 3)), (4, (0.25, -1.5, 0.75)), (10, (1.3, -0.7, 2.1)), (100, (0.37, -1.05, 0.5))):
        ref, mov = _pair(shape, shift, seed=3)
        out = vm.register(ref, mov, upsample=u, mask=None)
        assert np.array_equal(out["shift"], np.asarray(shift, np.float64)), (u, out["shift"])
        # E is of the float32-rounded values and the peak of the float64 ones: the coefficient may pass 1 by their 2^-24 each
        assert 0.99 < out["coefficient"] <= 1.0 + 2.0 ** -22 and out["error"] < 0.15


def test_index_wraps_to_a_negative_shift_past_the_middle():
    assert [vm.wrap_shift(i, 8) for i in range(8)] == [0, 1, 2, 3, 4, -3, -2, -1]
    assert [vm.wrap_shift(i, 7) for i in range(7)] == [0, 1, 2, 3, -3, -2, -1]
    assert list(vm.signed_k(8)) == [0, 1, 2, 3, -4, -3, -2, -1] and list(vm.signed_k(5)) == [0, 1, 2, -2, -1]
    # a roll by n/2 on an even axis comes back as +n/2, by -(n//2) on an odd axis as it is
    ref = vm.blobs((8, 7, 6), 1).astype(np.float32)
    out = vm.register(ref, np.roll(ref, (-4, 3, -3), (0, 1, 2)), upsample=1, mask=None)
    assert out["coarse"] == (4, -3, 3) and np.array_equal(out["shift"], [4.0, -3.0, 3.0])


def test_shift_by_integers_is_a_roll_and_the_nyquist_factor_is_real():
    rng = np.random.default_rng(5)
    v = rng.standard_normal((6, 5, 8))
    assert np.array_equal(vm.fourier_shift(v, (2, -1, 11)), np.roll(v, (2, -1, 11), (0, 1, 2)))
    # a pure Nyquist wave along an even axis: shifted by s it is cos(pi s) times itself, not a complex rotation lost in the C2R
    w = np.cos(np.pi * np.arange(8))[None, None, :] * np.ones((6, 5, 1))
    assert np.allclose(vm.fourier_shift(w, (0, 0, 0.25)), np.cos(np.pi * 0.25) * w, atol=1e-14)
    w = np.cos(np.pi * np.arange(6))[:, None, None] * np.ones((1, 5, 8))
    assert np.allclose(vm.fourier_shift(w, (0.5, 0, 0)), 0.0, atol=1e-14)
    # odd axes have no Nyquist frequency: a fractional shift there and back is the identity, and two half-voxel shifts are a roll by one
    odd = vm.blobs((5, 7, 9), 4)
    back = vm.fourier_shift(vm.fourier_shift(odd, (0.3, -1.2, 0.45)), (-0.3, 1.2, -0.45))
    assert np.max(np.abs(back - odd)) < 1e-13 * odd.max()
    assert np.allclose(vm.fourier_shift(vm.fourier_shift(odd, (0.5, 0.5, 0.5)), (0.5, 0.5, 0.5)), np.roll(odd, (1, 1, 1), (0, 1, 2)), atol=1e-13)


def test_argmax_rules_of_the_model():
    v = np.zeros((3, 4, 5), np.float32)
    v[1, 2, 3] = v[2, 0, 0] = 7.0
    assert vm.argmax(v) == (1 * 20 + 2 * 5 + 3, 7.0)
    v[0, 0, 1] = np.nan
    assert vm.argmax(v)[0] == 33
    i, val = vm.argmax(np.full((2, 2, 2), np.nan, np.float32))
    assert i == 0 and np.isnan(val)


# ------------------------------------------------------------------------------------------------------------------ registration.py

def test_registration_arithmetic():
    r = registration.Registration([1.5, -2.0, 0.25], 6.0, 16.0, 4.0, (2, -2, 0), 4, 1)
    assert r.coefficient == 6.0 / 8.0 and r.error == np.sqrt(1.0 - 0.75 ** 2)
    assert r.shift.dtype == np.float64 and r.coarse == (2, -2, 0) and (r.upsample, r.passes) == (4, 1)
    assert registration.Registration([0, 0, 0], 3.0, 0.0, 4.0, (0, 0, 0), 1, 1).coefficient == 0.0
    over = registration.Registration([0, 0, 0], 8.0000001, 16.0, 4.0, (0, 0, 0), 1, 1)           # rounding above 1 is no NaN
    assert over.coefficient > 1.0 and over.error == 0.0
    ph = registration.Registration([0, 0, 0], 0.5, 16.0, 4.0, (0, 0, 0), 1, 1, normalization="phase")
    assert ph.coefficient == 0.5 and ph.error == np.sqrt(0.75)
    assert "phase" in registration.register.__doc__ or "phase" in registration.Registrar.register.__doc__
    assert "float32 rounding noise" in registration.Registrar.register.__doc__


def test_argument_checks_need_no_device():
    a = np.zeros((8, 8, 8), np.float32)
    r = registration.Registrar()
    for kw in (dict(normalization="power"), dict(passes=0), dict(mask="cube"), dict(edge=-1), dict(radius=float("nan")),
               dict(mask=np.zeros((8, 8, 4), np.float32))):
        with pytest.raises(ValueError):
            r.register(a, a, **kw)
    with pytest.raises(ValueError):
        r.register(a, np.zeros((8, 8, 6), np.float32))
    with pytest.raises(ValueError):
        r.register(a.ravel(), a.ravel())
    with pytest.raises(ValueError):
        r.shift_volume(a, (1.0, 2.0))
    with pytest.raises(ValueError):
        r.shift_volume(a, (1.0, float("inf"), 0.0))
    for bad in ((8, 1, 8), (2049, 2, 2)):
        with pytest.raises(registration.VregUnsupported):
            r.register(np.zeros(bad, np.float32), np.zeros(bad, np.float32))
        with pytest.raises(registration.VregUnsupported):
            r.shift_volume(np.zeros(bad, np.float32), (0.5, 0, 0))
    for u in (0, 101, -3):
        with pytest.raises(registration.VregUnsupported):
            r.register(a, a, upsample=u)
    assert r.handle is None and r.ctx is None                      # all refused before a context or a handle was made
    with pytest.raises(ValueError):
        resolution.Resolution().fsc(a, np.zeros((8, 8, 6), np.float32), register=True)


# ------------------------------------------------------------------------------------------------------------------ the binding

def test_handle_less_calls_raise_in_the_common_format():
    assert issubclass(_vreg_lib.VregUnsupported, _lib.TomoError) and registration.VregUnsupported is _vreg_lib.VregUnsupported
    for shape in ((1, 8, 8), (8, 2049, 8), (8, 8, 0), (2048, 2048, 1024)):
        with pytest.raises(_vreg_lib.VregUnsupported, match=r"^libtomo_vreg error 4: tomo_vreg"):
            _vreg_lib.check(*shape)
    with pytest.raises(_vreg_lib.VregUnsupported, match=r"^libtomo_vreg error 4: tomo_vreg: upsample"):
        _vreg_lib.check(8, 8, 8, 101)
    _vreg_lib.check(2048, 2048, 511, 100)                           # 2^31 - 2^22 values: the largest legal volumes are fine
