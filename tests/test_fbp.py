"""CPU tests of recon/fbp.py's host side: the filter response and its windows, the angle weights, the float64 model of FBP (numpy
filter + the CPU oracle's adjoint) against a blob phantom, and the loud failure of libtomo_fbp.so without a device."""
import ctypes

import numpy as np
import pytest

import fbp_model as fm
from oracle import oracle as orc

from tomography_alignment_amd import _fbp_lib
from tomography_alignment_amd.recon import fbp


@pytest.mark.parametrize("ndx", [1, 31, 32, 33, 64, 100, 257, 1024, 4096])
def test_ramp_response_is_abs_f_within_the_truncation_bound(ndx):
    npad = fbp.padded_length(ndx)
    assert npad == max(64, 1 << int(np.ceil(np.log2(2 * ndx)))) and npad >= 2 * ndx
    H = fbp.filter_response(ndx, "ramp")
    f = np.abs(np.fft.fftfreq(npad)[:npad // 2 + 1])
    assert H.shape == (npad // 2 + 1,)
    dev = np.max(np.abs(H - f))
    print("ndx %d Npad %d: max |H - |f|| = %.3e (bound %.3e), H0 = %.3e" % (ndx, npad, dev, 0.25 / npad, H[0]))
    assert dev <= 0.25 / npad
    assert H[0] > 0


def test_padded_length_is_the_integer_rule_at_every_width():
    """tomo_fbp_set_response takes the table without a length and reads Npad/2 + 1 doubles, Npad from the library's integer log2_npad
    (Npad = 64 << l for the first l with 64 << l >= 2 ndx); padded_length and the binding's response_length must give the same.
    Every supported width, and the first unsupported one (its table is still handed to the library, which refuses it)."""
    for ndx in range(1, fbp.MAX_NDX + 2):
        npad = max(64, 1 << (2 * ndx - 1).bit_length())
        assert npad >= 2 * ndx and (npad == 64 or npad < 4 * ndx)
        assert fbp.padded_length(ndx) == npad, ndx
        assert _fbp_lib.response_length(ndx) == npad // 2 + 1, ndx
        if ndx <= fbp.MAX_NDX:
            assert fbp.filter_response(ndx).size == npad // 2 + 1, ndx
    for ndx in (1, 2, 31, 32, 33, 64, 65, 100, 128, 129, 256, 257, 1024, 1025, 2048, 2049, 4096):
        for name in fbp.FILTERS:
            assert fbp.filter_response(ndx, name).size == fbp.padded_length(ndx) // 2 + 1, (ndx, name)
    assert fbp.filter_response(4096).size == 4097 and fbp.filter_response(1).size == 33


def test_set_response_checks_the_length_before_the_c_call():
    h = object.__new__(_fbp_lib.FbpHandle)          # no library, no handle: anything past the length check would raise AttributeError
    for ndx, n in ((100, 128), (100, 130), (32, 65), (33, 33), (4096, 4096), (1, 1)):
        with pytest.raises(ValueError, match="Npad/2 \\+ 1"):
            h.set_response(ndx, np.zeros(n))


def test_pair_err_on_known_arrays():
    ref = np.zeros((2, 4, 5))
    ref[0, :, 0], ref[0, :, 1], ref[0, :, 4], ref[1] = 1.0, 100.0, 2.0, 1.0
    got = ref.copy()
    got[0, 2, 0] += 0.5          # pair 0 of projection 0: 0.5 / 100
    got[0, 1, 4] -= 0.5          # the lone last column: 0.5 / 2
    got[1, 3, 3] += 0.125        # pair 1 of projection 1: 0.125 / 1
    e = fm.pair_errs(got, ref)
    assert e.shape == (2, 3)
    assert np.array_equal(e, [[0.005, 0.0, 0.25], [0.0, 0.125, 0.0]])
    assert fm.pair_err(got, ref) == 0.25


def test_windows_at_zero_and_nyquist():
    expect = {"ramp": (1.0, 1.0), "shepp-logan": (1.0, 2 / np.pi), "cosine": (1.0, 0.0), "hamming": (1.0, 0.08), "hann": (1.0, 0.0)}
    for name, (w0, wn) in expect.items():
        assert fbp.window(name, 0.0) == pytest.approx(w0, abs=1e-15)
        for f in (0.5, -0.5):
            assert fbp.window(name, f) == pytest.approx(wn, abs=1e-15), (name, f)
        H, R = fbp.filter_response(100, name), fbp.filter_response(100, "ramp")
        np.testing.assert_allclose(H, R * fbp.window(name, np.fft.fftfreq(256)[:129]), rtol=0, atol=1e-15)
    for bad in ("ram-lak", "Hann", "", None):
        with pytest.raises(ValueError):
            fbp.filter_response(64, bad)


def test_angle_weights_layouts():
    for n in (1, 2, 3, 90, 180):
        w = fbp.angle_weights(np.linspace(0, np.pi, n, endpoint=False))
        np.testing.assert_allclose(w, np.pi / n, rtol=1e-12)
        w = fbp.angle_weights(np.linspace(0, 2 * np.pi, 2 * n, endpoint=False))          # full 2 pi scan: pi / (2n) each
        np.testing.assert_allclose(w, np.pi / (2 * n), rtol=1e-12)
    for n in (3, 91, 181):                       # endpoint-inclusive (examples/generate_data.py, Geometry): Delta inside, Delta / 2 at the ends
        d = np.pi / (n - 1)
        w = fbp.angle_weights(np.linspace(0, np.pi, n))
        np.testing.assert_allclose(w[1:-1], d, rtol=1e-12)
        np.testing.assert_allclose(w[[0, -1]], d / 2, rtol=1e-12)
    rng = np.random.default_rng(0)
    for _ in range(20):
        phi = rng.uniform(-7, 7, rng.integers(1, 50))
        w = fbp.angle_weights(phi)
        assert np.all(w >= 0) and abs(w.sum() - np.pi) < 1e-12
        perm = rng.permutation(phi.size)
        np.testing.assert_allclose(fbp.angle_weights(phi[perm]), w[perm], rtol=1e-12, atol=1e-15)      # order does not matter
    w = fbp.angle_weights([0.3, 0.3 + np.pi])                       # the same line twice: half the circle each
    np.testing.assert_allclose(w, np.pi / 2)


def test_scale_of_a_non_unit_geometry():
    g = orc.Geo(4, np.array([8, 8, 8]), np.full(3, 0.5), np.array([8, 8]), np.array([0.5, 0.25]), step_size=0.5)
    np.testing.assert_allclose(fbp.projection_scales(g, np.ones(4)), 0.25 * 0.25 / 0.125)


def test_filter_model_is_the_linear_convolution_for_the_ramp():
    rng = np.random.default_rng(1)
    p = rng.standard_normal((2, 37, 3))
    q = fm.filter_model(p, "ramp")
    h = fbp.ramlak_kernel(fbp.padded_length(37))
    m = np.arange(-36, 37)
    hm = h[m % h.size]
    ref = np.stack([np.stack([np.convolve(p[i, :, z], hm)[36:36 + 37] for z in range(3)], axis=1) for i in range(2)])
    assert np.max(np.abs(q - ref)) < 1e-13


# Measured on the model (64^3 blobs, 180 angles): rel-L2 0.0140 and mean ratio 1.00027 at step 1, 0.0081 / 1.00028 at step 0.5,
# 0.0140 / 1.00027 for linspace(0, pi, 181) with its endpoint weights.
@pytest.mark.parametrize("step,phi", [(1.0, np.linspace(0, np.pi, 180, endpoint=False)), (0.5, np.linspace(0, np.pi, 180, endpoint=False)),
                                      (1.0, np.linspace(0, np.pi, 181))], ids=["step1", "step0.5", "endpoints181"])
def test_cpu_model_reconstructs_the_blob_phantom(step, phi):
    N = 64
    x = fm.blob_phantom(N)
    og = orc.Geo(phi.size, np.array([N, N, N]), np.ones(3), np.array([N, N]), np.ones(2), step_size=step)
    p = orc.forward(og, x, phi=phi).reshape(phi.size, N, N)
    rec = fm.fbp_model(og, p, phi)
    err, ratio = fm.accuracy(rec, x)
    print("CPU model, step %.1f, %d angles: rel-L2 %.4f, mean ratio %.5f" % (step, phi.size, err, ratio))
    assert err <= 0.05
    assert abs(ratio - 1) <= 0.02


def test_no_device_means_loud_failure():
    lib = _fbp_lib.load()
    n = ctypes.c_int(0)
    from tomography_alignment_amd import _lib
    rc = _lib.load().tomo_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_lib.TomoError):
        _fbp_lib.FbpHandle(0)
    assert lib.tomo_fbp_filter(None, None, None, None, 1, 64, 64, None) != 0
