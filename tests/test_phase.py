"""CPU tests of the Paganin phase retrieval of tomography_alignment_amd/preprocess.py: paganin_strength, the numpy model
(tests/phase_model.py) and its identities, the padded-length rule, the pinned effect on fringed data, argument validation before any
device is touched, the names of the timed passes against include/tomo_phase.h, and the argument handling of the examples."""
import math

import numpy as np
import pytest

import abi
import phase_model as pm

from tomography_alignment_amd import _lib, _phase_lib, preprocess
from tomography_alignment_amd.examples import generate_data
from tomography_alignment_amd.examples import preprocess as ex_pre


def test_paganin_strength_worked_example():
    a = preprocess.paganin_strength(1e-6, 0.1, energy=25.0, delta_beta=100.0)
    expect = math.pi * (1.2398419843320026e-9 / 25.0) * 0.1 * 100.0 / 1e-12
    assert abs(a - expect) <= 1e-12 * expect
    assert abs(a - 1558.03) < 0.01                                   # "a is about 1558"
    assert abs(a - pm.strength(1e-6, 0.1, energy=25.0, delta_beta=100.0)) <= 1e-12 * a
    b = preprocess.paganin_strength(1e-6, 0.1, wavelength=1.2398419843320026e-9 / 25.0, delta_beta=100.0)
    assert abs(a - b) <= 1e-12 * a
    assert preprocess.paganin_strength(2e-6, 0.1, energy=25.0) == pytest.approx(10 * a / 4, rel=1e-12)     # delta_beta defaults to 1000
    with pytest.raises(ValueError):
        preprocess.paganin_strength(1e-6, 0.1, energy=25.0, wavelength=5e-11)
    with pytest.raises(ValueError):
        preprocess.paganin_strength(1e-6, 0.1)
    for bad in (dict(pixel_size=0.0), dict(dist=-1.0), dict(energy=0.0), dict(delta_beta=float("nan"))):
        kw = dict(pixel_size=1e-6, dist=0.1, energy=25.0, delta_beta=100.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            preprocess.paganin_strength(**kw)


# n_axis, strength, pad -> (m, P).  8 l = 8 sqrt(a) / (2 pi): 1.27 (a = 1), 6.37 (25), 25.5 (400), 50.3 (1558), 80.5 (4000).
PADDING_TABLE = [
    (1024, 0.0, None, 0, 1024), (1024, 1.0, None, 2, 1080), (1024, 25.0, None, 7, 1080), (1024, 400.0, None, 26, 1080),
    (1024, 1558.0, None, 51, 1152), (1024, 4000.0, None, 81, 1200), (1024, 1558.0, 128, 128, 1280), (1024, 1558.0, 0, 0, 1024),
    (2048, 1558.0, None, 51, 2160), (2048, 400.0, None, 26, 2160), (2048, 0.0, 0, 0, 2048),
    (64, 25.0, None, 7, 80), (48, 25.0, None, 7, 64), (33, 25.0, None, 7, 48), (31, 25.0, None, 7, 48), (33, 0.0, None, 0, 36),
    (31, 0.0, 0, 0, 32), (96, 4000.0, None, 81, 270), (48, 4000.0, None, 48, 144), (1, 0.0, None, 0, 2), (1, 400.0, None, 1, 4),
    (7, 0.0, 0, 0, 8), (11, 0.0, 0, 0, 12), (13, 0.0, 0, 0, 16), (17, 0.0, 0, 0, 18),
]


@pytest.mark.parametrize("n, a, pad, m, P", PADDING_TABLE)
def test_padded_length_rule_is_pinned(n, a, pad, m, P):
    assert (pm.pad_width(n, a, pad), pm.padded_length(n, pm.pad_width(n, a, pad))) == (m, P)
    assert preprocess.phase_padding(n, a, pad) == (m, P)
    assert P % 2 == 0 and pm.is_fast_even(P) and P >= n + 2 * m
    assert not any(pm.is_fast_even(q) for q in range(n + 2 * m, P))          # the smallest such length


def test_padded_length_of_the_package_equals_the_model_everywhere():
    for want in range(1, 2500):
        assert preprocess._fast_even(want) == pm.padded_length(want, 0)
    assert preprocess._fast_even(8192) == 8192 and preprocess._fast_even(8193) == 8640


def test_model_constant_frame_and_identity():
    for c in (0.25, 1.0, 1.7):
        T = np.full((2, 33, 31), c)
        for a in (0.0, 25.0, 4000.0):
            assert np.max(np.abs(pm.retrieve(T, a) + math.log(c))) < 1e-13
    assert np.max(np.abs(pm.retrieve(np.zeros((1, 8, 6)), 25.0) + math.log(1e-6))) < 1e-9          # the clamp
    rng = np.random.default_rng(0)
    T = rng.uniform(0.2, 1.3, (3, 40, 27))
    for pad in (None, 0, 5):
        assert np.max(np.abs(pm.retrieve(T, 0.0, pad=pad, minus_log=False) - T)) < 1e-14
    assert pm.transfer(48, 36, 400.0)[0, 0] == 1.0                                           # the DC gain is exactly 1
    # H is symmetric in the signed kx, and the even-length transfer of the header equals the general form
    H = pm.transfer(48, 36, 400.0)
    assert np.array_equal(H[1:24], H[:24:-1]) and np.allclose(H, pm.transfer_any(48, 36, 400.0), rtol=1e-15, atol=0)


def test_model_retrieval_inverts_the_forward_model_on_the_same_periodic_grid():
    T, _ = pm.ellipsoid_frames(2, 64, 48, seed=3)
    for a in (1.0, 25.0, 400.0):
        back = pm.retrieve_periodic(pm.propagate_periodic(T, a), a)
        assert np.max(np.abs(back - T)) < 1e-13, a
    # with the padding of the header the pair is no exact inverse (the crop drops what the filter spread into the margin): small, not zero
    err = np.max(np.abs(pm.retrieve(pm.propagate(T, 25.0), 25.0, minus_log=False) - T))
    print("padded retrieve(propagate(T)) - T: %.2e" % err)
    assert err < 0.05


def test_model_float32_variant_measures_transform_rounding():
    rng = np.random.default_rng(1)
    T = rng.uniform(0.3, 1.2, (3, 33, 31)).astype(np.float32)
    for a in (1.0, 400.0):
        d, ref = pm.d32(T, a)
        print("d32 at a = %g: %.2e" % (a, d))
        assert ref.dtype == np.float64 and 1e-8 < d < 1e-5


def test_pinned_effect_retrieval_removes_the_fringes():
    """Four 128 x 96 frames of ellipsoid projections, propagated with a = 25, noise sigma 0.01: the RMS error of the retrieved line
    integrals against -log T is at least 3 times smaller than that of the plain -log of the fringed data (a float64 sketch gave 6.6;
    this data 5.2: 0.0038 against 0.0196, with line integrals up to 0.85)."""
    T, p = pm.ellipsoid_frames(4, 128, 96, seed=0)
    intensity = pm.propagate(T, 25.0)
    print("propagated intensities %.2f ... %.2f" % (intensity.min(), intensity.max()))
    assert intensity.min() > 0.2
    noisy = intensity + 0.01 * np.random.default_rng(1).standard_normal(intensity.shape)
    e_ret = float(np.sqrt(np.mean((pm.retrieve(noisy, 25.0) - p) ** 2)))
    e_raw = float(np.sqrt(np.mean((pm.finish(noisy) - p) ** 2)))
    print("rms error: retrieved %.4f, plain -log %.4f, ratio %.2f (largest line integral %.2f)" % (e_ret, e_raw, e_raw / e_ret, p.max()))
    assert e_raw / e_ret >= 3.0


class _NoDevice(object):
    """Stands in for _lib.Context / the phase handle: any use fails the test."""

    def __init__(self, *a, **k):
        raise AssertionError("a device object was made before the arguments were checked")


class _FakeDev(_lib.DeviceArray):
    """A DeviceArray that owns nothing: shape, dtype and a pointer value are all the validation reads."""

    def __init__(self, shape, dtype=np.float32, ptr=1 << 20):
        import ctypes
        self.ctx = None
        self.shape = tuple(shape)
        self.dtype = np.dtype(dtype)
        self.size = int(np.prod(shape))
        self.nbytes = self.size * self.dtype.itemsize
        self.ptr = ctypes.c_void_p(ptr)
        self._owner = False

    def free(self):
        pass


@pytest.fixture
def no_device(monkeypatch):
    monkeypatch.setattr(_lib, "Context", _NoDevice)
    monkeypatch.setattr(_phase_lib, "PhaseHandle", _NoDevice)
    monkeypatch.setattr(preprocess._prep_lib, "PrepHandle", _NoDevice)


def test_retrieve_phase_checks_its_arguments_before_any_device(no_device):
    ok = np.full((2, 8, 6), 0.5, np.float32)
    pre = preprocess.Preprocessor()
    bad = [
        (dict(proj=ok.astype(np.float64), strength=1.0), ValueError),                 # dtype
        (dict(proj=ok.astype(np.uint16), strength=1.0), ValueError),
        (dict(proj=ok[0], strength=1.0), ValueError),                                 # dimensions
        (dict(proj=ok[None], strength=1.0), ValueError),
        (dict(proj=ok[:0], strength=1.0), ValueError),                                # empty
        (dict(proj=ok, strength=-1.0), ValueError),
        (dict(proj=ok, strength=float("nan")), ValueError),
        (dict(proj=ok, strength=float("inf")), ValueError),
        (dict(proj=ok, strength="strong"), ValueError),
        (dict(proj=ok), ValueError),                                                  # neither
        (dict(proj=ok, strength=1.0, pixel_size=1e-6), ValueError),                   # both
        (dict(proj=ok, strength=1.0, delta_beta=100.0), ValueError),
        (dict(proj=ok, pixel_size=1e-6, dist=0.1), ValueError),                       # no energy
        (dict(proj=ok, pixel_size=1e-6, dist=0.1, energy=25.0, wavelength=5e-11), ValueError),
        (dict(proj=ok, pixel_size=1e-6, energy=25.0), ValueError),                    # no distance
        (dict(proj=ok, strength=1.0, pad=-1), ValueError),
        (dict(proj=ok, strength=1.0, pad=2.5), ValueError),
        (dict(proj=ok, strength=1.0, pad=True), ValueError),
        (dict(proj=ok, strength=1.0, min_ratio=0.0), ValueError),
        (dict(proj=ok, strength=1.0, min_ratio=-1e-6), ValueError),
        (dict(proj=ok, strength=1.0, min_ratio=float("nan")), ValueError),
        (dict(proj=ok, strength=1.0, min_ratio=1e-60), ValueError),                   # 0 in float32
        (dict(proj=ok, strength=1.0, max_scratch_bytes=-1), ValueError),
        (dict(proj=ok, strength=1.0, out=np.empty_like(ok)), ValueError),             # out is for device input
        (dict(proj=ok, strength=1.0, pad=5000), preprocess.PrepUnsupported),          # 8 + 10000 > 8192
        (dict(proj=np.broadcast_to(np.float32(1), (1, 8200, 2)), strength=1.0), preprocess.PrepUnsupported),   # not at strength 0: no padding there
    ]
    for kw, exc in bad:
        with pytest.raises(exc):
            pre.retrieve_phase(**kw)
        with pytest.raises(exc):
            preprocess.retrieve_phase(**kw)
    with pytest.raises(TypeError):
        pre.retrieve_phase(ok, 1.0, 1e-6)                                             # the physical quantities are keyword-only
    assert pre.ctx is None and pre.handle is None and pre._phase is None


def test_minus_log_checks_its_arguments_before_any_device(no_device):
    ok = np.full((2, 8, 6), 0.5, np.float32)
    pre = preprocess.Preprocessor()
    for kw in (dict(proj=ok.astype(np.float64)), dict(proj=ok[0]), dict(proj=ok, min_ratio=0.0), dict(proj=ok, min_ratio=float("inf")),
               dict(proj=ok, out=np.empty_like(ok))):
        with pytest.raises(ValueError):
            pre.minus_log(**kw)
        with pytest.raises(ValueError):
            preprocess.minus_log(**kw)
    assert pre.ctx is None and pre._phase is None


def test_an_overlapping_out_is_refused_before_any_device(no_device):
    pre = preprocess.Preprocessor()
    d = _FakeDev((4, 8, 6), ptr=1 << 20)
    for off in (4, 4 * 8 * 6 * 4 - 4, -4):
        o = _FakeDev((4, 8, 6), ptr=(1 << 20) + off)
        with pytest.raises(ValueError, match="overlap"):
            pre.retrieve_phase(d, 25.0, out=o)
        with pytest.raises(ValueError, match="overlap"):
            pre.minus_log(d, out=o)
    for o in (_FakeDev((4, 8, 5)), _FakeDev((4, 8, 6), np.uint16)):
        with pytest.raises(ValueError):
            pre.retrieve_phase(d, 25.0, out=o)
    assert pre._phase is None


def test_a_preprocessor_that_never_retrieves_never_makes_a_phase_handle():
    pre = preprocess.Preprocessor()
    assert pre._phase is None
    pre.close()
    assert pre._phase is None


def test_the_passes_are_the_headers():
    constants = abi.parse_header(abi.header_path("phase")).constants
    assert constants["TOMO_PHASE_MS_N"] == len(_phase_lib.PASSES)
    assert [constants["TOMO_PHASE_MS_" + name.upper()] for name in _phase_lib.PASSES] == list(range(len(_phase_lib.PASSES)))


def test_examples_preprocess_phase_arguments():
    a = ex_pre.parse_args(["raw.npz"])
    assert a.phase is None
    a = ex_pre.parse_args(["raw.npz", "--phase-strength", "400"])
    assert a.phase == dict(strength=400.0)
    a = ex_pre.parse_args(["raw.npz", "--pixel-size", "1e-6", "--dist", "0.1", "--energy", "25", "--delta-beta", "100"])
    assert a.phase == dict(pixel_size=1e-6, dist=0.1, energy=25.0, delta_beta=100.0)
    for argv in (["raw.npz", "--phase-strength", "400", "--dist", "0.1"], ["raw.npz", "--pixel-size", "1e-6"],
                 ["raw.npz", "--phase-strength", "-1"]):
        with pytest.raises(SystemExit):
            ex_pre.parse_args(argv)
    with pytest.raises(ValueError):
        ex_pre.run(dict(counts=0, flats=0, darks=0), phase=dict(strenght=1.0))        # an unknown keyword, before any device


def test_generate_data_propagate_leaves_the_default_byte_identical():
    proj = np.random.default_rng(0).uniform(0, 20, (3, 16, 12))
    base = generate_data.make_raw(proj, seed=5)
    again = generate_data.make_raw(proj, seed=5, propagate=None)
    zero = generate_data.make_raw(proj, seed=5, propagate=0)
    for k in ("counts", "flats", "darks"):
        assert base[k].tobytes() == again[k].tobytes() == zero[k].tobytes()
    fringed = generate_data.make_raw(proj, seed=5, propagate=25.0)
    assert fringed["counts"].shape == base["counts"].shape and fringed["counts"].dtype == np.uint16
    assert not np.array_equal(fringed["counts"], base["counts"])
    # the noiseless expectation of the fringed counts is the model's forward propagation of the transmission
    mu = float(base["mu"])
    att = np.exp(-mu * proj)
    assert np.allclose(generate_data.tie_propagate(att, 25.0), pm.propagate(att, 25.0), rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        generate_data.make_raw(proj, seed=5, propagate=-1.0)
