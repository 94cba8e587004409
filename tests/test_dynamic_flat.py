"""Dynamic flat-field correction without a GPU: the numpy model of tests/dff_model.py (its gradient against finite differences, the
eigenvalue rule and the gain over the conventional normalisation on generate_data's drifting beam), generate_data --beam-drift, the
option parsing of both examples, the library's refusals and batch rules, and every refusal of preprocess.eigen_flats /
normalize_dynamic before a device is touched."""
import numpy as np
import pytest

import dff_model as dm
import prep_model as pm

from tomography_alignment_amd import _dff_lib, preprocess
from tomography_alignment_amd.examples import generate_data
from tomography_alignment_amd.examples import preprocess as ex_pre


@pytest.fixture(scope="module")
def drifting():
    mp = pytest.MonkeyPatch()
    try:
        yield dm.drifting_data(mp.setattr)
    finally:
        mp.undo()


# ------------------------------------------------------------------------------------------------------------------------ the model

def test_model_gradient_equals_finite_differences():
    """m = 3 on a 9 x 11 binned frame at random weights: central differences of the model's own float64 cost (step 1e-6, truncation
    error ~ h^2 f''' ~ 1e-12 relative, rounding ~ 1e-16 f / h ~ 1e-10 f) against its gradient, relative to the sum of |terms|."""
    rng = np.random.default_rng(0)
    zb, xb, m = 9, 11, 3
    Fb = rng.uniform(800, 1200, (zb, xb))
    Eb = rng.standard_normal((m, zb, xb)) * 30
    Rb = Fb * rng.uniform(0.3, 1.0, (zb, xb))
    a = dm.means(Fb, Eb)
    for trial in range(4):
        w = rng.uniform(-2, 2, m)
        f, g, ab = dm.cost_w(Rb, Fb, Eb, w, a, 1e-3, round32=False)
        for j in range(m):
            h = 1e-6
            e = np.zeros(m)
            e[j] = h
            fd = (dm.cost_w(Rb, Fb, Eb, w + e, a, 1e-3, round32=False)[0] - dm.cost_w(Rb, Fb, Eb, w - e, a, 1e-3, round32=False)[0]) / (2 * h)
            assert abs(fd - g[j]) <= 1e-6 * ab[j], (trial, j, fd, g[j])


def test_model_gradient_drops_the_clamped_pixels_second_term():
    """A pixel whose D falls below 1e-6 is held there: its q no longer depends on the weights through D, only through s."""
    rng = np.random.default_rng(1)
    zb, xb, m = 5, 6, 2
    Fb = rng.uniform(800, 1200, (zb, xb))
    Eb = rng.standard_normal((m, zb, xb)) * 30
    Eb[0, 2, 3] = -5000.0
    Rb = Fb * rng.uniform(0.3, 1.0, (zb, xb))
    Rb[2, 3] = 5e-7                                   # q = 0.5 at the held pixel: of the size of its neighbours'
    a = dm.means(Fb, Eb)
    w = np.array([1.5, -0.5])
    assert Fb[2, 3] + w @ Eb[:, 2, 3] < 0
    f, g, ab = dm.cost_w(Rb, Fb, Eb, w, a, 1e-3, round32=False)
    for j in range(m):
        e = np.zeros(m)
        e[j] = 1e-6
        fd = (dm.cost_w(Rb, Fb, Eb, w + e, a, 1e-3, round32=False)[0] - dm.cost_w(Rb, Fb, Eb, w - e, a, 1e-3, round32=False)[0]) / 2e-6
        assert abs(fd - g[j]) <= 1e-6 * ab[j]


def test_binning_and_the_eigenvector_rule():
    src = np.arange(2 * 5 * 7, dtype=np.float32).reshape(2, 5, 7)
    dark = np.ones((5, 7), np.float32)
    b1 = dm.bin_frames(src, dark, 1)
    assert np.array_equal(b1, src - 1)
    b2 = dm.bin_frames(src, dark, 2)
    assert b2.shape == (2, 2, 3) and b2[0, 0, 0] == (0 + 1 + 7 + 8) - 4 and b2[1, 1, 2] == 4 * 35 + (18 + 19 + 25 + 26) - 4
    assert dm.bin_frames(src[0], None, 3).shape == (1, 2) and dm.bin_frames(src[0], None, 3)[0, 1] == sum(src[0, r, c] for r in range(3) for c in (3, 4, 5))
    G = np.array([[2.0, -1.0, 0.0], [-1.0, 2.0, -1.0], [0.0, -1.0, 2.0]])
    for lam, V in (dm.eigen(G), preprocess.eigen_decomposition(G)):
        assert np.all(np.diff(lam) <= 0) and np.allclose(G @ V, V * lam[None])
        for j in range(3):
            k = int(np.argmax(np.abs(V[:, j])))
            assert V[k, j] > 0
    assert dm.choose(np.array([100.0, 50.0, 3.0, 1.0, 1.0, 1.0, 0.9]), 2.0) == 3 == preprocess.count_eigen_flats(np.array([100.0, 50.0, 3.0, 1.0, 1.0, 1.0, 0.9]), 2.0)
    assert dm.choose(np.ones(5), 2.0) == 0 == preprocess.count_eigen_flats(np.ones(5), 2.0)
    assert preprocess.count_eigen_flats(np.array([9.0] * 10 + [1.0] * 11), 2.0) == preprocess.MAX_EFF == dm.MAX_EFF == 8


def test_eigenvalue_rule_on_a_drifting_beam(drifting):
    """The beam's centre moves in x and z: the leading eigenvalues stand far above the noise floor, and the first one the rule leaves
    out lies below eig_ratio x the median.  Measured: eigenvalue / median = 108, 88, 3.3 | 1.22, 1.11, ...: m = 3."""
    fbar = pm.reference_mean(drifting["flats"])
    lam, V = dm.eigen(dm.gram(drifting["flats"], fbar))
    m = dm.choose(lam, 2.0)
    med = float(np.median(lam))
    print("eigenvalue / median: %s -> m = %d" % (np.round(lam[:6] / med, 2).tolist(), m))
    assert 2 <= m <= dm.MAX_EFF
    assert lam[m - 1] > 2.0 * med >= lam[m]
    assert lam[0] > 20 * med                                    # the drift is no borderline case
    assert abs(V[:, :m].T @ V[:, :m] - np.eye(m)).max() < 1e-12
    E = dm.eff(drifting["flats"], fbar, V, m)
    c = dm.centered(drifting["flats"], fbar)
    scores = c @ E.reshape(m, -1).astype(np.float64).T / (E.reshape(m, -1).astype(np.float64) ** 2).sum(axis=1)[None]
    assert np.allclose((scores ** 2).mean(axis=0), 1.0, rtol=1e-4)      # the flats' own scores have unit mean square


def test_model_beats_the_conventional_normalisation(drifting):
    """The rms -log error against mu * projections, each projection's median error over its air pixels removed, with the automatically
    chosen m and the defaults (bin 2): at most 0.7 x the conventional normalisation's.  Measured: 0.0186 against 0.0318, ratio 0.585
    (seed 1: 0.515)."""
    truth, air = dm.truth_and_air(drifting)
    conv = dm.metric(pm.normalize(drifting["counts"], drifting["flats"], drifting["darks"]), truth, air)
    sino, W = dm.normalize_dynamic(drifting["counts"], drifting["flats"], drifting["darks"])
    dyn = dm.metric(sino, truth, air)
    print("rms -log error: conventional %.4f, dynamic %.4f (m = %d), ratio %.3f; largest |w| %.2f" % (conv, dyn, W.shape[1], dyn / conv, np.abs(W).max()))
    assert W.shape == (12, 3)
    assert dyn <= 0.7 * conv
    assert np.abs(W).max() < 10.0                                # no weight ran to the bound
    zero = dm.apply(drifting["counts"], pm.reference_mean(drifting["flats"]), pm.reference_mean(drifting["darks"]),
                    np.zeros((0, 48, 48), np.float32), np.zeros((12, 0)))
    assert np.array_equal(zero, pm.normalize(drifting["counts"], drifting["flats"], drifting["darks"]))


# ------------------------------------------------------------------------------------------------------------------ generate_data

PROJ = np.random.default_rng(0).uniform(0, 16, (6, 32, 5))


def test_make_raw_without_beam_drift_is_unchanged():
    a, b = generate_data.make_raw(PROJ, seed=3), generate_data.make_raw(PROJ, seed=3, beam_drift=0)
    c = generate_data.make_raw(PROJ, seed=3, beam_drift=0.0, n_flat=10)
    assert sorted(a) == sorted(b) == sorted(c)
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() == np.asarray(c[k]).tobytes(), k


def test_make_raw_beam_drift():
    clean, d = generate_data.make_raw(PROJ, seed=3), generate_data.make_raw(PROJ, seed=3, beam_drift=4.0, n_flat=7)
    assert d["flats"].shape == (7, 5, 32) and d["counts"].shape == clean["counts"].shape and d["counts"].dtype == np.uint16
    assert d["darks"].shape == clean["darks"].shape and d["mu"] == clean["mu"]
    again = generate_data.make_raw(PROJ, seed=3, beam_drift=4.0, n_flat=7)
    assert np.array_equal(again["counts"], d["counts"]) and np.array_equal(again["flats"], d["flats"])
    prof = generate_data.beam_profiles(3, 5, 32, 4.0, np.random.default_rng([3, 0x22]))
    assert prof.shape == (3, 5, 32) and prof.max() <= 1.0 and prof.min() >= 0.6
    centred = generate_data.beam_profiles(1, 5, 33, 0.0, np.random.default_rng(0))[0]
    assert centred[2, 16] == 1.0 and np.isclose(centred[2, 0], 0.6 + 0.4 * np.exp(-16.0 ** 2 / (2 * (0.6 * 33) ** 2)))
    # dimmer than the drift-free flats everywhere but at the beam's centre, by at most the profile's range
    ratio = (d["flats"].astype(np.float64).mean(axis=0) - 100) / (clean["flats"].astype(np.float64).mean(axis=0) - 100)
    assert 0.55 < ratio.min() and ratio.max() < 1.05 and ratio.mean() < 0.99
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="beam_drift"):
            generate_data.make_raw(PROJ, seed=3, beam_drift=bad)
    assert generate_data.make_raw(PROJ, seed=3, n_flat=0)["flats"].shape == (0, 5, 32)      # as before the option: not refused


def test_generate_data_arguments():
    a = generate_data.parse_args([])
    assert a.beam_drift == 0.0 and a.flats == 10
    a = generate_data.parse_args(["--raw", "--beam-drift", "6", "--flats", "20"])
    assert a.beam_drift == 6.0 and a.flats == 20
    assert generate_data.parse_args(["--raw", "--flats", "3"]).flats == 3
    for argv in (["--beam-drift", "6"], ["--raw", "--beam-drift", "-1"], ["--raw", "--beam-drift", "nan"], ["--raw", "--flats", "0"]):
        with pytest.raises(SystemExit):
            generate_data.parse_args(argv)


def test_examples_preprocess_dynamic_flat_arguments():
    assert ex_pre.parse_args(["raw.npz"]).dynamic_flat is None
    assert ex_pre.parse_args(["raw.npz", "--dynamic-flat"]).dynamic_flat == "auto"
    assert ex_pre.parse_args(["raw.npz", "--dynamic-flat", "auto"]).dynamic_flat == "auto"
    assert ex_pre.parse_args(["raw.npz", "--dynamic-flat", "3"]).dynamic_flat == 3
    assert ex_pre.parse_args(["raw.npz", "--dynamic-flat", "0"]).dynamic_flat == 0
    assert ex_pre.parse_args(["--dynamic-flat", "--out", "o.npz", "raw.npz"]).dynamic_flat == "auto"
    for argv in (["raw.npz", "--dynamic-flat", "-1"], ["raw.npz", "--dynamic-flat", "many"], ["raw.npz", "--dynamic-flat", "2", "--method", "median"]):
        with pytest.raises(SystemExit):
            ex_pre.parse_args(argv)
    data = dict(counts=np.zeros((2, 4, 4), np.uint16), flats=np.zeros((3, 4, 4), np.uint16), darks=np.zeros((2, 4, 4), np.uint16))
    for bad in ("all", -1, 1.5, True):
        with pytest.raises(ValueError, match="dynamic_flat"):
            ex_pre.run(data, dynamic_flat=bad)
    with pytest.raises(ValueError, match="method must be 'mean'"):
        ex_pre.run(data, dynamic_flat="auto", method="median")


# ------------------------------------------------------------------------------------------------------------------ the binding

def test_the_front_end_repeats_the_bindings_limits():
    assert (_dff_lib.MAX_FLATS, _dff_lib.MAX_EFF, _dff_lib.ERR_UNSUPPORTED) == (128, 8, 4) and preprocess.MAX_EFF == 8
    assert preprocess.DffUnsupported is _dff_lib.DffUnsupported


def test_the_library_refuses_what_it_does_not_take_with_the_reason():
    cases = [((1, 0, 16, 16, 1), "2 <= K <= 128"), ((129, 0, 16, 16, 1), "2 <= K <= 128"), ((5, -1, 16, 16, 1), "0 <= m <= 8"),
             ((20, 9, 16, 16, 1), "0 <= m <= 8"), ((5, 5, 16, 16, 1), "m <= K - 1 = 4"), ((5, 1, 16, 16, 0), "1 <= bin <= 8"),
             ((5, 1, 16, 16, 9), "1 <= bin <= 8"), ((5, 1, 3, 16, 2), "fewer than 2 x 2"), ((5, 1, 16, 7, 4), "fewer than 2 x 2"),
             ((5, 1, 0, 16, 1), "rows cols < 2\\^31"), ((5, 1, 65536, 32768, 1), "rows cols < 2\\^31")]
    for args, why in cases:
        with pytest.raises(_dff_lib.DffUnsupported, match=r"^libtomo_dff error 4: tomo_dff: .*" + why):
            _dff_lib.check(*args)
    _dff_lib.check(2, 1, 2, 2, 1)
    _dff_lib.check(128, 8, 16, 16, 8)
    _dff_lib.check(9, 8, 4096, 4096, 2)
    with pytest.raises(_dff_lib.DffUnsupported):
        _dff_lib.scratch_bytes(3, 16, 2)
    with pytest.raises(_dff_lib.DffUnsupported):
        _dff_lib.batch(5, 16, 16, 9)
    with pytest.raises(_dff_lib.DffUnsupported):
        _dff_lib.gram_chunk(1)


def test_batches_follow_the_budget_and_chunks_the_flats():
    """The binned counts of a projection are (rows // bin) (cols // bin) floats; a chunk of the Gram kernel is the largest multiple of 64
    pixels, at most 512 and at least 64, for which K rows of C + 1 floats and C more fit 32 KiB."""
    assert _dff_lib.scratch_bytes(37, 45, 1) == 4 * 37 * 45 and _dff_lib.scratch_bytes(37, 45, 2) == 4 * 18 * 22 and _dff_lib.scratch_bytes(37, 45, 3) == 4 * 12 * 15
    per = 4 * 18 * 22
    assert _dff_lib.batch(5, 37, 45, 2, 0) == 5 and _dff_lib.batch(5, 37, 45, 2, 1) == 1 and _dff_lib.batch(5, 37, 45, 2, per) == 1
    assert _dff_lib.batch(5, 37, 45, 2, 2 * per + 3) == 2 and _dff_lib.batch(5, 37, 45, 2, 100 * per) == 5
    assert [_dff_lib.gram_chunk(K) for K in (2, 3, 17, 20, 64, 128)] == [512, 512, 448, 384, 64, 64]
    for K in range(2, 129):
        C = _dff_lib.gram_chunk(K)
        assert C % 64 == 0 and 64 <= C <= 512 and (C == 64 or K * (C + 1) + C <= 8192)


# ---------------------------------------------------------------------------------------------------- refusals before any device

def _stacks(n=3, K=4, rows=8, cols=10, dtype=np.uint16):
    rng = np.random.default_rng(0)
    return (rng.integers(100, 1000, (n, rows, cols)).astype(dtype), rng.integers(900, 1100, (K, rows, cols)).astype(dtype),
            rng.integers(90, 110, (2, rows, cols)).astype(dtype))


def test_eigen_flats_checks_its_arguments_before_any_device():
    frames, flats, darks = _stacks()
    for kw, why in ((dict(n_eff=-1), "n_eff"), (dict(n_eff=1.5), "n_eff"), (dict(n_eff=True), "n_eff"), (dict(eig_ratio=0), "eig_ratio"),
                    (dict(eig_ratio=float("nan")), "eig_ratio"), (dict(eig_ratio="x"), "eig_ratio")):
        with pytest.raises(ValueError, match=why):
            preprocess.Preprocessor().eigen_flats(flats, darks, **kw)
    with pytest.raises(ValueError, match="uint16 or float32"):
        preprocess.Preprocessor().eigen_flats(flats.astype(np.float64), darks)
    with pytest.raises(ValueError, match="same frame shape"):
        preprocess.Preprocessor().eigen_flats(flats, darks[:, :, :9])
    with pytest.raises(ValueError, match="ctx"):
        preprocess.eigen_flats(flats, darks)                     # the result lives on the device: host flats need a context
    for f, kw in ((flats[:1], {}), (flats[0], {}), (np.zeros((129, 4, 4), np.uint16), {}), (flats, dict(n_eff=4)), (flats, dict(n_eff=9))):
        with pytest.raises(preprocess.DffUnsupported, match="nothing was launched"):
            preprocess.Preprocessor().eigen_flats(f, darks[:, :f.shape[-2], :f.shape[-1]], **kw)


def test_normalize_dynamic_checks_its_arguments_before_any_device():
    frames, flats, darks = _stacks()
    p = preprocess.Preprocessor()
    bad = [(dict(bin=0), preprocess.DffUnsupported, "bin"), (dict(bin=9), preprocess.DffUnsupported, "bin"),
           (dict(bin=5), preprocess.DffUnsupported, "fewer than 2 x 2"), (dict(bin=2.0), ValueError, "bin"), (dict(bin=True), ValueError, "bin"),
           (dict(n_eff=4), preprocess.DffUnsupported, "m <= K - 1"), (dict(n_eff=-1), ValueError, "n_eff"),
           (dict(tv_eps=0), ValueError, "tv_eps"), (dict(tv_eps=float("inf")), ValueError, "tv_eps"), (dict(w_max=0), ValueError, "w_max"),
           (dict(w_max=-1), ValueError, "w_max"), (dict(eig_ratio=-2), ValueError, "eig_ratio"),
           (dict(weights=np.zeros((2, 1))), ValueError, "weights"), (dict(weights=np.zeros(3)), ValueError, "weights"),
           (dict(weights=np.full((3, 1), np.nan)), ValueError, "weights"), (dict(weights=np.zeros((3, 2)), n_eff=1), ValueError, "columns"),
           (dict(weights=np.zeros((3, 4))), preprocess.DffUnsupported, "m <= K - 1"),
           (dict(min_ratio=0), ValueError, "min_ratio"), (dict(cutoff=float("nan")), ValueError, "cutoff"),
           (dict(crop=((0, 9), (0, 10))), ValueError, "crop"), (dict(max_scratch_bytes=-1), ValueError, "max_scratch_bytes"),
           (dict(out=np.zeros((3, 10, 8), np.float32)), ValueError, "out")]
    for kw, exc, why in bad:
        with pytest.raises(exc, match=why):
            p.normalize_dynamic(frames, flats, darks, **kw)
    with pytest.raises(ValueError, match="darks must be given"):
        p.normalize_dynamic(frames, flats)
    with pytest.raises(ValueError, match="frames' shape"):
        p.normalize_dynamic(frames[:, :7], flats, darks)
    with pytest.raises(ValueError, match="3 dimensions"):
        p.normalize_dynamic(frames[0], flats, darks)
    with pytest.raises(preprocess.DffUnsupported, match="2 <= K <= 128"):
        p.normalize_dynamic(frames, flats[:1], darks)
    assert p.ctx is None and p.handle is None and p._dff is None       # nothing was made

    class Freed(object):
        ctx, shape = None, (8, 10)

        def free(self):
            pass
    ef = preprocess.EigenFlats(Freed(), Freed(), Freed(), np.ones(4), 2)
    for kw, why in ((dict(darks=darks), "darks must be None"), (dict(n_eff=3), "exceeds the 2 fields"), (dict(weights=np.zeros((3, 3))), "exceeds the 2 fields"),
                    (dict(bin=True), "bin")):
        with pytest.raises(ValueError, match=why):
            p.normalize_dynamic(frames, ef, **kw)
    with pytest.raises(ValueError, match="frames' shape"):
        p.normalize_dynamic(frames[:, :, :9], ef)
    with pytest.raises(preprocess.DffUnsupported, match="fewer than 2 x 2"):
        p.normalize_dynamic(frames, ef, bin=5)
    with ef:
        pass
    assert ef.flat is None and ef.eff is None
    with pytest.raises(ValueError, match="freed"):
        p.normalize_dynamic(frames, ef)
    assert p.ctx is None and p._dff is None
