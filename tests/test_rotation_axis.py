"""The rotation-axis search without a GPU: the numpy model of tests/cor_model.py against scipy and against itself (half-spectrum against
the full transform, the mask's symmetries), that it recovers the axis of analytic ellipse sinograms, the separation condition every GPU
parity case of tests/test_gpu_rotation_axis.py relies on, the argument and angle checks of rotation_axis, and the handle-less calls of
libtomo_cor.so."""
import numpy as np
import pytest
import scipy.ndimage

import cor_model as cm

from oracle import oracle as orc

from tomography_alignment_amd import _cor_lib, _lib, rotation_axis
from tomography_alignment_amd.examples import generate_data

SHAPES, PARITY_SHAPES, OFFSETS = cm.SHAPES, cm.PARITY_SHAPES, cm.OFFSETS
GPU_TOLERANCE_D32 = 16.0          # tests/test_gpu_rotation_axis.py compares curves within 16 d32
SEPARATION = 50.0                 # ... and the two smallest values of a curve must be 50 times that apart
found = cm.found


def cases():
    for n, nx in SHAPES + cm.PARITY_SHAPES_WIDE:
        for off in OFFSETS:
            if (n, nx) == (24, 33) and abs(off) > 5.5:       # 2 |offset| reaches nx / 2 there
                continue
            yield n, nx, off


# ------------------------------------------------------------------------------------------------------------------- the model

@pytest.mark.parametrize("t", [0.5, -0.5, 3.5, -7.5, 2.25, 11.75])
def test_the_spline_shift_is_scipys(t):
    S = cm.ellipse_sinogram(37, 50, 3.25, seed=1, noise=0.02)
    flip = S[:, ::-1].astype(np.float64)
    ref = scipy.ndimage.shift(flip, (0, t), order=3, mode="mirror")
    got = cm.spline_shift(flip, t)
    keep = ~cm.filled_columns(50, t)
    err = float(np.max(np.abs(got[:, keep] - ref[:, keep])))
    print("t %g: max difference from scipy.ndimage.shift %.1e" % (t, err))
    assert err <= 1e-13 * np.max(np.abs(ref))
    coef = scipy.ndimage.spline_filter1d(flip, 3, axis=1, mode="mirror")
    assert np.max(np.abs(cm.spline_coefficients(flip) - coef)) <= 1e-13 * np.max(np.abs(coef))


def test_integer_shifts_are_exact_copies_and_both_sides_fill():
    S = cm.ellipse_sinogram(24, 33, 1.0, seed=3, noise=0.02)
    n, nx = S.shape
    for t in (0, 1, -1, 7, -12):
        M = cm.stack(S, t)
        assert M.dtype == np.float32 and M.shape == (2 * n, nx) and np.array_equal(M[:n], S)
        B = M[n:]
        for j in range(nx):
            if (t >= 0 and j < t) or (t < 0 and j >= nx + t):
                assert np.array_equal(B[:, j], S[::-1, j])
            else:
                assert np.array_equal(B[:, j], S[:, nx - 1 - (j - t)])
    assert cm.filled_columns(33, 2.25).sum() == 3 and cm.filled_columns(33, -2.25).sum() == 3 and cm.filled_columns(33, 0.0).sum() == 0


@pytest.mark.parametrize("n,nx", [(24, 33), (37, 50), (45, 96)])
def test_the_half_spectrum_sum_is_the_full_one(n, nx):
    S = cm.ellipse_sinogram(n, nx, 2.0, seed=4, noise=0.02)
    for t in (0, 3, -4.5):
        M = cm.stack(S, t)
        half, full = cm.metric_of_stack(M), cm.metric_full(M)
        print("(%d, %d) t %g: half %.15g full %.15g" % (n, nx, t, half, full))
        assert abs(half - full) <= 1e-12 * full


@pytest.mark.parametrize("R,nx", [(48, 33), (74, 50), (90, 96), (120, 48)])
def test_mask_facts(R, nx):
    for ratio, drop in ((0.5, 20), (1.0, 3), (0.25, 0)):
        W = cm.mask_full(R, nx, ratio, drop)
        kv = np.where(np.arange(R) <= R // 2, np.arange(R), np.arange(R) - R)
        ku = np.where(np.arange(nx) <= nx // 2, np.arange(nx), np.arange(nx) - nx)
        # symmetric under (kv, ku) -> (-kv, -ku): index k -> (-k) mod n; the Nyquist rows and columns map to themselves
        assert np.array_equal(W, W[(-np.arange(R)) % R][:, (-np.arange(nx)) % nx])
        assert not W[:, np.abs(ku) <= 1].any()
        cut = min(drop, int(np.ceil(0.05 * R)))
        assert not W[np.abs(kv) <= cut].any()
        # a monotone wedge: the columns that count in a row are 2 <= |ku| <= w, and w does not decrease with |kv|
        w, _ = cm.wedge(R, nx, ratio, drop)
        order = np.argsort(np.abs(kv), kind="stable")
        assert np.all(np.diff(w[order]) >= 0)
        for r in range(R):
            on = np.abs(ku)[W[r]]
            if on.size:
                assert abs(kv[r]) > cut and np.array_equal(np.sort(np.unique(on)), np.arange(2, min(w[r], nx // 2) + 1))
        assert W.any()


@pytest.mark.parametrize("n,nx,off", list(cases()))
def test_the_model_recovers_the_axis(n, nx, off):
    _, clean, _ = found(n, nx, off, 0.0)
    _, noisy, _ = found(n, nx, off, 0.02)
    print("(%d, %d) offset %g: noise-free %g, 2 %% noise %g" % (n, nx, off, clean.offset, noisy.offset))
    assert clean.offset == off
    assert abs(noisy.offset - off) <= 0.25                  # one step


@pytest.mark.parametrize("noise", [0.0, 0.02])
@pytest.mark.parametrize("n,nx", PARITY_SHAPES + cm.PARITY_SHAPES_WIDE)
def test_separation_condition_of_the_gpu_parity_cases(n, nx, noise):
    """An argmin comparison between the GPU and the model is fair only where rounding cannot decide it: the two smallest values of each
    curve are at least 50 x the GPU tolerance (16 d32) apart."""
    for off in OFFSETS:
        _, r64, r32 = found(n, nx, off, noise)
        d32 = cm.d32_of(r64, r32)
        gap = min(cm.gap(r64.coarse[1]), cm.gap(r64.fine[1]))
        print("(%d, %d) offset %g noise %g: d32 %.2e, smallest gap %.2e = %.0f x 16 d32" % (n, nx, off, noise, d32, gap, gap / (16 * d32)))
        assert 1e-9 < d32 < 1e-5
        assert gap >= SEPARATION * GPU_TOLERANCE_D32 * d32


# ------------------------------------------------------------------------------------------------------- arguments and angles

def test_angles_either_span_pi_or_include_the_endpoint():
    n = 90
    assert rotation_axis.angle_span(None, n) == n
    assert rotation_axis.angle_span(np.arange(n) * np.pi / n, n) == n
    assert rotation_axis.angle_span(0.3 + np.arange(n) * np.pi / n, n) == n
    assert rotation_axis.angle_span(np.linspace(0.0, np.pi, n), n) == n - 1                   # generate_data.make
    assert rotation_axis.angle_span(-np.linspace(0.0, np.pi, n), n) == n - 1
    for bad in (np.linspace(0.0, 2 * np.pi, n), np.linspace(0.0, 3.0, n), np.arange(n) * np.pi / n * (1 + 1e-5), np.arange(n - 1) * np.pi / n):
        with pytest.raises(ValueError):
            rotation_axis.angle_span(bad, n)
    uneven = np.arange(n) * np.pi / n
    uneven[7] += 1e-4 * np.pi / n
    with pytest.raises(ValueError, match="uniformly"):
        rotation_axis.angle_span(uneven, n)


def test_argument_errors_need_no_device():
    ok = dict(smin=-10, smax=10, srad=6, step=0.25)
    rotation_axis.check_arguments(60, 48, **ok)
    rotation_axis.check_arguments(60, 48, -17, 17, 6, 0.25)
    for bad in (dict(ok, smin=-18), dict(ok, smax=18), dict(ok, smin=3, smax=2), dict(ok, step=0.0), dict(ok, step=-1.0)):
        with pytest.raises(ValueError):
            rotation_axis.check_arguments(60, 48, **bad)
        with pytest.raises(ValueError):
            cm.check_arguments(60, 48, **bad)
    for n, nx in ((7, 48), (60, 15)):
        with pytest.raises(ValueError):
            rotation_axis.check_arguments(n, nx, -1, 1, 0, 0.25)
    # the public call refuses before it needs a context: none can be made here without a GPU, and none is asked for
    proj = np.zeros((60, 48, 3), np.float32)
    with pytest.raises(ValueError, match="smin"):
        rotation_axis.find_center(proj)                                # the defaults' +-50 do not fit 48 columns
    with pytest.raises(ValueError, match="step"):
        rotation_axis.find_center(proj, smin=-5, smax=5, step=0)
    with pytest.raises(ValueError, match="span pi"):
        rotation_axis.find_center(proj, angles=np.linspace(0, 1, 60), smin=-5, smax=5)
    with pytest.raises(ValueError, match="n >= 8"):
        rotation_axis.find_center(np.zeros((6, 48, 3), np.float32), smin=-5, smax=5)
    with pytest.raises(ValueError, match="rows"):
        rotation_axis.find_center(proj, rows=[3], smin=-5, smax=5)
    with pytest.raises(ValueError, match=r"\(n, nx, nz\)"):
        rotation_axis.find_center(np.zeros((60, 48), np.float32), smin=-5, smax=5)


def test_the_search_lists_and_helpers():
    assert np.array_equal(rotation_axis.coarse_list(-3, 2), cm.coarse_list(-3, 2)) and rotation_axis.coarse_list(-3, 2)[0] == -6.0
    for t0 in (-7.0, 0.0, 13.0):
        a, b = rotation_axis.fine_list(t0, 6, 0.25), cm.fine_list(t0, 6, 0.25)
        assert np.array_equal(a, b) and a.size == 49 and a[24] == t0 and a[0] == t0 - 12.0
    assert rotation_axis.widest_range(64) == (-25, 25) and rotation_axis.widest_range(2048) == (-50, 50)
    assert np.array_equal(rotation_axis.spread_rows(64, 9), np.arange(16, 49, 4)) and np.array_equal(rotation_axis.spread_rows(5, 1), [2])
    assert rotation_axis.spread_rows(3, 9).max() <= 2
    c = rotation_axis.to_cor_shift(2.5, 4)
    assert c.shape == (4, 3) and np.all(c[:, 0] == -2.5) and not c[:, 1:].any()
    r = rotation_axis.CenterResult([1.0, 3.0, 2.0], [0, 1, 2], 65)
    assert r.offset == 2.0 and r.center == 34.0


# ---------------------------------------------------------------------------------------------------------------- generate_data

class _OracleProjector(object):
    """utilities.projection_operators.ProjectionMatrix as generate_data.make uses it, on the CPU oracle: a function of its arguments
    (the HIP forward adds with float atomics and is not), so that equal arguments give equal bits.  It records the geometry it got."""
    seen = []

    def __init__(self, geom, precision=np.float32):
        type(self).seen.append(geom)
        self.geo = orc.Geo(geom.n_proj, np.asarray(geom.vox_shape), np.ones(3), np.asarray(geom.det_shape), np.ones(2),
                           cor_shift=np.asarray(geom.cor_shift, np.float64))

    def projection_matrix(self, alpha, beta, phi, xyz_shift):
        self.poses = dict(alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz_shift)
        return self

    def dot(self, x):
        vol = np.asarray(x, np.float64).reshape(tuple(int(v) for v in self.geo.vox_shape))
        return np.asarray(orc.forward(self.geo, vol, **self.poses), np.float32).ravel()


def test_generate_data_without_an_offset_is_what_it_was(monkeypatch):
    monkeypatch.setattr(generate_data.projection_operators, "ProjectionMatrix", _OracleProjector)
    _OracleProjector.seen = []
    a = generate_data.make(16, 12, seed=1)
    b = generate_data.make(16, 12, seed=1, cor_offset=0.0)
    c = generate_data.make(16, 12, seed=1, cor_offset=2.0)
    assert sorted(a) == sorted(b) == sorted(c) and float(a["cor_offset"]) == 0.0 and float(c["cor_offset"]) == 2.0
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    ga, gb, gc = _OracleProjector.seen
    assert not np.any(ga.cor_shift) and np.array_equal(ga.cor_shift, gb.cor_shift)
    assert np.array_equal(np.asarray(gc.cor_shift), np.tile([2.0, 0.0, 0.0], (12, 1)))
    for k in ("alpha", "beta", "xyz", "phi", "phantom"):
        assert np.array_equal(a[k], c[k]), k
    assert a["projections"].any() and not np.array_equal(a["projections"], c["projections"])
    with pytest.raises(ValueError):
        generate_data.make(16, 12, seed=1, cor_offset=float("nan"))


# ------------------------------------------------------------------------------------------------------------------ the binding

def test_handle_less_calls_raise_in_the_common_format():
    assert issubclass(_cor_lib.CorUnsupported, _lib.TomoError) and rotation_axis.CorUnsupported is _cor_lib.CorUnsupported
    for n, nx, ns in ((7, 64, 1), (64, 15, 1), (8193, 64, 1), (64, 8193, 1), (64, 64, 4097)):
        with pytest.raises(_cor_lib.CorUnsupported, match=r"^libtomo_cor error 4: tomo_cor"):
            _cor_lib.check_shape(n, nx, ns)
    _cor_lib.check_shape(8192, 8192, 4096)
    with pytest.raises(_lib.TomoError, match=r"^libtomo_cor error 1: tomo_cor_batch") as e:
        _cor_lib.batch(0, 64, 64)
    assert type(e.value) is _lib.TomoError
    # a shape beyond the limits is refused by the public call before it asks for a context
    with pytest.raises(_cor_lib.CorUnsupported):
        rotation_axis.find_center(np.zeros((8200, 64, 1), np.float32), smin=-5, smax=5)


@pytest.mark.parametrize("n,nx", [(24, 33), (37, 50), (45, 96), (900, 2048), (8, 16)])
def test_the_librarys_wedge_table_is_the_models(n, nx):
    for ratio, drop in ((0.5, 20), (1.0, 3), (0.3, 0)):
        w, cut = cm.wedge(2 * n, nx, ratio, drop)
        assert np.array_equal(_cor_lib.wedge(n, nx, ratio, drop), np.where(cut, 0, np.minimum(w, nx // 2)))


def test_batches_follow_the_budget():
    fb = 4 * 74 * 52                                  # one stacked (37, 50) sinogram in the R2C layout: 74 rows of 2 (25 + 1) floats
    assert _cor_lib.batch(21, 37, 50, 0) == 21 and _cor_lib.batch(21, 37, 50, 1) == 1 and _cor_lib.batch(21, 37, 50, 2 * fb) == 1
    assert _cor_lib.batch(21, 37, 50, 4 * fb) == 2 and _cor_lib.batch(21, 37, 50, 6 * fb + 5) == 3 and _cor_lib.batch(2, 37, 50, 100 * fb) == 2
