"""The large-, dead- and all-stripe removal without a GPU: the numpy model of tests/stripe_model.py against independent code (np.polyfit,
scipy's uniform filter, np.interp, a restatement of Vo's algorithm 5 that sorts the normalised column again), its effect on a phantom
sinogram with dead and mis-gained columns, and the host logic: argument checks before any upload, generate_data's new arguments, the
example's --stripe options."""
import numpy as np
import pytest
from scipy import ndimage

import prep_model as pm
import stripe_model as sm

from tomography_alignment_amd import _prep_lib, preprocess
from tomography_alignment_amd.examples import generate_data
from tomography_alignment_amd.examples import preprocess as ex_pre


# ---- the model against independent code
@pytest.mark.parametrize("nx, seed", [(8, 0), (9, 1), (96, 2), (257, 3), (2048, 4)])
def test_line_fit_against_polyfit(nx, seed):
    rng = np.random.default_rng(seed)
    d = np.sort((1.0 + 0.05 * rng.standard_normal(nx)).astype(np.float32))[::-1].astype(np.float64)       # a sorted factor list
    nd = int(0.25 * nx)
    c, m = sm.line_fit(d, nd, nx - nd - 1)
    i = np.arange(nd, nx - nd - 1)
    m_ref, c_ref = np.polyfit(i, d[i], 1)
    print("nx %d: slope %.3e rel, intercept %.3e rel" % (nx, abs(m - m_ref) / abs(m_ref), abs(c - c_ref) / abs(c_ref)))
    assert abs(m - m_ref) <= 1e-9 * abs(m_ref) and abs(c - c_ref) <= 1e-9 * abs(c_ref)


def test_running_mean_against_scipy_uniform_filter():
    rng = np.random.default_rng(5)
    for n in (10, 11, 37, 180):
        p = rng.uniform(0.5, 4.0, (n, 7, 3)).astype(np.float32)
        ref = ndimage.uniform_filter1d(p.astype(np.float64), size=10, axis=0, mode="reflect")
        u = sm.running_mean(p)
        assert u.dtype == np.float32
        assert np.all(np.abs(u - ref) <= 1e-6 * np.abs(ref)), n


def test_interpolation_against_np_interp():
    rng = np.random.default_rng(6)
    p = rng.uniform(0.5, 4.0, (12, 40, 2)).astype(np.float32)
    mask = np.zeros((40, 2), bool)
    mask[[5, 6, 7, 20, 36, 37], 0] = True
    mask[[2, 3, 30], 1] = True
    out = sm.interpolate_columns(p, mask)
    for z in range(2):
        good = np.flatnonzero(~mask[:, z])
        for a in range(12):
            ref = np.interp(np.arange(40), good, p[a, good, z].astype(np.float64))
            assert np.all(np.abs(out[a, :, z] - ref) <= 1e-6 * np.abs(ref))
    assert np.array_equal(out[:, ~mask[:, 0], 0], p[:, ~mask[:, 0], 0])


def _large_by_resorting(sino, snr, size, drop_ratio):
    """Vo's algorithm 5 as the paper lists it, for one tie-free [n_proj][nx] sinogram: the NORMALISED sinogram is sorted again, column by
    column with its angle index, the smoothed sorted data are put in its place and sorted back by the index."""
    n, nx = sino.shape
    srt = np.sort(sino, axis=0)
    smooth = ndimage.median_filter(srt, (1, size), mode="reflect")
    nd = int(0.5 * np.clip(drop_ratio, 0.0, 0.8) * n)
    f = (srt[nd:n - nd].astype(np.float64).mean(axis=0) / smooth[nd:n - nd].astype(np.float64).mean(axis=0)).astype(np.float32)
    mask, _ = sm.detect(f, snr)
    normed = (sino / f[None]).astype(np.float32)
    out = normed.copy()
    for x in np.flatnonzero(mask):
        pairs = sorted(zip(normed[:, x], range(n)))                       # (value, angle), by value
        back = sorted(zip([a for _, a in pairs], smooth[:, x]))           # (angle, smoothed value at that rank), by angle
        out[:, x] = [v for _, v in back]
    return out, mask, normed


def test_large_pass_equals_the_paper_listing_where_the_division_merges_nothing():
    rng = np.random.default_rng(7)
    sino = (2.0 + np.sin(np.linspace(0, 3, 60))[:, None] * np.linspace(0.5, 1.5, 48)[None]
            + 0.01 * rng.standard_normal((60, 48))).astype(np.float32)
    sino[:, 17] *= 1.3
    sino[:, 33] *= 0.75
    assert all(np.unique(sino[:, x]).size == 60 for x in range(48))                # tie-free
    out, mask, _ = sm.remove_large_stripe(sino[:, :, None], 3.0, 11, 0.1, True)
    ref, mask_ref, normed = _large_by_resorting(sino, 3.0, 11, 0.1)
    assert mask[17, 0] and mask[33, 0] and np.array_equal(mask[:, 0], mask_ref)
    kept = np.array([np.unique(normed[:, x]).size == 60 for x in range(48)])       # columns where the division merged no two values
    assert kept[mask[:, 0]].any()
    assert np.array_equal(out[:, kept, 0], ref[:, kept])


# ---- effect
N_PX, N_ANG, I0 = 256, 180, 2e4
DEAD_COLS, GAIN_COLS = (40, 131, 200), (77, 150, 222)
# (density, semi-axes a and b, centre x and y, rotation) in pixels: a region-of-interest slice.  The body is wider than the detector, as
# the large-stripe factor l1 / l2 needs: in air both means are zero up to noise, their ratio is anything, and on a 256-px Shepp-Logan
# slice with its 10 air columns on each side the large-stripe detector flagged 23 % of the columns of stripe-free data.
ELLIPSES = ((0.375, 400, 500, 0, 0, 0.3), (-0.3, 60, 90, -30, 10, 0.5), (0.4, 25, 40, 50, -20, 1.0), (0.3, 15, 15, -10, 60, 0.0),
            (0.5, 8, 20, 20, 30, 2.0))


def ellipse_sinogram(ellipses, n_ang, n_px):
    """The exact line integrals [n_ang][n_px] of a sum of ellipses over 180 degrees."""
    t = np.arange(n_px) - (n_px - 1) / 2.0
    th = np.linspace(0, np.pi, n_ang, endpoint=False)[:, None]
    s = np.zeros((n_ang, n_px))
    for rho, a, b, x0, y0, phi in ellipses:
        a2 = (a * np.cos(th - phi)) ** 2 + (b * np.sin(th - phi)) ** 2
        tt = t[None] - (x0 * np.cos(th) + y0 * np.sin(th))
        s += 2 * rho * a * b / a2 * np.sqrt(np.maximum(a2 - tt ** 2, 0))
    return s


@pytest.fixture(scope="module")
def slices():
    sino = ellipse_sinogram(ELLIPSES, N_ANG, N_PX)
    rng = np.random.default_rng(1)
    mu = 1.6 / sino.max()                                                          # transmission between 0.2 and 0.37
    gain = np.ones(N_PX)
    gain[list(GAIN_COLS)] *= 1.25
    counts = rng.poisson(I0 * gain * np.exp(-mu * sino)).astype(np.float64)
    for j, c in enumerate(DEAD_COLS):
        counts[:, c] = I0 * (0.3 + 0.1 * j)
    defect = (-np.log(np.maximum(counts / I0, 1e-6))).astype(np.float32)[:, :, None]
    clean = (-np.log(np.maximum(rng.poisson(I0 * np.exp(-mu * sino)) / I0, 1e-6))).astype(np.float32)[:, :, None]
    return defect, clean


def test_all_removes_what_sorting_leaves(slices):
    defect, _ = slices
    out, dead_mask, large_mask, _ = sm.remove_all_stripe(defect, 3.0, 61, 21)
    assert all(dead_mask[c, 0] for c in DEAD_COLS)
    assert all(large_mask[c, 0] for c in GAIN_COLS)
    a_sort = pm.stripe_amplitude(pm.remove_stripe_sorting(defect, 21))
    a_all = pm.stripe_amplitude(out)
    print("stripe amplitude: input %.3e, sorting alone %.3e, all %.3e; dead mask %d columns, large mask %d columns"
          % (pm.stripe_amplitude(defect), a_sort, a_all, dead_mask.sum(), large_mask.sum()))
    assert a_all < a_sort


def test_all_leaves_clean_data_mostly_alone(slices):
    _, clean = slices
    out, dead_mask, large_mask, _ = sm.remove_all_stripe(clean, 3.0, 61, 21)
    flagged = (dead_mask | large_mask).sum() / float(N_PX)
    change = np.linalg.norm(out - clean) / np.linalg.norm(clean)
    print("clean slice: %.1f %% of the columns flagged, relative L2 change %.4f" % (100 * flagged, change))
    assert flagged <= 0.05


# ---- host logic
OK = np.zeros((12, 64, 3), np.float32)


@pytest.mark.parametrize("fn, kw, msg", [
    ("remove_large_stripe", dict(size=4), "odd"), ("remove_large_stripe", dict(size=65), "odd"),
    ("remove_dead_stripe", dict(size=20), "odd"), ("remove_all_stripe", dict(la_size=60), "la_size"),
    ("remove_all_stripe", dict(sm_size=22), "sm_size"), ("remove_all_stripe", dict(la_size=21.5), "odd integer"),
    ("remove_large_stripe", dict(snr=0), "snr"), ("remove_dead_stripe", dict(snr=-1.0), "snr"),
    ("remove_all_stripe", dict(snr=float("nan")), "snr"), ("remove_all_stripe", dict(snr=float("inf")), "snr"),
    ("remove_large_stripe", dict(snr="high"), "snr"), ("remove_large_stripe", dict(drop_ratio=float("nan")), "drop_ratio"),
    ("remove_large_stripe", dict(max_scratch_bytes=-1), "max_scratch_bytes"),
    ("remove_large_stripe", dict(out=np.zeros(OK.shape, np.float32)), "out must be"),
    ("remove_dead_stripe", dict(out=np.zeros(OK.shape, np.float32)), "out must be"),
    ("remove_all_stripe", dict(out="x"), "out must be"),
])
def test_arguments_are_checked_before_any_upload(fn, kw, msg):
    kw = dict({"size": 21} if "all" not in fn else {"la_size": 31}, **kw)
    with pytest.raises(ValueError, match=msg):
        getattr(preprocess, fn)(OK, **kw)
    with pytest.raises(ValueError, match=msg):
        getattr(preprocess.Preprocessor(), fn)(OK, **kw)


def test_shapes_are_checked_before_any_upload():
    for fn in ("remove_large_stripe", "remove_dead_stripe"):
        with pytest.raises(ValueError, match="odd"):
            getattr(preprocess, fn)(np.zeros((12, 10, 3), np.float32), size=11)                 # size > nx
        with pytest.raises(ValueError, match="nx >= 8"):
            getattr(preprocess, fn)(np.zeros((12, 7, 3), np.float32), size=3)
        with pytest.raises(ValueError, match="float32"):
            getattr(preprocess, fn)(np.zeros((12, 64, 3), np.uint16), size=3)
        with pytest.raises(ValueError, match="dimensions"):
            getattr(preprocess, fn)(np.zeros((12, 64), np.float32), size=3)
    with pytest.raises(ValueError, match="odd"):
        preprocess.remove_all_stripe(np.zeros((12, 32, 3), np.float32))                         # the default la_size 61 > nx
    with pytest.raises(ValueError, match="nx >= 8"):
        preprocess.remove_all_stripe(np.zeros((12, 7, 3), np.float32), la_size=3, sm_size=3)
    with pytest.raises(ValueError, match="n_proj >= 10"):
        preprocess.remove_dead_stripe(np.zeros((9, 64, 3), np.float32))
    with pytest.raises(ValueError, match="n_proj >= 10"):
        preprocess.remove_all_stripe(np.zeros((9, 64, 3), np.float32))
    preprocess._check_stripe_args(np.zeros((9, 64, 3), np.float32), 3.0, None, None, 1, "remove_large_stripe")     # 9 angles: large only
    for fn in ("remove_large_stripe", "remove_dead_stripe"):
        with pytest.raises(_prep_lib.PrepUnsupported, match="nothing was written"):
            getattr(preprocess, fn)(np.zeros((8193, 8, 1), np.float32), size=3)
        with pytest.raises(_prep_lib.PrepUnsupported, match="nothing was written"):
            getattr(preprocess, fn)(np.zeros((10, 8193, 1), np.float32), size=3)


def test_binding_table_has_the_new_entry_points():
    for method in ("stripe_large", "stripe_dead", "stripe_all"):
        assert callable(getattr(_prep_lib.PrepHandle, method))
    # 10 bytes per value and 13 per column: 3 rows of (19, 70) fit 3 * (10 * 19 + 13) * 70 bytes, 4 do not
    assert _prep_lib.stripe_all_chunk(19, 70, 70, 3 * (10 * 19 + 13) * 70) == 3
    assert _prep_lib.stripe_all_chunk(19, 70, 70, 0) == 70
    assert _prep_lib.stripe_chunk(19, 70, 70, 3 * 10 * 19 * 70) == 3              # the sorting pass's chunking keeps its meaning


def test_generate_data_defaults_are_bit_identical_and_defects_are_where_it_says():
    proj = np.random.default_rng(0).uniform(0, 16, (12, 48, 5))
    base = generate_data.make_raw(proj, seed=3)
    same = generate_data.make_raw(proj, seed=3, dead_columns=0, gain_columns=0)
    assert sorted(base) == sorted(same) == ["counts", "darks", "flats", "mu"]
    for k in base:
        assert np.array_equal(base[k], same[k]), k
    d = generate_data.make_raw(proj, seed=3, dead_columns=2, gain_columns=1)
    dead, gained = d["dead_cols"], d["gain_cols"]
    assert dead.size == 2 and gained.size == 1 and np.unique(np.concatenate([dead, gained])).size == 3
    assert dead.min() >= 4 and dead.max() < 44
    for c in dead:
        assert np.unique(d["counts"][:, :, c]).size == 1                              # stuck
    untouched = np.setdiff1d(np.arange(48), np.concatenate([dead, gained]))
    assert np.array_equal(d["counts"][:, :, untouched], base["counts"][:, :, untouched])
    assert np.array_equal(d["flats"], base["flats"]) and np.array_equal(d["darks"], base["darks"])
    ratio = (d["counts"][:, :, gained[0]].astype(float) - 100).mean() / (base["counts"][:, :, gained[0]].astype(float) - 100).mean()
    assert abs(ratio - generate_data.DEFECT_GAIN) < 0.02
    with pytest.raises(ValueError, match="dead_columns"):
        generate_data.make_raw(proj, seed=3, dead_columns=20)


def test_example_stripe_options():
    a = ex_pre.parse_args(["raw.npz"])
    assert (a.stripe, a.stripe_snr, a.stripe_size, a.stripe_la_size) == ("sorting", 3.0, 21, None)
    a = ex_pre.parse_args(["raw.npz", "--stripe", "all", "--stripe-snr", "2.5", "--stripe-size", "11", "--stripe-la-size", "31"])
    assert (a.stripe, a.stripe_snr, a.stripe_size, a.stripe_la_size) == ("all", 2.5, 11, 31)
    assert ex_pre.parse_args(["raw.npz", "--stripe", "none"]).stripe == "none"
    for bad in (["raw.npz", "--stripe", "some"], ["raw.npz", "--stripe-snr", "0"], ["raw.npz", "--stripe", "all", "--stripe-size", "0"],
                ["raw.npz", "--stripe-la-size", "30"]):
        with pytest.raises(SystemExit):
            ex_pre.parse_args(bad)
    assert ex_pre.la_size_for(2048) == 61 and ex_pre.la_size_for(32) == 31 and ex_pre.la_size_for(33) == 33 and ex_pre.la_size_for(64, 21) == 21
    with pytest.raises(ValueError, match="stripe must be"):
        ex_pre.run({"counts": 0, "flats": 0, "darks": 0}, stripe="some")
