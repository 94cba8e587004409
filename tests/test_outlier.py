"""CPU tests of the zinger removal and the 2-D median filter: the numpy model (tests/outlier_model.py) against scipy, argument
validation before anything is uploaded, the batch query, the zingers of examples/generate_data.py and the command-line options."""
import numpy as np
import pytest

import abi
import outlier_model as om

from tomography_alignment_amd import _prep_lib, preprocess
from tomography_alignment_amd.examples import generate_data
from tomography_alignment_amd.examples import preprocess as ex_pre


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("size", [3, 5, 7])
def test_median_model_equals_scipy_on_finite_data(dtype, size):
    ndimage = pytest.importorskip("scipy").ndimage
    rng = np.random.default_rng(size)
    shape = (3, 11, 17)
    if dtype == np.uint16:
        cases = [rng.integers(0, 4, shape).astype(np.uint16), rng.integers(0, 65536, shape).astype(np.uint16)]
    else:
        cases = [rng.integers(0, 4, shape).astype(np.float32), (rng.standard_normal(shape) * 1e3).astype(np.float32)]
    for a in cases:
        ref = ndimage.median_filter(a, size=(1, size, size), mode="reflect")
        got = om.median_filter(a, size)
        assert got.dtype == a.dtype and np.array_equal(om.bits(got), om.bits(ref))
        assert np.array_equal(om.median_filter(a[1], size), ref[1])          # one 2-D image


def test_model_orders_the_special_values_and_decodes_the_median():
    nan1, nan2 = np.array([0x7fc00001, 0xffc12345], np.uint32).view(np.float32)
    a = np.array([[-0.0, -0.0, 0.0], [-0.0, -1.0, 1.0], [2.0, -np.inf, 3.0]], np.float32)
    assert om.bits(om.median(a, 3))[1, 1] == 0                               # a median of -0 is written as +0
    a = np.array([[nan1, nan2, nan1], [nan2, 5.0, nan1], [1.0, 2.0, 3.0]], np.float32)
    assert om.bits(om.median(a, 3))[1, 1] == om.QUIET_NAN                    # five NaNs of nine: the median is the quiet NaN
    out, count = om.remove_outlier(a, np.inf)
    assert count == 5 and np.array_equal(np.isnan(out), np.isnan(om.median(a, 3)) & np.isnan(a))
    u = np.array([[0, 65535, 0], [65535, 65535, 0], [0, 65535, 0]], np.uint16)
    assert om.median(u, 3)[1, 1] == 0 and om.remove_outlier(u, 65535)[0][1, 1] == 0      # d == dif replaces
    assert om.remove_outlier(u, 65535, two_sided=False)[1] == np.sum(om.distance(u, 3)[1] >= 65535)


@pytest.mark.parametrize("kw, msg", [
    (dict(size=4), "size"), (dict(size=9), "size"), (dict(size=1), "size"), (dict(size=3.5), "size"), (dict(size=True), "size"),
    (dict(dif=-1.0), "dif"), (dict(dif=float("nan")), "dif"), (dict(dif="x"), "dif"), (dict(dif=None), "dif"),
    (dict(max_scratch_bytes=-1), "max_scratch_bytes"),
])
def test_remove_outlier_arguments_are_checked_before_anything_is_uploaded(kw, msg):
    args = dict(dif=10.0)
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        preprocess.remove_outlier(np.zeros((2, 8, 9), np.uint16), **args)


def test_outlier_rejects_bad_frames():
    for fn in (lambda a, **kw: preprocess.remove_outlier(a, 1.0, **kw), preprocess.median_filter):
        with pytest.raises(ValueError, match="uint16 or float32"):
            fn(np.zeros((2, 8, 9), np.int32))
        with pytest.raises(ValueError, match="dimensions"):
            fn(np.zeros((9,), np.float32))
        with pytest.raises(ValueError, match="dimensions"):
            fn(np.zeros((1, 2, 8, 9), np.float32))
        with pytest.raises(ValueError, match="smaller than the window"):
            fn(np.zeros((2, 4, 9), np.float32), size=5)
        with pytest.raises(ValueError, match="smaller than the window"):
            fn(np.zeros((6, 9), np.uint16), size=7)
        with pytest.raises(ValueError, match="size"):
            fn(np.zeros((2, 8, 9), np.float32), size=2)
        with pytest.raises(ValueError, match="out"):
            fn(np.zeros((2, 8, 9), np.float32), out=np.zeros((2, 8, 9), np.float32))


def test_batch_query():
    assert _prep_lib.outlier_batch(100, 200, _prep_lib.U16, 7, 0) == 7
    assert _prep_lib.outlier_batch(100, 200, _prep_lib.U16, 7, 100 * 200 * 2) == 1
    assert _prep_lib.outlier_batch(100, 200, _prep_lib.F32, 7, 100 * 200 * 2) == 1         # never fewer than one frame
    assert _prep_lib.outlier_batch(100, 200, _prep_lib.F32, 7, 100 * 200 * 4 * 3 + 5) == 3
    assert _prep_lib.outlier_batch(100, 200, _prep_lib.F32, 7, 1 << 40) == 7
    for bad in ((2, 200, _prep_lib.U16, 7), (100, 200, 2, 7), (100, 200, _prep_lib.U16, 0), (1 << 16, 1 << 15, _prep_lib.U16, 1)):
        with pytest.raises(_prep_lib.TomoError):
            _prep_lib.outlier_batch(*bad)


def test_binding_constants_match_the_header():
    limit = abi.parse_header(abi.header_path("prep")).constants["TOMO_PREP_MAX_OUTLIER_SIZE"]
    assert max(_prep_lib.OUTLIER_SIZES) == _prep_lib.MAX_OUTLIER_SIZE == limit


PROJ = np.random.default_rng(0).uniform(0, 16, (6, 32, 5))


def test_make_raw_without_zingers_is_unchanged():
    a, b = generate_data.make_raw(PROJ, seed=3), generate_data.make_raw(PROJ, seed=3, zingers=0)
    assert sorted(a) == sorted(b) == ["counts", "darks", "flats", "mu"]
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_make_raw_zingers():
    clean, d = generate_data.make_raw(PROJ, seed=3), generate_data.make_raw(PROJ, seed=3, zingers=4)
    mask = d["zinger_mask"]
    assert mask.dtype == bool and mask.shape == d["counts"].shape
    assert np.all(mask.reshape(mask.shape[0], -1).sum(axis=1) == 4)
    assert np.array_equal(d["counts"][~mask], clean["counts"][~mask])
    rise = d["counts"][mask].astype(np.int64) - clean["counts"][mask]
    assert np.all((rise >= 6000) & (rise <= 30000))                          # far below 65535 here: nothing was clipped
    changed = d["flats"] != clean["flats"]
    assert np.all(changed.reshape(changed.shape[0], -1).sum(axis=1) == 4)
    assert np.array_equal(d["darks"], clean["darks"]) and d["mu"] == clean["mu"]
    again = generate_data.make_raw(PROJ, seed=3, zingers=4)
    assert np.array_equal(again["counts"], d["counts"]) and np.array_equal(again["flats"], d["flats"])
    with pytest.raises(ValueError, match="zingers"):
        generate_data.make_raw(PROJ, seed=3, zingers=-1)
    assert "zinger_mask" in ex_pre.RAW_KEYS


def smooth_projections(n=24, nx=32, nz=32):
    """Projections [n][nx][nz] of a smooth object: a Gaussian blob that moves with the angle, up to 0.6 nx thick (a transmission of
    0.09 at make_raw's mu = 4 / nx)."""
    x = (np.arange(nx) - (nx - 1) / 2)[:, None] / (0.30 * nx)
    z = (np.arange(nz) - (nz - 1) / 2)[None, :] / (0.35 * nz)
    return np.stack([0.6 * nx * np.exp(-0.5 * ((x - 0.2 * np.cos(a)) ** 2 + z ** 2)) for a in np.linspace(0, np.pi, n)])


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("size", [3, 5])
def test_model_removes_exactly_the_zingers_of_a_smooth_object(size, seed):
    """What the threshold of the pipeline's test rests on: on make_raw's frames of a smooth object (i0 = 2e4, 4 zingers per frame) the
    model at dif = 3000 replaces exactly the zinger pixels and nothing in the zinger-free frames, for the windows 3 and 5 and four seeds
    (the largest d of a clean pixel is 1.1e3 - 2.2e3, the smallest of a zinger 5.6e3), and in the flats it replaces the zinger pixels and no other."""
    proj = smooth_projections()
    clean, data = generate_data.make_raw(proj, seed=seed), generate_data.make_raw(proj, seed=seed, zingers=4)
    assert om.removes_exactly_the_zingers(clean, data, 3000.0, size)
    flats, count = om.remove_outlier(data["flats"], 3000.0, size)
    assert np.all(count == 4) and np.array_equal(flats != data["flats"], data["flats"] != clean["flats"])
    assert not om.removes_exactly_the_zingers(clean, data, 30001.0, size)      # no zinger adds that much: the check can fail


def test_zingers_clip_at_the_top_of_the_range():
    frames = np.full((2, 4, 5), 65000, np.uint16)
    mask = generate_data.add_zingers(frames, 20, np.random.default_rng(0))
    assert mask.all() and np.all(frames == 65535)


def test_command_line_options():
    a = ex_pre.parse_args(["raw.npz", "--zinger-dif", "3000", "--zinger-size", "5"])
    assert (a.zinger_dif, a.zinger_size) == (3000.0, 5)
    a = ex_pre.parse_args(["raw.npz"])
    assert (a.zinger_dif, a.zinger_size) == (None, 3)
    for bad in (["raw.npz", "--zinger-dif", "-1"], ["raw.npz", "--zinger-dif", "nan"], ["raw.npz", "--zinger-dif", "3000", "--zinger-size", "4"],
                ["raw.npz", "--zinger-size", "9"]):
        with pytest.raises(SystemExit):
            ex_pre.parse_args(bad)
    g = generate_data.parse_args(["--raw", "--zingers", "3"])
    assert g.zingers == 3 and generate_data.parse_args([]).zingers == 0
    for bad in (["--zingers", "3"], ["--raw", "--zingers", "-1"]):
        with pytest.raises(SystemExit):
            generate_data.parse_args(bad)
