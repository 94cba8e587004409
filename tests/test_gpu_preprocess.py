"""preprocess.py on the GPU (libtomo_prep.so) against the numpy models of tests/prep_model.py: reference frames and the normalisation bit
for bit (the log within 2e-6 relative), the stripe removal under np.array_equal over tie-heavy and signed-zero data, in place, chunked,
the 8192-angle limit, device residency with no leaked buffers, and generate_data --raw -> examples/preprocess -> FBP -> align_rigid.
Every path the host can choose for these kernels (frame groups, tiles, median windows, group widths, chunks): test_gpu_prep_paths.py."""
import numpy as np
import pytest

import prep_model as pm

from tomography_alignment_amd import _lib, _prep_lib, preprocess
from tomography_alignment_amd.examples import align_rigid, generate_data
from tomography_alignment_amd.examples import preprocess as ex_pre
from tomography_alignment_amd.recon import fbp
from tomography_alignment_amd.utilities.geometry import Geometry

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def pre(ctx):
    p = preprocess.Preprocessor(ctx)
    yield p
    p.close()


def _frames(rng, shape, dtype):
    if dtype == np.uint16:
        return rng.integers(0, 65536, shape).astype(np.uint16)
    return (rng.standard_normal(shape) * 1000).astype(np.float32)


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("n", [1, 2, 7, 20, 64])
def test_reference_frames_bitwise(pre, n, dtype):
    rng = np.random.default_rng(n)
    shape = (n, 13, 301)
    flats, darks = _frames(rng, shape, dtype), _frames(rng, shape, dtype)
    if dtype == np.uint16:
        flats[:, :3] = 7                               # ties
    for method in ("mean", "median"):
        f, d = pre.reference_frames(flats, darks, method)
        assert np.array_equal(f, pm.reference(flats, method)), method
        assert np.array_equal(d, pm.reference(darks, method)), method


def _raw_case(rng, n, nz, nx, dtype):
    flats = (rng.uniform(900, 1100, (5, nz, nx))).astype(dtype)
    darks = (rng.uniform(90, 110, (3, nz, nx))).astype(dtype)
    frames = rng.uniform(0, 1200, (n, nz, nx)).astype(dtype)
    frames.reshape(-1)[:: 7] = 0                      # zero counts
    frames.reshape(-1)[3:: 11] = 50                   # below dark
    if dtype == np.uint16:
        frames.reshape(-1)[5:: 13] = 65535            # saturated
    flats[0, 0, 0] = darks[0, 0, 0]                  # a dead flat pixel: den clamps to 1e-6
    return frames, flats, darks


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("nz, nx", [(1, 1), (7, 100), (33, 257), (1, 257), (33, 1)])
def test_normalize_against_the_model(pre, dtype, nz, nx):
    rng = np.random.default_rng(nz * 1000 + nx)
    frames, flats, darks = _raw_case(rng, 5, nz, nx, dtype)
    crops = [None]
    if nz > 2 and nx > 2:
        crops.append(((1, nz - 1), (2, nx)))
    for crop in crops:
        for cutoff in (None, 1.05):
            lin = pre.normalize(frames, flats, darks, cutoff=cutoff, minus_log=False, crop=crop)
            assert np.array_equal(lin, pm.normalize(frames, flats, darks, cutoff=cutoff, minus_log=False, crop=crop))
            lg = pre.normalize(frames, flats, darks, cutoff=cutoff, crop=crop)
            ref = pm.normalize(frames, flats, darks, cutoff=cutoff, crop=crop)
            assert lg.shape == ref.shape and np.all(np.isfinite(lg))
            assert np.all(np.abs(lg - ref) <= 2e-6 * np.maximum(1.0, np.abs(ref)))


def _stripe_gpu(ctx, pre, p, size, in_place=False, budget=None):
    d = ctx.to_device(p)
    out = d if in_place else None
    r = pre.remove_stripe_sorting(d, size=size, out=out, max_scratch_bytes=budget)
    host = r.download()
    d.free()
    r.free()
    return host


@pytest.mark.parametrize("n, nx, nz, size", [(1, 5, 3, 3), (2, 21, 7, 21), (90, 63, 33, 63), (181, 100, 5, 21), (1024, 30, 65, 3),
                                             (8192, 21, 3, 21)])
def test_stripe_removal_equals_the_model(ctx, pre, n, nx, nz, size):
    rng = np.random.default_rng(n + nx)
    p = (np.round(rng.standard_normal((n, nx, nz)) * 100) / 100).astype(np.float32)     # a few hundred levels: ties dominate
    p.reshape(-1)[::5] = 0.0
    p.reshape(-1)[1::9] = -0.0
    assert np.array_equal(_stripe_gpu(ctx, pre, p, size), pm.remove_stripe_sorting(p, size))


def test_stripe_in_place_and_chunked_are_bitwise_equal(ctx, pre):
    rng = np.random.default_rng(5)
    p = (np.round(rng.standard_normal((181, 70, 150)) * 30) / 30).astype(np.float32)
    p.reshape(-1)[::4] = -0.0
    ref = _stripe_gpu(ctx, pre, p, 11, budget=0)
    assert _prep_lib.stripe_chunk(181, 70, 150, 10 * 181 * 70 * 7) == 7
    chunked = _stripe_gpu(ctx, pre, p, 11, budget=10 * 181 * 70 * 7)
    inplace = _stripe_gpu(ctx, pre, p, 11, in_place=True, budget=10 * 181 * 70 * 64)
    assert np.array_equal(ref.view(np.uint32), chunked.view(np.uint32))
    assert np.array_equal(ref.view(np.uint32), inplace.view(np.uint32))
    assert np.array_equal(ref, pm.remove_stripe_sorting(p, 11))


def test_stripe_refuses_8193_angles_and_leaves_the_buffers(ctx, pre):
    p = np.random.default_rng(0).standard_normal((8193, 3, 2)).astype(np.float32)
    d = ctx.to_device(p)
    o = ctx.zeros(p.shape)
    with pytest.raises(_prep_lib.PrepUnsupported):
        pre.remove_stripe_sorting(d, size=3, out=o)
    assert np.array_equal(d.download(), p)
    assert not np.any(o.download())


def test_device_residency_and_no_leaks(ctx, pre):
    rng = np.random.default_rng(2)
    frames, flats, darks = _raw_case(rng, 6, 9, 40, np.uint16)
    d_frames, d_flats, d_darks = ctx.to_device(frames, np.uint16), ctx.to_device(flats, np.uint16), ctx.to_device(darks, np.uint16)
    before = len(ctx._arrays)
    sino = pre.normalize(d_frames, d_flats, d_darks)
    assert isinstance(sino, _lib.DeviceArray) and sino.shape == (6, 40, 9)
    assert len(ctx._arrays) == before + 1
    normalized = sino.download()
    again = pre.remove_stripe_sorting(sino, size=5)
    assert isinstance(again, _lib.DeviceArray)
    pre.remove_stripe_sorting(sino, size=5, out=sino)
    f, d = pre.reference_frames(d_flats, d_darks)
    assert isinstance(f, _lib.DeviceArray)
    host = sino.download()
    assert np.array_equal(host, again.download())
    assert np.array_equal(host, pm.remove_stripe_sorting(normalized, 5))     # the log differs from numpy's in the last bit
    for buf in (sino, again, f, d):
        buf.free()
    del sino, again, f, d, buf
    assert len(ctx._arrays) == before
    assert isinstance(preprocess.normalize(frames, flats, darks, ctx=ctx), np.ndarray)
    assert len(ctx._arrays) == before


def _fbp_rmse(data, proj):
    n, nx, nz = proj.shape
    geom = Geometry(n, np.array([nx, nx, nz]), np.ones(3), np.array([nx, nz]), np.ones(2))
    angles = np.zeros((n, 3))
    angles[:, 0] = data["phi"]
    rec = fbp.FBP(geom, proj, angles, np.zeros((n, 3))).run()
    gt = data["phantom"]
    c = (np.arange(nx) - (nx - 1) / 2.0)
    inside = (c[:, None] ** 2 + c[None, :] ** 2 < (0.45 * nx) ** 2)[:, :, None] * np.ones((1, 1, nz), bool)
    return float(np.sqrt(np.mean((rec - gt)[inside] ** 2)))


def test_end_to_end_raw_to_fbp_and_align_rigid(ctx):
    data = generate_data.make(64, 90, seed=0, ang_deg=0.0, shift_px=0.0, raw=True)
    with_stripes = ex_pre.run(data, stripe_size=0, ctx=ctx)
    corrected = ex_pre.run(data, stripe_size=21, ctx=ctx)
    assert "counts" not in corrected and corrected["projections"].shape == (90, 64, 64)
    a0, a1 = pm.stripe_amplitude(with_stripes["projections"]), pm.stripe_amplitude(corrected["projections"])
    assert a1 * 10 <= a0, (a0, a1)
    # At 64 px, size 21 spans a third of the detector: the median of the sorted profiles also bends the object's own structure, and the
    # FBP RMSE inside the cylinder went from 0.075 (stripes left in) to 0.115.  Bound the damage rather than assert a gain.
    e0, e1 = _fbp_rmse(data, with_stripes["projections"]), _fbp_rmse(data, corrected["projections"])
    assert np.isfinite(e1) and e1 < 2.0 * e0, (e0, e1)
    res = align_rigid.run(corrected, n_outer=1, sirt_iters=5, verbose=False, init="fbp")
    assert res is not None
