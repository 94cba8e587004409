"""align.consistency on the GPU (libtomo_mom.so) against the model of tests/mom_model.py, whose sums are correctly rounded: the marginals
bit for bit on exactly summable data, within (N - 1) 2^-53 sum |v| per sum of N terms on random float32 data, with a threshold, z
windows and planted non-finite values; identical bits across scratch budgets, handles, repeats, sub-stacks, the 16-byte and the 4-byte
load path and the host and device inputs; the handle's lifetime; and, end to end, the estimate on generate_data's +-10 px series,
align_rigid.run(prealign="moment"), examples/preprocess --prealign and run_multires(prealign=).  Every test prints the figures it
measured."""
import numpy as np
import pytest

import mom_model as mm

from tomography_alignment_amd import _lib, _mom_lib
from tomography_alignment_amd.align import consistency
from tomography_alignment_amd.examples import align_rigid, generate_data, preprocess

pytestmark = pytest.mark.gpu

# one lane (3, 5, 7); the 4-byte path with a z tail past a wave (2, 33, 65); an x tail past a tile of 128 and a z tail past two waves
# (5, 70, 130 is the 4-byte path, 130 = 2 * 64 + 2); several tiles, n = 1, nz odd (1, 129, 513); the 16-byte path (4, 64, 256)
# and past them (mm.GPU_SHAPES_WIDE): two row groups of a work-group (256 < nz <= 512) on both load paths, with one element in the
# second wave and with an x tail in the second group; two and three chunks of z, with one element in the last and on both load paths
SHAPES = mm.GPU_SHAPES + mm.GPU_SHAPES_WIDE
IDS = ["%dx%dx%d" % s for s in SHAPES]


def _chunks(nz):
    return -(-nz // _mom_lib.CHUNK_Z)


def _two_groups(nz):
    """groups_of of csrc/mom/tomo_mom.hip gives two row groups, of two waves of 256 z each, for these nz."""
    return 256 < nz <= 512


def test_the_shapes_reach_a_third_chunk_both_row_group_splits_and_a_second_tile():
    """Host only: the list reaches what its comment claims, so a change of the library's constants fails here and not silently."""
    assert any(_chunks(nz) >= 3 for _, _, nz in SHAPES) and any(_chunks(nz) == 2 for _, _, nz in SHAPES)
    assert any(_chunks(nz) >= 2 and nz % 4 == 0 for _, _, nz in SHAPES) and any(_chunks(nz) >= 2 and nz % 4 for _, _, nz in SHAPES)
    assert any(_two_groups(nz) and nz % 4 for _, _, nz in SHAPES) and any(_two_groups(nz) and nz % 4 == 0 for _, _, nz in SHAPES)
    assert any(nx > _mom_lib.TILE_X for _, nx, _ in SHAPES)
    assert any(nx > _mom_lib.TILE_X and _chunks(nz) >= 2 for _, nx, nz in SHAPES) and any(nx > _mom_lib.TILE_X and _two_groups(nz) for _, nx, nz in SHAPES)
    assert all(_chunks(s[2]) >= 2 or _two_groups(s[2]) for s in BIT_SHAPES[2:])


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def cons(ctx):
    c = consistency.Consistency(ctx)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(m, Q, Z, bad):
    return np.array_equal(_bits(m.Q), _bits(Q)) and np.array_equal(_bits(m.Z), _bits(Z)) and np.array_equal(m.bad, bad)


def _integers(shape, seed, lo=0, hi=1024):
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------- the marginals

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exactly_summable_data_give_the_models_bits(cons, shape):
    p = _integers(shape, 1)
    m = cons.marginals(p)
    Q, Z, bad = mm.marginals(p)
    dq, dz = int(np.count_nonzero(_bits(m.Q) != _bits(Q))), int(np.count_nonzero(_bits(m.Z) != _bits(Z)))
    print("%s: %d of %d values of Q and %d of %d of Z differ from the model" % (shape, dq, Q.size, dz, Z.size))
    assert m.Q.shape == Q.shape and m.Z.shape == Z.shape and m.Q.dtype == np.float64 and m.bad.dtype == np.int32
    assert dq == 0 and dz == 0 and not m.bad.any() and not bad.any()
    mass, cx, cz = mm.moments(Q, Z)
    assert np.max(np.abs(m.mass / mass - 1)) <= 1e-15 and np.max(np.abs(m.cx - cx)) <= 1e-12 and np.max(np.abs(m.cz - cz)) <= 1e-12


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_random_data_within_the_bound_of_float64_summation(cons, shape):
    """Any order of float64 additions of N terms is within (N - 1) 2^-53 sum |v| of the exact sum to first order; the model's sum is
    the exact one rounded.  The values span 18 decades: float32 values of one magnitude add exactly in float64, and nothing would round."""
    rng = np.random.default_rng(2)
    p = (rng.standard_normal(shape) * 10.0 ** rng.uniform(-9, 9, shape)).astype(np.float32)      # 18 decades, or float64 sums of float32 are exact
    m = cons.marginals(p)
    Q, Z, _ = mm.marginals(p)
    bq, bz = mm.sum_bounds(p)
    with np.errstate(invalid="ignore", divide="ignore"):
        fq = np.where(bq > 0, np.abs(m.Q - Q) / bq, np.where(m.Q == Q, 0.0, np.inf))
        fz = np.where(bz > 0, np.abs(m.Z - Z) / bz, np.where(m.Z == Z, 0.0, np.inf))
    print("%s: largest fraction of the bound, Q (sums of %d) %.3g, Z (sums of %d) %.3g" % (shape, shape[2], fq.max(), shape[1], fz.max()))
    assert np.all(np.abs(m.Q - Q) <= bq) and np.all(np.abs(m.Z - Z) <= bz)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_floor_window_and_non_finite_values(cons, shape):
    n, nx, nz = shape
    p = _integers(shape, 3, -512, 512)
    tail_x, tail_z = nx - 1, nz - 1                                   # past the last full tile, wave and 16-byte group where there is one
    planted = [((0, 0, 0), np.nan), ((n - 1, nx - 1, nz - 1), np.inf), ((n // 2, tail_x, nz // 2), -np.inf), ((0, nx // 2, tail_z), np.nan),
               ((n - 1, 0, min(1, nz - 1)), np.inf)]
    windows = [None, (1, nz - 1), (nz // 2, nz // 2 + 1), (0, 1), (nz - 1, nz), (2, min(nz, 5))]
    # windows that cut at the boundary of the first chunk or of the first wave of a row group, so that one chunk or wave takes the
    # path of a wave with nothing inside the window while its neighbour is live; non-finite values on either side of that boundary
    edge = _mom_lib.CHUNK_Z if _chunks(nz) > 1 else 256 if _two_groups(nz) else None
    if edge is not None:
        windows += [(edge, edge + 1), (edge - 1, edge + 1), (0, edge), (edge, nz)]
        planted += [((0, 0, edge), -np.inf), ((n - 1, nx // 2, edge - 1), np.nan), ((0, nx - 1, min(edge + 1, nz - 1)), np.inf)]
    for idx, v in planted:
        p[idx] = v
    checked = 0
    for floor in (None, 0.0, 17.5, -100.0):
        for zr in windows:
            m = cons.marginals(p, floor=floor, zrange=zr)
            Q, Z, bad = mm.marginals(p, floor, zr)
            assert _same(m, Q, Z, bad), (floor, zr, m.bad, bad)
            if zr is not None:
                assert not m.Z[:, :zr[0]].any() and not m.Z[:, zr[1]:].any()
            checked += 1
    full = cons.marginals(p)
    print("%s: %d (floor, window) pairs equal the model bit for bit; bad per projection without a window %s" % (shape, checked, full.bad.tolist()))
    assert int(full.bad.sum()) == len(set(i for i, _ in planted))
    assert np.all(np.isfinite(full.Q)) and np.all(np.isfinite(full.Z))
    if n >= 4:
        with pytest.raises(ValueError, match="non-finite"):
            consistency.shifts_from_marginals(full, np.linspace(0, np.pi, n))


# ------------------------------------------------------------------------------------------------------------------- determinism

# the last two are 16-byte shapes whose misaligned run takes the 4-byte loads across a chunk boundary and across the row-group split
BIT_SHAPES = [(5, 70, 130), (4, 64, 256), (3, 5, 1028), (3, 70, 512)]


@pytest.mark.parametrize("shape", BIT_SHAPES, ids=["4-byte loads", "16-byte loads", "two chunks", "two row groups"])
def test_budgets_handles_sub_stacks_and_paths_give_the_same_bits(ctx, cons, shape):
    n, nx, nz = shape
    p = (np.random.default_rng(4).standard_normal(shape) * 2.0 + 0.5).astype(np.float32)
    ref = cons.marginals(p, max_scratch_bytes=None)
    per = _mom_lib.scratch_bytes(nx, nz)
    assert _mom_lib.batch(n, nx, nz, 1) == 1 and _mom_lib.batch(n, nx, nz, per) == 1 and _mom_lib.batch(n, nx, nz, 0) == n
    results = {}
    for budget in (1, per, 2 * per + 1, None):
        results["budget %s" % budget] = cons.marginals(p, max_scratch_bytes=budget)
    cons.marginals(_integers((2, 33, 65), 5))                                       # another shape between the calls
    results["repeat"] = cons.marginals(p)
    with consistency.Consistency(ctx) as fresh:
        results["fresh handle"] = fresh.marginals(p)
    results["module level"] = consistency.marginals(p, ctx=ctx)
    results["module level, given handle"] = consistency.marginals(p, handle=cons)
    d = ctx.to_device(p)
    results["device"] = cons.marginals(d)
    results["flat device buffer"] = cons.marginals(d.view(0, d.size), shape=shape)
    # the same values four bytes further on: no 16-byte alignment, so the 4-byte loads even where nz % 4 == 0
    shifted = ctx.to_device(np.concatenate([np.zeros(1, np.float32), p.ravel()]))
    results["misaligned device buffer"] = cons.marginals(shifted.view(1, p.size), shape=shape)
    for name, m in results.items():
        diff = int(np.count_nonzero(_bits(m.Q) != _bits(ref.Q)) + np.count_nonzero(_bits(m.Z) != _bits(ref.Z)))
        print("%s %s: %d values differ from the unbatched run" % (shape, name, diff))
        assert diff == 0 and np.array_equal(m.bad, ref.bad), name
    sub_host = cons.marginals(p[1:3])
    sub_dev = cons.marginals(d.view(nx * nz, 2 * nx * nz), shape=(2, nx, nz))
    for name, m in (("host", sub_host), ("device", sub_dev)):
        assert np.array_equal(_bits(m.Q), _bits(ref.Q[1:3])) and np.array_equal(_bits(m.Z), _bits(ref.Z[1:3])), name
    assert np.array_equal(d.download(), p)                                          # the input is only read
    d.free()
    shifted.free()


def test_the_estimate_on_the_device_is_the_models(ctx, cons):
    """Analytic series in float32: the device's marginals and the module's estimator against the model's on the same values, both
    vertical modes; and against the true shifts at what float32 pixel values allow (relative 2^-24 per pixel: 1e-5 px is generous)."""
    n, nx, nz = 12, 96, 100
    phi = np.arange(n) * np.pi / n
    rng = np.random.default_rng(6)
    xyz = np.zeros((n, 3))
    xyz[:, 0], xyz[:, 2] = rng.uniform(-8, 8, n), rng.uniform(-8, 8, n)
    p = mm.ellipsoid_series(nx, nz, phi, xyz, dtype=np.float32)
    Q, Z, _ = mm.marginals(p)
    d = ctx.to_device(p)
    for vertical in ("moment", "profile"):
        got = cons.estimate_shifts(d, phi, vertical=vertical, return_marginals=True)
        ref = mm.estimate(Q, Z, phi, vertical=vertical)
        diff = float(np.max(np.abs(got.xyz0 - ref["xyz0"])))
        err = np.abs(consistency.gauge_fix(got.xyz0, phi) - consistency.gauge_fix(xyz, phi))
        print("%s: device minus model %.1e px; against the true shifts x %.1e z %.1e px" % (vertical, diff, err[:, 0].max(), err[:, 2].max()))
        assert diff <= 1e-9 and abs(got.axis_offset - ref["axis_offset"]) <= 1e-9 and got.marginals.Q.shape == (n, nx)
        assert err[:, 0].max() <= 1e-5 and err[:, 2].max() <= (1e-5 if vertical == "moment" else 1.0 / 20)
    d.free()


# ---------------------------------------------------------------------------------------------------------- refusals and lifetime

def test_refusals_come_before_any_launch(ctx, cons):
    p = _integers((4, 8, 12), 7)
    d = ctx.to_device(p)
    cons.marginals(d)
    before = cons.device_bytes()
    for kw in (dict(zrange=(0, 13)), dict(zrange=(5, 5)), dict(zrange=(-1, 4))):
        with pytest.raises(consistency.MomUnsupported):
            cons.marginals(d, **kw)
    with pytest.raises(ValueError):
        cons.marginals(d, floor=float("nan"))
    with pytest.raises(ValueError):
        cons.marginals(d.view(0, d.size))                                           # flat, and no shape
    with pytest.raises(ValueError):
        cons.marginals(d, shape=(4, 8, 13))
    with pytest.raises(ValueError):
        cons.estimate_shifts(d, np.linspace(0, 1.0, 4))
    h = _mom_lib.MomHandle(ctx.device)
    with pytest.raises(_lib.TomoError, match="no marginals were computed"):
        h.fetch(ctx.stream())
    with pytest.raises(_mom_lib.MomUnsupported):
        h.marginals(ctx.stream(), d.ptr, 4, 8, _mom_lib.MAX_NZ + 1)
    with pytest.raises(_lib.TomoError, match="misaligned"):
        h.marginals(ctx.stream(), d.ptr.value + 2, 4, 8, 12)
    assert h.device_bytes() == 0
    assert h.marginals(ctx.stream(), d.ptr, 4, 8, 12, fetch=False) is None              # enqueued only
    Q, Z, bad = h.fetch(ctx.stream())
    ref = mm.marginals(p)
    assert np.array_equal(Q, ref[0]) and np.array_equal(Z, ref[1]) and not bad.any() and h.device_bytes() > 0
    h.close()
    assert cons.device_bytes() == before and np.array_equal(d.download(), p)
    d.free()


def test_handle_lifetime():
    h = _mom_lib.MomHandle(0)
    assert h.handle and h.device == 0
    h.close()
    h.close()
    with pytest.raises(_lib.TomoError, match="^mom handle closed$"):
        h.handle
    with _mom_lib.MomHandle(0) as h2:
        assert h2.handle
    with pytest.raises(_lib.TomoError, match="^mom handle closed$"):
        h2.handle
    with pytest.raises(_lib.TomoError, match="device out of range"):
        _mom_lib.MomHandle(10**6)
    live = len(_lib.LIVE_CONTEXTS)
    p = consistency.Consistency()
    p._ready(None)
    c, hh = p.ctx, p.handle
    assert isinstance(hh, _mom_lib.MomHandle) and hh.handle and c.handle and len(_lib.LIVE_CONTEXTS) == live + 1
    p.close()
    assert p.ctx is None and p.handle is None and len(_lib.LIVE_CONTEXTS) == live
    with pytest.raises(_lib.TomoError, match="handle closed"):
        hh.handle
    with pytest.raises(_lib.TomoError, match="context closed"):
        c.handle
    p.close()
    given = _lib.Context(0)
    live = len(_lib.LIVE_CONTEXTS)
    with consistency.Consistency(given) as q:
        q._ready(None)
        hq = q.handle
        assert q.ctx is given and hq.device == given.device and len(_lib.LIVE_CONTEXTS) == live
    assert q.handle is None and q.ctx is given and given.handle and len(_lib.LIVE_CONTEXTS) == live
    with pytest.raises(_lib.TomoError, match="handle closed"):
        hq.handle
    given.close()


# ---------------------------------------------------------------------------------------------------------------------- end to end

def test_prealigned_run_on_10_px_of_jitter():
    """generate_data.make(64, 90, seed=3, shift_px=10.0): +-10 px of jitter, beyond the +-3 px the alignment searches.  The estimate
    equals the model's on the same projections; run(prealign="moment") must end below run(prealign=None) and below the pre-alignment's
    own starting error, all three gauge-fixed (shift_err_gauge_px)."""
    data = generate_data.make(64, 90, seed=3, shift_px=10.0)
    phi, proj = data["phi"], np.asarray(data["projections"], np.float32)
    est = consistency.estimate_shifts(proj, phi)
    ref = mm.estimate(*mm.marginals(proj)[:2], phi)
    diff = float(np.max(np.abs(est.xyz0 - ref["xyz0"])))
    start = align_rigid.gauge_shift_error(est.xyz0, data["xyz"], phi)
    print("estimate: device minus model %.1e px, mass spread %.2f %%, gauge-fixed starting error %.3f px" % (diff, 100 * est.mass_spread, start))
    assert diff <= 1e-9 and est.mass_spread > 0.01
    kw = dict(n_outer=2, sirt_iters=30, verbose=False, download=False)
    pre = align_rigid.run(dict(data), prealign="moment", return_loop=True, **kw)
    none = align_rigid.run(dict(data), prealign=None, return_loop=True, **kw)
    e_pre, e_none = pre[4][-1]["shift_err_gauge_px"], none[4][-1]["shift_err_gauge_px"]
    print("shift_err_gauge_px after 2 outer iterations: prealign='moment' %.3f px, prealign=None %.3f px; the start was %.3f px (plain "
          "shift_err_px: %.3f and %.3f px)" % (e_pre, e_none, start, pre[4][-1]["shift_err_px"], none[4][-1]["shift_err_px"]))
    assert np.array_equal(pre[5].base[0], est.xyz0) and not pre[5].base[1].any() and none[5].base is None
    assert e_pre < e_none
    assert e_pre < start


def test_the_drivers_carry_the_prealignment():
    """examples/preprocess --prealign stores the estimate of the finished sinogram (the division by mu afterwards rescales every pixel by
    one float32 rounding, which moves a centroid by far less than 1e-4 px), and run_multires starts its coarsest level from it."""
    data = generate_data.make(32, 24, seed=1, raw=True, shift_px=4.0)
    out = preprocess.run(dict(data), prealign="moment")
    assert out["xyz0"].shape == (24, 3) and not out["xyz0"][:, 1].any() and "counts" not in out
    est = consistency.estimate_shifts(out["projections"], data["phi"])
    diff = float(np.max(np.abs(out["xyz0"] - est.xyz0)))
    err = align_rigid.gauge_shift_error(out["xyz0"], data["xyz"], data["phi"])
    print("preprocess --prealign: xyz0 differs from the estimate on the stored projections by %.1e px; gauge-fixed error %.3f px, "
          "axis_offset %.3f, mass_spread %.3f" % (diff, err, float(out["axis_offset"]), float(out["mass_spread"])))
    assert diff <= 1e-4 and abs(float(out["axis_offset"]) - est.axis_offset) <= 1e-4 and abs(float(out["mass_spread"]) - est.mass_spread) <= 1e-4
    assert "xyz0" not in preprocess.run(dict(data))
    clean = generate_data.make(32, 24, seed=1, shift_px=4.0)
    res = align_rigid.run_multires(dict(clean), levels=2, n_outer=1, sirt_iters=5, verbose=False, download=False, prealign=out["xyz0"])
    hist = res[4]
    print("run_multires(levels=2, prealign=xyz0): shift_err_gauge_px %s" % [round(h["shift_err_gauge_px"], 3) for h in hist])
    assert [h["factor"] for h in hist] == [2, 1] and all(np.isfinite(h["shift_err_gauge_px"]) for h in hist)
    assert np.max(np.abs(res[3][:, [0, 2]] - out["xyz0"][:, [0, 2]])) <= 2 * 3.0 + 3.0          # each level moves at most its bounds from its base
