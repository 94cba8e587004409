"""The ingest kernels of libtomo_prep.so on every path the host can choose, against the numpy models of tests/prep_model.py at the bar of
test_gpu_preprocess.py: the same bits for the reference frames, the linear normalisation and the stripe removal (where an output may hold
NaN: the same NaN mask and the same bits elsewhere -- the kernels return one NaN, the model the input's), and
|gpu - model| <= 2e-6 max(1, |model|) for the -log.  The small functions below restate the host's choices in tomo_prep.hip; every case
asserts the path it was written for, and test_the_case_tables_reach_every_path that the tables together leave none out:
  reference_frames        1, 2, 3, 63, 64 frames of fewer, as many and more pixels than a 256-thread block; float32 stacks in which the odd
                          and the even median take NaN (of both signs), +-inf and +-0 at their middle ranks;
  normalize               every frame count around the 16-frame groups on detectors one below, at and one above the 64 x 64 tile, crops
                          that move the tile edges off the grid, NaN and +-inf counts, a flat below its dark;
  remove_stripe_sorting   all eight median windows W at size == W and padded, the z group widths of the sort (8192 / Np) and the scatter
                          (16384 / n, no power of two for n > 256), Np = 8192 with padding keys, chunks of 1, 64 and 128 rows, and one
                          handle's scratch over a large, a small and the large case again."""
import numpy as np
import pytest

import prep_model as pm

from tomography_alignment_amd import _lib, _prep_lib, preprocess

pytestmark = pytest.mark.gpu

f32 = np.float32
NEG_NAN = np.array([0xffc00000], np.uint32).view(f32)[0]        # what 0 / 0 gives on x86: the sign bit is set
POISON = np.array([0x7fc55a5a], np.uint32).view(f32)[0]         # a NaN no kernel here writes


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


# ---- the host's choices (tomo_prep.hip: median(), tomo_prep_stripe_sorting, tomo_prep_normalize, reference_t)
MEDIAN_W = (3, 7, 11, 15, 21, 31, 41, 63)
SORT_KEYS, SCATTER_VALS, MAX_ZC = 8192, 16384, 64
NORM_TILE, NORM_FR, REF_T = 64, 16, 256


def median_bucket(size):
    """The W of the k_stripe_median<W> that filters a window of `size`."""
    return next(w for w in MEDIAN_W if size <= w)


def sort_keys(n):
    """Np: the keys per z column of k_stripe_sort, n padded to a power of two."""
    Np = 1
    while Np < n:
        Np *= 2
    return Np


def sort_cols(n):
    """zc1: the z columns per work-group of k_stripe_sort."""
    return min(MAX_ZC, max(1, SORT_KEYS // sort_keys(n)))


def scatter_cols(n):
    """zc3: the z columns per work-group of k_stripe_scatter."""
    return min(MAX_ZC, max(1, SCATTER_VALS // n))


def norm_grid(n, nz, nx):
    """(tiles_z, tiles_x, groups) of k_normalize for n frames and a (cropped) window of nz rows and nx columns."""
    return (nz + NORM_TILE - 1) // NORM_TILE, (nx + NORM_TILE - 1) // NORM_TILE, (n + NORM_FR - 1) // NORM_FR


def ref_blocks(rows, cols):
    """The work-groups of k_reference_mean / k_reference_median."""
    return (rows * cols + REF_T - 1) // REF_T


def _pow2(v):
    return v & (v - 1) == 0


# ---- the comparisons
def assert_same_bits(got, ref):
    """The same NaN mask, and the same bits wherever the model is no NaN."""
    assert got.dtype == f32 and ref.dtype == f32 and got.shape == ref.shape
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], ref.view(np.uint32)[~nan])


def assert_log_close(got, ref):
    """The -log bar of test_normalize_against_the_model; what is not finite (-log(+inf) without a cutoff) must be the same value."""
    assert got.dtype == f32 and got.shape == ref.shape
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin)
    assert np.array_equal(got[~fin], ref[~fin])
    assert np.all(np.abs(got[fin] - ref[fin]) <= 2e-6 * np.maximum(1.0, np.abs(ref[fin])))


# ---- reference_frames
REF_FRAMES = {(1, 1): 1, (1, 255): 1, (1, 256): 1, (1, 257): 2, (3, 171): 3}      # (rows, cols): work-groups
REF_N = (1, 2, 3, 63, 64)


def _stack(rng, shape, dtype):
    if dtype == np.uint16:
        s = rng.integers(0, 65536, shape).astype(np.uint16)
        s[:, :, ::3] = rng.integers(6, 9, s[:, :, ::3].shape)      # every third column: three levels, ties at the middle ranks
        return s
    return (np.round(rng.standard_normal(shape) * 4) / 4 * 1000).astype(f32)            # a few dozen levels: ties


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("rows, cols", sorted(REF_FRAMES))
@pytest.mark.parametrize("n", REF_N)
def test_reference_frames_around_a_block(pre, n, rows, cols, dtype):
    assert ref_blocks(rows, cols) == REF_FRAMES[(rows, cols)]
    rng = np.random.default_rng(1000 * n + rows * cols)
    flats, darks = _stack(rng, (n, rows, cols), dtype), _stack(rng, (n, rows, cols), dtype)
    for method in ("mean", "median"):
        f, d = pre.reference_frames(flats, darks, method)
        assert_same_bits(f, pm.reference(flats, method))
        assert_same_bits(d, pm.reference(darks, method))


N_KINDS = 11


def _special_stack(rng, n, npix):
    """n frames of npix float32 pixels; pixel p holds pattern p % N_KINDS, placed on frames drawn at random."""
    f = (np.round(rng.standard_normal((n, npix)) * 4) / 4).astype(f32)
    k1, k2 = (n - 1) // 2, n // 2
    both = np.array([np.nan, NEG_NAN] * (n + 1), f32)

    def plant(p, vals):
        vals = np.asarray(vals, f32)[:n]
        f[rng.permutation(n)[:len(vals)], p] = vals

    for p in range(npix):
        kind = p % N_KINDS
        nans = both[(p // N_KINDS) % 2:]             # NaNs of both signs, either first
        if kind == 1:
            plant(p, nans[:n - k2])                   # the upper middle rank is NaN; for an even n the lower one is finite
        elif kind == 2:
            plant(p, nans[:n - k1])                   # both middle ranks are NaN
        elif kind == 3:
            plant(p, nans[:n - k2 - 1])               # one NaN fewer: the median is the largest value below them
        elif kind == 4:
            plant(p, [np.inf] * (n - k2))             # the upper middle rank is +inf
        elif kind == 5:
            plant(p, [-np.inf] * (k1 + 1))            # the lower middle rank is -inf
        elif kind == 6:
            plant(p, [-np.inf] * (k1 + 1) + [np.inf] * n)     # an even n: 0.5 (-inf + inf)
        elif kind == 7:
            f[:, p] = 0.0
            f[::2, p] = -0.0                          # -0 next to +0
        elif kind == 8:
            f[:, p] = rng.integers(1, 3, n)           # two levels
        elif kind == 9:
            plant(p, [np.nan, np.inf, -np.inf, -0.0, 0.0])
        elif kind == 10:
            f[:, p] = -0.0
    return f


@pytest.mark.parametrize("n", REF_N)
def test_reference_frames_of_nan_inf_and_signed_zeros(pre, n):
    rows, cols = 3, 171
    rng = np.random.default_rng(n)
    flats = _special_stack(rng, n, rows * cols).reshape(n, rows, cols)
    darks = np.ascontiguousarray(flats[::-1])            # the same medians, the mean summed in another order
    s = np.sort(flats, axis=0)                           # numpy sorts every NaN last, as the kernel's key does
    a, b = s[(n - 1) // 2], s[n // 2]
    assert np.isnan(a).any() and np.isinf(a).any() and np.isnan(b).any() and np.isinf(b).any()
    assert np.signbit(flats[np.isnan(flats)]).any() and not np.signbit(flats[np.isnan(flats)]).all()
    if n % 2 == 0:
        assert (np.isnan(b) & np.isfinite(a)).any() and (np.isinf(b) & np.isfinite(a)).any() and (np.isinf(a) & np.isfinite(b)).any()
    with np.errstate(all="ignore"):
        refs = {m: (pm.reference(flats, m), pm.reference(darks, m)) for m in ("mean", "median")}
    med = refs["median"][0]
    assert np.isnan(med).any() and (med == np.inf).any() and (med == -np.inf).any() and np.isfinite(med).any()
    for method in ("mean", "median"):
        fgot, dgot = pre.reference_frames(flats, darks, method)
        assert_same_bits(fgot, refs[method][0])
        assert_same_bits(dgot, refs[method][1])


def test_the_library_refuses_a_65_frame_median_and_writes_nothing(ctx, pre):
    stack = np.random.default_rng(0).standard_normal((65, 2, 3)).astype(f32)
    pre.reference_frames(stack[:1], stack[:1])           # the handle exists
    d, o = ctx.to_device(stack), ctx.to_device(np.full((2, 3), POISON))
    with pytest.raises(_prep_lib.PrepUnsupported):
        pre.handle.reference(ctx.stream(), d.ptr, _prep_lib.F32, 65, 2, 3, _prep_lib.MEDIAN, o.ptr)
    assert np.array_equal(o.download().view(np.uint32), np.full((2, 3), POISON).view(np.uint32))
    pre.handle.reference(ctx.stream(), d.ptr, _prep_lib.F32, 65, 2, 3, _prep_lib.MEAN, o.ptr)       # the mean has no such limit
    assert_same_bits(o.download(), pm.reference_mean(stack))
    d.free()
    o.free()


# ---- normalize
NORM_TILES = {(63, 65): (1, 2), (64, 64): (1, 1), (65, 63): (2, 1), (129, 70): (3, 2), (130, 129): (3, 3)}     # tiles_z, tiles_x
NORM_GROUPS = {1: 1, 15: 1, 16: 1, 17: 2, 33: 3, 48: 3}                                                     # frames: groups of 16
NORM_CASES = [(n, rows, cols) for rows, cols in sorted(NORM_TILES) if (rows, cols) != (130, 129) for n in sorted(NORM_GROUPS)]
NORM_CASES.append((17, 130, 129))
OFF_GRID_CROP = ((3, 3 + 64), (5, 5 + 65))           # on the 130 x 129 frame: one tile row and one tile column + 1, starting off the grid


def _clamped(rows, cols):
    """Pixels whose flat lies below the dark: one that every window crop holds, one on the one-row and the one-column crop."""
    return (10, 12), (rows - 1, cols - 2)


def _crops(rows, cols):
    crops = [None, ((1, rows), (0, cols - 1)), ((rows - 1, rows), (0, cols)), ((0, rows), (cols - 2, cols - 1))]
    if (rows, cols) == (130, 129):
        crops.append(OFF_GRID_CROP)
    return crops


def _raw(rng, n, rows, cols, dtype):
    """_raw_case of test_gpu_preprocess.py (zero counts, counts below dark, saturation, the dead flat pixel; flats and darks differ in
    every pixel, the frames from one another), with flats below their darks and, for float32, NaN and +-inf counts."""
    flats = rng.uniform(900, 1100, (5, rows, cols)).astype(dtype)
    darks = rng.uniform(90, 110, (3, rows, cols)).astype(dtype)
    frames = rng.uniform(0, 1200, (n, rows, cols)).astype(dtype)
    flat = frames.reshape(-1)
    flat[::7] = 0
    flat[3::11] = 50
    if dtype == np.uint16:
        flat[5::13] = 65535
    else:
        flat[17::101] = np.nan
        flat[29::103] = np.inf
        flat[31::107] = -np.inf
        flat[37::109] = NEG_NAN
    flats[0, 0, 0] = darks[0, 0, 0]
    for z, x in _clamped(rows, cols):
        flats[:, z, x] = 40                          # den < 1e-6: clamped
    return frames, flats, darks


@pytest.mark.parametrize("dtype", [np.uint16, np.float32])
@pytest.mark.parametrize("n, rows, cols", NORM_CASES)
def test_normalize_frame_groups_tiles_and_crops(ctx, pre, n, rows, cols, dtype):
    assert norm_grid(n, rows, cols) == NORM_TILES[(rows, cols)] + (NORM_GROUPS[n],)
    rng = np.random.default_rng(100000 * n + 1000 * rows + cols)
    frames, flats, darks = _raw(rng, n, rows, cols, dtype)
    mean_flat, mean_dark = pm.reference_mean(flats), pm.reference_mean(darks)
    assert all(mean_flat[p] < mean_dark[p] for p in _clamped(rows, cols))
    dev = [ctx.to_device(a, dtype) for a in (frames, flats, darks)]
    try:
        for crop in _crops(rows, cols):
            (z0, z1), (x0, x1) = crop if crop is not None else ((0, rows), (0, cols))
            if crop == OFF_GRID_CROP:
                assert norm_grid(n, z1 - z0, x1 - x0) == (1, 2, 2)
            oshape = (n, x1 - x0, z1 - z0)
            d_out = ctx.empty(oshape)
            for minus_log in (False, True):
                for cutoff in (None, 1.05):
                    kw = dict(cutoff=cutoff, minus_log=minus_log, crop=crop)
                    ref = pm.normalize(frames, flats, darks, **kw)
                    assert ref.shape == oshape
                    if dtype == np.float32 and crop is None and not minus_log and cutoff is None:
                        assert np.isnan(ref).any() and (ref == np.inf).any() and (ref == -np.inf).any()
                    if minus_log and cutoff is not None:
                        assert np.all(np.isfinite(ref))
                    host = pre.normalize(frames, flats, darks, **kw)
                    d_out.upload(np.full(oshape, POISON))             # a frame the kernel leaves out shows
                    assert pre.normalize(*dev, out=d_out, **kw) is d_out
                    for got in (host, d_out.download()):
                        if minus_log:
                            assert_log_close(got, ref)
                        else:
                            assert_same_bits(got, ref)
            d_out.free()
    finally:
        for d in dev:
            d.free()


# ---- remove_stripe_sorting
STRIPE_CASES = [      # (n, nx, nz, size), (Np, zc1, zc3, W)
    ((4097, 9, 3, 5), (8192, 1, 3, 7)),            # Np = 8192 with padding keys, the narrowest groups, W = 7 padded
    ((5000, 8, 2, 7), (8192, 1, 3, 7)),            # the same at size == W
    ((300, 9, 120, 9), (512, 16, 54, 11)),         # zc3 no power of two; nz ragged against zc1 and zc3; W = 11 padded
    ((5, 66, 3, 11), (8, 64, 64, 11)),             # W = 11 at size == W, two x tiles
    ((257, 200, 2, 15), (512, 16, 63, 15)),        # W = 15; four x tiles with a ragged last
    ((129, 70, 65, 13), (256, 32, 64, 15)),        # W = 15 padded; nz one past a z tile; nx one tile + 6
    ((4, 40, 5, 19), (4, 64, 64, 21)),             # W = 21 padded
    ((5, 21, 3, 21), (8, 64, 64, 21)),             # W = 21 at size == W == nx
    ((6, 67, 2, 29), (8, 64, 64, 31)),             # W = 31 padded, the halo crosses the tile edge
    ((3, 130, 129, 31), (4, 64, 64, 31)),          # W = 31; nx two tiles + 2; three z tiles
    ((17, 64, 64, 41), (32, 64, 64, 41)),          # W = 41; exactly one tile in both directions
    ((17, 65, 64, 33), (32, 64, 64, 41)),          # W = 41 padded; one column past a tile
    ((33, 65, 70, 61), (64, 64, 64, 63)),          # W = 63 padded
    ((2, 63, 1, 63), (2, 64, 64, 63)),             # size == nx: every window is reflected on both sides
    ((1, 8, 1, 3), (1, 64, 64, 3)),                # Np = 1: nothing to sort
    ((2, 8, 64, 3), (2, 64, 64, 3)),
    ((3, 8, 65, 3), (4, 64, 64, 3)),
]
CHUNK_SHAPE = (90, 20, 150)


def _sino(rng, shape):
    """test_stripe_removal_equals_the_model's tie-heavy data with both zeros, and infinities of both signs."""
    p = (np.round(rng.standard_normal(shape) * 100) / 100).astype(f32)
    flat = p.reshape(-1)
    flat[::5] = 0.0
    flat[1::9] = -0.0
    flat[7::97] = np.inf
    flat[11::89] = -np.inf
    return p


def _stripe_gpu(ctx, pre, p, size, in_place=False, budget=None):
    d = ctx.to_device(p)
    r = pre.remove_stripe_sorting(d, size=size, out=d if in_place else None, max_scratch_bytes=budget)
    host = r.download()
    d.free()
    r.free()
    return host


@pytest.mark.parametrize("case, path", STRIPE_CASES, ids=["-".join(str(v) for v in c) for c, _ in STRIPE_CASES])
def test_stripe_removal_on_every_window_and_group_width(ctx, pre, case, path):
    n, nx, nz, size = case
    assert (sort_keys(n), sort_cols(n), scatter_cols(n), median_bucket(size)) == path
    p = _sino(np.random.default_rng(n + nx + nz), (n, nx, nz))
    ref = pm.remove_stripe_sorting(p, size)
    assert not np.isnan(ref).any()
    assert_same_bits(_stripe_gpu(ctx, pre, p, size), ref)


def test_stripe_chunks_of_1_64_and_128_rows(ctx, pre):
    n, nx, nz = CHUNK_SHAPE
    per_z = 10 * n * nx
    budgets = {64: 100 * per_z, 128: 140 * per_z, 1: 2 * per_z - 1}           # the raw quotients 100 and 140 are cut to whole 64-row tiles
    for zc, budget in budgets.items():
        assert _prep_lib.stripe_chunk(n, nx, nz, budget) == zc
    assert _prep_lib.stripe_chunk(n, nx, nz, 0) == nz
    p = _sino(np.random.default_rng(7), CHUNK_SHAPE)
    whole = _stripe_gpu(ctx, pre, p, 9, budget=0)
    for budget in budgets.values():
        assert np.array_equal(_stripe_gpu(ctx, pre, p, 9, budget=budget).view(np.uint32), whole.view(np.uint32))
        assert np.array_equal(_stripe_gpu(ctx, pre, p, 9, in_place=True, budget=budget).view(np.uint32), whole.view(np.uint32))
    assert_same_bits(whole, pm.remove_stripe_sorting(p, 9))


def test_one_handle_keeps_its_bits_over_large_small_large(ctx):
    """The scratch grows for the first call and is kept for the two that follow, all enqueued on the context's stream before any result
    is read."""
    rng = np.random.default_rng(11)
    large, small = _sino(rng, (300, 9, 120)), _sino(rng, (3, 8, 65))
    with preprocess.Preprocessor(ctx) as own:
        d_large, d_small = ctx.to_device(large), ctx.to_device(small)
        outs = [own.remove_stripe_sorting(d, size=s) for d, s in ((d_large, 9), (d_small, 3), (d_large, 9))]
        got = [o.download() for o in outs]
        for d in [d_large, d_small] + outs:
            d.free()
    ref_large = pm.remove_stripe_sorting(large, 9)
    assert_same_bits(got[0], ref_large)
    assert_same_bits(got[1], pm.remove_stripe_sorting(small, 3))
    assert_same_bits(got[2], ref_large)


# ---- the tables against the dispatch
def test_the_case_tables_reach_every_path():
    sizes = [c[3] for c, _ in STRIPE_CASES]
    for w in MEDIAN_W:
        assert any(s == w for s in sizes), "no case with size == W = %d" % w
        if w > 3:                                    # 3 is the smallest window there is
            assert any(s < w and median_bucket(s) == w for s in sizes), "no padded case for W = %d" % w
    ns = [c[0] for c, _ in STRIPE_CASES] + [CHUNK_SHAPE[0]]
    zc3 = [scatter_cols(n) for n in ns]
    assert any(_pow2(z) for z in zc3) and any(not _pow2(z) for z in zc3)
    assert any(sort_keys(n) == SORT_KEYS and n < SORT_KEYS for n in ns)
    assert {1, MAX_ZC} <= {sort_cols(n) for n in ns} and any(1 < sort_cols(n) < MAX_ZC for n in ns)
    assert any(nz % sort_cols(n) and nz % scatter_cols(n) and nz > max(sort_cols(n), scatter_cols(n)) for (n, _, nz, _), _ in STRIPE_CASES)
    assert {1, 2, 4} <= {sort_keys(n) for n in ns}
    grids = [norm_grid(n, rows, cols) for n, rows, cols in NORM_CASES]
    assert any(min(g) > 1 for g in grids)
    assert any(n % NORM_FR and n > NORM_FR for n, _, _ in NORM_CASES) and any(n % NORM_FR == 0 and n > NORM_FR for n, _, _ in NORM_CASES)
    assert {1, 2, 3} <= {ref_blocks(*s) for s in REF_FRAMES} and any(r * c % REF_T == 0 for r, c in REF_FRAMES)
