"""The work-group order of the gather-form flat forward (option "fwd_gather_patch": 0 plain, 1 automatic, 2 XCD patches of FPG projection
groups x FPR row tiles, kernels_tile_gather.hip.h).  The order decides which work-group computes a ray, never how it is summed: for every
case the sinograms of orders 0 and 2 must have the same bits, and one of them is held against the CPU oracle at the suite's bar
max|a - b| / max|b| < 1e-5, so that a mapping that drops the same rays in both orders cannot pass (tomo_forward zero-fills the sinogram: a
ray that no work-group owns shows as zeros against the oracle).  The cases are the edges of the patch grid: less than one patch, one
group / one row tile past a whole number of patches, detector rows that are no multiple of 8, lists padded with -1 where the poses jump,
empty lists, several z quads with an empty first one and regrouped z chunks, patch counts that are no multiple of the 8 XCDs, and
fractional translations (tau != 0: two edge atomics per chunk)."""
import numpy as np
import pytest

from conftest import rel_max

pytestmark = pytest.mark.gpu
TOL = 1e-5
FPG, FPR = 16, 4            # the kernel's patch: projection groups (of 8 poses) x row tiles (of 8 detector rows)
DEG = np.pi / 180.0


def n_patches(phi, ndx, nz):
    """Patches the host deals for these angles (all lists, all z quads), restating forward_tiles: a list per (walk, weight count), groups
    of eight entries, a list padded to the next group where it jumps to another range of poses."""
    entries = [0, 0, 0, 0]
    last = [None, None, None, None]
    for i, p in enumerate(phi):
        dx, dy = abs(np.sin(p)), abs(np.cos(p))
        ds, dl = max(dx, dy), min(dx, dy)
        l = 2 * (1 if dx < dy else 0) + (0 if 2 * dl <= ds else 1)
        if last[l] is not None and last[l] != i - 1:
            entries[l] = (entries[l] + 7) // 8 * 8
        entries[l] += 1
        last[l] = i
    nrt, nzq = (ndx + 7) // 8, (nz + 255) // 256 + 1
    groups = [(e + 7) // 8 for e in entries]
    return sum(((g + FPG - 1) // FPG) * ((nrt + FPR - 1) // FPR) * nzq for g in groups), groups


took_patches = {}           # order -> the last run_orders' launch of that order was dealt in patches


def run_orders(shape, ndx, phi, xyz, x, orders=(0, 2)):
    """{order: sinogram} for the given orders, and the oracle's."""
    from tomography_alignment_amd.utilities.geometry import Geometry
    from tomography_alignment_amd.utilities.projection_operators import ProjectionMatrix
    from oracle import oracle as orc
    n = len(phi)
    args = (n, np.array(shape), np.ones(3), np.array([ndx, shape[2]]), np.ones(2))
    kw = dict(alpha=np.zeros(n), beta=np.zeros(n), phi=np.asarray(phi, float), xyz_shift=xyz)
    got = {}
    took_patches.clear()
    for order in orders:
        P = ProjectionMatrix(Geometry(*args))
        ctx = P.backend.ctx
        ctx.set_option("fwd_gather_patch", order)
        ctx.profile_reset()
        ctx.profile_enable(True)
        got[order] = P.projection_matrix(**kw).dot(x.ravel())
        ctx.profile_enable(False)
        assert ctx.profile_get("k_fwd_tile_flat")[0] == 1 and ctx.profile_get("k_fwd_tile")[0] == 0, "one launch per forward"
        # which order the host took: a launch in patches is profiled as "k_fwd_tile_flat(patched)" (and counted under the plain name as well)
        took_patches[order] = ctx.profile_get("k_fwd_tile_flat(patched)")[0] == 1
    assert took_patches.get(0, False) is False and took_patches.get(2, True) is True, "option fwd_gather_patch does not select the order"
    return got, orc.forward(orc.Geo(*args), x, **kw).ravel()


def check(name, shape, ndx, phi, xyz, x):
    got, ref = run_orders(shape, ndx, phi, xyz, x)
    e = rel_max(got[2], ref)
    np_, groups = n_patches(phi, ndx, shape[2])
    print("%s: volume %s, %d rows, %d poses, groups per list %s, %d patches: patched vs oracle %.2e, zero rays %d / %d"
          % (name, shape, ndx, len(phi), groups, np_, e, int((got[2] == 0).sum()), got[2].size))
    assert np.array_equal(got[0].view(np.uint32), got[2].view(np.uint32)), "the two work-group orders give different bits"
    assert e < TOL
    return np_, groups


def vol(shape, seed):
    return np.random.default_rng(seed).uniform(0.1, 1.0, shape).astype(np.float32)


def zeros_xyz(n):
    return np.zeros((n, 3))


@pytest.mark.parametrize("ndx", [40, 24])        # 5 row tiles: one past a patch's; 3: fewer than a patch's
def test_fewer_than_one_patch(ndx):
    n = 9
    phi = np.random.default_rng(1).uniform(0.0, np.pi, n)
    _, groups = check("fewer than one patch", (40, 40, 70), ndx, phi, zeros_xyz(n), vol((40, 40, 70), 2))
    assert max(groups) < FPG and (ndx == 40 or (ndx + 7) // 8 < FPR)


@pytest.mark.parametrize("lo,hi,ndx,nz", [(64.0, 116.0, 8 * (FPR + 1), 64),     # x walk, three weights; FPR + 1 row tiles
                                          (27.0, 44.5, 8 * (FPR + 1) + 3, 64),  # y walk, four weights; a last row tile of 3 rows
                                          (45.5, 63.0, 8 * FPR + 1, 260)])      # x walk, four weights; a last row tile of 1 row; 3 z quads
def test_one_group_and_one_row_tile_past_whole_patches(lo, hi, ndx, nz):
    n = 8 * FPG + 1                                                             # FPG + 1 groups in ONE list
    phi = np.linspace(lo, hi, n) * DEG
    shape = (72, 72, nz) if nz == 64 else (40, 40, nz)
    np_, groups = check("remainders", shape, ndx, phi, zeros_xyz(n), vol(shape, 3))
    assert sorted(groups) == [0, 0, 0, FPG + 1] and FPR < (ndx + 7) // 8 <= 2 * FPR
    assert np_ == 2 * 2 * (2 if nz == 64 else 3)                                # 2 x 2 patches per z quad: 8, and with nz = 260 12 -- no multiple of the 8 XCDs


def test_four_lists_with_padded_groups():
    """Angles in random order: every list jumps between ranges of poses, and the host pads it with -1 up to the next group at each jump."""
    n = 96
    phi = np.random.default_rng(4).permutation(np.linspace(1.0, 179.0, n)) * DEG
    np_, groups = check("four lists, padded", (48, 40, 64), 8 * (FPR + 1), phi, zeros_xyz(n), vol((48, 40, 64), 5))
    assert min(groups) > 0 and sum(groups) > (n + 7) // 8 + 4                   # all four lists, and many more groups than whole ones
    assert max(groups) > FPG                                                    # ... so that a list has a padded group patch as well


def test_empty_lists():
    n = 11
    phi = np.random.default_rng(6).uniform(-20.0, 20.0, n) * DEG                # within 20 degrees of one axis: one walk, three weights
    _, groups = check("three lists empty", (40, 32, 64), 40, phi, zeros_xyz(n), vol((40, 32, 64), 7))
    assert sorted(groups)[:3] == [0, 0, 0]
    phi = np.concatenate([phi, np.linspace(100.0, 130.0, 9) * DEG])             # ... and with the other walk: two of four
    _, groups = check("one walk's four-weight list empty", (40, 32, 64), 40, phi, zeros_xyz(n + 9), vol((40, 32, 64), 7))
    assert sorted(groups)[0] == 0 and sorted(groups)[1] > 0


@pytest.mark.parametrize("nz,zero_below", [(300, 0), (300, 256), (520, 330)])
def test_z_quads(nz, zero_below):
    """nz is no multiple of 256; zero_below = 256: the first z quad is empty (its work-groups end at once); 330: the first live chunk is
    the sixth, so zshift regroups the chunks and the last layer of work-groups is used."""
    n = 9
    shape = (16, 24, nz)
    x = vol(shape, 8)
    x[:, :, :zero_below] = 0
    phi = np.random.default_rng(9).uniform(0.0, np.pi, n)
    xyz = zeros_xyz(n)
    xyz[:, 2] = np.random.default_rng(10).uniform(-5.0, 5.0, n)                 # rays of one chunk land in two chunks of the sinogram
    check("z quads", shape, 24, phi, xyz, x)


def test_fractional_translations():
    """tau != 0: a wave stores 63 values and completes the two it shares with its neighbours by one atomic from each side."""
    n = 8 * FPG + 1
    shape = (24, 24, 130)
    rng = np.random.default_rng(12)
    xyz = zeros_xyz(n)
    xyz[:, 0] = rng.uniform(-2.0, 2.0, n)
    xyz[:, 2] = rng.uniform(-2.0, 2.0, n)
    assert np.all(xyz[:, 2] != np.round(xyz[:, 2]))
    check("fractional translations", shape, 8 * FPR + 5, np.linspace(0.0, np.pi, n), xyz, vol(shape, 13))


def test_automatic_order_at_a_small_size_is_the_plain_one():
    n = 17
    shape = (40, 40, 70)
    phi = np.random.default_rng(14).uniform(0.0, np.pi, n)
    x = vol(shape, 15)
    got, ref = run_orders(shape, 40, phi, zeros_xyz(n), x, orders=(0, 1))       # (run_orders counts one k_fwd_tile_flat launch per forward)
    assert took_patches[1] is False, "the automatic order deals patches on a grid of a few patches"
    assert np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32))
    assert rel_max(got[1], ref) < TOL


def test_option_range():
    from tomography_alignment_amd.utilities.geometry import Geometry
    from tomography_alignment_amd.utilities.projection_operators import ProjectionMatrix
    ctx = ProjectionMatrix(Geometry(2, np.array([8, 8, 8]), np.ones(3), np.array([8, 8]), np.ones(2))).backend.ctx
    for bad in (-1, 3):
        with pytest.raises(Exception):
            ctx.set_option("fwd_gather_patch", bad)
    ctx.set_option("fwd_gather_patch", 1)
