"""The direct-to-LDS loop of the gather adjoint (option "adj_gather_dma", k_adj_gather_flat<3, UPD, 1>, kernels_tile_gather.hip.h): the
sinogram rows of projection ip + 1 are loaded straight into one of two LDS row buffers while ip accumulates from the other.  It moves no
sum: for every case `tomo_adjoint` (and where named `tomo_adjoint_update`) runs with the option 0 and 1, the two results must have the
same bits, and the option-1 result is held against the CPU oracle at the suite's bar max|a - b| / max|b| < 1e-5, so that a row dropped in
both runs cannot pass.  The sinograms are random and nowhere zero unless a band is asked for: a row read before it landed, or a buffer
overwritten before its last reader, shows as different bits.  Which kernel a launch took is read from the profile: a direct-to-LDS launch
is recorded as "k_adj_gather_flat(dma)" (and counted under the plain name as well).

The host takes the loop when every pose has tau == 0 (integer z offsets), three samples per row suffice and the plan's largest
ea = (|cos phi| + |sin phi|) / det_dx is below 1.427 (13 rows per tile).  The declining cases are one fractional z translation among
integer ones, a step of 0.6 (six samples per row) and a pitch at which ea really passes 1.427: detector-x pitch 0.8 at 9 degrees from an
axis, ea = 1.4305 (still below the gather adjoint's own 1.45).  Detector-x pitch 1.25 -- where the loop was first expected to decline at
45 degrees -- has ea = sqrt 2 / 1.25 = 1.131 there: a coarser detector means FEWER rows per tile, the bound holds and the launch is a
direct-to-LDS one; the case is kept and checked as such."""
import numpy as np
import pytest

from conftest import rel_max

pytestmark = pytest.mark.gpu
TOL = 1e-5
DMA = "k_adj_gather_flat(dma)"
W4 = (9, 17, 256)                       # four z chunks: four live waves per work-group
# 45 degrees is where a tile touches its 13 rows; the list is cut to n poses from the front
ANGLES = [np.pi / 4 - 1e-3, 0.0, 3 * np.pi / 4 + 1e-3, np.pi / 2, np.pi / 4 + 1e-3, 3 * np.pi / 4 - 1e-3]


def angles(n, seed=0):
    return np.array((ANGLES + list(np.random.default_rng(seed).uniform(0.0, np.pi, max(0, n - len(ANGLES)))))[:n])


def sinogram(n, ndet, seed, band=None):
    y = np.random.default_rng(seed).standard_normal((n, ndet[0], ndet[1])).astype(np.float32)
    assert np.all(y != 0)
    if band is not None:
        y[:, :, :band[0]] = 0
        y[:, :, band[1]:] = 0
    return y.ravel()


class Case(object):
    """One geometry and pose set; run() gives {option: result} of an operation and the profile counts that go with it."""

    def __init__(self, shape, phi, xyz=None, ndet=None, det_pix=(1.0, 1.0), step=1.0):
        from tomography_alignment_amd import _lib
        from tomography_alignment_amd.utilities.geometry import Geometry
        from oracle import oracle as orc
        self.shape, self.n = shape, len(phi)
        self.ndet = (shape[0], shape[2]) if ndet is None else ndet
        self.xyz = np.zeros((self.n, 3)) if xyz is None else xyz
        args = (self.n, np.array(shape), np.ones(3), np.array(self.ndet), np.array(det_pix, np.float64))
        self.geo, self.og = Geometry(*args, step_size=step), orc.Geo(*args, step_size=step)
        self.kw = dict(alpha=np.zeros(self.n), beta=np.zeros(self.n), phi=np.asarray(phi, float), xyz_shift=self.xyz)
        self.poses = _lib.poses_array(self.kw["phi"], self.kw["alpha"], self.kw["beta"], self.xyz, np.zeros(3))
        self.n_vox = int(np.prod(shape))

    def oracle_adjoint(self, y):
        from oracle import oracle as orc
        return orc.adjoint(self.og, y, coloured_rows=self.n >= 32, **self.kw).ravel()      # (the threaded form for the one long case: same sums)

    def run(self, op):
        """op(backend) -> host result, once per option value -> ({0: ..., 1: ...}, {0: (launches, dma launches), 1: ...})"""
        from tomography_alignment_amd.backend import HipBackend
        got, took = {}, {}
        for dma in (0, 1):
            be = HipBackend(self.geo)
            ctx = be.ctx
            ctx.set_option("adj_gather_dma", dma)
            ctx.profile_reset()
            ctx.profile_enable(True)
            got[dma] = op(be)
            ctx.profile_enable(False)
            took[dma] = (ctx.profile_get("k_adj_gather_flat")[0], ctx.profile_get(DMA)[0])
            assert ctx.profile_get("k_adj_tile_flat")[0] == 0 and ctx.profile_get("k_adj_tile")[0] == 0, "a pose left the gather adjoint"
        return got, took


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def check_adjoint(name, case, y, expect_dma=True, launches=1):
    got, took = case.run(lambda be: be.adjoint(case.poses, be.upload(y), be.zeros(case.n_vox)).download())
    ref = case.oracle_adjoint(y)
    e = rel_max(got[1], ref)
    print("%s: volume %s, detector %s, %d poses: launches (all, direct-to-LDS) %s / %s, option 1 vs oracle %.2e, zero voxels %d / %d"
          % (name, case.shape, case.ndet, case.n, took[0], took[1], e, int((got[1] == 0).sum()), got[1].size))
    assert took[0] == (launches, 0), "option 0 must take the register kernel"
    assert took[1] == (launches, launches if expect_dma else 0), "the host took the other kernel than this case is meant for"
    assert same_bits(got[0], got[1]), "the two loops give different bits"
    assert np.abs(ref).max() > 0 and e < TOL
    return got[1]


def update_inputs(case, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(case.n_vox).astype(np.float32), rng.uniform(0.1, 1.0, case.n_vox).astype(np.float32),
            rng.standard_normal(case.n_vox).astype(np.float32))


def check_update(name, case, y, seed):
    """tomo_adjoint_update with clamp and ground truth: the bits of the volume, the error sum to 1e-13 relative (its double atomics arrive
    in any order), and the option-1 volume against rec + V * (oracle adjoint), clamped."""
    rec0, V, gt = update_inputs(case, seed)

    def op(be):
        rec = be.upload(rec0)
        fused, err = be.adjoint_update(case.poses, be.upload(y), rec, be.upload(V), True, be.upload(gt))
        assert fused
        return rec.download(), err

    got, took = case.run(op)
    ref = np.maximum(rec0.astype(np.float64) + V.astype(np.float64) * case.oracle_adjoint(y), 0.0)
    e = rel_max(got[1][0], ref)
    print("%s (fused update): launches %s / %s, option 1 vs oracle %.2e, error sums %.17g / %.17g" % (name, took[0], took[1], e, got[0][1], got[1][1]))
    assert took[0] == (1, 0) and took[1] == (1, 1)
    assert same_bits(got[0][0], got[1][0]), "the two loops give different bits"
    assert abs(got[0][1] - got[1][1]) <= 1e-13 * abs(got[0][1])
    assert np.count_nonzero(got[1][0] != rec0) > 0 and e < TOL
    # (the kernel's own sum: float32 differences, squared and added as doubles)
    assert abs(got[1][1] - float(np.sum((gt - got[1][0]).astype(np.float64) ** 2))) <= 1e-12 * got[1][1]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 9])
def test_loop_tails(n):
    """Odd and even tails of the loop's two passes, group tails for four live waves (groups of four projections)."""
    case = Case(W4, angles(n))
    check_adjoint("loop tails", case, sinogram(n, case.ndet, 10 + n))


@pytest.mark.parametrize("band,n", [((70, 120), 9), ((70, 180), 9), ((10, 180), 8), ((70, 180), 5)])
def test_live_waves(band, n):
    """Zero bands of the sinogram that leave 1, 2 and 3 live waves: groups of 1, 2 and 3 projections against the two passes."""
    case = Case(W4, angles(n, 1))
    check_adjoint("live waves, band %s" % (band,), case, sinogram(n, case.ndet, 20, band))


def zc_pm5(n):
    xyz = np.zeros((n, 3))
    xyz[:, 2] = np.where(np.arange(n) % 2 == 0, 5.0, -5.0)
    return xyz


BOTH_LOOPS = {"w4": (W4, None), "nz200": ((16, 5, 200), None), "ndz240": (W4, (9, 240)), "ndz300": ((9, 17, 200), (12, 300))}


def both_loops_case(key, n=9):
    shape, ndet = BOTH_LOOPS[key]
    return Case(shape, angles(n, 2), zc_pm5(n), ndet)


@pytest.mark.parametrize("key", sorted(BOTH_LOOPS))
def test_both_loops_in_one_launch(key):
    """Integer z offsets +5 and -5 in one call (tau == 0): the first and last z chunks are partly off the detector and take the register
    loop, the middle ones the direct-to-LDS loop, in the same work-groups.  nz = 200: the last chunk is partial; detectors lower (240)
    and higher (300, over a volume of 200 planes) than the volume."""
    case = both_loops_case(key)
    check_adjoint("both loops, " + key, case, sinogram(case.n, case.ndet, 30))


def test_declines_a_fractional_z_translation():
    n = 6
    xyz = zc_pm5(n)
    xyz[3, 2] = 1.5
    case = Case(W4, angles(n), xyz)
    check_adjoint("one tau != 0", case, sinogram(n, case.ndet, 40), expect_dma=False)


def test_declines_when_the_row_bound_fails():
    """Detector-x pitch 0.8 at 9 degrees from an axis: ea = 1.4305 >= 1.427, still a gather adjoint (< 1.45)."""
    phi = np.deg2rad([4.0, 9.0, 99.0, 171.0])
    ea = np.max((np.abs(np.cos(phi)) + np.abs(np.sin(phi))) / 0.8)
    assert 1.427 <= ea < 1.45
    case = Case(W4, phi, ndet=(11, 256), det_pix=(0.8, 1.0))
    check_adjoint("row bound", case, sinogram(4, case.ndet, 41), expect_dma=False)


def test_detector_pitch_125_at_45_degrees():
    """ea = 1.131 at 45 degrees: the bound holds (a coarser detector means fewer rows per tile), the launch is a direct-to-LDS one."""
    n = 6
    assert np.max((np.abs(np.cos(angles(n))) + np.abs(np.sin(angles(n)))) / 1.25) < 1.427
    case = Case(W4, angles(n), ndet=(7, 256), det_pix=(1.25, 1.0))
    check_adjoint("detector pitch 1.25", case, sinogram(n, case.ndet, 42), expect_dma=True)


def test_declines_six_samples_per_row():
    n = 6
    case = Case(W4, angles(n), step=0.6)
    check_adjoint("step 0.6", case, sinogram(n, case.ndet, 43), expect_dma=False)


@pytest.mark.parametrize("key", ["tails5", "tails8", "w4", "nz200"])
def test_fused_update(key):
    if key.startswith("tails"):
        n = int(key[5:])
        case = Case(W4, angles(n))
    else:
        case = both_loops_case(key)
    check_update(key, case, sinogram(case.n, case.ndet, 50), 51)


def test_two_x_slabs_equal_the_whole():
    n = 7
    shape = (24, 9, 256)                    # 24 voxels in x: two tile columns
    case = Case(shape, angles(n), zc_pm5(n))
    y = sinogram(n, case.ndet, 60)
    whole = check_adjoint("whole", case, y)

    def op(be):
        n_xt, _ = be.xslab_info()
        assert n_xt == 2
        d_y, d_v = be.upload(y), be.zeros(case.n_vox)
        for i in range(n_xt):
            be.adjoint_xslab(case.poses, d_y, d_v, i, i + 1, same_sinogram=i > 0)
        return d_v.download()

    got, took = case.run(op)
    e = rel_max(got[1], whole)
    print("two x slabs: launches %s / %s, summed vs the whole %.2e" % (took[0], took[1], e))
    assert took[0] == (2, 0) and took[1] == (2, 2)
    assert same_bits(got[0], got[1])
    assert e < 2e-6                         # the bar of the suite's slab sums


def test_mid_size():
    """128 x 128 x 256 with 64 angles: 512 work-groups, each running the pipeline for 64 projections -- long enough for an ordering
    mistake between loads and reads to show."""
    n = 64
    shape = (128, 128, 256)
    case = Case(shape, np.linspace(0.0, np.pi, n, endpoint=False))
    check_adjoint("mid-size", case, sinogram(n, case.ndet, 70))


def test_option_values():
    from tomography_alignment_amd.backend import HipBackend
    case = Case(W4, angles(2))
    be = HipBackend(case.geo)
    ctx = be.ctx
    y = sinogram(2, case.ndet, 80)

    def dma_launches():
        ctx.profile_reset()
        ctx.profile_enable(True)
        be.adjoint(case.poses, be.upload(y), be.zeros(case.n_vox))
        ctx.profile_enable(False)
        return ctx.profile_get(DMA)[0]

    assert dma_launches() == 1, "the default is 1"
    ctx.set_option("adj_gather_dma", 0)
    for bad in (-1, 2):
        with pytest.raises(Exception, match="error -2"):        # TOMO_ERR_ARG
            ctx.set_option("adj_gather_dma", bad)
    assert dma_launches() == 0, "a refused value must leave the option as it was"
    ctx.set_option("adj_gather_dma", 1)
    assert dma_launches() == 1
