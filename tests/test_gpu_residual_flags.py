"""The residual pass that also notes the sinogram's non-empty detector planes (tomo_vec_residual_scale_flags): the back-projection that
follows takes the note instead of its own pass over the sinogram (k_sino_zflags) and computes the same bits as with that pass; the note
does not survive anything that could have written the sinogram in between."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PHI = np.array([0.0, 0.4, np.pi / 4, np.pi / 2, 2.0, 2.7, np.pi])
ZSHIFT = np.array([0.0, 3.0, -2.5, 0.6, -4.0, 1.25, 2.0])
SHAPE = (20, 27, 150)
# detector (ndx, ndz) -> is the note taken?  The vector passes run min(ceil(n / 256), 2048) work-groups of 256 threads.
#   36 x 128: stride = n, a multiple of 128, every thread has one value;  160 x 512: n = 573 440 > the capped stride 2^19, threads loop;
#   36 x 150: stride 148 * 256 is no multiple of 150 -- a thread meets many planes, nothing may be noted.
DETECTORS = {"ndz128": ((36, 128), True), "ndz512_strided": ((160, 512), True), "ndz150": ((36, 150), False)}


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def setup(ndet, seed=5):
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.backend import HipBackend
    from tomography_alignment_amd.utilities.geometry import Geometry
    rng = np.random.default_rng(seed)
    n = PHI.size
    xyz = np.zeros((n, 3))
    xyz[:, 0] = rng.uniform(-2, 2, n)
    xyz[:, 2] = ZSHIFT
    geo = Geometry(n, np.array(SHAPE), np.ones(3), np.array(ndet), np.ones(2))
    be = HipBackend(geo)
    poses = _lib.poses_array(PHI, np.zeros(n), np.zeros(n), xyz, np.zeros(3))
    x = rng.uniform(0.1, 1.0, SHAPE).astype(np.float32)
    d_ax = be.forward(poses, be.upload(x), be.empty(n * be.n_det))          # the projector stages these poses, as in a SIRT iteration
    b = rng.standard_normal((n, ndet[0], ndet[1])).astype(np.float32)
    return be, poses, d_ax, b


def weights(kind, ndet, band):
    w = np.zeros((PHI.size, ndet[0], ndet[1]), np.float32)
    if kind == "banded":
        w[:, :, band[0]:band[1]] = 1.0
    elif kind == "dense":
        w[:] = 1.0
    return w


def counted(ctx, fn):
    ctx.profile_reset()
    ctx.profile_enable(True)
    out = fn()
    ctx.profile_enable(False)
    return out, ctx.profile_get("k_sino_zflags")[0] > 0        # did the back-projection scan the sinogram itself (the scan and what derives from it)?


@pytest.mark.parametrize("det", sorted(DETECTORS))
@pytest.mark.parametrize("kind", ["banded", "zero", "dense"])
def test_adjoint_after_the_noting_residual_pass(det, kind):
    ndet, noted = DETECTORS[det]
    be, poses, d_ax, b = setup(ndet)
    ctx = be.ctx
    # detector plane ndz / 2 looks at voxel plane 75: the band reaches the planes 86 .. 114 -- chunk 1 of the three, so the chunk grouping shifts
    band = (ndet[1] // 2 + 15, ndet[1] // 2 + 35)
    d_b, d_w = be.upload(b), be.upload(weights(kind, ndet, band))
    plain, out = be.empty(d_b.size), be.empty(d_b.size)
    s_plain = be.residual_scale(d_b, d_ax, d_w, plain)
    s = be.residual_scale(d_b, d_ax, d_w, out, n_proj=PHI.size)
    assert s == s_plain or abs(s - s_plain) <= 1e-12 * abs(s_plain)        # double atomics, another order
    assert np.array_equal(bits(out.download()), bits(plain.download()))
    vol1, n_scan1 = counted(ctx, lambda: be.adjoint(poses, out, be.empty(be.n_vox)).download())
    assert n_scan1 == (not noted), "the back-projection %s its own scan" % ("made" if noted else "skipped")
    vol2, n_scan2 = counted(ctx, lambda: be.adjoint(poses, out, be.empty(be.n_vox)).download())      # the note served one call: this one scans
    assert n_scan2
    assert np.array_equal(bits(vol1), bits(vol2))
    assert (np.count_nonzero(vol1) > 0) == (kind != "zero")
    if kind == "banded":
        assert np.count_nonzero(vol1.reshape(SHAPE)[:, :, :40]) == 0 and np.count_nonzero(vol1.reshape(SHAPE)[:, :, 140:]) == 0
    # ... and the fused step takes the note the same way
    d_V, rec0 = be.upload(np.full(be.n_vox, 0.5, np.float32)), np.linspace(-1, 1, be.n_vox).astype(np.float32)
    rec = be.upload(rec0)
    be.residual_scale(d_b, d_ax, d_w, out, n_proj=PHI.size)      # (after the upload: a copy into the context drops the note)
    (fused, _), n_scan3 = counted(ctx, lambda: be.adjoint_update(poses, out, rec, d_V, False, None))
    assert fused and n_scan3 == (not noted)
    bp = be.upload(vol2)
    want = be.upload(rec0)
    be.update(want, bp, d_V, False, None)
    assert np.array_equal(bits(rec.download()), bits(want.download()))


@pytest.mark.parametrize("writer", ["axpy", "fill_view", "upload", "copy"])
def test_a_write_in_between_drops_the_note(writer):
    """All-zero residual noted (no plane flagged: every chunk dead), then one detector plane made non-zero through another entry point
    of the library: the back-projection must see it."""
    ndet, _ = DETECTORS["ndz128"]
    be, poses, d_ax, b = setup(ndet)
    d_b, d_w = be.upload(b), be.upload(weights("zero", ndet, None))
    out = be.empty(d_b.size)
    be.residual_scale(d_b, d_ax, d_w, out, n_proj=PHI.size)
    delta = np.zeros((PHI.size, ndet[0], ndet[1]), np.float32)
    delta[:, :, 30] = 1.0
    if writer == "axpy":
        be.axpy(out, be.upload(delta), 1.0)
    elif writer == "fill_view":
        be.fill(out.view(18 * ndet[1] + 30, 1), 1.0)        # one element: projection 0, the detector row through the centre, plane 30
        delta[:] = 0
        delta[0, 18, 30] = 1.0
    elif writer == "upload":
        out.upload(delta.ravel())
    else:
        be.copy(out, be.upload(delta))
    vol, n_scan = counted(be.ctx, lambda: be.adjoint(poses, out, be.empty(be.n_vox)).download())
    assert n_scan
    assert np.count_nonzero(vol) > 0
    fresh = setup(ndet)[0]          # another context: nothing noted, nothing cached
    want = fresh.adjoint(poses, fresh.upload(delta), fresh.empty(fresh.n_vox)).download()
    assert np.array_equal(bits(vol), bits(want))


def test_without_staged_poses_nothing_is_noted():
    """The note needs the z offsets of the poses the projector staged last: a context that has projected nothing takes none."""
    from tomography_alignment_amd.backend import HipBackend
    ndet, _ = DETECTORS["ndz128"]
    be, poses, d_ax, b = setup(ndet)
    other = HipBackend(be.geometry)
    ax = other.upload(d_ax.download())
    out = other.empty(ax.size)
    other.residual_scale(other.upload(b), ax, None, out, n_proj=PHI.size)
    vol, n_scan = counted(other.ctx, lambda: other.adjoint(poses, out, other.empty(other.n_vox)).download())
    assert n_scan and np.count_nonzero(vol) > 0
