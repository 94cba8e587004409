"""FBP on the GPU: the HIP ramp filter of libtomo_fbp.so against the float64 model (tests/fbp_model.py), recon/fbp.py's FBP against the
model through the CPU oracle's adjoint, its accuracy on a blob phantom, the warm start of SIRT and of examples/align_rigid, and the
angle-sharded FBP at world 2 on one GPU."""
import numpy as np
import pytest

import fbp_model as fm
from conftest import rel_max
from fbp_model import pair_err, pair_errs
from gloo_world import run_world
from oracle import oracle as orc

from tomography_alignment_amd import _fbp_lib, _lib
from tomography_alignment_amd.recon import fbp, sirt
from tomography_alignment_amd.utilities.geometry import Geometry

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context()
    yield c
    c.close()


def _filter_gpu(ctx, h, p, scales, in_place):
    n, ndx, ndz = p.shape
    d_in = ctx.to_device(p)
    d_out = d_in if in_place else ctx.zeros(p.shape)
    h.filter(ctx.stream(), d_in.ptr, d_out.ptr, n, ndx, ndz, scales)
    ctx.sync()
    return d_out.download()


@pytest.mark.parametrize("ndx", [64, 100, 257, 1024, 4096])
def test_filter_parity_with_the_float64_model(ctx, ndx):
    rng = np.random.default_rng(ndx)
    worst = 0.0
    with _fbp_lib.FbpHandle(ctx.device) as h:
        for ndz in (1, 7, 20, 33):
            n = 3
            p = rng.standard_normal((n, ndx, ndz)).astype(np.float32)
            scales = rng.uniform(0.5, 2.0, n)
            for k, name in enumerate(fbp.FILTERS):
                h.set_response(ndx, fbp.filter_response(ndx, name))
                ref = fm.filter_model(p, name, scales)
                got = _filter_gpu(ctx, h, p, scales, in_place=bool((k + ndz) % 2))
                e = rel_max(got, ref)
                worst = max(worst, e)
                assert e <= 1e-5, (ndx, ndz, name, e)
    print("filter parity ndx %d: worst rel_max %.2e over ndz {1, 7, 20, 33} x %s" % (ndx, worst, ", ".join(fbp.FILTERS)))


def test_filter_in_and_out_of_place_agree(ctx):
    rng = np.random.default_rng(5)
    p = rng.standard_normal((4, 300, 45)).astype(np.float32)
    with _fbp_lib.FbpHandle(ctx.device) as h:
        h.set_response(300, fbp.filter_response(300, "shepp-logan"))
        a = _filter_gpu(ctx, h, p, np.arange(1.0, 5.0), in_place=True)
        b = _filter_gpu(ctx, h, p, np.arange(1.0, 5.0), in_place=False)
    print("in place vs out of place: max |diff| %.1e" % np.max(np.abs(a - b)))
    assert np.array_equal(a, b)


def test_filter_one_call_at_1024(ctx):
    rng = np.random.default_rng(11)
    n, ndx, ndz = 16, 1024, 1024
    p = rng.standard_normal((n, ndx, ndz)).astype(np.float32)
    scales = rng.uniform(0.5, 2.0, n)
    with _fbp_lib.FbpHandle(ctx.device) as h:
        h.set_response(ndx, fbp.filter_response(ndx, "ramp"))
        got = _filter_gpu(ctx, h, p, scales, in_place=False)
    e = max(rel_max(got[i], fm.filter_model(p[i:i + 1], "ramp", scales[i:i + 1])[0]) for i in range(n))
    print("filter parity 16 x 1024 x 1024: worst per-projection rel_max %.2e" % e)
    assert e <= 1e-5


def test_wider_than_4096_is_unsupported_and_writes_nothing(ctx):
    with _fbp_lib.FbpHandle(ctx.device) as h:
        with pytest.raises(_fbp_lib.FbpUnsupported):
            h.set_response(4097, fbp.filter_response(4097, "ramp"))
        d = ctx.to_device(np.full((2, 4097, 3), 7.0, np.float32))
        with pytest.raises(_fbp_lib.FbpUnsupported) as ei:
            h.filter(ctx.stream(), d.ptr, d.ptr, 2, 4097, 3, [1.0, 1.0])
        ctx.sync()
        print("ndx 4097:", ei.value)
        assert np.all(d.download() == 7.0)
        with pytest.raises(_lib.TomoError):          # a width whose response was not set
            h.filter(ctx.stream(), d.ptr, d.ptr, 2, 100, 3, [1.0, 1.0])


def _columns_per_group(ndx):
    """Cfg<LOGN>::C of csrc/fbp/tomo_fbp.hip: a work-group holds S = (TOMO_FBP_LDS_KIB * 1024 / 8) >> LOGN complex signals of Npad
    values (at least one), two detector columns each.  8192 is the shipped TOMO_FBP_LDS_KIB = 64."""
    return 2 * max(1, 8192 // fbp.padded_length(ndx))


def _per_projection(got, ref):
    return [rel_max(got[i], ref[i]) for i in range(ref.shape[0])]


# LOGN -> the smallest and the largest detector width that pad to Npad = 2^LOGN
WIDTHS = {6: (1, 32), 7: (33, 64), 8: (65, 128), 9: (129, 256), 10: (257, 512), 11: (513, 1024), 12: (1025, 2048), 13: (2049, 4096)}


@pytest.mark.parametrize("logn", sorted(WIDTHS))
def test_every_fft_length_at_both_ends_of_its_width_range(ctx, logn):
    """Every k_ramp_filter<LOGN> (6, 9 and 12 start with a radix-8 pass, the others with radix 2 or 4), with one partly filled
    work-group per projection, a full one, and two or three chunks whose last holds one lone column; measured per projection."""
    worst, k = 0.0, 0
    for ndx in WIDTHS[logn]:
        assert fbp.padded_length(ndx) == 1 << logn
        C = _columns_per_group(ndx)
        rng = np.random.default_rng(100 * ndx + logn)
        with _fbp_lib.FbpHandle(ctx.device) as h:
            for a, ndz in enumerate(sorted({1, C - 1, C, C + 1, 2 * C + 1} - {0})):
                n = 3
                p = rng.standard_normal((n, ndx, ndz)).astype(np.float32)
                scales = rng.uniform(0.5, 2.0, n)
                names = fbp.FILTERS if ndz == C + 1 else ("ramp", fbp.FILTERS[1 + a % 4])
                for name in names:
                    h.set_response(ndx, fbp.filter_response(ndx, name))
                    ref = fm.filter_model(p, name, scales)
                    got = _filter_gpu(ctx, h, p, scales, in_place=bool(k % 2))
                    k += 1
                    e = _per_projection(got, ref)
                    worst = max(worst, max(e))
                    assert max(e) <= 1e-5, (ndx, ndz, name, e)
    print("filter parity LOGN %d (ndx %d and %d, C %d): worst per-projection rel_max %.2e over %d launches"
          % (logn, WIDTHS[logn][0], WIDTHS[logn][1], C, worst, k))


def _structured(ndx, rng):
    """One projection of eight columns, ordered so that unlike kinds share a complex signal."""
    x = np.arange(ndx)
    cols = [np.ones(ndx),                                   # constant: all of it at DC and the lowest bins
            (x == 0) * 1.0,                                 # impulse at row 0
            (x == ndx - 1) * 1.0,                           # impulse at the last row
            2 + np.cos(2 * np.pi * x / ndx),
            (x >= ndx // 3) * 1.0,                          # step
            1.0 - 2.0 * (x % 2),                            # alternating +-1: the Nyquist bin
            rng.standard_normal(ndx),
            1000 + rng.standard_normal(ndx)]
    return np.stack(cols, axis=1)[None]


@pytest.mark.parametrize("ndx", [20] + [WIDTHS[l][1] for l in sorted(WIDTHS)])
def test_structured_columns_per_pair(ctx, ndx):
    """Inputs with their weight at DC, at Nyquist and at single rows, each pair of columns measured against its own maximum: a wrong
    H[0] or H[min(i, N - i)] off by one, which white noise under an array-wide maximum hides, moves these by far more than 1e-5
    (H[0] = 0 moves every pair by 1.7e-5 ... 1.2e-2).  Measured on an MI355X: worst pair 2.2e-7 (ndx 20) ... 4.4e-7 (ndx 4096); a
    float32 two-columns-per-signal FFT on the CPU is within 5e-7 of the model."""
    logn = fbp.padded_length(ndx).bit_length() - 1
    base = _structured(ndx, np.random.default_rng(ndx))
    worst, k = 0.0, 0
    with _fbp_lib.FbpHandle(ctx.device) as h:
        for amp in ((1, 1, 1, 1, 1, 1, 1, 1), (1, 1, 1e3, 1e-3, 1, 1, 1, 1)):
            p = (base * np.array(amp, np.float64)).astype(np.float32)
            for name in fbp.FILTERS:
                h.set_response(ndx, fbp.filter_response(ndx, name))
                ref = fm.filter_model(p, name, [1.3])
                got = _filter_gpu(ctx, h, p, [1.3], in_place=bool(k % 2))
                k += 1
                e = pair_errs(got, ref)
                assert pair_err(got, ref) == e.max()
                worst = max(worst, e.max())
                assert e.max() <= 1e-5, (ndx, amp, name, "per pair (1,2) (3,4) (5,6) (7,8):", e[0])
    print("structured columns LOGN %d (ndx %d): worst pair_err %.2e over 2 amplitude sets x %s" % (logn, ndx, worst, ", ".join(fbp.FILTERS)))


@pytest.mark.parametrize("z0", [70, 5, 128], ids=["even", "odd", "lone-last"])
def test_a_non_finite_value_stays_in_its_column_pair(ctx, z0):
    """Columns 2s and 2s+1 share one complex signal, so a NaN or an infinity spoils its own column and its partner (DESIGN.md 7b,
    Limits); every other column, and every other projection, must not change by a bit."""
    ndx = 100
    C = _columns_per_group(ndx)
    ndz = 2 * C + 1
    assert C == 64 and z0 < ndz
    rng = np.random.default_rng(z0)
    p = rng.standard_normal((3, ndx, ndz)).astype(np.float32)
    scales = [0.7, 1.1, 1.9]
    keep = np.ones(p.shape, bool)
    keep[1, :, z0 & ~1:(z0 & ~1) + 2] = False
    with _fbp_lib.FbpHandle(ctx.device) as h:
        h.set_response(ndx, fbp.filter_response(ndx, "hamming"))
        clean = _filter_gpu(ctx, h, p, scales, in_place=False)
        assert np.all(np.isfinite(clean)) and max(_per_projection(clean, fm.filter_model(p, "hamming", scales))) <= 1e-5
        for bad in (np.nan, np.inf):
            q = p.copy()
            q[1, 37, z0] = bad
            got = _filter_gpu(ctx, h, q, scales, in_place=bool(z0 % 2))
            same = got.view(np.uint32)[keep] == clean.view(np.uint32)[keep]
            print("%s at projection 1, column %d: %d of %d values outside its pair differ; %d of %d inside are non-finite"
                  % (bad, z0, np.count_nonzero(~same), same.size, np.count_nonzero(~np.isfinite(got[~keep])), np.count_nonzero(~keep)))
            assert np.all(same), (bad, z0, np.argwhere(~(got.view(np.uint32) == clean.view(np.uint32)) & keep)[:5])


@pytest.mark.parametrize("ndx", [WIDTHS[6][1], WIDTHS[9][1], WIDTHS[13][1]])
def test_a_column_pair_filters_the_same_wherever_it_lies(ctx, ndx):
    """The same two columns as the first pair of the only projection, and as the first pair of the third chunk of the last projection
    (another chunk, another blockIdx, another base offset): the same result up to the order of the sums."""
    C = _columns_per_group(ndx)
    rng = np.random.default_rng(ndx + 1)
    cols = rng.standard_normal((ndx, 2)).astype(np.float32)
    big = rng.standard_normal((3, ndx, 2 * C + 2)).astype(np.float32)
    big[2, :, 2 * C:] = cols
    with _fbp_lib.FbpHandle(ctx.device) as h:
        h.set_response(ndx, fbp.filter_response(ndx, "shepp-logan"))
        a = _filter_gpu(ctx, h, cols[None], [1.7], in_place=False)
        b = _filter_gpu(ctx, h, big, [0.6, 1.2, 1.7], in_place=True)[2:, :, 2 * C:]
    assert pair_err(a, fm.filter_model(cols[None], "shepp-logan", [1.7])) <= 1e-5
    e = pair_err(b, a)
    print("placement ndx %d (C %d): pair_err %.2e between z = 0, 1 of 1 projection and z = %d, %d of projection 2 of 3; bit-equal: %s"
          % (ndx, C, e, 2 * C, 2 * C + 1, np.array_equal(a.view(np.uint32), b.view(np.uint32))))
    assert e <= 1e-6


def _buffers(ctx, p):
    """The uploaded input and a zeroed output.  Uploads synchronise the context's stream, so whatever must stay queued behind a filter
    gets its buffers before that filter is issued."""
    return ctx.to_device(p), ctx.zeros(p.shape)


def _enqueue(h, st, bufs, shape, scales):
    """filter() out of place on stream st: no upload, no allocation, no sync."""
    h.filter(st, bufs[0].ptr, bufs[1].ptr, shape[0], shape[1], shape[2], scales)


def test_one_handle_through_a_sequence(ctx):
    """One handle: the tables replaced when the FFT length goes down, up, stays and comes back; the scale buffers grown and then larger
    than needed; two filters queued with no sync between them (they share the pinned scale staging); the response replaced while a
    filter is still queued; an empty call; a scales array of the wrong length."""
    rng = np.random.default_rng(4)
    with _fbp_lib.FbpHandle(ctx.device) as h:
        for ndx, name, n, ndz in ((2048, "ramp", 2, 5), (20, "cosine", 5, 70), (300, "shepp-logan", 1, 9), (300, "hamming", 1, 9),
                                  (2048, "hann", 2, 3)):
            p = rng.standard_normal((n, ndx, ndz)).astype(np.float32)
            scales = rng.uniform(0.5, 2.0, n)
            h.set_response(ndx, fbp.filter_response(ndx, name))
            e = _per_projection(_filter_gpu(ctx, h, p, scales, in_place=False), fm.filter_model(p, name, scales))
            print("sequence: ndx %4d %-11s n_proj %d: worst per-projection rel_max %.2e" % (ndx, name, n, max(e)))
            assert max(e) <= 1e-5, (ndx, name, n, e)

        # two filters back to back (2048, hann): different inputs, outputs, scales and projection counts, one sync
        p1, p2 = rng.standard_normal((2, 2048, 3)).astype(np.float32), rng.standard_normal((4, 2048, 5)).astype(np.float32)
        s1, s2 = rng.uniform(0.5, 2.0, 2), rng.uniform(2.0, 8.0, 4)
        b1, b2, st = _buffers(ctx, p1), _buffers(ctx, p2), ctx.stream()
        _enqueue(h, st, b1, p1.shape, s1)
        _enqueue(h, st, b2, p2.shape, s2)          # rewrites the pinned scales the first filter's copy reads: tomo_fbp_filter waits first
        ctx.sync()
        e1 = _per_projection(b1[1].download(), fm.filter_model(p1, "hann", s1))
        e2 = _per_projection(b2[1].download(), fm.filter_model(p2, "hann", s2))
        print("sequence: two filters, one sync: worst per-projection rel_max %.2e and %.2e" % (max(e1), max(e2)))
        assert max(e1) <= 1e-5 and max(e2) <= 1e-5, (e1, e2)

        # the response replaced at the same FFT length while the filter that reads the old one is still queued
        p = rng.standard_normal((3, 300, 40)).astype(np.float32)
        s = rng.uniform(0.5, 2.0, 3)
        ramp, hann = fbp.filter_response(300, "ramp"), fbp.filter_response(300, "hann")
        bA, bB = _buffers(ctx, p), _buffers(ctx, p)
        h.set_response(300, ramp)
        _enqueue(h, st, bA, p.shape, s)
        h.set_response(300, hann)
        _enqueue(h, st, bB, p.shape, s)
        ctx.sync()
        A, B = bA[1].download(), bB[1].download()
        eA, eB = _per_projection(A, fm.filter_model(p, "ramp", s)), _per_projection(B, fm.filter_model(p, "hann", s))
        print("sequence: ramp, set_response(hann), hann, one sync: worst per-projection rel_max %.2e (ramp) and %.2e (hann); "
              "ramp vs hann differ by %.2e" % (max(eA), max(eB), rel_max(A, B)))
        assert max(eA) <= 1e-5 and max(eB) <= 1e-5, (eA, eB)

        # no projections: nothing is launched; scales of the wrong length: the binding raises, and nothing is launched either
        d = ctx.to_device(np.full((3, 300, 4), 7.0, np.float32))
        h.filter(ctx.stream(), d.ptr, d.ptr, 0, 300, 4, [])
        for bad in ([1.0, 2.0], [1.0, 2.0, 3.0, 4.0], []):
            with pytest.raises(ValueError):
                h.filter(ctx.stream(), d.ptr, d.ptr, 3, 300, 4, bad)
        ctx.sync()
        assert np.all(d.download() == 7.0)


def test_a_response_table_of_the_wrong_length_is_refused(ctx):
    """tomo_fbp_set_response reads Npad/2 + 1 doubles from a bare pointer; the binding refuses any other length before the call, and the
    handle keeps the response it had."""
    rng = np.random.default_rng(9)
    p = rng.standard_normal((2, 100, 5)).astype(np.float32)
    good = fbp.filter_response(100, "hann")
    assert good.size == 129 == _fbp_lib.response_length(100)
    with _fbp_lib.FbpHandle(ctx.device) as h:
        h.set_response(100, good)
        for ndx, table in ((100, good[:-1]), (100, np.append(good, 0.0)), (300, good), (20, good)):
            with pytest.raises(ValueError):
                h.set_response(ndx, table)
        e = _per_projection(_filter_gpu(ctx, h, p, [1.0, 2.0], in_place=True), fm.filter_model(p, "hann", [1.0, 2.0]))
        print("after four refused tables: worst per-projection rel_max %.2e" % max(e))
        assert max(e) <= 1e-5


def _case(N, n, seed, perturbed):
    rng = np.random.default_rng(seed)
    phi = np.linspace(0, np.pi, n, endpoint=False)
    alpha, beta, xyz, cor = np.zeros(n), np.zeros(n), np.zeros((n, 3)), np.zeros(3)
    if perturbed:
        alpha, beta = np.deg2rad(rng.uniform(-1, 1, n)), np.deg2rad(rng.uniform(-1, 1, n))
        xyz[:, 0], xyz[:, 2] = rng.uniform(-2, 2, n), rng.uniform(-2, 2, n)
        cor = np.array([0.6, 0.0, 0.0])
    og = orc.Geo(n, np.array([N, N, N]), np.ones(3), np.array([N, N]), np.ones(2), cor_shift=cor)
    geo = Geometry(n, np.array([N, N, N]), np.ones(3), np.array([N, N]), np.ones(2), cor_shift=cor)
    x = fm.blob_phantom(N, seed=seed, n_blobs=6)
    p = orc.forward(og, x, alpha=alpha, beta=beta, phi=phi, xyz_shift=xyz).reshape(n, N, N).astype(np.float32)
    return og, geo, x, p, phi, alpha, beta, xyz


@pytest.mark.parametrize("perturbed", [False, True], ids=["nominal", "poses"])
@pytest.mark.parametrize("device_input", [False, True], ids=["numpy", "device"])
def test_fbp_run_equals_the_cpu_model(perturbed, device_input):
    og, geo, x, p, phi, alpha, beta, xyz = _case(40, 60, 2, perturbed)
    ref = fm.fbp_model(og, p, phi, alpha, beta, xyz, filter="hamming")
    from tomography_alignment_amd.backend import HipBackend
    be = HipBackend(geo)
    proj = be.upload(p) if device_input else p
    f = fbp.FBP(geo, proj, np.array([phi, alpha, beta]).T, xyz, options={"filter": "hamming", "_backend": be})
    rec = f.run()
    e = rel_max(rec, ref)
    print("FBP.run vs CPU model (%s poses, %s input): rel_max %.2e" % ("perturbed" if perturbed else "nominal", "device" if device_input else "numpy", e))
    assert rec.shape == (40, 40, 40)
    assert e <= 1e-5
    if device_input:
        assert np.array_equal(proj.download(), p.reshape(proj.shape))          # not overwritten by default
        f2 = fbp.FBP(geo, proj, np.array([phi, alpha, beta]).T, xyz, options={"filter": "hamming", "_backend": be, "overwrite_projections": True})
        rec2 = f2.run()
        assert rel_max(rec2, rec) <= 1e-6               # the tilted adjoint sums with atomics: equal up to the order of the sums
        assert not np.array_equal(proj.download(), p.reshape(proj.shape))      # filtered in place


@pytest.mark.parametrize("step,n,endpoint", [(1.0, 180, False), (0.5, 180, False), (1.0, 181, True)], ids=["step1", "step0.5", "endpoints181"])
def test_fbp_accuracy_on_the_gpu(step, n, endpoint):
    N = 64
    x = fm.blob_phantom(N)
    phi = np.linspace(0, np.pi, n, endpoint=endpoint)
    og = orc.Geo(n, np.array([N, N, N]), np.ones(3), np.array([N, N]), np.ones(2), step_size=step)
    geo = Geometry(n, np.array([N, N, N]), np.ones(3), np.array([N, N]), np.ones(2), step_size=step)
    p = orc.forward(og, x, phi=phi).reshape(n, N, N).astype(np.float32)
    f = fbp.FBP(geo, p, np.array([phi, 0 * phi, 0 * phi]).T, np.zeros((n, 3)), options={"ground_truth": x})
    rec = f.run()
    err, ratio = fm.accuracy(rec, x)
    print("GPU FBP, step %.1f, %d angles: rel-L2 in the cylinder %.4f, mean ratio %.5f, rms_error (whole volume) %.4f"
          % (step, n, err, ratio, f.rms_error))
    assert err <= 0.05 and abs(ratio - 1) <= 0.02


def test_fbp_warm_start_lowers_the_first_sirt_error():
    from tomography_alignment_amd.examples import generate_data
    d = generate_data.make(64, 90, seed=0, ang_deg=0.0, shift_px=0.0)
    n = d["phi"].size
    geo = Geometry(n, np.array([64, 64, 64]), np.ones(3), np.array([64, 64]), np.ones(2))
    angles = np.array([d["phi"], d["alpha"], d["beta"]]).T
    f = fbp.FBP(geo, d["projections"], angles, d["xyz"], options={"ground_truth": d["phantom"]})
    f.run()
    rms = {}
    for tag, opts in (("zero", {}), ("fbp", {"rec": f.d_rec, "_backend": f.be})):
        s = sirt.SIRT(geo, d["projections"], angles, d["xyz"], options=dict(opts, ground_truth=d["phantom"]))
        k, r = s.iterate_device(niter=5)
        rms[tag] = r[0]
    print("SIRT rms_error[0]: from zero %.4f, from the FBP %.4f (FBP alone %.4f)" % (rms["zero"], rms["fbp"], f.rms_error))
    assert rms["fbp"] < rms["zero"]


def test_align_rigid_init_fbp():
    from tomography_alignment_amd.examples import align_rigid, generate_data
    d = generate_data.make(48, 60, seed=1)
    first = {}
    for init in ("zero", "fbp"):
        out = align_rigid.run(dict(d), n_outer=1, sirt_iters=5, verbose=False, return_loop=True, init=init)
        first[init] = float(out[5].solver.rms_error[0])
        assert len(out[4]) == 1 and np.isfinite(out[4][0]["rmse"])
    print("align_rigid first SIRT rms: init zero %.4f, init fbp %.4f" % (first["zero"], first["fbp"]))
    assert first["fbp"] < first["zero"]
    with pytest.raises(ValueError):
        align_rigid.run(dict(d), n_outer=1, sirt_iters=1, verbose=False, init="ones")


def test_sharded_fbp_world_2_on_one_gpu(tmp_path):
    one = run_world("_gloo_gpu_fbp_worker.py", 1, str(tmp_path / "w1"), timeout=300, per_rank=True)[0]
    two = run_world("_gloo_gpu_fbp_worker.py", 2, str(tmp_path / "w2"), timeout=300, per_rank=True)
    assert two[0]["ramp_rows"].size + two[1]["ramp_rows"].size == one["ramp_rows"].size
    for filt in ("ramp", "hann"):
        for r in range(2):
            e = rel_max(two[r][filt], one[filt])
            print("sharded FBP (%s), world 2 rank %d vs world 1: rel_max %.2e" % (filt, r, e))
            assert e <= 1e-6
