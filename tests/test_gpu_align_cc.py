"""align/align_cc.py on the GPU (libtomo_xcorr.so): the reference's own results (golden G15), the pcc stand-in on every G15 pair,
the spline shift against scipy.ndimage.shift, caller filters, a 128 x 512^2 series against the numpy models, recovery of a known
drift, edge cases, and that no call leaves device memory behind."""
import numpy as np
import pytest
from scipy import ndimage

import pcc_standin as ps
import xcorr_model
from conftest import golden, rel_max

pytestmark = pytest.mark.gpu

TIE = 1e-9          # relative argmax margin below which two float64 implementations may pick different peaks


def _cc():
    from tomography_alignment_amd.align import align_cc
    return align_cc


def _check_skimage_offsets(off, ref_off, margins, tag):
    """Exact where every argmax of the step has a margin above TIE, else within 1/100 px."""
    for i in range(len(off)):
        if np.min(margins[i]) > TIE:
            assert np.array_equal(off[i], ref_off[i]), (tag, i, off[i], ref_off[i], margins[i])
        else:
            assert np.max(np.abs(off[i] - ref_off[i])) <= 0.01 + 1e-12, (tag, i, off[i], ref_off[i])


def test_g15_numpy_chain():
    g = golden("g15_align_cc")
    off, al = _cc().cross_correlation_numpy(g["proj"])
    assert al.dtype == np.float32
    assert np.array_equal(off, g["np_offsets"]), (off, g["np_offsets"])
    assert np.array_equal(al, g["np_aligned"])


def test_g15_skimage_chain(capsys):
    g = golden("g15_align_cc")
    off, al = _cc().cross_correlation_skimage(g["proj"], sinogram_order=False)
    assert al.dtype == np.float32
    _check_skimage_offsets(off, g["sk_offsets"], g["sk_margin"], "g15")
    e = rel_max(al, g["sk_aligned"])
    with capsys.disabled():
        print("\n[G15 skimage chain] max |offset diff| %.1e, aligned rel-max %.1e" % (np.max(np.abs(off - g["sk_offsets"])), e))
    assert e < 1e-6


def test_g15_pcc_pairs_and_batch():
    cc = _cc()
    g = golden("g15_align_cc")
    for k in range(3):
        ref, mov = g["pair%d_ref" % k], g["pair%d_mov" % k]
        for u in (1, 16, 100):
            for norm in ("phase", None):
                tag = "pair%d_u%d_%s" % (k, u, norm or "none")
                s, e, p = cc.phase_cross_correlation(ref, mov, upsample_factor=u, normalization=norm)
                assert np.array_equal(s, g[tag + "_shifts"]) or np.min(g[tag + "_margin"]) <= TIE, (tag, s, g[tag + "_shifts"])
                assert abs(e - g[tag + "_error"]) < 1e-9 and abs(p - g[tag + "_phasediff"]) < 1e-9, (tag, e, p)
                # the batch form: the same pair among others gives the same numbers
                refs = np.stack([mov, ref, ref])
                movs = np.stack([ref, mov, ps.fourier_shift(mov, (0.0, 1.5))])
                sb, eb, pb = cc.phase_cross_correlation_batch(refs, movs, upsample_factor=u, normalization=norm)
                assert np.array_equal(sb[1], s) and eb[1] == e and pb[1] == p, tag
                for b in (0, 2):
                    s2, e2, p2, _ = ps.phase_cross_correlation_margins(refs[b], movs[b], u, norm)
                    assert np.max(np.abs(sb[b] - s2)) <= 1.0 / u and abs(eb[b] - e2) < 1e-6, (tag, b, sb[b], s2)


def test_spline_shift_matches_scipy(capsys):
    from tomography_alignment_amd._xcorr_lib import XcorrHandle
    rng = np.random.default_rng(3)
    worst = 0.0
    with XcorrHandle() as h:
        for shp in [(64, 64), (9, 13), (1, 12), (7, 1), (2, 5), (33, 70)]:
            shifts = np.array([(0.3, -1.7), (2.0, 0.0), (-0.5, 0.5), (3.99, -4.01), (0.0, 0.0), (-1e-9, 1e-9), (8.5, 0.2),
                               (-0.01, 0.99), (shp[0] - 1.0, 0.0), (0.0, -(shp[1] - 1.0))])
            for dt in (np.float32, np.float64):
                img = rng.standard_normal(shp).astype(dt)
                imgs = np.ascontiguousarray(np.broadcast_to(img, (len(shifts),) + shp))
                out = h.spline_shift(imgs, np.ascontiguousarray(shifts))
                assert out.dtype == dt
                for b, s in enumerate(shifts):
                    r = ndimage.shift(img, s, order=3, mode="constant", cval=0.0)
                    d = float(np.max(np.abs(out[b].astype(np.float64) - r))) if r.size else 0.0
                    tol = 1e-12 if dt == np.float64 else 1e-6
                    assert d <= tol * max(1.0, float(np.abs(r).max())), (shp, s, dt, d)
                    if dt == np.float64:
                        worst = max(worst, d)
    with capsys.disabled():
        print("\n[spline shift vs scipy] float64 max abs err %.1e" % worst)


def test_cor_flipping_recovers_offset():
    cc = _cc()
    rng = np.random.default_rng(5)
    img = ps.fourier_shift(rng.standard_normal((48, 96)), (0, 0))
    img = np.real(np.fft.ifft2(np.fft.fft2(img) * np.exp(-40 * (np.fft.fftfreq(48)[:, None] ** 2 + np.fft.fftfreq(96)[None] ** 2))))
    for cor in (3.25, -7.5, 0.0625):
        p0 = ps.fourier_shift(img, (0.0, cor))
        p180 = np.fliplr(ps.fourier_shift(img, (0.0, -cor)))
        got = cc.cor_flipping(p0, p180)
        assert abs(got - 2 * cor) <= 1.0 / 16, (cor, got)


def test_cross_correlation_align_caller_filters():
    cc = _cc()
    rng = np.random.default_rng(7)
    nx, nz = 40, 56
    ref = rng.standard_normal((nx, nz)).astype(np.float32)
    img = np.roll(ref, (5, -9), axis=(0, 1)) + 0.1 * rng.standard_normal((nx, nz)).astype(np.float32)
    rF = rng.uniform(0.2, 1.0, (nx, nz))
    kF = rng.uniform(0.0, 1.0, (nx, nz))
    shifts, out = cc.crossCorrelationAlign(img, ref, rF, kF)
    a = np.fft.fft2((img.astype(np.float64) - img.astype(np.float64).mean()) * rF)
    b = np.fft.fft2((ref.astype(np.float64) - ref.astype(np.float64).mean()) * rF)
    xcor = np.abs(np.fft.ifft2(np.conj(a) * b * kF))
    want = np.unravel_index(xcor.argmax(), xcor.shape)
    assert tuple(int(s) for s in shifts) == tuple(int(s) for s in want) == ((-5) % nx, 9)
    assert out.dtype == np.float32
    assert np.array_equal(out, np.roll(np.roll(img, want[0], axis=0), want[1], axis=1))


def _drifting_series(n, size, seed):
    rng = np.random.default_rng(seed)
    x = np.random.RandomState(seed).standard_normal((size, size))
    base = ps.fourier_shift(x, (0, 0))
    f = np.fft.fft2(base) * np.exp(-60 * (np.fft.fftfreq(size)[:, None] ** 2 + np.fft.fftfreq(size)[None] ** 2))
    base = np.real(np.fft.ifft2(f))
    drift = np.cumsum(rng.uniform(-1.5, 1.5, (n, 2)), axis=0)
    drift[0] = 0
    return np.stack([ps.fourier_shift(base, d) + 0.01 * rng.standard_normal((size, size)) for d in drift]).astype(np.float32)


def test_user_size_512_against_numpy_model(capsys):
    cc = _cc()
    proj = _drifting_series(128, 512, 11)
    from tomography_alignment_amd._xcorr_lib import XcorrHandle
    with XcorrHandle() as h:
        off_n, al_n = cc.cross_correlation_numpy(proj, handle=h)
        off_s, al_s = cc.cross_correlation_skimage(proj, handle=h)
    mo_n, ma_n, _ = xcorr_model.chain_numpy(proj)
    mo_s, ma_s, mm_s = xcorr_model.chain_skimage(proj)
    assert np.array_equal(off_n, mo_n) and np.array_equal(al_n, ma_n)
    _check_skimage_offsets(off_s, mo_s, mm_s, "512")
    e = rel_max(al_s, ma_s)
    with capsys.disabled():
        print("\n[128 x 512^2] numpy path exact; skimage max |offset diff| %.1e, aligned rel-max %.1e"
              % (np.max(np.abs(off_s - mo_s)), e))
    assert e < 1e-6


def _phantom_projection():
    """One projection of the 128^3 phantom, in a 192^2 field: a +-20 px drift then moves no content across the border."""
    from tomography_alignment_amd.utilities import generate_phantom
    return np.pad(generate_phantom.shepp3d(128).astype(np.float64).sum(axis=1), 32)


def _drift(n, seed):
    rng = np.random.default_rng(seed)
    return np.clip(np.cumsum(rng.uniform(-2.0, 2.0, (n, 2)), axis=0), -20, 20)


def test_recovers_pure_translation(capsys):
    cc = _cc()
    img = _phantom_projection()
    n = 40
    d_int = np.round(_drift(n, 21)).astype(int)
    proj = np.stack([np.roll(img, tuple(d), axis=(0, 1)) for d in d_int]).astype(np.float32)
    off, _ = cc.cross_correlation_numpy(proj)
    mo, _, _ = xcorr_model.chain_numpy(proj)
    assert np.array_equal(off, mo)
    assert np.array_equal(off, (d_int[0] - d_int).astype(np.float64))
    d = _drift(n, 22)
    proj = np.stack([ps.fourier_shift(img, s) for s in d]).astype(np.float32)
    off, _ = cc.cross_correlation_skimage(proj)
    mo, _, mm = xcorr_model.chain_skimage(proj)
    _check_skimage_offsets(off, mo, mm, "translation")
    err = np.abs(off - (d[0] - d)).max(axis=1)
    with capsys.disabled():
        print("\n[pure translation] skimage path |offset + drift|: step 1 %.3f px, max over %d steps %.3f px" % (err[1], n, err.max()))
    # The chain registers each projection to the previous spline-shifted one, so its error is a walk: the numpy model measures
    # 0.007 px at step 1 and 1.27 px at step 40 on this series; what is asserted here is what the model meets.
    assert err[1] <= 0.02 and err.max() <= 1.5


def test_recovers_z_drift_of_rotating_series(capsys):
    cc = _cc()
    from tomography_alignment_amd.examples.generate_data import make
    p = make(size=128, n_proj=90, seed=0, ang_deg=0.01, shift_px=0.01)["projections"].astype(np.float64)
    d_int = np.round(_drift(90, 23)).astype(int)
    proj = np.stack([np.roll(q, tuple(d), axis=(0, 1)) for q, d in zip(p, d_int)]).astype(np.float32)
    off, _ = cc.cross_correlation_numpy(proj)
    mo, _, _ = xcorr_model.chain_numpy(proj)
    assert np.array_equal(off, mo)
    ez_n = np.max(np.abs(off[:, 1] - (d_int[0, 1] - d_int[:, 1])))
    d = _drift(90, 24)
    proj = np.stack([ps.fourier_shift(q, s) for q, s in zip(p, d)]).astype(np.float32)
    off, _ = cc.cross_correlation_skimage(proj)
    mo, _, mm = xcorr_model.chain_skimage(proj)
    _check_skimage_offsets(off, mo, mm, "rotating")
    ez_s = np.max(np.abs(off[:, 1] - (d[0, 1] - d[:, 1])))
    with capsys.disabled():
        print("\n[rotating series] max |z offset + z drift|: numpy path %.2f px, skimage path %.2f px" % (ez_n, ez_s))
    assert ez_n <= 1.0 and ez_s <= 1.0


def test_edge_cases():
    cc = _cc()
    for dt in (np.float32, np.float64):
        for n in (0, 1):
            p = np.random.default_rng(n).standard_normal((n, 16, 12)).astype(dt)
            for fn in (cc.cross_correlation_numpy, cc.cross_correlation_skimage):
                off, al = fn(p)
                assert off.shape == (n, 2) and not off.any() and al.dtype == dt and np.array_equal(al, p) and al is not p
    # an axis of length 1: that shift is 0, the other recovered
    row = np.sin(np.linspace(0, 6, 40))[None, :] + np.cos(np.linspace(0, 17, 40))[None, :]
    s, _, _ = cc.phase_cross_correlation(row, ps.fourier_shift(row, (0.0, -3.0)), upsample_factor=16)
    assert s[0] == 0.0 and abs(s[1] - 3.0) <= 1.0 / 16, s
    p = np.stack([ps.fourier_shift(row, (0.0, k)) for k in (0.0, 1.0, 2.5)]).astype(np.float32)
    off, al = cc.cross_correlation_skimage(p)
    mo, ma, _ = xcorr_model.chain_skimage(p)
    assert np.all(off[:, 0] == 0.0) and np.max(np.abs(off - mo)) <= 0.01 and rel_max(al, ma) < 1e-6
    with pytest.raises(TypeError):
        cc.cross_correlation_numpy(np.zeros((3, 8, 8), np.int32))


def test_no_device_memory_left_behind():
    from tomography_alignment_amd import _xcorr_lib
    cc = _cc()
    g = golden("g15_align_cc")
    before = _xcorr_lib.device_bytes()
    assert before == 0, before
    for k in range(5):
        cc.cross_correlation_numpy(g["proj"][:4])
        cc.cross_correlation_skimage(g["proj"][:4])
        cc.phase_cross_correlation(g["pair0_ref"], g["pair0_mov"], upsample_factor=16)
        cc.crossCorrelationAlign(g["proj"][1], g["proj"][0], 1.0, 1.0)
    assert _xcorr_lib.device_bytes() == 0
    with _xcorr_lib.XcorrHandle() as h:
        cc.cross_correlation_numpy(g["proj"], handle=h)
        assert _xcorr_lib.device_bytes() > 0
    assert _xcorr_lib.device_bytes() == 0
