"""CPU tests of align/align_cc.py's host side: the pcc stand-in (what the GPU module computes) recovers known sub-pixel shifts, and the
image-axis-order filters are the reference's for square images."""
import numpy as np
import pytest

import pcc_standin as ps

from tomography_alignment_amd.align import align_cc


@pytest.mark.parametrize("u", [1, 16, 100])
@pytest.mark.parametrize("norm", ["phase", None])
def test_standin_recovers_fourier_shifts(u, norm):
    rng = np.random.default_rng(u + (norm is None))
    for shp in [(64, 64), (63, 80), (48, 33)]:
        # band-limited, so that a sub-pixel Fourier shift is a true translation (no Nyquist term to lose in the real part)
        f = np.fft.fft2(rng.standard_normal(shp)) * np.exp(-30 * (np.fft.fftfreq(shp[0])[:, None] ** 2 + np.fft.fftfreq(shp[1])[None] ** 2))
        for ax, n in enumerate(shp):
            if n % 2 == 0:
                f[(slice(None),) * ax + (n // 2,)] = 0
        img = np.real(np.fft.ifft2(f))
        for _ in range(3):
            true = rng.uniform(-6, 6, 2)
            s, err, ph = ps.phase_cross_correlation(img, ps.fourier_shift(img, true), upsample_factor=u, normalization=norm)
            assert np.all(np.abs(s + true) <= 1.0 / u), (shp, true, s)
            assert np.isfinite(err) and np.isfinite(ph)


def test_standin_length_one_axis():
    row = np.sin(np.linspace(0, 7, 40))[None, :]
    s, _, _ = ps.phase_cross_correlation(row, ps.fourier_shift(row, (0.0, 2.5)), upsample_factor=16)
    assert s[0] == 0.0 and abs(s[1] + 2.5) <= 1.0 / 16


def _reference_filters(nx, nz):
    """align/align_cc.py:49-59 of the reference, verbatim in its arithmetic: filters of shape (nz, nx)."""
    kx = np.fft.fftfreq(nx)
    kz = np.fft.fftfreq(nz)
    [kx, kz] = np.meshgrid(kx, kz)
    abs_k = np.sqrt(kx ** 2 + kz ** 2)
    cutoff = 4
    filter_k = (abs_k <= (0.5 / cutoff)) * np.sin(2 * np.pi * cutoff * abs_k) ** 2
    x = np.linspace(1, nx, nx)
    z = np.linspace(1, nz, nz)
    [x, z] = np.meshgrid(x, z)
    filter_r = (np.sin(np.pi * x / nx) * np.sin(np.pi * z / nz)) ** 2
    return filter_r, filter_k


@pytest.mark.parametrize("n", [1, 2, 7, 64, 100])
def test_square_filters_are_the_reference_filters(n):
    fr, fk = align_cc.cc_filters(n, n)
    rr, rk = _reference_filters(n, n)
    assert np.array_equal(fr, rr) and np.array_equal(fk, rk)
    sr, sk = ps.cc_filters(n, n)
    assert np.array_equal(sr, rr) and np.array_equal(sk, rk)


def test_nonsquare_filters_follow_image_axes():
    fr, fk = align_cc.cc_filters(30, 50)
    rr, rk = _reference_filters(30, 50)
    assert fr.shape == fk.shape == (30, 50)
    assert np.allclose(fr, rr.T, rtol=0, atol=1e-15) and np.allclose(fk, rk.T, rtol=0, atol=1e-15)


def test_bad_input_is_rejected_before_any_device_call():
    with pytest.raises(TypeError):
        align_cc.cross_correlation_numpy(np.zeros((3, 8, 8), np.int32))
    with pytest.raises(ValueError):
        align_cc.cross_correlation_skimage(np.zeros((8, 8), np.float32))
    with pytest.raises(ValueError):
        align_cc.phase_cross_correlation(np.zeros((8, 8)), np.zeros((8, 9)))
    with pytest.raises(ValueError):
        align_cc.phase_cross_correlation_batch(np.zeros((2, 8, 8)), np.zeros((2, 8, 8)), normalization="bogus")
    with pytest.raises(ValueError):
        align_cc.phase_cross_correlation_batch(np.zeros((2, 8, 8)), np.zeros((2, 8, 8)), upsample_factor=1.5)
