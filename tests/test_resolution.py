"""Host side of the Fourier shell correlation (tomography_alignment_amd/resolution.py) and the numpy model the GPU is compared with
(tests/fsc_model.py): what fixes the definition.  No GPU."""
import numpy as np
import pytest

import fsc_model as fm

from tomography_alignment_amd import resolution
from tomography_alignment_amd.recon import fbp

SHAPES = [(16, 16, 16), (15, 15, 15), (24, 32, 20), (24, 32, 21), (33, 64, 31), (12, 10)]


@pytest.mark.parametrize("shape", SHAPES)
def test_rfft_form_with_hermitian_weights_equals_the_full_transform(shape):
    rng = np.random.default_rng(1)
    a, b = rng.standard_normal(shape), rng.standard_normal(shape)
    C, PA, PB, n = fm.sums(a, b, mask=None, subtract_mean=False)
    Cf, PAf, PBf, nf, cut = fm.sums_full(a, b)
    assert np.array_equal(n, nf)
    for got, ref in ((C, Cf), (PA, PAf), (PB, PBf)):
        assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(np.abs(ref))
    # every coefficient is in a shell or in the corners beyond the smallest axis' Nyquist
    assert n.sum() + cut == np.prod(shape)


def test_cube_counts_anchor_and_integer_form():
    for N in (16, 32, 33):
        s, w, S = fm.shell_index((N, N, N))
        assert np.array_equal(s, fm.shell_index_cube_int(N))
        n = np.bincount(s[s < S], w[s < S], S)
        assert list(n[:4]) == [1, 18, 62, 98]


def test_identical_and_negated():
    a = np.random.default_rng(2).standard_normal((20, 20, 20))
    C, PA, PB, n = fm.sums(a, a)
    assert np.allclose(fm.curve(C, PA, PB)[1:], 1.0, atol=1e-12)
    C, PA, PB, n = fm.sums(a, -a)
    assert np.allclose(fm.curve(C, PA, PB)[1:], -1.0, atol=1e-12)
    c = resolution.FSCCurve(C, PA, PB, n, 20)
    assert np.allclose(c.fsc[1:], -1.0, atol=1e-12)


def test_shifted_white_noise_follows_sinc():
    """b = roll(a, d, axis 0): the curve is the average of cos(2 pi kx d / N) over a shell, sin(t)/t with t = 2 pi s d / N.  Pins the
    frequency axis and the shell convention.  The bound is statistical and scales with 1/sqrt(count): a shell of n coefficients (n/2
    independent ones) averages terms of variance <= 1/2 around the sphere's average, so the standard error is at most 1/sqrt(n).  The
    shell's width (r within s +- 1/2, weighted with r^2) adds a systematic part: t is off by about 2 pi d / (6 N s) on average and
    spreads by +- pi d / N, which moves the curve by less than 0.005 from shell 6 on.  Per shell: 4 standard errors plus 0.01.  Pooled:
    the root mean square of z = deviation * sqrt(n) over the 27 shells is below sqrt(1.54^2 + 0.55^2) = 1.64 (unit normals at 4 sigma
    of the chi-square, plus the systematic part at the largest n); a shell index off by one gives more than 2."""
    N, d = 64, 3
    a = np.random.default_rng(3).standard_normal((N, N, N))
    C, PA, PB, n = fm.sums(a, np.roll(a, d, axis=0), mask=None, subtract_mean=False)
    f = fm.curve(C, PA, PB)
    s = np.arange(f.size)

    def z_of(shift):
        t = 2 * np.pi * (s + shift) * d / N
        return ((f - np.sinc(t / np.pi)) * np.sqrt(n))[6:]

    z = z_of(0)
    dev = np.abs(z) / np.sqrt(n[6:])
    print("shifted noise: largest deviation from sin(t)/t %.4f, largest |z| %.2f, rms z %.2f (one shell off: %.2f, %.2f)"
          % (dev.max(), np.abs(z).max(), np.sqrt(np.mean(z ** 2)), np.sqrt(np.mean(z_of(1) ** 2)), np.sqrt(np.mean(z_of(-1) ** 2))))
    assert np.all(dev < 4.0 / np.sqrt(n[6:]) + 0.01)
    assert np.sqrt(np.mean(z ** 2)) < 1.7
    assert np.sqrt(np.mean(z_of(1) ** 2)) > 2.0 and np.sqrt(np.mean(z_of(-1) ** 2)) > 2.0
    # the shift along another axis gives the same curve up to the statistics: the axis scales agree (a cube cannot tell more)
    C2, PA2, PB2, _ = fm.sums(a, np.roll(a, d, axis=2), mask=None, subtract_mean=False)
    assert np.all(np.abs(fm.curve(C2, PA2, PB2) - f)[6:] < 8.0 / np.sqrt(n[6:]))


def test_signal_plus_independent_noise_is_one_half():
    N = 64
    rng = np.random.default_rng(4)
    sgn, n1, n2 = (rng.standard_normal((N, N, N)) for _ in range(3))
    C, PA, PB, n = fm.sums(sgn + n1, sgn + n2, mask=None, subtract_mean=False)
    f = fm.curve(C, PA, PB)
    se = (1 - 0.25) / np.sqrt(n / 2)
    z = ((f - 0.5) / se)[4:]
    print("signal + noise: pooled mean %.4f, largest |z| over %d shells %.2f" % (np.average(f[4:], weights=n[4:]), z.size, np.abs(z).max()))
    assert np.abs(z).max() < 4.5


def test_sphere_mask_model():
    m = fm.sphere_mask((32, 32, 32))
    assert m[16, 16, 16] == 1.0 and m[0, 0, 0] == 0.0 and m.min() >= 0 and m.max() <= 1
    assert m[16, 16, 16 + 9] == 1.0                      # d = 9.5 <= R = 10
    assert 0 < m[16, 16, 16 + 12] < 1                    # d = 12.5 in the edge
    assert abs(m[16, 16, 28] - 0.5 * (1 + np.cos(np.pi * (np.sqrt(0.5 + 12.5 ** 2) - 10) / 6))) < 1e-15
    assert m[0, 16, 31] == 0.0                           # d = 21.9 >= R + E = 16


def test_thresholds():
    n = np.array([1.0, 4.0, 100.0, 1e12])
    hb = resolution.threshold_curve("half-bit", n)
    ob = resolution.threshold_curve("one-bit", n)
    assert np.allclose(hb, [(0.2071 + 1.9102) / (1.2071 + 0.9102), (0.2071 + 0.9551) / (1.2071 + 0.4551), (0.2071 + 0.19102) / (1.2071 + 0.09102),
                            0.2071 / 1.2071], atol=2e-6)
    assert np.allclose(ob, [(0.5 + 2.4142) / (1.5 + 1.4142), (0.5 + 1.2071) / (1.5 + 0.7071), (0.5 + 0.24142) / (1.5 + 0.14142), 1 / 3.0], atol=2e-6)
    assert np.all(resolution.threshold_curve("0.143", n) == 0.143) and np.all(resolution.threshold_curve("0.5", n) == 0.5)
    assert resolution.threshold_curve("half-bit", np.array([0.0]))[0] == 1.0
    with pytest.raises(ValueError):
        resolution.threshold_curve("two-bit", n)


def _curve(f, nmax=None, voxel_size=1.0):
    f = np.asarray(f, np.float64)
    return resolution.FSCCurve(f, np.ones_like(f), np.ones_like(f), np.full(f.size, 1e6), 2 * (f.size - 1) if nmax is None else nmax, voxel_size)


def test_resolution_on_hand_made_curves():
    # between shells 3 and 4: 0.8 -> 0.2 meets 0.5 half way
    c = _curve([1, 1, 0.9, 0.8, 0.2, 0.1, 0.0, 0.0, 0.0])
    shell, status = c.crossing("0.5")
    assert status == "crossed" and abs(shell - 3.5) < 1e-12
    assert abs(c.resolution("0.5") - 16 / 3.5) < 1e-12
    assert abs(_curve([1, 1, 0.9, 0.8, 0.2, 0.1, 0.0, 0.0, 0.0], voxel_size=2.0).resolution("0.5") - 2 * 16 / 3.5) < 1e-12
    assert np.allclose(c.freq, np.arange(9) / 16.0)
    # never crosses
    c = _curve([1, 1, 0.9, 0.9, 0.8, 0.8, 0.7, 0.7, 0.6])
    assert c.crossing("0.5") == (None, "none") and c.resolution("0.5") is None
    # only at the last shell: at Nyquist, no number
    c = _curve([1, 1, 0.9, 0.9, 0.8, 0.8, 0.7, 0.7, 0.1])
    assert c.crossing("0.5") == (None, "nyquist") and c.resolution("0.5") is None and c.nyquist == 2.0
    # a dip that recovers: the first crossing counts
    c = _curve([1, 1, 0.9, 0.3, 0.9, 0.9, 0.2, 0.0, 0.0])
    shell, status = c.crossing("0.5")
    assert status == "crossed" and abs(shell - (2 + 0.4 / 0.6)) < 1e-12
    # shell 0 is not looked at (mean-free inputs leave 0 / 0 there)
    c = _curve([0, 1, 0.9, 0.8, 0.2, 0.1, 0.0, 0.0, 0.0])
    assert abs(c.crossing("0.5")[0] - 3.5) < 1e-12
    # the bit curves use the shell's count
    f = np.array([1, 1, 0.9, 0.6, 0.3, 0.1, 0.0])
    c = resolution.FSCCurve(f, np.ones(7), np.ones(7), np.array([1, 18, 62, 98, 210, 350, 450.0]), 12)
    d = f - resolution.threshold_curve("half-bit", c.count)
    assert d[4] > 0 > d[5]
    assert abs(c.crossing("half-bit")[0] - (4 + d[4] / (d[4] - d[5]))) < 1e-12


def test_pool_curves_adds_the_sums():
    rng = np.random.default_rng(5)
    cs = [resolution.FSCCurve(rng.random(5), rng.random(5) + 1, rng.random(5) + 1, np.arange(5.0) + 1, 8) for _ in range(3)]
    p = resolution.pool_curves(cs)
    assert np.allclose(p.C, sum(c.C for c in cs)) and np.allclose(p.count, 3 * (np.arange(5.0) + 1))
    assert np.allclose(p.fsc, p.C / np.sqrt(p.PA * p.PB))


@pytest.mark.parametrize("n_proj", [90, 91, 10, 7])
def test_half_split_is_the_same_for_every_world(n_proj):
    phi = np.linspace(0, np.pi, n_proj, endpoint=False)
    (e1, pe1), (o1, po1) = resolution.split_rows(n_proj)
    assert np.array_equal(e1, np.arange(0, n_proj, 2)) and np.array_equal(o1, np.arange(1, n_proj, 2))
    assert np.array_equal(pe1, np.arange(e1.size)) and np.array_equal(po1, np.arange(o1.size))
    for parity in (0, 1):
        w = resolution.half_weights(phi, parity)
        assert abs(w.sum() - np.pi) < 1e-12
        assert np.array_equal(w, fbp.angle_weights(phi[parity::2]))
    for world in (1, 2, 3):
        ev, od, wsum = [], [], [0.0, 0.0]
        for rank in range(world):
            held = np.array_split(np.arange(n_proj), world)[rank]
            (e, pe), (o, po) = resolution.split_rows(n_proj, held)
            assert set(e) <= set(held) and set(o) <= set(held)
            # a rank's rows of a half are every second row of its block, which is what the device gather takes
            for rows in (e, o):
                if rows.size:
                    first = int(np.searchsorted(held, rows[0]))
                    assert np.array_equal(held[first::2][:rows.size], rows)
            assert np.array_equal(np.arange(0, n_proj, 2)[pe], e) and np.array_equal(np.arange(1, n_proj, 2)[po], o)
            ev.append(e)
            od.append(o)
            wsum[0] += resolution.half_weights(phi, 0)[pe].sum()
            wsum[1] += resolution.half_weights(phi, 1)[po].sum()
        assert np.array_equal(np.concatenate(ev), e1) and np.array_equal(np.concatenate(od), o1)
        assert abs(wsum[0] - np.pi) < 1e-12 and abs(wsum[1] - np.pi) < 1e-12


def test_argument_checks_need_no_device():
    a = np.zeros((8, 8, 8), np.float32)
    with pytest.raises(ValueError):
        resolution.fsc(a, np.zeros((8, 8, 9), np.float32))
    with pytest.raises(ValueError):
        resolution.fsc(a, a, mask="cube")
    with pytest.raises(ValueError):
        resolution.fsc(a[0], a[0])
    with pytest.raises(ValueError):
        resolution.FSCCurve([1.0], [1.0], [1.0], [1.0], 2, voxel_size=0.0)
