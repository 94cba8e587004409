#!/usr/bin/env python3
"""
G15: the reference's own align/align_cc.py, unedited, on a seeded drifting series and on pcc pairs.

The reference imports `phase_cross_correlation` from scikit-image; a `skimage.registration` module placed in sys.modules supplies
it from the numpy stand-in tests/pcc_standin.py (float64 throughout).  scipy.ndimage is real (scipy 1.15.3 wrote this file).

Inputs: 12 projections at 64^2 (float32): a smooth random image under a seeded drift, circular Fourier shifts with integer and
sub-pixel parts, plus a little noise per projection.  Pairs: (64, 64), (63, 80) and (1, 40) images and a known Fourier shift,
for upsample_factor 1, 16 and 100 and normalization "phase" and None.
Recorded: the series, both chains' offsets and aligned_proj, per step the argmax margins (relative margin of the maximum over the
runner-up: numpy path, skimage coarse and fine), and per pair shifts, error, phasediff and margins.
Run in the authoring environment:  REF=<reference checkout> python tests/golden/make_golden_g15.py
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.environ["REF"])
import numpy as np  # noqa: E402
import pcc_standin as ps  # noqa: E402

reg = types.ModuleType("skimage.registration")
reg.phase_cross_correlation = ps.phase_cross_correlation
sk = types.ModuleType("skimage")
sk.registration = reg
sys.modules["skimage"] = sk
sys.modules["skimage.registration"] = reg
from align import align_cc  # noqa: E402

SHAPES = [(64, 64), (63, 80), (1, 40)]
UPS = [1, 16, 100]
NORMS = ["phase", None]


def smooth_image(rng, shape, sigma=3.0):
    f = np.fft.fftn(rng.standard_normal(shape))
    kk = [np.fft.fftfreq(n).reshape([-1 if a == ax else 1 for a in range(len(shape))]) for ax, n in enumerate(shape)]
    f *= np.exp(-2 * (np.pi * sigma) ** 2 * sum(k ** 2 for k in kk))
    img = np.real(np.fft.ifftn(f))
    return img / np.abs(img).max()


def series(rng, n=12, size=64):
    base = smooth_image(rng, (size, size)) + 0.5 * smooth_image(rng, (size, size), 1.0)
    steps = np.round(rng.uniform(-3, 3, (n, 2)) * 4) / 4 + rng.uniform(-0.1, 0.1, (n, 2)) * (rng.random((n, 1)) < 0.5)
    steps[0] = 0
    drift = np.cumsum(steps, axis=0)
    proj = np.stack([ps.fourier_shift(base, d) + 0.01 * rng.standard_normal((size, size)) for d in drift]).astype(np.float32)
    return proj, drift


def numpy_margins(proj, aligned):
    n, nx, nz = proj.shape
    filter_r, filter_k = ps.cc_filters(nx, nz)
    out = [np.inf]
    for i in range(1, n):
        image, reference = proj[i], aligned[i - 1]
        image_f = np.fft.fft2((image - np.mean(image)) * filter_r)
        reference_f = np.fft.fft2((reference - np.mean(reference)) * filter_r)
        xcor = abs(np.fft.ifft2(np.conj(image_f) * reference_f * filter_k))
        out.append(ps._argmax_margin(xcor)[1])
    return np.array(out)


def main():
    rng = np.random.default_rng(15)
    proj, drift = series(rng)
    out = dict(proj=proj, drift=drift)
    off_n, al_n = align_cc.cross_correlation_numpy(proj)
    out.update(np_offsets=off_n, np_aligned=al_n, np_margin=numpy_margins(proj, al_n))
    off_s, al_s = align_cc.cross_correlation_skimage(proj)
    m = [(np.inf, np.inf)] + [ps.phase_cross_correlation_margins(al_s[i - 1], proj[i], 100)[3] for i in range(1, len(proj))]
    out.update(sk_offsets=off_s, sk_aligned=al_s, sk_margin=np.array(m))
    cor = align_cc.cor_flipping(proj[0], proj[3])
    out.update(cor_flipping=np.float64(cor))
    for k, shp in enumerate(SHAPES):
        ref = smooth_image(rng, shp, 2.0) + 0.05 * rng.standard_normal(shp)
        true = np.array([rng.uniform(-5, 5) if shp[0] > 1 else 0.0, rng.uniform(-5, 5)])
        mov = ps.fourier_shift(ref, true) + 0.02 * rng.standard_normal(shp)
        out["pair%d_ref" % k] = ref.astype(np.float32)
        out["pair%d_mov" % k] = mov.astype(np.float32)
        out["pair%d_true" % k] = true
        for u in UPS:
            for norm in NORMS:
                tag = "pair%d_u%d_%s" % (k, u, norm or "none")
                s, e, p, mg = ps.phase_cross_correlation_margins(out["pair%d_ref" % k], out["pair%d_mov" % k], u, norm)
                out[tag + "_shifts"], out[tag + "_error"], out[tag + "_phasediff"] = s, np.float64(e), np.float64(p)
                out[tag + "_margin"] = np.array(mg)
    path = os.path.join(HERE, "g15_align_cc.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    print("numpy offsets", off_n.tolist())
    print("skimage offsets", np.round(off_s, 3).tolist())
    print("min margins numpy %.2e skimage coarse %.2e fine %.2e" % (out["np_margin"].min(), out["sk_margin"][:, 0].min(),
                                                                   out["sk_margin"][:, 1].min()))


if __name__ == "__main__":
    main()
