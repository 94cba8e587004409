"""numpy model of the zinger removal and the 2-D median filter of tomography_alignment_amd/preprocess.py (remove_outlier, median_filter),
written as include/tomo_prep.h specifies `outlier`: a size x size window per pixel inside its own frame with half-sample-symmetric
reflection, uint16 ordered by value and float32 by the stripe sort's key, the median decoded from its key, one float32 subtraction and a
compare.  Frames are [n][rows][cols] or one [rows][cols] image, uint16 or float32; every frame is independent."""
import numpy as np

from prep_model import stripe_keys

OUTLIER, MEDIAN = "outlier", "median"
QUIET_NAN = 0x7fc00000


def keys(a):
    """The order of the window's values as int64 keys: uint16 by value, float32 by stripe_keys (-0 -> +0, every NaN above +inf)."""
    a = np.asarray(a)
    return a.astype(np.int64) if a.dtype == np.uint16 else stripe_keys(a)


def decode(k, dtype):
    """The value a key stands for: the canonical +0 for both zeros, the quiet NaN 0x7fc00000 for every NaN."""
    if np.dtype(dtype) == np.uint16:
        return k.astype(np.uint16)
    k = k.astype(np.int64)
    u = np.where(k & 0x80000000, k ^ 0x80000000, (~k) & 0xffffffff)
    u = np.where(k == 0xffffffff, QUIET_NAN, u)
    return u.astype(np.uint32).view(np.float32)


def median(frames, size):
    """The window's element of rank (size^2 - 1) / 2, per pixel: a stable argsort of the keys, decoded from the key."""
    a = np.asarray(frames)
    h = size // 2
    pad = [(0, 0)] * (a.ndim - 2) + [(h, h), (h, h)]
    w = np.lib.stride_tricks.sliding_window_view(np.pad(a, pad, mode="symmetric"), (size, size), axis=(-2, -1))
    k = keys(w.reshape(w.shape[:-2] + (size * size,)))
    order = np.argsort(k, axis=-1, kind="stable")
    r = (size * size - 1) // 2
    return decode(np.take_along_axis(k, order[..., r:r + 1], axis=-1)[..., 0], a.dtype)


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def distance(frames, size, two_sided=False):
    """(med, d): the median and d = float32(v) - float32(med), |d| if two_sided, as the kernel compares it with dif."""
    a = np.asarray(frames)
    med = median(a, size)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (a.astype(np.float32) - med.astype(np.float32)).astype(np.float32)
        if two_sided:
            d = np.abs(d)
    return med, d


def apply(frames, size=3, mode=OUTLIER, dif=0.0, two_sided=False):
    """(out, count): the filtered frames in the input's dtype and, per frame (one number for a 2-D input), the pixels replaced --
    OUTLIER: those with d >= dif or a non-finite value, whether or not the median differs; MEDIAN: those whose bits changed."""
    a = np.asarray(frames)
    assert a.dtype in (np.uint16, np.float32) and a.ndim in (2, 3) and size in (3, 5, 7)
    med, d = distance(a, size, two_sided)
    if mode == MEDIAN:
        hit = bits(a) != bits(med)
    else:
        assert dif >= 0
        with np.errstate(invalid="ignore"):
            hit = d >= np.float32(dif)
        if a.dtype == np.float32:
            hit |= ~np.isfinite(a)
    out = np.where(hit, med, a).astype(a.dtype)
    if a.dtype == np.float32:                      # np.where keeps bits; make sure nothing canonicalised a payload on the way
        assert np.array_equal(bits(out)[~hit], bits(a)[~hit])
    return out, hit.reshape(hit.shape[:-2] + (-1,)).sum(axis=-1).astype(np.int64)


def remove_outlier(frames, dif, size=3, two_sided=False):
    return apply(frames, size, OUTLIER, dif, two_sided)


def median_filter(frames, size=3):
    return apply(frames, size, MEDIAN)[0]


def dif_margin(d, dif):
    """min |d - dif| / dif over the finite values of d (distance's): how far the nearest decision is from going the other way (inf for
    a dif of 0 or inf, which no rounding can move)."""
    if dif == 0 or np.isinf(dif):
        return np.inf
    d = d[np.isfinite(d)].astype(np.float64)
    return float(np.min(np.abs(d - dif)) / dif) if d.size else np.inf


def removes_exactly_the_zingers(clean, data, dif, size):
    """The check a threshold and a data set are chosen by: on the frames with zingers (examples/generate_data: data['counts'] and
    data['zinger_mask']) the model replaces exactly the zinger pixels, and on the zinger-free frames of the same seed it replaces nothing."""
    out, count = remove_outlier(data["counts"], dif, size)
    k = data["zinger_mask"].reshape(data["zinger_mask"].shape[0], -1).sum(axis=1)
    return bool(np.array_equal(out != data["counts"], data["zinger_mask"]) and np.array_equal(count, k)
                and not remove_outlier(clean["counts"], dif, size)[1].any())
