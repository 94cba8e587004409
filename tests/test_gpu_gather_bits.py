"""The gather projectors keep their bits: `forward` (gather path on), `adjoint` and `tomo_adjoint_update` (clamp and error sum on) give
the float32 bytes that the library of the commit BEFORE the set-up / addressing rework of k_fwd_gather_flat and k_adj_gather_flat gave --
that rework moves no sum: per accumulator still previous sum, W0, W1, W2, W3; slabs and windows ascending.

tests/golden/gather_bits_parent.json holds, per case, the SHA-256 of the inputs and of the three outputs and the error sum, recorded on an
MI355X from that earlier commit's library (never from the code under test):

    TOMO_HIP_LIB=/path/to/the/earlier/libtomo_hip.so python tests/test_gpu_gather_bits.py out.json

The error sum of the update is compared to 1e-13 relative, not by bits: its double atomics arrive in any order.

The cases are the smallest at which the reworked code can take another path: the three shapes of tests/test_gpu_forward_gather.py; two
with four live waves per work-group; zero bands that leave 1, 2 and 3 live waves; walks of 1, 2, 3, 5 and 9 slabs (group tails, slab
counts that are no multiple of the live waves); 17 "special" + 9 random angles; tau = 0 and tau != 0; step 1.0 and 0.95; a detector wider
(and narrower) than the volume; a volume of exactly 4 GiB (forward only: the one size at which a bound on the loads' 32-bit offsets can
cut off the last voxel); and one case whose wave-steps span more than FGROWS = 24 lines, i.e. need a second window (shown on the host
with the counting of tools/fwd_gather_model.py, asserted below)."""
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_FILE = os.path.join(ROOT, "tests", "golden", "gather_bits_parent.json")
FGROWS = 24

SPECIAL = [0.0, np.pi / 2, np.pi,                             # samples on integers
           np.arctan(0.5) - 1e-3, np.arctan(0.5) + 1e-3,      # the 3 / 4-weight switch
           np.pi / 4 - 1e-3, np.pi / 4 + 1e-3,                # the walk switch, inside one group of eight
           3 * np.pi / 4 - 1e-3, 3 * np.pi / 4 + 1e-3]

# the second-window case: eight consecutive poses of ONE list (x walk, three weights: 2 |cos| <= |sin|), so they form one group of eight
# rays per row whose lines fan out by up to |cot 64 deg - cot 116 deg| = 0.98 lines per slab of distance from the rotation centre
WIN2_N = 80
WIN2_PHI = np.deg2rad(np.linspace(64.0, 116.0, 8))

# name -> (shape, ndx - nx, angle kind, pose kind, step, z band of non-zero planes or None)
#   pose kinds: "plain" (tau = 0, no shifts), "cor" (tau = 0: integer z offsets, a COR shift), "shift" (tau != 0: fractional x / z translations)
CASES = {
    "s24_shift":     ((24, 24, 64), 0, "special26", "shift", 1.0, None),
    "s17_cor_wide":  ((17, 23, 65), 7, "special26", "cor", 0.95, None),
    "s40_narrow":    ((40, 9, 130), -5, "special26", "shift", 1.0, None),
    "w4_shift":      ((9, 17, 256), 0, "special26", "shift", 0.95, None),           # four live waves, 9 and 17 slabs
    "w4_plain_wide": ((16, 5, 200), 7, "special26", "plain", 1.0, None),            # four waves, the last chunk partial; 16 and 5 slabs
    "nl1":           ((9, 17, 256), 0, "special26", "plain", 1.0, (70, 120)),       # one live chunk (not the first of its work-group)
    "nl2_shift":     ((9, 17, 256), 0, "special26", "shift", 1.0, (70, 180)),       # two: 9 and 17 slabs are odd tails of groups of two
    "nl3":           ((9, 17, 256), 0, "special26", "plain", 0.95, (10, 180)),      # three: 9 = 3 groups, 17 = 5 groups + 2
    "slabs_1_2":     ((1, 2, 70), 0, "special26", "shift", 1.0, None),
    "slabs_2_3":     ((2, 3, 64), 3, "special26", "plain", 1.0, None),
    "slabs_3_5":     ((3, 5, 64), 0, "special26", "shift", 0.95, None),
    "win2":          ((WIN2_N, WIN2_N, 64), 0, "win2", "plain", 1.0, None),
    # a volume of exactly 4 GiB, the largest the gather forward takes: its 32-bit byte offsets and whatever bounds its loads must reach the
    # last voxel (a fault of that kind shows at no smaller size).  Forward only; one y-walk and one x-walk pose whose edge rays pass that voxel
    "vol_4gib":      ((1024, 1024, 1024), 0, "axes", "plain", 1.0, None),
}
FORWARD_ONLY = ("vol_4gib",)


def case_inputs(name):
    """-> (shape, ndet, step, cor, poses-array arguments, host arrays); everything from one seeded generator per case."""
    shape, wide, akind, pkind, step, band = CASES[name]
    rng = np.random.default_rng(int(hashlib.sha256(name.encode()).hexdigest()[:8], 16))
    if akind == "win2":
        phi = WIN2_PHI.copy()
    elif akind == "axes":
        phi = np.array([0.0, np.pi / 2])
    else:                                   # 17 "special" angles (the nine switches + eight random ones) plus 9 random ones
        phi = np.array(SPECIAL + list(rng.uniform(0.0, np.pi, 8)) + list(rng.uniform(0.0, np.pi, 9)))
    n = phi.size
    xyz, cor = np.zeros((n, 3)), None
    if pkind == "shift":
        xyz[:, 0] = rng.uniform(-3.0, 3.0, n)
        xyz[:, 2] = rng.uniform(-21.0, 21.0, n)
    elif pkind == "cor":
        cor = np.array([1.37, 0.0, 0.0])
        xyz[:, 2] = np.round(rng.uniform(-9.0, 9.0, n))
    ndet = (shape[0] + wide, shape[2])
    n_vox, n_sino = int(np.prod(shape)), n * ndet[0] * ndet[1]
    if name in FORWARD_ONLY:                # (a seeded x slab, scaled per slab: a generator would take longer than the kernels)
        x = rng.uniform(0.1, 1.0, (1,) + shape[1:]).astype(np.float32) * (1.0 + np.arange(shape[0], dtype=np.float32) / 4096.0)[:, None, None]
        return shape, ndet, step, cor, (phi, xyz), {"x": x.ravel(), "y": np.zeros(n_sino, np.float32)}
    x = rng.uniform(0.1, 1.0, shape).astype(np.float32)
    y = rng.standard_normal((n, ndet[0], ndet[1])).astype(np.float32)
    if band is not None:                    # zero z bands: dead chunks for the forward (volume planes) and the adjoint (detector planes)
        x[:, :, :band[0]] = 0
        x[:, :, band[1]:] = 0
        y[:, :, :band[0]] = 0
        y[:, :, band[1]:] = 0
    h = {"x": x.ravel(), "y": y.ravel(), "rec": rng.standard_normal(n_vox).astype(np.float32),
         "V": rng.uniform(0.1, 1.0, n_vox).astype(np.float32), "gt": rng.standard_normal(n_vox).astype(np.float32)}
    assert h["y"].size == n_sino
    return shape, ndet, step, cor, (phi, xyz), h


def sha(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return hashlib.sha256(a.tobytes()).hexdigest()


def compute(name):
    """The three outputs of one case on the loaded library -> dict of digests (and the error sum)."""
    from tomography_alignment_amd import _lib
    from tomography_alignment_amd.backend import HipBackend
    from tomography_alignment_amd.utilities.geometry import Geometry
    shape, ndet, step, cor, (phi, xyz), h = case_inputs(name)
    n = phi.size
    geo = Geometry(n, np.array(shape), np.ones(3), np.array(ndet), np.ones(2), cor_shift=cor, step_size=step)
    be = HipBackend(geo)
    ctx = be.ctx
    ctx.set_option("fwd_flat_gather", 1)
    poses = _lib.poses_array(phi, np.zeros(n), np.zeros(n), xyz, np.zeros(3) if cor is None else cor)
    out = {"inputs": hashlib.sha256(b"".join(h[k][:1 << 22].tobytes() + h[k][-(1 << 22):].tobytes() for k in sorted(h)) + poses.tobytes()).hexdigest()}
    ctx.profile_reset()
    ctx.profile_enable(True)
    fwd = be.forward(poses, be.upload(h["x"]), be.zeros(h["y"].size)).download()
    assert ctx.profile_get("k_fwd_tile_flat")[0] == 1
    # (both flat forwards carry that profile name.  What shows that the gather one ran: the default one adds the same products in another
    #  order, so its bits differ -- recorded per case as "gather_differs" and asserted again by the test)
    ctx.set_option("fwd_flat_gather", 0)
    out["gather_differs"] = bool(np.any(be.forward(poses, be.upload(h["x"]), be.zeros(h["y"].size)).download().view(np.uint32) != fwd.view(np.uint32)))
    ctx.set_option("fwd_flat_gather", 1)
    if name in FORWARD_ONLY:
        ctx.profile_enable(False)
        assert np.all(fwd[[0, -1]] != 0)
        out.update(forward=sha(fwd))
        return out
    adj = be.adjoint(poses, be.upload(h["y"]), be.zeros(h["x"].size)).download()
    assert ctx.profile_get("k_adj_gather_flat")[0] == 1 and ctx.profile_get("k_adj_tile")[0] == 0
    rec = be.upload(h["rec"])
    fused, err = be.adjoint_update(poses, be.upload(h["y"]), rec, be.upload(h["V"]), True, be.upload(h["gt"]))
    ctx.profile_enable(False)
    assert fused and ctx.profile_get("k_adj_gather_flat")[0] == 2
    upd = rec.download()
    assert np.any(fwd != 0) and np.any(adj != 0) and np.count_nonzero(upd != h["rec"]) > 0
    out.update(forward=sha(fwd), adjoint=sha(adj), update=sha(upd), err=float(err))
    return out


def load_golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gather_bits_are_the_parents(name):
    want = load_golden()[name]
    got = compute(name)
    print("[%s] " % name + ", ".join("%s %s" % (k, str(got[k])[:18]) for k in sorted(got)) + (" (err recorded: %.17g)" % want["err"] if "err" in want else ""))
    assert sorted(got) == sorted(want)
    assert got["inputs"] == want["inputs"], "this numpy's generator gives other inputs than the recorded ones"
    assert want["gather_differs"] and got["gather_differs"], "the forward under test is not told apart from the default flat forward"
    for k in ("forward", "adjoint", "update"):
        if k in want:
            assert got[k] == want[k], "%s: %s differs from the recorded bits" % (name, k)
    if "err" in want:
        assert abs(got["err"] - want["err"]) <= 1e-13 * abs(want["err"])


def fwd_model():
    spec = importlib.util.spec_from_file_location("fwd_gather_model", os.path.join(ROOT, "tools", "fwd_gather_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_second_window_case_needs_a_second_window():
    """tools/fwd_gather_model.py's counting for the eight poses of "win2" (one group: consecutive poses of the x-walk, three-weight list):
    some live wave-step has wave_max(L0) - wave_min(L0) >= FGROWS - 3 + 1, the kernel's rule for a further window -- by a margin of 8
    lines, far more than the phase of the samples along the rays (the model's own ray start) can move a line index."""
    shape, _, akind, pkind, step, _ = CASES["win2"]
    assert akind == "win2" and pkind == "plain" and step == 1.0 and shape[0] == shape[1] == WIN2_N
    s, c = np.abs(np.sin(WIN2_PHI)), np.abs(np.cos(WIN2_PHI))
    assert np.all(s >= c) and np.all(2 * c <= s)                    # all eight in the x-walk, NW = 3 list: one group of eight
    m = fwd_model()
    lmin, lmax, live, _ = m.group_stats([(p, 0.0) for p in WIN2_PHI], 0, WIN2_N, [FGROWS], 8)
    sw = FGROWS - 3 + 1
    span = np.where(live, lmax - lmin, 0)
    n_two = int((span >= sw).sum())
    print("win2: %d of %d live wave-steps need a second window (advance %d); widest first-line span %d" % (n_two, int(live.sum()), sw, int(span.max())))
    assert span.max() >= sw + 8 and n_two > 0                       # (the widest steps, span >= 2 * advance, take a third window too)


if __name__ == "__main__":      # the recorder: the EARLIER commit's library only
    sys.path.insert(0, ROOT)
    if not os.environ.get("TOMO_HIP_LIB"):
        sys.exit("set TOMO_HIP_LIB to the library of the commit before the change under test: digests are never taken from the code under test")
    rec = {name: compute(name) for name in sorted(CASES)}
    again = {name: compute(name) for name in sorted(CASES)}
    for name in rec:                                                 # the recorded library repeats its own bits
        assert all(rec[name][k] == again[name][k] for k in rec[name] if k != "err"), name
    with open(sys.argv[1], "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    assert all(r["gather_differs"] for r in rec.values()), [n for n in rec if not rec[n]["gather_differs"]]
    print("recorded %d cases from %s" % (len(rec), os.environ["TOMO_HIP_LIB"]))
