"""Case tables, data rules and the call runner of tests/test_gpu_context_state.py (no test lives here).

A `Call` is one call of the C-ABI as a solver makes it (or a short fixed sequence that only makes sense together, such as the noting
residual pass and the back-projection it serves): geometry, poses, options and host inputs.  `Runner.run` executes it on the one
long-lived context, whose device buffers are pooled by (role, size) so that addresses come back across steps, and again on a fresh
context that sees this call only; `compare` holds the two results against each other and `oracle_check` holds the long-lived one against
the float64 oracle."""
import numpy as np

from conftest import rel_max

TOL_ORACLE = 1e-5        # the suite's bar against the oracle (rel_max)
TOL_FAMILY = 5e-6        # tests/test_gpu_fuzz.py: the bar between kernel families -- here between two runs of a kernel with float atomics
TOL_DOUBLE_SUM = 1e-12   # tests/test_gpu_residual_flags.py: sums reduced with double atomics in another order

# constants of the kernels the relations below are stated in (csrc/kernels_tile.hip.h, kernels_tile_flat.hip.h, tomo_raycore.h)
ATX, FTZ, HALO = 16, 63, 2

# name -> (volume, detector)
POOL = {
    "a150": ((20, 27, 150), (36, 128)),
    "b150": ((27, 20, 150), (36, 128)),
    "a150z": ((20, 27, 150), (36, 150)),
    "small": ((12, 9, 70), (16, 80)),
    "onez": ((12, 9, 60), (16, 64)),
    "large": ((40, 33, 200), (48, 256)),
}
STEPS = (1.0, 0.5)

OPTION_SPACE = {
    "fwd_variant": (1, 2, 3), "adj_variant": (1, 2), "tile_flat": (0, 1), "adj_flat_gather": (0, 1), "fwd_flat_gather": (0, 1),
    "fused_update": (0, 1), "fwd_flat_ztiles": (1, 2), "fwd_gather_patch": (0, 1, 2), "grad_variant": (1, 2, 3, 4),
}
DEFAULTS = {"fwd_variant": 3, "adj_variant": 2, "tile_flat": 1, "adj_flat_gather": 1, "fwd_flat_gather": 1, "fused_update": 1,
            "fwd_flat_ztiles": 2, "fwd_gather_patch": 1, "grad_variant": 4}

POSE_KINDS = ("gather", "pitch13", "pitch05", "tilted", "mixed", "steep")
DET_DX = {"pitch13": 1.3, "pitch05": 0.5}          # detector x pitch of the kind's geometry (every other kind: 1)

# profile names (TOMO_LAUNCH) read after every call of the long-lived context
NAMES = ("k_fwd_tile_flat", "k_fwd_tile", "k_fwd_v1", "k_fwd_v2", "k_fwd_live", "k_adj_gather_flat", "k_adj_tile_flat", "k_adj_tile", "k_adj_v1",
         "k_pad", "k_sino_zflags", "k_residual_scale", "k_proj_grad", "k_cost_grad", "k_bp_voxel", "k_update", "k_absmax", "k_unpad")
REQUIRED = ("k_fwd_tile_flat", "k_fwd_tile", "k_fwd_v1", "k_fwd_v2", "k_adj_gather_flat", "k_adj_tile_flat", "k_adj_tile", "k_adj_v1",
            "k_pad", "k_sino_zflags", "k_residual_scale")


def vec_grid(n):
    return min((n + 255) // 256, 2048)


def note_possible(ndx, ndz, n_proj):
    """tomo_vec_residual_scale_flags: the grid stride of the vector pass must be a multiple of ndz."""
    return (vec_grid(n_proj * ndx * ndz) * 256) % ndz == 0


def check_pool_relations():
    """The buffer relations each pool entry is there for, from the numbers (see the table in tests/test_gpu_context_state.py)."""
    padded = lambda s: (s[0] + 2 * HALO) * (s[1] + 2 * HALO) * (s[2] + 2 * HALO)
    ztiles = lambda nz: (nz + 1 + FTZ - 1) // FTZ               # tile_grid(g, FTZ).x
    xcols = lambda nx: (nx + 1 + ATX - 1) // ATX                # tile_grid(g).z
    (va, da), (vb, db), (vz, dz), (vs, ds), (vo, do), (vl, dl) = (POOL[k] for k in ("a150", "b150", "a150z", "small", "onez", "large"))
    assert (va[2] + 63) // 64 == 3 and all(note_possible(da[0], da[1], n) for n in range(1, 8))
    assert padded(va) == padded(vb) and va[0] * va[1] == vb[0] * vb[1] and va != vb           # d_volpad kept
    assert (da[1], da[0], va[2]) == (db[1], db[0], vb[2])                                     # ndz, ndx, nz of ZfKey
    assert dz[1] == 150 and not any(note_possible(dz[0], dz[1], n) for n in range(1, 8))
    for v, d in ((vs, ds), (vo, do)):                           # every buffer shrinks in use
        assert all(padded(v) < padded(w) and v[0] * v[1] < w[0] * w[1] and d[0] * d[1] < e[0] * e[1] for w, e in ((va, da), (vb, db), (vz, dz), (vl, dl)))
    # FTZ = 63: 70 planes are TWO flat z tiles (k_fwd_flat_tab unless option fwd_flat_ztiles is 1); the entry with ONE z tile is "onez"
    assert ztiles(vs[2]) == 2 and ztiles(vo[2]) == 1
    assert all(padded(vl) > padded(w) and dl[0] * dl[1] > e[0] * e[1] for w, e in ((va, da), (vb, db), (vz, dz), (vs, ds), (vo, do)))
    assert xcols(vl[0]) == 3 and xcols(va[0]) == 2


class Call(object):
    """op: name in OPS; geo: (pool entry, step, detector x pitch); poses: (n, 7); opts: option -> value (the rest: DEFAULTS); a: the
    op's host inputs and parameters."""

    def __init__(self, op, geo, poses, opts=None, kind="", **a):
        self.op, self.geo, self.poses, self.kind, self.a = op, tuple(geo), np.ascontiguousarray(poses, np.float64), kind, a
        self.opts = dict(DEFAULTS)
        self.opts.update(opts or {})

    @property
    def shape(self):
        return POOL[self.geo[0]][0]

    @property
    def det(self):
        return POOL[self.geo[0]][1]

    @property
    def n(self):
        return self.poses.shape[0]

    def but(self, **kw):
        """A copy with some fields replaced (op, geo, poses, opts, kind; anything else goes to the op's inputs)."""
        c = Call(self.op, self.geo, self.poses.copy(), dict(self.opts), self.kind, **dict(self.a))
        for k, v in kw.items():
            if k == "opts":
                c.opts.update(v)
            elif k in ("op", "kind"):
                setattr(c, k, v)
            elif k == "geo":
                c.geo = tuple(v)
            elif k == "poses":
                c.poses = np.ascontiguousarray(v, np.float64)
            else:
                c.a[k] = v
        return c


def geo_of(entry, step=1.0, det_dx=1.0):
    return (entry, float(step), float(det_dx))


def geometries(c, poses=None):
    """-> (Geometry for the library, oracle Geo with the poses' rotation-centre shifts)."""
    from oracle import oracle as orc
    from tomography_alignment_amd.utilities.geometry import Geometry
    poses = c.poses if poses is None else poses
    entry, step, det_dx = c.geo
    shape, det = POOL[entry]
    n = poses.shape[0]
    cor = np.zeros((n, 3))
    cor[:, 0] = poses[:, 6]
    args = (n, np.array(shape), np.ones(3), np.array(det), np.array([det_dx, 1.0]))
    return Geometry(*args, cor_shift=cor, step_size=step), orc.Geo(*args, cor_shift=cor, step_size=step)


def pose_kw(poses):
    return dict(alpha=poses[:, 1].copy(), beta=poses[:, 2].copy(), phi=poses[:, 0].copy(), xyz_shift=poses[:, 3:6].copy())


# ------------------------------------------------------------------------------------------------
# poses and data
# ------------------------------------------------------------------------------------------------
Z_BASES = (-6, -3, 0, 3, 6)


def draw_poses(rng, kind, n, zbase, cor_x=None):
    """n poses of `kind`; the integer parts of their z shifts are zbase or zbase + 1."""
    from tomography_alignment_amd import _lib
    phi = rng.uniform(0.02, np.pi - 0.02, n)
    alpha, beta = np.zeros(n), np.zeros(n)
    xyz = np.zeros((n, 3))
    xyz[:, 0] = rng.uniform(-2, 2, n)
    xyz[:, 2] = zbase + rng.integers(0, 2, n) + (rng.uniform(0.1, 0.9, n) if rng.integers(0, 3) else 0.0)     # one set in three: integer z (tau = 0)
    if kind in ("tilted", "mixed"):
        alpha, beta = np.deg2rad(rng.uniform(-4, 4, n)), np.deg2rad(rng.uniform(-4, 4, n))
        alpha[np.abs(alpha) < 1e-3] = 0.02
        if kind == "mixed":
            h = max(1, n // 2)
            alpha[h:] = 0.0
            beta[h:] = 0.0
    elif kind == "steep":
        alpha[int(rng.integers(0, n))] = np.deg2rad(50.0)
    cor = np.zeros(3)
    cor[0] = rng.uniform(-1, 1) if cor_x is None else cor_x
    return _lib.poses_array(phi, alpha, beta, xyz, cor)


def assert_poses_differ(p, q):
    """Consecutive pose sets: other angles, other integer parts of the z shifts (a stale plan or a stale zc_lo / zc_hi moves whole planes)."""
    assert not np.intersect1d(p[:, 0], q[:, 0]).size
    assert not np.intersect1d(np.floor(p[:, 5]), np.floor(q[:, 5])).size


def draw_band(rng, n, prev, width=8):
    """[lo, hi) in [0, n] at least `width` wide whose ends differ from `prev` by >= 20 planes at one end."""
    for _ in range(10000):
        lo, hi = sorted(int(v) for v in rng.integers(0, n + 1, 2))
        if hi - lo >= width and (prev is None or abs(lo - prev[0]) >= 20 or abs(hi - prev[1]) >= 20):
            return lo, hi
    raise AssertionError("no band of %d planes differs from %s" % (n, prev))


def band_volume(rng, shape, zb, xb):
    """Smooth positive values (the gradient kernels' conditioning, tests/test_gpu_fuzz.py) inside the z band and x range, exact zeros outside."""
    ii, jj, kk = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing="ij")
    fr, ph = rng.uniform(0.05, 0.35, 3), rng.uniform(0, 6.28, 3)
    x = (0.6 + 0.4 * np.cos(fr[0] * ii + ph[0]) * np.cos(fr[1] * jj + ph[1]) * np.cos(fr[2] * kk + ph[2])).astype(np.float32)
    x[:, :, :zb[0]] = 0
    x[:, :, zb[1]:] = 0
    x[:xb[0]] = 0
    x[xb[1]:] = 0
    return x


def band_sino(rng, n, det, db):
    y = rng.standard_normal((n, det[0], det[1])).astype(np.float32)
    y[y == 0] = 1.0
    y[:, :, :db[0]] = 0
    y[:, :, db[1]:] = 0
    return y


def assert_volume_band(x, zb, xb):
    nzx = np.nonzero(x.any(axis=(1, 2)))[0]
    nzz = np.nonzero(x.any(axis=(0, 1)))[0]
    assert nzz.size and nzz[0] == zb[0] and nzz[-1] == zb[1] - 1 and nzx[0] == xb[0] and nzx[-1] == xb[1] - 1


def assert_sino_band(y, db):
    nz = np.nonzero(y.any(axis=(0, 1)))[0]
    assert nz.size and nz[0] == db[0] and nz[-1] == db[1] - 1


def assert_bands_differ(b, prev):
    assert prev is None or abs(b[0] - prev[0]) >= 20 or abs(b[1] - prev[1]) >= 20


# ------------------------------------------------------------------------------------------------
# buffers
# ------------------------------------------------------------------------------------------------
class Pooled(object):
    """The long-lived context's buffers: one per (role, size), kept until the context closes, so later steps meet earlier addresses."""

    def __init__(self, ctx):
        self.ctx, self.pool, self.addr_back = ctx, {}, None

    def get(self, role, host=None, size=None):
        size = int(np.size(host)) if host is not None else int(size)
        b = self.pool.get((role, size))
        if b is None:
            b = self.pool[(role, size)] = self.ctx.empty((size,), np.float32)
        if host is not None:
            b.upload(np.asarray(host, np.float32).ravel())
        return b

    def realloc(self, role, size):
        """Free the role's buffer and allocate it again; records whether the address came back."""
        old = self.pool.pop((role, int(size)), None)
        addr = old.ptr.value if old is not None else None
        if old is not None:
            old.free()
        b = self.pool[(role, int(size))] = self.ctx.empty((int(size),), np.float32)
        self.addr_back = addr is not None and b.ptr.value == addr
        return b


class Fresh(Pooled):
    """A fresh context's buffers: same interface (a role asked for twice within one call is one buffer there as well)."""


# ------------------------------------------------------------------------------------------------
# the operations.  op(be, buf, c) -> {name: numpy array or float}
# ------------------------------------------------------------------------------------------------
def _declined(e):
    if "do not take the tile kernels" not in str(e):
        raise e
    return {"declined": np.ones(1, np.float32)}


def _vol(buf, c):
    """The call's volume on the device; `vol_role`: in a buffer of its own, not the one earlier calls of the same size used."""
    return buf.get(c.a.get("vol_role", "vol"), c.a["vol"])


def op_forward(be, buf, c):
    out = be.forward(c.poses, _vol(buf, c), buf.get("proj", size=c.n * be.n_det))
    return {"proj": out.download()}


def op_adjoint(be, buf, c):
    acc = c.a.get("vol0") is not None
    out = buf.get("bp", c.a["vol0"]) if acc else buf.get("bp", size=be.n_vox)
    be.adjoint(c.poses, buf.get("sino", c.a["sino"]), out, accumulate=acc)
    return {"vol": out.download()}


def op_adjoint_update(be, buf, c):
    gt = buf.get("gt", c.a["gt"]) if c.a.get("gt") is not None else None
    pos = bool(c.a.get("positivity", False))
    res, rec, v = buf.get("sino", c.a["sino"]), buf.get("rec", c.a["rec0"]), buf.get("v", c.a["v"])
    bp = buf.get("bp", size=be.n_vox)
    fused, err = be.adjoint_update(c.poses, res, rec, v, pos, gt)
    if not fused:                                   # the caller's two calls (recon/sirt.py)
        be.adjoint(c.poses, res, bp)
        err = be.update(rec, bp, v, pos, gt)
    out = {"rec": rec.download(), "fused": float(fused)}
    if gt is not None:
        out["err"] = float(err)
    return out


def op_adjoint_xslab(be, buf, c):
    """One pass over the x slabs `cuts` as recon/sirt_mpi.py makes it; `between`: a forward call after the first slab; `vouch_first`: the
    sinogram is the previous back-projection call's, unchanged, and the caller says so on the first slab as well."""
    from tomography_alignment_amd import _lib
    sino, out = buf.get("sino", c.a["sino"]), buf.get("bp", np.zeros(be.n_vox, np.float32))
    vol = buf.get("vol", c.a["vol"]) if c.a.get("between") else None
    proj = buf.get("proj", size=c.n * be.n_det) if c.a.get("between") else None
    cuts = c.a["cuts"]
    try:
        for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            be.adjoint_xslab(c.poses, sino, out, a, b, same_sinogram=(i > 0 or bool(c.a.get("vouch_first"))))
            if i == 0 and c.a.get("between") == "forward":
                be.forward(c.a.get("between_poses", c.poses), vol, proj)
    except _lib.TomoError as e:
        return _declined(e)
    return {"vol": out.download()}


def op_forward_xslab(be, buf, c):
    from tomography_alignment_amd import _lib
    vol, out = buf.get("vol", c.a["vol"]), buf.get("proj", np.zeros(c.n * be.n_det, np.float32))
    cuts = c.a["cuts"]
    try:
        for a, b in zip(cuts[:-1], cuts[1:]):
            be.forward_xslab(c.poses, vol, out, a, b)
    except _lib.TomoError as e:
        return _declined(e)
    return {"proj": out.download()}


def op_residual_adjoint(be, buf, c):
    """A SIRT iteration's middle: the forward stages the poses, the residual pass writes `res` and (where it can) notes its planes, the
    back-projection of `res` follows.  The residual is taken against the host array `ax`, so `res` and its sum depend on host data only.
    `between`: what runs between the residual pass and the back-projection; `adj_poses`: back-project with other poses."""
    from tomography_alignment_amd.backend import HipBackend
    n, a = c.n, c.a
    d_vol = buf.get("vol", a["vol"])
    d_b, d_ax, d_w = buf.get("b", a["b"]), buf.get("ax_host", a["ax"]), (buf.get("w", a["w"]) if a.get("w") is not None else None)
    res, bp, proj = buf.get("res", size=n * be.n_det), buf.get("bp", size=be.n_vox), buf.get("proj", size=n * be.n_det)
    bt = a.get("between")
    d_delta = buf.get("delta", a["delta"]) if a.get("delta") is not None else None
    d_b2 = buf.get("b2", a["b2"]) if a.get("b2") is not None else None
    pg_p, pg_g = (buf.get("pg_p", size=be.n_det), buf.get("pg_g", size=6 * be.n_det)) if bt == "proj_grad" else (None, None)
    bp2 = buf.get("bp2", size=be.n_vox) if bt in ("backproject_voxel", "geom_roundtrip") else None
    proj2 = buf.get("proj2", size=n * be.n_det) if bt == "forward" else None
    if a.get("stage", True):
        be.forward(c.poses, d_vol, proj)
    s = be.residual_scale(d_b, d_ax, d_w, res, n_proj=n if a.get("note", True) else None)
    if bt == "proj_grad":
        be.proj_grad(c.poses[:1], d_vol, pg_p, pg_g)
    elif bt == "cost_grad":
        be.cost_grad(c.poses, d_vol, d_b)
    elif bt == "backproject_voxel":
        be.backproject_voxel(c.poses, d_b, bp2)
    elif bt == "forward":
        be.forward(c.poses, d_vol, proj2)
    elif bt == "fill":
        be.fill(res, 1.0)
    elif bt == "update":
        be.update(res, d_delta, None)
    elif bt == "free_alloc":
        res = buf.realloc("res", n * be.n_det)
        res.upload(a["delta"].ravel())
    elif bt == "residual_plain":
        be.residual_scale(d_b2, d_ax, None, res)
    elif bt == "geom_roundtrip":                    # another pool entry and back; a back-projection there rewrites the plane flags in d_blk
        other = c.but(geo=a["other_geo"])
        be2 = HipBackend(geometries(other)[0], ctx=be.ctx)
        be2.adjoint(c.poses, d_delta if d_delta is not None else d_b, buf.get("bp_other", size=be2.n_vox))
    elif bt is not None:
        raise KeyError(bt)
    be.adjoint(a.get("adj_poses", c.poses), res, bp)
    out = {"res": res.download(), "sumsq": float(s), "vol": bp.download()}
    if a.get("stage", True):
        out["ax"] = proj.download()
    return out


def op_proj_grad(be, buf, c):
    p, g = buf.get("pg_p", size=be.n_det), buf.get("pg_g", size=6 * be.n_det)
    be.proj_grad(c.poses[:1], _vol(buf, c), p, g)
    return {"gproj": p.download(), "grad": g.download()}


def op_proj_grad_pinned(be, buf, c):
    """projection_operators.pinned_call: the first evaluation stages the volume, the second (other pose) reuses the padded copy; the
    option goes back to 0."""
    vol = buf.get("vol", c.a["vol"])
    p0, g0, p1, g1 = (buf.get(r, size=s) for r, s in (("pg_p", be.n_det), ("pg_g", 6 * be.n_det), ("pg_p1", be.n_det), ("pg_g1", 6 * be.n_det)))
    be.proj_grad(c.poses[:1], vol, p0, g0)
    be.ctx.set_option("reuse_staged_volume", 1)
    try:
        be.proj_grad(c.poses[1:2], vol, p1, g1)
    finally:
        be.ctx.set_option("reuse_staged_volume", 0)
    return {"gproj": p0.download(), "grad": g0.download(), "gproj1": p1.download(), "grad1": g1.download()}


def op_proj_grad_reuse(be, buf, c):
    """One evaluation with the caller's vouch: `vol` is the buffer staged by an earlier call of the long-lived context and is unchanged
    (upload False: the pooled buffer is taken as it is; a fresh context uploads -- it has nothing staged)."""
    vol = buf.get("vol", size=c.a["vol"].size) if (c.a.get("keep") and isinstance(buf, Pooled) and not isinstance(buf, Fresh)) else buf.get("vol", c.a["vol"])
    p, g = buf.get("pg_p", size=be.n_det), buf.get("pg_g", size=6 * be.n_det)
    be.ctx.set_option("reuse_staged_volume", 1)
    try:
        be.proj_grad(c.poses[:1], vol, p, g)
    finally:
        be.ctx.set_option("reuse_staged_volume", 0)
    return {"gproj": p.download(), "grad": g.download()}


def op_cost_grad(be, buf, c):
    cost, g6 = be.cost_grad(c.poses, _vol(buf, c), buf.get("btab", c.a["b"]), rows=c.a.get("rows"))
    return {"cost": cost, "g6": g6}


def op_backproject_voxel(be, buf, c):
    out = be.backproject_voxel(c.poses, buf.get("sino", c.a["sino"]), buf.get("bp", size=be.n_vox))
    return {"bpv": out.download()}


OPS = {"forward": op_forward, "adjoint": op_adjoint, "adjoint_update": op_adjoint_update, "adjoint_xslab": op_adjoint_xslab,
       "forward_xslab": op_forward_xslab, "residual_adjoint": op_residual_adjoint, "proj_grad": op_proj_grad,
       "proj_grad_pinned": op_proj_grad_pinned, "proj_grad_reuse": op_proj_grad_reuse, "cost_grad": op_cost_grad,
       "backproject_voxel": op_backproject_voxel}


# ------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def takes_gather_forward(c):
    """forward_tiles: a whole-volume call ALL of whose poses are gather-eligible with three samples per row (step 1 here) under the
    default options of the three switches.  Detector x pitch 1.3 keeps ea = (|cos| + |sin|) / 1.3 < 1.45; pitch 0.5 does not."""
    o = c.opts
    return (c.kind in ("gather", "pitch13") and c.geo[1] == 1.0 and o["fwd_variant"] == 3 and o["tile_flat"] and o["adj_flat_gather"] and
            o["fwd_flat_gather"])


def fwd_exact(c, prof, whole=True):
    """No float atomic on the forward path: ray-driven kernels, or the gather forward (its one pair of atomics per value meets a zero:
    0 + a + b, either order the same bits)."""
    return prof["k_fwd_tile"] == 0 and (prof["k_fwd_tile_flat"] == 0 or (whole and takes_gather_forward(c)))


def adj_exact(prof):
    """No float atomic on the adjoint path: the gather adjoint only (k_adj_tile_flat / k_adj_tile flush shared faces, k_adj_v1 scatters)."""
    return prof["k_adj_tile_flat"] == 0 and prof["k_adj_tile"] == 0 and prof["k_adj_v1"] == 0


def exactness(c, prof):
    """name of an output -> compared bit for bit?"""
    fe, ae = fwd_exact(c, prof, whole=c.op != "forward_xslab"), adj_exact(prof)
    return {"proj": fe, "ax": fe, "vol": ae, "rec": ae, "res": True, "gproj": True, "grad": True, "gproj1": True, "grad1": True,
            "cost": True, "g6": True, "bpv": True, "declined": True, "fused": True}


def compare(c, got, want, prof, where):
    """Long-lived (`got`) against fresh (`want`).  -> {output: (mode, figure)} for printing."""
    assert sorted(got) == sorted(want), (where, sorted(got), sorted(want))
    ex = exactness(c, prof)
    seen = {}
    for k in sorted(got):
        a, b = got[k], want[k]
        if k == "sumsq":
            d = abs(a - b) / max(abs(b), 1e-300)
            assert a == b or d <= TOL_DOUBLE_SUM, (where, k, a, b)
            seen[k] = ("1e-12", d)
        elif k == "err":
            if ex["rec"]:
                d = abs(a - b) / max(abs(b), 1e-300)
                assert a == b or d <= TOL_DOUBLE_SUM, (where, k, a, b)
                seen[k] = ("1e-12", d)
            else:
                # err = sum (gt - rec)^2 and the two rec agree to 5e-6 max|rec|: |d err| <= 2 * (5e-6 max|rec|) * sum |gt - rec| (+ second order)
                rec, gt = want["rec"].astype(np.float64), c.a["gt"].ravel().astype(np.float64)
                bound = 2.0 * TOL_FAMILY * np.max(np.abs(rec)) * np.sum(np.abs(gt - rec)) * (1.0 + TOL_FAMILY)
                assert abs(a - b) <= bound, (where, k, a, b, bound)
                seen[k] = ("bound", abs(a - b) / max(bound, 1e-300))
        elif k in ("cost", "g6", "fused"):
            assert np.array_equal(np.asarray(a), np.asarray(b)), (where, k, a, b)
            seen[k] = ("bits", 0.0)
        elif ex[k]:
            same = np.array_equal(bits(a), bits(b))
            assert same, (where, k, "bit for bit", rel_max(a, b) if np.any(b) else float(np.max(np.abs(a))))
            seen[k] = ("bits", 0.0)
        else:
            if np.any(b):
                d = rel_max(a, b)
                assert d <= TOL_FAMILY, (where, k, d)
            else:
                d = 0.0
                assert not np.any(a), (where, k, "fresh context gives zeros")
            seen[k] = ("5e-6", d)
    return seen


def _against(where, k, got, ref, seen):
    if np.any(ref):
        d = rel_max(got, ref)
        assert d <= TOL_ORACLE, (where, k, "oracle", d)
    else:
        d = 0.0
        assert not np.any(got), (where, k, "oracle gives zeros")
    seen[k] = d


def _grad_against(where, tag, og, x, pose, p, g, seen):
    """tests/test_gpu_fuzz.py: the value on every ray, the gradient on the rays whose samples keep 2e-5 voxel from a cell face."""
    from oracle import oracle as orc
    cor3 = np.array([pose[6], 0.0, 0.0])
    want_p, want_g = orc.projection_gradient(og, x, pose[1], pose[2], pose[0], pose[3:6], cor3, precision=np.float64)
    _against(where, "gproj" + tag, p, want_p, seen)
    if np.any(want_g):
        well = orc.ray_face_distance(og, pose[1], pose[2], pose[0], pose[3:6], cor3) >= 2e-5
        g = g.reshape(6, -1).astype(np.float64)
        gmax = [max(np.max(np.abs(want_g[:3])), 1e-30)] * 3 + [max(np.max(np.abs(want_g[3:])), 1e-30)] * 3
        e = max(float(np.max(np.abs(g[r] - want_g[r])[well], initial=0.0)) / gmax[r] for r in range(6))
        assert e <= TOL_ORACLE, (where, "grad" + tag, "oracle", e)
        seen["grad" + tag] = e


def oracle_check(c, got, where):
    """The long-lived context's result against oracle/oracle.py in float64.  -> {output: rel_max}."""
    from oracle import oracle as orc
    seen = {}
    if "declined" in got:
        return seen
    _, og = geometries(c)
    kw = pose_kw(c.poses)
    a = c.a
    if c.op in ("forward", "forward_xslab"):
        _against(where, "proj", got["proj"], orc.forward(og, a["vol"], **kw).ravel(), seen)
    elif c.op in ("adjoint", "adjoint_xslab"):
        ref = orc.adjoint(og, a["sino"], **kw)
        if a.get("vol0") is not None:
            ref = ref + a["vol0"].ravel().astype(np.float64)
        _against(where, "vol", got["vol"], ref, seen)
    elif c.op == "adjoint_update":
        ref = a["rec0"].ravel().astype(np.float64) + a["v"].ravel().astype(np.float64) * orc.adjoint(og, a["sino"], **kw)
        if a.get("positivity"):
            ref = np.maximum(ref, 0.0)
        _against(where, "rec", got["rec"], ref, seen)
        if a.get("gt") is not None:
            want = float(np.sum((a["gt"].ravel().astype(np.float64) - ref) ** 2))
            d = abs(got["err"] - want) / max(want, 1e-300)
            assert d <= TOL_ORACLE, (where, "err", "oracle", d)
            seen["err"] = d
    elif c.op == "residual_adjoint":
        if "ax" in got:
            _against(where, "ax", got["ax"], orc.forward(og, a["vol"], **kw).ravel(), seen)
        adj_poses = a.get("adj_poses", c.poses)
        _, og2 = geometries(c, adj_poses)
        _against(where, "vol", got["vol"], orc.adjoint(og2, got["res"], **pose_kw(adj_poses)), seen)       # of the sinogram the device holds
        if a.get("between") is None:
            r = a["b"].ravel().astype(np.float32) - a["ax"].ravel().astype(np.float32)
            want = r * a["w"].ravel() if a.get("w") is not None else r
            assert np.array_equal(bits(got["res"]), bits(want)), (where, "res", "numpy float32")
            s = float(np.sum(r.astype(np.float64) ** 2))
            assert abs(got["sumsq"] - s) <= TOL_DOUBLE_SUM * s, (where, "sumsq", got["sumsq"], s)
    elif c.op in ("proj_grad", "proj_grad_reuse"):
        _grad_against(where, "", og, a["vol"], c.poses[0], got["gproj"], got["grad"], seen)
    elif c.op == "proj_grad_pinned":
        _grad_against(where, "", og, a["vol"], c.poses[0], got["gproj"], got["grad"], seen)
        _grad_against(where, "1", og, a["vol"], c.poses[1], got["gproj1"], got["grad1"], seen)
    elif c.op == "cost_grad":
        p = orc.forward(og, a["vol"], **kw)
        rows = a.get("rows")
        b = a["b"].reshape(-1, og.n_det).astype(np.float64)
        b = b[np.asarray(rows)] if rows is not None else b[:c.n]
        want = 0.5 * np.sum((b - p) ** 2, axis=1)
        d = float(np.max(np.abs(got["cost"] - want) / np.maximum(want, 1e-300)))
        assert d <= TOL_ORACLE, (where, "cost", "oracle", d)
        seen["cost"] = d
    return seen


# ------------------------------------------------------------------------------------------------
# the runner
# ------------------------------------------------------------------------------------------------
class Runner(object):
    def __init__(self):
        from tomography_alignment_amd import _lib
        self.ctx = _lib.Context()
        self.buf = Pooled(self.ctx)
        self.ctx.profile_enable(True)
        self.prof = {}
        self.log = []

    def close(self):
        self.ctx.close()

    def backend(self, c):
        from tomography_alignment_amd.backend import HipBackend
        return HipBackend(geometries(c)[0], ctx=self.ctx)

    def long_only(self, c):
        """The call on the long-lived context alone (a step that only sets state up) -> (outputs, profile counts)."""
        be = self.backend(c)
        for k, v in sorted(c.opts.items()):
            self.ctx.set_option(k, v)
        self.ctx.profile_reset()
        got = OPS[c.op](be, self.buf, c)
        self.prof = {k: self.ctx.profile_get(k)[0] for k in NAMES}
        return got, self.prof

    @staticmethod
    def fresh(c):
        from tomography_alignment_amd import _lib
        from tomography_alignment_amd.backend import HipBackend
        ctx = _lib.Context()
        try:
            be = HipBackend(geometries(c)[0], ctx=ctx)
            for k, v in sorted(c.opts.items()):
                ctx.set_option(k, v)
            return OPS[c.op](be, Fresh(ctx), c)
        finally:
            ctx.close()

    def run(self, c, where, oracle=True):
        """-> (outputs of the long-lived context, its profile counts); asserts against a fresh context and, with `oracle`, the oracle."""
        got, prof = self.long_only(c)
        seen = compare(c, got, self.fresh(c), prof, where)
        orc_seen = oracle_check(c, got, where) if oracle else {}
        self.log.append((where, c.op, c.kind, c.geo, seen, orc_seen))
        print("%s: %s %s %s n=%d | vs fresh: %s%s | kernels: %s" % (
            where, c.op, c.kind, c.geo, c.n, ", ".join("%s %s %.1e" % (k, m, d) for k, (m, d) in sorted(seen.items())),
            (" | vs oracle: " + ", ".join("%s %.1e" % kv for kv in sorted(orc_seen.items()))) if orc_seen else "",
            " ".join("%s:%d" % (k, v) for k, v in sorted(prof.items()) if v)))
        return got, prof


# ------------------------------------------------------------------------------------------------
# building a call
# ------------------------------------------------------------------------------------------------
SEQ_OPS = ("forward", "adjoint", "adjoint_acc", "adjoint_update", "adjoint_update_gt", "adjoint_xslab", "forward_xslab", "residual_adjoint",
           "residual_between", "proj_grad", "cost_grad", "cost_grad_rows", "backproject_voxel", "proj_grad_pinned", "repeat")
BETWEEN = ("proj_grad", "cost_grad", "backproject_voxel", "forward")


def n_xtiles(shape):
    return (shape[0] + 1 + ATX - 1) // ATX


def make_call(rng, op, entry="a150", kind="gather", n=5, step=1.0, zbase=0, zb=None, xb=None, db=None, opts=None, poses=None, **extra):
    """A call of `op` (a name of SEQ_OPS or OPS) with banded data drawn from rng.  zb / xb: z band and x range of the volume, db: band of
    detector planes of the sinograms (drawn when None)."""
    shape, det = POOL[entry]
    zb = draw_band(rng, shape[2], None) if zb is None else zb
    xb = draw_band(rng, shape[0], None, width=3) if xb is None else xb
    db = draw_band(rng, det[1], None) if db is None else db
    poses = draw_poses(rng, kind, n, zbase) if poses is None else poses
    n = poses.shape[0]
    vol, sino = band_volume(rng, shape, zb, xb), band_sino(rng, n, det, db)
    assert_volume_band(vol, zb, xb)
    assert_sino_band(sino, db)
    a = {"vol": vol, "sino": sino, "zb": zb, "xb": xb, "db": db, "zbase": zbase}
    name = op
    if op == "adjoint_acc":
        name, a["vol0"] = "adjoint", band_volume(rng, shape, zb, xb)
    elif op in ("adjoint_update", "adjoint_update_gt"):
        name = "adjoint_update"
        a["rec0"], a["v"] = rng.uniform(-1, 1, shape).astype(np.float32), rng.uniform(0.1, 1.0, shape).astype(np.float32)
        a["positivity"] = bool(rng.integers(0, 2))
        if op.endswith("_gt"):
            a["gt"], a["positivity"] = rng.uniform(0, 1, shape).astype(np.float32), True
    elif op in ("adjoint_xslab", "forward_xslab"):
        nxt = n_xtiles(shape)
        a["cuts"] = sorted(set([0, nxt] + [int(v) for v in rng.integers(0, nxt + 1, 2)]))
    elif op in ("residual_adjoint", "residual_between"):
        name = "residual_adjoint"
        a["b"], a["ax"] = sino, band_sino(rng, n, det, db)
        a["w"] = (np.abs(band_sino(rng, n, det, (0, det[1]))) + 0.5) if rng.integers(0, 2) else None
        if op == "residual_between":
            a["between"] = BETWEEN[int(rng.integers(0, len(BETWEEN)))]
    elif op in ("cost_grad", "cost_grad_rows"):
        name = "cost_grad"
        if op == "cost_grad_rows":
            a["b"] = band_sino(rng, n + 2, det, db)
            a["rows"] = rng.integers(0, n + 2, n).astype(np.int32)
        else:
            a["b"] = sino
    elif op == "proj_grad_pinned" and n < 2:
        poses = np.concatenate([poses, draw_poses(rng, "gather" if kind == "steep" else kind, 1, zbase)])
    a.update(extra)
    return Call(name, geo_of(entry, step, DET_DX.get(kind, 1.0)), poses, opts, kind, **a)
