"""One long-lived context against fresh ones, over the host state a tomo_ctx keeps between calls: the staged pose constants
(TilePlan, stage_tile_consts), the sinogram plane flags in d_blk (ZfKey, zf_has_cum, zf_has_shift), the note of the residual pass
(zf_recorded), the zero-padded volume (d_volpad, staged_src, halo_dirty, option reuse_staged_volume), the geometry key of
_lib.Context, and the grow-only buffers (d_stage, d_blk, d_red, d_red_part, d_volpad).  A wrong key or a missing drop is silent: the
kernels run correctly on the previous call's poses, flags or volume.  The other GPU tests open a context per case and cannot see it.

Every call of the long-lived context is repeated on a fresh context (same options set explicitly, same host inputs uploaded anew, that
call only) and compared (tests/ctx_state_cases.py: compare):

    path of the call (profile names of the long-lived context)                       compared
    gather forward (k_fwd_gather_flat; its pair of atomics per value meets a zero)   bit for bit
    ray-driven forwards k_fwd_v1 / k_fwd_v2 (plain stores)                           bit for bit
    gather adjoint k_adj_gather_flat, tomo_adjoint_update fused (plain stores)       bit for bit
    tomo_proj_grad (per ray), tomo_cost_grad* (partial sums added in a fixed order)  bit for bit
    k_bp_voxel (voxel gather), k_residual_scale / k_update outputs (element-wise)    bit for bit
    flat forwards k_fwd_flat_tab / k_tile_flat<true>, general k_tile<true>           rel_max <= 5e-6 (float atomics into the sinogram)
    k_adj_tile_flat, k_adj_tile (faces shared by tiles flushed with float atomics)   rel_max <= 5e-6
    k_adj_v1 (float atomics per sample)                                              rel_max <= 5e-6
    residual sum, error sum of a bit-exact update (one double atomic per group)      1e-12 relative
    error sum of an update whose back-projection is in a 5e-6 row                    2 * 5e-6 max|rec| * sum|gt - rec| (first-order bound)

On every fifth step of the sequences and on every step of the directed tests the long-lived result also goes against oracle/oracle.py in
float64 (forward, adjoint, projection_gradient) at the suite's 1e-5, so two wrong runs that agree do not pass.

Geometry pool (ctx_state_cases.POOL; the relations are asserted from the numbers in test_pool_relations):

    a150   (20, 27, 150) / (36, 128)   three 64-plane chunks; ndz divides the vector grid: the note is taken
    b150   (27, 20, 150) / (36, 128)   same padded size and nx * ny as a150: d_volpad is kept; same ndz, ndx, nz: a ZfKey that survived would match
    a150z  (20, 27, 150) / (36, 150)   ndz = 150: the note is not taken, the scan runs
    small  (12, 9, 70) / (16, 80)      every buffer shrinks in use.  FTZ = 63 makes 70 planes TWO flat z tiles, not one: k_tile_flat<true> runs
                                       here under fwd_flat_ztiles 1 only
    onez   (12, 9, 60) / (16, 64)      ... so this entry has the one z tile (k_tile_flat<true> under any option)
    large  (40, 33, 200) / (48, 256)   every buffer grows; three x tile columns

each with step_size 1 and 0.5.  Pose kinds: gather (untilted, unit lattice), pitch13 (detector x pitch 1.3: by stage_tile_consts still
gather-eligible, ea = (|cos| + |sin|) / 1.3 < 1.45, on a non-unit lattice), pitch05 (detector x pitch 0.5: ea >= 2, the flat kernels that
are not gather-eligible), tilted (up to 4 degrees: general), mixed (general + flat in one call), steep (one pose at 50 degrees: the call
is declined by the tile kernels).  (A detector z pitch other than 1 makes a pose general; tests/test_gpu_pitch.py.)

Directed tests: one per key field and per drop; each asserts from the profile that the cache was in play where the profile can show it.

Teeth, checked once on three one-line mutations of the host code (each keeps every size and count and changes only which values are read):
TOMO_LAUNCH no longer clears zf_recorded -- test_a_write_in_between_drops_the_note[fill, update, residual_plain, cost_grad] fail;
stage_tile_consts without the memcmp of the poses -- test_plan_same_n_other_poses (all three), test_plan_geometry_changes_that_keep_every_shape
(both), test_plan_declined_set_then_the_accepted_one, three of the test_flags_* tests, test_note_taken_under_one_pose_set_serves_no_other and
test_grow_only_buffers_large_small_large[gather, mixed] fail; adjoint_atomic without halo_dirty = true --
test_staged_volume_after_the_atomic_adjoint_dirtied_the_halo and test_grow_only_buffers_large_small_large[steep] fail.  All by assertion.  The
seeded sequences caught none of the three: their banded data keeps away from the faces of the volume and their consecutive steps rarely share a
geometry, a pose count and the options -- the directed tests are what pins the keys, the sequences what pins the buffers and the mixture."""
import numpy as np
import pytest

import ctx_state_cases as C
from ctx_state_cases import Runner, make_call

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, 2)
N_STEPS = 40
_SEQ = {}


@pytest.fixture
def R():
    r = Runner()
    yield r
    r.close()


def test_pool_relations():
    C.check_pool_relations()
    print("pool relations hold: padded sizes", {k: (v[0][0] + 4) * (v[0][1] + 4) * (v[0][2] + 4) for k, v in C.POOL.items()})


# ------------------------------------------------------------------------------------------------
# seeded sequences
# ------------------------------------------------------------------------------------------------
def _cycle(rng, items, n):
    out = []
    while len(out) < n:
        out += [items[i] for i in rng.permutation(len(items))]
    return out[:n]


def _sequence(seed):
    """Runs the sequence of `seed` once per process -> (pair counts, kernel counts, notes taken)."""
    if seed in _SEQ:
        if isinstance(_SEQ[seed], BaseException):
            raise _SEQ[seed]                       # failed already: test_sequences_reach_every_path does not run it again
        return _SEQ[seed]
    # every (operation, pose kind) pair runs once over the three seeds together (30 of the 90 each), then ten more pairs per seed
    sched = np.random.default_rng(4199).permutation(len(C.SEQ_OPS) * len(C.POSE_KINDS))
    rng = np.random.default_rng(4200 + seed)
    mine = list(sched[30 * SEEDS.index(seed):30 * SEEDS.index(seed) + 30]) + list(rng.integers(0, sched.size, N_STEPS - 30))
    mine = [mine[i] for i in rng.permutation(N_STEPS)]
    ops, kinds = [C.SEQ_OPS[k // len(C.POSE_KINDS)] for k in mine], [C.POSE_KINDS[k % len(C.POSE_KINDS)] for k in mine]
    entries = _cycle(rng, sorted(C.POOL), N_STEPS)
    if ops[0] == "repeat":
        j = [o != "repeat" for o in ops].index(True)
        ops[0], ops[j] = ops[j], ops[0]
    pairs, kernels, notes = {}, {k: 0 for k in C.NAMES + ("gather forward (of k_fwd_tile_flat)",)}, 0
    prev = None
    R = Runner()
    try:
        for i in range(N_STEPS):
            where = "seed %d step %d" % (seed, i)
            if ops[i] == "repeat":
                c, op_name = prev, "repeat"
            else:
                shape, det = C.POOL[entries[i]]
                zbase = int(rng.choice([z for z in C.Z_BASES if prev is None or z != prev.a["zbase"]]))
                n = int(rng.integers(2 if kinds[i] == "mixed" else 1, 8))
                opts = {k: int(rng.choice(v)) for k, v in sorted(C.OPTION_SPACE.items())}
                # the options and the step a solver runs with: every other step, and three in four of the gather-eligible pose kinds, whose
                # paths keep the most state (the gather forward's plane flags, the note)
                likely = 0.75 if kinds[i] in ("gather", "pitch13") else 0.5
                if rng.uniform() < likely:
                    opts = dict(C.DEFAULTS)
                step = 1.0 if rng.uniform() < likely else 0.5
                zb = C.draw_band(rng, shape[2], prev.a["zb"] if prev is not None else None)
                db = C.draw_band(rng, det[1], prev.a["db"] if prev is not None else None)
                c = make_call(rng, ops[i], entry=entries[i], kind=kinds[i], n=n, step=step, zbase=zbase, zb=zb, db=db,
                              opts=opts)
                op_name = ops[i]
                if prev is not None:             # conditions of the test, on the host arrays
                    C.assert_poses_differ(c.poses, prev.poses)
                    C.assert_bands_differ(c.a["zb"], prev.a["zb"])
                    C.assert_bands_differ(c.a["db"], prev.a["db"])
            _, prof = R.run(c, where, oracle=(i % 5 == 0))
            pairs[(c.kind, op_name)] = pairs.get((c.kind, op_name), 0) + 1
            for k in C.NAMES:
                kernels[k] += prof[k]
            if c.op == "residual_adjoint" and prof["k_adj_gather_flat"] and not prof["k_sino_zflags"]:
                notes += 1
            if c.op in ("forward", "residual_adjoint") and prof["k_fwd_tile_flat"] and C.takes_gather_forward(c):
                kernels["gather forward (of k_fwd_tile_flat)"] += 1
            prev = c
    except BaseException as e:
        _SEQ[seed] = e
        raise
    finally:
        R.close()
    _SEQ[seed] = (pairs, kernels, notes)
    return _SEQ[seed]


@pytest.mark.parametrize("seed", SEEDS)
def test_sequence_matches_fresh_contexts(seed):
    pairs, kernels, notes = _sequence(seed)
    print("seed %d: (pose kind, operation) counts: %s" % (seed, ", ".join("%s/%s %d" % (k[0], k[1], v) for k, v in sorted(pairs.items()))))
    print("seed %d: kernel launches: %s; back-projections that took the note: %d" % (seed, ", ".join("%s %d" % kv for kv in sorted(kernels.items())), notes))
    assert sum(pairs.values()) == N_STEPS


def test_sequences_reach_every_path():
    total, notes = {}, 0
    for seed in SEEDS:
        _, kernels, n = _sequence(seed)
        notes += n
        for k in kernels:
            total[k] = total.get(k, 0) + kernels[k]
    print("all seeds: kernel launches: %s; notes taken: %d" % (", ".join("%s %d" % kv for kv in sorted(total.items())), notes))
    missing = [k for k in C.REQUIRED if total[k] == 0]
    assert not missing, missing
    assert notes > 0 and total["gather forward (of k_fwd_tile_flat)"] > 0


# ------------------------------------------------------------------------------------------------
# directed: TilePlan
# ------------------------------------------------------------------------------------------------
def _rng(tag):
    return np.random.default_rng([77, tag])


@pytest.mark.parametrize("kind", ["gather", "tilted", "pitch05"])
def test_plan_same_n_other_poses(R, kind):
    rng = _rng(1)
    for op in ("adjoint", "forward"):
        c1 = make_call(rng, op, kind=kind, n=4, zbase=0)
        c2 = c1.but(poses=C.draw_poses(rng, kind, 4, 3))
        C.assert_poses_differ(c1.poses, c2.poses)
        R.run(c1, "plan/poses %s first" % op)
        R.run(c1, "plan/poses %s again (plan kept)" % op)
        got2, _ = R.run(c2, "plan/poses %s other poses" % op)
        key = "vol" if op == "adjoint" else "proj"
        got1, _ = R.long_only(c1)
        assert C.rel_max(got2[key], got1[key]) > 1e-2          # the two pose sets are far apart: a stale plan could not hide in a tolerance


def test_plan_option_changes(R):
    rng = _rng(2)
    c = make_call(rng, "adjoint", kind="gather", n=4)
    _, p = R.run(c, "plan/opts default")
    assert p["k_adj_gather_flat"] and not p["k_adj_tile_flat"] and not p["k_adj_tile"]
    _, p = R.run(c.but(opts={"adj_flat_gather": 0}), "plan/opts adj_flat_gather 0")
    assert p["k_adj_tile_flat"] and not p["k_adj_gather_flat"]
    _, p = R.run(c, "plan/opts default again")
    assert p["k_adj_gather_flat"] and not p["k_adj_tile_flat"]
    _, p = R.run(c.but(opts={"tile_flat": 0}), "plan/opts tile_flat 0")
    assert p["k_adj_tile"] and not p["k_adj_gather_flat"] and not p["k_adj_tile_flat"]
    f = c.but(op="forward")
    _, p = R.run(f, "plan/opts forward default")
    assert p["k_fwd_tile_flat"] and not p["k_fwd_tile"]
    _, p = R.run(f.but(opts={"tile_flat": 0}), "plan/opts forward tile_flat 0")
    assert p["k_fwd_tile"] and not p["k_fwd_tile_flat"]


@pytest.mark.parametrize("kind", ["gather", "tilted"])
def test_plan_geometry_changes_that_keep_every_shape(R, kind):
    rng = _rng(3)
    c = make_call(rng, "adjoint", kind=kind, n=4)
    g1, _ = R.run(c, "plan/geometry step 1")
    half = c.but(geo=C.geo_of("a150", 0.5))
    g2, _ = R.run(half, "plan/geometry step 0.5, same poses")
    assert C.rel_max(g2["vol"], g1["vol"]) > 0.3               # twice the samples
    R.run(c, "plan/geometry step 1 again")
    p = c.poses.copy()
    p[:, 6] += 2.25
    g3, _ = R.run(c.but(poses=p), "plan/geometry cor_shift + 2.25, same angles and shifts")
    assert C.rel_max(g3["vol"], g1["vol"]) > 1e-2
    f = c.but(op="forward")
    R.run(f, "plan/geometry forward")
    R.run(f.but(geo=C.geo_of("a150", 0.5)), "plan/geometry forward step 0.5")
    R.run(f.but(poses=p), "plan/geometry forward cor_shift")


@pytest.mark.parametrize("user", ["proj_grad", "cost_grad", "backproject_voxel"])
def test_plan_after_another_user_of_the_staging_buffer(R, user):
    rng = _rng(4)
    c = make_call(rng, "adjoint", kind="mixed", n=5)
    R.run(c, "plan/stage adjoint")
    R.run(make_call(rng, user, kind="tilted", n=5, zbase=3), "plan/stage %s in between" % user)
    R.run(c, "plan/stage adjoint, same poses")
    R.run(c.but(op="forward"), "plan/stage forward, same poses")
    R.run(make_call(rng, user, kind="gather", n=5, zbase=-3), "plan/stage %s in between" % user)
    R.run(c.but(op="forward"), "plan/stage forward, same poses again")


def test_plan_declined_set_then_the_accepted_one(R):
    rng = _rng(5)
    ok = make_call(rng, "adjoint", kind="gather", n=4)
    steep = ok.but(poses=C.draw_poses(rng, "steep", 4, 3), kind="steep")
    for op in ("adjoint", "forward"):
        _, p = R.run(ok.but(op=op), "plan/declined accepted %s" % op)
        assert p["k_adj_gather_flat"] or p["k_fwd_tile_flat"]
        _, p = R.run(steep.but(op=op), "plan/declined steep %s" % op)
        assert p["k_adj_v1"] or p["k_fwd_v2"]
        _, p = R.run(ok.but(op=op), "plan/declined accepted %s again" % op)
        assert p["k_adj_gather_flat"] or p["k_fwd_tile_flat"]


# ------------------------------------------------------------------------------------------------
# directed: ZfKey.  Launches profiled as k_sino_zflags: gather poses only -- the scan + the chunk shift = 2 per scan, 0 when cached;
# general poses only -- scan + prefix counts + live tiles + compaction = 4 per scan, 2 when cached
# ------------------------------------------------------------------------------------------------
def test_flags_two_geometries_of_equal_key_shape_back_to_back(R):
    rng = _rng(10)
    c1 = make_call(rng, "adjoint_xslab", entry="a150", kind="gather", n=4, db=(5, 40), cuts=[0, 1, 2])
    c2 = make_call(rng, "adjoint_xslab", entry="b150", kind="gather", n=4, db=(70, 120), cuts=[0, 1, 2], poses=c1.poses)
    assert c1.a["sino"].size == c2.a["sino"].size
    _, p = R.run(c1, "flags/geometries a150")
    assert p["k_sino_zflags"] == 2
    R.buf.realloc("sino", c1.a["sino"].size)
    print("flags/geometries: the freed sinogram's address came back: %s" % R.buf.addr_back)
    _, p = R.run(c2, "flags/geometries b150, other sinogram")
    assert p["k_sino_zflags"] == 2


def test_flags_same_pointer_new_contents(R):
    rng = _rng(11)
    c1 = make_call(rng, "adjoint", kind="gather", n=4, db=(5, 40))
    c2 = c1.but(sino=C.band_sino(rng, 4, c1.det, (70, 120)))
    g1, p = R.run(c1, "flags/contents first")
    assert p["k_sino_zflags"] == 2
    g2, p = R.run(c2, "flags/contents same pointer, other band")
    assert p["k_sino_zflags"] == 2
    z1, z2 = (np.nonzero(g["vol"].reshape(c1.shape).any(axis=(0, 1)))[0] for g in (g1, g2))
    assert z1.max() < z2.min()                                      # whole planes moved


def test_flags_forward_between_two_slabs(R):
    rng = _rng(12)
    c = make_call(rng, "adjoint_xslab", kind="gather", n=4, cuts=[0, 1, 2])
    _, p = R.run(c, "flags/slabs one pass")
    assert p["k_sino_zflags"] == 2                                  # the second slab took the first slab's flags: the cache is in play
    _, p = R.run(c.but(between="forward"), "flags/slabs forward in between")
    assert p["k_sino_zflags"] == 4 and p["k_fwd_tile_flat"]         # ... and is dropped by the live lists
    _, p = R.run(c.but(between="forward", opts={"fwd_flat_gather": 0}), "flags/slabs flat forward in between")
    assert p["k_sino_zflags"] == 4 and p["k_fwd_live"]
    t = make_call(rng, "adjoint_xslab", kind="tilted", n=4, cuts=[0, 1, 2])
    _, p = R.run(t, "flags/slabs tilted one pass")
    assert p["k_sino_zflags"] == 4 + 2
    _, p = R.run(t.but(between="forward"), "flags/slabs tilted, forward in between")
    assert p["k_sino_zflags"] == 4 + 4 and p["k_fwd_tile"]


def test_flags_later_slab_needs_a_larger_block_buffer(R):
    rng = _rng(13)
    c = make_call(rng, "adjoint_xslab", entry="large", kind="tilted", n=4, cuts=[0, 1, 3])
    _, p = R.run(c, "flags/grow one column, then two")
    assert p["k_sino_zflags"] == 4 + 4                              # d_blk grew for the second slab's tile list: its flags went with it
    _, p = R.run(c, "flags/grow again, nothing grows")
    assert p["k_sino_zflags"] == 4 + 2


def test_flags_other_z_offsets_on_an_unchanged_sinogram(R):
    rng = _rng(14)
    c1 = make_call(rng, "adjoint_xslab", kind="gather", n=4, zbase=-6, cuts=[0, 2])
    c2 = c1.but(poses=C.draw_poses(rng, "gather", 4, 6), vouch_first=True)
    C.assert_poses_differ(c1.poses, c2.poses)
    R.run(c1, "flags/zc first pass")
    _, p = R.run(c1.but(vouch_first=True), "flags/zc same poses, sinogram vouched for")
    assert p["k_sino_zflags"] == 0                                  # the cache is in play
    _, p = R.run(c2, "flags/zc other z offsets, sinogram vouched for")
    assert p["k_sino_zflags"] == 2


def test_flags_prefix_counts_and_chunk_shift_wanted_later(R):
    rng = _rng(15)
    g = make_call(rng, "adjoint_xslab", kind="gather", n=4, zbase=0, cuts=[0, 2])
    g.poses[:2, 5], g.poses[2:, 5] = 0.25, 1.5                       # z offsets 0 and 1 among the first two and the last two
    m = g.poses.copy()
    m[1, 1], m[3, 2] = np.deg2rad(3.0), np.deg2rad(-2.0)             # poses 1 and 3 tilted: general; 0 and 2 keep the offsets 0 and 1
    _, p = R.run(g, "flags/cum gather pass (no prefix counts)")
    assert p["k_sino_zflags"] == 2
    _, p = R.run(g.but(poses=m, vouch_first=True, kind="mixed"), "flags/cum mixed pass wants prefix counts")
    assert p["k_sino_zflags"] == 3 + 2 and p["k_adj_tile"] and p["k_adj_gather_flat"]
    t = make_call(rng, "adjoint_xslab", kind="tilted", n=4, cuts=[0, 2], sino=g.a["sino"])
    _, p = R.run(t, "flags/shift tilted pass (no chunk shift)")
    assert p["k_sino_zflags"] == 4
    _, p = R.run(g.but(vouch_first=True), "flags/shift gather pass wants the chunk shift")
    assert p["k_sino_zflags"] == 2


# ------------------------------------------------------------------------------------------------
# directed: the note of the residual pass
# ------------------------------------------------------------------------------------------------
def _noted_call(rng, zero):
    c = make_call(rng, "residual_adjoint", kind="gather", n=5, db=(40, 100))
    det = c.det
    c.a["w"] = np.zeros((5, det[0], det[1]), np.float32) if zero else np.ones((5, det[0], det[1]), np.float32)
    delta = np.zeros((5, det[0], det[1]), np.float32)
    delta[:, :, 30] = 1.0                                            # a plane outside the band
    c.a["delta"] = delta
    c.a["b2"] = (c.a["ax"] + delta).astype(np.float32)
    return c


@pytest.mark.parametrize("writer", ["fill", "free_alloc", "update", "residual_plain", "geom_roundtrip", "forward", "cost_grad"])
def test_a_write_in_between_drops_the_note(R, writer):
    """All-zero residual noted (no plane flagged), then the sinogram made non-zero through another entry point.  geom_roundtrip writes
    nothing: there the noted residual is the banded one and a back-projection of another sinogram under the other geometry rewrites the
    flags in d_blk."""
    rng = _rng(20)
    c = _noted_call(rng, zero=writer not in ("geom_roundtrip", "forward", "cost_grad"))
    got, p = R.run(c, "note/%s control" % writer)
    assert p["k_sino_zflags"] == 0 and p["k_adj_gather_flat"]        # the note was taken: it is in play
    got, p = R.run(c.but(between=writer, other_geo=C.geo_of("b150")), "note/%s" % writer)
    assert p["k_sino_zflags"] >= 2
    assert np.count_nonzero(got["vol"]) > 0
    if writer == "free_alloc":
        print("note/free_alloc: the freed sinogram's address came back: %s" % R.buf.addr_back)


def test_note_taken_under_one_pose_set_serves_no_other(R):
    rng = _rng(21)
    c = _noted_call(rng, zero=False)
    _, p = R.run(c, "note/poses control")
    assert p["k_sino_zflags"] == 0
    far = C.draw_poses(rng, "gather", 5, 6)
    C.assert_poses_differ(c.poses, far)
    _, p = R.run(c.but(adj_poses=far), "note/poses other z offsets")
    assert p["k_sino_zflags"] == 2
    turned = c.poses.copy()
    turned[:, 0] = rng.uniform(0.02, 3.1, 5)                         # other angles, the same z shifts: the flags still describe the sinogram
    R.run(c.but(adj_poses=turned), "note/poses other angles")
    tilted = C.draw_poses(rng, "tilted", 5, 0)
    _, p = R.run(c.but(adj_poses=tilted), "note/poses tilted")
    assert p["k_adj_tile"] and p["k_sino_zflags"] == 4


# ------------------------------------------------------------------------------------------------
# directed: the staged volume
# ------------------------------------------------------------------------------------------------
def _border_volume_call(rng, op="proj_grad", entry="a150", **kw):
    shape = C.POOL[entry][0]
    return make_call(rng, op, entry=entry, kind="tilted", n=2, zb=(0, shape[2] - 40), xb=(0, shape[0]), **kw)      # non-zero up to the faces x = 0, y = 0, y = ny - 1, z = 0


def test_staged_volume_reuse_is_in_play(R):
    rng = _rng(30)
    c = _border_volume_call(rng)
    _, p = R.run(c, "staged/control first")
    assert p["k_pad"] == 1
    _, p = R.run(c.but(op="proj_grad_reuse", keep=True, poses=c.poses[1:]), "staged/control reuse")
    assert p["k_pad"] == 0
    _, p = R.run(c.but(op="proj_grad_pinned"), "staged/control pinned pair")
    assert p["k_pad"] == 1 and p["k_proj_grad"] == 2


def test_staged_volume_after_the_atomic_adjoint_dirtied_the_halo(R):
    rng = _rng(31)
    c = _border_volume_call(rng)
    R.run(c, "staged/halo first")
    a = make_call(rng, "adjoint", kind="tilted", n=3, db=(0, 128), opts={"adj_variant": 1})
    _, p = R.run(a, "staged/halo atomic adjoint")
    assert p["k_adj_v1"]
    _, p = R.run(c.but(op="proj_grad_reuse", keep=True), "staged/halo reuse after it")
    assert p["k_pad"] == 1
    _, p = R.run(a, "staged/halo atomic adjoint again")
    _, p = R.run(c.but(op="forward", opts={"fwd_variant": 2}), "staged/halo ray-driven forward after it")
    assert p["k_fwd_v2"] and p["k_pad"] == 1
    _, p = R.run(a, "staged/halo atomic adjoint once more")
    _, p = R.run(c.but(op="cost_grad", b=c.a["sino"]), "staged/halo cost_grad after it")
    assert p["k_pad"] == 1


@pytest.mark.parametrize("other", ["b150", "small"])
def test_staged_volume_after_a_geometry_round_trip(R, other):
    rng = _rng(32)
    c = _border_volume_call(rng)
    R.run(c, "staged/geometry first")
    R.run(_border_volume_call(rng, entry=other, vol_role="vol2"), "staged/geometry %s" % other)      # (b150's volume has a150's size: its own buffer)
    _, p = R.run(c.but(op="proj_grad_reuse", keep=True), "staged/geometry back, reuse")
    assert p["k_pad"] == 1
    R.backend(c.but(geo=C.geo_of(other)))                           # set_geometry alone, nothing run under it
    _, p = R.run(c.but(op="proj_grad_reuse", keep=True), "staged/geometry set and back, reuse")
    assert p["k_pad"] == 1


def test_staged_volume_after_a_ray_driven_forward_of_another_volume(R):
    rng = _rng(33)
    c = _border_volume_call(rng)
    R.run(c, "staged/other first")
    q = make_call(rng, "forward", kind="tilted", n=2, zb=(100, 150), opts={"fwd_variant": 1}, vol_role="vol2")      # in a buffer of its own
    _, p = R.run(q, "staged/other ray-driven forward of another volume")
    assert p["k_fwd_v1"] and p["k_pad"] == 1
    _, p = R.run(c.but(op="proj_grad_reuse", keep=True), "staged/other reuse of the first")
    assert p["k_pad"] == 1


def test_staged_volume_kept_buffer_under_the_transposed_geometry(R):
    rng = _rng(34)
    a = make_call(rng, "forward", entry="a150", kind="steep", n=3, zb=(0, 60), xb=(0, 20))
    b = make_call(rng, "forward", entry="b150", kind="steep", n=3, zb=(90, 150), xb=(5, 27), poses=a.poses)
    _, p = R.run(a, "staged/transposed a150 declined forward")
    assert p["k_fwd_v2"] and p["k_pad"] == 1
    R.run(a.but(op="adjoint"), "staged/transposed a150 atomic adjoint")
    _, p = R.run(b, "staged/transposed b150 declined forward on the kept buffer")
    assert p["k_fwd_v2"] and p["k_pad"] == 1
    _, p = R.run(b.but(op="adjoint"), "staged/transposed b150 atomic adjoint")
    assert p["k_adj_v1"]
    R.run(b.but(op="proj_grad"), "staged/transposed b150 proj_grad")
    R.run(a.but(op="cost_grad", b=a.a["sino"]), "staged/transposed a150 cost_grad")


# ------------------------------------------------------------------------------------------------
# directed: the grow-only buffers
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gather", "mixed", "steep"])
def test_grow_only_buffers_large_small_large(R, kind):
    rng = _rng(40)
    for entry in ("large", "onez", "large", "small", "large"):
        for op in ("forward", "adjoint", "cost_grad"):
            R.run(make_call(rng, op, entry=entry, kind=kind, n=7 if entry == "large" else 2), "grow/%s %s %s" % (kind, entry, op))
