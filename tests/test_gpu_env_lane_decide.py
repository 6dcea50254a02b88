"""The mask-only environment loop with its per-lane classification (env_item_undecided, csrc/kernels_collision.h) against the fp32
oracle, bit for bit: self_mask, env_mask, jlim_mask, ext_cost and the [S, 8] summary of fused launches, the stand-alone collision
kernel on a partly filled wavefront, and min_env of the stage that keeps every test (COLL = 2) on the same inputs.

Robots: Panda (specialised: capsules in registers) and a random 7-joint chain on the generic kernels (capsules in LDS).
Launches: 2 seeds x 64 waypoints (one wavefront per seed, the in-launch summary); K = 1 without clamp (the stage's copy for rows that
may lie outside the limits) and K = 2 with clamp.  One collision_masks call on 100 rows (a full and a partly filled wavefront).
Rows: seed 0 is BUILT so that its wavefront holds, for one (capsule, cuboid) item, lanes of every class -- far, certain hit, within
1 cm of touching (undecided), already hit by an earlier capsule or cuboid -- 16 of each, interleaved; they are picked from a pool of
random configurations with the oracle and start on their own targets, so the LM steps leave them where they are (the classes are
asserted again on the launch's own x_out).  Seed 1 holds independent random configurations, the incoherent case, and one NaN row.
Obstacle sets: one cuboid; the two of panda__2cubes; a plate 8 mm thin with a cuboid large enough to contain capsule centres."""

import functools

import numpy as np
import pytest
import torch

from cppflow_amd import _hip, gen_robots
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
W, S, POOL, PER_CLASS = 64, 2, 30000, 16
LM = dict(lm_lambda=1e-6, alpha_position=3.5, alpha_rotation=0.35)
SETS = {
    "1cube": H.PANDA_1CUBE,
    "2cubes": H.PANDA_2CUBES,
    "thin_and_large": [H.cuboid_obstacle(0.3, 0.0, 0.5, 0.4, 0.008, 0.4), H.cuboid_obstacle(-0.2, 0.3, 0.6, 0.3, 0.3, 0.3)],
}
ROBOTS = ["panda", "generic7"]


@functools.lru_cache(maxsize=None)
def model(name):
    """(chain, fp32 oracle, fp64 oracle) -- the generic robot is tests/helpers.random_chain_spec(7, seed=21)"""
    if name == "panda":
        return H.chain(name), H.oracle32(name), H.oracle64(name)
    from cppflow_amd.robot_model import canonicalize
    from oracle.oracle import Oracle

    ch = canonicalize(H.random_chain_spec(7, seed=21))
    return ch, Oracle(ch, f32=True, threads=8), Oracle(ch, f32=False, threads=8)


@pytest.fixture(scope="module")
def robots():
    from cppflow_amd.robots import Robot, get_robot

    rbs = {"panda": get_robot("panda"), "generic7": Robot(H.random_chain_spec(7, seed=21), specialize=False)}
    assert rbs["panda"].specialization(DEV) >= 0 and rbs["generic7"].specialization(DEV) == -1
    return rbs


def lane_classes(name, q, lo, hi, item):
    """bool [n] per class of the rows q for the item (capsule c, cuboid o), in the order the stage visits items (capsules outermost)"""
    ch, o32, _ = model(name)
    c, o = item
    ep = o32.capsule_endpoints(q)
    centre = 0.5 * (ep[:, c, :3] + ep[:, c, 3:])
    clear = np.stack([o32.env_dists(q, lo[k], hi[k]) for k in range(lo.shape[0])], axis=-1)  # [n, L, O]: distance - r
    earlier = (clear[:, :c] < 0).any(axis=(1, 2)) | (clear[:, c, :o] < 0).any(axis=1)
    half = gen_robots.capsule_centred(ch.cap_p0, ch.cap_p1)[4][c]
    r = float(np.float32(ch.cap_r[c]))
    pd = ((centre - np.clip(centre, lo[o], hi[o])) ** 2).sum(axis=1)
    return dict(far=~earlier & (pd > float(gen_robots.cull_threshold(half + r))), certain_hit=~earlier & (pd < float(gen_robots.inside_threshold(r))),
                touching=~earlier & (np.abs(clear[:, c, o]) < 0.01), already_hit=earlier)  # fmt: skip


@functools.lru_cache(maxsize=None)
def problem(name, set_name):
    """-> x0 [128, d], target [64, 7], (lo, hi) of the cuboids, the item whose classes seed 0 holds, the NaN row"""
    ch, o32, o64 = model(name)
    obs = SETS[set_name]
    lo, hi = H.box_corners([c for c, _ in obs], [T for _, T in obs])
    rng = np.random.RandomState(97)
    pool = H.f32(rng.uniform(ch.lo + 0.05, ch.hi - 0.05, size=(POOL, ch.ndof)))
    best = None
    for c in range(1, ch.n_capsules):
        for o in range(lo.shape[0]):
            cls = lane_classes(name, pool, lo, hi, (c, o))
            least = min(int(v.sum()) for v in cls.values())
            if best is None or least > best[0]:
                best = (least, (c, o), cls)
    least, item, cls = best
    assert least >= PER_CLASS, (name, set_name, item, {k: int(v.sum()) for k, v in cls.items()})
    rows = np.stack([np.flatnonzero(cls[k])[:PER_CLASS] for k in ("far", "certain_hit", "touching", "already_hit")], axis=1).reshape(-1)
    path = pool[rows]  # lane i is of class i % 4
    target = H.f32(o64.fk(path))
    seed1 = H.f32(rng.uniform(ch.lo, ch.hi, size=(W, ch.ndof)))
    x0 = np.concatenate([path, seed1])
    nan_row = W + 37
    x0[nan_row, 2] = np.nan
    return x0, target, (lo, hi), item, nan_row


def expected(name, x, boxes, jl):
    _, o32, _ = model(name)
    return o32.masks(x, boxes[0], boxes[1], jl[0].astype(np.float64), jl[1].astype(np.float64))


def launch_and_check(rb, name, set_name, K, clamp):
    x0, target, boxes, item, nan_row = problem(name, set_name)
    ch = model(name)[0]
    n = x0.shape[0]
    xd = torch.tensor(x0, dtype=torch.float32, device=DEV)
    td = torch.tensor(target, dtype=torch.float32, device=DEV)
    packed = torch.empty(rb.PACKED_BYTES_PER_ROW * n, dtype=torch.uint8, device=DEV)
    summary = torch.full((S, 8), -1.0, dtype=torch.float32, device=DEV)
    r = rb.lm_pose_steps(xd, td, n_steps=K, clamp=clamp, packed_out=packed, summary_out=summary, shape=_hip.SHAPE_ROW, **LM)
    again = rb.seed_summary(r["x"], packed, S, W)
    # the stage that keeps every test, on the same inputs
    full = rb.lm_pose_steps(xd, td, n_steps=K, clamp=clamp, want_errors=True, want_collisions=True, want_min_dists=True, shape=_hip.SHAPE_ROW, **LM)
    torch.cuda.synchronize()
    x = r["x"].cpu().numpy().astype(np.float64)
    assert np.array_equal(full["x"].cpu().numpy(), r["x"].cpu().numpy(), equal_nan=True)
    assert np.isnan(x[nan_row]).any() and np.isfinite(np.delete(x, nan_row, axis=0)).all()
    want = expected(name, x, boxes, rb.padded_joint_limits())
    got = {k: r[k].cpu().numpy() for k in ("self_mask", "env_mask", "jlim_mask", "ext_cost")}
    for k in ("self_mask", "env_mask", "jlim_mask"):
        assert np.array_equal(got[k], want[k]), (name, set_name, K, k, np.flatnonzero(got[k] != want[k])[:8])
        assert np.array_equal(full[k].cpu().numpy(), got[k]), (name, set_name, K, k, "COLL = 2")
    assert np.array_equal(got["ext_cost"], want["ext_cost"].astype(np.float32))
    assert got["env_mask"][nan_row] == 0 and got["self_mask"][nan_row] == 0
    for k in ("min_env", "min_self"):
        g, w = full[k].cpu().numpy(), want[k].astype(np.float32)
        bad = np.flatnonzero(g != w)
        bad = bad[bad != nan_row]  # (the minima of a NaN row are whatever its finite capsules give: not pinned, and not this stage's)
        assert bad.size == 0, (name, set_name, K, k, bad[:8], g[bad[:8]], w[bad[:8]])
    sm = summary.cpu().numpy()
    assert np.array_equal(sm, again.cpu().numpy(), equal_nan=True)
    for col, k in ((4, "self_mask"), (5, "env_mask"), (6, "jlim_mask")):
        assert np.array_equal(sm[:, col], got[k].reshape(S, W).sum(1).astype(np.float32)), k
    assert np.array_equal(sm[:, 7], got["ext_cost"].reshape(S, W).astype(np.float64).sum(1).astype(np.float32))
    # seed 0's wavefront still holds every class for the item it was built for; the masks are neither empty nor full
    cls = lane_classes(name, x[:W], boxes[0], boxes[1], item)
    assert all(int(v.sum()) >= PER_CLASS // 2 for v in cls.values()), (name, set_name, K, {k: int(v.sum()) for k, v in cls.items()})
    assert 0 < got["env_mask"][:W].sum() < W and got["env_mask"][W:].sum() < W
    return x, boxes


@pytest.mark.parametrize("set_name", list(SETS))
@pytest.mark.parametrize("name", ROBOTS)
def test_fused_launches_bit_for_bit(robots, name, set_name):
    rb = robots[name]
    obs = SETS[set_name]
    rb.set_obstacles([c for c, _ in obs], [T for _, T in obs])
    rb.set_joint_limit_padding(float(np.deg2rad(1.5)), 0.03)
    try:
        launch_and_check(rb, name, set_name, K=1, clamp=False)
        x, boxes = launch_and_check(rb, name, set_name, K=2, clamp=True)
    finally:
        rb.set_obstacles([], [])
        rb.set_joint_limit_padding(None, None)
    if set_name == "thin_and_large":  # the set is what it says: a capsule centre inside the large cuboid, a plate thinner than 1 cm
        ep = model(name)[1].capsule_endpoints(np.delete(x, problem(name, set_name)[4], axis=0))
        centre = 0.5 * (ep[..., :3] + ep[..., 3:])
        assert ((centre > boxes[0][1]) & (centre < boxes[1][1])).all(axis=-1).any()
        assert (boxes[1][0] - boxes[0][0]).min() < 0.01


@pytest.mark.parametrize("set_name", list(SETS))
@pytest.mark.parametrize("name", ROBOTS)
def test_stand_alone_kernel_on_a_partly_filled_wavefront(robots, name, set_name):
    """collision_masks on 100 rows: the built wavefront, then 36 rows of which one has ONE NaN joint (capsules in front of that joint
    stay finite, the others are NaN in part or in whole: the certain-hit rule must not fire on them)"""
    rb = robots[name]
    x0, _, boxes, item, nan_row = problem(name, set_name)
    q = x0[:100].copy()
    assert nan_row >= 100
    q[80, 3] = np.nan
    obs = SETS[set_name]
    rb.set_obstacles([c for c, _ in obs], [T for _, T in obs])
    rb.set_joint_limit_padding(float(np.deg2rad(1.5)), 0.03)
    try:
        qd = torch.tensor(q, dtype=torch.float32, device=DEV).view(1, 100, -1)
        got = rb.collision_masks(qd)
        full = rb.collision_masks(qd, want_min_dists=True)
        torch.cuda.synchronize()
        want = expected(name, q, boxes, rb.padded_joint_limits())
    finally:
        rb.set_obstacles([], [])
        rb.set_joint_limit_padding(None, None)
    for k in ("self_mask", "env_mask", "jlim_mask"):
        assert np.array_equal(got[k].cpu().numpy().reshape(-1).astype(np.uint8), want[k]), (name, set_name, k)
        assert np.array_equal(full[k].cpu().numpy().reshape(-1).astype(np.uint8), want[k]), (name, set_name, k, "with minima")
    assert np.array_equal(got["ext_cost"].cpu().numpy().reshape(-1), want["ext_cost"].astype(np.float32))
    finite = np.isfinite(q).all(axis=1)  # (the minima of the NaN row are not pinned)
    assert np.array_equal(full["min_env"].cpu().numpy().reshape(-1)[finite], want["min_env"].astype(np.float32)[finite])
    cls = lane_classes(name, q[:W], boxes[0], boxes[1], item)
    assert all(int(v.sum()) == PER_CLASS for v in cls.values())
