"""The fused launch's mask-only collision stage with the tests dropped that are known before a row runs (csrc/kernels_collision.h:
collide_tests_static<RB, false, IN_LIMITS>) against the fp32 oracle and the stand-alone collision kernel, bit for bit.

  pruned path     a launch that clamps (K = 2): the self pairs of Table::pair_never are not tested, the capsules without a reach bit
                  (csrc/obstacle_reach.h) are skipped.
  unpruned path   K = 1 without clamp: x_out may lie outside the joint limits, where a certified pair CAN collide; one row is built so
                  that it does (and the oracle says so).

Rows: 3 x 64 + 17.  A fused launch takes whole seeds, so the 209 rows go as two launches of the same code: 3 seeds of W = 64 (with the
in-launch summary) and the remaining 17 rows as one seed of W = 17 (a partial wavefront; its summary comes from the second kernel).
A third of the rows start far outside the limits (the clamp saturates), a third are random in-limit configurations, the rest follow
the smooth path.  Two cuboids: one just outside the reach of the capsules of the base and the first two links, one at the path's own
end-effector positions."""

import functools

import numpy as np
import pytest
import torch

from cppflow_amd import _hip, gen_robots
from cppflow_amd.problems_synthetic import obstacle_arrays
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROBOTS = ["panda", "fetch", "fetch_arm", "chain12"]
W, S, TAIL = 64, 3, 17
LM = dict(lm_lambda=1e-6, alpha_position=3.5, alpha_rotation=0.35)


def capsule_reach_from_joint0(ch, c):
    """how far capsule c gets from the origin of joint 0's frame (the bound of csrc/obstacle_reach.h, restated to PLACE a cuboid)"""
    l = int(ch.cap_link[c])
    far = sum(np.linalg.norm(ch.F[j][9:12]) for j in range(1, l + 1))
    far += sum(max(abs(ch.lo[j]), abs(ch.hi[j])) for j in range(l + 1) if ch.jtype[j] == 1)
    return far + max(np.linalg.norm(ch.cap_p0[c]), np.linalg.norm(ch.cap_p1[c])) + ch.cap_r[c]


def colliding_outside_limits(name):
    """(q, pair index): a configuration OUTSIDE the joint limits at which a certified pair is 1 cm deep in collision and every
    uncertified pair is clear by 1 cm; None for a robot without certified pairs"""
    ch = H.chain(name)
    never = gen_robots.pair_never(ch)
    if not any(never):
        return None
    rng = np.random.RandomState(3)
    mid = 0.5 * (ch.lo + ch.hi)
    q = np.tile(mid, (40_000, 1))
    for pi in np.flatnonzero(never):
        joints = gen_robots.pair_joints(ch, int(ch.pairs[pi][0]), int(ch.pairs[pi][1]))[2]
        joints = [j for j in joints if ch.jtype[j] == 0]
        q[:] = mid
        q[:, joints] = rng.uniform(ch.lo[joints] - 1.5, ch.hi[joints] + 1.5, size=(q.shape[0], len(joints)))
        q = H.f32(q)
        d = H.oracle64(name).self_dists(q)
        ok = (d[:, pi] < -0.01) & (d[:, ~np.array(never)] > 0.01).all(axis=1) & ((q < ch.lo) | (q > ch.hi)).any(axis=1)
        if ok.any():
            return q[np.flatnonzero(ok)[0]].copy(), int(pi)
    raise AssertionError(f"{name}: no out-of-limits collision of a certified pair found")


@functools.lru_cache(maxsize=None)
def problem(name):
    """-> x0 [209, d], target [64, 7] (fp32-representable float64), obstacles, the special row (or None)"""
    ch = H.chain(name)
    d, n = ch.ndof, S * W + TAIL
    rng = np.random.RandomState(41)
    mid, half = 0.5 * (ch.lo + ch.hi), 0.5 * (ch.hi - ch.lo)
    qa, qb = mid + 0.5 * half * rng.uniform(-1, 1, d), mid + 0.5 * half * rng.uniform(-1, 1, d)
    path = H.f32(qa + (qb - qa) * np.linspace(0.0, 1.0, W)[:, None])
    special = colliding_outside_limits(name)
    if special is not None:
        path[5] = special[0]  # seed 0, waypoint 5 starts ON its target: the step leaves it where it is
    target = H.f32(H.oracle64(name).fk(path))
    x0 = np.tile(path, (S + 1, 1))[:n] + 0.01 * rng.randn(n, d)
    rows = np.arange(n)
    far = rows % 3 == 0
    x0[far] += np.where(rng.rand(far.sum(), d) < 0.5, -1.0, 1.0) * 6.0 * half  # far outside: the clamp saturates
    x0[rows % 3 == 1] = rng.uniform(ch.lo, ch.hi, size=((rows % 3 == 1).sum(), d))
    if special is not None:
        x0[5] = special[0]
    # cuboid A: its near face 3 cm beyond the reach of every capsule of the base and links 0, 1 (along -y from joint 0's origin)
    o = ch.F[0][9:12]
    prox = [c for c in range(ch.n_capsules) if ch.cap_link[c] <= 1]
    reach = max(capsule_reach_from_joint0(ch, c) for c in prox if ch.cap_link[c] >= 0)
    a = (o[0], o[1] - (reach + 0.03 + 0.1), o[2], 0.2, 0.2, 0.2)
    # cuboid B: where the path's end effector passes
    b = tuple(target[W // 2, :3]) + (0.15, 0.15, 0.15)
    return H.f32(x0), target, obstacle_arrays([a, b]), (5 if special is not None else None), (special[1] if special is not None else None)


@pytest.fixture(scope="module")
def robots():
    from cppflow_amd.robots import get_robot

    return {n: get_robot(n) for n in ROBOTS}


def launch_and_check(rb, name, x0, target, obs, K, clamp):
    """one fused launch (row shape, collision stage, summary) -> x_out, masks; everything compared with the oracle and the stand-alone
    collision kernel on the launch's own x_out"""
    ch = H.chain(name)
    n, Wl = x0.shape[0], target.shape[0]
    Sl = n // Wl
    xd = torch.tensor(x0, dtype=torch.float32, device=DEV)
    td = torch.tensor(target, dtype=torch.float32, device=DEV)
    packed = torch.empty(rb.PACKED_BYTES_PER_ROW * n, dtype=torch.uint8, device=DEV)
    summary = torch.full((Sl, 8), -1.0, dtype=torch.float32, device=DEV)
    r = rb.lm_pose_steps(xd, td, n_steps=K, clamp=clamp, packed_out=packed, summary_out=summary, shape=_hip.SHAPE_ROW, **LM)
    alone = rb.collision_masks(r["x"].view(Sl, Wl, ch.ndof))
    again = rb.seed_summary(r["x"], packed, Sl, Wl)
    torch.cuda.synchronize()
    x = r["x"].cpu().numpy().astype(np.float64)
    lo, hi = H.box_corners([c for c, _ in obs], [T for _, T in obs])
    jl_lo, jl_hi = rb.padded_joint_limits()
    want = H.oracle32(name).masks(x, lo, hi, jl_lo.astype(np.float64), jl_hi.astype(np.float64))
    got = {k: r[k].cpu().numpy() for k in ("self_mask", "env_mask", "jlim_mask", "ext_cost")}
    for k in ("self_mask", "env_mask", "jlim_mask"):
        assert np.array_equal(got[k], want[k]), (name, K, k, np.flatnonzero(got[k] != want[k])[:8])
        assert np.array_equal(alone[k].cpu().numpy().reshape(-1).astype(np.uint8), got[k]), (name, K, k, "stand-alone kernel")
    assert np.array_equal(got["ext_cost"], want["ext_cost"].astype(np.float32))
    assert np.array_equal(alone["ext_cost"].cpu().numpy().reshape(-1), got["ext_cost"])
    sm = summary.cpu().numpy()
    assert np.array_equal(sm.view(np.int32), again.cpu().numpy().view(np.int32))
    for col, k in ((4, "self_mask"), (5, "env_mask"), (6, "jlim_mask")):
        assert np.array_equal(sm[:, col], got[k].reshape(Sl, Wl).sum(1).astype(np.float32)), k
    assert np.array_equal(sm[:, 7], got["ext_cost"].reshape(Sl, Wl).astype(np.float64).sum(1).astype(np.float32))
    return x, got


def both_launches(rb, name, K, clamp):
    x0, target, obs, _, _ = problem(name)
    rb.set_obstacles([c for c, _ in obs], [T for _, T in obs])
    rb.set_joint_limit_padding(float(np.deg2rad(1.5)), 0.03)
    try:
        xa, ga = launch_and_check(rb, name, x0[: S * W], target, obs, K, clamp)
        xb, gb = launch_and_check(rb, name, x0[S * W :], target[:TAIL], obs, K, clamp)
    finally:
        rb.set_obstacles([], [])
        rb.set_joint_limit_padding(None, None)
    return np.concatenate([xa, xb]), {k: np.concatenate([ga[k], gb[k]]) for k in ga}


@pytest.mark.parametrize("name", ROBOTS)
def test_pruned_path_bit_for_bit(robots, name):
    ch = H.chain(name)
    x, got = both_launches(robots[name], name, K=2, clamp=True)
    # the launch clamped: every row inside the limits, the rows that started far outside on them
    lo32, hi32 = ch.lo.astype(np.float32), ch.hi.astype(np.float32)
    assert ((x >= lo32) & (x <= hi32)).all()
    assert ((x == lo32) | (x == hi32)).any(axis=1).sum() >= x.shape[0] // 4
    assert got["env_mask"].any() and not got["env_mask"].all()  # the cuboid in the sweep is hit by some rows, not by all


@pytest.mark.parametrize("name", ROBOTS)
def test_unpruned_path_bit_for_bit(robots, name):
    ch = H.chain(name)
    x, got = both_launches(robots[name], name, K=1, clamp=False)
    assert ((x < ch.lo) | (x > ch.hi)).any(axis=1).sum() >= x.shape[0] // 4  # nothing clamped
    _, _, _, row, pi = problem(name)
    if row is None:
        assert name == "chain12"  # (no certified pair: both paths are the same code)
        return
    # the row built to collide in a certified pair outside the limits still does after its step, ONLY in certified pairs, and is reported
    d = H.oracle64(name).self_dists(x[row : row + 1])[0]
    never = np.array(gen_robots.pair_never(ch))
    assert d[pi] < 0 and (d[~never] > 0).all() and ((x[row] < ch.lo) | (x[row] > ch.hi)).any()
    assert H.oracle32(name).masks(x[row : row + 1])["self_mask"][0] == 1
    assert got["self_mask"][row] == 1


@pytest.mark.parametrize("name", ["panda", "fetch"])
def test_reach_bits_follow_set_obstacles(robots, name):
    """a cuboid out of reach of the proximal capsules, then one around the base: the capsules that were dead are live again"""
    rb, ch = robots[name], H.chain(name)
    x0, target, obs, _, _ = problem(name)
    o = ch.F[0][9:12]
    around_base = obstacle_arrays([(o[0], o[1], o[2], 0.3, 0.3, 0.3)])
    rb.set_joint_limit_padding(float(np.deg2rad(1.5)), 0.03)
    try:
        rb.set_obstacles([c for c, _ in obs[:1]], [T for _, T in obs[:1]])
        _, far = launch_and_check(rb, name, x0[: S * W], target, obs[:1], 2, True)
        rb.set_obstacles([c for c, _ in around_base], [T for _, T in around_base])
        _, near = launch_and_check(rb, name, x0[: S * W], target, around_base, 2, True)
    finally:
        rb.set_obstacles([], [])
        rb.set_joint_limit_padding(None, None)
    assert not far["env_mask"].all() and near["env_mask"].all()
