"""The fused launch's per-seed summary epilogue (block_seed_summary, csrc/kernels_fused.h) against two independent reductions of the
same launch's outputs, bit for bit: cppf_seed_summary (seed_summary_kernel, which re-reads x_out and the per-row outputs) and numpy.

The epilogue reduces the four maxima as unsigned integers on their bit patterns, carries the three hit counts packed in one word
(10 bits each) and skips wrap_pi_all unless a wavefront holds a revolute change beyond 171 degrees; the inputs below are built so that
every one of those paths is taken (and checked, on the launch's own outputs, to have been taken):

  seed 0  x0 at +- the joint limits.  The padded limits are the middle half of every joint's range (`padded_limits`), which a few LM steps
          from a limit do not reach with every joint at once: every row violates them and the jl field is full, W; with a cuboid around
          the whole workspace every row of every seed is env-colliding too (that field full at the same time).  Folded configurations
          that self-collide are among them.
  seed 1  a smooth path whose widest revolute joint jumps from -2.8 to +2.8 between waypoints 10 | 11 (inside a wavefront) and back
          between 63 | 64 (lanes 63 | 0 of two wavefronts of the seed, W > 64): the wrap path, in the seed's first wavefront only.
  seed 2  the same path with that joint held at -2.8 (no jump: its later wavefronts take the unwrapped path) and one NaN row, whose
          summary holds +inf.

S = 3 leaves the last 256-row workgroup with inactive wavefronts (192, 384 and 768 rows)."""

import functools

import numpy as np
import pytest
import torch

from cppflow_amd.problems_synthetic import obstacle_arrays
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S = 3
JUMP = 2.8
LM = dict(lm_lambda=1e-6, alpha_position=3.5, alpha_rotation=0.35)
RAD2DEG = np.float32(57.29577951308232087680)


def wrap_joint(name):
    """the first revolute joint whose limits allow -2.8 and +2.8 (from the robot's table)"""
    ch = H.chain(name)
    ok = [j for j in range(ch.ndof) if ch.jtype[j] == 0 and ch.lo[j] < -JUMP - 0.05 and ch.hi[j] > JUMP + 0.05]
    assert ok, name
    return ok[0]


def padded_limits(name):
    """the middle half of every joint's range (seeds 1 and 2 start inside it, seed 0 far outside); the wrap joint, which seeds 1 and 2
    hold next to its limits, is left unpadded"""
    ch = H.chain(name)
    mid, half = 0.5 * (ch.lo + ch.hi), 0.5 * (ch.hi - ch.lo)
    lo, hi = mid - 0.5 * half, mid + 0.5 * half
    lo[wrap_joint(name)], hi[wrap_joint(name)] = -4.0, 4.0
    return lo.astype(np.float32), hi.astype(np.float32)


def nan_row(W):
    return 2 * W + W - 24  # in seed 2's last wavefront


@functools.lru_cache(maxsize=None)
def summary_problem(name, W):
    """-> x0 [3 W, d], target [W, 7] (fp32-representable float64)"""
    ch = H.chain(name)
    d, jw = ch.ndof, wrap_joint(name)
    rng = np.random.RandomState(1000 + W)
    mid, half = 0.5 * (ch.lo + ch.hi), 0.5 * (ch.hi - ch.lo)
    qa, qb = mid + 0.4 * half * rng.uniform(-1, 1, d), mid + 0.4 * half * rng.uniform(-1, 1, d)
    t = np.linspace(0.0, 1.0, W)[:, None]
    q_smooth = qa + (qb - qa) * t  # a straight line in joint space: consecutive waypoints differ by < 0.05 rad
    w = np.arange(W)
    q_smooth[:, jw] = -JUMP + 1e-3 * np.sin(w)
    q_jump = q_smooth.copy()
    q_jump[11:64, jw] += 2 * JUMP  # -2.8 -> +2.8 at 10 | 11, back at 63 | 64 (W > 64)
    target = H.f32(H.oracle64(name).fk(H.f32(q_jump)))
    x0 = np.empty((S, W, d))
    x0[0] = np.where(rng.rand(W, d) < 0.5, ch.lo, ch.hi)
    x0[0, ::7] = ch.hi  # (every joint at its upper limit: folded)
    x0[1] = q_jump + 0.002 * rng.randn(W, d)
    x0[2] = q_smooth + 0.002 * rng.randn(W, d)
    x0 = np.clip(x0, ch.lo, ch.hi).reshape(S * W, d)
    x0[nan_row(W), d // 2] = np.nan
    return H.f32(x0), target


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.fixture(scope="module")
def robots():
    from cppflow_amd.robots import get_robot

    return {n: get_robot(n) for n in ("panda", "fetch")}


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("W", [64, 128, 256])
@pytest.mark.parametrize("name", ["panda", "fetch"])
def test_summary_epilogue_bit_for_bit(robots, name, W, K):
    rb = robots[name]
    ch = H.chain(name)
    d, jw, n = ch.ndof, wrap_joint(name), S * W
    obs = obstacle_arrays([(0.0, 0.0, 0.5, 6.0, 6.0, 6.0)])  # encloses the whole workspace
    rb.set_obstacles([c for c, _ in obs], [T for _, T in obs])
    rb.set_padded_joint_limits(padded_limits(name))
    try:
        x0, target = summary_problem(name, W)
        x0, target = torch.tensor(x0, dtype=torch.float32, device=DEV), torch.tensor(target, dtype=torch.float32, device=DEV)
        packed = torch.empty(rb.PACKED_BYTES_PER_ROW * n, dtype=torch.uint8, device=DEV)
        fused = torch.full((S, 8), -1.0, dtype=torch.float32, device=DEV)
        r = rb.lm_pose_steps(x0, target, n_steps=K, packed_out=packed, summary_out=fused, **LM)
        want = rb.seed_summary(r["x"], packed, S, W)
        torch.cuda.synchronize()
        got = fused.cpu().numpy()
        # 1. the independent reduction kernel on the launch's own outputs
        assert np.array_equal(bits(got), bits(want.cpu().numpy())), (got, want)
        # 2. numpy on the per-row outputs (fp32 products, as the kernels form them; NaN -> +inf)
        pe, re = (r[k].cpu().numpy().reshape(S, W) for k in ("pos_err_m", "rot_err_rad"))
        masks = {k: r[k].cpu().numpy().reshape(S, W).astype(np.int64) for k in ("self_mask", "env_mask", "jlim_mask")}
        cost = r["ext_cost"].cpu().numpy().reshape(S, W)

        def inf_max(a):
            return np.where(np.isnan(a), np.float32(np.inf), a).max(1)

        assert np.array_equal(bits(got[:, 0]), bits(inf_max(np.float32(100.0) * pe)))
        assert np.array_equal(bits(got[:, 1]), bits(inf_max(RAD2DEG * re)))
        for col, key in ((4, "self_mask"), (5, "env_mask"), (6, "jlim_mask")):
            assert np.array_equal(got[:, col], masks[key].sum(1).astype(np.float32)), key
        assert np.array_equal(bits(got[:, 7]), bits(cost.astype(np.float64).sum(1).astype(np.float32)))  # (integers < 2^24: exact)
        # 3. the inputs took the paths they were built for
        x = r["x"].cpu().numpy().reshape(S, W, d)
        assert masks["jlim_mask"][0].sum() == W and (masks["env_mask"].sum(1) == W).all()  # both fields full at once
        assert masks["self_mask"][0].sum() >= 1
        dq = np.abs(np.diff(x, axis=1))[:, :, ch.jtype == 0]  # [S, W - 1, revolute joints]; row w: the change w -> w + 1
        dj = np.abs(np.diff(x[:, :, jw], axis=1))
        assert dj[1, 10] > np.pi and dj[2, 10] < 0.5
        far = np.zeros((S, W), dtype=bool)
        far[:, :-1] = ~(RAD2DEG * dq < 170.9).all(2)  # (NaN counts as far)
        wave_far = far.reshape(S, W // 64, 64).any(2)
        assert wave_far[1, 0]
        if W > 64:
            assert dj[1, 63] > np.pi and dj[2, 63] < 0.5
            assert not wave_far[1, 1:].any() and not wave_far[2, : W // 64 - 1].any()  # the unwrapped path, in the same launch
        assert np.isnan(x[2, nan_row(W) - 2 * W]).all() and wave_far[2, -1]
        assert np.isposinf(got[2, 0]) and np.isposinf(got[2, 1]) and np.isposinf(got[2, 2])
        assert np.isfinite(got[:2, :4]).all()
        if name == "fetch":
            assert got[0, 3] > 0  # mpri: the prismatic joint moves between the limit seed's waypoints
    finally:
        rb.set_obstacles([], [])
        rb.set_padded_joint_limits(None)
