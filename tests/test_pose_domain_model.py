"""CPU side of the pose-domain sweep (tests/pose_domain.py; the GPU side is tests/test_gpu_pose_domain.py).

  * The numpy fp32 restatement of atan2_lm / asin_lm stays inside the FUNCTION budget (4 u relative plus one ulp of pi, resp. pi/2,
    behind a fix-up) against fp64 on the operands of the GPU sweep and on dense 1-D sweeps down to the denormals and the 1e-30
    floor: the bars of the GPU module can be met by a correct implementation.
  * The sweep's reference agrees with the fp64 oracle within the suite's existing 1e-5 on calm rows (which guards the reference's own
    rpy convention), and the frame it starts from reproduces the fp32 oracle's FK bit for bit.
  * At most 2 % of any robot's sweep is excluded from the tight bars outside the deliberately constructed +-pi/2 pitch block.
"""

import numpy as np
import pytest

from tests import helpers as H
from tests import pose_domain as P

CASES = [(n, k) for n in P.ROBOTS for k in range(P.N_BASES)]


def test_sweep_shape_and_determinism():
    R, delta, blocks = P.offsets()
    n = len(R)
    assert 20000 <= n <= 26000 and delta.shape == (n, 3)
    assert np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3)).max() < 1e-6 and np.allclose(np.linalg.det(R), 1.0, atol=1e-6)
    assert sorted((s.start, s.stop) for s in blocks.values())[0][0] == 0 and max(s.stop for s in blocks.values()) == n
    assert np.array_equal(R[blocks["zero"]][0], np.eye(3)) and not delta[blocks["zero"]].any()
    lengths = np.linalg.norm(delta, axis=1)
    assert (lengths == 0).mean() > 0.2 and lengths.max() <= 1.0 + 1e-12 and lengths[lengths > 0].min() < 2e-7
    idx = P.subsample(2048)
    assert len(idx) == 2048 == len(np.unique(idx)) and all(((idx >= s.start) & (idx < s.stop)).any() for s in blocks.values())


@pytest.mark.parametrize("name,k", CASES)
def test_reference_frame_is_the_fp32_oracles_end_effector(name, k):
    """link_frames(x)[:, ndof] converted with the fp32 restatement of mat_to_quat reproduces oracle32.fk(x) bit for bit"""
    q = np.concatenate([P.base_config(name, k)[None], H.random_configs(name, 512, seed=3 + k)])
    R, p = P.ee_frame32(name, q)
    pose = H.oracle32(name).fk(q)
    assert np.array_equal(p.astype(np.float64), pose[:, :3])
    assert np.array_equal(P.mat_to_quat32(R).astype(np.float64), pose[:, 3:])


@pytest.mark.parametrize("name,k", CASES)
def test_reference_agrees_with_the_fp64_oracle_on_calm_rows(name, k):
    x, target = P.problem(name, k)
    ref = P.sweep_reference(name, k)
    e64, _ = H.oracle64(name).pose_errors(x, target)
    pe64, re64 = H.oracle64(name).pose_metrics_exact(x, target)
    ex = P.excluded(ref)
    # calm: far from gimbal lock (the rpy of a nearly locked rotation is ill-conditioned) and from the +-pi seam of roll / yaw
    calm = (~ex.any(axis=1)) & (np.abs(ref["sp"]) < 0.99) & (np.abs(ref["e"][:, [0, 2]]).max(axis=1) < np.pi - 1e-3)
    assert calm.mean() > 0.3
    assert np.abs(ref["e"] - e64)[calm].max() < 1e-5
    assert np.abs(ref["pos"] - pe64).max() < 1e-5
    assert np.abs(ref["rot"] - re64).max() < 1e-5


@pytest.mark.parametrize("name,k", CASES)
def test_construction_puts_the_offsets_rpy_into_the_residual(name, k):
    """R_err = R_off by construction, up to the fp32 rounding of the target quaternion and of the frame (1e-6)"""
    R_off, delta, blocks = P.offsets()
    ref = P.sweep_reference(name, k)
    s = blocks["grid"]
    assert np.abs(np.clip(-R_off[s, 2, 0], -1, 1) - ref["sp"][s]).max() < 2e-6
    assert np.abs(R_off[s, 2, 1] - ref["roll_yx"][0][s]).max() < 2e-6 and np.abs(R_off[s, 0, 0] - ref["yaw_yx"][1][s]).max() < 2e-6
    lad = ref["theta"][blocks["ladder"]].reshape(P.N_LADDER_AXES, -1)
    assert np.abs(lad - P.THETA_LADDER).max() < 2e-6
    assert np.abs(ref["pos"] - np.linalg.norm(delta, axis=1)).max() < 2e-7


@pytest.mark.parametrize("name", P.ROBOTS)
def test_exclusion_cap(name):
    _, _, blocks = P.offsets()
    lock = blocks["grid_lock"]
    for k in range(P.N_BASES):
        ex = P.excluded(P.sweep_reference(name, k)).any(axis=1)
        outside = np.ones(len(ex), dtype=bool)
        outside[lock] = False
        assert ex[outside].sum() <= 0.02 * len(ex), (name, k, ex[outside].sum(), len(ex))
        assert ex[lock].mean() > 0.5  # the block is what it is said to be


@pytest.mark.parametrize("name,k", CASES)
def test_restated_functions_meet_the_function_budget_on_the_sweep(name, k):
    ref = P.sweep_reference(name, k)
    for y, x in (ref["roll_yx"], ref["yaw_yx"]):
        y32, x32 = y.astype(np.float32), x.astype(np.float32)
        want = np.arctan2(y32.astype(np.float64), x32.astype(np.float64))
        got = P.atan2_lm32(y32, x32).astype(np.float64)
        d = np.abs(got - want)
        d = np.minimum(d, np.abs(2 * np.pi - d))  # the seam
        assert (d <= P.atan2_budget(y32, x32, want)).all(), (d - P.atan2_budget(y32, x32, want)).max()
    sp32 = ref["sp"].astype(np.float32)
    want = np.arcsin(sp32.astype(np.float64))
    assert (np.abs(P.asin_lm32(sp32) - want) <= P.asin_budget(sp32, want)).all()


def test_restated_atan2_dense():
    rng = np.random.RandomState(0)
    # the unit circle, random radii from 1e-30 (the floor) to 1, and a log sweep of y at x = +-1 down to the denormals
    t = np.linspace(-np.pi, np.pi, 1 << 20)
    r = 10.0 ** rng.uniform(-29.9, 0, size=t.shape)
    y = np.concatenate([np.sin(t), r * np.sin(t), np.logspace(-45, 0, 4096), -np.logspace(-45, 0, 4096), np.logspace(-45, 0, 4096)]).astype(np.float32)
    x = np.concatenate([np.cos(t), r * np.cos(t), np.ones(4096), np.ones(4096), -np.ones(4096)]).astype(np.float32)
    keep = np.maximum(np.abs(x), np.abs(y)) >= np.float32(1e-30)  # (below the floor the quotient is taken against the floor)
    y, x = y[keep], x[keep]
    want = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    got = P.atan2_lm32(y, x).astype(np.float64)
    d = np.abs(got - want)
    d = np.minimum(d, np.abs(2 * np.pi - d))
    bud = P.atan2_budget(y, x, want)
    assert (d <= bud).all(), (d / np.maximum(bud, 1e-300)).max()
    small = (np.abs(want) < 1e-3) & (want != 0)
    assert (d[small] / np.abs(want[small])).max() < 2 * P.U  # full RELATIVE accuracy towards 0
    # exact values, and the floor: with both operands below 1e-30 the quotient is taken against the floor (atan2(0, 0) = 0 by design)
    assert P.atan2_lm32(0.0, 1.0) == 0 and P.atan2_lm32(0.0, 0.0) == 0 and P.atan2_lm32(0.0, -1.0) == P.PI32
    assert P.atan2_lm32(1.0, 0.0) == P.HALF_PI32 and P.atan2_lm32(-1.0, 0.0) == -P.HALF_PI32
    fl = np.float32(1e-30)
    at = np.array([fl, np.nextafter(fl, np.float32(1))], dtype=np.float32)
    assert np.abs(P.atan2_lm32(at, at).astype(np.float64) - np.pi / 4).max() <= 4 * P.U * np.pi / 4
    tiny = np.array([1e-31, 1e-38, 1e-40, 1e-45], dtype=np.float32)
    below = P.atan2_lm32(tiny, tiny)
    assert np.isfinite(below).all() and (below >= 0).all() and (below <= np.float32(np.pi / 4)).all()


def test_restated_asin_dense():
    x = np.concatenate([np.linspace(-1, 1, (1 << 20) + 1), np.logspace(-45, 0, 4096), -np.logspace(-45, 0, 4096)]).astype(np.float32)
    for v in (0.5, -0.5, 1.0, -1.0):
        x = np.concatenate([x, np.array(P._neighbours(v), dtype=np.float32)])
    x = x[np.abs(x) <= 1]
    want = np.arcsin(x.astype(np.float64))
    d = np.abs(P.asin_lm32(x).astype(np.float64) - want)
    bud = P.asin_budget(x, want)
    assert (d <= bud).all(), (d / np.maximum(bud, 1e-300)).max()
    small = (np.abs(want) < 1e-3) & (want != 0)
    assert (d[small] / np.abs(want[small])).max() < 2 * P.U
    assert P.asin_lm32(0.0) == 0 and P.asin_lm32(1.0) == P.HALF_PI32 and P.asin_lm32(-1.0) == -P.HALF_PI32


@pytest.mark.parametrize("name", P.ROBOTS)
def test_bars_pass_the_restated_functions_and_fail_their_mutants(name):
    """The residual check of the GPU module, run on the restated functions over the same sweep: a correct implementation passes
    it; a polynomial coefficient off by 1e-6, asin's pi/2 one fp32 neighbour down, and a swapped pi fix-up constant each fail it."""
    ref = P.sweep_reference(name, 1)
    P.check_residual(P.model_residual(ref), ref, name)
    mutant = list(P.ATAN_COEFFS)
    mutant[6] = 0.19989519
    with pytest.raises(AssertionError):
        P.check_residual(P.model_residual(ref, coeffs=tuple(mutant)), ref, name)
    with pytest.raises(AssertionError):
        P.check_residual(P.model_residual(ref, half_pi=np.nextafter(P.HALF_PI32, np.float32(0))), ref, name)
    # the floor: 8.9e-4 in place of 8.94427191e-4 is 4.4e-6 away, the bar there 1.4e-6
    assert abs(P.FLOOR - 8.9e-4) > (8 * P.DELTA + 4 * P.U * P.FLOOR) * 3
    rot = np.maximum(ref["theta"], 8.9e-4)
    with pytest.raises(AssertionError):
        P.check_metrics(ref["pos"], rot, ref, name)
    P.check_metrics(ref["pos"], ref["rot"], ref, name)
