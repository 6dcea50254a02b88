"""The oracle (oracle/lmik_oracle.c in fp64 and fp32, oracle/ref_torch.py) against recorded runs of the reference's own code.

tests/golden/reference_runs_<robot>.npz hold what the reference's cppflow functions returned for seeded inputs (made by
tests/golden/make_reference_runs.py through oracle/reference_run.py; nothing here needs the reference, except the freshness test,
which skips without it).  Search paths, chosen candidates, masks, verdicts and row counts must be EQUAL.  fp64 quantities are held to
16 x the worst difference measured between the fp64 oracle and the recording over all robots and cases (the allowance is for another
summation order, in the Cholesky above all), and each such bar stays below a thousandth of the bar the kernels are held to for the
same quantity in tests/test_gpu_reference_runs.py:

    quantity                                        measured worst     bar (16 x)   kernel bar / 1000
    coupled step  x_new                             3.0e-11            4.8e-10      2e-7
    coupled step  stacked residual r                8.3e-16            1.4e-14      2e-10
    pose step     x_new (rows sigma_min >= 2e-2)    2.2e-10            3.6e-9       5e-6
    pose step     scaled J, scaled e                1.6e-15            2.5e-14      1e-8
    pose errors (rad, m), current position          6.0e-16            9.6e-15      1e-8
    plan metrics  (cm, deg, rad, m)                 1.5e-12            2.4e-11      2e-7
    angular / prismatic changes                     0 (equal)          -            -

The worst coupled step is fetch's plain pose case (six pose rows per eight joints, lambda = 1e-6: the least conditioned system of the
set); every case with differencing rows stays below 1e-12.  These figures hold on the robot the runs were recorded on, ref_torch's
kinematics over the canonical chain's fp32-rounded constants (ref_torch.canonical_spec): on the URDF doubles, or with box corners
summed in fp64, the same comparison shows 1e-9 .. 1e-7, which measures constants, not the reference's logic.
"""

import os

import numpy as np
import pytest
import torch

from oracle import ref_torch
from tests import helpers as H
from tests import reference_runs as R

BAR = dict(step_x=4.8e-10, step_r=1.4e-14, pose_x=3.6e-9, pose_Je=2.5e-14, pose_err=9.6e-15, plan=2.4e-11)
KERNEL_BAR = dict(step_x=2e-4, step_r=2e-7, pose_x=5e-3, pose_Je=1e-5, pose_err=1e-5, plan=2e-4)
MAX_BYTES = 99832  # tests/golden/lm_golden_chain12.npz, the largest fixture before these
REF_ROOT = os.environ.get("CPPFLOW_REFERENCE_ROOT", "/root/reference")

_worst = {}


def _hold(key, got, want, what):
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max())
    _worst[key] = max(_worst.get(key, 0.0), err)
    print(f"{what}: {key} differs by {err:.3e} (bar {BAR[key]:.1e})")
    assert err <= BAR[key], (what, key, err, BAR[key])


def _boxes(obstacles):
    pairs = [H.cuboid_obstacle(*o) for o in obstacles]
    return H.box_corners([c for c, _ in pairs], [T for _, T in pairs])


def _torch_robot(name, dtype):
    from cppflow_amd.robot_zoo import ROBOT_SPECS

    return ref_torch.TorchRobot(ref_torch.canonical_spec(ROBOT_SPECS[name]()), dtype=dtype)  # (the robot the runs were recorded on)


def test_bars_stay_a_thousandth_of_the_kernel_bars():
    for k, b in BAR.items():
        assert b < KERNEL_BAR[k] / 1000, k


@pytest.mark.parametrize("name", R.ROBOTS)
def test_fixture_is_plain_data_within_the_size_limit(name):
    assert os.path.getsize(R.fixture_path(name)) <= MAX_BYTES
    with np.load(R.fixture_path(name), allow_pickle=False) as z:
        assert all(z[k].dtype != object for k in z.files)
    runs = R.load(name)
    assert len(runs) > 250 and {f"step_{f}__x_new" for f in R.STEP_FAMILIES} <= set(runs)


@pytest.mark.parametrize("name", R.ROBOTS)
def test_joint_limit_almost_violations(name):
    """joint_limit_almost_violations_3d (cppflow/search.py:25-52): configurations ON a padded limit, one ulp inside and one ulp outside"""
    runs, ch = R.load(name), H.chain(name)
    qs, want = runs["jl__qs"], runs["jl__violations"]
    eps_r, eps_p = runs["jl__eps"]
    rb = _torch_robot(name, torch.float32)
    got = ref_torch.joint_limit_almost_violations_3d(rb, torch.tensor(qs), float(eps_r), float(eps_p)).numpy()
    assert np.array_equal(got, want)
    lo = np.asarray(ch.lo, dtype=np.float32)
    hi = np.asarray(ch.hi, dtype=np.float32)
    pad = np.where(np.asarray(ch.jtype) == 0, np.float32(eps_r), np.float32(eps_p)).astype(np.float32)
    m = H.oracle32(name).masks(qs.reshape(-1, ch.ndof).astype(np.float64), None, None, (lo + pad).astype(np.float64), (hi - pad).astype(np.float64))
    assert np.array_equal(m["jlim_mask"].reshape(want.shape).astype(np.float32), want)


@pytest.mark.parametrize("name", R.ROBOTS)
def test_mjacs(name):
    """_get_mjacs (cppflow/search.py:100-125), prismatic scaling included"""
    runs = R.load(name)
    q = torch.tensor(runs["mjacs__q"].astype(np.float32))
    got = ref_torch._get_mjacs(q, _torch_robot(name, torch.float32)).numpy()
    assert np.array_equal(got, runs["mjacs__mjacs"])


@pytest.mark.parametrize("k,T", R.DP_CASES)
@pytest.mark.parametrize("name", R.ROBOTS)
def test_dp_search_path_and_candidates(name, k, T):
    """dp_search (cppflow/search.py:128-191) with its first-minimum tie rule; dp_search_slow (:55-97), which weighs a prismatic joint
    like a revolute one, where it was recorded"""
    c = R.section(R.load(name), f"dp_{k}x{T}")
    q, ext = c["q"].astype(np.float64), c["ext_cost"].astype(np.float64)
    idx, _ = H.oracle32(name).dp_search(q, ext)
    assert np.array_equal(idx, c["idx"])
    assert np.array_equal(q[idx, np.arange(T)].astype(np.float32), c["path"])
    rb = _torch_robot(name, torch.float32)
    path = ref_torch.dp_search(rb, torch.tensor(c["q"].astype(np.float32)), torch.tensor(c["ext_cost"])).numpy()
    assert np.array_equal(path, c["path"])
    if "path_slow" in c:
        idx1, _ = H.oracle32(name).dp_search(q, ext, prismatic_scaling=1.0)
        assert np.array_equal(q[idx1, np.arange(T)].astype(np.float32), c["path_slow"])
        if not rb.prismatic_joint_idxs:
            assert np.array_equal(c["path_slow"], c["path"])


@pytest.mark.parametrize("family", R.STEP_FAMILIES)
@pytest.mark.parametrize("name", R.ROBOTS)
def test_coupled_step(name, family):
    """LmResidualFns.get_r_and_J + _lm_full_step (cppflow/optimization_utils.py:486-731, optimization.py:95-113), one option family per
    case: the fp64 oracle's step on the recorded inputs, its stacked residual row for row, and the number of rows of every block"""
    runs = R.load(name)
    c = R.section(runs, f"step_{family}")
    S, T, d = c["x"].shape
    x = c["x"].astype(np.float64).reshape(S * T, d)
    xv = c["virtual_configs"].astype(np.float64).reshape(S * T, d) if "virtual_configs" in c else None
    pm = R.project_params(c["params"])
    lo, hi = _boxes(c["obstacles"])
    got, r = H.oracle64(name).lm_full_step(x, c["target"].astype(np.float64), pm, S, T, virtual_configs=xv, boxes_lo=lo, boxes_hi=hi,
                                           return_residual=True, constraints=R.project_constraints(runs["step__constraints"]))  # fmt: skip
    want_r = np.concatenate([c[f"s0__r_{b}"][:, 0] for b in R.BLOCKS if f"s0__r_{b}" in c])
    assert r.shape == want_r.shape, (name, family, "the stacked residual has another number of rows")
    _hold("step_r", r, want_r, f"{name} {family}")
    _hold("step_x", got, c["x_new"].reshape(S * T, d), f"{name} {family}")
    # what the recording itself promises: the blocks named present are there, J has r's rows, the filter dropped rows
    for s in range(S):
        for bi, b in enumerate(R.BLOCKS):
            assert (f"s{s}__r_{b}" in c) == bool(c["blocks_present"][s, bi])
            if f"s{s}__r_{b}" in c:
                assert c[f"s{s}__J_{b}"].shape == (c[f"s{s}__r_{b}"].shape[0], T * d)
    if family == "diff_filter":
        assert all(c[f"s{s}__r_differencing"].shape[0] < (T - 1) * d for s in range(S))


@pytest.mark.parametrize("name", R.ROBOTS)
def test_pose_step_errors_and_clamp(name):
    """levenberg_marquardt_only_pose (cppflow/optimization.py:61-92), get_6d_pose_errors and clamp_to_joint_limits
    (optimization_utils.py:802-833)"""
    runs = R.load(name)
    c = R.section(runs, "pose")
    S = int(c["S"])
    x, target = c["x"], H.stacked(c["target"], S)
    lm = dict(zip(("lm_lambda", "alpha_position", "alpha_rotation"), (float(v) for v in c["lm"])))
    orc = H.oracle64(name)
    e, cur = orc.pose_errors(x, target)
    _hold("pose_err", e, c["errors"], f"{name} pose errors")
    _hold("pose_err", cur[:, :3], c["current_poses"][:, :3], f"{name} current position")
    xo, Jo, eo, fails = orc.lm_step(x, target, solver=0, **lm)
    assert fails == 0
    _hold("pose_Je", Jo, c["J_scaled"], f"{name} scaled J")
    _hold("pose_Je", eo, c["e_scaled"], f"{name} scaled e")
    ok = np.linalg.svd(c["J_scaled"], compute_uv=False)[:, -1] >= 2e-2
    assert ok.mean() > 0.85
    _hold("pose_x", xo[ok], c["x_new"][ok], f"{name} pose step")
    # ref_torch issues the reference's op sequence on the same kinematics
    rb = _torch_robot(name, torch.float64)
    xt = ref_torch.levenberg_marquardt_only_pose(rb, torch.tensor(x), torch.tensor(target), lm["lm_lambda"], lm["alpha_position"], lm["alpha_rotation"])
    _hold("pose_x", xt.numpy()[ok], c["x_new"][ok], f"{name} pose step (ref_torch)")
    k = R.section(runs, "clamp")
    assert np.array_equal(H.oracle32(name).clamp(k["x"].astype(np.float64)).astype(np.float32), k["clamped"])
    got = ref_torch.clamp_to_joint_limits(_torch_robot(name, torch.float32), torch.tensor(k["x"].copy())).numpy()
    assert np.array_equal(got, k["clamped"])


@pytest.mark.parametrize("name", R.ROBOTS)
def test_evaluation(name):
    """cppflow/evaluation_utils.py and x_is_valid (optimization_utils.py:836-923) on four short paths against one target path: path 0
    meets every constraint, the others cross thresholds that it clears"""
    runs, ch = R.load(name), H.chain(name)
    c = R.section(runs, "eval")
    paths, target = c["paths"], c["target"]
    n, W, d = paths.shape
    orc = H.oracle64(name)
    rev = np.asarray(ch.jtype) == 0
    for i in range(n):
        assert np.array_equal(orc.angular_changes(paths[i]), c["angular_changes"][i])
        assert np.array_equal(np.diff(paths[i][:, ~rev], axis=0), c["prismatic_changes"][i])
    x = paths.reshape(n * W, d)
    m = orc.plan_metrics(x, H.stacked(target, n), n, W)
    plan = c["plan"]
    _hold("plan", m[:, :8], plan[:, :8], f"{name} plan metrics")
    assert np.array_equal(m[:, 8], plan[:, 8])  # joint-limit violations
    _hold("plan", m[:, 4], c["mjac_deg"], f"{name} calculate_mjac_deg")
    _hold("plan", m[:, [4, 5]], c["get_mjacs"], f"{name} get_mjacs")
    _hold("plan", m[:, 4], c["per_ts_mjac_deg"].max(axis=1), f"{name} per-timestep mjac deg")
    _hold("plan", m[:, 5], c["per_ts_mjac_cm"].max(axis=1), f"{name} per-timestep mjac cm")
    _hold("plan", m[:, 0], c["pos_err_cm"].max(axis=1), f"{name} position error")
    _hold("plan", m[:, 2], c["rot_err_deg"].max(axis=1), f"{name} rotation error")
    # the verdicts: the four thresholds on the oracle's maxima, strict, as errors_are_below_threshold compares them
    sv = orc.seed_validity(x, H.stacked(target, n), n, W)
    flags = sv < c["constraints"][None, :]
    assert np.array_equal(flags, c["below"][:, 1:]) and np.array_equal(flags.all(axis=1), c["below"][:, 0])
    lo, hi = _boxes(c["obstacles"])
    masks = H.oracle32(name).masks(x, lo, hi, None, None)
    colliding = (masks["self_mask"] | masks["env_mask"]).reshape(n, W)
    assert np.array_equal(masks["self_mask"].reshape(n, W) > 0, c["batched_self"])
    assert np.array_equal(masks["env_mask"].reshape(n, W) > 0, c["batched_env"])
    valid = flags.all(axis=1) & ~colliding.any(axis=1)
    assert np.array_equal(valid, c["valid_alone"]) and np.array_equal(valid, plan[:, 12] > 0)
    for order, first in zip(c["orders"], c["first_valid"]):
        order = [int(o) for o in order if o >= 0]
        hits = [j for j, p in enumerate(order) if valid[p]]
        assert (hits[0] if hits else -1) == int(first)


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF_ROOT, "cppflow", "optimization_utils.py")), reason="no checkout of the reference here")
@pytest.mark.parametrize("name", R.ROBOTS)
def test_recorded_runs_are_fresh(name):
    """Where the reference is at hand: run every case again, in memory, and require the committed file to hold exactly that"""
    from oracle.reference_run import load_reference
    from tests.golden.make_reference_runs import generate

    dtype = torch.get_default_dtype()
    try:
        fresh = generate(name, load_reference(REF_ROOT))
    finally:
        torch.set_default_dtype(dtype)
    runs = R.load(name)
    assert list(fresh) == list(runs)
    for k, v in fresh.items():
        v = np.asarray(v)
        assert v.shape == runs[k].shape and v.dtype.kind == runs[k].dtype.kind, k
        assert np.array_equal(v, runs[k], equal_nan=v.dtype.kind == "f"), k
