"""The HIP kernels and the port against recorded runs of the reference's own code (tests/golden/reference_runs_<robot>.npz, made by
tests/golden/make_reference_runs.py; read through tests/reference_runs.py -- the reference itself is not needed here).

Bars are the ones the parity tests of this suite already hold the same quantities to against the project's own oracle; the oracle in
turn is held to these recordings at a thousandth of them on the CPU (tests/test_reference_runs.py).
"""

import numpy as np
import pytest
import torch

from cppflow_amd import _hip
from tests import helpers as H
from tests import reference_runs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


@pytest.fixture(scope="module")
def robots():
    from cppflow_amd.robots import get_robot

    return {n: get_robot(n) for n in R.ROBOTS}


def _obstacle_lists(obstacles):
    pairs = [H.cuboid_obstacle(*o) for o in obstacles]
    return [c for c, _ in pairs], [T for _, T in pairs]


# ---- search --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.ROBOTS)
def test_dp_search_in_every_form(robots, name):
    """dp_search (cppflow/search.py:128-191): the path and the chosen candidate of every waypoint, the last one included, in the
    resident form (k = 257: beyond 256 candidates), with one launch per waypoint and in the table form (k <= 256)"""
    rb, runs = robots[name], R.load(name)
    try:
        for k, T in R.DP_CASES:
            c = R.section(runs, f"dp_{k}x{T}")
            q, ext = dev(c["q"].astype(np.float32)), dev(c["ext_cost"])
            forms = [("resident", "resident", 1), ("launches", "resident", 0)] + ([("table", "table", 1)] if k <= 256 else [])
            for label, method, persistent in forms:
                rb.debug_set("dp_persistent", persistent)
                path, idx, _ = rb.dp_search(q, ext, method=method)
                assert np.array_equal(idx.cpu().numpy(), c["idx"]), (k, T, label)
                assert np.array_equal(path.cpu().numpy(), c["path"]), (k, T, label)
            if "path_slow" in c:  # dp_search_slow (:55-97): no prismatic scaling
                rb.debug_set("dp_persistent", 1)
                slow, _, _ = rb.dp_search(q, ext, prismatic_joint_scaling=1.0)
                assert np.array_equal(slow.cpu().numpy(), c["path_slow"]), (k, T)
    finally:
        rb.debug_set("dp_persistent", 1)


@pytest.mark.parametrize("name", R.ROBOTS)
def test_mjacs(robots, name):
    """cppf_mjacs against _get_mjacs (cppflow/search.py:100-125).  The bar tests/angle_domain.py states for the wrapped joint change is
    the fp32 remainder form BIT FOR BIT -- which is what the reference's fp32 torch.remainder line computes, prismatic scaling first"""
    runs = R.load(name)
    got = robots[name].mjacs(dev(runs["mjacs__q"].astype(np.float32)), 5.0).cpu().numpy()
    want = runs["mjacs__mjacs"]
    assert got.shape == want.shape and got.dtype == want.dtype
    print(f"{name}: mjacs differ by {np.abs(got.astype(np.float64) - want).max():.3e}")
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", R.ROBOTS)
def test_joint_limit_mask_of_the_fused_launch(robots, name):
    """joint_limit_almost_violations_3d (cppflow/search.py:25-52) through the fused launch's jlim_mask, on configurations ON a padded
    limit and one ulp either side.  The launch reports the masks of its OUTPUT, so it is run with the early-out on targets that are
    the kernel's own FK of these configurations: every row is converged on entry and comes back untouched (asserted)."""
    rb, runs = robots[name], R.load(name)
    qs, want = runs["jl__qs"], runs["jl__violations"]
    x = dev(qs.reshape(-1, rb.ndof))
    eps_r, eps_p = (float(v) for v in runs["jl__eps"])
    rb.set_joint_limit_padding(eps_r, eps_p)
    try:
        inside = ((x >= dev(H.chain(name).lo)) & (x <= dev(H.chain(name).hi))).all(dim=1)
        xi = x[inside].contiguous()
        res = rb.lm_pose_steps(xi, rb.forward_kinematics(xi), 1e-6, 3.5, 0.35, n_steps=1, want_collisions=True, tol_pos_m=1e-3,
                               tol_rot_rad=1e-2)  # fmt: skip
        assert torch.equal(res["x"], xi)
        assert np.array_equal(res["jlim_mask"].cpu().numpy().astype(np.float32), want.reshape(-1)[inside.cpu().numpy()])
        assert int(inside.sum()) >= 6 * rb.ndof  # every on-the-limit row is inside the limits proper
        m = rb.collision_masks(x.reshape(qs.shape), only=("jlim",))  # the rows past the limits too
        assert np.array_equal(m["jlim_mask"].cpu().numpy().astype(np.float32), want)
    finally:
        rb.set_joint_limit_padding(None, None)


# ---- the coupled step ------------------------------------------------------------------------------------------------------------------
def _step_case(runs, family):
    c = R.section(runs, f"step_{family}")
    S, T, d = c["x"].shape
    x = c["x"].astype(np.float64).reshape(S * T, d)
    xv = c["virtual_configs"].astype(np.float64).reshape(S * T, d) if "virtual_configs" in c else None
    return c, S, T, d, x, xv


@pytest.mark.parametrize("family", R.STEP_FAMILIES)
@pytest.mark.parametrize("name", R.ROBOTS)
def test_lm_full_step_in_every_elimination_form(robots, name, family):
    """cppf_lm_full_step (parallel cyclic reduction, two-ended row-per-lane elimination, one wavefront per trajectory) against the x_new
    the reference's get_r_and_J + _lm_full_step returned for the three trajectories of every option family, at 2e-4 + 2e-3 * step.

    The two families that have the pose block and nothing else (pose_plain, pose_scale) are what this test found wrong: with six pose
    rows per waypoint and seven or eight joints, J^T J + 1e-6 I has d - 6 eigenvalues equal to lambda; J^T r has no component along
    them in exact arithmetic, an fp32 one has 6e-8 |J| |r|, and the solve divides it by 1e-6.  The fp32 eliminations missed the bar
    there on all three robots (worst |x_new - reference| 2.7e-3 .. 7.2e-3 at steps 3e-2 .. 1.2e-1, bars 2.6e-4 .. 4.5e-4).  No row
    couples the waypoints in that configuration, so it now takes no elimination at all: the lane that builds a waypoint's block
    accumulates it in fp64 and solves it (full_local_solve, kernels_coupled.h), whatever the debug switches say -- 2e-7 .. 1.4e-6."""
    rb, runs = robots[name], R.load(name)
    c, S, T, d, x, xv = _step_case(runs, family)
    pm = R.project_params(c["params"], dev(xv) if xv is not None else None)
    cons = R.project_constraints(runs["step__constraints"])
    rb.set_obstacles(*_obstacle_lists(c["obstacles"]))
    want = c["x_new"].reshape(S * T, d)
    step = np.abs(want - x).max()
    errs = {}
    try:
        for mode, (pcr, rows) in {"pcr": (1 << 30, 1), "rows": (0, 1), "wave": (0, 0)}.items():
            rb.debug_set("pcr_max_rows", pcr)
            rb.debug_set("full_rows", rows)
            got = host(rb.lm_full_step(dev(x), dev(c["target"]), pm, virtual_configs=dev(xv) if xv is not None else None, constraints=cons))
            errs[mode] = np.abs(got - want).max() if np.isfinite(got).all() else np.inf
            print(f"{name} {family} {mode}: x_new differs by {errs[mode]:.3e}, step {step:.3e}, bar {2e-4 + 2e-3 * step:.3e}")
    finally:
        rb.debug_set("pcr_max_rows", -1)
        rb.debug_set("full_rows", 1)
        rb.set_obstacles([], [])
    for mode, err in errs.items():
        assert err < 2e-4 + 2e-3 * step, (mode, err, step)


# bars of test_dense_residual_and_jacobian_reproduce_the_device_step (r of the differencing, virtual-config and collision rows: 2e-7)
# and of the per-row quantities the blocks are placed from, times the block's alpha: pose error and Jacobian 1e-5 (tests/test_gpu_parity.py;
# that test has no pose block, and an fp32 FK is 1e-6 m off before alpha_position = 3.5 multiplies it), distance Jacobians 2e-3
# (test_distance_jacobians_match_oracle)
R_BAR = 2e-7


@pytest.mark.parametrize("family", R.STEP_FAMILIES)
@pytest.mark.parametrize("name", R.ROBOTS)
def test_port_residual_and_jacobian_blocks(robots, name, family):
    """cppflow_amd.optimization_utils.LmResidualFns.get_r_and_J on the GPU robot: every block of r and J, the invalid-row sets and the
    filtered shapes against the reference's"""
    from cppflow_amd.optimization_utils import LmResidualFns

    rb, runs = robots[name], R.load(name)
    c, S, T, d, x, xv = _step_case(runs, family)
    cons = R.project_constraints(runs["step__constraints"])
    cuboids, Tcuboids = _obstacle_lists(c["obstacles"])
    rb.set_obstacles(cuboids, Tcuboids)
    try:
        for s in range(S):
            xs = dev(x[s * T : (s + 1) * T])
            pm = R.project_params(c["params"], dev(xv[s * T : (s + 1) * T]) if xv is not None else None)
            jac, res = LmResidualFns.get_r_and_J(pm, rb, xs, dev(c["target"]), Tcuboids=[torch.tensor(t) for t in Tcuboids],
                                                 cuboids=[torch.tensor(b) for b in cuboids], constraints=cons)  # fmt: skip
            for bi, b in enumerate(R.BLOCKS):
                r_b, J_b = getattr(res, b), getattr(jac, b)
                if not c["blocks_present"][s, bi]:
                    assert r_b is None or r_b.numel() == 0, (s, b)
                    continue
                want_r, want_J = c[f"s{s}__r_{b}"], c[f"s{s}__J_{b}"].astype(np.float64)
                assert tuple(r_b.shape) == want_r.shape and tuple(J_b.shape) == want_J.shape, (s, b, tuple(r_b.shape), want_r.shape)
                alpha = {"pose": max(pm.alpha_position or 0, pm.alpha_rotation or 0), "differencing": 1.0, "virtual_configs": 1.0,
                         "self_collisions": pm.alpha_self_collision, "env_collisions": pm.alpha_env_collision}[b]  # fmt: skip
                j_bar = {"pose": 1e-5, "differencing": 1e-6, "virtual_configs": 1e-6, "self_collisions": 2e-3, "env_collisions": 2e-3}[b] * alpha
                r_bar = 1e-5 * alpha if b == "pose" else R_BAR
                er, eJ = np.abs(host(r_b) - want_r).max(), np.abs(host(J_b) - want_J).max()
                print(f"{name} {family} s{s} {b}: r differs by {er:.3e} (bar {r_bar:.1e}), J by {eJ:.3e} (bar {j_bar:.1e})")
                assert er < r_bar and eJ < j_bar, (s, b, er, eJ)
            for b in ("pose", "differencing"):
                key = f"s{s}__{b}_invalid_row_idxs"
                inv = getattr(res, f"{b}_invalid_row_idxs")
                assert (inv is not None) == (key in c), (s, b)
                if inv is not None:
                    assert np.array_equal(inv.cpu().numpy().astype(bool), c[key]), (s, b)
    finally:
        rb.set_obstacles([], [])


# ---- the pose step, pose errors, clamp ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["row", "quad"])
@pytest.mark.parametrize("name", R.ROBOTS)
def test_one_pose_step(robots, name, shape):
    """lm_pose_steps(n_steps=1) in both kernel shapes against levenberg_marquardt_only_pose (cppflow/optimization.py:61-92), at the bars
    of test_single_lm_step_matches_reference_order_oracle"""
    c = R.section(R.load(name), "pose")
    lm = dict(zip(("lm_lambda", "alpha_position", "alpha_rotation"), (float(v) for v in c["lm"])))
    row = shape == "row"  # (the four-lanes-per-row shape has no J / e outputs: its x alone)
    res = robots[name].lm_pose_steps(dev(c["x"]), dev(c["target"]), n_steps=1, clamp=False, return_residual=row,
                                     shape=_hip.SHAPE_ROW if row else _hip.SHAPE_QUAD, **lm)  # fmt: skip
    if row:
        assert np.abs(host(res["J"]) - c["J_scaled"]).max() < 1e-5
        assert np.abs(host(res["e"])[:, :, 0] - c["e_scaled"]).max() < 1e-5
    ok = np.linalg.svd(c["J_scaled"], compute_uv=False)[:, -1] >= 2e-2
    assert ok.mean() > 0.85
    assert np.isfinite(host(res["x"])).all() and np.abs(host(res["x"]) - c["x_new"])[ok].max() < 5e-3


@pytest.mark.parametrize("name", R.ROBOTS)
def test_pose_errors_and_clamp(robots, name):
    """get_6d_pose_errors and clamp_to_joint_limits (cppflow/optimization_utils.py:802-833) at the bars of tests/test_gpu_parity.py:
    1e-5 (rad, m), 2e-6 m for the current position, the clamp bit for bit"""
    from cppflow_amd.optimization_utils import clamp_to_joint_limits, get_6d_pose_errors

    rb, runs = robots[name], R.load(name)
    c = R.section(runs, "pose")
    e, cur = get_6d_pose_errors(rb, dev(c["x"]), dev(c["target"]))
    assert np.abs(host(e)[:, :, 0] - c["errors"]).max() < 1e-5
    assert np.abs(host(cur)[:, :3] - c["current_poses"][:, :3]).max() < 2e-6
    k = R.section(runs, "clamp")
    x = dev(k["x"])
    assert clamp_to_joint_limits(rb, x) is x and np.array_equal(x.cpu().numpy(), k["clamped"])


# ---- evaluation ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.ROBOTS)
def test_plan_metrics_seed_selection_and_validity(robots, name):
    """plan_metrics, seed_summary + select_valid_seed and x_is_valid against the reference's evaluation_utils, Plan properties and
    x_is_valid (cppflow/evaluation_utils.py, data_types.py:140-264, optimization_utils.py:836-923): numeric fields at the bars of
    test_plan_metrics_match_oracle, verdicts equal on every path and for every stacking of paths as parallel seeds"""
    from cppflow_amd.data_type_utils import problem_from_arrays
    from cppflow_amd.optimization_utils import x_is_valid

    rb, runs = robots[name], R.load(name)
    c = R.section(runs, "eval")
    paths, target = c["paths"], c["target"]
    n, W, d = paths.shape
    cons = R.project_constraints(c["constraints"])
    plan = c["plan"]
    problem = problem_from_arrays(rb, target, [tuple(o) for o in c["obstacles"]], constraints=cons, device=DEV)
    try:
        x = dev(paths.reshape(n * W, d))
        masks = problem.collision_masks(x.view(n, W, d), only=("self", "env"))
        assert np.array_equal(masks["self_mask"].cpu().numpy().astype(bool), c["batched_self"])
        assert np.array_equal(masks["env_mask"].cpu().numpy().astype(bool), c["batched_env"])
        got = host(rb.plan_metrics(x, dev(target), masks["self_mask"].view(-1), masks["env_mask"].view(-1)))
        np.testing.assert_allclose(got[:, [0, 1]], plan[:, [0, 1]], rtol=2e-3, atol=2e-4)
        np.testing.assert_allclose(got[:, [2, 3]], plan[:, [2, 3]], rtol=2e-3, atol=2.6e-2)
        np.testing.assert_allclose(got[:, 4:8], plan[:, 4:8], rtol=1e-5, atol=1e-5)
        assert np.array_equal(got[:, 8:11], plan[:, 8:11])
        np.testing.assert_allclose(got[:, 4], c["mjac_deg"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(got[:, [4, 5]], c["get_mjacs"], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(got[:, 0], c["pos_err_cm"].max(axis=1), rtol=2e-3, atol=2e-4)
        np.testing.assert_allclose(got[:, 2], c["rot_err_deg"].max(axis=1), rtol=2e-3, atol=2.6e-2)
        # each path alone, then the recorded stackings: the verdict, the seed chosen, the six flags of the last seed examined
        for i in range(n):
            x_i, idx, flags = x_is_valid(problem, cons, dev(target), dev(paths[i]), parallel_count=1)
            assert (x_i is not None) == bool(c["valid_alone"][i]) == bool(plan[i, 12]), i
            assert [-1 if f is None else int(bool(f)) for f in flags] == c["flags_alone"][i].tolist(), i
        # the fused launch's per-seed summary (early-out on, tolerances wide open: every row comes back untouched) and the device's choice
        packed = torch.empty(rb.PACKED_BYTES_PER_ROW * n * W, dtype=torch.uint8, device=DEV)
        for order, first, flags_want in zip(c["orders"], c["first_valid"], c["flags"]):
            order = [int(o) for o in order if o >= 0]
            xs = dev(np.concatenate([paths[i] for i in order]))
            x_i, idx, flags = x_is_valid(problem, cons, dev(target), xs, parallel_count=len(order))
            assert (-1 if idx is None else idx) == int(first), order
            assert [-1 if f is None else int(bool(f)) for f in flags] == flags_want.tolist(), order
            pk = packed[: rb.PACKED_BYTES_PER_ROW * len(order) * W]
            r = rb.lm_pose_steps(xs, dev(target), 1e-6, 3.5, 0.35, n_steps=1, packed_out=pk, tol_pos_m=10.0, tol_rot_rad=4.0)
            assert torch.equal(r["x"], xs)
            chosen = rb.select_valid_seed(rb.seed_summary(r["x"], pk, len(order), W), cons).cpu().numpy()
            assert int(chosen[0]) == int(first), order
    finally:
        rb.set_obstacles([], [])
