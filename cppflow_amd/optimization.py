"""The LM optimiser surface of the reference (`cppflow/optimization.py`): dataclasses (`:26-57`), the batched pose-only
step (`:61-92`), the loop (`:147-373`) and the entry point (`:376-426`).

What runs where
  * `levenberg_marquardt_only_pose` = ONE launch of the fused kernel with K = 1 and no clamp (x_new, and J / e scaled
    exactly as the reference returns them when `return_residual=True`).
  * `levenberg_marquardt_full` = the coupled step (`:95-144`) as a block-tridiagonal solve per trajectory on the device
    (`cppf_lm_full_step`), for any number of seeds.
  * `run_lm_alternating_loss` keeps the reference's Python control flow (alternation rule, TL convergence, termination)
    around those launches.
  * `run_lm_pose_refinement` is the batched form the MI355X path is built for: all S seeds x W waypoints, K fused
    iterations, per-seed validity and collision masks / search cost in the same launch.
"""

import warnings
from dataclasses import dataclass
from time import time
from typing import Dict, Optional

import torch

from cppflow_amd.config import ENV_COLLISIONS_IGNORED, SELF_COLLISIONS_IGNORED
from cppflow_amd.data_types import Constraints, Problem
from cppflow_amd.lm_hyper_parameters import ALT_LOSS_V2_1_DIFF, ALT_LOSS_V2_1_POSE, OptimizationParameters
from cppflow_amd.scene import DEFAULT_SCENE_ACTIVATION_DISTANCE_M
from cppflow_amd.optimization_utils import LmResidualFns, clamp_to_joint_limits, evaluate_seeds, x_is_valid
from cppflow_amd.utils import make_text_green_or_red


@dataclass
class OptimizationProblem:
    problem: Problem
    constraints: Constraints
    seed: torch.Tensor
    target_path: torch.Tensor
    verbosity: int
    parallel_count: int
    results_df: Optional[Dict]
    # _hip.PIN_FIRST | _hip.PIN_LAST: waypoint 0 / W-1 of every trajectory is a constant of the optimisation (its value: the seed's)
    pin_mask: int = 0

    @property
    def robot(self):
        return self.problem.robot

    @property
    def n_timesteps(self) -> int:
        return self.problem.n_timesteps


@dataclass
class OptimizationState:
    x: torch.Tensor
    n_steps: int
    t0: float


@dataclass
class OptimizationResult:
    x_opt: torch.Tensor
    n_steps_taken: int
    is_valid: bool
    parallel_seed_idx: int
    # device_loop=True only: per loop-control record, one (step taken "pose" / "diff", TL, the six x_is_valid flags or None, valid or
    # None) per iteration decided -- what the device wrote down, for comparing decision by decision; and the records themselves
    trace: Optional[list] = None
    records: Optional[list] = None
    # problems with more than 8 cuboids only (run_lm_optimization): how often the active set was selected (1, or 2 after a
    # re-selection) and the cuboid indices the last run's kernels were given; 0 / None otherwise
    scene_selection_rounds: int = 0
    active_obstacles: Optional[list] = None


def _unstacked_target(opt_problem: OptimizationProblem) -> torch.Tensor:
    """The kernels index target[row % W]; the reference's stacked [k*W, 7] tensor is just W rows repeated."""
    W = opt_problem.n_timesteps
    t = opt_problem.target_path
    return t if t.shape[0] == W else t[:W]


def levenberg_marquardt_only_pose(
    opt_problem: OptimizationProblem,
    opt_state: OptimizationState,
    opt_params: OptimizationParameters,
    return_residual: bool = False,
):
    """One batched pose-only LM step: `x + (J^T J + lambda I)^-1 J^T e` with rows of J / e scaled by alpha_rotation
    (rows 0:3) and alpha_position (rows 3:6).  Returns x_new, or (x_new, J [n,6,d], e [n,6,1]) -- J and e scaled, as the
    reference returns them (cppflow/optimization.py:77-80, 90-92)."""
    n, ndof = opt_state.x.shape
    assert ndof == opt_problem.robot.ndof
    assert opt_problem.target_path.shape[0] in (n, opt_problem.n_timesteps), "target_path must be [n,7] or [W,7]"
    res = opt_problem.robot.lm_pose_steps(
        opt_state.x,
        _unstacked_target(opt_problem),
        lm_lambda=opt_params.lm_lambda,
        alpha_position=opt_params.alpha_position,
        alpha_rotation=opt_params.alpha_rotation,
        n_steps=1,
        clamp=False,
        return_residual=return_residual,
    )
    if return_residual:
        return res["x"], res["J"], res["e"]
    return res["x"]


def levenberg_marquardt_full(
    opt_problem: OptimizationProblem,
    opt_state: OptimizationState,
    opt_params: OptimizationParameters,
    return_residual: bool = False,
    scene_in_step: bool = False,
):
    """The coupled LM step (cppflow/optimization.py:116-144): pose / differencing / virtual-config / capsule-collision
    residuals of whole trajectories, solved as a block-tridiagonal system per trajectory on the device
    (`cppf_lm_full_step`).  Unlike the reference (`assert parallel_count == 1`, :128) any number of seeds is accepted:
    opt_state.x is [parallel_count * W, ndof] and every trajectory is smoothed independently in the same launch.
    `scene_in_step`: the environment rows come from every cuboid of the problem's scene in device memory
    (`cppf_lm_full_step_scene`) instead of what `bind_obstacles` hands the robot handle."""
    scene = None
    if scene_in_step:  # every cuboid of the scene, from device memory: the handle's own are not involved
        sc = opt_problem.problem.scene(opt_state.x.device)
        scene = (sc.lo, sc.hi)
    else:
        opt_problem.problem.bind_obstacles()
    x_new = opt_problem.robot.lm_full_step(
        opt_state.x, _unstacked_target(opt_problem), opt_params, virtual_configs=opt_params.virtual_configs,
        pin=opt_problem.pin_mask, scene=scene,
    )  # fmt: skip
    if not return_residual:
        return x_new
    assert not scene_in_step, "the dense residual / Jacobian take the handle's cuboids"
    # inspection path: the dense (J, r) the reference would have factored (the step above never forms them)
    assert opt_problem.parallel_count == 1, "the dense residual / Jacobian are defined for one trajectory (:128)"
    jacobian, residual = LmResidualFns.get_r_and_J(
        opt_params, opt_problem.robot, opt_state.x, _unstacked_target(opt_problem),
        Tcuboids=opt_problem.problem.obstacles_Tcuboids, cuboids=opt_problem.problem.obstacles_cuboids,
    )  # fmt: skip
    return x_new, jacobian, residual


def run_lm_alternating_loss(
    opt_problem: OptimizationProblem,
    opt_state: OptimizationState,
    params_diff: OptimizationParameters,
    params_pose: OptimizationParameters,
    return_residuals: bool,
    tmax_sec: Optional[float],
    max_n_steps: Optional[int],
    return_if_valid_after_n_steps: Optional[int],
    convergence_threshold: float,
    verbosity: int = 0,
    save_images: bool = False,
    results_df: Optional[Dict] = None,
    on_pose_valid: str = "differencing",
    device_loop: bool = False,
    sync_every: Optional[int] = None,
    per_trajectory: bool = False,
    scene_in_step: bool = False,
):
    """The alternating loop of cppflow/optimization.py:147-373 with its bookkeeping and termination rules.

    Per iteration: if both pose flags are valid take the coupled differencing step (virtual configs := current x, :253),
    else a pose-only step; clamp; evaluate `x_is_valid`; TL-convergence (:275-297) and termination (:326-358) as in the
    reference.  `on_pose_valid` = "stop" / "continue" replace the differencing branch by stopping / more pose steps.

    `device_loop=True`: the same loop with the decision taken on the device (`cppf_lm_optimize_enqueue`): `sync_every` iterations
    are enqueued at a time (default: all `max_n_steps` without a time limit, DEVICE_LOOP_TIMED_CHUNK with one) and the loop-control
    block is copied back once per chunk -- ONE device-to-host copy per chunk instead of one per iteration.  Iterations enqueued
    after the loop has ended are gated off on the device.  `tmax_sec` is checked between chunks only: the time limit has chunk
    granularity in this mode (the last valid trajectory is still what comes back).  `per_trajectory=True` (device loop only): every
    one of the `parallel_count` trajectories alternates and terminates by its OWN flags (a finished one is gated off) instead of
    all following one decision; the result is the lowest-index valid trajectory (`parallel_seed_idx`), `x_opt` holds every
    trajectory's own result.

    `scene_in_step` (host loop only; `run_lm_optimization` decides it): every coupled step reads the problem's whole scene
    (`levenberg_marquardt_full(scene_in_step=True)`); nothing is bound to the robot handle for the environment.

    `opt_problem.pin_mask` (`run_lm_optimization(pin_first=..., pin_last=...)`): the named end waypoints of every trajectory are
    constants of the optimisation.  The coupled step takes them as boundary conditions (`cppf_lm_full_step_pinned`); the pose step
    is the unchanged kernel and its result for those rows is discarded -- here they are put back after the clamp, on the device
    the clamp (the loop's only writer of x) skips them.  Validity, masks and metrics see the whole path, pinned rows included."""
    assert not return_residuals and not save_images and results_df is None, "debug outputs are not supported"
    assert on_pose_valid in ("differencing", "stop", "continue")
    assert device_loop or (sync_every is None and not per_trajectory), "sync_every / per_trajectory belong to device_loop=True"
    assert sync_every is None or (isinstance(sync_every, int) and sync_every >= 1), "sync_every must be a positive int"
    assert not (device_loop and scene_in_step), "scene_in_step belongs to the host loop: the device loop's launches read the robot handle"
    if tmax_sec is None:
        assert (max_n_steps is not None) and (return_if_valid_after_n_steps is not None)
        assert return_if_valid_after_n_steps <= max_n_steps
    if max_n_steps is None:
        assert tmax_sec is not None
        max_n_steps = 10**6
    if device_loop:
        return _run_device_loop(opt_problem, opt_state, params_diff, params_pose, tmax_sec, max_n_steps,
                                return_if_valid_after_n_steps, convergence_threshold, on_pose_valid, sync_every, per_trajectory)
    robot = opt_problem.robot
    target = _unstacked_target(opt_problem)
    printc = print if verbosity > 1 else (lambda *a, **k: None)
    W = opt_problem.n_timesteps
    pinned_rows = _pinned_rows(opt_problem.pin_mask, opt_problem.parallel_count, W, opt_state.x.device)
    x_pinned = opt_state.x[pinned_rows].clone() if pinned_rows is not None else None
    # copies: the loop overwrites virtual_configs (the reference copies for the same reason, :184-187)
    params_diff = OptimizationParameters(**params_diff.__dict__)
    params_pose = OptimizationParameters(**params_pose.__dict__)

    tls_post_differencing = []
    last_valid, last_valid_idx, valid_seed_idx = None, -1, 0
    pose_pos_valid, pose_rot_valid = True, False  # the reference's initial values (:218-219): lead with a pose step
    converged = False
    t0 = time()
    i = -1
    for i in range(max_n_steps):
        took_differencing = False
        if pose_pos_valid and pose_rot_valid and on_pose_valid == "stop":
            printc("  pose is valid -- stopping (on_pose_valid='stop')")
            break
        if pose_pos_valid and pose_rot_valid and on_pose_valid == "differencing":
            printc(f"i: {i}  ----> differencing")
            params_diff.virtual_configs = opt_state.x.clone()  # :253
            # (the keyword only where it is set: the call without it is the one callers that substitute the step function know)
            scene_kw = {"scene_in_step": True} if scene_in_step else {}
            x_new = levenberg_marquardt_full(opt_problem, opt_state, params_diff, **scene_kw)
            took_differencing = True
        else:
            printc(f"i: {i}  --> only pose")
            x_new = levenberg_marquardt_only_pose(opt_problem, opt_state, params_pose)
        opt_state.x = clamp_to_joint_limits(robot, x_new)  # :259
        if pinned_rows is not None:
            opt_state.x[pinned_rows] = x_pinned  # (a copy: the same bits the seed held)
        opt_state.n_steps += 1

        # one evaluation of every trajectory per iteration: validity maxima, collision counts and the TL measure (the summed
        # revolute path length, :221-227) come back in a single [S,16] host tensor
        seed_metrics = evaluate_seeds(opt_problem.problem, target, opt_state.x, opt_problem.parallel_count)
        tl_new = float(seed_metrics[:, 6].sum())
        printc(f"  tl: {tl_new}")
        stop_now = False
        if took_differencing:  # :275-297
            if not converged and len(tls_post_differencing) > 0:
                diff = abs(tl_new - tls_post_differencing[-1])
                if diff < convergence_threshold:
                    converged = True
                    if last_valid_idx == i - 1:
                        stop_now = True
            tls_post_differencing.append(tl_new)
        if stop_now:
            break

        x_sol, seed_idx, flags = x_is_valid(
            opt_problem.problem, opt_problem.constraints, target, opt_state.x, opt_problem.parallel_count, verbosity=verbosity,
            seed_metrics=seed_metrics,
        )
        pose_pos_valid, pose_rot_valid = flags[0], flags[1]
        if x_sol is not None:
            last_valid_idx, last_valid, valid_seed_idx = i, opt_state.x.clone(), seed_idx
            if converged:
                printc(make_text_green_or_red("  x is valid and TL has converged, exiting", True))
                break
            printc(make_text_green_or_red("  x is valid, continuing", True))
        if tmax_sec is not None and time() - t0 > tmax_sec:
            if last_valid is not None:
                opt_state.x = last_valid.clone()
            break
        if last_valid is not None and return_if_valid_after_n_steps is not None and i > return_if_valid_after_n_steps:
            break
    x_return = last_valid if last_valid is not None else opt_state.x
    return OptimizationResult(
        x_opt=x_return, n_steps_taken=max(i, 0), is_valid=last_valid is not None, parallel_seed_idx=valid_seed_idx
    )


def _pinned_rows(pin_mask: int, S: int, W: int, device) -> Optional[torch.Tensor]:
    """Row indices of the pinned end waypoints of S stacked trajectories of W waypoints, or None without a pin."""
    from cppflow_amd import _hip

    assert 0 <= pin_mask <= (_hip.PIN_FIRST | _hip.PIN_LAST), pin_mask
    if pin_mask == 0:
        return None
    starts = torch.arange(S, device=device, dtype=torch.long) * W
    rows = ([starts] if pin_mask & _hip.PIN_FIRST else []) + ([starts + (W - 1)] if pin_mask & _hip.PIN_LAST else [])
    return torch.unique(torch.cat(rows))


DEVICE_LOOP_TIMED_CHUNK = 4  # iterations enqueued between two looks at the clock when the device loop runs under a time limit
DEVICE_LOOP_TRACE_CAPACITY = 4096  # iterations whose decision the device writes down (an anytime run may take more; those are not traced)


def _run_device_loop(opt_problem, opt_state, params_diff, params_pose, tmax_sec, max_n_steps, return_if_valid_after_n_steps,
                     convergence_threshold, on_pose_valid, sync_every, per_trajectory) -> OptimizationResult:
    """`run_lm_alternating_loss(device_loop=True)`: enqueue chunks of gated iterations, copy the loop-control block back once per
    chunk, assemble the result the host loop would return."""
    import numpy as np

    from cppflow_amd import _hip

    robot, problem = opt_problem.robot, opt_problem.problem
    target = _unstacked_target(opt_problem)
    W, S = opt_problem.n_timesteps, opt_problem.parallel_count
    x = opt_state.x
    assert x.shape == (S * W, robot.ndof) and x.is_contiguous(), tuple(x.shape)
    if max_n_steps == 0:
        return OptimizationResult(x_opt=x, n_steps_taken=0, is_valid=False, parallel_seed_idx=0, trace=[], records=[])
    problem.bind_obstacles()
    c = opt_problem.constraints
    prm = _hip.OptloopParams()
    prm.pose_lm_lambda, prm.pose_alpha_position = float(params_pose.lm_lambda), float(params_pose.alpha_position)
    prm.pose_alpha_rotation = float(params_pose.alpha_rotation)
    prm.diff = robot.full_params(params_diff)
    prm.constraints = _hip.Constraints(c.max_allowed_position_error_cm, c.max_allowed_rotation_error_deg, c.max_allowed_mjac_deg,
                                       c.max_allowed_mjac_cm, int(bool(SELF_COLLISIONS_IGNORED)), int(bool(ENV_COLLISIONS_IGNORED)))  # fmt: skip
    prm.max_n_steps = int(max_n_steps)
    prm.return_if_valid_after_n_steps = -1 if return_if_valid_after_n_steps is None else min(int(return_if_valid_after_n_steps), 2**31 - 1)
    prm.on_pose_valid = _hip.OPT_ON_POSE_VALID[on_pose_valid]
    prm.per_trajectory = int(bool(per_trajectory))
    prm.trace_capacity = min(int(max_n_steps), DEVICE_LOOP_TRACE_CAPACITY)
    prm.convergence_threshold = float(convergence_threshold)
    C = S if per_trajectory else 1
    workspace, control = robot.lm_optimize_buffers(S, W, prm, x.device)
    chunk = sync_every if sync_every is not None else (max_n_steps if tmax_sec is None else DEVICE_LOOP_TIMED_CHUNK)
    t0 = time()
    enqueued = 0
    while True:
        k = min(chunk, max_n_steps - enqueued)
        robot.lm_optimize_enqueue(x, target, prm, workspace, control, k, pin=opt_problem.pin_mask)
        enqueued += k
        host = control.cpu().numpy()  # the one device-to-host copy of this chunk
        rec = host[: C * 16].reshape(C, 16)
        if bool((rec[:, 0] == _hip.OPT_MODE_DONE).all()) or enqueued >= max_n_steps:
            break
        if tmax_sec is not None and time() - t0 > tmax_sec:
            break  # (optimization.py: the last valid trajectory comes back, as below)
    opt_state.n_steps += int(rec[:, 5].max())
    done = rec[:, 0] == _hip.OPT_MODE_DONE
    i_final = np.where(done, rec[:, 10], rec[:, 5] - 1)
    valid = rec[:, 8] != 0
    snapshot = workspace[: S * W * robot.ndof].view(S * W, robot.ndof)
    if not per_trajectory:
        x_opt = snapshot.clone() if valid[0] else x
        seed_idx = int(rec[0, 9])
    else:
        x_opt = x.clone()
        for s in np.nonzero(valid)[0]:
            x_opt[s * W : (s + 1) * W] = snapshot[s * W : (s + 1) * W]
        seed_idx = int(np.nonzero(valid)[0][0]) if valid.any() else 0
    tr = host[C * 16 :].reshape(C, prm.trace_capacity, 4)
    names = {_hip.OPT_MODE_POSE: "pose", _hip.OPT_MODE_DIFF: "diff"}
    trace = [
        [(names[int(r[0])], float(r[1:2].view(np.float32)[0]), _hip.optloop_flags(int(r[2])), None if r[3] < 0 else bool(r[3]))
         for r in tr[ci, : min(int(rec[ci, 5]), prm.trace_capacity)]]
        for ci in range(C)
    ]  # fmt: skip
    records = [_hip.OptloopRecord.from_buffer_copy(rec[ci].tobytes()) for ci in range(C)]
    return OptimizationResult(x_opt=x_opt, n_steps_taken=max(int(i_final.max()), 0), is_valid=bool(valid.any()),
                              parallel_seed_idx=seed_idx, trace=trace, records=records)  # fmt: skip


def run_lm_optimization(
    problem: Problem,
    x_seed: torch.Tensor,
    tmax_sec: Optional[float],
    max_n_steps: int,
    return_if_valid_after_n_steps: int,
    convergence_threshold: float,
    parallel_count: int = 1,
    results_df: Optional[Dict] = None,
    verbosity: int = 1,
    on_pose_valid: str = "differencing",
    device_loop: bool = False,
    sync_every: Optional[int] = None,
    per_trajectory: bool = False,
    pin_first: bool = False,
    pin_last: bool = False,
    scene_activation_distance_m: float = DEFAULT_SCENE_ACTIVATION_DISTANCE_M,
    scene_in_step: bool = False,
) -> OptimizationResult:
    """Optimise a trajectory (or `parallel_count` seeds at once): x_seed is [parallel_count * W, ndof]
    (cppflow/optimization.py:376-426).  The target path is NOT stacked: rows index it modulo W.
    `device_loop` / `sync_every` / `per_trajectory`: see `run_lm_alternating_loss`.
    `pin_first` / `pin_last`: waypoint 0 / W-1 of EVERY trajectory is held at its value in `x_seed` (`x_opt` carries those rows
    bit for bit) -- a start the robot stands at, a goal configuration that is given.  Any combination is served.
    A problem with more than 8 cuboids: the kernels of the loop take the <= 8 cuboids that come within
    `scene_activation_distance_m` of the seed path (`Problem.choose_active_obstacles`); the result is re-evaluated against the
    whole scene, and if it hits a cuboid outside the active set the set is re-selected ONCE -- the cuboids hit first, then by
    distance to the result -- and the loop runs again from the seed within what is left of `tmax_sec`.  `is_valid` always speaks
    for the whole scene: the host loop evaluates every iteration against it, the device loop decides on the active set and is
    re-validated here (the trajectory it chose is the one that is checked).  `scene_selection_rounds` / `active_obstacles` of
    the result say what happened.
    `scene_in_step=True` (host loop only): for such a problem the coupled step reads EVERY cuboid of the scene from device memory
    (`Robot.lm_full_step(scene=...)`, `cppf_lm_full_step_scene`) -- no active set is chosen, nothing is bound to the handle for the
    environment and nothing is re-selected (`scene_selection_rounds` = 0, `active_obstacles` = None); the per-iteration evaluation
    is the whole scene's as before.  On a problem of at most 8 cuboids the host loop runs exactly as without the flag.  Together
    with `device_loop=True` the flag is refused (AssertionError) whatever the problem holds: the combination is a mistake of the
    caller's, and it is reported the same way for every problem (`Planner` refuses it at construction)."""
    # (first of all, before anything touches the device: the device loop's gated launches read the handle, not a scene)
    assert not (device_loop and scene_in_step), (
        "scene_in_step=True is not combined with device_loop=True: the device loop's gated mask and step launches take their "
        "cuboids from the robot handle"
    )
    if SELF_COLLISIONS_IGNORED:
        warnings.warn("robot-robot are collisions will be ignored during LM optimization")
    if ENV_COLLISIONS_IGNORED:
        warnings.warn("environment-robot collisions will be ignored during LM optimization")
    assert problem.target_path.shape == (problem.n_timesteps, 7)
    assert problem.n_timesteps * parallel_count == x_seed.shape[0]
    assert x_seed.shape[1] == problem.robot.ndof
    assert isinstance(max_n_steps, int), f"error: max_n_steps must be int, is {type(max_n_steps)}"
    from cppflow_amd import _hip

    opt_problem = OptimizationProblem(
        problem, problem.constraints, x_seed, problem.target_path, verbosity, parallel_count, results_df,
        pin_mask=(_hip.PIN_FIRST if pin_first else 0) | (_hip.PIN_LAST if pin_last else 0),
    )  # fmt: skip
    scene_in_step = bool(scene_in_step) and problem.uses_scene

    def run(tmax) -> OptimizationResult:
        opt_state = OptimizationState(x_seed.clone(), 0, time())
        return run_lm_alternating_loss(
            opt_problem, opt_state, ALT_LOSS_V2_1_DIFF, ALT_LOSS_V2_1_POSE, return_residuals=False, verbosity=verbosity,
            tmax_sec=tmax, max_n_steps=max_n_steps, return_if_valid_after_n_steps=return_if_valid_after_n_steps,
            convergence_threshold=convergence_threshold, save_images=False, results_df=results_df, on_pose_valid=on_pose_valid,
            device_loop=device_loop, sync_every=sync_every, per_trajectory=per_trajectory, scene_in_step=scene_in_step,
        )  # fmt: skip

    if not problem.uses_scene:
        return run(tmax_sec)
    if scene_in_step:  # (is_valid: the host loop evaluated every iteration against the whole scene)
        return run(tmax_sec)

    W, t_start = problem.n_timesteps, time()
    reach = float(scene_activation_distance_m)
    problem.choose_active_obstacles(x_seed.view(parallel_count, W, -1), reach)
    rounds = 1
    while True:
        res = run(tmax_sec)
        # the whole scene's verdict on what came back: the trajectory the loop chose (all of them when it chose none)
        s = res.parallel_seed_idx if 0 <= res.parallel_seed_idx < parallel_count else 0
        x_chk = res.x_opt[s * W : (s + 1) * W] if res.is_valid else res.x_opt
        sc = problem.scene_collisions(x_chk.contiguous(), reach)
        hit = sorted(set(sc["nearest_obs"][sc["env_mask"]].cpu().tolist()))
        res.is_valid = bool(res.is_valid and len(hit) == 0)
        new = [o for o in hit if o not in problem.active_obstacles]
        out_of_time = tmax_sec is not None and time() - t_start > tmax_sec
        if not new or rounds >= 2 or out_of_time:
            break
        from cppflow_amd.robot_model import MAX_OBSTACLES
        from cppflow_amd.scene import select_active_obstacles

        problem.active_obstacles = select_active_obstacles(sc["obs_min"], MAX_OBSTACLES, first=new)
        rounds += 1
        if tmax_sec is not None:
            tmax_sec = tmax_sec - (time() - t_start)
            t_start = time()
    res.scene_selection_rounds, res.active_obstacles = rounds, list(problem.active_obstacles)
    return res


@dataclass
class PoseRefinementResult:
    x: torch.Tensor  # [S*W, d]
    pos_err_m: torch.Tensor  # [S, W]
    rot_err_rad: torch.Tensor  # [S, W]
    self_mask: torch.Tensor  # bool [S, W]
    env_mask: torch.Tensor  # bool [S, W]
    jlim_mask: torch.Tensor  # bool [S, W]
    ext_cost: torch.Tensor  # float [S, W]: 100*jlim + 1000*env + 1000*self (cppflow/search.py:146-150)
    packed: torch.Tensor  # the uint8 buffer the six per-row outputs live in (what the all-gather ships)


def run_lm_pose_refinement(
    problem: Problem,
    x_seeds: torch.Tensor,
    n_steps: int,
    params_pose: OptimizationParameters = ALT_LOSS_V2_1_POSE,
    x_out: Optional[torch.Tensor] = None,
    packed_out: Optional[torch.Tensor] = None,
) -> PoseRefinementResult:
    """All seeds x waypoints through `n_steps` fused { pose step ; clamp } iterations in ONE launch, with pose errors,
    collision / joint-limit masks and the search cost of the result written to one packed buffer."""
    from cppflow_amd.search import DEFAULT_JLIM_SAFETY_PADDING_PRISMATIC, DEFAULT_JLIM_SAFETY_PADDING_REVOLUTE

    W = problem.n_timesteps
    assert x_seeds.dim() == 2 and x_seeds.shape[0] % W == 0, tuple(x_seeds.shape)
    S, n = x_seeds.shape[0] // W, x_seeds.shape[0]
    robot = problem.robot
    assert not problem.uses_scene, (
        f"{problem.n_obstacles} cuboids: run_lm_pose_refinement takes its obstacles from the robot handle (at most 8) in the fused launch's epilogue; "
        "problems with more than 8 cuboids are served by CppFlowPlanner / run_lm_optimization and Problem.collision_masks"
    )
    problem.bind_obstacles()
    robot.set_joint_limit_padding(DEFAULT_JLIM_SAFETY_PADDING_REVOLUTE, DEFAULT_JLIM_SAFETY_PADDING_PRISMATIC)
    if packed_out is None:
        packed_out = torch.empty(robot.PACKED_BYTES_PER_ROW * n, dtype=torch.uint8, device=x_seeds.device)
    r = robot.lm_pose_steps(
        x_seeds, problem.target_path, params_pose.lm_lambda, params_pose.alpha_position, params_pose.alpha_rotation,
        n_steps=n_steps, clamp=True, x_out=x_out, packed_out=packed_out,
    )  # fmt: skip
    return PoseRefinementResult(
        x=r["x"], pos_err_m=r["pos_err_m"].view(S, W), rot_err_rad=r["rot_err_rad"].view(S, W),
        self_mask=r["self_mask"].view(S, W).view(torch.bool), env_mask=r["env_mask"].view(S, W).view(torch.bool),
        jlim_mask=r["jlim_mask"].view(S, W).view(torch.bool), ext_cost=r["ext_cost"].view(S, W), packed=packed_out,
    )  # fmt: skip
