"""Planner surface of the reference (`cppflow/planners.py`): `Planner` / `PlannerSearcher` / `CppFlowPlanner` with
`generate_plan(problem) -> PlannerResult`, wired to the device pipeline

    candidate q-paths [k,T,d]  ->  collision masks + search cost (one launch)  ->  dp_search (device)
                               ->  run_lm_optimization (fused LM launches + coupled differencing steps)

The reference draws its k candidate paths from IKFlow, a pretrained conditional normalizing flow (`planners.py:155-172`);
neither the package nor its weights exist here, so candidates come from a `seed_provider(problem, k) -> [k,T,d]` callable.
`LmIkSeedProvider` is a plain numerical stand-in built on this package's own LM kernel (random restarts at waypoint 0,
then warm-started tracking along the path): it is NOT IKFlow, only a way to exercise the pipeline end to end; anything
that returns a [k,T,d] tensor (an IKFlow wrapper included) can be dropped in.

Seed sharding.  When torch.distributed is initialised with more than one rank (one process per GPU), `_run_pipeline`
shards the k candidates: every rank asks its seed provider for k / world of them (the provider must return RANK-DISTINCT candidates:
`LmIkSeedProvider` offsets its generator by the rank), evaluates -- optionally refines, `candidate_lm_steps` -- its own, and
`cppflow_amd.distributed.sharded_candidate_evaluation` all-gathers the packed per-row outputs and the paths, so that every rank runs
the same `dp_search` over all k candidates (cppflow/planners.py:231-274, cppflow/search.py:146-151) and returns the same plan.
"""

from time import time
from typing import Callable, Dict, Optional, Tuple

import torch
import torch.distributed as dist

from cppflow_amd.collision_detection import qpaths_batched_collisions
from cppflow_amd.config import OPTIMIZATION_CONVERGENCE_THRESHOLD, SUCCESS_THRESHOLD_initial_q_norm_dist
from cppflow_amd.data_type_utils import plan_from_qpath
from cppflow_amd.data_types import PlannerResult, PlannerSettings, Problem, TimingData
from cppflow_amd.evaluation_utils import get_mjacs
from cppflow_amd.optimization import run_lm_optimization
from cppflow_amd.search import dp_search, dp_search_nbest

DEFAULT_RERUN_NEW_K = 125  # planners.py:47

SeedProvider = Callable[[Problem, int], torch.Tensor]


def add_search_path_mjac(debug_info: Dict, problem: Problem, qpath_search: torch.Tensor) -> None:
    """Diagnostics of the searched path the reference records (cppflow/planners.py:50-73): its maximum joint changes and its
    closest approach to a joint limit (cm for a leading prismatic joint, degrees for the rest) -- one min/max pass over
    [T, d] on the device, one copy back."""
    mjac_deg, mjac_cm = get_mjacs(problem.robot, qpath_search)
    debug_info["search_path_mjac-cm"], debug_info["search_path_mjac-deg"] = mjac_cm, mjac_deg
    limits = torch.tensor(problem.robot.actuated_joints_limits, dtype=qpath_search.dtype, device=qpath_search.device)  # [d, 2]
    margin = torch.minimum((qpath_search - limits[:, 0]).abs().min(dim=0).values,
                           (qpath_search - limits[:, 1]).abs().min(dim=0).values).cpu()  # fmt: skip
    lead_prismatic = problem.robot.has_prismatic_joints  # the reference treats joint 0 as THE prismatic joint (:60)
    debug_info["search_path_min_dist_to_jlim_cm"] = 100 * float(margin[0]) if lead_prismatic else -1
    rest = margin[1:] if lead_prismatic else margin
    debug_info["search_path_min_dist_to_jlim_deg"] = min(float(torch.rad2deg(rest.min())), 10000) if rest.numel() else 10000


def add_motion_certificate(debug_info: Dict, problem: Problem, qpath: torch.Tensor, level: int, depth: Optional[int] = None) -> None:
    """`Problem.motion_clearance` of the path [T, d] about to be returned -> debug_info: is every transition certified collision-free,
    and which transitions are hit / left undecided (indices t: the move from waypoint t to t + 1).  With `depth` the certificate is
    taken by adaptive bisection from `level` down to `depth`, and the deepest level any transition ended at and the mean number of
    interval tests per transition are reported as well."""
    mc = problem.motion_clearance(qpath.detach().contiguous(), level=level, resolve_depth=depth)
    if depth is not None:
        debug_info["motion_resolve_depth"] = int(mc.depth.max())
        debug_info["motion_tests_per_transition"] = float(mc.n_tested.to(torch.float64).mean())
    debug_info["motion_certified"] = bool(mc.all_certified[0])
    debug_info["motion_hit_transitions"] = torch.nonzero(mc.hit[0]).flatten().tolist()
    debug_info["motion_undecided_transitions"] = torch.nonzero(mc.undecided[0]).flatten().tolist()


class LmIkSeedProvider:
    """k candidate joint-space paths for a problem by numerical IK (stand-in for IKFlow, see module docstring)."""

    def __init__(self, seed: int = 0, damping: float = 1e-2, n_restart_steps: int = 40, n_track_steps: int = 6):
        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0  # rank-distinct candidates under sharding
        self._gen = torch.Generator().manual_seed(seed + 7919 * rank)
        self._damping, self._n_restart, self._n_track = damping, n_restart_steps, n_track_steps

    def __call__(self, problem: Problem, k: int) -> torch.Tensor:
        rb, dev = problem.robot, problem.target_path.device
        T, d = problem.n_timesteps, rb.ndof
        lo = torch.tensor([l for l, _ in rb.actuated_joints_limits], dtype=torch.float32)
        hi = torch.tensor([u for _, u in rb.actuated_joints_limits], dtype=torch.float32)
        q = (lo + (hi - lo) * (0.1 + 0.8 * torch.rand((k, d), generator=self._gen))).to(dev)
        out = torch.empty((k, T, d), dtype=torch.float32, device=dev)
        for t in range(T):
            tgt = problem.target_path[t : t + 1].contiguous()
            steps = self._n_restart if t == 0 else self._n_track
            q = rb.lm_pose_steps(q, tgt, self._damping, 3.5, 0.35, n_steps=steps, clamp=True)["x"]
            out[:, t] = q
        return out


class TrackingSeedProvider:
    """k candidate joint-space paths for a problem by tracking IK in ONE launch (`Robot.track_paths`, csrc/kernels_track.h): the same
    `(problem, k) -> [k,T,d]` contract as `LmIkSeedProvider`, without its per-waypoint loop of launches.  The path is cut into
    segments that every candidate tracks independently (one lane each); rows that miss the tolerances or jump by more than
    `max_jump_rad` / `max_jump_m` climb the recovery ladder (warm continuation, then `n_random_restarts` random restarts).

    Every call draws new candidates: a call counter goes into the kernel's hash (a planner's rerun, DEFAULT_RERUN_NEW_K, gets other
    candidates), and so does the rank of torch.distributed, read at call time (rank-distinct candidates under seed sharding).  With
    `problem.initial_configuration`, candidate 0 starts its first segment exactly there and the others from uniform perturbations of
    width `init_width` around it, clamped to the joint limits (the joint-space analogue of the reference's `_sample_latents_near`,
    cppflow/planners.py:136-153).  `last` holds the last call's per-row `status`, `pos_err_m` and `rot_err_rad` [k,T].

    Segments: `n_segments` if given, else ceil(T / `waypoints_per_segment`).  A lane runs n_restart + (T / S - 1) n_track LM
    iterations in sequence, and one iteration of a lone lane takes 1.5 - 1.7 us on gfx950 whatever S is (profiles/track_sweep.txt), so
    the default of 35 waypoints per segment caps that depth at 40 + 34 x 6 = 244 iterations, ~0.4 ms of fixed work for any path
    length (fetch__hello, T = 553: S = 16), while a short path (T <= 35) stays one continuous track per candidate."""

    def __init__(self, seed: int = 0, n_segments: Optional[int] = None, waypoints_per_segment: int = 35, damping: float = 1e-2, n_restart_steps: int = 40, n_track_steps: int = 6,
                 n_random_restarts: int = 2, tol_pos_m: float = 5e-5, tol_rot_rad: float = 5e-4, max_jump_rad: float = 0.0,
                 max_jump_m: float = 0.0, init_width: float = 0.25):  # fmt: skip
        assert n_segments is None or int(n_segments) >= 1, "n_segments must be >= 1"
        assert int(waypoints_per_segment) >= 1, "waypoints_per_segment must be >= 1"
        assert float(damping) > 0.0, "damping must be > 0"
        assert int(n_restart_steps) >= 1 and int(n_track_steps) >= 1, "n_restart_steps / n_track_steps must be >= 1"
        assert int(n_random_restarts) >= 0, "n_random_restarts must be >= 0"
        assert float(tol_pos_m) >= 0.0 and float(tol_rot_rad) >= 0.0, "tolerances must be >= 0"
        assert (float(tol_pos_m) > 0.0) == (float(tol_rot_rad) > 0.0), "set both tolerances or neither"
        assert float(max_jump_rad) >= 0.0 and float(max_jump_m) >= 0.0, "jump bars must be >= 0 (0 = off)"
        assert float(init_width) >= 0.0, "init_width must be >= 0"
        self.seed = int(seed)
        self.n_segments = None if n_segments is None else int(n_segments)
        self.waypoints_per_segment = int(waypoints_per_segment)
        self._kw = dict(lm_lambda=float(damping), n_restart=int(n_restart_steps), n_track=int(n_track_steps),
                        n_random_restarts=int(n_random_restarts), tol_pos_m=float(tol_pos_m), tol_rot_rad=float(tol_rot_rad),
                        max_jump_rad=float(max_jump_rad), max_jump_m=float(max_jump_m))  # fmt: skip
        self.init_width = float(init_width)
        self.n_calls = 0
        self.last: Optional[Dict[str, torch.Tensor]] = None

    def _q0_near(self, problem: Problem, k: int, S: int, seed: int) -> torch.Tensor:
        """[k*S, d] starts: segment 0 of candidate 0 at the initial configuration, of the others clamped uniform perturbations around it;
        the later segments uniform in the joint box the kernel draws from."""
        rb, dev = problem.robot, problem.target_path.device
        d = rb.ndof
        gen = torch.Generator().manual_seed(seed)
        lo = torch.tensor([l for l, _ in rb.actuated_joints_limits], dtype=torch.float32)
        hi = torch.tensor([u for _, u in rb.actuated_joints_limits], dtype=torch.float32)
        q0 = (lo + (hi - lo) * (0.1 + 0.8 * torch.rand((k, S, d), generator=gen)))
        center = problem.initial_configuration.detach().reshape(-1).to("cpu", torch.float32)
        near = center + self.init_width * (torch.rand((k, d), generator=gen) - 0.5)
        near[0] = center
        q0[:, 0] = torch.minimum(torch.maximum(near, lo), hi)
        q0[0, 0] = center  # exactly there, even outside the limits
        return q0.reshape(k * S, d).to(dev)

    def __call__(self, problem: Problem, k: int) -> torch.Tensor:
        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        T = problem.n_timesteps
        S = self.n_segments if self.n_segments is not None else -(-T // self.waypoints_per_segment)
        S = max(1, min(S, T))
        call = self.n_calls
        self.n_calls += 1
        seed = (self.seed + 0x9E3779B1 * rank) & 0xFFFFFFFF
        q0 = None
        if problem.initial_configuration is not None:
            q0 = self._q0_near(problem, k, S, (seed * 1000003 + call) & 0x7FFFFFFF)
        res = problem.robot.track_paths(problem.target_path.contiguous(), k, n_segments=S, q0=q0, seed=seed, call_index=call,
                                        **self._kw)  # fmt: skip
        self.last = {key: res[key] for key in ("status", "pos_err_m", "rot_err_rad")}
        return res["x"]


class Planner:
    def __init__(self, settings: PlannerSettings, robot, seed_provider: Optional[SeedProvider] = None, process_group=None,
                 candidate_lm_steps: int = 0, device_optimizer: bool = False, n_search_paths: int = 1,
                 search_path_separation_rad: float = 0.5, pin_initial_configuration: bool = False, scene_optimizer: bool = False,
                 certify_motion_level: Optional[int] = None, certify_motion_depth: Optional[int] = None):
        """`process_group` / `candidate_lm_steps`: the sharded candidate stage (module docstring); with `candidate_lm_steps` > 0 every
        (candidate, waypoint) row takes that many fused pose-only LM iterations before the masks are evaluated (one launch).
        `device_optimizer`: the LM optimiser's loop is decided on the device (`run_lm_optimization(device_loop=True)`); same plan.
        `n_search_paths` > 1: the search returns up to that many paths at least `search_path_separation_rad` apart from each other
        (`dp_search_nbest`; the first one is the path a plain search returns) and `CppFlowPlanner` optimises them together, one
        trajectory each, and continues with the first valid one.  One rank only.
        `pin_initial_configuration`: with `problem.initial_configuration` given, `CppFlowPlanner`'s optimiser holds waypoint 0 of
        every search path (they all start there) fixed (`run_lm_optimization(pin_first=True)`): the plan starts at the initial
        configuration bit for bit and the transition out of it is one the optimiser saw, instead of accepting any start within
        SUCCESS_THRESHOLD_initial_q_norm_dist of it or swapping it in afterwards.  Off: the reference's behaviour.
        `scene_optimizer`: for a problem with more than 8 cuboids `CppFlowPlanner`'s optimiser steps against the whole scene
        (`run_lm_optimization(scene_in_step=True)`) instead of an active set of 8; not together with `device_optimizer`.
        `certify_motion_level` (0 .. 6; default None = off): `CppFlowPlanner` checks the MOTION between the waypoints of the plan
        it returns once (`Problem.motion_clearance` at 2^level intervals per transition) and reports `motion_certified`,
        `motion_hit_transitions` and `motion_undecided_transitions` in `debug_info`.  The plan and `Plan.is_valid` are unchanged.
        `certify_motion_depth` (certify_motion_level .. 16; default None = off; needs `certify_motion_level`): the certificate is
        taken by adaptive bisection (`Problem.motion_clearance(resolve_depth=)`): what the uniform test at the level leaves undecided
        is bisected down to this depth, and `debug_info` gains `motion_resolve_depth` (the deepest level any transition ended at)
        and `motion_tests_per_transition` (the mean number of interval tests)."""
        assert certify_motion_level is None or 0 <= int(certify_motion_level) <= 6, "certify_motion_level must be None or 0 .. 6"
        self._certify_motion_level = None if certify_motion_level is None else int(certify_motion_level)
        assert certify_motion_depth is None or (
            self._certify_motion_level is not None and self._certify_motion_level <= int(certify_motion_depth) <= 16
        ), "certify_motion_depth needs certify_motion_level and must be None or certify_motion_level .. 16"
        self._certify_motion_depth = None if certify_motion_depth is None else int(certify_motion_depth)
        assert not (device_optimizer and scene_optimizer), (
            "scene_optimizer=True is not combined with device_optimizer=True: the device loop's gated mask and step launches take "
            "their cuboids from the robot handle"
        )
        self._scene_optimizer = bool(scene_optimizer)
        self._pin_initial_configuration = bool(pin_initial_configuration)
        assert int(n_search_paths) >= 1, "n_search_paths must be >= 1"
        assert float(search_path_separation_rad) >= 0.0, "search_path_separation_rad must be >= 0"
        self._n_search_paths = int(n_search_paths)
        self._search_path_separation_rad = float(search_path_separation_rad)
        self._search_paths: Optional[torch.Tensor] = None  # [n,T,d]: the last search's paths when n_search_paths > 1
        self._device_optimizer = bool(device_optimizer)
        self._cfg = settings
        self._robot = robot
        self._seed_provider = seed_provider if seed_provider is not None else LmIkSeedProvider()
        self._group = process_group
        self._candidate_lm_steps = int(candidate_lm_steps)

    @property
    def robot(self):
        return self._robot

    @property
    def name(self) -> str:
        return str(self.__class__.__name__)

    def set_settings(self, settings: PlannerSettings) -> None:
        self._cfg = settings

    def _run_pipeline(self, problem: Problem, **kwargs) -> Tuple[torch.Tensor, bool, TimingData, dict, tuple]:
        """Candidates -> collision masks -> dp_search (cppflow/planners.py:191-292)."""
        existing = kwargs.get("rerun_data")
        k = self._cfg.k if existing is None else DEFAULT_RERUN_NEW_K
        world = dist.get_world_size(self._group) if dist.is_available() and dist.is_initialized() else 1
        assert self._n_search_paths == 1 or world == 1, (
            "n_search_paths > 1 is not supported with more than one rank: the sharded planner keeps one search path"
        )
        t0 = time()
        if world > 1:
            from cppflow_amd.distributed import padded_shard_size, sharded_candidate_evaluation

            k_local = padded_shard_size(k, problem.n_timesteps, world)  # (k is rounded up to world * k_local candidates)
            qs = self._seed_provider(problem, k_local)  # this rank's [k_local, T, d]
            assert qs.dim() == 3 and tuple(qs.shape) == (k_local, problem.n_timesteps, self.robot.ndof), tuple(qs.shape)
        else:
            qs = self._seed_provider(problem, k)  # [k, T, d]
            assert qs.dim() == 3 and qs.shape[1:] == (problem.n_timesteps, self.robot.ndof), tuple(qs.shape)
        time_seeds = time() - t0
        if self._cfg.return_only_1st_plan:
            return qs[0], False, TimingData(-1, time_seeds, 0.0, 0.0, 0.0, 0.0), {}, (qs[0], None, None)

        t0 = time()
        if world > 1:
            qs, self_viol, env_viol = sharded_candidate_evaluation(problem, qs, self._candidate_lm_steps, self._group)
        elif self._candidate_lm_steps > 0:
            from cppflow_amd.distributed import sharded_candidate_evaluation

            qs, self_viol, env_viol = sharded_candidate_evaluation(problem, qs, self._candidate_lm_steps, None)
        else:
            self_viol, env_viol = qpaths_batched_collisions(problem, qs.contiguous())
        for name, v in (("self", self_viol), ("env", env_viol)):
            pct = float(v.float().mean()) * 100
            assert pct < 95.0, f"too many {name} collisions: {pct} %"  # planners.py:237,247
        if existing is not None:
            qs_prev, self_prev, env_prev = existing
            qs = torch.cat([qs_prev, qs], dim=0)
            self_viol, env_viol = torch.cat([self_prev, self_viol], dim=0), torch.cat([env_prev, env_viol], dim=0)
        if problem.initial_configuration is not None:
            qs[:, 0, :] = problem.initial_configuration
            self_viol[:, 0], env_viol[:, 0] = False, False  # assumed collision-free (planners.py:265-266)
        time_coll = time() - t0

        t0 = time()
        if self._n_search_paths > 1:
            self._search_paths, _, _ = dp_search_nbest(self.robot, qs.contiguous(), self_viol, env_viol, self._n_search_paths,
                                                       self._search_path_separation_rad)  # fmt: skip
            qpath_search = self._search_paths[0]
        else:
            qpath_search = dp_search(self.robot, qs.contiguous(), self_viol, env_viol)
        time_dp = time() - t0
        debug_info = {}
        if self._cfg.do_return_search_path_mjac:  # (cppflow/planners.py:283-284)
            add_search_path_mjac(debug_info, problem, qpath_search)
        return qpath_search, False, TimingData(-1, time_seeds, time_coll, 0.0, time_dp, 0.0), debug_info, (qs, self_viol, env_viol)


class PlannerSearcher(Planner):
    """dp_search over k candidate paths, no optimisation (cppflow/planners.py:301-336)."""

    def __init__(self, settings: PlannerSettings, robot, seed_provider: Optional[SeedProvider] = None, **kwargs):
        super().__init__(settings, robot, seed_provider, **kwargs)
        assert self._cfg.run_dp_search

    def generate_plan(self, problem: Problem, **kwargs) -> PlannerResult:
        assert problem.robot.name == self.robot.name
        t0 = time()
        qpath, _, td, debug_info, q_data = self._run_pipeline(problem, **kwargs)
        if self._cfg.do_rerun_if_large_dp_search_mjac:
            mjac_deg, mjac_cm = get_mjacs(problem.robot, qpath)
            if mjac_deg > self._cfg.rerun_mjac_threshold_deg or mjac_cm > self._cfg.rerun_mjac_threshold_cm:
                qpath, _, td, debug_info, _ = self._run_pipeline(problem, rerun_data=q_data)
        return PlannerResult(
            plan_from_qpath(qpath.detach(), problem),
            TimingData(time() - t0, td.ikflow, td.coll_checking, td.batch_opt, td.dp_search, 0.0), [], [], debug_info,
        )  # fmt: skip


class CppFlowPlanner(Planner):
    """Candidates -> dp_search -> LM optimisation (cppflow/planners.py:339-468)."""

    def generate_plan(self, problem: Problem, **kwargs) -> PlannerResult:
        t0 = kwargs.get("t0", time())
        rerun_data = kwargs.get("rerun_data")
        search_qpath, is_valid, td, debug_info, q_data = self._run_pipeline(problem, **kwargs)

        def out_of_time() -> bool:
            return time() - t0 > self._cfg.tmax_sec

        def result(qpath) -> PlannerResult:
            if self._certify_motion_level is not None:
                add_motion_certificate(debug_info, problem, qpath, self._certify_motion_level, self._certify_motion_depth)
            return PlannerResult(
                plan_from_qpath(qpath, problem),
                TimingData(time() - t0, td.ikflow, td.coll_checking, td.batch_opt, td.dp_search, td.optimizer), [], [],
                debug_info,
            )  # fmt: skip

        if self._cfg.return_only_1st_plan:
            return result(search_qpath)
        if self._cfg.do_rerun_if_large_dp_search_mjac:
            mjac_deg, mjac_cm = get_mjacs(problem.robot, search_qpath)
            if mjac_deg > self._cfg.rerun_mjac_threshold_deg or mjac_cm > self._cfg.rerun_mjac_threshold_cm:
                search_qpath, is_valid, td, debug_info, q_data = self._run_pipeline(problem, rerun_data=q_data)
        if out_of_time() or ((not self._cfg.anytime_mode_enabled) and is_valid):
            return result(search_qpath)

        t0_opt = time()
        budget = dict(max_n_steps=75, return_if_valid_after_n_steps=int(1e8),
                      convergence_threshold=OPTIMIZATION_CONVERGENCE_THRESHOLD) if self._cfg.anytime_mode_enabled else dict(
            max_n_steps=20, return_if_valid_after_n_steps=0, convergence_threshold=1e6)  # fmt: skip  (planners.py:402-422)
        pin_first = self._pin_initial_configuration and problem.initial_configuration is not None
        if self._n_search_paths > 1:
            # the search's paths as one stack of trajectories [n*T, d]; the device loop lets each alternate and end on its own record
            n, T = self._search_paths.shape[0], problem.n_timesteps
            opt = run_lm_optimization(problem, self._search_paths.reshape(n * T, -1).contiguous(),
                                      tmax_sec=self._cfg.tmax_sec - (time() - t0), verbosity=self._cfg.verbosity, parallel_count=n,
                                      per_trajectory=self._device_optimizer, device_loop=self._device_optimizer, pin_first=pin_first,
                                      scene_in_step=self._scene_optimizer, **budget)  # fmt: skip
            s = opt.parallel_seed_idx if 0 <= opt.parallel_seed_idx < n else 0
            x_opt = opt.x_opt.detach()[s * T : (s + 1) * T]
            debug_info["n_search_paths"], debug_info["optimized_path_index"] = n, s
        else:
            opt = run_lm_optimization(problem, search_qpath.contiguous(), tmax_sec=self._cfg.tmax_sec - (time() - t0),
                                      verbosity=self._cfg.verbosity, device_loop=self._device_optimizer, pin_first=pin_first,
                                      scene_in_step=self._scene_optimizer, **budget)  # fmt: skip
            x_opt = opt.x_opt.detach()
        td.optimizer = time() - t0_opt
        debug_info["n_optimization_steps"] = opt.n_steps_taken
        if problem.uses_scene:  # (more than 8 cuboids: what the optimiser's kernels were given, and how often it was chosen)
            debug_info["scene_selection_rounds"], debug_info["active_obstacles"] = opt.scene_selection_rounds, opt.active_obstacles
            if self._scene_optimizer:
                debug_info["scene_optimizer"] = True
        if opt.is_valid:
            if problem.initial_configuration is None or pin_first:  # (pinned: x_opt[0] IS the initial configuration)
                return result(x_opt)
            if torch.norm(problem.initial_configuration - x_opt[0]) < SUCCESS_THRESHOLD_initial_q_norm_dist:
                return result(x_opt)
            swapped = torch.cat((problem.initial_configuration, x_opt[1:]), dim=0)
            return result(swapped) if plan_from_qpath(swapped, problem).is_valid else result(x_opt)
        if self._cfg.do_rerun_if_optimization_fails and rerun_data is None and not out_of_time():
            return self.generate_plan(problem, rerun_data=q_data, t0=t0)
        return result(x_opt)
