"""The alternating LM optimiser loop decided on the device (`run_lm_optimization(device_loop=True)`, cppf_lm_optimize_enqueue,
csrc/kernels_optloop.h) against the host loop it restates, on the MI355X.

A gated launch that runs executes the same instructions on the same inputs as the ungated launch of the host loop, so everything
here is compared for EQUALITY: decisions (step sequence, n_steps_taken, is_valid) and the bits of x.  Nothing is retried; sizes
are small (W <= 553, S <= 8, 20 iterations)."""

import os

import pytest
import torch

from cppflow_amd import _hip
from cppflow_amd import optimization as opt
from cppflow_amd.data_types import Constraints
from cppflow_amd.lm_hyper_parameters import (
    ALTERNATING_LOSS_CONVERGENCE_THRESHOLD,
    ALTERNATING_LOSS_MAX_N_STEPS,
    ALTERNATING_LOSS_RETURN_IF_SOL_FOUND_AFTER,
)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_files")
BUDGET = dict(tmax_sec=None, max_n_steps=ALTERNATING_LOSS_MAX_N_STEPS, return_if_valid_after_n_steps=ALTERNATING_LOSS_RETURN_IF_SOL_FOUND_AFTER,
              convergence_threshold=ALTERNATING_LOSS_CONVERGENCE_THRESHOLD, verbosity=0)  # fmt: skip
SHIPPED = ("panda__line", "fetch__line")
FIXTURES = ("panda__2cubes", "fetch__hello", "fetch_arm__s__truncated")

_cache = {}


def _problem(name):
    from cppflow_amd.data_type_utils import problem_from_filename

    if name in SHIPPED:
        return problem_from_filename(None, name, robot=None, device=DEV)
    # (the reference's evaluation constraints, scripts/evaluate.py:51-56 there: 0.01 cm, 0.1 deg, 7 deg, 2 cm)
    constraints = Constraints(max_allowed_position_error_cm=0.01, max_allowed_rotation_error_deg=0.1, max_allowed_mjac_deg=7.0,
                              max_allowed_mjac_cm=2.0)  # fmt: skip
    kw = dict(problems_dir=os.path.join(REF, "problems"), paths_dir=os.path.join(REF, "paths"), device=DEV)
    if name == "fetch_arm__s__truncated":
        kw["filepath_override"] = os.path.join(REF, name + ".yaml")
    return problem_from_filename(constraints, name, **kw)


def _base(name):
    """(problem, a path the host optimiser has worked on): the dp_search path over 24 tracked candidates, optimised by the host loop"""
    if name not in _cache:
        from cppflow_amd.data_types import PlannerSettings
        from cppflow_amd.planners import LmIkSeedProvider, PlannerSearcher

        problem = _problem(name)
        search = PlannerSearcher(PlannerSettings(k=24, tmax_sec=30.0, anytime_mode_enabled=False, verbosity=0), problem.robot,
                                 LmIkSeedProvider(seed=1)).generate_plan(problem).plan.q_path  # fmt: skip
        r = opt.run_lm_optimization(problem, search.contiguous(), **BUDGET)
        _cache[name] = (problem, r.x_opt.clone())
    return _cache[name]


def _starts(x_base, S, seed, widths):
    g = torch.Generator().manual_seed(seed)
    out = [x_base.cpu() + w * torch.randn(x_base.shape, generator=g) for w in widths]
    assert len(out) == S
    return torch.cat(out, dim=0).to(DEV).contiguous()


def _host(problem, x0, S=1, monkeypatch=None, **kw):
    """the host loop, with the sequence of steps it takes written down"""
    calls = []
    if monkeypatch is not None:
        pose, full = opt.levenberg_marquardt_only_pose, opt.levenberg_marquardt_full

        def rec_pose(*a, **k):
            calls.append("pose")
            return pose(*a, **k)

        def rec_full(*a, **k):
            calls.append("diff")
            return full(*a, **k)

        monkeypatch.setattr(opt, "levenberg_marquardt_only_pose", rec_pose)
        monkeypatch.setattr(opt, "levenberg_marquardt_full", rec_full)
    args = dict(BUDGET)
    args.update(kw)
    r = opt.run_lm_optimization(problem, x0.clone(), parallel_count=S, **args)
    if monkeypatch is not None:
        monkeypatch.undo()
    return calls, r


def _device(problem, x0, S=1, **kw):
    args = dict(BUDGET)
    args.update(kw)
    return opt.run_lm_optimization(problem, x0.clone(), parallel_count=S, device_loop=True, **args)


def _steps(trace):
    return [t[0] for t in trace]


@pytest.mark.parametrize("name", SHIPPED + FIXTURES)
def test_same_decisions_same_bits_as_the_host_loop(name, monkeypatch):
    """start paths of growing distance from an optimised one: the host loop and the device loop take the same steps, end at the same
    iteration with the same verdict, and return bit-identical x; the chunking of the enqueue does not matter"""
    problem, x_base = _base(name)
    taken = []
    for k, width in enumerate((0.0, 1e-3, 3e-2, 0.5)):
        x0 = _starts(x_base, 1, 100 + k, (width,))
        calls, h = _host(problem, x0, monkeypatch=monkeypatch)
        d = _device(problem, x0)
        print(f"{name} width {width}: host n_steps_taken {h.n_steps_taken} valid {h.is_valid} steps {''.join(c[0] for c in calls)} | "
              f"device n_steps_taken {d.n_steps_taken} valid {d.is_valid} steps {''.join(c[0] for c in _steps(d.trace[0]))}")
        assert _steps(d.trace[0]) == calls
        assert d.n_steps_taken == h.n_steps_taken and d.is_valid == h.is_valid and d.parallel_seed_idx == h.parallel_seed_idx
        assert torch.equal(d.x_opt, h.x_opt)
        assert d.records[0].mode == _hip.OPT_MODE_DONE
        taken.append(h.n_steps_taken)
        if k in (0, 2):
            for sync_every in (1, 3, 20):
                c = _device(problem, x0, sync_every=sync_every)
                assert c.n_steps_taken == d.n_steps_taken and c.is_valid == d.is_valid and c.trace == d.trace
                assert torch.equal(c.x_opt, d.x_opt)
    problem.robot.set_obstacles([], [])


def test_gated_launches_are_no_ops():
    """control block preset to done: an enqueued iteration leaves x, the whole workspace (sentinel pattern, snapshot included) and
    the control block untouched"""
    problem, x_base = _base("panda__line")
    rb, W = problem.robot, problem.n_timesteps
    problem.bind_obstacles()
    for S, per_traj in ((1, False), (3, False), (3, True)):
        x = _starts(x_base, S, 7, (0.01,) * S)
        x_before = x.clone()
        prm = _hip.OptloopParams()
        prm.pose_lm_lambda, prm.pose_alpha_position, prm.pose_alpha_rotation = 1e-6, 3.5, 0.35
        from cppflow_amd.lm_hyper_parameters import ALT_LOSS_V2_1_DIFF

        prm.diff = rb.full_params(ALT_LOSS_V2_1_DIFF)
        prm.constraints = _hip.Constraints(0.01, 0.1, 3.0, 2.0, 0, 0)
        prm.max_n_steps, prm.return_if_valid_after_n_steps, prm.trace_capacity, prm.convergence_threshold = 20, 15, 20, 0.3
        prm.per_trajectory = int(per_traj)
        workspace, control = rb.lm_optimize_buffers(S, W, prm, DEV)
        sentinel = torch.full_like(workspace.view(torch.int32), 0x7FC0BEEF)  # (a NaN pattern, should anything compute on it)
        workspace.view(torch.int32).copy_(sentinel)
        C = S if per_traj else 1
        control[: C * 16].view(C, 16)[:, 0] = _hip.OPT_MODE_DONE
        control_before = control.clone()
        rb.lm_optimize_enqueue(x, problem.target_path, prm, workspace, control, 2)
        torch.cuda.synchronize()
        assert torch.equal(x, x_before)
        assert torch.equal(workspace.view(torch.int32), sentinel)
        assert torch.equal(control, control_before)
    rb.set_obstacles([], [])


def test_per_trajectory_mode_and_the_reference_rule_for_parallel_seeds(monkeypatch):
    """S = 8 starts of one problem, some at an optimised path, some far from it.  per_trajectory=True: every trajectory's decisions and
    final x are those of a separate S = 1 device-loop run of the same start, bit for bit.  per_trajectory=False: the host loop at
    parallel_count = 8."""
    problem, x_base = _base("panda__line")
    W, S = problem.n_timesteps, 8
    widths = (0.0, 0.3, 1e-3, 0.0, 0.6, 2e-2, 1e-3, 0.3)
    x0 = _starts(x_base, S, 5, widths)
    per = _device(problem, x0, S=S, per_trajectory=True)
    singles = [_device(problem, x0[s * W : (s + 1) * W].contiguous()) for s in range(S)]
    for s in range(S):
        print(f"trajectory {s} width {widths[s]}: n_steps_taken {singles[s].n_steps_taken} valid {singles[s].is_valid}")
        assert per.trace[s] == singles[s].trace[0]
        assert torch.equal(per.x_opt[s * W : (s + 1) * W], singles[s].x_opt)
        assert per.records[s].i_final == singles[s].records[0].i_final and per.records[s].is_valid == singles[s].records[0].is_valid
    ok = [r.is_valid for r in singles]
    assert per.is_valid == any(ok) and per.parallel_seed_idx == (ok.index(True) if any(ok) else 0)
    assert per.n_steps_taken == max(r.n_steps_taken for r in singles)
    assert len({len(t) for t in per.trace}) > 1, "the starts were meant to need different numbers of iterations"
    # one decision for all: the reference's rule
    calls, h = _host(problem, x0, S=S, monkeypatch=monkeypatch)
    d = _device(problem, x0, S=S)
    assert _steps(d.trace[0]) == calls
    assert d.n_steps_taken == h.n_steps_taken and d.is_valid == h.is_valid and d.parallel_seed_idx == h.parallel_seed_idx
    assert torch.equal(d.x_opt, h.x_opt)
    problem.robot.set_obstacles([], [])


@pytest.mark.parametrize("on_pose_valid", ["stop", "continue"])
@pytest.mark.parametrize("name", ["panda__line", "fetch_arm__s__truncated"])
def test_on_pose_valid_stop_and_continue_match_the_host_loop(name, on_pose_valid, monkeypatch):
    """the two branches that replace the differencing step (stop once the pose is valid / keep taking pose steps), from a start near
    an optimised path and from one far from it: same steps, same end, same bits as the host loop"""
    problem, x_base = _base(name)
    for k, width in enumerate((1e-3, 0.5)):
        x0 = _starts(x_base, 1, 200 + k, (width,))
        calls, h = _host(problem, x0, monkeypatch=monkeypatch, on_pose_valid=on_pose_valid)
        d = _device(problem, x0, on_pose_valid=on_pose_valid)
        print(f"{name} {on_pose_valid} width {width}: host n_steps_taken {h.n_steps_taken} valid {h.is_valid} steps {''.join(c[0] for c in calls)} | "
              f"device n_steps_taken {d.n_steps_taken} valid {d.is_valid} steps {''.join(c[0] for c in _steps(d.trace[0]))}")
        assert "diff" not in calls
        assert _steps(d.trace[0]) == calls
        assert d.n_steps_taken == h.n_steps_taken and d.is_valid == h.is_valid and d.parallel_seed_idx == h.parallel_seed_idx
        assert torch.equal(d.x_opt, h.x_opt)
    problem.robot.set_obstacles([], [])


def _smooth_fetch_553():
    """(problem, path): Fetch (8 joints), 553 waypoints -- beyond the parallel-in-time limit, so the coupled step is eliminated row per
    lane by default -- with the target = FK of a smooth joint path that is free of self-collisions (checked here on the host) and
    without obstacles: the path itself is a valid trajectory, starts near it end early, starts far from it do not"""
    if "fetch__553" not in _cache:
        import numpy as np

        from cppflow_amd.data_type_utils import problem_from_arrays
        from cppflow_amd.robots import get_robot
        from tests import helpers as H

        ch, W = H.chain("fetch"), 553
        rng = np.random.RandomState(500)
        q0 = rng.uniform(ch.lo + 0.3 * (ch.hi - ch.lo), ch.hi - 0.3 * (ch.hi - ch.lo))
        step = 0.004 * rng.randn(W, ch.ndof)
        step[:, ch.jtype == 1] *= 0.1
        path = H.f32(np.clip(q0[None] + np.cumsum(step, axis=0), ch.lo + 0.01, ch.hi - 0.01))
        assert not H.oracle32("fetch").masks(path, None, None, None, None)["self_mask"].any()
        problem = problem_from_arrays(get_robot("fetch"), H.f32(H.oracle64("fetch").fk(path)), [], name="fetch__553", device=DEV)
        _cache["fetch__553"] = (problem, torch.tensor(path, dtype=torch.float32, device=DEV))
    return _cache["fetch__553"]


@pytest.mark.parametrize("name,S,switches", [("fetch_arm__s__truncated", 8, {}), ("fetch_arm__s__truncated", 8, {"pcr_max_rows": 0}),
                                             ("fetch__553", 3, {})])  # fmt: skip
def test_per_trajectory_at_an_unaligned_width_and_on_the_row_per_lane_path(name, S, switches, monkeypatch):
    """per_trajectory=True where a trajectory boundary falls inside a wavefront (W is not a multiple of 16) and where the coupled step
    is eliminated one trajectory per lane group (pcr_max_rows = 0; W > 512): every trajectory takes the steps, ends at the iteration
    and returns the bits of a separate HOST loop of the same start under the same tuning.
    The W > 512 case is Fetch at the 553 waypoints of fetch__hello with a reachable target (`_smooth_fetch_553`), not fetch__hello's own
    target: from the search path of fetch__hello (24 or 175 candidates) every start of width 0, 1e-3 and 0.3 alike takes 20 pose steps
    and is never valid (host n_steps_taken 19, valid False, steps pppppppppppppppppppp), so no coupled step would run and no two
    trajectories would differ in what they need."""
    problem, x_base = _smooth_fetch_553() if name == "fetch__553" else _base(name)
    W, rb = problem.n_timesteps, problem.robot
    assert W % 16 != 0
    widths = (0.0, 0.3, 1e-3, 0.0, 0.6, 2e-2, 1e-3, 0.3)[:S]
    x0 = _starts(x_base, S, 5, widths)
    try:
        for key, value in switches.items():
            rb.debug_set(key, value)
        per = _device(problem, x0, S=S, per_trajectory=True)
        for s in range(S):
            calls, h = _host(problem, x0[s * W : (s + 1) * W].contiguous(), monkeypatch=monkeypatch)
            print(f"trajectory {s} width {widths[s]}: host n_steps_taken {h.n_steps_taken} valid {h.is_valid} steps {''.join(c[0] for c in calls)}")
            assert _steps(per.trace[s]) == calls
            assert max(per.records[s].i_final, 0) == h.n_steps_taken and bool(per.records[s].is_valid) == h.is_valid
            assert torch.equal(per.x_opt[s * W : (s + 1) * W], h.x_opt)
        assert len({len(t) for t in per.trace}) > 1, "the starts were meant to need different numbers of iterations"
        assert any("diff" in _steps(t) for t in per.trace), "no trajectory took a coupled step"
    finally:
        for key in switches:
            rb.debug_set(key, None)
        rb.set_obstacles([], [])


def test_planner_with_the_device_optimizer_returns_the_same_plan():
    from cppflow_amd.data_types import PlannerSettings
    from cppflow_amd.planners import CppFlowPlanner, LmIkSeedProvider

    problem = _problem("panda__line")
    settings = PlannerSettings(k=64, tmax_sec=30.0, anytime_mode_enabled=False, verbosity=0)
    a = CppFlowPlanner(settings, problem.robot, LmIkSeedProvider(seed=1)).generate_plan(problem)
    b = CppFlowPlanner(settings, problem.robot, LmIkSeedProvider(seed=1), device_optimizer=True).generate_plan(problem)
    assert a.plan.is_valid and b.plan.is_valid
    assert torch.equal(a.plan.q_path, b.plan.q_path)
    assert a.debug_info["n_optimization_steps"] == b.debug_info["n_optimization_steps"]
    problem.robot.set_obstacles([], [])
    problem.robot.set_joint_limit_padding(None, None)


def test_determinism_and_a_non_finite_start_row():
    problem, x_base = _base("fetch__line")
    W = problem.n_timesteps
    x0 = _starts(x_base, 1, 11, (2e-2,))
    a, b = _device(problem, x0), _device(problem, x0)
    assert a.trace == b.trace and torch.equal(a.x_opt, b.x_opt)
    assert [bytes(r) for r in a.records] == [bytes(r) for r in b.records]
    # a non-finite row: never valid, runs to max_n_steps, as the host loop does
    x_bad = x0.clone()
    x_bad[W // 2, 3] = float("nan")
    calls, h = _host(problem, x_bad)
    d = _device(problem, x_bad)
    assert not h.is_valid and h.n_steps_taken == ALTERNATING_LOSS_MAX_N_STEPS - 1
    assert not d.is_valid and d.n_steps_taken == h.n_steps_taken and len(d.trace[0]) == ALTERNATING_LOSS_MAX_N_STEPS
    assert torch.equal(torch.isnan(d.x_opt), torch.isnan(h.x_opt))
    assert torch.equal(torch.nan_to_num(d.x_opt, nan=0.0), torch.nan_to_num(h.x_opt, nan=0.0))
    problem.robot.set_obstacles([], [])


def test_one_device_to_host_copy_per_run(monkeypatch):
    """sync_every=None, tmax_sec=None: the whole run is enqueued ahead and the loop-control block comes back in ONE copy -- no
    synchronize, no .item(), one .cpu() of a device tensor"""
    problem, x_base = _base("panda__line")
    x0 = _starts(x_base, 1, 3, (1e-3,))
    _device(problem, x0)  # (handles, obstacles and buffers of the caching allocator are warm)
    counts = dict(cpu=0, item=0, sync=0, tolist=0)
    cpu, item, sync, tolist = torch.Tensor.cpu, torch.Tensor.item, torch.cuda.synchronize, torch.Tensor.tolist

    def count(key, fn, only_device):
        def wrapped(self, *a, **k):
            if not only_device or self.is_cuda:
                counts[key] += 1
            return fn(self, *a, **k)

        return wrapped

    def counted_sync(*a, **k):
        counts["sync"] += 1
        return sync(*a, **k)

    monkeypatch.setattr(torch.Tensor, "cpu", count("cpu", cpu, True))
    monkeypatch.setattr(torch.Tensor, "item", count("item", item, True))
    monkeypatch.setattr(torch.Tensor, "tolist", count("tolist", tolist, True))
    monkeypatch.setattr(torch.cuda, "synchronize", counted_sync)
    d = _device(problem, x0)
    monkeypatch.undo()
    assert counts == dict(cpu=1, item=0, sync=0, tolist=0), counts
    assert d.records[0].mode == _hip.OPT_MODE_DONE
    # the host loop, for contrast: one copy per iteration
    monkeypatch.setattr(torch.Tensor, "cpu", count("cpu", cpu, True))
    counts["cpu"] = 0
    _, h = _host(problem, x0)
    monkeypatch.undo()
    assert counts["cpu"] >= h.n_steps_taken + 1
    problem.robot.set_obstacles([], [])
