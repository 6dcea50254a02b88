#!/usr/bin/env python3
"""Planning record on the reference's own problems: CppFlowPlanner.generate_plan with both seed providers.

    python scripts/plan_table.py [--out profiles/plan_table.txt] [--problems a,b,...] [--k 175] [--tmax 5]
    python scripts/plan_table.py --device-loop [--out profiles/plan_table_device_loop.txt] [--repeats 5]

The 13 problems of the reference's README plus the `_mini` / truncated fixtures, loaded from tests/golden/reference_files with
problem_from_filename, k = 175, tmax_sec = 5 and the constraints of the reference's scripts/evaluate.py:51-56 (0.01 cm, 0.1 deg, 7 deg,
2 cm).  Per problem and provider: valid or not, the constraints that failed, the LM optimisation steps, ms per stage (seeds / masks /
dp_search / optimiser), the searched path's mjac (deg / cm) and the seed stage's own ms measured around the provider call after a
synchronize (TimingData.ikflow is host time up to the provider's return, which for a one-launch provider is mostly enqueue).

`--device-loop` writes a second table instead: per problem (LmIk provider) the optimiser stage with the host loop and with the loop
decided on the device (`CppFlowPlanner(device_optimizer=True)`), same process, alternating, median of `--repeats` plans each after one
warm-up plan of either kind; and the cost of enqueuing gated-off iterations behind a finished loop (host time per iteration to
enqueue, device time per iteration to drain), which is what enqueuing ahead pays for.

`--pin` writes a third table (profiles/plan_table_pinned.txt): per problem (Tracking provider) the initial configuration is row 0 of
the problem's own unpinned valid plan; then the planner runs from it twice -- the swap route (`pin_initial_configuration=False`:
accept a start within 0.2 rad, else swap q0 in) and the pinned route (`True`: waypoint 0 held fixed through the optimiser) -- and
the table puts side by side: valid or not, the failing constraint, LM steps, `initial_q_norm_dist` and the joint change of
transition 0 -> 1 (max over the joints; degrees over the revolute, cm over the prismatic ones)."""

import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cppflow_amd.data_type_utils import problem_from_filename  # noqa: E402
from cppflow_amd.data_types import Constraints, PlannerSettings  # noqa: E402
from cppflow_amd.planners import CppFlowPlanner, LmIkSeedProvider, TrackingSeedProvider  # noqa: E402

REF = os.path.join(ROOT, "tests", "golden", "reference_files")
README_PROBLEMS = ["fetch__circle", "fetch__hello", "fetch__rot_yz", "fetch__s", "fetch__square", "fetch_arm__circle",
                   "fetch_arm__hello", "fetch_arm__rot_yz", "fetch_arm__s", "fetch_arm__square", "panda__flappy_bird",
                   "panda__2cubes", "panda__1cube"]  # fmt: skip
FIXTURES = ["fetch_arm__hello_mini", "panda__1cube_mini", "fetch_arm__s__truncated"]
CONSTRAINTS = Constraints(max_allowed_position_error_cm=0.01, max_allowed_rotation_error_deg=0.1, max_allowed_mjac_deg=7.0,
                          max_allowed_mjac_cm=2.0)  # fmt: skip


def load(name: str, device: str):
    if name == "fetch_arm__s__truncated":  # the reference's tests/ fixture: a problem file with its own path location
        return problem_from_filename(CONSTRAINTS, name, filepath_override=os.path.join(REF, name + ".yaml"),
                                     problems_dir=os.path.join(REF, "problems"), paths_dir=os.path.join(REF, "paths"), device=device)  # fmt: skip
    return problem_from_filename(CONSTRAINTS, name, problems_dir=os.path.join(REF, "problems"), paths_dir=os.path.join(REF, "paths"),
                                 device=device)  # fmt: skip


class Timed:
    """wraps a seed provider: device time of each call (synchronize before and after)"""

    def __init__(self, inner):
        self.inner, self.ms = inner, []

    def __call__(self, problem, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = self.inner(problem, k)
        torch.cuda.synchronize()
        self.ms.append(1e3 * (time.perf_counter() - t0))
        return out


def providers():
    return {"LmIk": lambda: LmIkSeedProvider(seed=0), "Tracking": lambda: TrackingSeedProvider(seed=0)}


def run(name: str, prov_name: str, k: int, tmax: float, device: str, device_optimizer: bool = False) -> dict:
    problem = load(name, device)
    prov = Timed(providers()[prov_name]())
    settings = PlannerSettings(k=k, tmax_sec=tmax, anytime_mode_enabled=False, do_rerun_if_large_dp_search_mjac=True,
                               do_rerun_if_optimization_fails=False, do_return_search_path_mjac=True, verbosity=0)  # fmt: skip
    planner = CppFlowPlanner(settings, problem.robot, seed_provider=prov, device_optimizer=device_optimizer)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = planner.generate_plan(problem)
    torch.cuda.synchronize()
    wall = 1e3 * (time.perf_counter() - t0)
    flags = res.plan.validity_flags()
    td, di = res.timing, res.debug_info
    return dict(problem=name, provider=prov_name, T=problem.n_timesteps, valid=res.plan.is_valid,
                failed=",".join(f for f, ok in flags.items() if not ok) or "-", lm_steps=di.get("n_optimization_steps", 0),
                seeds_ms=1e3 * td.ikflow, seed_dev_ms=sum(prov.ms), n_seed_calls=len(prov.ms), masks_ms=1e3 * td.coll_checking,
                dp_ms=1e3 * td.dp_search, opt_ms=1e3 * td.optimizer, total_ms=wall,
                mjac_deg=di.get("search_path_mjac-deg", float("nan")), mjac_cm=di.get("search_path_mjac-cm", float("nan")),
                pos_cm=res.plan.max_positional_error_cm, rot_deg=res.plan.max_rotational_error_deg,
                plan_mjac_deg=res.plan.mjac_deg, plan_mjac_cm=res.plan.mjac_cm)  # fmt: skip


def noop_iteration_cost(name: str, device: str, n_iterations: int = 20, repeats: int = 20):
    """(host us per iteration to enqueue, device us per iteration to drain) for iterations enqueued behind a loop that is done"""
    import statistics

    from cppflow_amd import _hip
    from cppflow_amd.lm_hyper_parameters import ALT_LOSS_V2_1_DIFF

    problem = load(name, device)
    rb, W = problem.robot, problem.n_timesteps
    problem.bind_obstacles()
    prm = _hip.OptloopParams()
    prm.pose_lm_lambda, prm.pose_alpha_position, prm.pose_alpha_rotation = 1e-6, 3.5, 0.35
    prm.diff = rb.full_params(ALT_LOSS_V2_1_DIFF)
    prm.constraints = _hip.Constraints(0.01, 0.1, 7.0, 2.0, 0, 0)
    prm.max_n_steps, prm.return_if_valid_after_n_steps, prm.trace_capacity, prm.convergence_threshold = 20, 0, 20, 1e6
    workspace, control = rb.lm_optimize_buffers(1, W, prm, device)
    control[0] = _hip.OPT_MODE_DONE
    x = torch.zeros((W, rb.ndof), dtype=torch.float32, device=device)
    host, dev = [], []
    for r in range(repeats + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rb.lm_optimize_enqueue(x, problem.target_path, prm, workspace, control, n_iterations)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if r >= 3:
            host.append(1e6 * (t1 - t0) / n_iterations)
            dev.append(1e6 * (t2 - t0) / n_iterations)
    return statistics.median(host), statistics.median(dev), W


def main_device_loop(a, names):
    import statistics

    device = "cuda:0"
    for dl in (False, True):
        run("panda__1cube_mini", "LmIk", a.k, a.tmax, device, device_optimizer=dl)
    lines = [f"# scripts/plan_table.py --device-loop: the optimiser stage of CppFlowPlanner.generate_plan (LmIk provider, k = {a.k}, "
             f"tmax_sec = {a.tmax}), host loop vs the loop decided on the device; ms, median of {a.repeats} plans each, alternating, "
             f"same process, after one warm-up plan of either kind per problem",
             f"# torch {torch.__version__}, device {torch.cuda.get_device_name(0)}",
             f"{'problem':26s} {'T':>4s} {'lm':>3s} {'opt_host':>9s} {'opt_dev':>9s} {'min_host':>9s} {'min_dev':>9s} {'same':>5s}"]  # fmt: skip
    print("\n".join(lines), flush=True)
    for name in names:
        res = {False: [], True: []}
        for rep in range(a.repeats + 1):
            for dl in (False, True):
                r = run(name, "LmIk", a.k, a.tmax, device, device_optimizer=dl)
                if rep > 0:
                    res[dl].append(r)
        h, d = [r["opt_ms"] for r in res[False]], [r["opt_ms"] for r in res[True]]
        same = all(x["lm_steps"] == y["lm_steps"] and x["valid"] == y["valid"] for x, y in zip(res[False], res[True]))
        ln = (f"{name:26s} {res[False][0]['T']:4d} {res[False][0]['lm_steps']:3d} {statistics.median(h):9.3f} {statistics.median(d):9.3f} "
              f"{min(h):9.3f} {min(d):9.3f} {str(same):>5s}")  # fmt: skip
        print(ln, flush=True)
        lines.append(ln)
    lines.append("# gated-off iterations enqueued behind a finished loop (7 or 8 launches each): host us per iteration to enqueue, us per "
                 "iteration until the device has drained them (median of 20 x 20 iterations)")
    for name in ("panda__1cube_mini", "fetch__hello"):
        if name in names or name == "panda__1cube_mini":
            hu, du, W = noop_iteration_cost(name, device)
            ln = f"# noop {name:24s} T {W:4d}  enqueue {hu:7.2f} us/iteration  drained {du:7.2f} us/iteration"
            print(ln, flush=True)
            lines.append(ln)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def first_transition(plan, robot):
    """(max |revolute joint change| in degrees, max |prismatic joint change| in cm) of transition 0 -> 1 of the plan"""
    import math

    rev, pris = robot.split_configs_to_revolute_and_prismatic(plan.q_path[1:2] - plan.q_path[0:1])
    rev = (torch.remainder(rev + math.pi, 2 * math.pi) - math.pi).abs()
    return (math.degrees(float(rev.max())) if rev.numel() else 0.0), (100.0 * float(pris.abs().max()) if pris.numel() else 0.0)


def main_pin(a, names):
    import dataclasses

    device = "cuda:0"

    def plan(problem, pin):
        settings = PlannerSettings(k=a.k, tmax_sec=a.tmax, anytime_mode_enabled=False, do_rerun_if_large_dp_search_mjac=True,
                                   do_rerun_if_optimization_fails=False, verbosity=0)  # fmt: skip
        planner = CppFlowPlanner(settings, problem.robot, seed_provider=TrackingSeedProvider(seed=0), pin_initial_configuration=pin)
        return planner.generate_plan(problem)

    def cells(res, robot):
        flags = res.plan.validity_flags()
        deg, cm = first_transition(res.plan, robot)
        failed = ",".join(f for f, ok in flags.items() if not ok) or "-"
        return (f"{str(res.plan.is_valid):5s} {res.debug_info.get('n_optimization_steps', 0):3d} {res.plan.initial_q_norm_dist:9.2e} {deg:7.3f} {cm:6.3f} "
                f"{res.plan.mjac_deg:7.3f} {res.plan.mjac_cm:6.3f} {failed:24s}")  # fmt: skip

    plan(load("panda__1cube_mini", device), False)  # warm-up
    side = f"{'valid':5s} {'lm':>3s} {'q0_dist':>9s} {'t01_deg':>7s} {'t01_cm':>6s} {'mjacdeg':>7s} {'mjaccm':>6s} {'failed':24s}"
    lines = [f"# scripts/plan_table.py --pin: CppFlowPlanner.generate_plan (Tracking provider, k = {a.k}, tmax_sec = {a.tmax}, constraints "
             "0.01 cm / 0.1 deg / 7 deg / 2 cm) from an initial configuration = row 0 of the problem's own unpinned valid plan; the swap "
             "route (pin_initial_configuration=False) and the pinned route (True) side by side.  q0_dist = initial_q_norm_dist (rad), "
             "t01 = the joint change of transition 0 -> 1, mjac = the plan's maximum joint change",
             f"# torch {torch.__version__}, device {torch.cuda.get_device_name(0)}",
             f"{'problem':26s} {'T':>4s} | swap: {side} | pinned: {side}"]  # fmt: skip
    print("\n".join(lines), flush=True)
    for name in names:
        problem = load(name, device)
        base = plan(problem, False)
        if not base.plan.is_valid:
            ln = f"{name:26s} {problem.n_timesteps:4d} | no valid unpinned plan to take q0 from"
        else:
            with_q0 = dataclasses.replace(problem, initial_configuration=base.plan.q_path[0:1].clone())
            ln = f"{name:26s} {problem.n_timesteps:4d} | swap: {cells(plan(with_q0, False), problem.robot)} | pinned: {cells(plan(with_q0, True), problem.robot)}"
        print(ln, flush=True)
        lines.append(ln)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--device-loop", action="store_true", help="the optimiser stage, host loop vs device loop (a table of its own)")
    ap.add_argument("--pin", action="store_true", help="swap route vs pinned initial configuration (a table of its own)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--problems", default=",".join(README_PROBLEMS + FIXTURES))
    ap.add_argument("--k", type=int, default=175)
    ap.add_argument("--tmax", type=float, default=5.0)
    a = ap.parse_args()
    device = "cuda:0"
    assert torch.cuda.is_available(), "plan_table.py runs the planner on the MI355X"
    names = [n for n in a.problems.split(",") if n]
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "plan_table_pinned.txt" if a.pin else "plan_table_device_loop.txt" if a.device_loop else "plan_table.txt")
    if a.pin:
        return main_pin(a, names)
    if a.device_loop:
        return main_device_loop(a, names)
    # warm-up: the first planning call of a process pays for allocator growth and library loading
    for pn in providers():
        run("panda__1cube_mini", pn, a.k, a.tmax, device)
    head = (f"{'problem':26s} {'provider':8s} {'T':>4s} {'valid':5s} {'lm':>3s} {'seeds':>8s} {'seed_dev':>8s} {'masks':>7s} "
            f"{'dp':>7s} {'opt':>8s} {'total':>8s} {'s_mjac_deg':>10s} {'s_mjac_cm':>9s} {'pos_cm':>8s} {'rot_deg':>8s} "
            f"{'mjac_deg':>8s} {'mjac_cm':>7s}  failed")  # fmt: skip
    lines = [f"# scripts/plan_table.py: CppFlowPlanner.generate_plan, k = {a.k}, tmax_sec = {a.tmax}, constraints 0.01 cm / 0.1 deg / "
             f"7 deg / 2 cm, rerun on large dp_search mjac; ms per stage (seeds = TimingData.ikflow, seed_dev = the provider "
             f"call(s) between two synchronizes, summed over the {{1, 2}} calls a rerun makes); s_mjac = the searched path's mjac",
             f"# torch {torch.__version__}, device {torch.cuda.get_device_name(0)}", head]  # fmt: skip
    print("\n".join(lines), flush=True)
    for name in names:
        for pn in providers():
            r = run(name, pn, a.k, a.tmax, device)
            ln = (f"{r['problem']:26s} {r['provider']:8s} {r['T']:4d} {str(r['valid']):5s} {r['lm_steps']:3d} {r['seeds_ms']:8.2f} "
                  f"{r['seed_dev_ms']:8.2f} {r['masks_ms']:7.2f} {r['dp_ms']:7.2f} {r['opt_ms']:8.2f} {r['total_ms']:8.1f} "
                  f"{r['mjac_deg']:10.3f} {r['mjac_cm']:9.3f} {r['pos_cm']:8.5f} {r['rot_deg']:8.4f} {r['plan_mjac_deg']:8.3f} "
                  f"{r['plan_mjac_cm']:7.3f}  {r['failed']}")  # fmt: skip
            print(ln, flush=True)
            lines.append(ln)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
