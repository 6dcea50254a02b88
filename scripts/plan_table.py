#!/usr/bin/env python3
"""Planning record on the reference's own problems: CppFlowPlanner.generate_plan with both seed providers.

    python scripts/plan_table.py [--out profiles/plan_table.txt] [--problems a,b,...] [--k 175] [--tmax 5]

The 13 problems of the reference's README plus the `_mini` / truncated fixtures, loaded from tests/golden/reference_files with
problem_from_filename, k = 175, tmax_sec = 5 and the constraints of the reference's scripts/evaluate.py:51-56 (0.01 cm, 0.1 deg, 7 deg,
2 cm).  Per problem and provider: valid or not, the constraints that failed, the LM optimisation steps, ms per stage (seeds / masks /
dp_search / optimiser), the searched path's mjac (deg / cm) and the seed stage's own ms measured around the provider call after a
synchronize (TimingData.ikflow is host time up to the provider's return, which for a one-launch provider is mostly enqueue)."""

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


def run(name: str, prov_name: str, k: int, tmax: float, device: str) -> dict:
    problem = load(name, device)
    prov = Timed(providers()[prov_name]())
    settings = PlannerSettings(k=k, tmax_sec=tmax, anytime_mode_enabled=False, do_rerun_if_large_dp_search_mjac=True,
                               do_rerun_if_optimization_fails=False, do_return_search_path_mjac=True, verbosity=0)  # fmt: skip
    planner = CppFlowPlanner(settings, problem.robot, seed_provider=prov)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_table.txt"))
    ap.add_argument("--problems", default=",".join(README_PROBLEMS + FIXTURES))
    ap.add_argument("--k", type=int, default=175)
    ap.add_argument("--tmax", type=float, default=5.0)
    a = ap.parse_args()
    device = "cuda:0"
    assert torch.cuda.is_available(), "plan_table.py runs the planner on the MI355X"
    names = [n for n in a.problems.split(",") if n]
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
