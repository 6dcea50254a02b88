#!/usr/bin/env python3
"""What the N-best search paths cost and what they yield (developer tool; writes profiles/dp_nbest.txt).

    python scripts/dp_nbest_bench.py [--out profiles/dp_nbest.txt] [--problems a,b,...] [--k 175] [--tmax 5] [--skip-plans]

1. Selection time after a search: `cppf_dp_nbest` (three launches) at k = 175 / 300, T = 256, N = 1 / 4 / 8, threshold 0.5 rad, beside
   `cppf_dp_search` (resident form) at the same shape in the same process -- device events around the calls, median of 30 after 5
   warm-up calls; candidates = 3 clusters 2 rad apart with 0.01 rad of noise (a kill round does its full k x T compares).
2. Optimiser time for 1 / 4 / 8 stacked paths through the device loop (`run_lm_optimization(parallel_count = n, per_trajectory = True,
   device_loop = True)`, the planner's budget of 20 steps) on one problem: host clock around the call, which ends in the loop-control
   copy (a synchronise); median of 7 after 2 warm-up calls.
3. Plans on the problems of scripts/plan_table.py with n_search_paths = 1 vs 4 at the default separation (Tracking provider): valid or
   not, paths found, the path the plan came from, LM steps, search and optimiser ms."""

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cppflow_amd.robots import get_robot  # noqa: E402

from plan_table import FIXTURES, README_PROBLEMS, load  # noqa: E402  (scripts/ is sys.path[0])

DEV = "cuda:0"


def event_us(fn, warmup=5, reps=30):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def clustered(k, T, d, C=3, seed=0):
    rng = np.random.RandomState(seed)
    walk = np.cumsum(rng.uniform(-0.02, 0.02, size=(T, d)), axis=0)
    q = walk[None] + rng.uniform(-0.01, 0.01, size=(k, T, d))
    q[:, :, 1] += 2.0 * (np.arange(k) % C)[:, None] - 2.0
    return torch.tensor(q, dtype=torch.float32, device=DEV)


def selection_times(lines):
    import ctypes

    from cppflow_amd import _hip

    rb = get_robot("panda")
    lib, h, d = _hip.lib(), rb._handle(torch.device(DEV)), rb.ndof
    lines.append("# 1. selection after a search, panda, T = 256, threshold 0.5 rad, 3 clusters of candidates; C ABI calls on preallocated "
                 "buffers, us per call: device events around 10 calls back to back / 10, median (min .. max) of 30 windows")  # fmt: skip
    lines.append(f"{'k':>4s} {'N':>3s} {'found':>5s} {'dp_search':>22s} {'dp_nbest':>22s} {'share added':>11s}")
    for k in (175, 300):
        T = 256
        q = clustered(k, T, d)
        ext = torch.zeros((k, T), device=DEV)
        qT, costsT = torch.empty((T, k, d), device=DEV), torch.empty((T, k), device=DEV)
        memoT = torch.empty((T, k), dtype=torch.int32, device=DEV)
        bp, bi = torch.empty((T, d), device=DEV), torch.empty(T, dtype=torch.int32, device=DEV)
        st = torch.cuda.current_stream(DEV).cuda_stream

        def search():
            for _ in range(10):
                _hip.check(lib.cppf_dp_search(h, q.data_ptr(), ext.data_ptr(), k, T, 5.0, qT.data_ptr(), costsT.data_ptr(), memoT.data_ptr(),
                                              bp.data_ptr(), bi.data_ptr(), _hip.DP_RESIDENT, st))  # fmt: skip

        s = [v / 10 for v in event_us(search)]
        assert int(bi[0]) >= 0
        for N in (1, 4, 8):
            nb = ctypes.c_size_t(0)
            _hip.check(lib.cppf_dp_nbest_workspace_bytes(k, T, N, ctypes.byref(nb)))
            ws = torch.empty(nb.value // 4, dtype=torch.int32, device=DEV)
            paths, pidx = torch.empty((N, T, d), device=DEV), torch.empty((N, T), dtype=torch.int32, device=DEV)
            pcost, nf = torch.empty(N, device=DEV), torch.empty(1, dtype=torch.int32, device=DEV)

            def select():
                for _ in range(10):
                    _hip.check(lib.cppf_dp_nbest(h, q.data_ptr(), costsT.data_ptr(), memoT.data_ptr(), k, T, N, 0.5, 5.0, ws.data_ptr(),
                                                 paths.data_ptr(), pidx.data_ptr(), pcost.data_ptr(), nf.data_ptr(), st))  # fmt: skip

            n = [v / 10 for v in event_us(select)]
            lines.append(f"{k:4d} {N:3d} {int(nf[0]):5d} {s[0]:8.1f} ({s[1]:5.1f} ..{s[2]:6.1f}) {n[0]:8.1f} ({n[1]:5.1f} ..{n[2]:6.1f}) "
                         f"{100 * n[0] / s[0]:10.1f}%")  # fmt: skip
            print(lines[-1], flush=True)


def optimiser_times(lines, name="panda__1cube_mini"):
    from cppflow_amd.optimization import run_lm_optimization
    from cppflow_amd.planners import TrackingSeedProvider
    from cppflow_amd.search import dp_search_nbest, q_costs_external

    problem = load(name, DEV)
    T = problem.n_timesteps
    qs = TrackingSeedProvider(seed=0)(problem, 175)
    cost, _, _, _ = q_costs_external(problem.robot, qs, problem)
    paths, _, _ = dp_search_nbest(problem.robot, qs.contiguous(), None, None, 8, 0.0, q_costs=cost)  # threshold 0: 8 paths whatever they are
    lines.append(f"# 2. run_lm_optimization(device_loop, per_trajectory, max_n_steps = 20) on n stacked paths, {name} (T = {T}); "
                 f"ms of host clock around the call, median (min .. max) of 7")  # fmt: skip
    for n in (1, 4, 8):
        x = paths[:n].reshape(n * T, -1).contiguous()

        def call():
            return run_lm_optimization(problem, x, tmax_sec=None, max_n_steps=20, return_if_valid_after_n_steps=0,
                                       convergence_threshold=1e6, verbosity=0, parallel_count=n, per_trajectory=True, device_loop=True)  # fmt: skip

        for _ in range(2):
            call()
        ts = []
        for _ in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = call()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        lines.append(f"n = {n}: {statistics.median(ts):8.3f} ({min(ts):7.3f} ..{max(ts):8.3f}) ms   valid {r.is_valid}  "
                     f"first valid path {r.parallel_seed_idx}  steps {r.n_steps_taken}")  # fmt: skip
        print(lines[-1], flush=True)


def plans(lines, names, k, tmax):
    from cppflow_amd.data_types import PlannerSettings
    from cppflow_amd.planners import CppFlowPlanner, TrackingSeedProvider

    lines.append(f"# 3. CppFlowPlanner(device_optimizer = True, Tracking provider, k = {k}, tmax_sec = {tmax}, no reruns), n_search_paths = 1 "
                 f"vs 4 at search_path_separation_rad = 0.5: valid, paths found, the path the plan came from, LM steps, dp / optimiser ms")  # fmt: skip
    lines.append(f"{'problem':26s} {'T':>4s} | {'valid1':>6s} {'lm':>3s} {'dp_ms':>7s} {'opt_ms':>8s} | {'valid4':>6s} {'found':>5s} {'path':>4s} "
                 f"{'lm':>3s} {'dp_ms':>7s} {'opt_ms':>8s}")  # fmt: skip
    settings = PlannerSettings(k=k, tmax_sec=tmax, anytime_mode_enabled=False, do_rerun_if_large_dp_search_mjac=False,
                               do_rerun_if_optimization_fails=False, verbosity=0)  # fmt: skip
    for name in names:
        problem = load(name, DEV)
        row = []
        for n in (1, 4):
            for rep in range(2):  # (the second plan of either kind is the one recorded: same candidates, warm allocator)
                planner = CppFlowPlanner(settings, problem.robot, seed_provider=TrackingSeedProvider(seed=0), device_optimizer=True,
                                         n_search_paths=n)  # fmt: skip
                try:
                    res = planner.generate_plan(problem)
                    torch.cuda.synchronize()
                    err = None
                except (RuntimeError, AssertionError) as e:  # e.g. the device loop's row limit at n * T rows: recorded, not worked around
                    res, err = None, str(e).splitlines()[0][:60]
            row.append((res, err))
        (r1, e1), (r4, e4) = row
        a = f"{str(r1.plan.is_valid):>6s} {r1.debug_info.get('n_optimization_steps', 0):3d} {1e3 * r1.timing.dp_search:7.2f} {1e3 * r1.timing.optimizer:8.2f}" if r1 else f"refused: {e1}"  # fmt: skip
        b = (f"{str(r4.plan.is_valid):>6s} {r4.debug_info.get('n_search_paths', 1):5d} {r4.debug_info.get('optimized_path_index', 0):4d} "
             f"{r4.debug_info.get('n_optimization_steps', 0):3d} {1e3 * r4.timing.dp_search:7.2f} {1e3 * r4.timing.optimizer:8.2f}") if r4 else f"refused: {e4}"  # fmt: skip
        lines.append(f"{name:26s} {problem.n_timesteps:4d} | {a} | {b}")
        print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dp_nbest.txt"))
    ap.add_argument("--problems", default=",".join(README_PROBLEMS + FIXTURES))
    ap.add_argument("--k", type=int, default=175)
    ap.add_argument("--tmax", type=float, default=5.0)
    ap.add_argument("--skip-plans", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "dp_nbest_bench.py measures on the MI355X"
    lines = [f"# scripts/dp_nbest_bench.py   torch {torch.__version__}, device {torch.cuda.get_device_name(0)}"]
    selection_times(lines)
    optimiser_times(lines)
    if not a.skip_plans:
        plans(lines, [n for n in a.problems.split(",") if n], a.k, a.tmax)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
