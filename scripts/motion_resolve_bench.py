#!/usr/bin/env python3
"""What resolving the motion test by adaptive bisection costs next to the uniform test (developer tool; writes
profiles/motion_resolve.txt).

    python scripts/motion_resolve_bench.py [--out profiles/motion_resolve.txt] [--processes 3] [--step-timeout 120]

The shapes of scripts/motion_clearance_bench.py: Panda, 1 x 256 and 8 x 256 rows (a random walk at the planner's spacing, |dq| <= 0.03
rad per joint) against 0, 64 and 1024 cuboids (polar recipe: radius 0.30 .. 0.95 m, z 0 .. 1.3 m, half-sizes 0.5 .. 2 cm), reach 0.05 m:
  uniform  Robot.motion_clearance(level=6)            (cppf_motion_clearance: three launches; the baseline, unchanged by this work)
  resolve  Robot.motion_resolve(0, 16, 512)           (cppf_motion_resolve: one launch, one wavefront per transition)
Both through the Python methods (their output and workspace allocations included, from torch's caching allocator), device events
around one call, median of 30 after 5 warm-up calls in a process; the figure written down is the median over fresh processes, each
started under `timeout`; the first process that fails or times out ends the run (nothing more is started on the GPU).  Beside the
times: how the transitions ended under either test, and the mean number of interval tests per transition (the uniform test: 64)."""

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
SHAPES = ((1, 256), (8, 256))
N_OBS = (0, 64, 1024)
LEVEL, REACH = 6, 0.05
RESOLVE = (0, 16, 512)  # start_level, max_depth, max_frontier


def child():
    import numpy as np
    import torch

    from cppflow_amd.robots import get_robot

    rb = get_robot("panda")
    ch = rb.chain
    rng = np.random.default_rng(0)
    r, a, z = rng.uniform(0.30, 0.95, 1024), rng.uniform(0, 2 * np.pi, 1024), rng.uniform(0, 1.3, 1024)
    half = rng.uniform(0.005, 0.02, (1024, 3))
    centre = np.stack([r * np.cos(a), r * np.sin(a), z], axis=1)
    lo_all = torch.tensor(centre - half, dtype=torch.float32, device=DEV)
    hi_all = torch.tensor(centre + half, dtype=torch.float32, device=DEV)

    def event_us(fn, warmup=5, reps=30):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return statistics.median(ts)

    def counts(status):
        return [int((status == v).sum()) for v in (1, 2, 0, 4)]  # certified, hit, undecided, overflowed

    for S, W in SHAPES:
        prs = np.random.RandomState(1)
        q = np.zeros((S, W, ch.ndof))
        q[:, 0] = [0.0, -0.4, 0.0, -2.0, 0.0, 1.6, 0.8]
        for t in range(1, W):
            q[:, t] = np.clip(q[:, t - 1] + prs.uniform(-0.03, 0.03, size=(S, ch.ndof)), ch.lo + 0.05, ch.hi - 0.05)
        qd = torch.tensor(q, dtype=torch.float32, device=DEV)
        for O in N_OBS:
            lo, hi = lo_all[:O].contiguous(), hi_all[:O].contiguous()

            def uniform():
                return rb.motion_clearance(qd, lo, hi, level=LEVEL, reach=REACH)

            def resolve():
                return rb.motion_resolve(qd, lo, hi, start_level=RESOLVE[0], max_depth=RESOLVE[1], max_frontier=RESOLVE[2], reach=REACH)

            uni, res = uniform(), resolve()
            torch.cuda.synchronize()
            rec = dict(S=S, W=W, n_obs=O, uniform_us=event_us(uniform), resolve_us=event_us(resolve), uniform=counts(uni["status"]),
                       resolve=counts(res["status"]), tests=float(res["n_tested"].double().mean()), deepest=int(res["depth"].max()))  # fmt: skip
            print("RESOLVE_BENCH " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_resolve.txt"))
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds one measuring process may take")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child()
    runs = []
    for i in range(a.processes):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), sys.executable, os.path.abspath(__file__), "--child"]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(f"motion_resolve_bench: process {i} ended with status {p.returncode}; stopping")
        runs.append([json.loads(ln.split(" ", 1)[1]) for ln in p.stdout.splitlines() if ln.startswith("RESOLVE_BENCH ")])
        print(f"process {i}: {len(runs[-1])} shapes", flush=True)
    lines = [f"# scripts/motion_resolve_bench.py: panda, reach {REACH} m; us per call, device events, median of 30 in a process, median over",
             f"# {a.processes} fresh processes.  uniform = cppf_motion_clearance(level = {LEVEL}), 64 interval tests per transition; resolve =",
             f"# cppf_motion_resolve{RESOLVE}.  c / h / u / o: transitions certified / hit / undecided / overflowed, of S (W - 1); tests: the",
             "# mean n_tested per transition; deepest: the largest depth any transition ended at.",
             f"{'rows':>9s} {'n_obs':>6s} {'uniform_us':>10s} {'resolve_us':>10s} {'uniform c/h/u':>16s} {'resolve c/h/u/o':>20s} {'tests':>7s} {'deepest':>7s}"]  # fmt: skip
    for k, first in enumerate(runs[0]):
        recs = [r[k] for r in runs]
        u, v = first["uniform"], first["resolve"]
        lines.append(f"{first['S']:>3d} x {first['W']:<3d} {first['n_obs']:6d} {statistics.median(r['uniform_us'] for r in recs):10.1f} "
                     f"{statistics.median(r['resolve_us'] for r in recs):10.1f} {f'{u[0]}/{u[1]}/{u[2]}':>16s} "
                     f"{f'{v[0]}/{v[1]}/{v[2]}/{v[3]}':>20s} {first['tests']:7.1f} {first['deepest']:7d}")  # fmt: skip
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
