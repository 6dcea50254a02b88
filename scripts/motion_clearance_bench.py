#!/usr/bin/env python3
"""What certifying the motion between waypoints costs (developer tool; writes profiles/motion_clearance.txt).

    python scripts/motion_clearance_bench.py [--out profiles/motion_clearance.txt] [--processes 3] [--step-timeout 120]

Panda, 1 x 256 and 8 x 256 rows (a random walk at the planner's spacing, |dq| <= 0.03 rad per joint) at level 6 against 0, 64 and 1024
cuboids (polar recipe: radius 0.30 .. 0.95 m, z 0 .. 1.3 m, half-sizes 0.5 .. 2 cm -- a voxelised scene), reach 0.05 m:
  motion   Robot.motion_clearance (cppf_motion_clearance: three launches), status + min_clear + hit_node;
  nodes    the only other route today: the [S (W-1) 65, d] node tensor materialised with torch, then cppf_collision_masks (min_self) and
           cppf_scene_env_collisions (min_env) on it.  That route yields node minima only and cannot certify per pair.
Both through the Python methods (their output and workspace allocations included, from torch's caching allocator), device events
around one call, median of 30 after 5 warm-up calls in a process; the figure written down is the median over fresh processes, each
started under `timeout`; the first process that fails or times out ends the run (nothing more is started on the GPU)."""

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

    for S, W in SHAPES:
        prs = np.random.RandomState(1)
        q = np.zeros((S, W, ch.ndof))
        q[:, 0] = [0.0, -0.4, 0.0, -2.0, 0.0, 1.6, 0.8]
        for t in range(1, W):
            q[:, t] = np.clip(q[:, t - 1] + prs.uniform(-0.03, 0.03, size=(S, ch.ndof)), ch.lo + 0.05, ch.hi - 0.05)
        qd = torch.tensor(q, dtype=torch.float32, device=DEV)
        f = (torch.arange(65, device=DEV, dtype=torch.float32) / 64).view(1, 1, 65, 1)
        for O in N_OBS:
            lo, hi = lo_all[:O].contiguous(), hi_all[:O].contiguous()

            def motion():
                return rb.motion_clearance(qd, lo, hi, level=LEVEL, reach=REACH)

            def nodes_route():
                a_, b_ = qd[:, :-1, None, :], qd[:, 1:, None, :]
                nodes = torch.addcmul(a_, f, b_ - a_).reshape(1, -1, ch.ndof).contiguous()
                m_self = rb.collision_masks(nodes, want_min_dists=True, only=("self",))["min_self"]
                m_env = rb.scene_env_collisions(nodes, lo, hi, reach=REACH, want=("env_mask", "min_env"))["min_env"]
                return torch.minimum(m_self, m_env).view(S, W - 1, 65).amin(dim=2)

            got = motion()
            nodes_route()
            torch.cuda.synchronize()
            status = got["status"]
            rec = dict(S=S, W=W, n_obs=O, motion_us=event_us(motion), nodes_us=event_us(nodes_route),
                       certified=int((status == 1).sum()), hit=int((status == 2).sum()), undecided=int((status == 0).sum()))  # fmt: skip
            print("MOTION_BENCH " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_clearance.txt"))
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
            sys.exit(f"motion_clearance_bench: process {i} ended with status {p.returncode}; stopping")
        runs.append([json.loads(ln.split(" ", 1)[1]) for ln in p.stdout.splitlines() if ln.startswith("MOTION_BENCH ")])
        print(f"process {i}: {len(runs[-1])} shapes", flush=True)
    lines = [f"# scripts/motion_clearance_bench.py: panda, level {LEVEL}, reach {REACH} m; us per call, device events, median of 30 in a process,",
             f"# median over {a.processes} fresh processes.  motion = cppf_motion_clearance; nodes = torch node tensor + cppf_collision_masks +",
             "# cppf_scene_env_collisions on it (node minima only, no certificate).  certified / hit / undecided: transitions, of S (W - 1).",
             f"{'rows':>9s} {'n_obs':>6s} {'motion_us':>10s} {'nodes_us':>10s} {'certified':>9s} {'hit':>5s} {'undecided':>9s}"]  # fmt: skip
    for k, first in enumerate(runs[0]):
        recs = [r[k] for r in runs]
        lines.append(f"{first['S']:>3d} x {first['W']:<3d} {first['n_obs']:6d} {statistics.median(r['motion_us'] for r in recs):10.1f} "
                     f"{statistics.median(r['nodes_us'] for r in recs):10.1f} {first['certified']:9d} {first['hit']:5d} {first['undecided']:9d}")  # fmt: skip
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
