#!/usr/bin/env python3
"""Seed-stage time of the one-launch tracking kernel (cppf_track_paths) against the per-waypoint loop of LmIkSeedProvider, and the
segment count S that sets the tracking kernel's sequential depth.

    python scripts/track_sweep.py [--problem fetch__hello] [--k 175] [--out profiles/track_sweep.txt]

A lane runs  n_restart + (T / S - 1) n_track  LM iterations in sequence; with S = 1, no tolerances and no restarts that count is fixed,
so the launch time over it is the latency of one LM iteration of a lone lane (k = 175 lanes: three wavefronts on three compute units).
Times are medians of 5 calls between two synchronizes, after one warm-up call."""

import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cppflow_amd.planners import LmIkSeedProvider, TrackingSeedProvider  # noqa: E402
from scripts.plan_table import load  # noqa: E402


def timed(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problem", default="fetch__hello")
    ap.add_argument("--k", type=int, default=175)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_sweep.txt"))
    a = ap.parse_args()
    problem = load(a.problem, "cuda:0")
    rb, T, k = problem.robot, problem.n_timesteps, a.k
    tgt = problem.target_path.contiguous()
    lines = [f"# scripts/track_sweep.py: {a.problem} (T = {T}, {rb.name}, d = {rb.ndof}), k = {k}; {torch.cuda.get_device_name(0)}"]
    ms_loop = timed(lambda: LmIkSeedProvider(seed=0)(problem, k))
    lines.append(f"LmIkSeedProvider (T = {T} launches of k rows: 40 steps, then 6 per waypoint)      {ms_loop:9.3f} ms")
    lines.append("track_paths, no tolerances, R = 0 (fixed work): S, ms, LM iterations per lane, us per iteration")
    for S in (1, 2, 4, 8, 16, 32, 64):
        ms = timed(lambda: rb.track_paths(tgt, k, n_segments=S, n_restart=40, n_track=6))
        iters = 40 + (-(-T // S) - 1) * 6  # the longest segment
        lines.append(f"  S = {S:3d}  {ms:9.3f} ms  {iters:5d} iterations  {1e3 * ms / iters:7.3f} us / iteration")
    for S in (1, 4, 8, 16, None):
        ms = timed(lambda: TrackingSeedProvider(seed=0, n_segments=S)(problem, k))
        S = S if S is not None else f"default = {-(-T // TrackingSeedProvider().waypoints_per_segment)}"
        lines.append(f"TrackingSeedProvider(n_segments = {S}) (tolerances 5e-5 m / 5e-4 rad, R = 2)   {ms:9.3f} ms"
                     f"  (loop / this = {ms_loop / ms:5.2f})")  # fmt: skip
    print("\n".join(lines))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
