#!/usr/bin/env python3
"""What one scene call costs beside the only route without it (developer tool; writes profiles/scene_collisions.txt).

    python scripts/scene_bench.py [--out profiles/scene_collisions.txt] [--procs 3] [--windows 15]

Rows: Panda candidates tracked along a 256-waypoint path (`Robot.track_paths`; the path is the FK of a smooth joint-space curve, so the
script needs no data file) -- 175 x 256 rows (a planner's candidate stage) and 1 x 256 rows (one plan).  Scenes: O = 64 and 1024
cuboids of the recipe of tests/test_gpu_scene.py (polar centres, radius 0.30 - 0.95 m, z 0 - 1.3 m, half-sizes 0.02 - 0.06 m,
numpy.default_rng(0)).

Variants, all on preallocated buffers through the C ABI, alternating inside one process:
  scene 0.05 / scene inf   cppf_scene_env_collisions with all four outputs at reach = 0.05 / +inf (three launches)
  scene mask               the same call with env_mask only (no square roots, reach irrelevant)
  chunks of 8              ceil(O / 8) x (cppf_set_obstacles + cppf_collision_masks with env_mask and min_env), each round into
                           buffers of its own; the OR / min over the rounds that would make it the same answer is NOT included
Timing: device events around a window of `inner` calls back to back (10 for the scene calls, 1 for the chunked route at O = 1024, whose
128 launches are a window by themselves), per-call time = window / inner; per process the median over the windows after 3 warm-up
windows of every variant; every case runs in `--procs` fresh processes one after the other, the record holds the median of the process
medians and their range.  The scene call's answer is checked against the chunked route's (mask and min, bit for bit) in every process
before anything is timed."""

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
CASES = [(175, 64), (175, 1024), (1, 64), (1, 1024)]  # (candidates x 256 waypoints, cuboids)
T = 256


def recipe(n, seed=0):
    import numpy as np

    rng = np.random.default_rng(seed)
    r, a, z = rng.uniform(0.30, 0.95, n), rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 1.3, n)
    half = rng.uniform(0.02, 0.06, (n, 3)).astype(np.float32)
    cub = np.concatenate([-half, half], axis=1).astype(np.float32)
    Ts = np.zeros((n, 4, 4), dtype=np.float32)
    Ts[:, :3, :3] = np.eye(3, dtype=np.float32)
    Ts[:, 0, 3], Ts[:, 1, 3], Ts[:, 2, 3] = r * np.cos(a), r * np.sin(a), z
    return list(cub), list(Ts)


def child(k, O, windows):
    import ctypes

    import numpy as np
    import torch

    from cppflow_amd import _hip
    from cppflow_amd.robots import get_robot
    from cppflow_amd.scene import ObstacleScene

    rb = get_robot("panda")
    dev = torch.device(DEV)
    lo_j = np.array([l for l, _ in rb.actuated_joints_limits])
    hi_j = np.array([u for _, u in rb.actuated_joints_limits])
    s = np.linspace(0, 1, T)[:, None]
    curve = 0.5 * (lo_j + hi_j) + 0.25 * (hi_j - lo_j) * np.sin(2 * np.pi * (s * np.arange(1, 8) / 7 + np.arange(7) / 7))
    target = rb.forward_kinematics(torch.tensor(curve, dtype=torch.float32, device=dev)).contiguous()
    q = rb.track_paths(target, k, seed=0)["x"].contiguous()
    n = k * T
    cub, Ts = recipe(O)
    sc = ObstacleScene.from_cuboids(cub, Ts, dev)
    lib, h, st = _hip.lib(), rb._handle(dev), torch.cuda.current_stream(dev).cuda_stream
    nb = ctypes.c_size_t(0)
    _hip.check(lib.cppf_scene_workspace_bytes(n, O, ctypes.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    mask, mn = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, device=dev)
    near, om = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(O, device=dev)

    def scene(reach, full=True):
        _hip.check(lib.cppf_scene_env_collisions(h, q.data_ptr(), k, T, sc.lo.data_ptr(), sc.hi.data_ptr(), O, reach, mask.data_ptr(),
                                                 mn.data_ptr() if full else None, near.data_ptr() if full else None,
                                                 om.data_ptr() if full else None, ws.data_ptr(), nb.value, st))  # fmt: skip

    rounds = (O + 7) // 8
    packed = [rb._pack_obstacles(cub[i : i + 8], Ts[i : i + 8]) for i in range(0, O, 8)]
    cmask, cmin = torch.empty((rounds, n), dtype=torch.uint8, device=dev), torch.empty((rounds, n), device=dev)

    def chunks():
        for i, (c, rt) in enumerate(packed):
            _hip.check(lib.cppf_set_obstacles(h, c.shape[0], _hip.fptr(c), _hip.fptr(rt)))
            _hip.check(lib.cppf_collision_masks(h, q.data_ptr(), k, T, None, cmask[i].data_ptr(), None, None, None, cmin[i].data_ptr(), st))

    # same answer first
    scene(float("inf"))
    chunks()
    torch.cuda.synchronize()
    assert torch.equal(mask, cmask.max(dim=0).values) and torch.equal(mn.view(torch.int32), cmin.min(dim=0).values.view(torch.int32))
    share = float(mask.float().mean())

    variants = {"scene 0.05": (lambda: scene(0.05), 10), "scene inf": (lambda: scene(float("inf")), 10),
                "scene mask": (lambda: scene(0.0, full=False), 10), "chunks of 8": (chunks, 10 if O <= 64 else 1)}  # fmt: skip
    times = {name: [] for name in variants}
    for w in range(3 + windows):
        for name, (fn, inner) in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            if w >= 3:
                times[name].append(a.elapsed_time(b) * 1e3 / inner)
    _hip.check(lib.cppf_set_obstacles(h, 0, None, None))
    print("RESULT " + json.dumps({"k": k, "O": O, "colliding_share": share, "rounds": rounds,
                                  "device": f"torch {torch.__version__}, device {torch.cuda.get_device_name(0)}",
                                  "median_us": {name: statistics.median(v) for name, v in times.items()}}), flush=True)  # fmt: skip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_collisions.txt"))
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--child", nargs=2, type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.windows)
        return
    # (this process starts the measuring ones and never touches the GPU itself)
    lines = ["# scripts/scene_bench.py   DEVICE",
             f"# Panda, tracked candidates x {T} waypoints; us per call, device events; median of {a.procs} fresh processes' medians over "
             f"{a.windows} windows (lowest .. highest process median); 'chunks of 8' = ceil(O/8) x (set_obstacles + collision_masks), "
             "without the OR / min that would combine its rounds",
             f"{'rows':>9s} {'O':>5s} {'hit':>5s} | {'scene 0.05':>26s} | {'scene inf':>26s} | {'scene mask':>26s} | {'chunks of 8':>28s} | "
             f"{'chunks / scene 0.05':>19s} {'/ inf':>7s}"]  # fmt: skip
    for k, O in CASES:
        runs = []
        for _ in range(a.procs):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(k), str(O), "--windows", str(a.windows)],
                                 capture_output=True, text=True, timeout=400)  # fmt: skip
            if out.returncode != 0:
                raise SystemExit(f"child ({k}, {O}) failed with {out.returncode}:\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
            runs.append(json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
        lines[0] = lines[0].replace("DEVICE", runs[0]["device"])
        cell = {}
        for name in runs[0]["median_us"]:
            v = [r["median_us"][name] for r in runs]
            cell[name] = (statistics.median(v), min(v), max(v))
        f = lambda c: f"{c[0]:9.1f} ({c[1]:6.1f} ..{c[2]:7.1f})"  # noqa: E731
        lines.append(f"{k:3d} x {T:3d} {O:5d} {100 * runs[0]['colliding_share']:4.0f}% | {f(cell['scene 0.05'])} | {f(cell['scene inf'])} | "
                     f"{f(cell['scene mask'])} | {f(cell['chunks of 8'])}   | {cell['chunks of 8'][0] / cell['scene 0.05'][0]:19.2f} "
                     f"{cell['chunks of 8'][0] / cell['scene inf'][0]:7.2f}")  # fmt: skip
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
