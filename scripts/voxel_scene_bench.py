#!/usr/bin/env python3
"""What building a scene from sensor data costs beside the only other route (developer tool; writes profiles/voxel_scene.txt).

    python scripts/voxel_scene_bench.py [--out profiles/voxel_scene.txt] [--procs 3] [--windows 15]

Input: a synthetic 480 x 640 depth image (a rippled surface 0.6 - 2.1 m in front of a camera that looks along world +y from
(0, -1.2, 0.64); focal length 525 px; 2 % of the pixels invalid) and the cloud of its first 300 000 valid back-projected pixels, into a
128 x 128 x 64 grid of 2 cm at origin (-1.28, -1.28, 0).  Part of the surface lies outside the grid, as in a real frame.

Variants, all on preallocated buffers through the C ABI, alternating inside one process:
  depth / points            cppf_scene_from_depth / cppf_scene_from_points, filter off (five launches)
  depth self / points self  the same with n_self = 1 (Panda at the middle of its joint ranges, margin 3 cm; six launches)
  no input                  cppf_scene_from_points with n_points = 0: clear, row count, scan, emit -- what the grid alone costs
  torch cells               the other route's device half: floor, bounds mask, torch.unique of the linear cell index
Timing: device events around a window of 10 calls back to back, per-call time = window / 10; per process the median over the windows
after 3 warm-up windows of every variant; every case runs in `--procs` fresh processes, the record holds the median of the process
medians and their range.  Once per process, by the wall clock: `Robot.scene_from_depth` (allocation, the call, the one counts
copy), and the other route to the end -- torch cells, the cells to the host, the Python list of per-cuboid tensors,
`cuboid_corners` over it (what `ObstacleScene.from_cuboids` does before it refuses more than 4096 cuboids) and the upload.  One cuboid
per cell, no merging: the record holds the cell count beside the box count."""

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
H_, W_ = 480, 640
ORIGIN, VOXEL, DIMS = (-1.28, -1.28, 0.0), 0.02, (128, 128, 64)
N_CLOUD = 300_000


def frame():
    import numpy as np

    v, u = np.mgrid[0:H_, 0:W_].astype(np.float64)
    depth = (1.2 + 0.6 * np.sin(u / 90.0) * np.cos(v / 70.0) + 0.3 * v / H_).astype(np.float32)
    rng = np.random.default_rng(0)
    depth.reshape(-1)[rng.choice(H_ * W_, size=H_ * W_ // 50, replace=False)] = 0.0
    intr = np.array([525.0, 525.0, 319.5, 239.5], dtype=np.float32)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = [[1, 0, 0], [0, 0, 1], [0, -1, 0]]  # camera x -> world x, camera y (down) -> world -z, camera z -> world y
    T[:3, 3] = (0.0, -1.2, 0.64)
    return depth, intr, T


def child(windows):
    import ctypes

    import numpy as np
    import torch

    from cppflow_amd import _hip
    from cppflow_amd.robots import get_robot
    from cppflow_amd.scene import cuboid_corners

    rb = get_robot("panda")
    dev = torch.device(DEV)
    lib, h, st = _hip.lib(), rb._handle(dev), torch.cuda.current_stream(dev).cuda_stream
    depth_h, intr, T = frame()
    z_min, z_max = 0.3, 3.0
    depth = torch.tensor(depth_h, device=dev)
    # the cloud: the same pixels, back-projected with torch (not bit for bit the library's points, and it need not be)
    vv, uu = torch.meshgrid(torch.arange(H_, device=dev, dtype=torch.float32), torch.arange(W_, device=dev, dtype=torch.float32), indexing="ij")
    cam = torch.stack([(uu - intr[2]) * depth / intr[0], (vv - intr[3]) * depth / intr[1], depth], dim=-1).reshape(-1, 3)
    world = cam @ torch.tensor(T[:3, :3], device=dev).T + torch.tensor(T[:3, 3], device=dev)
    cloud = world[(depth.reshape(-1) > z_min) & (depth.reshape(-1) < z_max)][:N_CLOUD].contiguous()
    assert cloud.shape[0] == N_CLOUD
    q = torch.tensor([[0.5 * (l + u) for l, u in rb.actuated_joints_limits]], dtype=torch.float32, device=dev)

    grid = _hip.VoxelGrid((ctypes.c_float * 3)(*ORIGIN), VOXEL, (ctypes.c_int32 * 3)(*DIMS))
    nb = ctypes.c_size_t(0)
    _hip.check(lib.cppf_voxel_scene_workspace_bytes(ctypes.byref(grid), 1, ctypes.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    lo, hi = (torch.empty((4096, 3), device=dev) for _ in range(2))
    counts = torch.empty(8, dtype=torch.int32, device=dev)
    k = (ctypes.c_float * 4)(*intr.tolist())
    rt = (ctypes.c_float * 12)(*np.concatenate([T[:3, :3].reshape(9), T[:3, 3]]).tolist())

    def tail(n_self):
        return (ctypes.byref(grid), q.data_ptr() if n_self else None, n_self, 0.03, 4096, lo.data_ptr(), hi.data_ptr(), counts.data_ptr(),
                ws.data_ptr(), nb.value, st)  # fmt: skip

    def from_depth(n_self=0):
        _hip.check(lib.cppf_scene_from_depth(h, depth.data_ptr(), H_, W_, k, rt, z_min, z_max, *tail(n_self)))

    def from_points(n_self=0, n=N_CLOUD):
        _hip.check(lib.cppf_scene_from_points(h, cloud.data_ptr(), n, *tail(n_self)))

    o = torch.tensor(ORIGIN, device=dev)
    dims = torch.tensor(DIMS, device=dev)

    def torch_cells():
        idx = torch.floor((cloud - o) / VOXEL).to(torch.int64)
        ok = ((idx >= 0) & (idx < dims)).all(dim=1)
        idx = idx[ok]
        return torch.unique((idx[:, 2] * DIMS[1] + idx[:, 1]) * DIMS[0] + idx[:, 0])

    stats = {}
    for name, fn in (("depth", from_depth), ("points", from_points), ("depth self", lambda: from_depth(1)), ("points self", lambda: from_points(1))):
        fn()
        torch.cuda.synchronize()
        stats[name] = counts.cpu().tolist()
    stats["torch cells"] = [0, 0, int(torch_cells().numel()), 0, 0, 0, 0, 0]  # (floor of a quotient, not the planes: may differ by a cell)

    variants = {"depth": from_depth, "points": from_points, "depth self": lambda: from_depth(1), "points self": lambda: from_points(1),
                "no input": lambda: from_points(0, 0), "torch cells": torch_cells}  # fmt: skip
    times = {name: [] for name in variants}
    for w in range(3 + windows):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(10):
                fn()
            b.record()
            torch.cuda.synchronize()
            if w >= 3:
                times[name].append(a.elapsed_time(b) * 1e3 / 10)

    def wall(fn, reps=3):
        out = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(out)

    def other_route():
        lin = torch_cells().cpu().numpy()
        ix, iy, iz = lin % DIMS[0], (lin // DIMS[0]) % DIMS[1], lin // (DIMS[0] * DIMS[1])
        c_lo = np.stack([ix, iy, iz], axis=1).astype(np.float32) * np.float32(VOXEL) + np.asarray(ORIGIN, dtype=np.float32)
        cub = [torch.from_numpy(np.concatenate([c, c + np.float32(VOXEL)])) for c in c_lo]
        Ts = [torch.eye(4) for _ in cub]
        l, u = cuboid_corners(cub, Ts)
        return torch.from_numpy(l).to(dev), torch.from_numpy(u).to(dev)

    sensed = {}

    def method():
        sensed["scene"] = rb.scene_from_depth(depth, intr, T, z_min, z_max, ORIGIN, VOXEL, DIMS)

    wall_ms = {"Robot.scene_from_depth": wall(method), "torch + host list": wall(other_route)}
    st_ = sensed["scene"].stats
    stats["returned"] = [st_["boxes_total"], st_["boxes_written"], st_["occupied_cells"], st_["rounds"], st_["voxel_m"]]
    print("RESULT " + json.dumps({"device": f"torch {torch.__version__}, device {torch.cuda.get_device_name(0)}", "counts": stats,
                                  "median_us": {name: statistics.median(v) for name, v in times.items()}, "wall_ms": wall_ms}), flush=True)  # fmt: skip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_scene.txt"))
    ap.add_argument("--procs", type=int, default=3)
    ap.add_argument("--windows", type=int, default=15)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.windows)
        return
    # (this process starts the measuring ones and never touches the GPU itself)
    runs = []
    for _ in range(a.procs):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--windows", str(a.windows)], capture_output=True,
                             text=True, timeout=400)  # fmt: skip
        if out.returncode != 0:
            raise SystemExit(f"child failed with {out.returncode}:\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
        runs.append(json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    lines = [f"# scripts/voxel_scene_bench.py   {runs[0]['device']}",
             f"# {H_} x {W_} depth image / {N_CLOUD} points -> {DIMS[0]} x {DIMS[1]} x {DIMS[2]} grid of {VOXEL * 100:g} cm; us per call, device events, "
             f"windows of 10; median of {a.procs} fresh processes' medians over {a.windows} windows (lowest .. highest process median)",
             f"{'variant':>12s} | {'us per call':>28s} | {'boxes':>6s} {'cells':>6s} {'kept':>7s} {'outside':>7s} {'invalid':>7s} {'self':>6s}"]  # fmt: skip
    for name in runs[0]["median_us"]:
        v = [r["median_us"][name] for r in runs]
        c = runs[0]["counts"].get(name)
        c = c if c is None or len(c) == 8 else None
        tail = f"{c[0]:6d} {c[2]:6d} {c[3]:7d} {c[4]:7d} {c[5]:7d} {c[6]:6d}" if c else ""
        lines.append(f"{name:>12s} | {statistics.median(v):9.1f} ({min(v):7.1f} ..{max(v):8.1f}) | {tail}")
    lines.append("# by the wall clock, ms, median of 3 per process (median of the processes; lowest .. highest):")
    for name in runs[0]["wall_ms"]:
        v = [r["wall_ms"][name] for r in runs]
        lines.append(f"# {name:>24s} {statistics.median(v):9.2f} ({min(v):8.2f} ..{max(v):9.2f})")
    r0 = runs[0]["counts"]["returned"]
    lines.append(f"# Robot.scene_from_depth returned {r0[0]} cuboids from {r0[2]} cells after {r0[3]} round(s), voxel {r0[4] * 100:g} cm "
                 "(a round more than 1: the list at the finer voxel exceeded 4096 cuboids and the build was repeated coarser)")
    lines.append(f"# the other route ends in {runs[0]['counts']['points'][2]} cuboids, one per cell: ObstacleScene.from_cuboids refuses more than 4096")
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
