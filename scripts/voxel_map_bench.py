#!/usr/bin/env python3
"""What fusing frames into a voxel map and building the scene from it cost beside the one-frame route (developer tool; writes
profiles/voxel_map.txt).

    python scripts/voxel_map_bench.py [--out profiles/voxel_map.txt] [--procs 3] [--windows 15]

Input: the 480 x 640 depth image, camera and 128 x 128 x 64 grid of 2 cm of scripts/voxel_scene_bench.py.  Further views are the same
image from a camera turned about the world's z axis through the grid's middle by 12, -12 and 24 degrees: other surfaces, overlapping
the first in part, as when a manipulator looks at its workspace from several poses.

Variants, all on preallocated buffers through the C ABI, alternating inside one process:
  scene_from_depth       cppf_scene_from_depth, filter off: the one-frame route every other line is compared with
  add_depth              cppf_voxel_map_add_depth of the first view into a map that already holds it
  from_map xy / xyz      cppf_scene_from_map (min_frames = 1) of a map that holds the first view
  add + from_map xyz     the two calls back to back: a frame in, a scene out
Timing as in scripts/voxel_scene_bench.py: device events around a window of 10 calls, per-call time = window / 10; per process the
median over the windows after 3 warm-up windows of every variant; `--procs` fresh processes, the record holds the median of the
process medians and their range.  Box counts: boxes in total (not cut by a capacity) of the x/y list and the z-merged list for the
first view, the first two and all four, at min_frames = 1, and for all four at min_frames = 2."""

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import voxel_scene_bench as one_frame  # noqa: E402  (the frame, the camera and the grid)

DEV = "cuda:0"
H_, W_ = one_frame.H_, one_frame.W_
ORIGIN, VOXEL, DIMS = one_frame.ORIGIN, one_frame.VOXEL, one_frame.DIMS
TURNS_DEG = (0.0, 12.0, -12.0, 24.0)


def views():
    """[(depth, intrinsics, cam_to_world)]: the first is scripts/voxel_scene_bench.py's frame"""
    import numpy as np

    depth, intr, T = one_frame.frame()
    mid = np.array([ORIGIN[0] + 0.5 * DIMS[0] * VOXEL, ORIGIN[1] + 0.5 * DIMS[1] * VOXEL, 0.0])
    out = []
    for deg in TURNS_DEG:
        a = np.deg2rad(deg)
        Rz = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        Tv = np.eye(4)
        Tv[:3, :3] = Rz @ T[:3, :3].astype(np.float64)
        Tv[:3, 3] = Rz @ (T[:3, 3].astype(np.float64) - mid) + mid
        out.append((depth, intr, Tv.astype(np.float32)))
    return out


def child(windows):
    import ctypes

    import numpy as np
    import torch

    from cppflow_amd import _hip

    dev = torch.device(DEV)
    lib, st = _hip.lib(), torch.cuda.current_stream(dev).cuda_stream
    z_min, z_max = 0.3, 3.0
    vs = views()
    depth = torch.tensor(vs[0][0], device=dev)
    cams = [((ctypes.c_float * 4)(*intr.tolist()), (ctypes.c_float * 12)(*np.concatenate([T[:3, :3].reshape(9), T[:3, 3]]).tolist()))
            for _, intr, T in vs]  # fmt: skip

    grid = _hip.VoxelGrid((ctypes.c_float * 3)(*ORIGIN), VOXEL, (ctypes.c_int32 * 3)(*DIMS))
    nb = ctypes.c_size_t(0)
    _hip.check(lib.cppf_voxel_scene_workspace_bytes(ctypes.byref(grid), 0, ctypes.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    mb = ctypes.c_size_t(0)
    _hip.check(lib.cppf_voxel_map_bytes(ctypes.byref(grid), ctypes.byref(mb)))
    held, scratch = (torch.empty(mb.value, dtype=torch.uint8, device=dev) for _ in range(2))
    lo, hi = (torch.empty((4096, 3), device=dev) for _ in range(2))
    counts = torch.empty(8, dtype=torch.int32, device=dev)

    def clear(m):
        _hip.check(lib.cppf_voxel_map_clear(m.data_ptr(), mb.value, ctypes.byref(grid), st))

    def add(m, view=0):
        k, rt = cams[view]
        _hip.check(lib.cppf_voxel_map_add_depth(None, depth.data_ptr(), H_, W_, k, rt, z_min, z_max, ctypes.byref(grid), None, 0, 0.03,
                                                m.data_ptr(), mb.value, counts.data_ptr(), ws.data_ptr(), nb.value, st))  # fmt: skip

    def from_map(m, merge, min_frames=1):
        _hip.check(lib.cppf_scene_from_map(m.data_ptr(), mb.value, ctypes.byref(grid), min_frames, merge, 4096, lo.data_ptr(), hi.data_ptr(),
                                           counts.data_ptr(), ws.data_ptr(), nb.value, st))  # fmt: skip

    def from_depth():
        k, rt = cams[0]
        _hip.check(lib.cppf_scene_from_depth(None, depth.data_ptr(), H_, W_, k, rt, z_min, z_max, ctypes.byref(grid), None, 0, 0.03, 4096,
                                             lo.data_ptr(), hi.data_ptr(), counts.data_ptr(), ws.data_ptr(), nb.value, st))  # fmt: skip

    def read():
        torch.cuda.synchronize()
        return counts.cpu().tolist()

    # box counts: 1, 2 and 4 fused views
    boxes = {}
    from_depth()
    boxes["scene_from_depth"] = read()
    clear(held)
    for n_views in (1, 2, 3, 4):
        add(held, n_views - 1)
        if n_views == 3:
            continue
        row = {}
        for name, merge in (("xy", _hip.VOXEL_MERGE_XY), ("xyz", _hip.VOXEL_MERGE_XYZ)):
            from_map(held, merge)
            row[name] = read()
        boxes[f"{n_views} view(s), min_frames 1"] = row
    row = {}
    for name, merge in (("xy", _hip.VOXEL_MERGE_XY), ("xyz", _hip.VOXEL_MERGE_XYZ)):
        from_map(held, merge, 2)
        row[name] = read()
    boxes["4 view(s), min_frames 2"] = row
    clear(held)
    add(held)
    clear(scratch)
    add(scratch)

    def both():
        add(scratch)
        from_map(scratch, _hip.VOXEL_MERGE_XYZ)

    variants = {"scene_from_depth": from_depth, "add_depth": lambda: add(scratch), "from_map xy": lambda: from_map(held, _hip.VOXEL_MERGE_XY),
                "from_map xyz": lambda: from_map(held, _hip.VOXEL_MERGE_XYZ), "add + from_map xyz": both}  # fmt: skip
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
    print("RESULT " + json.dumps({"device": f"torch {torch.__version__}, device {torch.cuda.get_device_name(0)}", "boxes": boxes,
                                  "median_us": {name: statistics.median(v) for name, v in times.items()}}), flush=True)  # fmt: skip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_map.txt"))
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
    lines = [f"# scripts/voxel_map_bench.py   {runs[0]['device']}",
             f"# {H_} x {W_} depth image -> {DIMS[0]} x {DIMS[1]} x {DIMS[2]} grid of {VOXEL * 100:g} cm; us per call, device events, windows of 10; "
             f"median of {a.procs} fresh processes' medians over {a.windows} windows (lowest .. highest process median)",
             f"{'variant':>20s} | {'us per call':>28s} | over scene_from_depth"]  # fmt: skip
    ref = statistics.median([r["median_us"]["scene_from_depth"] for r in runs])
    for name in runs[0]["median_us"]:
        v = [r["median_us"][name] for r in runs]
        lines.append(f"{name:>20s} | {statistics.median(v):9.1f} ({min(v):7.1f} ..{max(v):8.1f}) | {statistics.median(v) - ref:+8.1f}")
    lines.append("# boxes in total (no capacity applied) and cells, x/y list against z-merged list:")
    b = runs[0]["boxes"]
    c = b["scene_from_depth"]
    lines.append(f"# {'cppf_scene_from_depth':>26s} | {c[0]:6d} boxes                | {c[2]:6d} cells")
    for name, row in b.items():
        if name == "scene_from_depth":
            continue
        xy, xyz = row["xy"], row["xyz"]
        lines.append(f"# {name:>26s} | {xy[0]:6d} xy  {xyz[0]:6d} xyz ({xyz[0] / max(xy[0], 1):5.2f}) | {xy[2]:6d} cells of {xy[3]:6d} seen, "
                     f"{xy[7]} frames")  # fmt: skip
    print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
