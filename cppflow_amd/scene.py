"""Obstacle scenes: more cuboids than a robot handle holds (`CPPF_MAX_OBSTACLES` = 8), kept in device memory and checked against
all rows in one call (`Robot.scene_env_collisions`, csrc/kernels_scene.h; up to `CPPF_MAX_SCENE_OBSTACLES` = 4096).

`ObstacleScene` is the device-side form of `Problem.obstacles_cuboids` / `obstacles_Tcuboids`; `select_active_obstacles` is how a
planner turns the scene kernel's per-cuboid minimum distance into the <= 8 cuboids the optimiser's kernels take.
"""

import ctypes
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from cppflow_amd import _hip
from cppflow_amd._marshal import _require_device_tensor, sized_buffer
from cppflow_amd.robot_model import MAX_OBSTACLES

MAX_SCENE_OBSTACLES = 4096  # CPPF_MAX_SCENE_OBSTACLES
DEFAULT_SCENE_ACTIVATION_DISTANCE_M = 0.25  # a setting (how far from the seed path a cuboid is still handed to the optimiser)


def cuboid_corners(cuboids: Sequence, Tcuboids: Sequence):
    """World-frame corners (lo [O,3], hi [O,3], fp32 numpy) of axis-aligned cuboids, formed exactly as `cppf_set_obstacles` forms
    them: translation + local corner, one fp32 addition each.  Rotated cuboids are refused, as there."""
    from cppflow_amd.robots import Robot

    packed = Robot._pack_obstacles(cuboids, Tcuboids)
    if packed is None:
        return np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.float32)
    cub, rt = packed
    eye = np.eye(3, dtype=np.float32).reshape(9)
    assert bool((np.abs(rt[:, :9] - eye) < 1e-8).all()), "only axis-aligned cuboids are supported (R must be I)"
    assert bool((cub[:, :3] <= cub[:, 3:]).all()), "cuboid min corner > max corner"
    lo = (rt[:, 9:] + cub[:, :3]).astype(np.float32)
    hi = (rt[:, 9:] + cub[:, 3:]).astype(np.float32)
    return np.ascontiguousarray(lo), np.ascontiguousarray(hi)


VOXEL_COUNT_NAMES = ("boxes_total", "boxes_written", "occupied_cells", "kept_points", "outside_points", "invalid_points",
                     "self_points")  # counts[0..6] of cppf_scene_from_points / cppf_scene_from_depth  # fmt: skip


@dataclass
class ObstacleScene:
    lo: torch.Tensor  # [O, 3] float32, world-frame min corners
    hi: torch.Tensor  # [O, 3] float32, world-frame max corners
    # a scene built from sensor data (`Robot.scene_from_points` / `scene_from_depth`) only: VOXEL_COUNT_NAMES of the round that
    # was returned, and the grid it was built on ("voxel_m", "dims", "origin", "rounds": 1 + the coarsening rounds taken); of a
    # `VoxelMap.scene`: what its docstring lists
    stats: Optional[dict] = None

    @property
    def n_obstacles(self) -> int:
        return int(self.lo.shape[0])

    def as_problem_obstacles(self):
        """(cuboids, Tcuboids) as `Problem.obstacles_cuboids` / `obstacles_Tcuboids` hold them: cuboid = [lo, hi] ([6], host), T the
        4x4 identity.  `cuboid_corners` forms 0 + lo and 0 + hi, so the loader path gives these corners back bit for bit (a plane is
        never -0).  One device-to-host copy."""
        cub = torch.cat([self.lo, self.hi], dim=1).detach().to("cpu", torch.float32).contiguous()
        eye = torch.eye(4, dtype=torch.float32)
        return [cub[i] for i in range(cub.shape[0])], [eye.clone() for _ in range(cub.shape[0])]

    @classmethod
    def from_cuboids(cls, cuboids: Sequence, Tcuboids: Sequence, device=None) -> "ObstacleScene":
        lo, hi = cuboid_corners(cuboids, Tcuboids)
        assert lo.shape[0] <= MAX_SCENE_OBSTACLES, f"a scene holds at most {MAX_SCENE_OBSTACLES} cuboids, got {lo.shape[0]}"
        dev = torch.device(device) if device is not None else torch.device("cpu")
        return cls(torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev))

    def to(self, device) -> "ObstacleScene":
        return ObstacleScene(self.lo.to(device), self.hi.to(device), self.stats)


MAP_ADD_COUNT_NAMES = ("frame_cells", "kept_points", "outside_points", "invalid_points", "self_points",
                       "frames")  # counts[2..7] of cppf_voxel_map_add_points / cppf_voxel_map_add_depth  # fmt: skip
MAP_SCENE_COUNT_NAMES = ("boxes_total", "boxes_written", "occupied_cells", "seen_cells")  # counts[0..3] of cppf_scene_from_map


class VoxelMap:
    """Per-cell hit counts of a voxel grid, fused over frames on the device (`Robot.voxel_map`; include/cppflow_hip.h, "Scenes fused
    over frames").  Owns the map tensor -- a 16-byte header { frames, 0, 0, 0 } and one uint8 counter per cell of the padded grid --
    and the workspaces of its calls.  A counter counts the FRAMES in which its cell held at least one kept point (saturating at 255),
    so `scene(min_frames=2)` drops what only one view ever saw.  Counters only grow until `clear()`."""

    def __init__(self, robot, origin, voxel_m: float, dims, device):
        self.robot = robot
        self.device = torch.device(device)
        assert self.device.type == "cuda", f"a VoxelMap lives on the MI355X, not on '{self.device}' (no CPU fallback)"
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.origin = tuple(float(v) for v in origin)
        self.voxel_m = float(voxel_m)
        self.dims = tuple(int(v) for v in dims)
        assert len(self.origin) == 3 and len(self.dims) == 3, "origin and dims have three entries"
        self._grid = _hip.VoxelGrid((_hip._f * 3)(*self.origin), self.voxel_m, (_hip._i32 * 3)(*self.dims))
        self._map = sized_buffer("cppf_voxel_map_bytes", self.device, ctypes.byref(self._grid))
        # one workspace for every call: that of an add with the most self-filter configurations serves the others
        self._work = sized_buffer("cppf_voxel_scene_workspace_bytes", self.device, ctypes.byref(self._grid), _hip.VOXEL_MAX_SELF)
        self._add_counts = torch.zeros((8,), dtype=torch.int32, device=self.device)
        self.clear()

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def clear(self) -> None:
        """every counter and `frames` to zero (one launch)"""
        with torch.cuda.device(self.device):  # (the map's calls without a handle launch on the current device)
            _hip.check(_hip.lib().cppf_voxel_map_clear(self._map.data_ptr(), self._map.numel(), ctypes.byref(self._grid), self._stream()))
            self._add_counts.zero_()

    def _add(self, call, q_self, self_margin_m: float) -> None:
        q_self, n_self, q_ptr, handle = self.robot._voxel_self(q_self, self.device)
        tail = (ctypes.byref(self._grid), q_ptr, n_self, float(self_margin_m), self._map.data_ptr(), self._map.numel(),
                self._add_counts.data_ptr(), self._work.data_ptr(), self._work.numel(), self._stream())  # fmt: skip
        with torch.cuda.device(self.device):
            _hip.check(call(handle, tail))

    def add_points(self, points: torch.Tensor, q_self: Optional[torch.Tensor] = None, self_margin_m: float = 0.03) -> None:
        """one frame from a world-frame point cloud [n, 3] (device); the arguments are `Robot.scene_from_points`'s.  No
        device-to-host copy: `last_counts()` fetches what the frame did."""
        points = _require_device_tensor(points, "points")
        assert points.dim() == 2 and points.shape[1] == 3, f"points must be [n, 3], is {tuple(points.shape)}"
        assert points.device == self.device, "points must be on the map's device"
        n = int(points.shape[0])
        self._add(lambda handle, tail: _hip.lib().cppf_voxel_map_add_points(handle, points.data_ptr() if n else None, n, *tail),
                  q_self, self_margin_m)  # fmt: skip

    def add_depth(self, depth: torch.Tensor, intrinsics, cam_to_world, z_min: float, z_max: float,
                  q_self: Optional[torch.Tensor] = None, self_margin_m: float = 0.03) -> None:
        """one frame from a depth image [H, W] (device, fp32 metres); the arguments are `Robot.scene_from_depth`'s.  No
        device-to-host copy."""
        depth, h, w, k, rt = self.robot._voxel_camera(depth, intrinsics, cam_to_world)
        assert depth.device == self.device, "depth must be on the map's device"
        self._add(lambda handle, tail: _hip.lib().cppf_voxel_map_add_depth(handle, depth.data_ptr() if h * w else None, h, w,
                                                                           _hip.fptr(k), _hip.fptr(rt), float(z_min), float(z_max), *tail),
                  q_self, self_margin_m)  # fmt: skip

    def last_counts(self) -> dict:
        """what the last add did (MAP_ADD_COUNT_NAMES; all zero before the first): one device-to-host copy"""
        return dict(zip(MAP_ADD_COUNT_NAMES, self._add_counts.cpu().tolist()[2:]))

    @property
    def frames(self) -> int:
        """the frames added since the last clear (one device-to-host copy of the header)"""
        return int(self._map[:4].view(torch.int32).item())

    def counts_tensor(self) -> torch.Tensor:
        """the counters as a [nz, ny, nxp] uint8 VIEW of the map, nxp = 64 ceil(nx / 64); columns x >= nx are, and must stay, 0"""
        nx, ny, nz = self.dims
        return self._map[16:].view(nz, ny, (nx + 63) // 64 * 64)

    def scene(self, min_frames: int = 1, merge_z: bool = True, max_cuboids: int = MAX_SCENE_OBSTACLES) -> ObstacleScene:
        """The cells counted in at least `min_frames` (1 .. 255) frames as an `ObstacleScene` of at most `max_cuboids` cuboids, merged
        along x and y (`cppf_scene_from_points`'s list) and, with `merge_z`, along z as well.  Its `.stats`: MAP_SCENE_COUNT_NAMES,
        "frames", "min_frames", "merge_z" and the grid.  One device-to-host copy (the counts).  A truncated scene is never returned:
        more boxes than `max_cuboids` raise RuntimeError.  There is no coarsening round as `Robot.scene_from_points` has one: a map
        cannot be voxelised again from points that are gone -- raise `min_frames`, or keep a second, coarser map beside this one."""
        cap = int(max_cuboids)
        assert 0 <= cap <= _hip.MAX_SCENE_OBSTACLES, f"max_cuboids must be in 0 .. {_hip.MAX_SCENE_OBSTACLES}"
        assert 1 <= int(min_frames) <= 255, "min_frames must be in 1 .. 255"
        lo = torch.empty((cap, 3), dtype=torch.float32, device=self.device)
        hi = torch.empty((cap, 3), dtype=torch.float32, device=self.device)
        counts = torch.empty((8,), dtype=torch.int32, device=self.device)
        merge = _hip.VOXEL_MERGE_XYZ if merge_z else _hip.VOXEL_MERGE_XY
        with torch.cuda.device(self.device):
            _hip.check(_hip.lib().cppf_scene_from_map(self._map.data_ptr(), self._map.numel(), ctypes.byref(self._grid), int(min_frames),
                                                      merge, cap, lo.data_ptr(), hi.data_ptr(), counts.data_ptr(), self._work.data_ptr(),
                                                      self._work.numel(), self._stream()))  # fmt: skip
        c = counts.cpu().tolist()  # (the one device-to-host copy)
        stats = dict(zip(MAP_SCENE_COUNT_NAMES, c[:4]), frames=c[7], min_frames=int(min_frames), merge_z=bool(merge_z),
                     voxel_m=self.voxel_m, dims=self.dims, origin=self.origin)  # fmt: skip
        if c[0] > cap:
            raise RuntimeError(f"the map gives {c[0]} boxes, more than max_cuboids = {cap} ({c[2]} occupied cells at min_frames = "
                               f"{int(min_frames)}, merge_z = {bool(merge_z)}, {c[7]} frames): a truncated scene is never returned")  # fmt: skip
        return ObstacleScene(lo[: c[1]].clone(), hi[: c[1]].clone(), stats)


def problem_with_scene(problem, scene: ObstacleScene):
    """`problem` with `scene` as its obstacles (a new Problem on the same robot; the old one is untouched).  The planner, `collision_masks`
    and `motion_clearance` then read the scene as they read any other; the new problem's scene cache is seeded with the device
    tensors `scene` already holds, and is rebuilt from the lists by `Problem.scene` wherever that does not apply (another device)."""
    import dataclasses

    cuboids, Tcuboids = scene.as_problem_obstacles()
    obstacles = [dict(x=float(c[0] + c[3]) / 2, y=float(c[1] + c[4]) / 2, z=float(c[2] + c[5]) / 2, size_x=float(c[3] - c[0]),
                      size_y=float(c[4] - c[1]), size_z=float(c[5] - c[2])) for c in cuboids]  # fmt: skip
    new = dataclasses.replace(problem, obstacles=obstacles, obstacles_cuboids=cuboids, obstacles_Tcuboids=Tcuboids, active_obstacles=None)
    dev = scene.lo.device
    if dev.type == "cuda":
        dev = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
    new.__dict__["_scene_cache"] = {(str(dev), new.n_obstacles): ObstacleScene(scene.lo, scene.hi, scene.stats)}  # (Problem.scene's key)
    return new


def select_active_obstacles(obs_min, max_active: int = MAX_OBSTACLES, first: Optional[Sequence[int]] = None) -> List[int]:
    """The up-to-`max_active` cuboids with the smallest FINITE `obs_min` (ties to the lower index), in ascending index order.
    `first`: indices that are taken before any other, whatever their `obs_min` (cuboids a result was found to hit).  Pure host."""
    v = obs_min.detach().cpu().numpy() if isinstance(obs_min, torch.Tensor) else np.asarray(obs_min)
    v = v.reshape(-1)
    assert max_active >= 0
    chosen: List[int] = []
    for i in first or ():
        i = int(i)
        assert 0 <= i < v.shape[0], f"obstacle index {i} out of range"
        if i not in chosen and len(chosen) < max_active:
            chosen.append(i)
    order = sorted((i for i in range(v.shape[0]) if math.isfinite(float(v[i])) and i not in chosen), key=lambda i: (float(v[i]), i))
    chosen += order[: max(0, max_active - len(chosen))]
    return sorted(chosen)
