"""Obstacle scenes: more cuboids than a robot handle holds (`CPPF_MAX_OBSTACLES` = 8), kept in device memory and checked against
all rows in one call (`Robot.scene_env_collisions`, csrc/kernels_scene.h; up to `CPPF_MAX_SCENE_OBSTACLES` = 4096).

`ObstacleScene` is the device-side form of `Problem.obstacles_cuboids` / `obstacles_Tcuboids`; `select_active_obstacles` is how a
planner turns the scene kernel's per-cuboid minimum distance into the <= 8 cuboids the optimiser's kernels take.
"""

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

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
    # was returned, and the grid it was built on ("voxel_m", "dims", "origin", "rounds": 1 + the coarsening rounds taken)
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
