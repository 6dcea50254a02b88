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


@dataclass
class ObstacleScene:
    lo: torch.Tensor  # [O, 3] float32, world-frame min corners
    hi: torch.Tensor  # [O, 3] float32, world-frame max corners

    @property
    def n_obstacles(self) -> int:
        return int(self.lo.shape[0])

    @classmethod
    def from_cuboids(cls, cuboids: Sequence, Tcuboids: Sequence, device=None) -> "ObstacleScene":
        lo, hi = cuboid_corners(cuboids, Tcuboids)
        assert lo.shape[0] <= MAX_SCENE_OBSTACLES, f"a scene holds at most {MAX_SCENE_OBSTACLES} cuboids, got {lo.shape[0]}"
        dev = torch.device(device) if device is not None else torch.device("cpu")
        return cls(torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev))

    def to(self, device) -> "ObstacleScene":
        return ObstacleScene(self.lo.to(device), self.hi.to(device))


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
