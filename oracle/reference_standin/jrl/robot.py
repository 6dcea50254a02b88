"""jrl.robot.Robot as an adaptor over oracle/ref_torch.TorchRobot (TEST INFRASTRUCTURE ONLY).

The method names, argument order and result shapes are what the reference's call sites expect (cppflow/optimization_utils.py:652-731,
collision_detection.py:27-120, evaluation_utils.py:101-116).  The numbers behind them are this project's reading of the robot:
ref_torch's URDF-style kinematics and capsule distances on the canonical chain's constants (`canonical_spec`), in the dtype of the
configurations passed in.  The two distance Jacobians
are torch autograd over those distances in fp64, so that they share nothing with the analytic gradients of oracle/lmik_oracle.c.
"""

from typing import List, Optional, Tuple

import numpy as np
import torch

from oracle.ref_torch import TorchRobot, canonical_spec


class Robot:
    def __init__(self, spec):
        spec = canonical_spec(spec)
        self._spec = spec
        self._by_dtype = {dt: TorchRobot(spec, dtype=dt) for dt in (torch.float32, torch.float64)}
        t = self._by_dtype[torch.float64]
        self.name = spec.name
        self.formal_robot_name = spec.name
        self.ndof = t.ndof
        self.actuated_joints_limits: List[Tuple[float, float]] = list(t.actuated_joints_limits)
        self.revolute_joint_idxs = list(t.revolute_joint_idxs)
        self.prismatic_joint_idxs = list(t.prismatic_joint_idxs)
        self.n_self_collision_pairs = len(t.pairs)
        self.n_capsules = len(spec.capsules)
        self._mesh_obstacles: List[Tuple[torch.Tensor, torch.Tensor]] = []

    def __str__(self) -> str:
        return f"<stand-in Robot {self.name}>"

    @property
    def has_prismatic_joints(self) -> bool:
        return len(self.prismatic_joint_idxs) > 0

    def _t(self, x: torch.Tensor) -> TorchRobot:
        return self._by_dtype[x.dtype]

    # ---- kinematics -------------------------------------------------------------------------------------------------------
    def forward_kinematics(self, x: torch.Tensor, out_device=None, dtype=None) -> torch.Tensor:
        return self._t(x).forward_kinematics(x)

    def jacobian(self, x: torch.Tensor) -> torch.Tensor:
        return self._t(x).jacobian(x)

    def split_configs_to_revolute_and_prismatic(self, x: torch.Tensor):
        return x[:, self.revolute_joint_idxs], x[:, self.prismatic_joint_idxs]

    # ---- capsule distances and their Jacobians ------------------------------------------------------------------------------
    def self_collision_distances(self, x: torch.Tensor) -> torch.Tensor:
        """[n, n_pairs]"""
        return self._t(x).self_collision_distances(x)

    def env_collision_distances(self, x: torch.Tensor, cuboid, Tcuboid) -> torch.Tensor:
        """[n, n_capsules] against one axis-aligned cuboid (cuboid[6] = the two corners about Tcuboid's translation)"""
        return self._t(x).env_collision_distances(x, *self._world_corners(cuboid, Tcuboid, x.dtype))

    @staticmethod
    def _world_corners(cuboid, Tcuboid, dtype):
        """The box's world-frame corners formed in fp32 (translation + extent, as the library and tests/helpers.box_corners form them),
        then handed on as a cuboid about the origin: in fp64 the same sum differs by an fp32 rounding, 1e-8 m"""
        c, t = torch.as_tensor(cuboid).to(torch.float32), torch.as_tensor(Tcuboid).to(torch.float32)[:3, 3]
        return torch.cat([t + c[:3], t + c[3:]]).to(dtype), torch.zeros((4, 4), dtype=dtype)

    @staticmethod
    def _row_jacobian(fn, x: torch.Tensor) -> torch.Tensor:
        """d fn(x)[i, p] / d x[i, :] -> [n, P, ndof]; row i of fn depends on row i of x alone, so one backward pass per column p"""
        xd = x.detach().to(torch.float64).requires_grad_(True)
        with torch.enable_grad():
            dist = fn(xd)
            cols = [torch.autograd.grad(dist[:, p].sum(), xd, retain_graph=True)[0] for p in range(dist.shape[1])]
        return torch.stack(cols, dim=1).to(x.dtype)

    def self_collision_distances_jacobian(self, x: torch.Tensor) -> torch.Tensor:
        """[n, n_pairs, ndof] (call site: optimization_utils.py:669-672)"""
        t = self._by_dtype[torch.float64]
        return self._row_jacobian(t.self_collision_distances, x)

    def env_collision_distances_jacobian(self, x: torch.Tensor, cuboid, Tcuboid) -> torch.Tensor:
        """[n, n_capsules, ndof] (call site: optimization_utils.py:709-712)"""
        t = self._by_dtype[torch.float64]
        corners, origin = self._world_corners(cuboid, Tcuboid, torch.float64)
        return self._row_jacobian(lambda xd: t.env_collision_distances(xd, corners, origin), x)

    # ---- what the reference asks klampt's meshes: answered by the capsules, as cppflow_amd.optimization_utils.x_is_valid does --------
    def set_mesh_standin_obstacles(self, cuboids, Tcuboids) -> None:
        self._mesh_obstacles = list(zip(cuboids, Tcuboids))

    def config_self_collides(self, x: np.ndarray) -> bool:
        q = torch.as_tensor(np.asarray(x)).reshape(1, self.ndof)
        return bool(self.self_collision_distances(q).min() < 0)

    def config_collides_with_env(self, x: np.ndarray, obstacle_idx: int, return_detailed: bool = False) -> bool:
        assert not return_detailed
        q = torch.as_tensor(np.asarray(x)).reshape(1, self.ndof)
        cuboid, Tcuboid = self._mesh_obstacles[obstacle_idx]
        return bool(self.env_collision_distances(q, cuboid, Tcuboid).min() < 0)
