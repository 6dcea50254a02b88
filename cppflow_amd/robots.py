"""`Robot`: the duck type the reference's hot path reads off `jrl.robot.Robot`, backed by the HIP library.

Attributes / methods mirrored (reference call sites):
  ndof, name, formal_robot_name, actuated_joints_limits, revolute_joint_idxs, prismatic_joint_idxs,
  has_prismatic_joints, split_configs_to_revolute_and_prismatic        cppflow/optimization_utils.py:228-234, 825-832;
                                                                       cppflow/search.py:46-51, 119-121
  forward_kinematics(x, out_device=, dtype=)                           cppflow/optimization_utils.py:811
  jacobian(x)                                                          cppflow/optimization.py:74
  self_collision_distances(x)                                          cppflow/collision_detection.py:65
  env_collision_distances(x, cuboid, Tcuboid)                          cppflow/collision_detection.py:40
  clamp_to_joint_limits(x), sample_joint_angles(n)                     tests/optimization_test.py:82, 135

Every compute method takes CUDA (ROCm) float32 tensors and launches a hand-written gfx950 kernel through the C ABI on
torch's current stream.  CPU tensors are rejected: this package has no CPU path.
"""

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from cppflow_amd import _hip
from cppflow_amd._marshal import (
    _check_summary_buffer, _ptr, _require_device_tensor, _require_output_tensor, _scene_boxes, _stream_ptr, device_packed_views,
    fill_lm_outputs, optional_outputs, paths_tensor, query_size, rows_and_target, rows_tensor, sized_buffer,
)  # fmt: skip
from cppflow_amd.packed_rows import PACKED_BYTES_PER_ROW
from cppflow_amd.robot_model import CanonicalChain, RobotSpec, canonicalize, urdf_forward_kinematics
from cppflow_amd.robot_zoo import ROBOT_SPECS
from cppflow_amd.scene import VOXEL_COUNT_NAMES, ObstacleScene, VoxelMap

# the per-row arguments of cppf_seed_summary, in the order of its signature (each a view of the packed buffer)
_SEED_SUMMARY_ROW_ARGS = ("ext_cost", "pos_err_m", "rot_err_rad", "self_mask", "env_mask", "jlim_mask")


class Robot:
    PACKED_BYTES_PER_ROW = PACKED_BYTES_PER_ROW  # (cppflow_amd/packed_rows.py)

    def __init__(self, spec: RobotSpec, specialize: Optional[bool] = None):
        """`specialize` (default: on unless CPPF_SPECIALIZE=0): a robot that is not one of the shipped tables gets its kernels
        compiled for it with hipRTC when its first handle is created (a few seconds once; the code object is cached on disk)."""
        import os

        self.specialize: bool = (os.environ.get("CPPF_SPECIALIZE", "1") != "0") if specialize is None else bool(specialize)
        self.spec: RobotSpec = spec
        self.chain: CanonicalChain = canonicalize(spec)
        self.name: str = spec.name
        self.formal_robot_name: str = spec.formal_name
        self.ndof: int = self.chain.ndof
        self.actuated_joints_limits: List[Tuple[float, float]] = [
            (float(l), float(u)) for l, u in zip(self.chain.lo, self.chain.hi)
        ]
        self.revolute_joint_idxs: List[int] = [j for j in range(self.ndof) if self.chain.jtype[j] == 0]
        self.prismatic_joint_idxs: List[int] = [j for j in range(self.ndof) if self.chain.jtype[j] == 1]
        self.n_capsules: int = self.chain.n_capsules
        self.n_collision_pairs: int = self.chain.n_pairs
        self.collision_capsule_names: List[str] = list(self.chain.cap_names)
        # jrl's ordered map link name -> capsule; column i of env_collision_distances is its i-th key
        # (cppflow/collision_detection.py:137-142).  Values: [p0 (3), p1 (3), radius] in the link's canonical frame.
        self._collision_capsules_by_link: Dict[str, torch.Tensor] = {}
        for c, link_name in enumerate(self.chain.cap_names):
            key = link_name if link_name not in self._collision_capsules_by_link else f"{link_name}#{c}"
            self._collision_capsules_by_link[key] = torch.tensor(
                [*self.chain.cap_p0[c], *self.chain.cap_p1[c], self.chain.cap_r[c]], dtype=torch.float32
            )
        self._desc = _hip.chain_to_desc(self.chain)
        self._handles: Dict[int, ctypes.c_void_p] = {}
        self._tuning: Dict[int, int] = {}  # cppf_debug_set switches, re-applied to every handle this Robot creates
        self._obstacles: Optional[Tuple[np.ndarray, np.ndarray]] = None
        self._jl_padding: Optional[Tuple[np.ndarray, np.ndarray]] = None

    # ---- static properties ------------------------------------------------------------------------------------------
    @property
    def has_prismatic_joints(self) -> bool:
        return len(self.prismatic_joint_idxs) > 0

    def __str__(self) -> str:
        return f"<Robot[{self.name}] ndof={self.ndof} capsules={self.n_capsules} pairs={self.n_collision_pairs}>"

    def split_configs_to_revolute_and_prismatic(self, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return x[:, self.revolute_joint_idxs], x[:, self.prismatic_joint_idxs]

    def sample_joint_angles(self, n: int) -> np.ndarray:
        lo, hi = self.chain.lo, self.chain.hi
        return np.random.uniform(lo, hi, size=(n, self.ndof))

    def link_frame_at_zero(self, link_name: str) -> np.ndarray:
        """4x4 world transform of a named link at q = 0 (host, fp64).  Used for `path_offset_frame`
        (reference cppflow/data_type_utils.py:65-73, there via klampt)."""
        return urdf_forward_kinematics(self.spec, np.zeros(self.ndof), link=link_name)

    # ---- handle management ---------------------------------------------------------------------------------------------
    def debug_set(self, key: str, value: Optional[int] = None) -> None:
        """Test / tuning switch of THIS robot's handles (include/cppflow_hip_debug.h; `None` restores the default).  Per
        handle: no other Robot in the process is affected."""
        k = _hip.TUNE_KEYS[key]
        self._tuning[k] = _hip.TUNE_DEFAULT if value is None else int(value)
        for h in self._handles.values():
            _hip.check(_hip.lib().cppf_debug_set(h, k, self._tuning[k]))

    def _handle(self, device: torch.device) -> ctypes.c_void_p:
        idx = device.index if device.index is not None else torch.cuda.current_device()
        h = self._handles.get(idx)
        if h is None:
            out = ctypes.c_void_p()
            _hip.check(_hip.lib().cppf_robot_create(ctypes.byref(self._desc), idx, ctypes.byref(out)))
            h = out
            self._handles[idx] = h
            for k, v in self._tuning.items():
                _hip.check(_hip.lib().cppf_debug_set(h, k, v))
            self._apply_obstacles(h)
            self._apply_jl_padding(h)
            if self.specialize and _hip.lib().cppf_robot_specialization(h) < 0:
                # a description that matches none of the generated tables: compile-time tables through hipRTC (cached on disk)
                rc = _hip.lib().cppf_robot_specialize(h, None)
                if rc != _hip.CPPF_OK:
                    import warnings

                    warnings.warn(
                        f"robot '{self.name}': run-time specialisation failed, running the generic kernels: "
                        + _hip.lib().cppf_last_error().decode("utf-8", "replace")[:500]
                    )
        return h

    def _call(self, entry: str, dev: torch.device, *args) -> None:
        """The entry point `entry` on this robot's handle for `dev`, with `args` between the handle and the stream.  The one place
        that holds for every such call that the stream is the current stream of the device the tensors live on, and that the return
        code is never dropped."""
        _hip.check(getattr(_hip.lib(), entry)(self._handle(dev), *args, _stream_ptr(dev)))

    def specialization(self, device=None) -> int:
        """>= 0: index of the generated table this robot runs; 1000: kernels compiled for it at run time (hipRTC); -1: generic."""
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        return int(_hip.lib().cppf_robot_specialization(self._handle(dev)))

    def __del__(self):
        try:
            for h in self._handles.values():
                _hip.lib().cppf_robot_destroy(h)
            self._handles = {}
        except Exception:
            pass

    def _apply_obstacles(self, h) -> None:
        if self._obstacles is None:
            _hip.check(_hip.lib().cppf_set_obstacles(h, 0, None, None))
        else:
            cub, rt = self._obstacles
            _hip.check(_hip.lib().cppf_set_obstacles(h, cub.shape[0], _hip.fptr(cub), _hip.fptr(rt)))

    def _apply_jl_padding(self, h) -> None:
        if self._jl_padding is None:
            _hip.check(_hip.lib().cppf_set_joint_limit_padding(h, None, None))
        else:
            lo, hi = self._jl_padding
            _hip.check(_hip.lib().cppf_set_joint_limit_padding(h, _hip.fptr(lo), _hip.fptr(hi)))

    @staticmethod
    def _pack_obstacles(cuboids: Sequence, Tcuboids: Sequence) -> Optional[Tuple[np.ndarray, np.ndarray]]:
        """Problem.obstacles_cuboids ([6] each) and obstacles_Tcuboids (4x4 each; only R and t are read -- element
        [3,3] is left 0 by the reference loader, cppflow/data_type_utils.py:120-124)."""
        if cuboids is None or len(cuboids) == 0:
            return None
        assert len(cuboids) == len(Tcuboids)
        cub = np.zeros((len(cuboids), 6), dtype=np.float32)
        rt = np.zeros((len(cuboids), 12), dtype=np.float32)
        for i, (c, T) in enumerate(zip(cuboids, Tcuboids)):
            c = c.detach().cpu().numpy() if isinstance(c, torch.Tensor) else np.asarray(c)
            T = T.detach().cpu().numpy() if isinstance(T, torch.Tensor) else np.asarray(T)
            cub[i] = c.astype(np.float32).reshape(6)
            rt[i, :9] = T[:3, :3].astype(np.float32).reshape(9)
            rt[i, 9:] = T[:3, 3].astype(np.float32)
        return cub, rt

    def set_obstacles(self, cuboids: Sequence, Tcuboids: Sequence) -> None:
        self._obstacles = self._pack_obstacles(cuboids, Tcuboids)
        for h in self._handles.values():
            self._apply_obstacles(h)

    def set_joint_limit_padding(self, eps_revolute: Optional[float], eps_prismatic: Optional[float]) -> None:
        """Padded limits exactly as cppflow/search.py:46-51 forms them: fp32 tensors, in-place += / -= of the scalar."""
        if eps_revolute is None:
            self._jl_padding = None
        else:
            lo = np.array([l for l, _ in self.actuated_joints_limits], dtype=np.float32)
            hi = np.array([u for _, u in self.actuated_joints_limits], dtype=np.float32)
            er, ep = np.float32(eps_revolute), np.float32(eps_prismatic)
            lo[self.prismatic_joint_idxs] += ep
            lo[self.revolute_joint_idxs] += er
            hi[self.prismatic_joint_idxs] -= ep
            hi[self.revolute_joint_idxs] -= er
            self._jl_padding = (lo, hi)
        for h in self._handles.values():
            self._apply_jl_padding(h)

    def padded_joint_limits(self) -> Optional[Tuple[np.ndarray, np.ndarray]]:
        return self._jl_padding

    def set_padded_joint_limits(self, padded: Optional[Tuple[np.ndarray, np.ndarray]]) -> None:
        """Install already-padded (lo, hi) fp32 arrays (or None to disable the joint-limit mask)."""
        if padded is None:
            self._jl_padding = None
        else:
            lo, hi = (np.ascontiguousarray(a, dtype=np.float32) for a in padded)
            assert lo.shape == (self.ndof,) and hi.shape == (self.ndof,)
            self._jl_padding = (lo, hi)
        for h in self._handles.values():
            self._apply_jl_padding(h)

    # ---- jrl-compatible compute methods --------------------------------------------------------------------------------
    def _x2d(self, x: torch.Tensor, name: str = "x") -> torch.Tensor:
        return rows_tensor(x, self.ndof, name)

    def forward_kinematics(self, x: torch.Tensor, out_device=None, dtype=None) -> torch.Tensor:
        x = self._x2d(x)
        poses = torch.empty((x.shape[0], 7), dtype=torch.float32, device=x.device)
        self._call("cppf_forward_kinematics", x.device, x.data_ptr(), x.shape[0], poses.data_ptr())
        if dtype is not None and dtype != torch.float32:
            poses = poses.to(dtype)
        if out_device is not None and torch.device(out_device) != poses.device:
            poses = poses.to(out_device)
        return poses

    def jacobian(self, x: torch.Tensor) -> torch.Tensor:
        x = self._x2d(x)
        J = torch.empty((x.shape[0], 6, self.ndof), dtype=torch.float32, device=x.device)
        self._call("cppf_jacobian", x.device, x.data_ptr(), x.shape[0], J.data_ptr())
        return J

    def self_collision_distances(self, x: torch.Tensor) -> torch.Tensor:
        x = self._x2d(x)
        d = torch.empty((x.shape[0], self.n_collision_pairs), dtype=torch.float32, device=x.device)
        self._call("cppf_self_collision_distances", x.device, x.data_ptr(), x.shape[0], d.data_ptr())
        return d

    def env_collision_distances(self, x: torch.Tensor, cuboid, Tcuboid) -> torch.Tensor:
        x = self._x2d(x)
        cub, rt = self._pack_obstacles([cuboid], [Tcuboid])
        d = torch.empty((x.shape[0], self.n_capsules), dtype=torch.float32, device=x.device)
        self._call("cppf_env_collision_distances", x.device, x.data_ptr(), x.shape[0], _hip.fptr(cub[0]), _hip.fptr(rt[0]), d.data_ptr())
        return d

    def self_collision_distances_jacobian(self, x: torch.Tensor, return_distances: bool = False):
        """[n, n_pairs, d] = d(self_collision_distances)/dq (jrl API; call site cppflow/optimization_utils.py:670)."""
        x = self._x2d(x)
        n = x.shape[0]
        J = torch.zeros((n, self.n_collision_pairs, self.ndof), dtype=torch.float32, device=x.device)
        dist = torch.empty((n, self.n_collision_pairs), dtype=torch.float32, device=x.device) if return_distances else None
        self._call("cppf_self_collision_distances_jacobian", x.device, x.data_ptr(), n, J.data_ptr(),
                   dist.data_ptr() if dist is not None else None)  # fmt: skip
        return (J, dist) if return_distances else J

    def env_collision_distances_jacobian(self, x: torch.Tensor, cuboid, Tcuboid, return_distances: bool = False):
        """[n, n_capsules, d] = d(env_collision_distances)/dq for ONE cuboid (jrl API; call site optimization_utils.py:710)."""
        x = self._x2d(x)
        n = x.shape[0]
        cub, rt = self._pack_obstacles([cuboid], [Tcuboid])
        J = torch.zeros((n, self.n_capsules, self.ndof), dtype=torch.float32, device=x.device)
        dist = torch.empty((n, self.n_capsules), dtype=torch.float32, device=x.device) if return_distances else None
        self._call("cppf_env_collision_distances_jacobian", x.device, x.data_ptr(), n, _hip.fptr(cub[0]), _hip.fptr(rt[0]), J.data_ptr(),
                   dist.data_ptr() if dist is not None else None)  # fmt: skip
        return (J, dist) if return_distances else J

    def clamp_to_joint_limits(self, x: torch.Tensor) -> torch.Tensor:
        """In place (and returned), like cppflow/optimization_utils.py:831-833."""
        x_c = self._x2d(x)
        assert x_c.data_ptr() == x.data_ptr(), "clamp_to_joint_limits mutates its argument: x must be contiguous"
        self._call("cppf_clamp_to_joint_limits", x.device, x.data_ptr(), x.shape[0])
        return x

    # ---- fused entry points ----------------------------------------------------------------------------------------------
    def pose_errors(self, x: torch.Tensor, target: torch.Tensor, want_current_poses: bool = True):
        """get_6d_pose_errors: returns (e [n,6,1], current_poses [n,7]).  `target` is [W,7] with n % W == 0."""
        x, target, n, W = rows_and_target(x, target, self.ndof)
        e = torch.empty((n, 6, 1), dtype=torch.float32, device=x.device)
        cur = torch.empty((n, 7), dtype=torch.float32, device=x.device) if want_current_poses else None
        self._call("cppf_pose_errors", x.device, x.data_ptr(), target.data_ptr(), n // W, W, e.data_ptr(),
                   cur.data_ptr() if cur is not None else None)  # fmt: skip
        return e, cur

    def lm_pose_steps(
        self,
        x: torch.Tensor,
        target: torch.Tensor,
        lm_lambda: float,
        alpha_position: float,
        alpha_rotation: float,
        n_steps: int = 1,
        clamp: bool = True,
        return_residual: bool = False,
        want_errors: bool = False,
        want_collisions: bool = False,
        want_min_dists: bool = False,
        x_out: Optional[torch.Tensor] = None,
        packed_out: Optional[torch.Tensor] = None,
        summary_out: Optional[torch.Tensor] = None,
        tol_pos_m: float = 0.0,
        tol_rot_rad: float = 0.0,
        want_iters: bool = False,
        shape: int = _hip.SHAPE_AUTO,
        solver: int = _hip.SOLVER_AUTO,
    ) -> Dict[str, torch.Tensor]:
        """K fused { levenberg_marquardt_only_pose ; clamp_to_joint_limits } iterations in ONE kernel launch, plus
        (optionally) pose-error metrics and collision masks / search cost of the result.  x is [S*W, d]; target [W, 7].

        `x_out` (may be `x` itself) and `packed_out` let a caller reuse buffers: `packed_out` is a uint8 tensor of
        `PACKED_BYTES_PER_ROW * n` bytes that receives ext_cost | pos_err_m | rot_err_rad (fp32 [n] each) then
        self_mask | env_mask | jlim_mask (u8 [n] each) back to back -- the single buffer one RCCL all-gather ships to
        every rank; it implies want_errors and want_collisions.  `summary_out` (fp32 [S,8], fields
        SEED_SUMMARY_FIELDS) receives the per-seed reduction of `seed_summary`, computed inside the same launch when
        W is 64, 128 or 256 and by a second kernel otherwise (which then needs the per-row outputs, i.e. `packed_out` or
        want_errors + want_collisions).

        `tol_pos_m` / `tol_rot_rad` (both or neither) switch on the in-launch early-out: rows already below tolerance at the
        start of an iteration are left untouched and a wavefront of such rows leaves the loop (cppflow/optimization.py:326-358
        stops the same way once the pose is valid); `want_iters` returns the per-row number of steps applied.  `shape` picks
        the kernel shape (`_hip.SHAPE_ROW`: one row per lane; `_hip.SHAPE_QUAD`: four lanes per row; default: by batch size);
        `solver` the precision of the damped solve: `_hip.SOLVER_AUTO` (default: the reference's dtype with the conditioning gate --
        rows whose fp32 solve is estimated to be off by more than 1e-5 in task space redo it in double precision),
        `_hip.SOLVER_F64` (every row in double precision: a verification mode, ~10x the iteration time) or `_hip.SOLVER_F32` (no gate)."""
        x, target, n, W = rows_and_target(x, target, self.ndof)
        out = _hip.LmOutputs()
        res, _ = fill_lm_outputs(out, x, W, x_out if x_out is not None else torch.empty_like(x), packed_out, None, summary_out)

        def on_request(key: str, dtype, *tail: int, field: Optional[str] = None) -> None:
            res[key] = torch.empty((n, *tail), dtype=dtype, device=x.device)
            setattr(out, field or key, res[key].data_ptr())

        if return_residual:
            on_request("J", torch.float32, 6, self.ndof, field="J_out")
            on_request("e", torch.float32, 6, 1, field="e_out")
        if want_errors and packed_out is None:
            on_request("pos_err_m", torch.float32)
            on_request("rot_err_rad", torch.float32)
        if want_collisions and packed_out is None:
            for k in ("self_mask", "env_mask", "jlim_mask"):
                on_request(k, torch.uint8)
            on_request("ext_cost", torch.float32)
            if want_min_dists:
                on_request("min_self", torch.float32)
                on_request("min_env", torch.float32)
        if want_iters:
            on_request("n_iters", torch.int32)
        prm = _hip.LmParams(float(lm_lambda), float(alpha_position), float(alpha_rotation), int(n_steps), int(bool(clamp)),
                            float(tol_pos_m), float(tol_rot_rad), int(shape), int(solver))
        self._call("cppf_lm_pose_steps", x.device, x.data_ptr(), target.data_ptr(), n // W, W, ctypes.byref(prm), ctypes.byref(out))
        return res

    def lm_launch_plan(self, x: torch.Tensor, target: torch.Tensor, lm_lambda: float, alpha_position: float,
                       alpha_rotation: float, n_steps: int, x_out: torch.Tensor, packed_out: Optional[torch.Tensor] = None,
                       clamp: bool = True, summary_out: Optional[torch.Tensor] = None,
                       shape: int = _hip.SHAPE_AUTO, solver: int = _hip.SOLVER_AUTO,
                       errors_out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> "LmLaunchPlan":  # fmt: skip
        """Pre-marshalled arguments for repeated fused launches over fixed buffers (what a planner loop or a benchmark
        holds on to): `plan.launch()` is then a single C call on torch's current stream, no Python-side allocation.
        `packed_out` (15 bytes per row: cost, pose errors, masks) makes it a launch with the collision stage; without it
        `errors_out` = (pos_err_m [n], rot_err_rad [n]) asks for the pose errors of the result alone."""
        return LmLaunchPlan(self, x, target, lm_lambda, alpha_position, alpha_rotation, n_steps, x_out, packed_out, clamp,
                            summary_out, shape, solver, errors_out)

    def lm_batch_plan(self, items: Sequence[dict], lm_lambda: float, alpha_position: float, alpha_rotation: float, n_steps: int,
                      clamp: bool = True, solver: int = _hip.SOLVER_AUTO) -> "LmBatchPlan":
        """Several INDEPENDENT problems of this robot in ONE fused launch (cppf_lm_batch_*; at most `_hip.MAX_BATCH`): what a planner
        serving several requests holds on to, and what a GPU that owns only a shard of the candidate seeds needs to fill the chip.
        Each item is a dict with `x` [S*W, d], `target` [W, 7], `x_out` [S*W, d] and optionally `packed_out` (15 bytes per row: cost,
        pose errors, masks -- makes it a launch with the collision stage), `summary_out` [S, 8], `errors_out` = (pos_err_m [n],
        rot_err_rad [n]).  Every problem's results are bit for bit those of `lm_pose_steps` / `lm_launch_plan` on it alone."""
        return LmBatchPlan(self, items, lm_lambda, alpha_position, alpha_rotation, n_steps, clamp, solver)

    def select_valid_seed(self, seed_summary: torch.Tensor, constraints, self_collisions_ignored: bool = False,
                          env_collisions_ignored: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x_is_valid's seed selection (cppflow/optimization_utils.py:856-909) over [S,8] per-seed summaries (one GPU's, or
        every rank's after the all-gather): int32 [4] on the device = (first valid seed or -1, number of valid seeds, seed of
        smallest summed external cost, 0).  `constraints` is a `Constraints` (max_allowed_* fields).
        Also accepts what one all-gather of [G, S_local, 8] buffers from `world` ranks leaves behind, as a 4-d tensor
        [world, G, S_local, 8]: the result is then int32 [G, 4], row g for the world * S_local seeds of step g."""
        s = _require_device_tensor(seed_summary, "seed_summary")
        assert s.dim() in (2, 4) and s.shape[-1] == 8, tuple(s.shape)
        n_chunks, n_groups, S_chunk = (1, 1, s.shape[0]) if s.dim() == 2 else tuple(s.shape[:3])
        if out is None:
            out = torch.empty(4 if s.dim() == 2 else (n_groups, 4), dtype=torch.int32, device=s.device)
        else:
            out = _require_output_tensor(out, "out", torch.int32)
            assert out.numel() == 4 * n_groups
        c = _hip.Constraints(float(constraints.max_allowed_position_error_cm), float(constraints.max_allowed_rotation_error_deg),
                             float(constraints.max_allowed_mjac_deg), float(constraints.max_allowed_mjac_cm),
                             int(bool(self_collisions_ignored)), int(bool(env_collisions_ignored)))  # fmt: skip
        self._call("cppf_select_valid_seed_gathered", s.device, s.data_ptr(), n_chunks, n_groups, S_chunk, ctypes.byref(c), out.data_ptr())
        return out

    def collision_masks(
        self, q: torch.Tensor, want_min_dists: bool = False, only: Optional[Sequence[str]] = None
    ) -> Dict[str, torch.Tensor]:
        """q [S, W, d] -> self_mask / env_mask / jlim_mask (bool [S,W]) and ext_cost (float [S,W]) in one launch, against
        the obstacles / limit padding last given to set_obstacles / set_joint_limit_padding.  `only` (subset of
        "self", "env", "jlim") restricts the work: the kernel skips what no requested output needs."""
        q, S, W = paths_tensor(q, self.ndof)
        dev = q.device
        parts = ("self", "env", "jlim") if only is None else tuple(only)
        assert set(parts) <= {"self", "env", "jlim"} and len(parts) > 0, parts
        res: Dict[str, torch.Tensor] = {}
        for part in parts:
            res[part + "_mask"] = torch.empty((S, W), dtype=torch.uint8, device=dev)
        if only is None:
            res["ext_cost"] = torch.empty((S, W), dtype=torch.float32, device=dev)
        if want_min_dists:
            if "self" in parts:
                res["min_self"] = torch.empty((S, W), dtype=torch.float32, device=dev)
            if "env" in parts:
                res["min_env"] = torch.empty((S, W), dtype=torch.float32, device=dev)
        self._call("cppf_collision_masks", dev, q.data_ptr(), S, W, _ptr(res, "self_mask"), _ptr(res, "env_mask"), _ptr(res, "jlim_mask"),
                   _ptr(res, "ext_cost"), _ptr(res, "min_self"), _ptr(res, "min_env"))  # fmt: skip
        for k in ("self_mask", "env_mask", "jlim_mask"):
            if k in res:
                res[k] = res[k].view(torch.bool)
        return res

    def scene_env_collisions(self, q: torch.Tensor, box_lo: torch.Tensor, box_hi: torch.Tensor, reach: float = float("inf"),
                             want: Sequence[str] = ("env_mask", "min_env", "nearest_obs", "obs_min")) -> Dict[str, torch.Tensor]:
        """q [S, W, d] (or [n, d]) against the O <= 4096 axis-aligned cuboids box_lo / box_hi [O, 3] (device, world-frame corners:
        `cppflow_amd.scene.ObstacleScene`) in one call (`cppf_scene_env_collisions`); the handle's own obstacles are not involved.
        env_mask (bool, always returned), min_env (float: the minimum distance where it is < reach, else +inf), nearest_obs (int32:
        the lowest cuboid index attaining it, else -1) are shaped like q without its last axis; obs_min [O] is the per-cuboid
        minimum over all rows where < reach, else +inf.  Asking for env_mask alone takes the form without square roots."""
        q = _require_device_tensor(q, "q")
        assert q.dim() in (2, 3) and q.shape[-1] == self.ndof, f"q must be [k, ntimesteps, {self.ndof}] or [n, {self.ndof}], is {tuple(q.shape)}"
        lead = tuple(q.shape[:-1])
        S, W = (1, lead[0]) if q.dim() == 2 else lead
        dev = q.device
        box_lo, box_hi, O = _scene_boxes(box_lo, box_hi, dev)
        spec = {"env_mask": torch.uint8, "min_env": torch.float32, "nearest_obs": torch.int32, "obs_min": (torch.float32, (O,))}
        res = optional_outputs((*want, "env_mask"), spec, lead, dev)
        work = sized_buffer("cppf_scene_workspace_bytes", dev, S * W, O)
        self._call("cppf_scene_env_collisions", dev, q.data_ptr(), S, W, box_lo.data_ptr(), box_hi.data_ptr(), O, float(reach),
                   _ptr(res, "env_mask"), _ptr(res, "min_env"), _ptr(res, "nearest_obs"), _ptr(res, "obs_min"), work.data_ptr(),
                   work.numel())  # fmt: skip
        res["env_mask"] = res["env_mask"].view(torch.bool)
        return res

    # ---- scenes from sensor data (cppf_scene_from_points / cppf_scene_from_depth; include/cppflow_hip.h) ------------------------------
    def _voxel_self(self, q_self, dev: torch.device):
        """the self filter's arguments: (q_self [n_self, d] -- to be kept alive over the call --, n_self, its pointer, the handle); without
        configurations the library takes neither pointer nor handle"""
        if q_self is None:
            return None, 0, None, None
        q_self = self._x2d(q_self.unsqueeze(0) if q_self.dim() == 1 else q_self, "q_self")
        assert q_self.device == dev, "q_self must be on the device of the sensor data"
        if int(q_self.shape[0]) == 0:
            return q_self, 0, None, None
        return q_self, int(q_self.shape[0]), q_self.data_ptr(), self._handle(dev)

    @staticmethod
    def _voxel_camera(depth: torch.Tensor, intrinsics, cam_to_world):
        """the depth form's arguments: (depth, H, W, intrinsics fp32 [4], cam_to_world as R row-major then t, fp32 [12])"""
        depth = _require_device_tensor(depth, "depth")
        assert depth.dim() == 2, f"depth must be [H, W], is {tuple(depth.shape)}"
        T = cam_to_world.detach().cpu().numpy() if isinstance(cam_to_world, torch.Tensor) else np.asarray(cam_to_world)
        T = T.astype(np.float32)
        assert T.shape in ((4, 4), (3, 4)), f"cam_to_world must be 4x4 or 3x4, is {T.shape}"
        rt = np.ascontiguousarray(np.concatenate([T[:3, :3].reshape(9), T[:3, 3]]), dtype=np.float32)
        k = np.ascontiguousarray(np.asarray([float(v) for v in intrinsics], dtype=np.float32))
        assert k.shape == (4,), "intrinsics = (fx, fy, cx, cy)"
        return depth, int(depth.shape[0]), int(depth.shape[1]), k, rt

    def _voxel_scene(self, source, dev: torch.device, origin, voxel_m: float, dims, q_self, self_margin_m: float, max_cuboids: int,
                     coarsen: bool):
        """the rounds behind `scene_from_points` / `scene_from_depth`; source(grid, tail) makes the library call of one round"""
        assert 0 <= int(max_cuboids) <= _hip.MAX_SCENE_OBSTACLES, f"max_cuboids must be in 0 .. {_hip.MAX_SCENE_OBSTACLES}"
        origin = [float(v) for v in origin]
        dims = [int(v) for v in dims]
        assert len(origin) == 3 and len(dims) == 3, "origin and dims have three entries"
        q_self, n_self, q_ptr, handle = self._voxel_self(q_self, dev)
        cap = int(max_cuboids)
        lo = torch.empty((cap, 3), dtype=torch.float32, device=dev)
        hi = torch.empty((cap, 3), dtype=torch.float32, device=dev)
        counts = torch.empty((8,), dtype=torch.int32, device=dev)
        voxel, history = float(voxel_m), []
        for rnd in range(4 if coarsen else 1):
            grid = _hip.VoxelGrid((_hip._f * 3)(*origin), voxel, (_hip._i32 * 3)(*dims))
            work = sized_buffer("cppf_voxel_scene_workspace_bytes", dev, ctypes.byref(grid), n_self)
            tail = (ctypes.byref(grid), q_ptr, n_self, float(self_margin_m), cap, lo.data_ptr(), hi.data_ptr(), counts.data_ptr(),
                    work.data_ptr(), work.numel(), _stream_ptr(dev))  # fmt: skip
            with torch.cuda.device(dev):  # (without a handle the library launches on the current device)
                _hip.check(source(handle, tail))
            c = counts.cpu().tolist()  # (the one device-to-host copy of this round)
            stats = dict(zip(VOXEL_COUNT_NAMES, c[:7]), voxel_m=voxel, dims=tuple(dims), origin=tuple(origin), rounds=rnd + 1)
            history.append(stats)
            if c[0] <= cap:
                n = c[1]
                return ObstacleScene(lo[:n].clone(), hi[:n].clone(), stats)
            voxel, dims = voxel * 2.0, [(d + 1) // 2 for d in dims]
        raise RuntimeError(
            f"the sensor data gives more cuboids than max_cuboids = {cap}"
            + (" after 3 coarsening rounds" if coarsen else " and coarsen is off") + ": "
            + "; ".join(f"voxel_m={h['voxel_m']:g} dims={h['dims']}: {h['boxes_total']} boxes, {h['occupied_cells']} cells, "
                        f"{h['kept_points']} kept / {h['outside_points']} outside / {h['invalid_points']} invalid / {h['self_points']} self points"
                        for h in history)
        )  # fmt: skip

    def scene_from_points(self, points: torch.Tensor, origin, voxel_m: float, dims, q_self: Optional[torch.Tensor] = None,
                          self_margin_m: float = 0.03, max_cuboids: int = _hip.MAX_SCENE_OBSTACLES, coarsen: bool = True):
        """A world-frame point cloud [n, 3] (device) -> `ObstacleScene` of at most `max_cuboids` axis-aligned cuboids on the same
        device: the occupied cells of the grid (origin, voxel_m, dims = (nx, ny, nz)), equal x-runs of neighbouring rows merged along
        y (`cppf_scene_from_points`; include/cppflow_hip.h states grid, classes and box list).  `q_self` [n_self <= 16, d] (device):
        points within `self_margin_m` of the robot's capsules at any of these configurations are dropped; None: no filter.  More
        cuboids than `max_cuboids`: with `coarsen` the build is repeated with voxel_m * 2 and ceil(dims / 2) at the same origin, at
        most 3 more times; otherwise, or if that does not fit either, RuntimeError -- a truncated scene is never returned.  The counts
        of the returned round are its `.stats`.  One device-to-host copy (the counts) per round."""
        points = _require_device_tensor(points, "points")
        assert points.dim() == 2 and points.shape[1] == 3, f"points must be [n, 3], is {tuple(points.shape)}"
        n = int(points.shape[0])

        def source(handle, tail):
            return _hip.lib().cppf_scene_from_points(handle, points.data_ptr() if n else None, n, *tail)

        return self._voxel_scene(source, points.device, origin, voxel_m, dims, q_self, self_margin_m, max_cuboids, coarsen)

    def scene_from_depth(self, depth: torch.Tensor, intrinsics, cam_to_world, z_min: float, z_max: float, origin, voxel_m: float, dims,
                         q_self: Optional[torch.Tensor] = None, self_margin_m: float = 0.03,
                         max_cuboids: int = _hip.MAX_SCENE_OBSTACLES, coarsen: bool = True):
        """A depth image [H, W] (device, fp32 metres) -> `ObstacleScene`, as `scene_from_points` on its back-projected pixels
        (`cppf_scene_from_depth`).  intrinsics = (fx, fy, cx, cy); cam_to_world: a 4x4 (or 3x4) transform, host; a pixel counts only
        with z_min < depth < z_max."""
        depth, h, w, k, rt = self._voxel_camera(depth, intrinsics, cam_to_world)

        def source(handle, tail):
            return _hip.lib().cppf_scene_from_depth(handle, depth.data_ptr() if h * w else None, h, w, _hip.fptr(k), _hip.fptr(rt),
                                                    float(z_min), float(z_max), *tail)  # fmt: skip

        return self._voxel_scene(source, depth.device, origin, voxel_m, dims, q_self, self_margin_m, max_cuboids, coarsen)

    def voxel_map(self, origin, voxel_m: float, dims, device):
        """A `VoxelMap` (cppflow_amd/scene.py) on `device`, cleared: the per-cell hit counts of the grid (origin, voxel_m, dims =
        (nx, ny, nz)) that frames are added to over time, and from which `VoxelMap.scene(min_frames, merge_z)` builds an
        `ObstacleScene` of the cells seen in at least `min_frames` frames (`cppf_voxel_map_*`, `cppf_scene_from_map`;
        include/cppflow_hip.h, "Scenes fused over frames")."""
        return VoxelMap(self, origin, voxel_m, dims, device)

    def motion_travel_table(self) -> np.ndarray:
        """rho [d, n_capsules] fp32: the travel bounds `motion_clearance` certifies with (`cppf_motion_rho`; include/cppflow_hip.h).
        Host only: needs no device."""
        rho = np.zeros((_hip.MAX_DOF, _hip.MAX_CAPSULES), dtype=np.float32)
        if self._handles:  # (any handle of this robot holds the same table)
            _hip.check(_hip.lib().cppf_motion_rho(next(iter(self._handles.values())), _hip.fptr(rho)))
            return rho[: self.ndof, : self.n_capsules].copy()
        out = ctypes.c_void_p()
        _hip.check(_hip.lib().cppf_robot_create(ctypes.byref(self._desc), -12345, ctypes.byref(out)))  # (a host-only handle)
        try:
            _hip.check(_hip.lib().cppf_motion_rho(out, _hip.fptr(rho)))
        finally:
            _hip.lib().cppf_robot_destroy(out)
        return rho[: self.ndof, : self.n_capsules].copy()

    def motion_clearance(self, q: torch.Tensor, box_lo: torch.Tensor, box_hi: torch.Tensor, level: int = 6, reach: float = 0.05,
                         want: Sequence[str] = ("status", "min_clear", "hit_node")) -> Dict[str, torch.Tensor]:
        """The motion between the waypoints of q [S, W, d] (W >= 2; straight joint-space lines in the stored values, no wrapping)
        against the self pairs and the O <= 4096 axis-aligned cuboids box_lo / box_hi [O, 3] (device, world-frame corners; O = 0: self
        only), by the adaptive-clearance test on 2^level intervals per transition (`cppf_motion_clearance`, csrc/kernels_motion.h).
        status (uint8 [S, W-1], always returned): bit 0 certified collision-free, bit 1 hit (a node penetrates), neither: undecided.
        min_clear (float [S, W-1]): the smallest node clearance (cuboids beyond `reach` do not count); hit_node (int32 [S, W-1]):
        the lowest penetrating node, else -1; nodes (float [S, W-1, 2^level + 1, d], only when asked for): the configurations tested."""
        q, S, W = paths_tensor(q, self.ndof)
        dev = q.device
        box_lo, box_hi, O = _scene_boxes(box_lo, box_hi, dev)
        level = int(level)
        assert 0 <= level <= _hip.MOTION_MAX_LEVEL and W >= 2, (level, W)
        spec = {"status": torch.uint8, "min_clear": torch.float32, "hit_node": torch.int32,
                "nodes": (torch.float32, (S, W - 1, (1 << level) + 1, self.ndof))}  # fmt: skip
        res = optional_outputs((*want, "status"), spec, (S, W - 1), dev)
        work = sized_buffer("cppf_motion_workspace_bytes", dev, S, W)
        self._call("cppf_motion_clearance", dev, q.data_ptr(), S, W, level, box_lo.data_ptr(), box_hi.data_ptr(), O, float(reach),
                   _ptr(res, "status"), _ptr(res, "min_clear"), _ptr(res, "hit_node"), _ptr(res, "nodes"), work.data_ptr(),
                   work.numel())  # fmt: skip
        return res

    def motion_resolve(self, q: torch.Tensor, box_lo: torch.Tensor, box_hi: torch.Tensor, start_level: int = 0, max_depth: int = 16,
                       max_frontier: int = 512, reach: float = 0.05, decided: Optional[torch.Tensor] = None,
                       want: Sequence[str] = ("status", "depth", "hit_num", "min_clear", "n_tested")) -> Dict[str, torch.Tensor]:
        """`motion_clearance` made adaptive (`cppf_motion_resolve`, csrc/kernels_motion_resolve.h): from 2^start_level intervals per
        transition only the intervals whose test fails are bisected, breadth first, until they pass (certified), a node penetrates
        (hit), `max_depth` is reached (undecided) or more than `max_frontier` intervals are open at one level (status bit 2,
        overflow).  status (uint8 [S, W-1], always returned); depth (int32): the level at which the transition ended; hit_num
        (int32): the lowest penetrating node of that level, at parameter hit_num / 2^depth, else -1; min_clear (float): the smallest
        clearance of any node evaluated; n_tested (int32): interval tests spent.  `decided` (uint8 or bool [S, W-1]): transitions
        where it is non-zero are not examined; given a uint8 tensor, it is ALSO the status output, so that a status from an earlier
        call is completed in place and the other outputs of such transitions keep what they held (here: zeros)."""
        q, S, W = paths_tensor(q, self.ndof)
        dev = q.device
        box_lo, box_hi, O = _scene_boxes(box_lo, box_hi, dev)
        start_level, max_depth, max_frontier = int(start_level), int(max_depth), int(max_frontier)
        assert 0 <= start_level <= _hip.MOTION_MAX_LEVEL and start_level <= max_depth <= _hip.MOTION_RESOLVE_MAX_DEPTH, (start_level, max_depth)
        assert (1 << start_level) <= max_frontier <= _hip.MOTION_RESOLVE_MAX_FRONTIER and W >= 2, (max_frontier, W)
        skipping = decided is not None
        if skipping:
            assert isinstance(decided, torch.Tensor) and decided.dtype in (torch.uint8, torch.bool), "decided must be a uint8 or bool tensor"
            decided = _require_device_tensor(decided, "decided", dtype=decided.dtype)
            assert decided.shape == (S, W - 1) and decided.device == dev, (tuple(decided.shape), decided.device)
            assert decided.is_contiguous(), "decided must be contiguous"
        in_place = skipping and decided.dtype == torch.uint8
        spec = {"status": torch.uint8, "depth": torch.int32, "hit_num": torch.int32, "min_clear": torch.float32, "n_tested": torch.int32}
        # with `decided` the skipped transitions are not written: their outputs must not be uninitialised memory (torch.zeros)
        res = optional_outputs((*want, "status"), spec, (S, W - 1), dev, given={"status": decided} if in_place else None,
                               new=torch.zeros if skipping else torch.empty)  # fmt: skip
        work = sized_buffer("cppf_motion_resolve_workspace_bytes", dev, S, W, max_frontier)
        self._call("cppf_motion_resolve", dev, q.data_ptr(), S, W, start_level, max_depth, max_frontier, box_lo.data_ptr(),
                   box_hi.data_ptr(), O, float(reach), decided.data_ptr() if skipping else None, _ptr(res, "status"), _ptr(res, "depth"),
                   _ptr(res, "hit_num"), _ptr(res, "min_clear"), _ptr(res, "n_tested"), work.data_ptr(), work.numel())  # fmt: skip
        return res

    def pose_error_metrics(self, x: torch.Tensor, target: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(positional error [n] in metres, rotational error [n] in radians); target [W,7], n % W == 0."""
        x, target, n, W = rows_and_target(x, target, self.ndof)
        pe = torch.empty(n, dtype=torch.float32, device=x.device)
        re = torch.empty(n, dtype=torch.float32, device=x.device)
        self._call("cppf_pose_error_metrics", x.device, x.data_ptr(), target.data_ptr(), n // W, W, pe.data_ptr(), re.data_ptr())
        return pe, re

    def track_paths(self, target_path: torch.Tensor, k: int, n_segments: int = 1, q0: Optional[torch.Tensor] = None,
                    seed: int = 0, call_index: int = 0, lm_lambda: float = 1e-2, alpha_position: float = 3.5,
                    alpha_rotation: float = 0.35, n_restart: int = 40, n_track: int = 6, n_random_restarts: int = 0,
                    tol_pos_m: float = 0.0, tol_rot_rad: float = 0.0, max_jump_rad: float = 0.0, max_jump_m: float = 0.0,
                    out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:  # fmt: skip
        """k candidate joint-space paths along `target_path` [T,7] in ONE launch (cppf_track_paths, include/cppflow_hip.h): the path is
        cut into `n_segments` contiguous segments, each candidate's segment starts fresh (from `q0` [k*n_segments, d], row
        i*n_segments + s, or a hashed uniform draw of (seed, call_index, candidate, segment)) with `n_restart` LM iterations and tracks
        the following waypoints warm-started with `n_track`, climbing the recovery ladder (warm continuation, then `n_random_restarts`
        random restarts) where a row misses the tolerances or a jump bar.  Returns {"x" [k,T,d], "pos_err_m" [k,T], "rot_err_rad"
        [k,T], "status" [k,T] uint8 (bits _hip.TRACK_*)}; `out` may hold preallocated tensors under those keys."""
        target = _require_device_tensor(target_path, "target_path")
        assert target.dim() == 2 and target.shape[1] == 7, tuple(target.shape)
        T, d, dev = target.shape[0], self.ndof, target.device
        k, S = int(k), int(n_segments)
        assert k >= 0 and 1 <= S <= max(T, 1), (k, S, T)
        if q0 is not None:
            q0 = _require_device_tensor(q0, "q0")
            assert tuple(q0.shape) == (k * S, d) and q0.device == dev, (tuple(q0.shape), (k * S, d))
        res = {} if out is None else dict(out)
        for name, shape, dtype in (("x", (k, T, d), torch.float32), ("pos_err_m", (k, T), torch.float32),
                                   ("rot_err_rad", (k, T), torch.float32), ("status", (k, T), torch.uint8)):  # fmt: skip
            if name in res:
                res[name] = _require_output_tensor(res[name], name, dtype)
                assert tuple(res[name].shape) == shape and res[name].device == dev, (name, tuple(res[name].shape))
            else:
                res[name] = torch.empty(shape, dtype=dtype, device=dev)
        prm = _hip.TrackParams(float(lm_lambda), float(alpha_position), float(alpha_rotation), int(n_restart), int(n_track),
                               int(n_random_restarts), float(tol_pos_m), float(tol_rot_rad), float(max_jump_rad), float(max_jump_m),
                               int(seed) & 0xFFFFFFFF, int(call_index) & 0xFFFFFFFF)  # fmt: skip
        self._call("cppf_track_paths", dev, target.data_ptr(), T, k, S, ctypes.byref(prm), q0.data_ptr() if q0 is not None else None,
                   res["x"].data_ptr(), res["pos_err_m"].data_ptr(), res["rot_err_rad"].data_ptr(), res["status"].data_ptr())  # fmt: skip
        return res

    PLAN_METRIC_FIELDS = ("max_pos_err_cm", "mean_pos_err_cm", "max_rot_err_deg", "mean_rot_err_deg", "mjac_deg", "mjac_cm",
                          "path_length_rad", "path_length_m", "n_joint_limit_violations", "n_self_colliding",
                          "n_env_colliding", "initial_q_norm_dist")  # fmt: skip
    SEED_SUMMARY_FIELDS = ("max_pos_err_cm", "max_rot_err_deg", "mjac_rev_deg", "mjac_pris_cm", "n_self_colliding",
                           "n_env_colliding", "n_jlim", "sum_ext_cost")  # fmt: skip

    def seed_summary(self, x: torch.Tensor, packed: torch.Tensor, S: int, W: int, out: Optional[torch.Tensor] = None):
        """[S,8] per-seed reduction (SEED_SUMMARY_FIELDS) of a fused launch's packed per-row outputs and its x_out."""
        x = self._x2d(x)
        assert x.shape[0] == S * W, (tuple(x.shape), S, W)
        rows = device_packed_views(packed, S * W, x.device)
        if out is None:
            out = torch.empty((S, 8), dtype=torch.float32, device=x.device)
        self._call("cppf_seed_summary", x.device, x.data_ptr(), S, W, *(rows[k].data_ptr() for k in _SEED_SUMMARY_ROW_ARGS), out.data_ptr())
        return out

    def lm_full_step(self, x: torch.Tensor, target: torch.Tensor, opt_params, virtual_configs: Optional[torch.Tensor] = None,
                     x_out: Optional[torch.Tensor] = None, constraints=None, pin: int = 0,
                     scene: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> torch.Tensor:  # fmt: skip
        """One coupled LM step (levenberg_marquardt_full, cppflow/optimization.py:95-144) for every trajectory in
        x [S*W, d]; target [W,7].  `opt_params` is an OptimizationParameters (e.g. ALT_LOSS_V2_1_DIFF); its "satisfied" row
        options (pose scale-down, differencing filter / scale-down: cppflow/optimization_utils.py:514-533, 562-598) are applied
        on the device, with thresholds from `constraints` (default: opt_params.constraints if present, else DEFAULT_CONSTRAINTS).
        `pin` = `_hip.PIN_FIRST | _hip.PIN_LAST`: waypoint 0 / W-1 of every trajectory is held fixed at its value in `x` (it comes
        back bit for bit; its free neighbour feels it through the differencing row).  Not combined with the "satisfied" options.
        `scene` = (box_lo, box_hi), device [O, 3] world-frame corners (`cppflow_amd.scene.ObstacleScene`: `.lo`, `.hi`), O <= 4096:
        the environment rows come from ALL of these cuboids instead of the handle's at most 8, which are then neither read nor
        changed (`cppf_lm_full_step_scene`).  Where a handle could hold the cuboids that penetrate, the result is the same bit for bit."""
        x, target, n, W = rows_and_target(x, target, self.ndof)
        p = opt_params
        xv = None
        if virtual_configs is not None and p.use_virtual_configs and virtual_configs.numel() > 0:
            xv = self._x2d(virtual_configs, "virtual_configs")
            assert xv.shape == x.shape, "virtual_configs must have the shape of x (optimization_utils.py:433)"
        prm = self.full_params(p, constraints)
        d = self.ndof
        nt = d * (d + 1) // 2
        dev = x.device
        blocks = torch.empty(n * (nt + d), dtype=torch.float32, device=dev)
        G = torch.empty(n * d * d, dtype=torch.float32, device=dev)  # L_t (dense) in the parallel-in-time form, G_t (packed) else
        y = torch.empty(n * d, dtype=torch.float32, device=dev)
        if x_out is None:
            x_out = torch.empty_like(x)
        head = (x.data_ptr(), target.data_ptr(), xv.data_ptr() if xv is not None else None, n // W, W, ctypes.byref(prm), int(pin))
        tail = (blocks.data_ptr(), G.data_ptr(), y.data_ptr(), x_out.data_ptr())
        if scene is not None:
            box_lo, box_hi, O = _scene_boxes(*scene, dev, rows="x")
            self._call("cppf_lm_full_step_scene", dev, *head, box_lo.data_ptr() if O else None, box_hi.data_ptr() if O else None, O, *tail)
        else:
            self._call("cppf_lm_full_step_pinned", dev, *head, *tail)
        return x_out

    @staticmethod
    def full_params(opt_params, constraints=None) -> "_hip.FullParams":
        """An OptimizationParameters record as the coupled step's `cppf_full_params` (thresholds of the "satisfied" row options from
        `constraints`, see `lm_full_step`)."""
        p = opt_params
        assert not (p.differencing_do_scale_satisfied and p.differencing_do_ignore_satisfied), "use one or the other, not both"
        from cppflow_amd.optimization_utils import satisfied_thresholds

        thr = satisfied_thresholds(p, constraints)

        def f(v):
            return 0.0 if v is None else float(v)

        return _hip.FullParams(f(p.lm_lambda), f(p.alpha_position), f(p.alpha_rotation), f(p.alpha_differencing),
                              f(p.alpha_differencing_prismatic_scaling), f(p.alpha_virtual_configs),
                              f(p.alpha_self_collision), f(p.alpha_env_collision), int(bool(p.use_pose)),
                              int(bool(p.use_differencing)), int(bool(p.use_virtual_configs)), int(p.n_virtual_configs or 0),
                              int(bool(p.use_self_collisions)), int(bool(p.use_env_collisions)),
                              int(bool(p.pose_do_scale_down_satisfied)), thr["pose_threshold_m"], thr["pose_threshold_rad"],
                              f(p.pose_ignore_satisfied_scale_down),
                              1 if p.differencing_do_ignore_satisfied else (2 if p.differencing_do_scale_satisfied else 0),
                              thr["differencing_threshold_rad"], thr["differencing_threshold_m"],
                              f(p.differencing_scale_down_satisfied_scale),
                              int(bool(p.differencing_scale_down_satisfied_shift_invalid_to_threshold)))  # fmt: skip

    # ---- the optimiser loop on the device (cppf_lm_optimize_enqueue) ---------------------------------------------------------------
    def lm_optimize_buffers(self, S: int, W: int, prm: "_hip.OptloopParams", device) -> Tuple[torch.Tensor, torch.Tensor]:
        """(workspace, control) for `lm_optimize_enqueue`: the workspace (fp32; its first S*W*ndof floats are the snapshot of the last
        valid x) and the loop-control block (int32: records then trace), initialised so that every record leads with a pose step."""
        dev = torch.device(device)
        n_floats = query_size("cppf_lm_optimize_workspace_bytes", self._handle(dev), S, W) // 4
        n_records = S if prm.per_trajectory else 1
        init = _hip.optloop_initial_control(n_records, prm.trace_capacity)
        assert init.nbytes == query_size("cppf_lm_optimize_control_bytes", S, ctypes.byref(prm))
        return torch.empty(n_floats, dtype=torch.float32, device=dev), torch.from_numpy(init).to(dev)

    def lm_optimize_enqueue(self, x: torch.Tensor, target: torch.Tensor, prm: "_hip.OptloopParams", workspace: torch.Tensor,
                            control: torch.Tensor, n_iterations: int, pin: int = 0) -> None:
        """Enqueue `n_iterations` gated iterations of the alternating loop on x [S*W, d] (in place) and return without
        synchronising; copy `control` back to see what was decided (`_hip.OptloopRecord` per record, then the trace).
        `pin` (`_hip.PIN_FIRST | _hip.PIN_LAST`): the named end rows of every trajectory are never written."""
        xc, target, n, W = rows_and_target(x, target, self.ndof)
        assert xc.data_ptr() == x.data_ptr(), "lm_optimize_enqueue works on x in place: x must be contiguous"
        assert workspace.is_cuda and workspace.dtype == torch.float32 and workspace.is_contiguous()
        assert control.is_cuda and control.dtype == torch.int32 and control.is_contiguous()
        self._call("cppf_lm_optimize_enqueue_pinned", x.device, x.data_ptr(), target.data_ptr(), n // W, W, ctypes.byref(prm), int(pin),
                   workspace.data_ptr(), control.data_ptr(), int(n_iterations))  # fmt: skip

    def dp_search(self, q: torch.Tensor, ext_cost: torch.Tensor, prismatic_joint_scaling: float = 5.0, method: str = "auto",
                  return_memo: bool = False, return_method: bool = False):
        """q [k,T,d], ext_cost [k,T] -> (best_path [T,d], best_idx [T] int32, cost table [T,k]); cppflow/search.py:128-191.
        `method`: "table" (k <= 256: transition table + the recurrence on one compute unit, cppf_dp_search_tabled), "resident"
        (cppf_dp_search: ONE launch of resident workgroups handing the cost row on up to k = 1024, one launch per waypoint beyond),
        "launches" (one launch per waypoint, any k -- for THIS call, no handle state involved), "auto" = whichever is fastest at this k
        (table up to 128 candidates, 192 for chains of more than 8 joints; resident up to 1024; launches beyond).  Bit-identical results.
        `return_method` appends the method that ran ("table" / "resident" / "launches") to the result."""
        assert method in ("auto", "table", "resident", "launches"), method
        (q, k, T), d = paths_tensor(q, self.ndof), self.ndof
        ext_cost = _require_device_tensor(ext_cost, "q_costs_external")
        assert ext_cost.shape == (k, T), (tuple(ext_cost.shape), (k, T))
        dev = q.device
        qT = torch.empty((T, k, d), dtype=torch.float32, device=dev)
        costsT = torch.empty((T, k), dtype=torch.float32, device=dev)
        memoT = torch.empty((T, k), dtype=torch.int32, device=dev)
        best_path = torch.empty((T, d), dtype=torch.float32, device=dev)
        best_idx = torch.empty(T, dtype=torch.int32, device=dev)
        n_table = query_size("cppf_dp_table_floats", k, T)
        # measured (scripts/dp_bench.py, profiles/r3_dp_bench.txt): the table form wins up to k = 128 (k = 64: 168 vs 321 us, 128: 365
        # vs 442); from 129 candidates on its rows take the 192-wide register sets (~540 us at T = 256 whatever k) and the resident
        # hand-off form is ahead (k = 175: 491 vs 537 us, 256: 493 vs 812) -- unless the chain has more than 8 joints, whose
        # per-pair arithmetic in front of every hand-off keeps the table form ahead up to k = 192 (12 joints: 551 vs 618 us)
        k_table = 128 if d <= 8 else 192
        tabled = method == "table" or (method == "auto" and k <= k_table and 2 <= T <= 65536 and n_table * 4 <= (1 << 30))
        head = (q.data_ptr(), ext_cost.data_ptr(), k, T, float(prismatic_joint_scaling), qT.data_ptr(), costsT.data_ptr(), memoT.data_ptr())
        if tabled:
            ran = "table"
            table = torch.empty(max(n_table, 1), dtype=torch.float32, device=dev)
            self._call("cppf_dp_search_tabled", dev, *head, table.data_ptr(), best_path.data_ptr(), best_idx.data_ptr())
        else:
            # ("resident" = this entry point as it decides itself, i.e. resident up to 1024 candidates unless the handle's
            # CPPF_TUNE_DP_PERSISTENT test switch is 0; "launches" forces one launch per waypoint for this call only)
            mode = _hip.DP_LAUNCHES if method == "launches" else _hip.DP_AUTO
            resident_on = self._tuning.get(_hip.TUNE_KEYS["dp_persistent"], 1) not in (0,)
            ran = "resident" if T >= 2 and k <= 1024 and mode == _hip.DP_AUTO and resident_on else "launches"
            self._call("cppf_dp_search", dev, *head, best_path.data_ptr(), best_idx.data_ptr(), mode)
        res = (best_path, best_idx, costsT) + ((memoT,) if return_memo else ())
        return res + ((ran,) if return_method else ())

    def dp_nbest(self, q: torch.Tensor, costsT: torch.Tensor, memoT: torch.Tensor, n_paths: int, min_separation: float,
                 prismatic_joint_scaling: float = 5.0):
        """The `n_paths` lowest-cost paths of a finished search that are at least `min_separation` (radians, prismatic joints scaled)
        apart from each other (`cppf_dp_nbest`): q [k,T,d] and the `costsT` / `memoT` [T,k] of `dp_search(..., return_memo=True)` ->
        (paths [n_paths,T,d], path_idx [n_paths,T] int32, path_cost [n_paths], n_found [1] int32 -- a DEVICE tensor: nothing is
        synchronised here).  Slot 0 is the search's own best path; slots from n_found on are NaN / -1 / +inf; n_found = -1 when the
        tables carry the resident search's timed-out flag."""
        (q, k, T), d = paths_tensor(q, self.ndof), self.ndof
        costsT = _require_device_tensor(costsT, "costsT")
        memoT = _require_device_tensor(memoT, "memoT", torch.int32)
        assert costsT.shape == (T, k) and memoT.shape == (T, k), (tuple(costsT.shape), tuple(memoT.shape), (T, k))
        n_paths = int(n_paths)
        dev = q.device
        work = sized_buffer("cppf_dp_nbest_workspace_bytes", dev, k, T, n_paths)
        paths = torch.empty((n_paths, T, d), dtype=torch.float32, device=dev)
        path_idx = torch.empty((n_paths, T), dtype=torch.int32, device=dev)
        path_cost = torch.empty(n_paths, dtype=torch.float32, device=dev)
        n_found = torch.empty(1, dtype=torch.int32, device=dev)
        self._call("cppf_dp_nbest", dev, q.data_ptr(), costsT.data_ptr(), memoT.data_ptr(), k, T, n_paths, float(min_separation),
                   float(prismatic_joint_scaling), work.data_ptr(), paths.data_ptr(), path_idx.data_ptr(), path_cost.data_ptr(),
                   n_found.data_ptr())  # fmt: skip
        return paths, path_idx, path_cost, n_found

    def plan_metrics(self, x: torch.Tensor, target: torch.Tensor, self_mask: Optional[torch.Tensor] = None,
                     env_mask: Optional[torch.Tensor] = None, q_init: Optional[torch.Tensor] = None) -> torch.Tensor:  # fmt: skip
        """[S,16] `Plan` metrics (cppflow/data_types.py:140-264) of S paths in one launch; columns PLAN_METRIC_FIELDS.
        x [S*W,d] (or [S,W,d]); masks are per-row uint8 / bool tensors of the same rows (optional); q_init [d] or [1,d]."""
        x, target, n, W = rows_and_target(x.reshape(-1, self.ndof) if x.dim() == 3 else x, target, self.ndof)
        ptrs = []
        for m, nm in ((self_mask, "self_mask"), (env_mask, "env_mask")):
            if m is None:
                ptrs.append(None)
                continue
            assert m.is_cuda and m.numel() == n and m.dtype in (torch.uint8, torch.bool), f"{nm} must be uint8 / bool [{n}]"
            m = m.contiguous()
            ptrs.append(m)
        qi = None
        if q_init is not None:
            qi = _require_device_tensor(q_init, "q_init").reshape(-1).contiguous()
            assert qi.numel() == self.ndof, tuple(q_init.shape)
        out = torch.empty((n // W, 16), dtype=torch.float32, device=x.device)
        self._call("cppf_plan_metrics", x.device, x.data_ptr(), target.data_ptr(), n // W, W,
                   ptrs[0].data_ptr() if ptrs[0] is not None else None, ptrs[1].data_ptr() if ptrs[1] is not None else None,
                   qi.data_ptr() if qi is not None else None, out.data_ptr())  # fmt: skip
        return out

    def mjacs(self, q: torch.Tensor, prismatic_joint_scaling: float = 5.0) -> torch.Tensor:
        """q [k,T,d] -> [k,k,T-1] maximum (wrapped, prismatic-scaled) joint change from candidate j at t to candidate i at
        t+1 (cppflow/search.py:100-125).  `dp_search` does not use it -- it is the tensor the reference builds."""
        q, k, T = paths_tensor(q, self.ndof)
        out = torch.empty((k, k, max(T - 1, 0)), dtype=torch.float32, device=q.device)
        self._call("cppf_mjacs", q.device, q.data_ptr(), k, T, float(prismatic_joint_scaling), out.data_ptr())
        return out

    def seed_validity(self, x: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """[S,4]: per seed max position error (cm), max rotation error (deg), mjac revolute (deg), mjac prismatic (cm)."""
        x, target, n, W = rows_and_target(x, target, self.ndof)
        out = torch.empty((n // W, 4), dtype=torch.float32, device=x.device)
        self._call("cppf_seed_validity", x.device, x.data_ptr(), target.data_ptr(), n // W, W, out.data_ptr())
        return out


class _PreboundLaunch:
    """A launch held ready: `_fn(*_args, stream)` is ONE C call on pre-marshalled arguments for the device `_device`, its return
    code checked only when it is not zero.  This is the timed hot path of bench.py and `ShardedRefiner`: nothing else runs in it."""

    def launch(self) -> None:
        rc = self._fn(*self._args, torch.cuda.current_stream(self._device).cuda_stream)
        if rc:
            _hip.check(rc)

    def launch_on(self, stream: "torch.cuda.Stream") -> None:
        """`launch()` on an explicit HIP stream: independent batches in flight on two streams overlap one launch's tail with
        the next one's ramp-up (each batch needs its own output buffers)."""
        rc = self._fn(*self._args, stream.cuda_stream)
        if rc:
            _hip.check(rc)


class LmLaunchPlan(_PreboundLaunch):
    def __init__(self, robot: Robot, x, target, lm_lambda, alpha_position, alpha_rotation, n_steps, x_out, packed_out, clamp,
                 summary_out=None, shape=_hip.SHAPE_AUTO, solver=_hip.SOLVER_AUTO, errors_out=None):  # fmt: skip
        x, target, n, W = rows_and_target(x, target, robot.ndof)
        self._out = _hip.LmOutputs()
        self.outputs, keep = fill_lm_outputs(self._out, x, W, x_out, packed_out, errors_out, summary_out)
        self._keep = [robot, x, target] + keep  # the plan owns references to every buffer it points at
        self._prm = _hip.LmParams(float(lm_lambda), float(alpha_position), float(alpha_rotation), int(n_steps), int(bool(clamp)),
                                  0.0, 0.0, int(shape), int(solver))
        self._fn = _hip.lib().cppf_lm_pose_steps
        self._args = (robot._handle(x.device), x.data_ptr(), target.data_ptr(), n // W, W, ctypes.byref(self._prm),
                      ctypes.byref(self._out))  # fmt: skip
        self._device = x.device

    def set_summary_out(self, summary_out: torch.Tensor) -> None:
        """Point the next launches' per-seed summary at another [S,8] buffer (a ring of buffers in flight on the wire)."""
        _check_summary_buffer(summary_out, self._args[3], self._device)
        self._out.seed_summary = summary_out.data_ptr()
        self.outputs["seed_summary"] = summary_out

    def summary_launcher(self, out: torch.Tensor):
        """A zero-allocation callable that reduces this plan's per-row outputs into `out` [S,8] (`Robot.seed_summary`)."""
        assert "ext_cost" in self.outputs, "the plan has no packed per-row outputs"
        handle, S, W, device = self._args[0], self._args[3], self._args[4], self._device
        _check_summary_buffer(out, S, device)
        fn = _hip.lib().cppf_seed_summary
        args = (handle, self.outputs["x"].data_ptr(), S, W, *(self.outputs[k].data_ptr() for k in _SEED_SUMMARY_ROW_ARGS),
                out.data_ptr())  # fmt: skip

        def launch() -> None:
            rc = fn(*args, torch.cuda.current_stream(device).cuda_stream)
            if rc:
                _hip.check(rc)

        return launch


class LmBatchPlan(_PreboundLaunch):
    """`Robot.lm_batch_plan`: owns a cppf_lm_batch (a device table of the items' pointers) and references to every buffer in it."""

    def __init__(self, robot: Robot, items, lm_lambda, alpha_position, alpha_rotation, n_steps, clamp=True, solver=_hip.SOLVER_AUTO):
        assert 1 <= len(items) <= _hip.MAX_BATCH, f"a batch holds 1 .. {_hip.MAX_BATCH} problems"
        arr = (_hip.LmBatchItem * len(items))()
        self._keep, self.outputs, dev = [robot], [], None
        for i, it in enumerate(items):
            x, target, n, W = rows_and_target(it["x"], it["target"], robot.ndof)
            dev = x.device if dev is None else dev
            assert x.device == dev and target.device == dev, "every buffer of a batch lives on one device"
            arr[i].x_in, arr[i].target, arr[i].S, arr[i].W = x.data_ptr(), target.data_ptr(), n // W, W
            views, keep = fill_lm_outputs(arr[i].out, x, W, it["x_out"], it.get("packed_out"), it.get("errors_out"), it.get("summary_out"))
            self.outputs.append(views)
            self._keep += [x, target] + keep
        prm = _hip.LmParams(float(lm_lambda), float(alpha_position), float(alpha_rotation), int(n_steps), int(bool(clamp)),
                            0.0, 0.0, _hip.SHAPE_ROW, int(solver))
        self._h = ctypes.c_void_p()
        self._lib = _hip.lib()
        _hip.check(self._lib.cppf_lm_batch_create(robot._handle(dev), len(items), arr, ctypes.byref(prm), ctypes.byref(self._h)))
        self._fn, self._args, self._device, self.n_items = self._lib.cppf_lm_batch_launch, (self._h,), dev, len(items)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h is not None and h.value:
            try:
                self._lib.cppf_lm_batch_destroy(h)
            except Exception:  # noqa: BLE001 -- interpreter shutdown
                pass


def get_robot(name: str) -> Robot:
    """Stands in for jrl.robots.get_robot (cppflow/data_type_utils.py:197)."""
    if name not in ROBOT_SPECS:
        raise ValueError(f"unknown robot '{name}' (have {sorted(ROBOT_SPECS)})")
    return Robot(ROBOT_SPECS[name]())


def Panda() -> Robot:
    return get_robot("panda")


def Fetch() -> Robot:
    return get_robot("fetch")


def FetchArm() -> Robot:
    return get_robot("fetch_arm")
