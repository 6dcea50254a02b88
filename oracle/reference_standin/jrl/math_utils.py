"""jrl.math_utils by the names the reference imports: the quaternion helpers of oracle/ref_torch.py, forwarded, and the two it lacks."""

import math

import torch

from oracle.ref_torch import (  # noqa: F401  (re-exported)
    geodesic_distance_between_quaternions,
    quaternion_inverse,
    quaternion_product,
    quaternion_to_rpy,
)


def angular_subtraction(angles_1: torch.Tensor, angles_2: torch.Tensor) -> torch.Tensor:
    """angles_1 - angles_2 wrapped to [-pi, pi): the form cppflow/evaluation_utils.py:144-154 uses for consecutive waypoints."""
    return torch.remainder(angles_1 - angles_2 + math.pi, 2 * math.pi) - math.pi


def rpy_tuple_to_rotation_matrix(rpy, device=None) -> torch.Tensor:
    from cppflow_amd.robot_model import rpy_to_matrix

    return torch.tensor(rpy_to_matrix(*rpy), dtype=torch.get_default_dtype(), device=device)


def quaternion_norm(q: torch.Tensor) -> torch.Tensor:
    return torch.norm(q, dim=1)
