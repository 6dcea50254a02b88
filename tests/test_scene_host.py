"""Host logic of obstacle scenes (cppflow_amd/scene.py, Problem): the active-set selection, the scene's corners, and what
`Problem.bind_obstacles()` does with 8 and with 9 cuboids.  No GPU."""

import dataclasses
import os

import numpy as np
import pytest
import torch

from tests import helpers as H

REFERENCE = os.path.join(os.path.dirname(__file__), "golden", "reference_files")
INF = float("inf")


def test_select_active_obstacles_takes_the_smallest_finite_ties_to_the_lower_index_in_index_order():
    from cppflow_amd.scene import select_active_obstacles

    # ties: 0.1 occurs at 1, 4 and 6; with room for three of {-0.2@7, 0.1@1, 0.1@4, 0.1@6} index 6 is the one left out
    v = [0.5, 0.1, INF, 0.3, 0.1, 0.7, 0.1, -0.2]
    assert select_active_obstacles(v, max_active=3) == [1, 4, 7]
    assert select_active_obstacles(v, max_active=4) == [1, 4, 6, 7]
    assert select_active_obstacles(v, max_active=1) == [7]
    assert select_active_obstacles(v, max_active=0) == []
    # fewer finite than the limit: all of them, never an infinite one; the default limit is the handle's 8
    assert select_active_obstacles(v) == [0, 1, 3, 4, 5, 6, 7]
    assert select_active_obstacles([INF] * 20) == [] and select_active_obstacles([]) == []
    many = np.arange(20, 0, -1, dtype=np.float32)  # descending: the eight smallest are the LAST eight indices
    assert select_active_obstacles(many) == list(range(12, 20))
    assert select_active_obstacles(torch.tensor(many)) == list(range(12, 20))  # (a tensor is taken as well)
    # result is sorted by index, not by distance
    assert select_active_obstacles([0.3, 0.2, 0.1], max_active=2) == [1, 2]
    # NaN is not finite
    assert select_active_obstacles([float("nan"), 0.2, INF], max_active=8) == [1]
    # `first`: taken before any other, whatever their value; the rest by distance
    assert select_active_obstacles(v, max_active=3, first=[2, 5]) == [2, 5, 7]
    assert select_active_obstacles(v, max_active=2, first=[5, 2, 0]) == [2, 5]
    with pytest.raises(AssertionError):
        select_active_obstacles(v, first=[8])


def _cuboids(n, seed=0):
    rng = np.random.default_rng(seed)
    obs = [H.cuboid_obstacle(*rng.uniform(-1, 1, 3), *rng.uniform(0.04, 0.12, 3)) for _ in range(n)]
    return [torch.tensor(c) for c, _ in obs], [torch.tensor(T) for _, T in obs]


def test_scene_corners_are_the_fp32_sums():
    from cppflow_amd.scene import ObstacleScene

    cub, Ts = _cuboids(37, seed=1)
    sc = ObstacleScene.from_cuboids(cub, Ts, "cpu")
    assert sc.n_obstacles == 37 and sc.lo.dtype == torch.float32 and sc.lo.shape == (37, 3) == sc.hi.shape
    for o in range(37):
        c, t = cub[o].numpy().astype(np.float32), Ts[o].numpy().astype(np.float32)[:3, 3]
        assert np.array_equal(sc.lo[o].numpy(), (t + c[:3]).astype(np.float32))  # one fp32 addition, as cppf_set_obstacles
        assert np.array_equal(sc.hi[o].numpy(), (t + c[3:]).astype(np.float32))
    want_lo, want_hi = H.box_corners([c.numpy() for c in cub], [T.numpy() for T in Ts])
    assert np.array_equal(sc.lo.numpy().astype(np.float64), want_lo) and np.array_equal(sc.hi.numpy().astype(np.float64), want_hi)
    empty = ObstacleScene.from_cuboids([], [], "cpu")
    assert empty.n_obstacles == 0 and empty.lo.shape == (0, 3)
    # a rotated cuboid is refused, as by cppf_set_obstacles (and by the reference)
    rot = Ts[0].clone()
    rot[:3, :3] = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    with pytest.raises(AssertionError, match="axis-aligned"):
        ObstacleScene.from_cuboids(cub[:1], [rot], "cpu")
    with pytest.raises(AssertionError, match="at most"):
        ObstacleScene.from_cuboids(cub * 111, Ts * 111, "cpu")  # 4107 > 4096


class _RecordingRobot:
    """stands in for the robot of a problem: records what bind_obstacles hands it"""

    def __init__(self, robot):
        self._robot, self.calls = robot, []

    def __getattr__(self, name):
        return getattr(self._robot, name)

    def set_obstacles(self, cuboids, Tcuboids):
        self.calls.append((list(cuboids), list(Tcuboids)))


def _problem(n_cuboids):
    from cppflow_amd.data_type_utils import problem_from_filename

    p = problem_from_filename(None, "panda__1cube_mini", problems_dir=os.path.join(REFERENCE, "problems"),
                              paths_dir=os.path.join(REFERENCE, "paths"), device="cpu")  # fmt: skip
    cub, Ts = _cuboids(n_cuboids, seed=2)
    return dataclasses.replace(p, obstacles_cuboids=cub, obstacles_Tcuboids=Ts, robot=_RecordingRobot(p.robot))


def test_bind_obstacles_is_unchanged_with_8_cuboids_and_needs_an_active_set_with_9():
    p8 = _problem(8)
    assert not p8.uses_scene and p8.active_obstacles is None
    p8.bind_obstacles()
    assert len(p8.robot.calls) == 1
    cub, Ts = p8.robot.calls[0]
    assert len(cub) == 8 and all(a is b for a, b in zip(cub, p8.obstacles_cuboids)) and all(a is b for a, b in zip(Ts, p8.obstacles_Tcuboids))
    assert p8.choose_active_obstacles(None, 0.25) == list(range(8)) and p8.active_obstacles is None  # (every cuboid, nothing kept)

    p9 = _problem(9)
    assert p9.uses_scene
    with pytest.raises(AssertionError, match=r"choose_active_obstacles\(q, reach_m\)"):
        p9.bind_obstacles()
    assert p9.robot.calls == []
    p9.active_obstacles = [0, 3, 8]
    p9.bind_obstacles()
    cub, Ts = p9.robot.calls[0]
    assert [c is p9.obstacles_cuboids[i] for c, i in zip(cub, (0, 3, 8))] == [True] * 3 and len(cub) == len(Ts) == 3
    assert Ts[2] is p9.obstacles_Tcuboids[8]
    # the scene holds all nine, whatever is active
    sc = p9.scene("cpu")
    assert sc.n_obstacles == 9 and p9.scene("cpu") is sc


def test_stages_that_take_obstacles_from_the_handle_refuse_a_scene():
    from cppflow_amd.optimization import run_lm_pose_refinement

    p9 = _problem(9)
    x = torch.zeros((p9.n_timesteps, 7))
    with pytest.raises(AssertionError, match="more than 8 cuboids"):
        run_lm_pose_refinement(p9, x, 3)
    from cppflow_amd.distributed import sharded_candidate_evaluation

    with pytest.raises(AssertionError, match="more than 8 cuboids"):
        sharded_candidate_evaluation(p9, x.view(1, p9.n_timesteps, 7), 0, None)
