"""Scenes from sensor data, without a GPU: the NumPy model of tests/voxel_scene.py against its own definitions (the boxes tile the
occupancy), what the recipes have to exercise, the C ABI of cppf_scene_from_points / cppf_scene_from_depth /
cppf_voxel_scene_workspace_bytes with every refusal on a host-only handle, and the round trip of a scene through the Problem's lists."""

import ctypes
import re

import numpy as np
import pytest
import torch

from tests import voxel_scene as V
from tests.test_abi import HEADER, declared_functions

F = np.float32


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def test_hand_made_occupancies_give_the_expected_boxes():
    for name, (occ, n_boxes) in V.hand_made_occupancies().items():
        assert V.tiles_exactly(occ), name
        assert len(V.heads(occ)) == n_boxes, (name, V.heads(occ))
    occ, _ = V.hand_made_occupancies()["a chain reaching y = ny - 1"]
    assert V.heads(occ) == [(60, 68, 1, 5, 1)]
    lo, hi = V.boxes(occ, V.ORIGIN, V.VOXELS[1])
    P = V.grid_planes(V.ORIGIN, V.VOXELS[1], (70, 5, 2))
    assert lo.dtype == F and lo.tolist() == [[P[0][60], P[1][1], P[2][1]]] and hi.tolist() == [[P[0][68], P[1][5], P[2][2]]]


@pytest.mark.parametrize("seed", range(6))
def test_random_occupancies_are_tiled_exactly(seed):
    rng = np.random.RandomState(seed)
    for dims in ((1, 1, 1), (63, 2, 1), (64, 5, 2), (65, 5, 5), (130, 2, 5)):
        for density in (0.0, 0.1, 0.5, 0.9, 1.0):
            occ = rng.uniform(size=dims[::-1]) < density
            if seed % 2:  # correlated along y, so that runs do repeat
                occ[:, 1:, :] = np.where(rng.uniform(size=occ[:, 1:, :].shape) < 0.7, occ[:, :-1, :], occ[:, 1:, :])
            assert V.tiles_exactly(occ), (dims, density)
            lo, hi = V.boxes(occ, V.ORIGIN, V.VOXELS[seed % 3])
            assert bool((lo < hi).all())
            # the boxes in metres hold the centre of every occupied cell exactly once, and of no other cell
            P = V.grid_planes(V.ORIGIN, V.VOXELS[seed % 3], dims)
            zz, yy, xx = np.meshgrid(*(np.arange(n) for n in dims[::-1]), indexing="ij")
            c = np.stack([V.cell_centre(P[0], xx.ravel()), V.cell_centre(P[1], yy.ravel()), V.cell_centre(P[2], zz.ravel())], axis=1)
            assert np.array_equal(V.contained(c, lo, hi).sum(axis=1), occ.ravel().astype(np.int64)), (dims, density)


def test_the_recipes_exercise_what_they_must():
    dims, voxel = (130, 5, 5), V.VOXELS[1]
    pts = V.point_recipe(1000, V.ORIGIN, voxel, dims, seed=1)
    P = V.grid_planes(V.ORIGIN, voxel, dims)
    for k in range(3):
        assert bool((np.diff(P[k]) > 0).all())
    m = V.scene_from_points(pts, V.ORIGIN, voxel, dims)
    cls, cells = m["classes"], m["cells"]
    for c in (V.INVALID, V.OUTSIDE, V.KEPT):
        assert int((cls == c).sum()) >= 64, c
    hs = V.heads(m["occ"])
    assert any(x0 < 64 < x1 for x0, x1, *_ in hs)  # a run crossing a 64-bit word boundary
    assert any(x1 == dims[0] for _, x1, *_ in hs) and dims[0] % 64 != 0  # a run ending at x = nx - 1
    assert any(y1 - y >= 2 for _, _, y, y1, _ in hs) and any(y1 == dims[1] and y1 - y >= 2 for _, _, y, y1, _ in hs)  # merged; a chain to ny - 1
    on = [(pts[:, k][:, None] == P[k][None, :-1]).any(axis=1) for k in range(3)]
    exact = on[0] & on[1] & on[2]
    assert int(exact.sum()) >= 1 and bool((cls[exact] == V.KEPT).all())  # a point on P(i) belongs to cell i ...
    i = np.flatnonzero(exact)[0]
    assert all(P[k][cells[i, k]] == pts[i, k] for k in range(3))
    for k in range(3):  # ... on P(n) it is outside
        top = (pts[:, k] == P[k][-1]) & np.isfinite(pts).all(axis=1)
        assert int(top.sum()) >= 1 and bool((cls[top] == V.OUTSIDE).all())
    below = (pts[:, 0] == np.nextafter(P[0][0], F(-np.inf))) & np.isfinite(pts).all(axis=1)
    assert int(below.sum()) >= 1 and bool((cls[below] == V.OUTSIDE).all())
    assert np.isnan(pts).any() and np.isposinf(pts).any() and np.isneginf(pts).any()
    assert bool((cls[~np.isfinite(pts).all(axis=1)] == V.INVALID).all())
    assert m["counts"][3:7].sum() == len(pts) and m["counts"][0] == len(hs) == len(m["lo"])
    # every kept point lies in exactly one box
    assert bool((V.contained(pts[cls == V.KEPT], m["lo"], m["hi"]).sum(axis=1) == 1).all())
    # thousands of points in one cell
    piled = V.point_recipe(64, V.ORIGIN, voxel, dims, seed=2, pile=3000)
    mp = V.scene_from_points(piled, V.ORIGIN, voxel, dims)
    _, per_cell = np.unique(mp["cells"][mp["classes"] == V.KEPT], axis=0, return_counts=True)
    assert per_cell.max() >= 3000
    # capacity cuts the list, not the counts
    cut = V.scene_from_points(pts, V.ORIGIN, voxel, dims, capacity=3)
    assert cut["written"] == 3 and cut["counts"][0] == m["counts"][0] and cut["counts"][1] == 3
    # the depth recipe: invalid pixels of every kind, kept and outside points
    for H, W in ((8, 10), (33, 65)):
        depth, intr, T, z_min, z_max, origin, vox, dd = V.depth_recipe(H, W)
        p, invalid = V.back_project(depth, intr, T, z_min, z_max)
        assert np.isnan(depth).any() and np.isinf(depth).any() and (depth <= 0).any() and (depth >= z_max).any()
        md = V.scene_from_points(p, origin, vox, dd, invalid=invalid)
        assert md["counts"][5] == invalid.sum() >= 8 and md["counts"][3] >= 20 and md["counts"][4] >= 1, md["counts"]
        assert abs(np.linalg.det(T[:3, :3].astype(np.float64)) - 1) < 1e-5 and abs(T[0, 1]) > 0.05 and abs(T[1, 2]) > 0.05


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from cppflow_amd import _hip, build

    build.build()
    return _hip.lib()


NEW = ("cppf_voxel_scene_workspace_bytes", "cppf_scene_from_points", "cppf_scene_from_depth")


def test_entry_points_are_declared_bound_and_exported(lib):
    from cppflow_amd import _hip, build

    for fn in NEW:
        assert fn in declared_functions() and fn in _hip.SIGNATURES and getattr(lib, fn) is not None
    text = open(HEADER).read()
    assert int(re.search(r"#define CPPF_VOXEL_MAX_DIM (\d+)", text).group(1)) == _hip.VOXEL_MAX_DIM == 1024
    assert re.search(r"#define CPPF_VOXEL_MAX_CELLS \(1 << 24\)", text) and _hip.VOXEL_MAX_CELLS == 1 << 24
    assert int(re.search(r"#define CPPF_VOXEL_MAX_SELF (\d+)", text).group(1)) == _hip.VOXEL_MAX_SELF == 16
    assert ctypes.sizeof(_hip.VoxelGrid) == 28
    assert lib.cppf_abi_version() == 6  # additive: the ABI version stays
    assert "kernels_voxel.h" in build.HEADERS  # the build id covers the new kernels


def _grid(origin=(0.1, 0.2, 0.3), voxel=0.02, dims=(65, 5, 2)):
    from cppflow_amd import _hip

    return _hip.VoxelGrid((ctypes.c_float * 3)(*origin), voxel, (ctypes.c_int32 * 3)(*dims))


def _nbytes(lib, grid, n_self):
    from cppflow_amd import _hip

    out = ctypes.c_size_t(0)
    assert lib.cppf_voxel_scene_workspace_bytes(ctypes.byref(grid), n_self, ctypes.byref(out)) == _hip.CPPF_OK, lib.cppf_last_error().decode()
    return out.value


BUF = ctypes.c_void_p(0x1000)  # never dereferenced: every call here is refused before any launch


def _points(lib, h, **kw):
    a = dict(points=BUF, n=10, grid=_grid(), q_self=BUF, n_self=1, margin=0.03, capacity=64, box_lo=BUF, box_hi=BUF, counts=BUF,
             workspace=BUF, workspace_bytes=1 << 30)  # fmt: skip
    a.update(kw)
    g = ctypes.byref(a["grid"]) if a["grid"] is not None else None
    return lib.cppf_scene_from_points(h, a["points"], a["n"], g, a["q_self"], a["n_self"], a["margin"], a["capacity"], a["box_lo"],
                                      a["box_hi"], a["counts"], a["workspace"], a["workspace_bytes"], None)  # fmt: skip


def _depth(lib, h, **kw):
    a = dict(depth=BUF, height=8, width=10, intr=(50.0, 50.0, 5.0, 4.0), cam=tuple(np.eye(3).reshape(9)) + (0.0, 0.0, 0.0), z_min=0.1,
             z_max=3.0, grid=_grid(), q_self=BUF, n_self=1, margin=0.03, capacity=64, box_lo=BUF, box_hi=BUF, counts=BUF, workspace=BUF,
             workspace_bytes=1 << 30)  # fmt: skip
    a.update(kw)
    g = ctypes.byref(a["grid"]) if a["grid"] is not None else None
    intr = (ctypes.c_float * 4)(*a["intr"]) if a["intr"] is not None else None
    cam = (ctypes.c_float * 12)(*a["cam"]) if a["cam"] is not None else None
    return lib.cppf_scene_from_depth(h, a["depth"], a["height"], a["width"], intr, cam, a["z_min"], a["z_max"], g, a["q_self"],
                                     a["n_self"], a["margin"], a["capacity"], a["box_lo"], a["box_hi"], a["counts"], a["workspace"],
                                     a["workspace_bytes"], None)  # fmt: skip


def test_bad_arguments_are_refused_before_a_device_is_selected(lib):
    from cppflow_amd import _hip
    from cppflow_amd.robot_model import canonicalize
    from cppflow_amd.robot_zoo import ROBOT_SPECS

    nan, inf = float("nan"), float("inf")
    for call in (_points, _depth):
        assert call(lib, None) == _hip.CPPF_ERR_INVALID and "NULL" in lib.cppf_last_error().decode()  # a NULL handle with n_self > 0
    desc = _hip.chain_to_desc(canonicalize(ROBOT_SPECS["panda"]()))
    h = ctypes.c_void_p()
    assert lib.cppf_robot_create(ctypes.byref(desc), -12345, ctypes.byref(h)) == _hip.CPPF_OK, lib.cppf_last_error().decode()
    try:
        need = _nbytes(lib, _grid(), 1)
        shared = [(dict(**{name: None}), "NULL") for name in ("grid", "q_self", "box_lo", "box_hi", "counts", "workspace")]
        shared += [
            (dict(grid=_grid(dims=(0, 5, 2))), "dims"),
            (dict(grid=_grid(dims=(65, 1025, 2))), "dims"),
            (dict(grid=_grid(dims=(65, 5, -1))), "dims"),
            (dict(grid=_grid(dims=(1024, 1024, 17))), "cells"),
            (dict(grid=_grid(dims=(65, 1024, 129))), "cells"),  # (the padded row counts: 128 x 1024 x 129 > 2^24)
            (dict(n_self=-1), "n_self"),
            (dict(n_self=17), "n_self"),
            (dict(capacity=-1), "capacity"),
            (dict(capacity=4097), "capacity"),
            (dict(grid=_grid(voxel=0.0)), "voxel_m"),
            (dict(grid=_grid(voxel=-0.02)), "voxel_m"),
            (dict(grid=_grid(voxel=nan)), "voxel_m"),
            (dict(grid=_grid(voxel=inf)), "voxel_m"),
            (dict(grid=_grid(origin=(1e6, 0.2, 0.3), voxel=0.02)), "strictly increasing"),  # (0.02 is below half an ulp of 1e6)
            (dict(grid=_grid(origin=(0.1, nan, 0.3))), "strictly increasing"),
            (dict(grid=_grid(origin=(0.1, 0.2, 3.4e38), voxel=1e37)), "strictly increasing"),  # (a plane overflows)
            (dict(margin=-0.01), "self_margin_m"),
            (dict(margin=nan), "self_margin_m"),
            (dict(workspace_bytes=need - 1), "workspace"),
            (dict(workspace_bytes=0), "workspace"),
            (dict(workspace=ctypes.c_void_p(0x1004)), "aligned"),
        ]
        own = {
            _points: [(dict(points=None), "NULL"), (dict(n=-1), "n_points")],
            _depth: [(dict(depth=None), "NULL"), (dict(intr=None), "NULL"), (dict(cam=None), "NULL"), (dict(height=-1), "height"),
                     (dict(width=-3), "height"), (dict(height=1 << 16, width=1 << 15), "2^31"), (dict(z_min=1.0, z_max=1.0), "z_min"),
                     (dict(z_min=2.0, z_max=1.0), "z_min"), (dict(z_min=nan), "z_min"), (dict(z_max=nan), "z_min"),
                     (dict(intr=(0.0, 50.0, 5.0, 4.0)), "fx / fy"), (dict(intr=(50.0, nan, 5.0, 4.0)), "fx / fy"),
                     (dict(intr=(inf, 50.0, 5.0, 4.0)), "fx / fy"), (dict(intr=(50.0, -0.0, 5.0, 4.0)), "fx / fy")],
        }  # fmt: skip
        for call in (_points, _depth):
            for kw, word in shared + own[call]:
                assert call(lib, h, **kw) == _hip.CPPF_ERR_INVALID, (call.__name__, kw)
                assert word in lib.cppf_last_error().decode(), (call.__name__, kw, lib.cppf_last_error().decode())
        # (what is NOT refused -- n_self = 0 without a handle, capacity = 0 without boxes, n_points = 0 -- and the destroyed handle
        # need a device: tests/test_gpu_voxel_scene.py)
    finally:
        lib.cppf_robot_destroy(h)


def test_workspace_bytes(lib):
    from cppflow_amd import _hip

    for n_self in (0, 1, 16):
        prev = 0
        for dims in ((1, 1, 1), (63, 1, 1), (64, 2, 1), (65, 2, 2), (130, 5, 5), (128, 128, 64), (1024, 1024, 16)):
            b = _nbytes(lib, _grid(voxel=0.001, dims=dims), n_self)
            nxp = (dims[0] + 63) // 64 * 64
            assert b >= prev and b % 16 == 0 and b >= nxp * dims[1] * dims[2] // 8 + 8 * dims[1] * dims[2] and b > 0, (dims, b)
            prev = b
    assert _nbytes(lib, _grid(), 16) > _nbytes(lib, _grid(), 1) > _nbytes(lib, _grid(), 0)
    out = ctypes.c_size_t(0)
    for g, n_self in ((_grid(dims=(0, 1, 1)), 0), (_grid(), 17), (_grid(), -1), (_grid(voxel=0.0), 0)):
        assert lib.cppf_voxel_scene_workspace_bytes(ctypes.byref(g), n_self, ctypes.byref(out)) == _hip.CPPF_ERR_INVALID
        assert lib.cppf_last_error().decode()
    assert lib.cppf_voxel_scene_workspace_bytes(ctypes.byref(_grid()), 0, None) == _hip.CPPF_ERR_INVALID
    assert lib.cppf_voxel_scene_workspace_bytes(None, 0, ctypes.byref(out)) == _hip.CPPF_ERR_INVALID


# ---- the Problem's lists ----------------------------------------------------------------------------------------------------------------
def test_a_scene_survives_the_round_trip_through_the_problem_lists():
    from cppflow_amd.scene import ObstacleScene, cuboid_corners

    pts = V.point_recipe(1000, V.ORIGIN, V.VOXELS[2], (65, 5, 5), seed=3)
    m = V.scene_from_points(pts, V.ORIGIN, V.VOXELS[2], (65, 5, 5))
    assert len(m["lo"]) > 8
    sc = ObstacleScene(torch.from_numpy(m["lo"].copy()), torch.from_numpy(m["hi"].copy()), stats={"boxes_total": len(m["lo"])})
    cuboids, Ts = sc.as_problem_obstacles()
    assert len(cuboids) == len(Ts) == len(m["lo"]) and tuple(cuboids[0].shape) == (6,) and tuple(Ts[0].shape) == (4, 4)
    assert all(torch.equal(T, torch.eye(4)) for T in Ts)
    lo, hi = cuboid_corners(cuboids, Ts)
    assert np.array_equal(lo.view(np.int32), m["lo"].view(np.int32)) and np.array_equal(hi.view(np.int32), m["hi"].view(np.int32))
    back = ObstacleScene.from_cuboids(cuboids, Ts)
    assert torch.equal(back.lo.view(torch.int32), sc.lo.view(torch.int32)) and torch.equal(back.hi.view(torch.int32), sc.hi.view(torch.int32))
    assert back.stats is None and sc.to("cpu").stats == sc.stats
    empty = ObstacleScene(torch.zeros((0, 3)), torch.zeros((0, 3)))
    assert empty.as_problem_obstacles() == ([], [])
