"""Scenes fused over frames, without a GPU: the NumPy model of tests/voxel_map.py against its own definitions (the z-merged cuboids
tile the occupancy, are no more than the x/y boxes, and come sorted), and the C ABI of cppf_voxel_map_* / cppf_scene_from_map with
every refusal on a host-only handle."""

import ctypes
import re

import numpy as np
import pytest

from tests import voxel_map as M
from tests.test_abi import HEADER, declared_functions

F = np.float32


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def check_tiling(occ, ctx):
    zh = M.zheads(occ)
    cover = M.rasterise(zh, occ.shape)
    assert np.array_equal(cover, occ.astype(np.int32)), ctx  # the union is the occupancy, no cell twice
    assert sum((x1 - x0) * (y1 - y) * (z1 - z) for x0, x1, y, y1, z, z1 in zh) == int(occ.sum()), ctx
    assert len(zh) <= len(M.heads(occ)), ctx
    keys = [(z, y, x0) for x0, _, y, _, z, _ in zh]
    assert keys == sorted(keys) and len(set(keys)) == len(keys), ctx
    return zh


def test_the_z_merge_cases_tile_their_occupancy_and_give_the_expected_numbers():
    for name, (occ, n) in M.zmerge_cases().items():
        assert M.tiles_exactly(occ), name
        zh = check_tiling(occ, name)
        if n is not None:
            assert len(zh) == n, (name, zh)
    occ, _ = M.zmerge_cases()["a slab pair differing in one cell in one layer"]
    zh = M.zheads(occ)
    # the untouched slab is one cuboid over all four layers; the other one is cut where its layer differs
    assert (60, 70, 3, 5, 0, 4) in zh and (3, 40, 0, 2, 0, 2) in zh and (3, 40, 0, 2, 3, 4) in zh
    assert len(zh) < len(M.heads(occ))
    lo, hi = M.boxes_xyz(occ, M.ORIGIN, M.VOXELS[1])
    assert lo.dtype == F and M.cell_ranges(lo, hi, M.ORIGIN, M.VOXELS[1], occ.shape[::-1]) == zh


@pytest.mark.parametrize("seed", range(4))
def test_random_occupancies_are_tiled_exactly(seed):
    rng = np.random.RandomState(seed)
    for dims in M.GRIDS:
        for density in (0.0, 0.1, 0.5, 0.9, 1.0):
            occ = rng.uniform(size=dims[::-1]) < density
            if seed % 2:  # correlated along z, so that boxes do repeat
                occ[1:] = np.where(rng.uniform(size=occ[1:].shape[:2])[:, :, None] < 0.7, occ[:-1], occ[1:])
            zh = check_tiling(occ, (dims, density))
            lo, hi = M.boxes_xyz(occ, M.ORIGIN, M.VOXELS[seed % 3])
            assert bool((lo < hi).all()) and M.cell_ranges(lo, hi, M.ORIGIN, M.VOXELS[seed % 3], dims) == zh


def test_integrate_and_threshold():
    dims = (65, 4, 3)
    rng = np.random.RandomState(0)
    m = M.empty_map(dims)
    assert m.shape == (3, 4, 128)
    frames = [rng.uniform(size=dims[::-1]) < 0.4 for _ in range(5)]
    for occ in frames:
        m = M.integrate(m, occ)
    assert np.array_equal(m[:, :, :65], np.sum(frames, axis=0).astype(np.uint8)) and not m[:, :, 65:].any()
    again = M.empty_map(dims)
    for i in (3, 0, 4, 2, 1):
        again = M.integrate(again, frames[i])
    assert np.array_equal(again, m)  # (a sum: the order does not matter)
    assert np.array_equal(M.threshold(m, 1, 65), np.any(frames, axis=0)) and np.array_equal(M.threshold(m, 5, 65), np.all(frames, axis=0))
    assert not M.threshold(m, 6, 65).any()
    full = np.full((1, 1, 64), 254, dtype=np.uint8)
    one = np.ones((1, 1, 64), dtype=bool)
    assert bool((M.integrate(M.integrate(full, one), one) == 255).all())  # saturates


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from cppflow_amd import _hip, build

    build.build()
    return _hip.lib()


NEW = ("cppf_voxel_map_bytes", "cppf_voxel_map_clear", "cppf_voxel_map_add_points", "cppf_voxel_map_add_depth", "cppf_scene_from_map")


def test_entry_points_and_constants_are_declared_bound_and_exported(lib):
    from cppflow_amd import _hip

    for fn in NEW:
        assert fn in declared_functions() and fn in _hip.SIGNATURES and getattr(lib, fn) is not None
    text = open(HEADER).read()
    assert int(re.search(r"#define CPPF_VOXEL_MERGE_XY\s+(\d+)", text).group(1)) == _hip.VOXEL_MERGE_XY == M.MERGE_XY == 0
    assert int(re.search(r"#define CPPF_VOXEL_MERGE_XYZ\s+(\d+)", text).group(1)) == _hip.VOXEL_MERGE_XYZ == M.MERGE_XYZ == 1
    assert lib.cppf_abi_version() == 6  # additive: the ABI version stays
    flowed = re.sub(r"\s*\n \*\s*", " ", text)  # (the comment's line breaks taken out)
    for words in ("tiles its layer exactly", "the interiors of the cuboids are disjoint", "a function of the occupancy alone"):
        assert words in flowed, words  # the three properties of the z-merged list


def _grid(origin=(0.1, 0.2, 0.3), voxel=0.02, dims=(65, 5, 2)):
    from cppflow_amd import _hip

    return _hip.VoxelGrid((ctypes.c_float * 3)(*origin), voxel, (ctypes.c_int32 * 3)(*dims))


def _map_bytes(lib, grid):
    from cppflow_amd import _hip

    out = ctypes.c_size_t(0)
    assert lib.cppf_voxel_map_bytes(ctypes.byref(grid), ctypes.byref(out)) == _hip.CPPF_OK, lib.cppf_last_error().decode()
    return out.value


def test_map_bytes(lib):
    from cppflow_amd import _hip

    for dims in ((1, 1, 1), (63, 1, 1), (64, 2, 1), (65, 2, 2), (130, 5, 5), (128, 128, 64), (1024, 1024, 16)):
        assert _map_bytes(lib, _grid(voxel=0.001, dims=dims)) == 16 + M.padded(dims[0]) * dims[1] * dims[2], dims
    assert _map_bytes(lib, _grid(voxel=0.001, dims=(1024, 1024, 16))) == (16 << 20) + 16
    out = ctypes.c_size_t(0)
    for g in (_grid(dims=(0, 1, 1)), _grid(voxel=0.0), _grid(dims=(1024, 1024, 17))):
        assert lib.cppf_voxel_map_bytes(ctypes.byref(g), ctypes.byref(out)) == _hip.CPPF_ERR_INVALID and lib.cppf_last_error().decode()
    assert lib.cppf_voxel_map_bytes(ctypes.byref(_grid()), None) == _hip.CPPF_ERR_INVALID
    assert lib.cppf_voxel_map_bytes(None, ctypes.byref(out)) == _hip.CPPF_ERR_INVALID


BUF = ctypes.c_void_p(0x1000)  # never dereferenced: every call here is refused before any launch
MAPB = 16 + 128 * 5 * 2  # cppf_voxel_map_bytes of _grid()


def _points(lib, h, **kw):
    a = dict(points=BUF, n=10, grid=_grid(), q_self=BUF, n_self=1, margin=0.03, map=BUF, map_bytes=MAPB, counts=BUF, workspace=BUF,
             workspace_bytes=1 << 30)  # fmt: skip
    a.update(kw)
    g = ctypes.byref(a["grid"]) if a["grid"] is not None else None
    return lib.cppf_voxel_map_add_points(h, a["points"], a["n"], g, a["q_self"], a["n_self"], a["margin"], a["map"], a["map_bytes"],
                                         a["counts"], a["workspace"], a["workspace_bytes"], None)  # fmt: skip


def _depth(lib, h, **kw):
    a = dict(depth=BUF, height=8, width=10, intr=(50.0, 50.0, 5.0, 4.0), cam=tuple(np.eye(3).reshape(9)) + (0.0, 0.0, 0.0), z_min=0.1,
             z_max=3.0, grid=_grid(), q_self=BUF, n_self=1, margin=0.03, map=BUF, map_bytes=MAPB, counts=BUF, workspace=BUF,
             workspace_bytes=1 << 30)  # fmt: skip
    a.update(kw)
    g = ctypes.byref(a["grid"]) if a["grid"] is not None else None
    intr = (ctypes.c_float * 4)(*a["intr"]) if a["intr"] is not None else None
    cam = (ctypes.c_float * 12)(*a["cam"]) if a["cam"] is not None else None
    return lib.cppf_voxel_map_add_depth(h, a["depth"], a["height"], a["width"], intr, cam, a["z_min"], a["z_max"], g, a["q_self"],
                                        a["n_self"], a["margin"], a["map"], a["map_bytes"], a["counts"], a["workspace"],
                                        a["workspace_bytes"], None)  # fmt: skip


def _scene(lib, _h=None, **kw):
    a = dict(map=BUF, map_bytes=MAPB, grid=_grid(), min_frames=1, merge=1, capacity=64, box_lo=BUF, box_hi=BUF, counts=BUF, workspace=BUF,
             workspace_bytes=1 << 30)  # fmt: skip
    a.update(kw)
    g = ctypes.byref(a["grid"]) if a["grid"] is not None else None
    return lib.cppf_scene_from_map(a["map"], a["map_bytes"], g, a["min_frames"], a["merge"], a["capacity"], a["box_lo"], a["box_hi"],
                                   a["counts"], a["workspace"], a["workspace_bytes"], None)  # fmt: skip


def _clear(lib, _h=None, **kw):
    a = dict(map=BUF, map_bytes=MAPB, grid=_grid())
    a.update(kw)
    g = ctypes.byref(a["grid"]) if a["grid"] is not None else None
    return lib.cppf_voxel_map_clear(a["map"], a["map_bytes"], g, None)


def test_bad_arguments_are_refused_before_a_device_is_selected(lib):
    from cppflow_amd import _hip
    from cppflow_amd.robot_model import canonicalize
    from cppflow_amd.robot_zoo import ROBOT_SPECS

    nan, inf = float("nan"), float("inf")
    assert MAPB == _map_bytes(lib, _grid())
    for call in (_points, _depth):
        assert call(lib, None) == _hip.CPPF_ERR_INVALID and "NULL" in lib.cppf_last_error().decode()  # a NULL handle with n_self > 0
    desc = _hip.chain_to_desc(canonicalize(ROBOT_SPECS["panda"]()))
    h = ctypes.c_void_p()
    assert lib.cppf_robot_create(ctypes.byref(desc), -12345, ctypes.byref(h)) == _hip.CPPF_OK, lib.cppf_last_error().decode()
    try:
        need1 = ctypes.c_size_t(0)
        assert lib.cppf_voxel_scene_workspace_bytes(ctypes.byref(_grid()), 1, ctypes.byref(need1)) == _hip.CPPF_OK
        need0 = ctypes.c_size_t(0)
        assert lib.cppf_voxel_scene_workspace_bytes(ctypes.byref(_grid()), 0, ctypes.byref(need0)) == _hip.CPPF_OK
        grid_cases = [
            (dict(grid=None), "NULL"),
            (dict(grid=_grid(dims=(0, 5, 2))), "dims"),
            (dict(grid=_grid(dims=(65, 1025, 2))), "dims"),
            (dict(grid=_grid(dims=(65, 5, -1))), "dims"),
            (dict(grid=_grid(dims=(1024, 1024, 17))), "cells"),
            (dict(grid=_grid(dims=(65, 1024, 129))), "cells"),
            (dict(grid=_grid(voxel=0.0)), "voxel_m"),
            (dict(grid=_grid(voxel=-0.02)), "voxel_m"),
            (dict(grid=_grid(voxel=nan)), "voxel_m"),
            (dict(grid=_grid(voxel=inf)), "voxel_m"),
            (dict(grid=_grid(origin=(1e6, 0.2, 0.3), voxel=0.02)), "strictly increasing"),
            (dict(grid=_grid(origin=(0.1, nan, 0.3))), "strictly increasing"),
            (dict(grid=_grid(origin=(0.1, 0.2, 3.4e38), voxel=1e37)), "strictly increasing"),
        ]
        map_cases = [
            (dict(map=None), "map is NULL"),
            (dict(map=ctypes.c_void_p(0x1008)), "map must be 16-byte aligned"),
            (dict(map_bytes=MAPB - 16), "map_bytes"),  # short
            (dict(map_bytes=MAPB + 16), "map_bytes"),
            (dict(map_bytes=0), "map_bytes"),
            (dict(grid=_grid(dims=(129, 5, 2))), "map_bytes"),  # (another grid's map)
        ]
        scratch_cases = [
            (dict(counts=None), "NULL"),
            (dict(workspace=None), "NULL"),
            (dict(workspace_bytes=0), "workspace"),
            (dict(workspace=ctypes.c_void_p(0x1004)), "aligned"),
        ]
        frame_cases = [
            (dict(q_self=None), "NULL"),
            (dict(n_self=-1), "n_self"),
            (dict(n_self=17), "n_self"),
            (dict(margin=-0.01), "self_margin_m"),
            (dict(margin=nan), "self_margin_m"),
            (dict(workspace_bytes=need1.value - 1), "workspace"),
        ]
        own = {
            _points: frame_cases + [(dict(points=None), "NULL"), (dict(n=-1), "n_points")],
            _depth: frame_cases + [(dict(depth=None), "NULL"), (dict(intr=None), "NULL"), (dict(cam=None), "NULL"), (dict(height=-1), "height"),
                     (dict(width=-3), "height"), (dict(height=1 << 16, width=1 << 15), "2^31"), (dict(z_min=1.0, z_max=1.0), "z_min"),
                     (dict(z_min=2.0, z_max=1.0), "z_min"), (dict(z_min=nan), "z_min"), (dict(z_max=nan), "z_min"),
                     (dict(intr=(0.0, 50.0, 5.0, 4.0)), "fx / fy"), (dict(intr=(50.0, nan, 5.0, 4.0)), "fx / fy"),
                     (dict(intr=(inf, 50.0, 5.0, 4.0)), "fx / fy"), (dict(intr=(50.0, -0.0, 5.0, 4.0)), "fx / fy")],
            _scene: [(dict(min_frames=0), "min_frames"), (dict(min_frames=256), "min_frames"), (dict(min_frames=-1), "min_frames"),
                     (dict(merge=2), "merge"), (dict(merge=-1), "merge"), (dict(capacity=-1), "capacity"), (dict(capacity=4097), "capacity"),
                     (dict(box_lo=None), "NULL"), (dict(box_hi=None), "NULL"), (dict(workspace_bytes=need0.value - 1), "workspace")],
        }  # fmt: skip
        for call in (_points, _depth, _scene):
            for kw, word in grid_cases + map_cases + scratch_cases + own[call]:
                assert call(lib, h, **kw) == _hip.CPPF_ERR_INVALID, (call.__name__, kw)
                assert word in lib.cppf_last_error().decode(), (call.__name__, kw, lib.cppf_last_error().decode())
        for kw, word in grid_cases + map_cases:
            assert _clear(lib, **kw) == _hip.CPPF_ERR_INVALID, ("clear", kw)
            assert word in lib.cppf_last_error().decode(), ("clear", kw, lib.cppf_last_error().decode())
        # (what is NOT refused -- n_self = 0 without a handle, capacity = 0 without boxes, n_points = 0 -- needs a device:
        # tests/test_gpu_voxel_map.py)
    finally:
        lib.cppf_robot_destroy(h)
