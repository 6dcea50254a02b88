"""Scenes from sensor data on the MI355X: cppf_scene_from_points / cppf_scene_from_depth (csrc/kernels_voxel.h) bit for bit against
the NumPy float32 model of tests/voxel_scene.py (what its recipes exercise is asserted in tests/test_voxel_scene_model.py), exact
containment, the self filter against fp64 capsule geometry, soundness through cppf_scene_env_collisions, memory discipline and
determinism, graph capture, coarsening, and a plan on a sensed scene.

Every raw call runs in a poisoned arena (`run_in_arena`): outputs and workspace are carved out of one buffer with guard gaps, and
whatever lies beyond the `written` boxes -- inside the capacity and beyond it -- must still hold the poison afterwards.

The self filter's tolerance: the recipe keeps only points whose fp64 value min_c(dist - r_c - margin) is at least 1e-4 m away from 0
(a condition on the inputs, not a measurement: positions of ~1.5 m carry 1.2e-7 m per fp32 rounding and the capsule FK a few of
those); inside that the device's classes must equal the fp64 reference exactly."""

import ctypes
import functools
import gc
import os

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import voxel_scene as V

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF = os.path.join(GOLDEN, "reference_files")
NS = (0, 1, 63, 64, 65, 1000)
NXS = (1, 63, 64, 65, 130)
NYZ = (1, 2, 5)


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


@functools.lru_cache(maxsize=None)
def robot(name):
    from cppflow_amd.robot_zoo import ROBOT_SPECS
    from cppflow_amd.robots import Robot

    return Robot(ROBOT_SPECS[name]())


def make_grid(origin, voxel, dims):
    from cppflow_amd import _hip

    return _hip.VoxelGrid((ctypes.c_float * 3)(*[float(v) for v in origin]), float(voxel), (ctypes.c_int32 * 3)(*[int(d) for d in dims]))


def run_in_arena(source, origin, voxel, dims, capacity, rb=None, q_self=None, margin=0.03, poison=0xA5, stream=None):
    """source = ("points", tensor [n, 3]) or ("depth", tensor [H, W], intrinsics, cam_to_world 4x4, z_min, z_max) -> dict(lo, hi (the
    written boxes, host f32), counts).  Asserts that nothing but the written boxes, counts and the workspace was touched."""
    from cppflow_amd import _hip

    lib = _hip.lib()
    grid = make_grid(origin, voxel, dims)
    n_self = 0 if q_self is None else int(q_self.shape[0])
    handle = rb._handle(torch.device(DEV)) if n_self > 0 else None
    nbytes = ctypes.c_size_t(0)
    _hip.check(lib.cppf_voxel_scene_workspace_bytes(ctypes.byref(grid), n_self, ctypes.byref(nbytes)))
    total = nbytes.value + 2 * 12 * capacity + 32 + 5 * 1024 + 3 * 4096 + 4 * 256
    arena = torch.full((total,), poison, dtype=torch.uint8, device=DEV)
    cursor, spans, bufs = 4096, {}, {}
    for nm, nb in (("workspace", nbytes.value), ("lo", 12 * capacity), ("hi", 12 * capacity), ("counts", 32)):
        start = (cursor + 255) // 256 * 256
        bufs[nm] = arena[start : start + nb]
        spans[nm] = (start, start + nb)
        cursor = start + nb + 1024
    assert cursor + 4096 <= arena.numel()
    torch.cuda.synchronize()
    st = (stream if stream is not None else torch.cuda.current_stream(DEV)).cuda_stream
    # (zero-sized outputs: a pointer into the arena all the same -- capacity = 0 must not write through it)
    ptr = {nm: arena.data_ptr() + spans[nm][0] for nm in spans}
    tail = (ctypes.byref(grid), q_self.data_ptr() if n_self else None, n_self, float(margin), capacity, ptr["lo"], ptr["hi"], ptr["counts"],
            ptr["workspace"], nbytes.value, st)  # fmt: skip
    if source[0] == "points":
        pts = source[1]
        rc = lib.cppf_scene_from_points(handle, pts.data_ptr() if pts.shape[0] else None, int(pts.shape[0]), *tail)
    else:
        _, depth, intr, T, z_min, z_max = source
        T = np.asarray(T, dtype=F)
        k = (ctypes.c_float * 4)(*[float(v) for v in intr])
        rt = (ctypes.c_float * 12)(*[float(v) for v in np.concatenate([T[:3, :3].reshape(9), T[:3, 3]])])
        rc = lib.cppf_scene_from_depth(handle, depth.data_ptr(), int(depth.shape[0]), int(depth.shape[1]), k, rt, float(z_min), float(z_max),
                                       *tail)  # fmt: skip
    _hip.check(rc)
    torch.cuda.synchronize()
    counts = host(bufs["counts"]).copy().view(np.int32)
    written = int(counts[1])
    assert 0 <= written <= capacity and written == min(int(counts[0]), capacity), counts
    keep = torch.ones(arena.numel(), dtype=torch.bool, device=DEV)
    for nm, (a, b) in spans.items():
        keep[a : (a + 12 * written if nm in ("lo", "hi") else b)] = False
    assert bool((arena[keep] == poison).all()), "something beyond the written boxes, counts and the workspace was written"
    lo = host(bufs["lo"][: 12 * written]).copy().view(F).reshape(-1, 3)
    hi = host(bufs["hi"][: 12 * written]).copy().view(F).reshape(-1, 3)
    return dict(lo=lo, hi=hi, counts=counts)


def check_against_model(got, m, capacity, ctx):
    want = m["counts"].copy()
    want[1] = min(int(want[0]), capacity)
    assert np.array_equal(got["counts"], want), (ctx, got["counts"], want)
    w = int(want[1])
    assert np.array_equal(bits(got["lo"]), bits(m["lo"][:w])) and np.array_equal(bits(got["hi"]), bits(m["hi"][:w])), ctx


# ---- 1. bit for bit against the model --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", NXS)
def test_points_bit_for_bit_against_the_model(nx):
    case = 0
    for ny in NYZ:
        for nz in NYZ:
            for n in NS:
                voxel = V.VOXELS[case % 3]
                case += 1
                dims = (nx, ny, nz)
                pts = V.point_recipe(n, V.ORIGIN, voxel, dims, seed=case)
                m = V.scene_from_points(pts, V.ORIGIN, voxel, dims)
                total = len(m["lo"])
                for capacity in sorted({0, max(total - 1, 0), total, V.MAX_BOXES}):
                    got = run_in_arena(("points", dev(pts).reshape(-1, 3)), V.ORIGIN, voxel, dims, capacity)
                    check_against_model(got, m, capacity, (dims, n, float(voxel), capacity))


def test_thousands_of_points_in_one_cell_and_containment():
    """the pile (3000 points in one cell: the same word, the same bit), and every kept point in [lo, hi) of exactly one written box --
    by the device's own corners"""
    dims, voxel = (130, 5, 5), V.VOXELS[1]
    pts = V.point_recipe(1000, V.ORIGIN, voxel, dims, seed=11, pile=3000)
    m = V.scene_from_points(pts, V.ORIGIN, voxel, dims)
    got = run_in_arena(("points", dev(pts)), V.ORIGIN, voxel, dims, V.MAX_BOXES)
    check_against_model(got, m, V.MAX_BOXES, "pile")
    kept = pts[m["classes"] == V.KEPT]
    assert len(kept) >= 3064
    inside = V.contained(kept, got["lo"], got["hi"]).sum(axis=1)
    assert bool((inside == 1).all()), np.flatnonzero(inside != 1)[:10]
    rest = pts[(m["classes"] == V.OUTSIDE)]
    assert bool((V.contained(rest, got["lo"], got["hi"]).sum(axis=1) == 0).all())  # (the boxes lie inside the grid)


@pytest.mark.parametrize("shape", [(8, 10), (33, 65)])
def test_depth_bit_for_bit_against_the_model(shape):
    depth, intr, T, z_min, z_max, origin, voxel, dims = V.depth_recipe(*shape)
    pts, invalid = V.back_project(depth, intr, T, z_min, z_max)
    m = V.scene_from_points(pts, origin, voxel, dims, invalid=invalid)
    total = len(m["lo"])
    assert total >= 2
    for capacity in (V.MAX_BOXES, total, total - 1, 0):
        got = run_in_arena(("depth", dev(depth), intr, T, z_min, z_max), origin, voxel, dims, capacity)
        check_against_model(got, m, capacity, (shape, capacity))
    kept = pts[m["classes"] == V.KEPT]
    got = run_in_arena(("depth", dev(depth), intr, T, z_min, z_max), origin, voxel, dims, V.MAX_BOXES)
    assert bool((V.contained(kept, got["lo"], got["hi"]).sum(axis=1) == 1).all())
    # the point form on the model's back-projected points gives the same list: the two forms share everything behind the point
    same = run_in_arena(("points", dev(pts[~invalid])), origin, voxel, dims, V.MAX_BOXES)
    assert np.array_equal(bits(same["lo"]), bits(got["lo"])) and np.array_equal(bits(same["hi"]), bits(got["hi"]))


# ---- 2. the self filter ----------------------------------------------------------------------------------------------------------------
SELF_ORIGIN, SELF_VOXEL, SELF_DIMS = (F(-1.6013), F(-1.6007), F(-0.4011)), F(0.02), (160, 160, 140)


def seg_dist(p, p0, p1):
    """fp64 distances [n, m] of points p [n, 3] from the segments p0 -> p1 [m, 3]"""
    d = p1 - p0
    dd = (d * d).sum(axis=1)
    t = np.where(dd > 0, ((p[:, None, :] - p0[None]) * d[None]).sum(axis=2) / np.where(dd > 0, dd, 1.0), 0.0)
    c = p0[None] + np.clip(t, 0.0, 1.0)[:, :, None] * d[None]
    return np.linalg.norm(p[:, None, :] - c, axis=2)


def device_occupancy(lo, hi, origin, voxel, dims):
    """the cells a written box list covers (every corner must BE a plane)"""
    P = V.grid_planes(origin, voxel, dims)
    occ = np.zeros(dims[::-1], dtype=bool)
    idx = []
    for k in range(3):
        a, b = np.searchsorted(P[k], lo[:, k]), np.searchsorted(P[k], hi[:, k])
        assert np.array_equal(P[k][a], lo[:, k]) and np.array_equal(P[k][np.minimum(b, dims[k])], hi[:, k])
        idx.append((a, b))
    for i in range(lo.shape[0]):
        occ[idx[2][0][i] : idx[2][1][i], idx[1][0][i] : idx[1][1][i], idx[0][0][i] : idx[0][1][i]] = True
    return occ


@pytest.mark.parametrize("name", ["panda", "fetch"])
def test_self_filter_equals_the_fp64_reference(name):
    margin = 0.03
    rng = np.random.RandomState(5)
    x = H.random_configs(name, 4)
    ends = H.oracle64(name).capsule_endpoints(x)  # [4, ncaps, 6]
    r = np.asarray(H.chain(name).cap_r, dtype=np.float64)
    p0, p1 = ends[:, :, :3].reshape(-1, 3), ends[:, :, 3:].reshape(-1, 3)
    rr = np.tile(r, 4)
    pts = []
    for s in range(p0.shape[0]):
        for _ in range(12):
            a = p0[s] + rng.uniform() * (p1[s] - p0[s])
            axis = p1[s] - p0[s]
            u = np.cross(axis, rng.randn(3)) if np.linalg.norm(axis) > 0 else rng.randn(3)
            u /= np.linalg.norm(u)
            delta = rng.choice([-1.0, 1.0]) * 10 ** rng.uniform(np.log10(2e-4), np.log10(0.03))
            pts.append(a + u * (rr[s] + margin + delta))
    pts = np.asarray(pts, dtype=F)
    f = (seg_dist(pts.astype(np.float64), p0, p1) - rr[None] - margin).min(axis=1)
    cls0, cells = V.classify(pts, SELF_ORIGIN, SELF_VOXEL, SELF_DIMS)
    keep = (np.abs(f) >= 1e-4) & (cls0 == V.KEPT)
    pts, f, cells = pts[keep], f[keep], cells[keep]
    is_self = f < 0
    assert int(is_self.sum()) >= 64 and int((~is_self).sum()) >= 64, (int(is_self.sum()), int((~is_self).sum()))
    rb, q = robot(name), dev(x)
    # all at once: the counts
    got = run_in_arena(("points", dev(pts)), SELF_ORIGIN, SELF_VOXEL, SELF_DIMS, V.MAX_BOXES, rb=rb, q_self=q, margin=margin)
    assert got["counts"][6] == is_self.sum() and got["counts"][3] == (~is_self).sum() and got["counts"][4] == got["counts"][5] == 0, got["counts"]
    # per point: groups of points in pairwise different cells, so that a cell's bit IS its point's class
    flat = (cells[:, 2] * SELF_DIMS[1] + cells[:, 1]) * SELF_DIMS[0] + cells[:, 0]
    rank = np.zeros(len(flat), dtype=np.int64)
    seen = {}
    for i, c in enumerate(flat.tolist()):
        rank[i] = seen.get(c, 0)
        seen[c] = rank[i] + 1
    for g in range(int(rank.max()) + 1):
        sel = rank == g
        got = run_in_arena(("points", dev(pts[sel])), SELF_ORIGIN, SELF_VOXEL, SELF_DIMS, V.MAX_BOXES, rb=rb, q_self=q, margin=margin)
        occ = device_occupancy(got["lo"], got["hi"], SELF_ORIGIN, SELF_VOXEL, SELF_DIMS)
        c = cells[sel]
        assert np.array_equal(occ[c[:, 2], c[:, 1], c[:, 0]], ~is_self[sel]), g
        assert int(occ.sum()) == int((~is_self[sel]).sum()) == got["counts"][2]
    # the filter off keeps them all; one configuration of the four filters a subset
    off = run_in_arena(("points", dev(pts)), SELF_ORIGIN, SELF_VOXEL, SELF_DIMS, V.MAX_BOXES)
    assert off["counts"][3] == len(pts) and off["counts"][6] == 0
    one = run_in_arena(("points", dev(pts)), SELF_ORIGIN, SELF_VOXEL, SELF_DIMS, V.MAX_BOXES, rb=rb, q_self=q[1:2].contiguous(), margin=margin)
    f1 = (seg_dist(pts.astype(np.float64), p0.reshape(4, -1, 3)[1], p1.reshape(4, -1, 3)[1]) - r[None] - margin).min(axis=1)
    sure = np.abs(f1) >= 1e-4
    assert int((f1[sure] < 0).sum()) <= one["counts"][6] <= int((f1[sure] < 0).sum()) + int((~sure).sum())


# ---- 3. soundness through the consumers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["panda", "fetch"])
def test_a_scene_of_the_robots_own_axis_points_hits_that_row_and_the_filter_empties_it(name):
    rb = robot(name)
    x = H.random_configs(name, 6, seed=9)
    xd = dev(x)
    ends = H.oracle64(name).capsule_endpoints(x)
    for r in range(x.shape[0]):
        C, Hh = 0.5 * (ends[r, :, :3] + ends[r, :, 3:]), 0.5 * (ends[r, :, 3:] - ends[r, :, :3])
        pts = np.concatenate([C + u * Hh for u in np.linspace(-1.0, 1.0, 9)], axis=0).astype(F)
        sc = rb.scene_from_points(dev(pts), SELF_ORIGIN, float(SELF_VOXEL), SELF_DIMS, q_self=None)
        assert sc.stats["kept_points"] == len(pts) and sc.stats["outside_points"] == 0 and sc.n_obstacles >= 1, sc.stats
        mask = rb.scene_env_collisions(xd, sc.lo, sc.hi, want=("env_mask",))["env_mask"]
        assert bool(mask[r]), (name, r)  # (an axis point lies in a box: the segment's distance to it is 0 < r_c)
        empty = rb.scene_from_points(dev(pts), SELF_ORIGIN, float(SELF_VOXEL), SELF_DIMS, q_self=xd[r], self_margin_m=0.03)
        assert empty.n_obstacles == 0 and empty.stats["self_points"] == len(pts) and empty.stats["occupied_cells"] == 0, empty.stats
        assert tuple(empty.lo.shape) == (0, 3) and empty.lo.device == xd.device


# ---- 4. memory, determinism, graph capture, what is and is not refused ----------------------------------------------------------------------
def test_memory_discipline_and_determinism():
    dims, voxel = (130, 5, 5), V.VOXELS[2]
    pts = V.point_recipe(1000, V.ORIGIN, voxel, dims, seed=4, pile=2000)
    q = dev(H.random_configs("panda", 3, seed=2))
    depth, intr, T, z_min, z_max, origin, dvoxel, ddims = V.depth_recipe(33, 65)
    cases = [
        (("points", dev(pts)), V.ORIGIN, voxel, dims, dict()),
        (("points", dev(pts)), V.ORIGIN, voxel, dims, dict(rb=robot("panda"), q_self=q, margin=0.05)),
        (("depth", dev(depth), intr, T, z_min, z_max), origin, dvoxel, ddims, dict()),
    ]
    for source, o, v, d, kw in cases:
        before = source[1].clone()
        runs = [run_in_arena(source, o, v, d, 300, poison=0xA5, **kw), run_in_arena(source, o, v, d, 300, poison=0x5A, **kw),
                run_in_arena(source, o, v, d, 300, poison=0xFF, stream=torch.cuda.Stream(device=DEV), **kw)]  # fmt: skip
        for r in runs[1:]:  # (three poisons: an uninitialised workspace word that was read would show)
            for nm in ("lo", "hi", "counts"):
                assert np.array_equal(r[nm].view(np.int32), runs[0][nm].view(np.int32)), nm
        assert torch.equal(source[1].view(torch.int32), before.view(torch.int32))
        assert runs[0]["counts"][0] >= 2
    m = V.scene_from_points(pts, V.ORIGIN, voxel, dims)
    check_against_model(run_in_arena(cases[0][0], V.ORIGIN, voxel, dims, 300), m, 300, "arena")


def test_graph_capture_replays_the_call():
    from cppflow_amd import _hip

    lib = _hip.lib()
    dims, voxel = (65, 5, 2), V.VOXELS[1]
    pts = dev(V.point_recipe(1000, V.ORIGIN, voxel, dims, seed=6))
    rb, q = robot("panda"), dev(H.random_configs("panda", 2, seed=1))
    want = run_in_arena(("points", pts), V.ORIGIN, voxel, dims, 128, rb=rb, q_self=q)
    grid = make_grid(V.ORIGIN, voxel, dims)
    nbytes = ctypes.c_size_t(0)
    _hip.check(lib.cppf_voxel_scene_workspace_bytes(ctypes.byref(grid), 2, ctypes.byref(nbytes)))
    lo, hi = (torch.empty((128, 3), dtype=torch.float32, device=DEV) for _ in range(2))
    counts = torch.empty(8, dtype=torch.int32, device=DEV)
    work = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
    handle = rb._handle(torch.device(DEV))

    def call(stream):
        _hip.check(lib.cppf_scene_from_points(handle, pts.data_ptr(), 1000, ctypes.byref(grid), q.data_ptr(), 2, 0.03, 128, lo.data_ptr(),
                                              hi.data_ptr(), counts.data_ptr(), work.data_ptr(), nbytes.value, stream.cuda_stream))  # fmt: skip

    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        call(side)
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            call(side)
    for _ in range(2):
        for t in (lo, hi, counts, work):
            t.view(torch.uint8).fill_(0x77)
        g.replay()
        torch.cuda.synchronize()
        w = int(want["counts"][1])
        assert np.array_equal(host(counts), want["counts"])
        assert np.array_equal(bits(host(lo[:w])), bits(want["lo"])) and np.array_equal(bits(host(hi[:w])), bits(want["hi"]))
        assert bool((lo[w:].contiguous().view(torch.uint8) == 0x77).all()) and bool((hi[w:].contiguous().view(torch.uint8) == 0x77).all())


def test_what_needs_no_handle_no_points_and_no_boxes_and_the_destroyed_handle():
    from cppflow_amd import _hip
    from cppflow_amd.robot_zoo import ROBOT_SPECS
    from cppflow_amd.robots import Robot

    lib = _hip.lib()
    dims, voxel = (65, 2, 2), V.VOXELS[0]
    none = run_in_arena(("points", torch.empty((0, 3), dtype=torch.float32, device=DEV)), V.ORIGIN, voxel, dims, 16)
    assert np.array_equal(none["counts"], np.zeros(8, dtype=np.int32)) and none["lo"].shape == (0, 3)
    empty = robot("panda").scene_from_points(torch.empty((0, 3), dtype=torch.float32, device=DEV), V.ORIGIN, float(voxel), dims)
    assert empty.n_obstacles == 0 and empty.stats["boxes_total"] == 0 and empty.stats["rounds"] == 1
    # capacity 0 with NULL boxes: the counts alone
    pts = dev(V.point_recipe(64, V.ORIGIN, voxel, dims, seed=1))
    grid = make_grid(V.ORIGIN, voxel, dims)
    nbytes = ctypes.c_size_t(0)
    _hip.check(lib.cppf_voxel_scene_workspace_bytes(ctypes.byref(grid), 0, ctypes.byref(nbytes)))
    counts = torch.full((8,), -1, dtype=torch.int32, device=DEV)
    work = torch.empty(nbytes.value, dtype=torch.uint8, device=DEV)
    _hip.check(lib.cppf_scene_from_points(None, pts.data_ptr(), 64, ctypes.byref(grid), None, 0, 0.0, 0, None, None, counts.data_ptr(),
                                          work.data_ptr(), nbytes.value, torch.cuda.current_stream(DEV).cuda_stream))  # fmt: skip
    torch.cuda.synchronize()
    m = V.scene_from_points(host(pts), V.ORIGIN, voxel, dims, capacity=0)
    assert np.array_equal(host(counts), m["counts"]) and m["counts"][0] > 0 and m["counts"][1] == 0
    # a handle that cppf_robot_destroy has marked dead (kept allocated by a live batch): refused, nothing launched
    rb = Robot(ROBOT_SPECS["panda"]())
    x0, target = H.lm_problem("panda", 4, 64, seed=1)
    x0, target = dev(x0), dev(target)
    plan = rb.lm_batch_plan([dict(x=x0, target=target, x_out=torch.empty_like(x0))], 1e-6, 3.5, 0.35, n_steps=3)
    handle = rb._handle(torch.device(DEV))
    plan._keep[0] = None
    lib.cppf_robot_destroy(handle)
    rb._handles = {}
    del rb
    gc.collect()
    q = dev(H.random_configs("panda", 1))
    counts.fill_(7)
    ws = torch.full((1 << 16,), 7, dtype=torch.uint8, device=DEV)
    rc = lib.cppf_scene_from_points(handle, pts.data_ptr(), 64, ctypes.byref(grid), q.data_ptr(), 1, 0.03, 0, None, None, counts.data_ptr(),
                                    ws.data_ptr(), ws.numel(), None)  # fmt: skip
    assert rc == _hip.CPPF_ERR_INVALID and "destroyed" in lib.cppf_last_error().decode()
    torch.cuda.synchronize()
    assert bool((counts == 7).all()) and bool((ws == 7).all())
    del plan
    gc.collect()


# ---- 5. coarsening ----------------------------------------------------------------------------------------------------------------------
def test_coarsening_takes_extra_rounds_and_never_truncates():
    rb = robot("panda")
    origin, voxel, dims = V.ORIGIN, float(V.VOXELS[1]), (32, 32, 8)
    rng = np.random.RandomState(3)
    P = V.grid_planes(origin, V.VOXELS[1], dims)
    lo = np.array([P[k][0] for k in range(3)], dtype=np.float64) + 1e-4
    hi = np.array([P[k][-1] for k in range(3)], dtype=np.float64) - 1e-4
    pts = rng.uniform(lo, hi, size=(20000, 3)).astype(F)
    fine = V.scene_from_points(pts, origin, V.VOXELS[1], dims)
    assert len(fine["lo"]) > 4 and fine["counts"][3] == len(pts)
    with pytest.raises(RuntimeError, match="boxes"):
        rb.scene_from_points(dev(pts), origin, voxel, dims, max_cuboids=4, coarsen=False)
    sc = rb.scene_from_points(dev(pts), origin, voxel, dims, max_cuboids=4)
    assert 2 <= sc.stats["rounds"] <= 4 and sc.n_obstacles == sc.stats["boxes_total"] <= 4, sc.stats
    k = sc.stats["rounds"] - 1
    assert sc.stats["voxel_m"] == float(V.VOXELS[1] * F(2**k)) and sc.stats["dims"] == tuple(-(-d // 2**k) for d in dims)
    assert sc.stats["kept_points"] == len(pts)
    assert bool((V.contained(pts, host(sc.lo), host(sc.hi)).sum(axis=1) == 1).all())  # every kept point, by the device's own corners
    m = V.scene_from_points(pts, origin, V.VOXELS[1] * F(2**k), sc.stats["dims"])
    assert np.array_equal(bits(host(sc.lo)), bits(m["lo"])) and np.array_equal(bits(host(sc.hi)), bits(m["hi"]))
    # what cannot fit even then: one box per cell of a checkerboard, max_cuboids = 0
    with pytest.raises(RuntimeError, match="coarsening"):
        rb.scene_from_points(dev(pts), origin, voxel, dims, max_cuboids=0)
    whole = rb.scene_from_points(dev(pts), origin, voxel, dims)
    assert whole.stats["rounds"] == 1 and whole.n_obstacles == len(fine["lo"])
    assert np.array_equal(bits(host(whole.lo)), bits(fine["lo"]))


# ---- 6. end to end: a plan on a sensed scene -------------------------------------------------------------------------------------------------
def test_a_plan_on_the_sensed_cube():
    from cppflow_amd.data_type_utils import problem_from_filename
    from cppflow_amd.data_types import PlannerSettings
    from cppflow_amd.planners import CppFlowPlanner, TrackingSeedProvider
    from cppflow_amd.scene import ObstacleScene, problem_with_scene

    base = problem_from_filename(None, "panda__1cube_mini", problems_dir=os.path.join(REF, "problems"), paths_dir=os.path.join(REF, "paths"),
                                 device=DEV)  # fmt: skip
    assert len(base.obstacles_cuboids) == 1
    clo, chi = H.box_corners([host(base.obstacles_cuboids[0])], [host(base.obstacles_Tcuboids[0])])
    clo, chi = clo[0], chi[0]
    voxel = 0.05
    # the cube's six faces, sampled at 2 cm: finer than the voxel
    axes = [np.arange(clo[k], chi[k] + 1e-9, 0.02) for k in range(3)]
    axes = [np.append(a, chi[k]) for k, a in enumerate(axes)]
    faces = []
    for k in range(3):
        i, j = (k + 1) % 3, (k + 2) % 3
        a, b = np.meshgrid(axes[i], axes[j], indexing="ij")
        for side in (clo[k], chi[k]):
            p = np.zeros((a.size, 3))
            p[:, k], p[:, i], p[:, j] = side, a.ravel(), b.ravel()
            faces.append(p)
    cloud = dev(np.concatenate(faces, axis=0).astype(F))
    origin = tuple(float(v) for v in (clo - 0.113))
    dims = tuple(int(np.ceil((chi[k] - clo[k] + 0.226) / voxel)) for k in range(3))
    rb = base.robot
    scene = rb.scene_from_points(cloud, origin, voxel, dims, q_self=None)
    assert scene.stats["kept_points"] == cloud.shape[0] and 8 < scene.n_obstacles <= 4096, scene.stats
    problem = problem_with_scene(base, scene)
    assert problem.uses_scene and problem.n_obstacles == scene.n_obstacles and problem.robot is rb and base.n_obstacles == 1
    cached = problem.scene(DEV)
    assert cached.lo.data_ptr() == scene.lo.data_ptr()  # the cache was seeded with the tensors the scene holds
    del problem.__dict__["_scene_cache"]  # ... and without it the lists give the same bits
    rebuilt = problem.scene(DEV)
    assert torch.equal(rebuilt.lo.view(torch.int32), scene.lo.view(torch.int32)) and torch.equal(rebuilt.hi.view(torch.int32), scene.hi.view(torch.int32))
    assert isinstance(rebuilt, ObstacleScene)

    settings = PlannerSettings(k=175, tmax_sec=60.0, anytime_mode_enabled=False, do_rerun_if_large_dp_search_mjac=False,
                               do_rerun_if_optimization_fails=False, verbosity=0)  # fmt: skip

    def plan(p):
        return CppFlowPlanner(settings, p.robot, seed_provider=TrackingSeedProvider(seed=0), device_optimizer=False).generate_plan(p)

    res = plan(problem)
    q_path = res.plan.q_path
    want = rb.scene_env_collisions(q_path.contiguous(), scene.lo, scene.hi, want=("env_mask",))["env_mask"]
    assert torch.equal(res.plan.env_colliding_per_ts.to(torch.bool).reshape(-1), want.reshape(-1))
    touches_cube = base.env_collision_mask(q_path.unsqueeze(0).contiguous())
    print(f"sensed cube: {scene.n_obstacles} cuboids from {scene.stats['occupied_cells']} cells, is_valid={res.plan.is_valid}, "
          f"waypoints touching the original cube: {int(touches_cube.sum())}")
    if res.plan.is_valid:
        assert not bool(touches_cube.any())  # the sensed scene contains the cube's surface
