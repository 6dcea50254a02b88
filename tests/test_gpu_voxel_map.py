"""Scenes fused over frames on the MI355X: cppf_voxel_map_* and cppf_scene_from_map (csrc/kernels_voxel.h) against the NumPy model of
tests/voxel_map.py (asserted on its own in tests/test_voxel_map_model.py) -- one frame against the single-frame entry points byte for
byte, the counters, the threshold, the z-merged list bit for bit, the capacity rule, memory discipline, determinism and graph capture,
and `VoxelMap` up to a plan on a fused scene.

Every raw call here runs on a workspace that was filled with 0xFF just before it: whatever a launch read without writing it first
would show.  Shapes are the smallest at which the kernels still take every path: one word per row, a full word, one bit in a second
word; the integration runs in two workgroups from 100 x 5 x 4 on, the threshold pass and the row kernels in the 65 x 20 x 14 case of
the z-merge."""

import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import voxel_map as M
from tests import voxel_scene as V

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF = os.path.join(GOLDEN, "reference_files")
SENTINEL = 0x77


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


def camera_args(intr, T):
    T = np.asarray(T, dtype=F)
    k = (ctypes.c_float * 4)(*[float(v) for v in intr])
    rt = (ctypes.c_float * 12)(*[float(v) for v in np.concatenate([T[:3, :3].reshape(9), T[:3, 3]])])
    return k, rt


class RawMap:
    """a map, its workspace and its outputs, driven through the C ABI alone"""

    def __init__(self, origin, voxel, dims, n_self=0):
        from cppflow_amd import _hip

        self.lib = _hip.lib()
        self.origin, self.voxel, self.dims = origin, voxel, tuple(int(d) for d in dims)
        self.grid = _hip.VoxelGrid((ctypes.c_float * 3)(*[float(v) for v in origin]), float(voxel), (ctypes.c_int32 * 3)(*self.dims))
        nb = ctypes.c_size_t(0)
        _hip.check(self.lib.cppf_voxel_map_bytes(ctypes.byref(self.grid), ctypes.byref(nb)))
        nx, ny, nz = self.dims
        assert nb.value == 16 + M.padded(nx) * ny * nz
        self.map = torch.full((nb.value,), 0xFF, dtype=torch.uint8, device=DEV)
        _hip.check(self.lib.cppf_voxel_scene_workspace_bytes(ctypes.byref(self.grid), n_self, ctypes.byref(nb)))
        self.work = torch.empty(nb.value, dtype=torch.uint8, device=DEV)
        _hip.check(self.lib.cppf_voxel_scene_workspace_bytes(ctypes.byref(self.grid), 0, ctypes.byref(nb)))
        self.scene_work_bytes = nb.value
        self.counts = torch.empty(8, dtype=torch.int32, device=DEV)
        self.lo = self.hi = None
        self.clear()

    def stream(self, st=None):
        return (st if st is not None else torch.cuda.current_stream(DEV)).cuda_stream

    def poison(self):
        self.work.fill_(0xFF)
        self.counts.fill_(-1)

    def clear(self, st=None):
        from cppflow_amd import _hip

        _hip.check(self.lib.cppf_voxel_map_clear(self.map.data_ptr(), self.map.numel(), ctypes.byref(self.grid), self.stream(st)))

    def _tail(self, rb, q_self, margin, st):
        n_self = 0 if q_self is None else int(q_self.shape[0])
        handle = rb._handle(torch.device(DEV)) if n_self > 0 else None
        return handle, (ctypes.byref(self.grid), q_self.data_ptr() if n_self else None, n_self, float(margin), self.map.data_ptr(),
                        self.map.numel(), self.counts.data_ptr(), self.work.data_ptr(), self.work.numel(), self.stream(st))  # fmt: skip

    def add_points(self, pts, rb=None, q_self=None, margin=0.03, st=None, poison=True):
        from cppflow_amd import _hip

        if poison:
            self.poison()
        handle, tail = self._tail(rb, q_self, margin, st)
        n = int(pts.shape[0])
        _hip.check(self.lib.cppf_voxel_map_add_points(handle, pts.data_ptr() if n else None, n, *tail))

    def add_depth(self, depth, intr, T, z_min, z_max, rb=None, q_self=None, margin=0.03, st=None, poison=True):
        from cppflow_amd import _hip

        if poison:
            self.poison()
        handle, tail = self._tail(rb, q_self, margin, st)
        k, rt = camera_args(intr, T)
        _hip.check(self.lib.cppf_voxel_map_add_depth(handle, depth.data_ptr(), int(depth.shape[0]), int(depth.shape[1]), k, rt,
                                                     float(z_min), float(z_max), *tail))  # fmt: skip

    def launch_scene(self, min_frames, merge, capacity, st=None, poison=True):
        """boxes beyond the written ones keep SENTINEL; the workspace is no larger than the header asks for"""
        from cppflow_amd import _hip

        if poison:
            self.poison()
            self.lo = torch.full((max(capacity, 1) + 4, 3), 0, dtype=torch.float32, device=DEV)
            self.hi = torch.full((max(capacity, 1) + 4, 3), 0, dtype=torch.float32, device=DEV)
            self.lo.view(torch.uint8).fill_(SENTINEL)
            self.hi.view(torch.uint8).fill_(SENTINEL)
        _hip.check(self.lib.cppf_scene_from_map(self.map.data_ptr(), self.map.numel(), ctypes.byref(self.grid), int(min_frames), int(merge),
                                                int(capacity), self.lo.data_ptr(), self.hi.data_ptr(), self.counts.data_ptr(),
                                                self.work.data_ptr(), self.scene_work_bytes, self.stream(st)))  # fmt: skip

    def read_scene(self, capacity):
        torch.cuda.synchronize()
        c = host(self.counts).copy()
        w = int(c[1])
        assert w == min(int(c[0]), capacity), c
        for t in (self.lo, self.hi):  # nothing beyond the written boxes was touched, inside the capacity or beyond it
            assert bool((t[w:].contiguous().view(torch.uint8) == SENTINEL).all())
        return dict(lo=host(self.lo[:w]).copy(), hi=host(self.hi[:w]).copy(), counts=c)

    def scene(self, min_frames=1, merge=M.MERGE_XY, capacity=V.MAX_BOXES):
        self.launch_scene(min_frames, merge, capacity)
        return self.read_scene(capacity)

    def add_counts(self):
        torch.cuda.synchronize()
        return host(self.counts).copy()

    def frames(self):
        return int(host(self.map[:16]).view(np.int32)[0])

    def header(self):
        return host(self.map[:16]).view(np.int32).tolist()

    def counters(self):
        nx, ny, nz = self.dims
        return host(self.map[16:]).reshape(nz, ny, M.padded(nx)).copy()

    def set_counters(self, c):
        """an occupancy or counter array [nz, ny, nx] straight into the map (the padding columns stay 0)"""
        nx, ny, nz = self.dims
        full = np.zeros((nz, ny, M.padded(nx)), dtype=np.uint8)
        full[:, :, :nx] = np.asarray(c).astype(np.uint8)
        self.map[16:] = torch.from_numpy(full.reshape(-1)).to(DEV)


def same_list(got, lo, hi, ctx):
    assert np.array_equal(bits(got["lo"]), bits(lo)) and np.array_equal(bits(got["hi"]), bits(hi)), ctx


# ---- 1. one frame equals the single-frame entry points ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", M.GRIDS)
def test_one_frame_of_points_gives_the_single_frame_scene_byte_for_byte(dims):
    from tests.test_gpu_voxel_scene import run_in_arena

    voxel = V.VOXELS[sum(dims) % 3]
    pts = dev(V.point_recipe(1000, V.ORIGIN, voxel, dims, seed=sum(dims)))
    rb, q = robot("panda"), dev(H.random_configs("panda", 3, seed=2))
    for kw in (dict(), dict(rb=rb, q_self=q, margin=0.05)):
        old = run_in_arena(("points", pts), V.ORIGIN, voxel, dims, V.MAX_BOXES, **kw)
        m = RawMap(V.ORIGIN, voxel, dims, n_self=3)
        m.add_points(pts, **kw)
        added = m.add_counts()
        assert added[0] == added[1] == 0 and added[2] == old["counts"][2] and added[7] == 1, added
        assert np.array_equal(added[3:7], old["counts"][3:7]) and added[3:7].sum() == 1000, (added, old["counts"])
        got = m.scene(1, M.MERGE_XY)
        same_list(got, old["lo"], old["hi"], (dims, bool(kw)))
        assert np.array_equal(got["counts"][:3], old["counts"][:3]) and got["counts"][3] == old["counts"][2], got["counts"]
        assert not got["counts"][4:7].any() and got["counts"][7] == 1


@pytest.mark.parametrize("shape", [(8, 10), (33, 65)])
def test_one_frame_of_depth_gives_the_single_frame_scene_byte_for_byte(shape):
    from tests.test_gpu_voxel_scene import run_in_arena

    depth, intr, T, z_min, z_max, origin, voxel, dims = V.depth_recipe(*shape)
    d = dev(depth)
    old = run_in_arena(("depth", d, intr, T, z_min, z_max), origin, voxel, dims, V.MAX_BOXES)
    assert old["counts"][0] >= 2
    m = RawMap(origin, voxel, dims)
    m.add_depth(d, intr, T, z_min, z_max)
    added = m.add_counts()
    assert np.array_equal(added[3:7], old["counts"][3:7]) and added[2] == old["counts"][2] and added[7] == 1 and not added[:2].any()
    got = m.scene(1, M.MERGE_XY)
    same_list(got, old["lo"], old["hi"], shape)
    assert np.array_equal(got["counts"][:3], old["counts"][:3])


# ---- 2. the counters ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def five_frames(dims):
    """(voxel, the five point clouds, their occupancies, the model's counters after all five)"""
    voxel = V.VOXELS[sum(dims) % 3]
    clouds = [V.point_recipe(300, V.ORIGIN, voxel, dims, seed=40 + s) for s in range(5)]
    occs = [V.occupancy(*V.classify(p, V.ORIGIN, voxel, dims), dims) for p in clouds]
    want = M.empty_map(dims)
    for occ in occs:
        want = M.integrate(want, occ)
    want.setflags(write=False)
    return voxel, clouds, occs, want


@pytest.mark.parametrize("dims", M.GRIDS)
def test_counters_equal_the_model_in_any_order_of_the_frames(dims):
    voxel, clouds, occs, want = five_frames(dims)
    first = None
    for order in ((0, 1, 2, 3, 4), (3, 0, 4, 2, 1), (4, 3, 2, 1, 0)):
        m = RawMap(V.ORIGIN, voxel, dims)
        for k, i in enumerate(order):
            m.add_points(dev(clouds[i]))
            c = m.add_counts()
            assert c[2] == occs[i].sum() and c[7] == k + 1, (order, i, c)
        got = m.counters()
        assert np.array_equal(got, want), (dims, order)
        assert not got[:, :, dims[0] :].any()
        assert m.header() == [5, 0, 0, 0]
        whole = host(m.map).copy()
        assert first is None or np.array_equal(whole, first)
        first = whole
    m.clear()
    torch.cuda.synchronize()
    assert not host(m.map).any()


def test_counters_saturate_at_255_and_frames_go_on_counting():
    dims, voxel = (64, 3, 3), V.VOXELS[1]
    P = V.grid_planes(V.ORIGIN, voxel, dims)
    cells = [(0, 0, 0), (63, 2, 2), (8, 1, 1), (15, 1, 1)]
    pts = dev(np.array([[V.cell_centre(P[0], x), V.cell_centre(P[1], y), V.cell_centre(P[2], z)] for x, y, z in cells], dtype=F))
    m = RawMap(V.ORIGIN, voxel, dims)
    for _ in range(254):
        m.add_points(pts, poison=False)
    want = np.zeros((3, 3, 64), dtype=np.uint8)
    for x, y, z in cells:
        want[z, y, x] = 254
    assert np.array_equal(m.counters(), want)
    other = dev(np.array([[V.cell_centre(P[0], 9), V.cell_centre(P[1], 1), V.cell_centre(P[2], 1)]], dtype=F))
    m.add_points(other)  # a neighbour in the same word of eight, while the others stand at 254 ...
    for _ in range(5):
        m.add_points(pts)  # ... and go to 255 and stay
    want[want == 254] = 255
    want[1, 1, 9] = 1
    assert np.array_equal(m.counters(), want) and m.frames() == 260 and m.add_counts()[7] == 260


# ---- 3. the threshold -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", M.GRIDS)
def test_threshold_gives_the_models_occupancy_and_xy_list(dims):
    voxel, _, _, want = five_frames(dims)
    m = RawMap(V.ORIGIN, voxel, dims)
    m.set_counters(want[:, :, : dims[0]])
    for mf in (1, 2, 3, 5, 6, 255):
        occ = M.threshold(want, mf, dims[0])
        lo, hi = M.boxes(occ, V.ORIGIN, voxel)
        got = m.scene(mf, M.MERGE_XY)
        same_list(got, lo, hi, (dims, mf))
        assert got["counts"].tolist() == [len(lo), len(lo), int(occ.sum()), int((want != 0).sum()), 0, 0, 0, 0], (dims, mf, got["counts"])


def test_threshold_over_the_whole_range_of_a_counter():
    """every counter value against thresholds on both sides of bit 7 -- and a byte in the padding that no bit may come of"""
    dims, voxel = (100, 5, 4), V.VOXELS[0]
    rng = np.random.RandomState(7)
    c = rng.randint(0, 256, size=(4, 5, 100)).astype(np.uint8)
    c[0, 0, :] = np.arange(100) + 78  # 78 .. 177: around 127 / 128 next to one another
    c[1, 1, :64] = np.arange(64) * 4 + 3
    m = RawMap(V.ORIGIN, voxel, dims)
    m.set_counters(c)
    m.map[16 + 101] = 200  # x = 101 >= nx of row 0
    for mf in (1, 2, 127, 128, 129, 200, 254, 255):
        occ = c >= mf
        lo, hi = M.boxes(occ, V.ORIGIN, voxel)
        got = m.scene(mf, M.MERGE_XY, capacity=V.MAX_BOXES)
        assert got["counts"][0] <= V.MAX_BOXES
        same_list(got, lo, hi, mf)
        assert got["counts"][2] == occ.sum() and got["counts"][3] == (c != 0).sum(), (mf, got["counts"])


# ---- 4. the z-merge -------------------------------------------------------------------------------------------------------------------------
CASES = M.zmerge_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_z_merged_list_equals_the_model_bit_for_bit_and_tiles_the_occupancy(name):
    occ, n = CASES[name]
    dims = occ.shape[::-1]
    voxel = V.VOXELS[len(name) % 3]
    lo, hi = M.boxes_xyz(occ, V.ORIGIN, voxel)
    m = RawMap(V.ORIGIN, voxel, dims)
    m.set_counters(occ)
    got = m.scene(1, M.MERGE_XYZ)
    same_list(got, lo, hi, name)
    assert got["counts"].tolist() == [len(lo), len(lo), int(occ.sum()), int(occ.sum()), 0, 0, 0, 0], (name, got["counts"])
    if n is not None:
        assert len(got["lo"]) == n, name
    # the device's own list, rasterised on the host: exactly the occupancy, no cell twice
    cover = M.rasterise(M.cell_ranges(got["lo"], got["hi"], V.ORIGIN, voxel, dims), occ.shape)
    assert np.array_equal(cover, occ.astype(np.int32)), name
    xy = m.scene(1, M.MERGE_XY)
    assert len(got["lo"]) <= len(xy["lo"])
    same_list(xy, *M.boxes(occ, V.ORIGIN, voxel), name)


# ---- 5. the capacity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("merge", [M.MERGE_XY, M.MERGE_XYZ])
def test_a_short_capacity_writes_the_first_boxes_of_the_same_list_and_nothing_else(merge):
    occ, _ = CASES["random 70x6x5 at density 0.5"]
    dims, voxel = occ.shape[::-1], V.VOXELS[1]
    lo, hi = (M.boxes_xyz if merge == M.MERGE_XYZ else M.boxes)(occ, V.ORIGIN, voxel)
    total = len(lo)
    assert total > 300
    m = RawMap(V.ORIGIN, voxel, dims)
    m.set_counters(occ)
    for capacity in (total, total - 1, 257, 3, 0):
        got = m.scene(1, merge, capacity)  # (read_scene: the sentinel behind the written boxes is intact)
        assert got["counts"][0] == total and got["counts"][1] == capacity and got["counts"][2] == occ.sum()
        same_list(got, lo[:capacity], hi[:capacity], (merge, capacity))
    # capacity 0 with NULL boxes: the counts alone
    from cppflow_amd import _hip

    m.poison()
    _hip.check(m.lib.cppf_scene_from_map(m.map.data_ptr(), m.map.numel(), ctypes.byref(m.grid), 1, merge, 0, None, None, m.counts.data_ptr(),
                                         m.work.data_ptr(), m.scene_work_bytes, m.stream()))  # fmt: skip
    assert m.add_counts()[:3].tolist() == [total, 0, int(occ.sum())]


# ---- 6. hygiene -------------------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bytes_and_the_inputs_are_left_alone():
    dims, voxel = (100, 5, 4), V.VOXELS[2]
    rb, q = robot("panda"), dev(H.random_configs("panda", 3, seed=2))
    clouds = [dev(V.point_recipe(1000, V.ORIGIN, voxel, dims, seed=60 + s, pile=500)) for s in range(3)]
    before = [c.clone() for c in clouds]
    runs = []
    for st in (None, torch.cuda.Stream(device=DEV)):
        m = RawMap(V.ORIGIN, voxel, dims, n_self=3)
        if st is not None:
            st.wait_stream(torch.cuda.current_stream(DEV))
        for k, c in enumerate(clouds):
            torch.cuda.synchronize()  # (the poison goes through the current stream: not while a frame on `st` still runs)
            m.poison()
            torch.cuda.synchronize()
            m.add_points(c, rb=rb if k == 1 else None, q_self=q if k == 1 else None, st=st, poison=False)
        torch.cuda.synchronize()
        frozen = host(m.map).copy()
        out = {}
        for merge in (M.MERGE_XY, M.MERGE_XYZ):
            got = m.scene(2, merge)
            out[merge] = (got["lo"], got["hi"], got["counts"])
        assert np.array_equal(host(m.map), frozen)  # cppf_scene_from_map reads the map only
        runs.append((frozen, out))
    assert np.array_equal(runs[0][0], runs[1][0])
    for merge in (M.MERGE_XY, M.MERGE_XYZ):
        for a, b in zip(runs[0][1][merge], runs[1][1][merge]):
            assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert runs[0][1][M.MERGE_XY][2][0] >= 2
    for c, b in zip(clouds, before):
        assert torch.equal(c.view(torch.int32), b.view(torch.int32))


def test_a_frame_without_points_counts_as_a_frame_and_changes_no_counter():
    dims, voxel = (65, 4, 3), V.VOXELS[0]
    m = RawMap(V.ORIGIN, voxel, dims)
    m.add_points(dev(V.point_recipe(300, V.ORIGIN, voxel, dims, seed=1)))
    before = m.counters()
    assert before.any()
    m.add_points(torch.empty((0, 3), dtype=torch.float32, device=DEV))
    assert m.add_counts().tolist() == [0, 0, 0, 0, 0, 0, 0, 2] and np.array_equal(m.counters(), before) and m.header() == [2, 0, 0, 0]
    depth = torch.empty((0, 7), dtype=torch.float32, device=DEV)
    from cppflow_amd import _hip

    m.poison()
    k, rt = camera_args((50.0, 50.0, 3.0, 0.0), np.eye(4))
    _hip.check(m.lib.cppf_voxel_map_add_depth(None, None, 0, 7, k, rt, 0.1, 3.0, ctypes.byref(m.grid), None, 0, 0.0, m.map.data_ptr(),
                                              m.map.numel(), m.counts.data_ptr(), m.work.data_ptr(), m.work.numel(), m.stream()))  # fmt: skip
    assert depth.numel() == 0 and m.add_counts()[7] == 3 and np.array_equal(m.counters(), before)
    got = m.scene(1, M.MERGE_XYZ)
    assert got["counts"][7] == 3 and got["counts"][2] == (before != 0).sum()


def test_graph_capture_of_two_adds_and_a_scene_replays_to_the_same_bytes():
    dims, voxel = (65, 4, 3), V.VOXELS[1]
    rb, q = robot("panda"), dev(H.random_configs("panda", 2, seed=1))
    a = dev(V.point_recipe(1000, V.ORIGIN, voxel, dims, seed=6))
    depth, intr, T, z_min, z_max, origin, dvoxel, ddims = V.depth_recipe(33, 65)
    d = dev(depth)
    for grid, second in (((V.ORIGIN, voxel, dims), "points"), ((origin, dvoxel, ddims), "depth")):
        b = dev(V.point_recipe(1000, *grid, seed=7))

        def calls(m, st, poison):
            m.add_points(b, rb=rb, q_self=q, st=st, poison=poison)
            if second == "points":
                m.add_points(a, st=st, poison=poison)
            else:
                m.add_depth(d, intr, T, z_min, z_max, st=st, poison=poison)
            m.launch_scene(2, M.MERGE_XYZ, 256, st=st, poison=poison)

        ref = RawMap(*grid, n_self=2)
        calls(ref, None, True)
        want = ref.read_scene(256)
        want_map = host(ref.map).copy()
        assert want["counts"][0] >= 1 and want["counts"][7] == 2

        m = RawMap(*grid, n_self=2)
        m.launch_scene(1, M.MERGE_XY, 256)  # (allocates the outputs)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=DEV)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            calls(m, side, False)
            side.synchronize()
            with torch.cuda.graph(g, stream=side):
                calls(m, side, False)
        for _ in range(2):
            m.clear()
            m.poison()
            m.lo.view(torch.uint8).fill_(SENTINEL)
            m.hi.view(torch.uint8).fill_(SENTINEL)
            g.replay()
            got = m.read_scene(256)
            assert np.array_equal(host(m.map), want_map), second
            for nm in ("lo", "hi", "counts"):
                assert np.array_equal(got[nm].view(np.int32), want[nm].view(np.int32)), (second, nm)


# ---- 7. Python, and a plan on a fused scene -------------------------------------------------------------------------------------------------
def test_voxel_map_reaches_every_path_and_never_returns_a_cut_list():
    rb = robot("panda")
    dims, voxel = (100, 5, 4), V.VOXELS[1]
    vm = rb.voxel_map(V.ORIGIN, float(voxel), dims, DEV)
    assert vm.frames == 0 and tuple(vm.counts_tensor().shape) == (4, 5, 128) and not bool(vm.counts_tensor().any())
    assert vm.last_counts()["frames"] == 0
    clouds = [V.point_recipe(600, V.ORIGIN, voxel, dims, seed=80 + s) for s in range(2)]
    depth, intr, T, z_min, z_max, origin, dvoxel, ddims = V.depth_recipe(33, 65)
    q = dev(H.random_configs("panda", 2, seed=3))
    want = M.empty_map(dims)
    for k, p in enumerate(clouds):
        vm.add_points(dev(p), q_self=q if k else None)
        cls, cells = V.classify(p, V.ORIGIN, voxel, dims)
        lc = vm.last_counts()
        if k == 0:
            want = M.integrate(want, V.occupancy(cls, cells, dims))
            assert lc == dict(frame_cells=int(V.occupancy(cls, cells, dims).sum()), kept_points=int((cls == V.KEPT).sum()),
                              outside_points=int((cls == V.OUTSIDE).sum()), invalid_points=int((cls == V.INVALID).sum()), self_points=0,
                              frames=1)  # fmt: skip
        else:
            assert lc["frames"] == 2 and lc["kept_points"] + lc["self_points"] == int((cls == V.KEPT).sum())
    assert vm.frames == 2
    one = rb.voxel_map(V.ORIGIN, float(voxel), dims, DEV)
    one.add_points(dev(clouds[0]))
    assert np.array_equal(host(one.counts_tensor()), want)
    for merge_z, model in ((False, M.boxes), (True, M.boxes_xyz)):
        sc = one.scene(min_frames=1, merge_z=merge_z)
        lo, hi = model(M.threshold(want, 1, dims[0]), V.ORIGIN, voxel)
        assert np.array_equal(bits(host(sc.lo)), bits(lo)) and np.array_equal(bits(host(sc.hi)), bits(hi))
        assert sc.stats["boxes_total"] == sc.n_obstacles == len(lo) and sc.stats["occupied_cells"] == sc.stats["seen_cells"] == (want != 0).sum()
        assert sc.stats["frames"] == 1 and sc.stats["min_frames"] == 1 and sc.stats["merge_z"] is merge_z
        assert sc.stats["dims"] == dims and sc.stats["voxel_m"] == float(voxel) and sc.lo.device == torch.device(DEV)
    total = one.scene().stats["boxes_total"]
    assert total > 3
    with pytest.raises(RuntimeError, match=rf"{total} boxes.*max_cuboids = 3.*occupied cells"):
        one.scene(max_cuboids=3)
    assert one.scene(max_cuboids=total).n_obstacles == total
    assert one.scene(min_frames=2).n_obstacles == 0
    one.clear()
    assert one.frames == 0 and not bool(one.counts_tensor().any()) and one.scene().n_obstacles == 0
    dm = rb.voxel_map(origin, float(dvoxel), ddims, DEV)
    dm.add_depth(dev(depth), intr, T, z_min, z_max)
    dm.add_depth(dev(depth), intr, torch.tensor(T), z_min, z_max, q_self=q[0])
    old = rb.scene_from_depth(dev(depth), intr, T, z_min, z_max, origin, float(dvoxel), ddims)
    flat = dm.scene(min_frames=1, merge_z=False)
    assert dm.frames == 2 and torch.equal(flat.lo.view(torch.int32), old.lo.view(torch.int32)) and torch.equal(flat.hi, old.hi)
    assert dm.last_counts()["frames"] == 2 and dm.scene(min_frames=1).n_obstacles <= flat.n_obstacles


def look_at(eye, target):
    """cam_to_world 4x4: the camera at `eye`, its z axis towards `target`, x to the right, y down"""
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, np.array([0.0, 0.0, 1.0]))
    x /= np.linalg.norm(x)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = x, np.cross(z, x), z, eye
    return T


def render_box(clo, chi, T, intr, shape):
    """the depth image [H, W] (0 where the ray misses) of the axis-aligned box clo .. chi: the slab test per pixel ray, in fp64"""
    fx, fy, cx, cy = (float(v) for v in intr)
    v, u = np.mgrid[0 : shape[0], 0 : shape[1]]
    d = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u, dtype=np.float64)], axis=-1) @ T[:3, :3].T  # (depth = the ray parameter)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (clo - T[:3, 3]) / d, (chi - T[:3, 3]) / d
    near, far = np.minimum(t0, t1).max(axis=-1), np.maximum(t0, t1).min(axis=-1)
    return np.where((near <= far) & (near > 0), near, 0.0).astype(F)


def test_two_views_fused_drop_the_strays_keep_the_cube_and_carry_a_plan():
    from cppflow_amd.data_type_utils import problem_from_filename
    from cppflow_amd.data_types import PlannerSettings
    from cppflow_amd.planners import CppFlowPlanner, TrackingSeedProvider
    from cppflow_amd.scene import problem_with_scene
    from tests.test_gpu_scene import expected

    base = problem_from_filename(None, "panda__1cube_mini", problems_dir=os.path.join(REF, "problems"), paths_dir=os.path.join(REF, "paths"),
                                 device=DEV)  # fmt: skip
    clo, chi = H.box_corners([host(base.obstacles_cuboids[0])], [host(base.obstacles_Tcuboids[0])])
    clo, chi = clo[0], chi[0]
    centre = 0.5 * (clo + chi)
    voxel = 0.05
    origin = tuple(float(v) for v in (clo - 0.263))
    dims = tuple(int(np.ceil((chi[k] - clo[k] + 0.526) / voxel)) for k in range(3))
    rb = base.robot
    vm = rb.voxel_map(origin, voxel, dims, DEV)
    shape, intr = (96, 128), (130.0, 130.0, 63.5, 47.5)
    half = 0.5 * (chi - clo)
    # one stray return per frame, beside the cube and at another place each time
    stray_at = [centre + np.array([0.0, -(half[1] + 0.16), half[2] + 0.12]), centre + np.array([0.05, half[1] + 0.17, -(half[2] + 0.11)])]
    strays = []
    for k, off in enumerate(([1.0, 0.45, 0.55], [0.95, 0.6, 0.5])):  # two nearby views of the same three faces
        T = look_at(centre + np.array(off), centre)
        depth = render_box(clo, chi, T, intr, shape)
        assert 500 < int((depth > 0).sum()) < depth.size - 500
        pc = T[:3, :3].T @ (stray_at[k] - T[:3, 3])  # the stray in the camera's frame -> its pixel and depth
        pix = (int(round(pc[1] / pc[2] * intr[1] + intr[3])), int(round(pc[0] / pc[2] * intr[0] + intr[2])))
        assert 0 <= pix[0] < shape[0] and 0 <= pix[1] < shape[1] and depth[pix] == 0, pix
        depth[pix] = F(pc[2])
        strays.append(V.back_project(depth, intr, T, 0.2, 3.0)[0][pix[0] * shape[1] + pix[1]])
        vm.add_depth(dev(depth), intr, T, 0.2, 3.0)
        lc = vm.last_counts()
        assert lc["frames"] == k + 1 and lc["kept_points"] == int((depth > 0).sum()) and lc["frame_cells"] > 20, lc
    strays = np.asarray(strays, dtype=F)
    seen = vm.scene(min_frames=1)
    scene = vm.scene(min_frames=2)
    flat = vm.scene(min_frames=2, merge_z=False)
    print(f"fused cube: {seen.stats['seen_cells']} cells seen, {scene.stats['occupied_cells']} in both views; "
          f"{flat.n_obstacles} boxes merged along x and y, {scene.n_obstacles} along z as well")
    # the strays are in the one-frame scene, each in one box, and gone from the two-frame scene; the cube's faces stay
    assert bool((V.contained(strays, host(seen.lo), host(seen.hi)).sum(axis=1) == 1).all())
    assert not V.contained(strays, host(scene.lo), host(scene.hi)).any()
    assert seen.stats["seen_cells"] == scene.stats["seen_cells"] >= scene.stats["occupied_cells"] + 2 and scene.stats["occupied_cells"] > 20
    assert 1 <= scene.n_obstacles <= flat.n_obstacles and scene.stats["frames"] == 2
    lo, hi = host(scene.lo).astype(np.float64), host(scene.hi).astype(np.float64)
    assert bool(((hi > clo - voxel) & (lo < chi + voxel)).all())  # every cuboid lies within a voxel of the cube
    for k in range(3):  # ... and the three faces both views saw are covered from end to end
        assert lo[:, k].min() <= clo[k] + voxel and hi[:, k].max() >= chi[k] - voxel
    ranges = M.cell_ranges(host(scene.lo), host(scene.hi), origin, F(voxel), dims)
    assert int(M.rasterise(ranges, dims[::-1]).sum()) == scene.stats["occupied_cells"]

    problem = problem_with_scene(base, scene)
    assert problem.n_obstacles == scene.n_obstacles and problem.robot is rb
    settings = PlannerSettings(k=175, tmax_sec=60.0, anytime_mode_enabled=False, do_rerun_if_large_dp_search_mjac=False,
                               do_rerun_if_optimization_fails=False, verbosity=0)  # fmt: skip
    res = CppFlowPlanner(settings, rb, seed_provider=TrackingSeedProvider(seed=0), device_optimizer=False).generate_plan(problem)
    assert res.plan.is_valid
    q_path = res.plan.q_path.contiguous()
    assert not bool(problem.env_collision_mask(q_path.unsqueeze(0)).any())
    # the scene kernel on the z-merged list against the fp32 oracle, bit for bit: the plan's rows and rows that do collide
    x = np.concatenate([host(q_path).astype(np.float64), H.random_configs("panda", 256, seed=5)], axis=0)
    orc = H.oracle32("panda")
    D = np.stack([orc.env_dists(x, lo[o], hi[o]).min(axis=1) for o in range(lo.shape[0])], axis=1).astype(F)
    mask, min_env, nearest, obs_min = expected(D, np.inf)
    got = problem.scene_collisions(dev(x))
    assert mask.any() and not mask[: q_path.shape[0]].any()
    assert np.array_equal(host(got["env_mask"]).astype(np.uint8), mask) and np.array_equal(bits(host(got["min_env"])), bits(min_env))
    assert np.array_equal(host(got["nearest_obs"]), nearest) and np.array_equal(bits(host(got["obs_min"])), bits(obs_min))
