"""Scenes fused over frames (cppf_voxel_map_*, cppf_scene_from_map): the NumPy restatement of the definitions in
include/cppflow_hip.h ("Scenes fused over frames") for tests/test_voxel_map_model.py (CPU) and tests/test_gpu_voxel_map.py (MI355X).
Grid, planes, classes, occupancy and the x/y box list are those of tests/voxel_scene.py, imported, not restated; nothing here calls
the library.

`boxes_xyz` is written from the header's sentences: B(z) as a Python set per layer, membership by `in`.  It walks no rows and
shares nothing with the kernel's run tests but `heads`, which IS the definition of B(z).
"""

import numpy as np

from tests.voxel_scene import (  # noqa: F401  (re-exported: the tests take the whole model from here)
    F,
    ORIGIN,
    VOXELS,
    boxes,
    classify,
    depth_recipe,
    grid_planes,
    hand_made_occupancies,
    heads,
    occupancy,
    planes,
    point_recipe,
    tiles_exactly,
)

MERGE_XY, MERGE_XYZ = 0, 1
GRIDS = ((1, 1, 1), (64, 3, 3), (65, 4, 3), (100, 5, 4), (70, 6, 5))  # (nx, ny, nz): one word, a full word, one bit in the second, ...


def padded(nx):
    return (nx + 63) // 64 * 64


def empty_map(dims):
    """the counters [nz, ny, nxp] uint8 of a cleared map (the header's `frames` is kept by the caller)"""
    nx, ny, nz = dims
    return np.zeros((nz, ny, padded(nx)), dtype=np.uint8)


def integrate(map_, occ):
    """the counters after one more frame of occupancy occ [nz, ny, nx]: + 1 where occupied, saturating at 255; the rest unchanged"""
    out = map_.copy()
    nx = occ.shape[2]
    view = out[:, :, :nx]
    view[occ] = np.minimum(view[occ].astype(np.int32) + 1, 255).astype(np.uint8)
    return out


def threshold(map_, m, nx=None):
    """occ [nz, ny, nx]: count >= m"""
    nx = map_.shape[2] if nx is None else nx
    return map_[:, :, :nx] >= m


def layer_sets(occ):
    """B(z), z = 0 .. nz - 1: the set of (x0, x1, y, y1) of the layer's boxes"""
    nz = occ.shape[0]
    out = [set() for _ in range(nz)]
    for x0, x1, y, y1, z in heads(occ):
        out[z].add((x0, x1, y, y1))
    return out


def zheads(occ):
    """[(x0, x1, y, y1, z, z1)] ascending by (z, y, x0): the boxes of B(z) that B(z - 1) does not contain, each up to the first layer
    that does not contain it"""
    B = layer_sets(occ)
    nz = occ.shape[0]
    out = []
    for z in range(nz):
        for box in B[z]:
            if z > 0 and box in B[z - 1]:
                continue
            z1 = z + 1
            while z1 < nz and box in B[z1]:
                z1 += 1
            out.append(box + (z, z1))
    return sorted(out, key=lambda b: (b[4], b[2], b[0]))


def boxes_xyz(occ, origin, voxel):
    """(lo [total, 3], hi [total, 3]) f32 of the whole z-merged list"""
    nz, ny, nx = occ.shape
    P = grid_planes(origin, voxel, (nx, ny, nz))
    h = np.asarray(zheads(occ), dtype=np.int64).reshape(-1, 6)
    lo = np.stack([P[0][h[:, 0]], P[1][h[:, 2]], P[2][h[:, 4]]], axis=1).astype(F)
    hi = np.stack([P[0][h[:, 1]], P[1][h[:, 3]], P[2][h[:, 5]]], axis=1).astype(F)
    return lo, hi


def rasterise(cuboids, shape):
    """how often each cell [nz, ny, nx] is covered by the cell ranges (x0, x1, y, y1, z, z1)"""
    cover = np.zeros(shape, dtype=np.int32)
    for x0, x1, y, y1, z, z1 in cuboids:
        assert x0 < x1 and y < y1 and z < z1
        cover[z:z1, y:y1, x0:x1] += 1
    return cover


def cell_ranges(lo, hi, origin, voxel, dims):
    """a box list in metres back to cell ranges [(x0, x1, y, y1, z, z1)]: every corner must BE a plane, bit for bit"""
    P = grid_planes(origin, voxel, dims)
    idx = []
    for k in range(3):
        a, b = np.searchsorted(P[k], lo[:, k]), np.searchsorted(P[k], hi[:, k])
        assert bool((b <= dims[k]).all())
        assert np.array_equal(P[k][a].view(np.int32), lo[:, k].view(np.int32)) and np.array_equal(P[k][b].view(np.int32), hi[:, k].view(np.int32))
        idx += [a, b]
    return [tuple(int(c[i]) for c in idx) for i in range(lo.shape[0])]


# ---- occupancies for the z-merge ----------------------------------------------------------------------------------------------------------
def stacked(occ2d, nz):
    """a one-layer occupancy [1, ny, nx] repeated over nz layers"""
    return np.repeat(occ2d[:1], nz, axis=0)


def zmerge_cases():
    """name -> (occ [nz, ny, nx], number of z-merged boxes or None)"""
    out = {}
    for name, (occ, n) in hand_made_occupancies().items():
        if occ.shape[0] == 1:
            out[f"{name}, stacked over 3 layers"] = (stacked(occ, 3), n)
        out[name] = (occ, None)
    for nx, ny, nz in GRIDS:
        out[f"full {nx}x{ny}x{nz}"] = (np.ones((nz, ny, nx), dtype=bool), 1)
        out[f"empty {nx}x{ny}x{nz}"] = (np.zeros((nz, ny, nx), dtype=bool), 0)
    zz, yy, xx = np.meshgrid(np.arange(3), np.arange(4), np.arange(65), indexing="ij")
    board = (xx + yy + zz) % 2 == 0
    out["3-D checkerboard 65x4x3"] = (board, int(board.sum()))
    for nx in (65, 100):
        wall = np.zeros((4, 3, nx), dtype=bool)
        wall[:, 1, :] = True
        out[f"wall {nx}x1x4"] = (wall, 1)
        end = np.zeros((3, 3, nx), dtype=bool)
        end[:, 0:2, nx - 7 : nx] = True
        end[1, 2, nx - 7 : nx] = True  # (the middle layer's box reaches one row further: three cuboids)
        out[f"a run ending at nx - 1 = {nx - 1}"] = (end, 3)
    pair = np.zeros((4, 5, 70), dtype=bool)
    pair[:, 0:2, 3:40] = True
    pair[:, 3:5, 60:70] = True
    pair[2, 1, 20] = False  # one cell of one slab missing in one layer
    out["a slab pair differing in one cell in one layer"] = (pair, None)
    stair = np.zeros((5, 6, 70), dtype=bool)
    for z in range(5):
        stair[z, 1:4, 2 + 3 * z : 30 + 3 * z] = True
    out["a staircase in z"] = (stair, 5)
    y1s = np.zeros((3, 6, 70), dtype=bool)
    y1s[0, 1:3, 10:20] = True  # the same head row and run in every layer, but the slab ends at another row in the middle one
    y1s[1, 1:5, 10:20] = True
    y1s[2, 1:3, 10:20] = True
    out["y1 differs between layers, head row the same"] = (y1s, 3)
    for seed, density in enumerate((0.1, 0.5, 0.9)):
        rng = np.random.RandomState(100 + seed)
        occ = rng.uniform(size=(5, 6, 70)) < density
        # correlated along y and z, so that runs and boxes do repeat
        occ[:, 1:, :] = np.where(rng.uniform(size=occ[:, 1:, :].shape) < 0.6, occ[:, :-1, :], occ[:, 1:, :])
        occ[1:] = np.where(rng.uniform(size=occ[1:].shape[:2])[:, :, None] < 0.6, occ[:-1], occ[1:])
        out[f"random 70x6x5 at density {density}"] = (occ, None)
    # 280 rows and 560 bitset words: more than one workgroup of the row kernels and of the threshold pass
    rng = np.random.RandomState(103)
    occ = rng.uniform(size=(14, 20, 65)) < 0.3
    occ[:, 1:, :] = np.where(rng.uniform(size=occ[:, 1:, :].shape) < 0.7, occ[:, :-1, :], occ[:, 1:, :])
    occ[1:] = np.where(rng.uniform(size=occ[1:].shape[:2])[:, :, None] < 0.7, occ[:-1], occ[1:])
    out["random 65x20x14 at density 0.3"] = (occ, None)
    return out
