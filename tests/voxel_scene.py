"""Scenes from sensor data (cppf_scene_from_points / cppf_scene_from_depth): the NumPy float32 restatement of the definitions in
include/cppflow_hip.h ("Scenes from sensor data") and the input recipes of tests/test_voxel_scene_model.py (CPU) and
tests/test_gpu_voxel_scene.py (MI355X).  Every float32 operation below is a NumPy float32 array operation, i.e. rounded once, in the
order the header states; nothing here calls the library.

Recipe (`point_recipe`): the first n points of a pool that deals its categories round-robin, so that every prefix is mixed --
  lines     cell centres of x-runs: one ending at x = nx - 1 at (y0, z0), the identical run at y0 + 1 (merges), the run shifted by
            one cell at y0 + 2 (does not), one crossing x = 64 in the last row where nx > 64, one down the whole column y = 0 .. ny - 1;
  planes    points exactly on planes: (P_x(i), P_y(j), P_z(k)) belongs to cell (i, j, k); a coordinate on P(n) and one fp32 neighbour
            below P(0) are outside;
  bad       NaN, +inf, -inf in one coordinate;
  uniform   uniform over the grid's box grown by two voxels each way (inside and outside);
  pile      (with pile > 0) that many points inside ONE cell.
"""

import numpy as np

F = np.float32
INVALID, OUTSIDE, SELF, KEPT = 0, 1, 2, 3
MAX_BOXES = 4096


def planes(origin_k, voxel, n):
    """P(i) = fadd(origin, fmul((float)i, voxel)), i = 0 .. n"""
    i = np.arange(n + 1, dtype=F)
    return (F(origin_k) + (i * F(voxel)).astype(F)).astype(F)


def grid_planes(origin, voxel, dims):
    return [planes(origin[k], voxel, dims[k]) for k in range(3)]


def cell_index(P, p):
    """the unique i in [0, n) with P(i) <= p < P(i+1), else -1 (p finite; P strictly increasing)"""
    i = np.searchsorted(P, p, side="right") - 1
    return np.where((i >= 0) & (i < len(P) - 1), i, -1)


def classify(points, origin, voxel, dims, is_self=None, invalid=None):
    """points f32 [n, 3] -> (classes [n], cells [n, 3] (x, y, z; -1 where not inside)).  `invalid`: the depth form's invalid pixels;
    `is_self`: the self filter's verdict per point (only asked of points inside the grid)."""
    points = np.asarray(points, dtype=F).reshape(-1, 3)
    n = points.shape[0]
    bad = ~np.isfinite(points).all(axis=1)
    if invalid is not None:
        bad |= np.asarray(invalid, dtype=bool)
    P = grid_planes(origin, voxel, dims)
    safe = np.where(np.isfinite(points), points, F(0))
    cells = np.stack([cell_index(P[k], safe[:, k]) for k in range(3)], axis=1)
    inside = (cells >= 0).all(axis=1) & ~bad
    cls = np.full(n, OUTSIDE, dtype=np.int32)
    cls[bad] = INVALID
    slf = inside & (np.asarray(is_self, dtype=bool) if is_self is not None else False)
    cls[slf] = SELF
    cls[inside & ~slf] = KEPT
    cells = np.where((cls == KEPT)[:, None] | (cls == SELF)[:, None], cells, -1)
    return cls, cells


def occupancy(cls, cells, dims):
    occ = np.zeros((dims[2], dims[1], dims[0]), dtype=bool)
    k = cells[cls == KEPT]
    occ[k[:, 2], k[:, 1], k[:, 0]] = True
    return occ


def row_runs(row):
    """the maximal intervals [x0, x1) of True"""
    d = np.diff(np.concatenate([[0], row.astype(np.int8), [0]]))
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def heads(occ):
    """[(x0, x1, y, y1, z)] ascending by (z, y, x0): a run is a head if row y - 1 does not hold the identical maximal run; its box
    spans y .. y1, the first row below that does not hold it"""
    nz, ny, _ = occ.shape
    out = []
    for z in range(nz):
        runs = [row_runs(occ[z, y]) for y in range(ny)]
        sets = [set(r) for r in runs]
        for y in range(ny):
            for run in runs[y]:
                if y > 0 and run in sets[y - 1]:
                    continue
                y1 = y + 1
                while y1 < ny and run in sets[y1]:
                    y1 += 1
                out.append((run[0], run[1], y, y1, z))
    return out


def boxes(occ, origin, voxel):
    """(lo [total, 3], hi [total, 3]) f32 of the whole list"""
    nz, ny, nx = occ.shape
    P = grid_planes(origin, voxel, (nx, ny, nz))
    h = np.asarray(heads(occ), dtype=np.int64).reshape(-1, 5)
    lo = np.stack([P[0][h[:, 0]], P[1][h[:, 2]], P[2][h[:, 4]]], axis=1).astype(F)
    hi = np.stack([P[0][h[:, 1]], P[1][h[:, 3]], P[2][h[:, 4] + 1]], axis=1).astype(F)
    return lo, hi


def counts(cls, occ, total, capacity):
    return np.array([total, min(total, capacity), int(occ.sum()), int((cls == KEPT).sum()), int((cls == OUTSIDE).sum()),
                     int((cls == INVALID).sum()), int((cls == SELF).sum()), 0], dtype=np.int32)  # fmt: skip


def scene_from_points(points, origin, voxel, dims, capacity=MAX_BOXES, is_self=None, invalid=None):
    """the whole definition -> dict(lo, hi (the FULL list), written, counts, classes, cells, occ)"""
    cls, cells = classify(points, origin, voxel, dims, is_self, invalid)
    occ = occupancy(cls, cells, dims)
    lo, hi = boxes(occ, origin, voxel)
    return dict(lo=lo, hi=hi, written=min(len(lo), capacity), counts=counts(cls, occ, len(lo), capacity), classes=cls, cells=cells, occ=occ)


def back_project(depth, intrinsics, cam_to_world, z_min, z_max):
    """depth f32 [H, W] -> (points f32 [H W, 3] (0 where invalid), invalid [H W]); every operation rounded separately, in the header's order"""
    depth = np.asarray(depth, dtype=F)
    H, W = depth.shape
    fx, fy, cx, cy = (F(v) for v in intrinsics)
    ifx, ify = F(1.0) / fx, F(1.0) / fy
    T = np.asarray(cam_to_world, dtype=F)
    R, t = T[:3, :3], T[:3, 3]
    z = depth.reshape(-1)
    with np.errstate(invalid="ignore"):
        valid = (z > F(z_min)) & (z < F(z_max))
    zz = np.where(valid, z, F(1)).astype(F)
    u = np.tile(np.arange(W, dtype=F), H)
    v = np.repeat(np.arange(H, dtype=F), W)
    with np.errstate(over="ignore", invalid="ignore"):
        xc = ((u - cx).astype(F) * (zz * ifx).astype(F)).astype(F)
        yc = ((v - cy).astype(F) * (zz * ify).astype(F)).astype(F)
        w = [((((R[k, 0] * xc).astype(F) + (R[k, 1] * yc).astype(F)).astype(F) + (R[k, 2] * zz).astype(F)).astype(F) + t[k]).astype(F)
             for k in range(3)]  # fmt: skip
    pts = np.where(valid[:, None], np.stack(w, axis=1), F(0)).astype(F)
    return pts, ~valid


def contained(points, lo, hi):
    """[n, n_boxes] bool: lo <= p < hi on every axis"""
    p = np.asarray(points, dtype=F)[:, None, :]
    return ((p >= lo[None]) & (p < hi[None])).all(axis=2)


# ---- recipes --------------------------------------------------------------------------------------------------------------------------
ORIGIN = (F(-0.4137), F(0.2871), F(0.0613))  # not a lattice point of any voxel size used
VOXELS = (F(2.0**-5), F(0.02), F(0.05))


def cell_centre(P, i):
    return (P[i] + (P[i + 1] - P[i]) * F(0.5)).astype(F)


def point_recipe(n, origin, voxel, dims, seed=0, pile=0):
    """f32 [n, 3]; see the module docstring"""
    nx, ny, nz = dims
    rng = np.random.RandomState(seed)
    P = grid_planes(origin, voxel, dims)

    def centre(ix, iy, iz):
        return [cell_centre(P[0], ix), cell_centre(P[1], iy), cell_centre(P[2], iz)]

    lines = []
    y0, z0 = 0, 0
    for x in range(max(0, nx - 12), nx):
        lines.append(centre(x, y0, z0))
        if ny > 1:
            lines.append(centre(x, y0 + 1, z0))
    if ny > 2:
        for x in range(max(0, nx - 13), max(1, nx - 1)):
            lines.append(centre(x, y0 + 2, z0))
    if nx > 64:
        for x in range(58, min(nx, 70)):
            lines.append(centre(x, ny - 1, nz - 1))
    xc = min(3, nx - 1)
    for y in range(ny):
        lines.append(centre(xc, y, nz // 2))
    on = []
    for _ in range(24):
        i, j, k = rng.randint(0, nx), rng.randint(0, ny), rng.randint(0, nz)
        on.append([P[0][i], P[1][j], P[2][k]])
    on.append([P[0][nx], cell_centre(P[1], 0), cell_centre(P[2], 0)])
    on.append([cell_centre(P[0], 0), P[1][ny], cell_centre(P[2], 0)])
    on.append([cell_centre(P[0], 0), cell_centre(P[1], 0), P[2][nz]])
    on.append([np.nextafter(P[0][0], F(-np.inf)), cell_centre(P[1], 0), cell_centre(P[2], 0)])
    on.append([cell_centre(P[0], 0), cell_centre(P[1], 0), np.nextafter(P[2][0], F(-np.inf))])
    bad = []
    for k, val in enumerate((np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf)):
        p = centre(0, 0, 0)
        p[k % 3] = F(val)
        bad.append(p)
    lo = np.array([P[k][0] for k in range(3)], dtype=np.float64) - 2 * float(voxel)
    hi = np.array([P[k][-1] for k in range(3)], dtype=np.float64) + 2 * float(voxel)
    uniform = rng.uniform(lo, hi, size=(max(n, 8), 3)).astype(F).tolist()
    cats = [lines, on, bad, uniform]
    pool, idx = [], [0, 0, 0, 0]
    while len(pool) < n:
        for c, cat in enumerate(cats):
            j = idx[c]
            idx[c] += 1
            pool.append(cat[j % len(cat)] if c != 3 else cat[min(j, len(cat) - 1)])
    pts = np.asarray(pool[:n], dtype=F).reshape(-1, 3)
    if pile > 0:
        c = np.asarray(centre(nx // 2, ny // 2, nz // 2), dtype=np.float64)
        heap = (c + rng.uniform(-0.4, 0.4, size=(pile, 3)) * float(voxel)).astype(F)
        pts = np.concatenate([pts, heap], axis=0)
    return np.ascontiguousarray(pts, dtype=F)


def depth_recipe(H, W, seed=0):
    """(depth f32 [H, W] with NaN, 0, negative, too-far and +inf pixels, intrinsics, cam_to_world 4x4 f32 (rotated about all three axes),
    z_min, z_max, grid origin, voxel, dims): a camera 1.2 m in front of a slanted wall that the grid covers in part"""
    rng = np.random.RandomState(seed)
    v, u = np.mgrid[0:H, 0:W]
    depth = (0.8 + 0.3 * u / max(W - 1, 1) + 0.15 * v / max(H - 1, 1) + 0.01 * rng.randn(H, W)).astype(F)
    flat = depth.reshape(-1)
    for j, val in zip(rng.choice(H * W, size=min(10, H * W), replace=False), (np.nan, 0.0, -1.0, 5.0, np.inf, -np.inf, 0.1, 3.0, np.nan, 2.9)):
        flat[j] = F(val)
    fx = fy = F(0.9 * W)
    intr = (fx, fy, F(W / 2 - 0.5), F(H / 2 - 0.25))
    a, b, c = 0.3, -0.5, 0.2
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = (0.3, -0.2, 0.5)
    T = T.astype(F)
    z_min, z_max = F(0.25), F(2.5)
    pts, invalid = back_project(depth, intr, T, z_min, z_max)
    good = pts[~invalid].astype(np.float64)
    voxel = F(0.05)
    origin = tuple(F(x) for x in (good.min(axis=0) + 0.013))  # (cuts a few points off: outside)
    dims = tuple(int(x) for x in np.maximum(1, np.ceil((good.max(axis=0) - good.min(axis=0)) * 0.8 / float(voxel))))
    return depth, intr, T, z_min, z_max, origin, voxel, dims


def hand_made_occupancies():
    """name -> (occ [nz, ny, nx], number of boxes)"""
    out = {}
    out["full 64x8x1 slab"] = (np.ones((1, 8, 64), dtype=bool), 1)
    two = np.zeros((1, 3, 10), dtype=bool)
    two[0, 0:2, 2:7] = True
    out["two identical runs stacked"] = (two, 1)
    sh = np.zeros((1, 3, 10), dtype=bool)
    sh[0, 0, 2:7] = True
    sh[0, 1, 3:8] = True
    out["runs shifted by one cell"] = (sh, 2)
    ch = np.zeros((2, 5, 70), dtype=bool)
    ch[1, 1:5, 60:68] = True
    out["a chain reaching y = ny - 1"] = (ch, 1)
    br = np.zeros((1, 4, 12), dtype=bool)
    br[0, 0, 1:9] = True  # one long run over ...
    br[0, 1, 1:4] = True  # ... two shorter ones ...
    br[0, 1, 5:9] = True
    br[0, 2, 1:9] = True  # ... and the long one again: a new head
    out["a run that splits and re-forms"] = (br, 4)
    return out


def tiles_exactly(occ):
    """the heads' boxes as cell ranges: their union is occ, no cell is covered twice, the order ascends"""
    cover = np.zeros(occ.shape, dtype=np.int32)
    hs = heads(occ)
    for x0, x1, y, y1, z in hs:
        assert x0 < x1 and y < y1
        cover[z, y:y1, x0:x1] += 1
    keys = [(z, y, x0) for x0, _, y, _, z in hs]
    return bool((cover == occ.astype(np.int32)).all()) and keys == sorted(keys) and len(set(keys)) == len(keys)
