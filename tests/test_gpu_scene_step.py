"""The coupled LM step on a whole obstacle scene (cppf_lm_full_step_scene, the scene form of full_blocks_kernel) on the MI355X: bit
for bit against the existing step on a handle that holds the penetrating cuboids, and the planner with `scene_optimizer=True`.

Rows.  Per robot a pool of 9 trajectories x 59 waypoints: trajectory s is its own random walk (0.03 rad per step) from its own start
inside the joint limits plus 0.003 rad of noise per waypoint, so pose errors against the target (FK of trajectory 0's walk) and joint
changes are non-trivial and different trajectories reach into different parts of the workspace.  A case (S, W) is the first W
waypoints of the first S trajectories: W in {25, 59} x S in {1, 3, 9} gives 25 .. 531 rows, every last wavefront partly filled (75,
177 rows ...), trajectories sharing wavefronts.  Parameters: ALT_LOSS_V2_1_DIFF with virtual_configs = x.

Elimination forms at these sizes (full_step_form): up to 8 joints every case is the parallel-in-time form with the state in LDS
(Panda, Fetch, the generic 7-joint chain: blocks without the folded terms); chain12 (12 joints) is the row-per-lane form, sixteen lanes
per trajectory (blocks WITH the folded differencing / virtual-config / lambda terms).  Both block layouts are therefore covered.

Cuboids.  Candidates per robot, numpy.default_rng(5): "near" -- 40 per trajectory, centred on a point of a capsule axis of one of the
trajectory's first 25 waypoints, pushed 0 .. 0.2 m in a random direction, half-sizes 0.02 .. 0.06 m; "big" -- 12 with half-sizes 0.12 ..
0.22 m pushed 0 .. 0.1 m; "far" -- 100 at 1 .. 2 m beyond the furthest capsule point of the pool.  Every (row, cuboid) pair is
classified ONCE on the CPU by oracle32.masks for that cuboid alone (env_mask: penetrates or not; min_env: how far), and every test
builds its scenes from that classification and asserts what it relies on before it compares anything."""

import ctypes
import dataclasses
import functools
import os

import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROBOTS = ("panda", "fetch", "generic7", "chain12")
S_MAX, W_MAX = 9, 59
N_NEAR = 40 * S_MAX  # candidates 0 .. N_NEAR-1: the small cuboids next to the capsules (then 12 big ones, then 100 far ones)
SHAPES = [(1, 25), (3, 25), (9, 25), (1, 59), (3, 59), (9, 59)]
PINS = (0, 3)  # 0, CPPF_PIN_FIRST | CPPF_PIN_LAST
SENTINEL = 0x7FC0BEEF
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF = os.path.join(GOLDEN, "reference_files")


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def bits(t):
    return t.contiguous().view(torch.int32)


def _params(**kw):
    from cppflow_amd.lm_hyper_parameters import ALT_LOSS_V2_1_DIFF, OptimizationParameters

    d = dict(ALT_LOSS_V2_1_DIFF.__dict__)
    d.update(kw)
    pm = OptimizationParameters(**d)
    pm.virtual_configs = torch.tensor([])
    return pm


@functools.lru_cache(maxsize=None)
def setup(name):
    """(Robot, canonical chain, fp32 oracle, fp64 oracle).  generic7: a description that matches no generated table and is not
    specialised at run time -- the description travels in the argument segment, the capsules are staged in LDS."""
    from cppflow_amd.robot_model import canonicalize
    from cppflow_amd.robot_zoo import ROBOT_SPECS
    from cppflow_amd.robots import Robot
    from oracle.oracle import Oracle

    if name == "generic7":
        spec = H.random_chain_spec(7, seed=21)
        rb = Robot(spec, specialize=False)
        assert rb.specialization() == -1
    else:
        spec = ROBOT_SPECS[name]()
        rb = Robot(spec)
        assert rb.specialization() >= 0  # a generated table
    ch = canonicalize(spec)
    return rb, ch, Oracle(ch, f32=True, threads=8), Oracle(ch, f32=False, threads=8)


@dataclasses.dataclass
class Pool:
    x: np.ndarray  # [S_MAX, W_MAX, d] fp32-representable
    target: np.ndarray  # [W_MAX, 7]
    obs: list  # (cuboid, Tcuboid) per candidate
    lo: np.ndarray  # [N, 3] f32 world-frame corners, as the library forms them
    hi: np.ndarray
    pen: np.ndarray  # [S_MAX, W_MAX, N] bool: the row penetrates the candidate (oracle32.masks, that cuboid alone)
    dist: np.ndarray  # [S_MAX, W_MAX, N] min over capsules of the signed distance
    # ... and some penetrating capsule's closest points are apart, so that the pair has a direction and its row is not zero: a capsule
    # whose AXIS crosses the cuboid penetrates with a zero gradient (kTouch) and leaves no trace in the step
    live: np.ndarray


@functools.lru_cache(maxsize=None)
def pool(name):
    _, ch, o32, o64 = setup(name)
    d = ch.ndof
    rng = np.random.RandomState(40 + len(name))
    mid, half = 0.5 * (ch.lo + ch.hi), 0.5 * (ch.hi - ch.lo)
    base = np.stack([np.clip(mid + 0.5 * half * rng.uniform(-1, 1, d) + np.cumsum(0.03 * rng.randn(W_MAX, d), axis=0), ch.lo + 0.05, ch.hi - 0.05)
                     for _ in range(S_MAX)])  # fmt: skip
    x = H.f32(np.clip(base + 0.003 * rng.randn(S_MAX, W_MAX, d), ch.lo, ch.hi))
    target = H.f32(o64.fk(H.f32(base[0])))
    rows = x.reshape(-1, d)
    ends = o32.capsule_endpoints(rows).reshape(S_MAX, W_MAX, -1, 6)
    L = ends.shape[2]
    g = np.random.default_rng(5)
    obs = []

    def near(s, push, half_lo, half_hi):
        e = ends[s, g.integers(0, 25), g.integers(0, L)]
        p = e[:3] + g.uniform() * (e[3:] - e[:3])
        v = g.normal(size=3)
        p = p + g.uniform(0, push) * v / np.linalg.norm(v)
        return H.cuboid_obstacle(*p, *(2 * g.uniform(half_lo, half_hi, 3)))

    for s in range(S_MAX):
        obs += [near(s, 0.2, 0.02, 0.06) for _ in range(40)]
    assert len(obs) == N_NEAR
    obs += [near(int(g.integers(0, S_MAX)), 0.1, 0.12, 0.22) for _ in range(12)]
    r_far = float(np.linalg.norm(ends.reshape(-1, 3), axis=1).max())
    for _ in range(100):
        r, a = r_far + g.uniform(1.0, 2.0), g.uniform(0, 2 * np.pi)
        obs.append(H.cuboid_obstacle(r * np.cos(a), r * np.sin(a), g.uniform(0, 1.3), *(2 * g.uniform(0.02, 0.06, 3))))
    lo, hi = H.box_corners([c for c, _ in obs], [T for _, T in obs])
    N = len(obs)
    pen, dist = np.zeros((rows.shape[0], N), dtype=bool), np.zeros((rows.shape[0], N))
    live = np.zeros_like(pen)
    for o in range(N):
        m = o32.masks(rows, lo[o : o + 1], hi[o : o + 1], None, None)
        pen[:, o], dist[:, o] = m["env_mask"] > 0, m["min_env"]
        if pen[:, o].any():
            dc, gc = o32.env_dists_grads(rows, lo[o], hi[o])
            live[:, o] = ((dc < 0) & (np.abs(gc).max(axis=2) > 0)).any(axis=1)
    assert np.array_equal(pen, dist < 0) and not (live & ~pen).any()
    shape = (S_MAX, W_MAX, N)
    return Pool(x, target, obs, lo.astype(np.float32), hi.astype(np.float32), pen.reshape(shape), dist.reshape(shape), live.reshape(shape))


@dataclasses.dataclass
class Case:
    name: str
    S: int
    W: int
    xd: torch.Tensor
    td: torch.Tensor
    pen: np.ndarray  # [S, W, N]
    dist: np.ndarray
    live: np.ndarray

    @property
    def hits(self):  # rows of the case each candidate penetrates
        return self.pen.reshape(-1, self.pen.shape[2]).sum(axis=0)

    @property
    def live_hits(self):  # ... with a non-zero row
        return self.live.reshape(-1, self.live.shape[2]).sum(axis=0)


def case(name, S, W, trajs=None):
    """the first W waypoints of the first S trajectories of the pool (or of the trajectories `trajs`)"""
    p = pool(name)
    t = list(range(S)) if trajs is None else list(trajs)
    assert len(t) == S
    x = np.ascontiguousarray(p.x[t, :W]).reshape(S * W, -1)
    return Case(name, S, W, dev(x), dev(p.target[:W]), p.pen[t, :W], p.dist[t, :W], p.live[t, :W])


def scene_of(name, idx):
    p = pool(name)
    idx = np.asarray(idx, dtype=np.int64)
    return dev(p.lo[idx].reshape(-1, 3)), dev(p.hi[idx].reshape(-1, 3))


def bind(name, idx):
    rb, p = setup(name)[0], pool(name)
    rb.set_obstacles([p.obs[i][0] for i in idx], [p.obs[i][1] for i in idx])


def step(c, pin, scene=None, pm=None):
    rb = setup(c.name)[0]
    out = rb.lm_full_step(c.xd, c.td, pm if pm is not None else _params(), virtual_configs=c.xd, pin=pin, scene=scene)
    torch.cuda.synchronize()
    return out.view(c.S, c.W, -1)


def free_step(c, pin):
    """the step with no obstacles at all"""
    bind(c.name, [])
    return step(c, pin)


def assert_the_obstacles_matter(c, idx, got, free):
    """the preconditions every comparison stands on: at least 10 % of the rows penetrate something of `idx`, and on every
    trajectory that penetrates something (with a non-zero row, see Pool.live) the step differs from the step without obstacles"""
    idx = np.asarray(idx, dtype=np.int64)
    row_hits = c.pen[:, :, idx].any(axis=2)
    assert row_hits.mean() >= 0.10, (c.name, c.S, c.W, float(row_hits.mean()))
    live = c.live[:, :, idx].any(axis=2).any(axis=1)
    assert live.any()
    for s in np.flatnonzero(live):
        assert not torch.equal(bits(got[s]), bits(free[s])), (c.name, c.S, c.W, int(s), "the obstacles leave no trace in the step")


def top_hitters(c, k, among=None):
    """the k candidates that penetrate the most rows of the case with a non-zero row (each at least one), most first"""
    h = c.live_hits.copy()
    if among is not None:
        keep = np.zeros_like(h, dtype=bool)
        keep[among] = True
        h[~keep] = 0
    order = np.argsort(-h, kind="stable")[:k]
    assert len(order) == k and (h[order] > 0).all(), (c.name, c.S, c.W, k, h[order])
    return [int(i) for i in order]


# ---- 1. same cuboids, same bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("O", [1, 8])
@pytest.mark.parametrize("S,W", SHAPES)
@pytest.mark.parametrize("name", ROBOTS)
def test_a_scene_equal_to_the_handles_cuboids_gives_the_same_bits(name, S, W, O):
    c = case(name, S, W)
    # O = 1: the candidate that penetrates the most rows; O = 8: the eight SMALL ones that penetrate the most
    idx = top_hitters(c, O, among=None if O == 1 else np.arange(N_NEAR))
    lo, hi = scene_of(name, idx)
    try:
        for pin in PINS:
            free = free_step(c, pin)
            bind(name, idx)
            want = step(c, pin)
            got = step(c, pin, scene=(lo, hi))
            assert_the_obstacles_matter(c, idx, want, free)
            assert torch.equal(bits(got), bits(want)), (name, S, W, O, pin)
    finally:
        bind(name, [])


# ---- 2. clutter changes nothing ----------------------------------------------------------------------------------------------------------
def cluttered(c, O, where):
    """(scene indices [O], positions of the penetrating ones): 8 candidates that penetrate (5 in a scene of 9), every other one penetrates no row of
    the case and is taken evenly from the whole range of distances, nearest first.  `where`: "spread" (evenly through the scene; at
    O = 65 one of them at index 64, the second tile) or "last" (the penetrating cuboids are the last ones)"""
    P = 8 if O >= 64 else 5
    hot = top_hitters(c, P)
    dmin = c.dist.reshape(-1, c.dist.shape[2]).min(axis=0)
    cold = np.flatnonzero(c.hits == 0)
    cold = cold[np.argsort(dmin[cold], kind="stable")]
    assert len(cold) >= O - P
    take = cold[np.unique(np.round(np.linspace(0, len(cold) - 1, O - P)).astype(int))]
    assert len(take) == O - P
    order = np.random.RandomState(O).permutation(take)  # (near and far cuboids mixed within every tile)
    if where == "last":
        pos = list(range(O - P, O))
    else:
        pos = sorted(set(np.round(np.linspace(0, O - 1, P)).astype(int).tolist()))
        assert len(pos) == P and (O != 65 or 64 in pos)
    idx, cold_it, hot_it = [], iter(order), iter(sorted(hot))
    for i in range(O):
        idx.append(next(hot_it) if i in pos else int(next(cold_it)))
    # what the scene is designed to hold
    d_cold = dmin[take]
    assert (d_cold > 0).all()
    assert (d_cold < 0.01).any(), (c.name, "no cuboid just outside a capsule", float(d_cold.min()))  # survives the tile and the capsule cull
    assert ((d_cold > 0.05) & (d_cold < 0.5)).any() or O < 64  # within the wavefront's box, beyond a capsule's own reach
    assert (d_cold > 0.9).any()  # beyond reach (1 m and more past the furthest capsule point): culled with its tile lane
    return idx, pos


@pytest.mark.parametrize("O,where", [(9, "spread"), (64, "spread"), (65, "spread"), (200, "spread"), (200, "last")])
@pytest.mark.parametrize("name", ROBOTS)
def test_clutter_that_penetrates_nothing_changes_no_bit(name, O, where):
    c = case(name, 3, 59)
    idx, pos = cluttered(c, O, where)
    hot = [idx[i] for i in pos]  # ascending scene index
    pen_rows = c.pen[:, :, np.asarray(idx)]
    assert set(np.flatnonzero(pen_rows.any(axis=(0, 1))).tolist()) == set(pos)  # the penetrating set is exactly as designed
    lo, hi = scene_of(name, idx)
    try:
        for pin in PINS:
            free = free_step(c, pin)
            bind(name, hot)
            want = step(c, pin)
            bind(name, top_hitters(c, 8)[::-1])  # (whatever the handle holds during the scene call is not read)
            got = step(c, pin, scene=(lo, hi))
            assert_the_obstacles_matter(c, hot, want, free)
            assert torch.equal(bits(got), bits(want)), (name, O, where, pin)
    finally:
        bind(name, [])


# ---- 3. more than 8 at once ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROBOTS)
def test_fifteen_penetrating_cuboids_in_one_launch(name):
    # three trajectories of the pool with at least 5 cuboids each that only they penetrate (the first such triple)
    import itertools

    whole = pool(name).pen.any(axis=1)  # [S_MAX, N]
    trajs = next(t for t in itertools.combinations(range(S_MAX), 3)
                 if all((whole[s] & ~whole[[u for u in t if u != s]].any(axis=0)).sum() >= 5 for s in t))  # fmt: skip
    c = case(name, 3, 59, trajs)
    per_traj = c.pen.any(axis=1)  # [S, N]
    A = []
    for s in range(3):
        own = np.flatnonzero(per_traj[s] & ~np.delete(per_traj, s, axis=0).any(axis=0))
        traj = dataclasses.replace(c, pen=c.pen[s : s + 1], dist=c.dist[s : s + 1], live=c.live[s : s + 1])
        A.append(sorted(top_hitters(traj, 5, among=own)))
    flat = sorted(i for a in A for i in a)
    assert len(set(flat)) == 15
    for s in range(3):  # trajectory s penetrates all of A_s and nothing outside it
        assert set(np.flatnonzero(per_traj[s][flat]).tolist()) == {flat.index(i) for i in A[s]}
    lo, hi = scene_of(name, flat)  # interleaved: ascending candidate index
    try:
        for pin in PINS:
            free = free_step(c, pin)
            got = step(c, pin, scene=(lo, hi))
            assert_the_obstacles_matter(c, flat, got, free)
            for s in range(3):
                bind(name, A[s])
                want = step(c, pin)
                assert torch.equal(bits(got[s]), bits(want[s])), (name, pin, s)
    finally:
        bind(name, [])


# ---- 4. degenerate scenes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROBOTS)
def test_an_empty_scene_and_the_env_switch(name):
    c = case(name, 3, 59)
    hot = top_hitters(c, 8)
    lo, hi = scene_of(name, hot)
    empty = torch.empty((0, 3), dtype=torch.float32, device=DEV)
    off = _params(use_env_collisions=False)
    try:
        for pin in PINS:
            free = free_step(c, pin)
            free_off = step(c, pin, pm=off)
            bind(name, hot)  # the handle penetrates: none of it may show below
            assert not torch.equal(bits(step(c, pin)), bits(free))
            assert torch.equal(bits(step(c, pin, scene=(empty, empty))), bits(free)), (name, pin, "n_obs = 0")
            assert torch.equal(bits(step(c, pin, scene=(lo, hi), pm=off)), bits(free_off)), (name, pin, "use_env_collisions = 0")
            assert torch.equal(bits(step(c, pin, pm=off)), bits(free_off))
    finally:
        bind(name, [])


# ---- 5. memory discipline and determinism --------------------------------------------------------------------------------------------------
def run_in_arena(name, c, lo, hi, pin, poison, stream=None):
    """the entry point with x_out and the three workspaces carved out of one sentinel-filled arena with guard gaps; the workspaces
    poisoned.  Returns x_out [S*W, d] (a copy)."""
    from cppflow_amd import _hip

    rb = setup(name)[0]
    d, n = rb.ndof, c.S * c.W
    prm = rb.full_params(_params())
    sizes = (("x_out", n * d), ("blocks", n * (d * (d + 1) // 2 + d)), ("G", n * d * d), ("y", n * d))
    arena = torch.full((sum(k for _, k in sizes) + 5 * 1024,), SENTINEL, dtype=torch.int32, device=DEV)
    cursor, spans, bufs = 512, [], {}
    for nm, k in sizes:
        bufs[nm] = arena[cursor : cursor + k]
        spans.append((cursor, cursor + k))
        cursor += k + 1024
    assert cursor <= arena.numel()
    for nm in ("blocks", "G", "y"):
        bufs[nm].fill_(poison)
    torch.cuda.synchronize()
    st = (stream if stream is not None else torch.cuda.current_stream(DEV)).cuda_stream
    _hip.check(_hip.lib().cppf_lm_full_step_scene(rb._handle(torch.device(DEV)), c.xd.data_ptr(), c.td.data_ptr(), c.xd.data_ptr(), c.S, c.W,
                                                 ctypes.byref(prm), pin, lo.data_ptr(), hi.data_ptr(), lo.shape[0], bufs["blocks"].data_ptr(),
                                                 bufs["G"].data_ptr(), bufs["y"].data_ptr(), bufs["x_out"].data_ptr(), st))  # fmt: skip
    torch.cuda.synchronize()
    keep = torch.ones(arena.numel(), dtype=torch.bool, device=DEV)
    for a, b in spans:
        keep[a:b] = False
    assert bool((arena[keep] == SENTINEL).all()), "a guard gap was written"
    out = bufs["x_out"].clone()
    assert bool((out != SENTINEL).all()), "a row of x_out was not written"
    return out.view(torch.float32).view(n, d)


@pytest.mark.parametrize("name,S,W", [("panda", 3, 59), ("fetch", 9, 25), ("generic7", 1, 59), ("chain12", 3, 25)])
def test_memory_discipline_and_determinism(name, S, W):
    c = case(name, S, W)
    idx, _ = cluttered(case(name, 3, 59), 200, "spread") if (S, W) == (3, 59) else (top_hitters(c, 8) + list(np.flatnonzero(c.hits == 0)[:57]), None)
    lo, hi = scene_of(name, idx)
    before = [t.clone() for t in (c.xd, c.td, lo, hi)]
    for pin in PINS:
        runs = [run_in_arena(name, c, lo, hi, pin, 0x7FC00000), run_in_arena(name, c, lo, hi, pin, 0x5A5A5A5A),
                run_in_arena(name, c, lo, hi, pin, 0x7FC00000, torch.cuda.Stream(device=DEV))]  # fmt: skip
        for r in runs[1:]:
            assert torch.equal(bits(r), bits(runs[0])), (name, pin)
        assert torch.equal(bits(runs[0]), bits(step(c, pin, scene=(lo, hi)).reshape(S * W, -1))), (name, pin)
    for t, b in zip((c.xd, c.td, lo, hi), before):
        assert torch.equal(bits(t), bits(b))


@pytest.mark.parametrize("name", ROBOTS)
def test_trajectories_in_another_order_give_the_permuted_result(name):
    c = case(name, 9, 25)
    hot = top_hitters(c, 12)
    lo, hi = scene_of(name, hot + list(np.flatnonzero(c.hits == 0)[:60]))
    perm = np.random.RandomState(3).permutation(c.S)
    assert not np.array_equal(perm, np.arange(c.S))
    x3 = c.xd.view(c.S, c.W, -1)
    shuffled = dataclasses.replace(c, xd=x3[torch.tensor(perm, device=DEV)].contiguous().view(c.S * c.W, -1))
    for pin in PINS:
        base = step(c, pin, scene=(lo, hi))
        assert_the_obstacles_matter(c, hot, base, free_step(c, pin))
        got = step(shuffled, pin, scene=(lo, hi))
        assert torch.equal(bits(got), bits(base[torch.tensor(perm, device=DEV)])), (name, pin)


def test_graph_capture_replays_the_call():
    c = case("panda", 3, 59)
    idx, _ = cluttered(c, 65, "spread")
    lo, hi = scene_of("panda", idx)
    rb = setup("panda")[0]
    pm = _params()
    want = step(c, 0, scene=(lo, hi))
    side = torch.cuda.Stream(device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        rb.lm_full_step(c.xd, c.td, pm, virtual_configs=c.xd, scene=(lo, hi))  # (warm: the allocator's pool, the handle)
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            got = rb.lm_full_step(c.xd, c.td, pm, virtual_configs=c.xd, scene=(lo, hi))
    for _ in range(2):
        bits(got).fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(got), bits(want.reshape(got.shape)))


# ---- 6. / 7. the planner with scene_optimizer=True -----------------------------------------------------------------------------------------
def _fixture_problem():
    from cppflow_amd.data_type_utils import problem_from_filename

    return problem_from_filename(None, "panda__1cube_mini", problems_dir=os.path.join(REF, "problems"), paths_dir=os.path.join(REF, "paths"),
                                 device=DEV)  # fmt: skip


def _planner(problem, scene_optimizer):
    from cppflow_amd.data_types import PlannerSettings
    from cppflow_amd.planners import CppFlowPlanner, TrackingSeedProvider

    settings = PlannerSettings(k=175, tmax_sec=60.0, anytime_mode_enabled=False, do_rerun_if_large_dp_search_mjac=False,
                               do_rerun_if_optimization_fails=False, verbosity=0)  # fmt: skip
    return CppFlowPlanner(settings, problem.robot, seed_provider=TrackingSeedProvider(seed=0), scene_optimizer=scene_optimizer)


def _with_cuboids(problem, obs):
    return dataclasses.replace(problem, obstacles_cuboids=[torch.tensor(c) for c, _ in obs],
                               obstacles_Tcuboids=[torch.tensor(T) for _, T in obs], active_obstacles=None)  # fmt: skip


def _plan_fields_equal(a, b):
    for f in dataclasses.fields(a):
        va, vb = getattr(a, f.name), getattr(b, f.name)
        if isinstance(va, torch.Tensor):
            assert torch.equal(va.view(torch.uint8) if va.dtype != torch.bool else va, vb.view(torch.uint8) if vb.dtype != torch.bool else vb), f.name
        elif f.name not in ("constraints",):
            assert va == vb or (va is None and vb is None), f.name


def cut_cube(base, k):
    """the cube of panda__1cube_mini cut into k x k x k equal sub-cuboids whose union is the cube"""
    c, T = base.obstacles_cuboids[0].cpu().numpy().astype(np.float64), base.obstacles_Tcuboids[0].cpu().numpy().astype(np.float64)
    size = c[3:] - c[:3]
    obs = []
    for i in range(k):
        for j in range(k):
            for l in range(k):
                centre = T[:3, 3] + c[:3] + (np.array([i, j, l]) + 0.5) * size / k
                obs.append(H.cuboid_obstacle(*centre, *(size / k)))
    return obs


def test_far_clutter_changes_nothing_end_to_end():
    """panda__1cube_mini + 60 cuboids at radius 1.5 - 2.5 m (the recipe of tests/test_gpu_scene.py), optimised against the whole
    scene: the plan equals the unchanged one-cube problem's bit for bit, and nothing was selected"""
    from tests.test_gpu_scene import polar_cuboids

    base = _fixture_problem()
    assert len(base.obstacles_cuboids) == 1
    cube = (base.obstacles_cuboids[0].cpu().numpy().astype(np.float32), base.obstacles_Tcuboids[0].cpu().numpy().astype(np.float32))
    _, _, far = polar_cuboids((1.5, 2.5), 60, np.random.default_rng(1))
    clut = _with_cuboids(base, [cube] + far)
    assert clut.uses_scene and clut.n_obstacles == 61 and clut.robot is base.robot
    want = _planner(base, False).generate_plan(base)
    got = _planner(clut, True).generate_plan(clut)
    assert torch.equal(got.plan.q_path, want.plan.q_path)
    assert got.debug_info["n_optimization_steps"] == want.debug_info["n_optimization_steps"]
    _plan_fields_equal(got.plan, want.plan)
    assert got.debug_info["scene_selection_rounds"] == 0 and got.debug_info["active_obstacles"] is None
    assert got.debug_info["scene_optimizer"] is True and "scene_optimizer" not in want.debug_info


def plan_on_a_cut_cube(k, scene_optimizer):
    """(PlannerResult, the oracle's env mask of its path over all k^3 pieces, what set_obstacles was given during the optimiser)"""
    from cppflow_amd import planners

    base = _fixture_problem()
    obs = cut_cube(base, k)
    problem = _with_cuboids(base, obs)
    assert problem.n_obstacles == k**3 and problem.uses_scene
    bound, inside = [], [False]
    set_obstacles, optimise = problem.robot.set_obstacles, planners.run_lm_optimization

    def recording(cuboids, Tcuboids):
        if inside[0]:
            bound.append(len(cuboids))
        return set_obstacles(cuboids, Tcuboids)

    def optimiser(*a, **kw):
        inside[0] = True
        try:
            return optimise(*a, **kw)
        finally:
            inside[0] = False

    problem.robot.set_obstacles, planners.run_lm_optimization = recording, optimiser
    try:
        res = _planner(problem, scene_optimizer).generate_plan(problem)
    finally:
        del problem.robot.set_obstacles
        planners.run_lm_optimization = optimise
    lo, hi = H.box_corners([c for c, _ in obs], [T for _, T in obs])
    ch = H.chain("panda")
    x = res.plan.q_path.cpu().numpy().astype(np.float64)
    want_env = H.oracle32("panda").masks(x, lo, hi, ch.lo, ch.hi)["env_mask"].astype(bool)
    return res, want_env, bound


def test_the_27_piece_cube_is_optimised_against_all_of_its_pieces():
    res, want_env, bound = plan_on_a_cut_cube(3, True)
    assert "n_optimization_steps" in res.debug_info  # the optimiser ran
    assert all(b == 0 for b in bound), bound  # nothing was bound to the handle for the environment
    assert res.debug_info["scene_selection_rounds"] == 0 and res.debug_info["active_obstacles"] is None and res.debug_info["scene_optimizer"] is True
    assert np.array_equal(res.plan.env_colliding_per_ts.cpu().numpy(), want_env)
    assert not (res.plan.is_valid and want_env.any())
    off, off_env, _ = plan_on_a_cut_cube(3, False)
    for tag, r, env in (("scene_optimizer=True ", res, want_env), ("scene_optimizer=False", off, off_env)):
        print(f"27 sub-cuboids, {tag}: is_valid={r.plan.is_valid}, LM steps={r.debug_info['n_optimization_steps']}, "
              f"rounds={r.debug_info['scene_selection_rounds']}, active={r.debug_info['active_obstacles']}, "
              f"env-colliding waypoints={int(env.sum())}, flags={r.plan.validity_flags()}")  # fmt: skip


def test_the_optimiser_loop_takes_its_coupled_steps_on_the_scene():
    """run_lm_optimization(scene_in_step=True) with a budget that makes the loop take coupled steps (the planner's non-anytime budget
    stops at the first valid iterate, usually before one): on panda__1cube_mini + 60 cuboids beyond reach every coupled step goes to
    the scene -- all 61 cuboids, nothing bound to the handle -- and x_opt, the step count and the verdict equal the unchanged one-cube
    problem's, whose loop steps on the handle.  The same on the 27-piece cube: the verdict speaks for all 27."""
    from cppflow_amd.optimization import run_lm_optimization
    from tests.test_gpu_scene import polar_cuboids

    base = _fixture_problem()
    cube = (base.obstacles_cuboids[0].cpu().numpy().astype(np.float32), base.obstacles_Tcuboids[0].cpu().numpy().astype(np.float32))
    _, _, far = polar_cuboids((1.5, 2.5), 60, np.random.default_rng(1))
    clut, cut = _with_cuboids(base, [cube] + far), _with_cuboids(base, cut_cube(base, 3))
    seed = _planner(base, False)._run_pipeline(base)[0].contiguous()
    budget = dict(tmax_sec=None, max_n_steps=12, return_if_valid_after_n_steps=8, convergence_threshold=0.0, verbosity=0)
    rb = base.robot
    calls, bound = [], []
    full_step, set_obstacles = rb.lm_full_step, rb.set_obstacles

    def stepping(*a, **kw):
        calls.append(None if kw.get("scene") is None else int(kw["scene"][0].shape[0]))
        return full_step(*a, **kw)

    def binding(cuboids, Tcuboids):
        bound.append(len(cuboids))
        return set_obstacles(cuboids, Tcuboids)

    rb.lm_full_step, rb.set_obstacles = stepping, binding
    try:
        want = run_lm_optimization(base, seed.clone(), **budget)
        on_handle, calls[:] = list(calls), []
        bound[:] = []
        got = run_lm_optimization(clut, seed.clone(), scene_in_step=True, **budget)
        on_scene, bound_scene = list(calls), list(bound)
        calls[:] = []
        got27 = run_lm_optimization(cut, seed.clone(), scene_in_step=True, **budget)
        on_27 = list(calls)
    finally:
        del rb.lm_full_step, rb.set_obstacles
    assert len(on_handle) >= 1 and all(c is None for c in on_handle)  # the loop did take coupled steps
    assert on_scene == [61] * len(on_handle) and all(b == 0 for b in bound_scene), (on_scene, bound_scene)
    assert torch.equal(bits(got.x_opt), bits(want.x_opt)) and got.n_steps_taken == want.n_steps_taken and got.is_valid == want.is_valid
    assert got.scene_selection_rounds == 0 and got.active_obstacles is None
    assert len(on_27) >= 1 and all(c == 27 for c in on_27)
    env27 = cut.env_collision_mask(got27.x_opt.view(1, -1, rb.ndof))
    assert not (got27.is_valid and bool(env27.any()))
    print(f"12-step budget: coupled steps {len(on_handle)} (one cube) / {len(on_scene)} (61 cuboids) / {len(on_27)} (27 pieces); "
          f"valid {want.is_valid} / {got.is_valid} / {got27.is_valid}")


# ---- 8. handles: specialised at run time, destroyed ------------------------------------------------------------------------------------------
def test_a_handle_specialised_at_run_time_is_served_by_the_generic_form():
    """generic7's description specialised with hipRTC: the scene step does not refuse, and equals the unspecialised handle's scene
    step and the step on a handle that holds the penetrating cuboids, bit for bit"""
    from cppflow_amd.robots import Robot

    rtc = Robot(H.random_chain_spec(7, seed=21), specialize=True)
    assert rtc.specialization() == 1000
    c = case("generic7", 3, 59)
    idx, pos = cluttered(c, 65, "spread")
    hot = [idx[i] for i in pos]
    lo, hi = scene_of("generic7", idx)
    p = pool("generic7")
    try:
        for pin in PINS:
            free = free_step(c, pin)
            bind("generic7", hot)
            want = step(c, pin)
            plain = step(c, pin, scene=(lo, hi))
            assert_the_obstacles_matter(c, hot, want, free)
            got = rtc.lm_full_step(c.xd, c.td, _params(), virtual_configs=c.xd, pin=pin, scene=(lo, hi)).view(c.S, c.W, -1)
            rtc.set_obstacles([p.obs[i][0] for i in hot], [p.obs[i][1] for i in hot])
            on_handle = rtc.lm_full_step(c.xd, c.td, _params(), virtual_configs=c.xd, pin=pin).view(c.S, c.W, -1)
            rtc.set_obstacles([], [])
            torch.cuda.synchronize()
            assert torch.equal(bits(got), bits(plain)) and torch.equal(bits(got), bits(want)) and torch.equal(bits(got), bits(on_handle)), pin
    finally:
        bind("generic7", [])


def test_a_destroyed_handle_is_refused():
    """on a handle that cppf_robot_destroy has marked dead (kept allocated by a live batch): CPPF_ERR_INVALID with a message, nothing
    launched -- x_out and the workspaces keep their sentinel"""
    import gc

    from cppflow_amd import _hip
    from cppflow_amd.robot_zoo import ROBOT_SPECS
    from cppflow_amd.robots import Robot

    rb = Robot(ROBOT_SPECS["panda"]())
    x0, target = H.lm_problem("panda", 4, 64, seed=1)
    x0, target = dev(x0), dev(target)
    plan = rb.lm_batch_plan([dict(x=x0, target=target, x_out=torch.empty_like(x0))], 1e-6, 3.5, 0.35, n_steps=3)
    handle = rb._handle(torch.device(DEV))
    prm = rb.full_params(_params())
    plan._keep[0] = None
    _hip.lib().cppf_robot_destroy(handle)
    rb._handles = {}
    del rb
    gc.collect()
    c = case("panda", 3, 59)
    lo, hi = scene_of("panda", top_hitters(c, 8))
    d, n = 7, c.S * c.W
    bufs = [torch.full((k,), SENTINEL, dtype=torch.int32, device=DEV) for k in (n * d, n * (d * (d + 1) // 2 + d), n * d * d, n * d)]
    out, blocks, G, y = bufs
    rc = _hip.lib().cppf_lm_full_step_scene(handle, c.xd.data_ptr(), c.td.data_ptr(), c.xd.data_ptr(), c.S, c.W, ctypes.byref(prm), 0,
                                            lo.data_ptr(), hi.data_ptr(), lo.shape[0], blocks.data_ptr(), G.data_ptr(), y.data_ptr(),
                                            out.data_ptr(), None)  # fmt: skip
    assert rc == _hip.CPPF_ERR_INVALID and "destroyed" in _hip.lib().cppf_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool((b == SENTINEL).all()) for b in bufs)  # nothing was launched
    del plan
    gc.collect()
