"""Obstacle scenes on the MI355X: cppf_scene_env_collisions (csrc/kernels_scene.h) bit for bit against the fp32 oracle and against
the existing 8-cuboid launch, its memory discipline and determinism, and the planner on problems with more than 8 cuboids.

The scene recipe: cuboid centres in polar form, radius uniform in [0.30, 0.95] m (Panda, chain12) / [0.50, 1.15] m (Fetch, FetchArm:
without the keep-out every scene hits Fetch's base capsule), angle uniform, z in [0, 1.3] m, half-sizes uniform in [0.02, 0.06] m per
axis, numpy.default_rng(0); 200 cuboids per robot, a scene of O cuboids is the first O of them.  Rows: the first n of
helpers.random_configs(name, 300, seed=3).  Expected values: oracle32(name).env_dists(x, lo[o], hi[o]) per cuboid, computed ONCE per
robot for 300 rows x 200 cuboids and reduced in NumPy by the definitions (include/cppflow_hip.h).

What the recipe has to exercise is asserted on the oracle's answer before anything is compared (test_the_recipe_exercises_...): for
every robot, with all 300 rows, each of O = 9, 65, 200 has colliding and free rows, and -- at reach = 0.05 -- finite and infinite
min_env and obs_min; the O = 200 scenes hold rows whose minimum is attained by more than one cuboid (the tie rule).  (O = 0, 1, 8 and
the single-row cases cannot hold both sides by construction; they are compared all the same.)"""

import ctypes
import dataclasses
import functools
import gc
import os

import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF = os.path.join(GOLDEN, "reference_files")
ROBOTS = ("panda", "fetch", "fetch_arm", "chain12")
RADII = {"panda": (0.30, 0.95), "chain12": (0.30, 0.95), "fetch": (0.50, 1.15), "fetch_arm": (0.50, 1.15)}
OS = (0, 1, 8, 9, 63, 64, 65, 200)
NS = (1, 63, 64, 65, 257, 300)
REACHES = (0.0, 0.05, float("inf"))
N_ROWS, O_MAX = 300, 200
INF = np.float32(np.inf)


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


def polar_cuboids(radii, n, rng):
    """(lo [n,3], hi [n,3]) fp32 corners, (cuboid [6], Tcuboid [4,4]) pairs as the loader builds them"""
    r, a, z = rng.uniform(*radii, n), rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 1.3, n)
    half = rng.uniform(0.02, 0.06, (n, 3))
    obs = [H.cuboid_obstacle(r[i] * np.cos(a[i]), r[i] * np.sin(a[i]), z[i], *(2 * half[i])) for i in range(n)]
    lo, hi = H.box_corners([c for c, _ in obs], [T for _, T in obs])
    return lo.astype(np.float32), hi.astype(np.float32), obs


@functools.lru_cache(maxsize=None)
def scene(name):
    """(x [300,d] f64, lo, hi [200,3] f32, obstacles, D [300,200] f32 = the oracle's min over capsules)"""
    x = H.random_configs(name, N_ROWS, seed=3)
    lo, hi, obs = polar_cuboids(RADII[name], O_MAX, np.random.default_rng(0))
    orc = H.oracle32(name)
    D = np.stack([orc.env_dists(x, lo[o].astype(np.float64), hi[o].astype(np.float64)).min(axis=1) for o in range(O_MAX)], axis=1)
    assert np.array_equal(D.astype(np.float32).astype(np.float64), D)  # (the fp32 oracle's values ARE fp32)
    return x, lo, hi, obs, D.astype(np.float32)


def expected(D, reach):
    """the definitions on D [n,O] -> env_mask u8 [n], min_env f32 [n], nearest_obs i32 [n], obs_min f32 [O]"""
    n, O = D.shape
    reach = np.float32(reach)
    m = D.min(axis=1) if O else np.full(n, INF, dtype=np.float32)
    mask = (D < 0).any(axis=1).astype(np.uint8) if O else np.zeros(n, dtype=np.uint8)
    min_env = np.where(m < reach, m, INF).astype(np.float32)
    nearest = np.where(np.isfinite(min_env), D.argmin(axis=1) if O else -1, -1).astype(np.int32)  # (argmin: the first = lowest index)
    om = D.min(axis=0) if n else np.full(O, INF, dtype=np.float32)
    obs_min = np.where(om < reach, om, INF).astype(np.float32)
    return mask, min_env, nearest, obs_min


@functools.lru_cache(maxsize=None)
def robot(name):
    from cppflow_amd.robot_zoo import ROBOT_SPECS
    from cppflow_amd.robots import Robot

    return Robot(ROBOT_SPECS[name]())


@functools.lru_cache(maxsize=None)
def device_scene(name):
    x, lo, hi, _, _ = scene(name)
    return dev(x), dev(lo), dev(hi)


def check_outputs(got, want, ctx):
    mask, min_env, nearest, obs_min = want
    assert np.array_equal(host(got["env_mask"]).astype(np.uint8).reshape(-1), mask), ctx
    if "min_env" in got:
        assert np.array_equal(bits(host(got["min_env"]).reshape(-1)), bits(min_env)), ctx
    if "nearest_obs" in got:
        assert np.array_equal(host(got["nearest_obs"]).reshape(-1), nearest), ctx
    if "obs_min" in got:
        assert np.array_equal(bits(host(got["obs_min"])), bits(obs_min)), ctx


def test_the_recipe_exercises_both_sides_of_every_truncation_and_the_tie_rule():
    n_tied_cases = 0
    for name in ROBOTS:
        D = scene(name)[4]
        for O in (9, 65, 200):
            mask, min_env, nearest, obs_min = expected(D[:, :O], 0.05)
            print(f"{name} O={O}: colliding {mask.mean():.3f}, min_env > 0.05 {np.isinf(min_env).mean():.3f}, "
                  f"cuboids never within 0.05 {int(np.isinf(obs_min).sum())}")  # fmt: skip
            assert mask.any() and not mask.all(), (name, O)
            assert np.isfinite(min_env).any() and np.isinf(min_env).any(), (name, O)
            assert np.isfinite(obs_min).any() and np.isinf(obs_min).any(), (name, O)
        d = D[:, :200]
        tied = int(((d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
        print(f"{name} O=200: rows whose minimum is attained more than once: {tied}")
        n_tied_cases += tied > 0
    assert n_tied_cases >= 1


# ---- 1. bit-exact parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("O", OS)
@pytest.mark.parametrize("name", ROBOTS)
def test_bit_exact_against_the_oracle(name, O):
    rb = robot(name)
    xd, lod, hid = device_scene(name)
    D = scene(name)[4]
    for n in NS:
        q = xd[:n].contiguous()
        for reach in REACHES:
            got = rb.scene_env_collisions(q, lod[:O].contiguous(), hid[:O].contiguous(), reach=reach)
            assert got["env_mask"].shape == (n,) and got["obs_min"].shape == (O,)
            check_outputs(got, expected(D[:n, :O], reach), (name, O, n, reach))
        # once with only env_mask requested (the form without square roots)
        got = rb.scene_env_collisions(q, lod[:O].contiguous(), hid[:O].contiguous(), reach=0.05, want=("env_mask",))
        assert set(got) == {"env_mask"}
        check_outputs(got, expected(D[:n, :O], 0.05), (name, O, n, "mask only"))
    # q as [S, W, d]: the same rows
    got = rb.scene_env_collisions(xd.view(3, 100, -1), lod[:O].contiguous(), hid[:O].contiguous(), reach=0.05)
    assert got["min_env"].shape == (3, 100) and got["nearest_obs"].shape == (3, 100)
    check_outputs(got, expected(D[:, :O], 0.05), (name, O, "3 x 100"))


# ---- 2. against the existing launch ------------------------------------------------------------------------------------------------------
def masks_in_chunks_of_8(rb, q, obs):
    """what the parent commit offers: ceil(O / 8) rounds of set_obstacles + cppf_collision_masks, OR / min over the rounds"""
    mask = torch.zeros(q.shape[:-1], dtype=torch.bool, device=q.device)
    m = torch.full(q.shape[:-1], float("inf"), device=q.device)
    try:
        for i in range(0, len(obs), 8):
            rb.set_obstacles([c for c, _ in obs[i : i + 8]], [T for _, T in obs[i : i + 8]])
            r = rb.collision_masks(q, want_min_dists=True, only=("env",))
            mask |= r["env_mask"]
            m = torch.minimum(m, r["min_env"])
    finally:
        rb.set_obstacles([], [])
    return mask, m


@pytest.mark.parametrize("name", ROBOTS)
def test_equals_the_existing_launch_over_chunks_of_8(name):
    rb = robot(name)
    xd, lod, hid = device_scene(name)
    obs = scene(name)[3][:65]
    q = xd.view(1, N_ROWS, -1)
    want_mask, want_min = masks_in_chunks_of_8(rb, q, obs)
    got = rb.scene_env_collisions(q, lod[:65].contiguous(), hid[:65].contiguous())
    assert torch.equal(got["env_mask"], want_mask) and torch.equal(got["min_env"].view(torch.int32), want_min.view(torch.int32))
    only = rb.scene_env_collisions(q, lod[:65].contiguous(), hid[:65].contiguous(), want=("env_mask",))
    assert torch.equal(only["env_mask"], want_mask)
    assert bool(want_mask.any()) and not bool(want_mask.all())


def test_equals_the_existing_launch_on_tracked_candidates_of_a_reference_path():
    """a coherent input: 4 candidates tracked along the first 64 waypoints of panda__1cube (tests/golden/reference_paths.npz) -- consecutive
    lanes are consecutive waypoints, the case the wavefront's bounding box is made for"""
    rb = robot("panda")
    target = dev(np.load(os.path.join(GOLDEN, "reference_paths.npz"))["panda__1cube_first64"])
    q = rb.track_paths(target.contiguous(), 4, seed=5)["x"].contiguous()
    assert q.shape == (4, 64, 7)
    _, lod, hid = device_scene("panda")
    obs = scene("panda")[3]
    for O in (65, 200):
        want_mask, want_min = masks_in_chunks_of_8(rb, q, obs[:O])
        for reach in (float("inf"), 0.05):
            got = rb.scene_env_collisions(q, lod[:O].contiguous(), hid[:O].contiguous(), reach=reach)
            assert torch.equal(got["env_mask"], want_mask)
            trunc = torch.where(want_min < reach, want_min, torch.full_like(want_min, float("inf")))
            assert torch.equal(got["min_env"].view(torch.int32), trunc.view(torch.int32))
        assert torch.equal(rb.scene_env_collisions(q, lod[:O].contiguous(), hid[:O].contiguous(), want=("env_mask",))["env_mask"], want_mask)


# ---- 3. arena and determinism ------------------------------------------------------------------------------------------------------------
def run_in_arena(rb, q, lo, hi, reach, poison, stream=None):
    """the entry point with outputs and workspace carved out of one poisoned arena with guard gaps -> dict of host arrays"""
    from cppflow_amd import _hip

    lib = _hip.lib()
    n, O = q.shape[0], lo.shape[0]
    nbytes = ctypes.c_size_t(0)
    _hip.check(lib.cppf_scene_workspace_bytes(n, O, ctypes.byref(nbytes)))
    arena = torch.full((1 << 20,), poison, dtype=torch.uint8, device=DEV)
    cursor, spans, bufs = 4096, [], {}
    for nm, nb in (("workspace", nbytes.value), ("env_mask", n), ("min_env", 4 * n), ("nearest_obs", 4 * n), ("obs_min", 4 * O)):
        start = (cursor + 255) // 256 * 256
        bufs[nm] = arena[start : start + nb]
        spans.append((start, start + nb))
        cursor = start + nb + 1024
    assert cursor + 4096 < arena.numel()
    torch.cuda.synchronize()
    st = (stream if stream is not None else torch.cuda.current_stream(DEV)).cuda_stream
    _hip.check(lib.cppf_scene_env_collisions(rb._handle(torch.device(DEV)), q.data_ptr(), 1, n, lo.data_ptr(), hi.data_ptr(), O, reach,
                                             bufs["env_mask"].data_ptr(), bufs["min_env"].data_ptr(), bufs["nearest_obs"].data_ptr(),
                                             bufs["obs_min"].data_ptr(), bufs["workspace"].data_ptr(), nbytes.value, st))  # fmt: skip
    torch.cuda.synchronize()
    keep = torch.ones(cursor + 4096, dtype=torch.bool, device=DEV)
    for a, b in spans:
        keep[a:b] = False
    assert bool((arena[: cursor + 4096][keep] == poison).all()), "a guard gap was written"  # nothing outside [n] / [O] / the workspace
    return {nm: host(bufs[nm]).copy() for nm in ("env_mask", "min_env", "nearest_obs", "obs_min")}


@pytest.mark.parametrize("name,n,O", [("panda", 300, 200), ("fetch", 65, 65), ("chain12", 257, 9), ("fetch_arm", 1, 63)])
def test_memory_discipline_and_determinism(name, n, O):
    rb = robot(name)
    xd, lod, hid = device_scene(name)
    q, lo, hi = xd[:n].contiguous(), lod[:O].contiguous(), hid[:O].contiguous()
    before = [t.clone() for t in (q, lo, hi)]
    runs = [run_in_arena(rb, q, lo, hi, 0.05, 0xA5), run_in_arena(rb, q, lo, hi, 0.05, 0x5A),
            run_in_arena(rb, q, lo, hi, 0.05, 0xA5, torch.cuda.Stream(device=DEV))]  # fmt: skip
    for r in runs[1:]:
        for nm, v in r.items():
            assert np.array_equal(v, runs[0][nm]), nm
    for t, b in zip((q, lo, hi), before):
        assert torch.equal(t.view(torch.int32), b.view(torch.int32))
    mask, min_env, nearest, obs_min = expected(scene(name)[4][:n, :O], 0.05)
    r = runs[0]
    assert np.array_equal(r["env_mask"], mask) and np.array_equal(r["min_env"].view(np.int32), bits(min_env))
    assert np.array_equal(r["nearest_obs"].view(np.int32), nearest) and np.array_equal(r["obs_min"].view(np.int32), bits(obs_min))


@pytest.mark.parametrize("name", ROBOTS)
def test_rows_may_share_a_wavefront_in_any_order_and_the_generic_form_agrees(name):
    rb = robot(name)
    xd, lod, hid = device_scene(name)
    lo, hi = lod[:200].contiguous(), hid[:200].contiguous()
    perm = torch.tensor(np.random.RandomState(7).permutation(N_ROWS), device=DEV)
    for reach in (0.05, float("inf")):
        base = rb.scene_env_collisions(xd, lo, hi, reach=reach)
        shuf = rb.scene_env_collisions(xd[perm].contiguous(), lo, hi, reach=reach)
        for nm in ("env_mask", "min_env", "nearest_obs"):
            assert torch.equal(shuf[nm].view(torch.uint8), base[nm][perm].contiguous().view(torch.uint8)), (nm, reach)
        assert torch.equal(shuf["obs_min"].view(torch.int32), base["obs_min"].view(torch.int32))
        assert rb.specialization() >= 0  # a generated table
        rb.debug_set("force_generic", 1)
        try:
            gen = rb.scene_env_collisions(xd, lo, hi, reach=reach)
            gen_mask = rb.scene_env_collisions(xd, lo, hi, want=("env_mask",))["env_mask"]
        finally:
            rb.debug_set("force_generic", None)
        for nm in base:
            assert torch.equal(gen[nm].view(torch.uint8), base[nm].view(torch.uint8)), (nm, reach)
        assert torch.equal(gen_mask, base["env_mask"])


def test_a_handle_specialised_at_run_time_is_served_by_the_generic_form():
    """a description that matches no generated table, specialised with hipRTC: the scene call does not refuse, and equals both the
    same description's unspecialised handle and the fp32 oracle, bit for bit"""
    from cppflow_amd import _hip
    from cppflow_amd.robot_model import canonicalize
    from cppflow_amd.robots import Robot
    from oracle.oracle import Oracle

    spec = H.random_chain_spec(7, seed=21)
    chain = canonicalize(spec)
    rtc, plain = Robot(spec, specialize=True), Robot(spec, specialize=False)
    assert rtc.specialization() == 1000 and plain.specialization() == -1
    n, O = 130, 65
    x = H.f32(np.random.RandomState(4).uniform(chain.lo, chain.hi, size=(n, chain.ndof)))
    _, lod, hid = device_scene("panda")
    lo, hi = scene("panda")[1][:O], scene("panda")[2][:O]
    orc = Oracle(chain, f32=True)
    D = np.stack([orc.env_dists(x, lo[o].astype(np.float64), hi[o].astype(np.float64)).min(axis=1) for o in range(O)], axis=1).astype(np.float32)
    for reach in (0.05, float("inf")):
        a = rtc.scene_env_collisions(dev(x), lod[:O].contiguous(), hid[:O].contiguous(), reach=reach)
        b = plain.scene_env_collisions(dev(x), lod[:O].contiguous(), hid[:O].contiguous(), reach=reach)
        for nm in a:
            assert torch.equal(a[nm].view(torch.uint8), b[nm].view(torch.uint8)), (nm, reach)
        check_outputs(a, expected(D, reach), ("rtc", reach))
    check_outputs(rtc.scene_env_collisions(dev(x), lod[:O].contiguous(), hid[:O].contiguous(), want=("env_mask",)), expected(D, 0.0), "rtc mask")
    assert _hip.lib().cppf_abi_version() == 6


def test_graph_capture_replays_the_call():
    rb = robot("panda")
    xd, lod, hid = device_scene("panda")
    lo, hi = lod[:65].contiguous(), hid[:65].contiguous()
    want = rb.scene_env_collisions(xd, lo, hi, reach=0.05)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        rb.scene_env_collisions(xd, lo, hi, reach=0.05)  # (warm: the allocator's pool, the handle)
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            got = rb.scene_env_collisions(xd, lo, hi, reach=0.05)
    for _ in range(2):
        for v in got.values():
            v.view(torch.uint8).fill_(0x77)
        g.replay()
        torch.cuda.synchronize()
        for nm in want:
            assert torch.equal(got[nm].view(torch.uint8), want[nm].view(torch.uint8)), nm


def test_a_destroyed_handle_is_refused():
    """on a handle that cppf_robot_destroy has marked dead (kept allocated by a live batch): CPPF_ERR_INVALID, nothing launched"""
    from cppflow_amd import _hip
    from cppflow_amd.robot_zoo import ROBOT_SPECS
    from cppflow_amd.robots import Robot

    rb = Robot(ROBOT_SPECS["panda"]())
    x0, target = H.lm_problem("panda", 4, 64, seed=1)
    x0, target = dev(x0), dev(target)
    plan = rb.lm_batch_plan([dict(x=x0, target=target, x_out=torch.empty_like(x0))], 1e-6, 3.5, 0.35, n_steps=3)
    handle = rb._handle(torch.device(DEV))
    plan._keep[0] = None
    _hip.lib().cppf_robot_destroy(handle)
    rb._handles = {}
    del rb
    gc.collect()
    xd, lod, hid = device_scene("panda")
    mask = torch.full((N_ROWS,), 7, dtype=torch.uint8, device=DEV)
    ws = torch.full((1 << 16,), 7, dtype=torch.uint8, device=DEV)
    rc = _hip.lib().cppf_scene_env_collisions(handle, xd.data_ptr(), 1, N_ROWS, lod.data_ptr(), hid.data_ptr(), 9, 0.05, mask.data_ptr(),
                                              None, None, None, ws.data_ptr(), ws.numel(), None)  # fmt: skip
    assert rc == _hip.CPPF_ERR_INVALID and "destroyed" in _hip.lib().cppf_last_error().decode()
    torch.cuda.synchronize()
    assert bool((mask == 7).all()) and bool((ws == 7).all())  # nothing was launched
    del plan
    gc.collect()


# ---- 4. / 5. the planner on more than 8 cuboids -------------------------------------------------------------------------------------------
def _fixture_problem():
    from cppflow_amd.data_type_utils import problem_from_filename

    return problem_from_filename(None, "panda__1cube_mini", problems_dir=os.path.join(REF, "problems"), paths_dir=os.path.join(REF, "paths"),
                                 device=DEV)  # fmt: skip


def _planner(problem, device_optimizer):
    from cppflow_amd.data_types import PlannerSettings
    from cppflow_amd.planners import CppFlowPlanner, TrackingSeedProvider

    settings = PlannerSettings(k=175, tmax_sec=60.0, anytime_mode_enabled=False, do_rerun_if_large_dp_search_mjac=False,
                               do_rerun_if_optimization_fails=False, verbosity=0)  # fmt: skip
    return CppFlowPlanner(settings, problem.robot, seed_provider=TrackingSeedProvider(seed=0), device_optimizer=device_optimizer)


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


@pytest.mark.parametrize("device_optimizer", [False, True])
def test_far_clutter_changes_nothing_end_to_end(device_optimizer):
    """panda__1cube_mini (T = 25) + 60 cuboids at radius 1.5 - 2.5 m, beyond the robot's reach: candidates' masks, search path, x_opt,
    LM steps and every Plan field equal the unchanged problem's bit for bit; the active set is the original cube, chosen once"""
    base = _fixture_problem()
    assert len(base.obstacles_cuboids) == 1
    cube = (host(base.obstacles_cuboids[0]).astype(np.float32), host(base.obstacles_Tcuboids[0]).astype(np.float32))
    _, _, far = polar_cuboids((1.5, 2.5), 60, np.random.default_rng(1))
    cluttered = _with_cuboids(base, [cube] + far)
    assert cluttered.uses_scene and cluttered.n_obstacles == 61 and cluttered.robot is base.robot
    pipes = []
    for problem in (base, cluttered):
        qpath, _, _, _, (qs, self_viol, env_viol) = _planner(problem, device_optimizer)._run_pipeline(problem)
        pipes.append((qpath, qs, self_viol, env_viol))
    for a, b in zip(*pipes):
        assert torch.equal(a, b)
    print(f"candidate rows touching the cube: {int(pipes[0][3].sum())} of {pipes[0][3].numel()}")
    want = _planner(base, device_optimizer).generate_plan(base)
    got = _planner(cluttered, device_optimizer).generate_plan(cluttered)
    assert torch.equal(got.plan.q_path, want.plan.q_path)
    assert got.debug_info["n_optimization_steps"] == want.debug_info["n_optimization_steps"]
    _plan_fields_equal(got.plan, want.plan)
    assert got.plan.is_valid == want.plan.is_valid
    assert got.debug_info["active_obstacles"] == [0] and got.debug_info["scene_selection_rounds"] == 1
    assert "active_obstacles" not in want.debug_info


@pytest.mark.parametrize("device_optimizer", [False, True])
def test_more_than_8_cuboids_within_reach(device_optimizer):
    """the cube of panda__1cube_mini cut into 27 equal sub-cuboids whose union is the cube: the planner returns, never binds more than 8,
    reports its selection rounds, and its verdict on the returned path is the oracle's over all 27"""
    base = _fixture_problem()
    c, T = host(base.obstacles_cuboids[0]).astype(np.float64), host(base.obstacles_Tcuboids[0]).astype(np.float64)
    size = c[3:] - c[:3]
    obs = []
    for i in range(3):
        for j in range(3):
            for k in range(3):
                centre = T[:3, 3] + c[:3] + (np.array([i, j, k]) + 0.5) * size / 3
                obs.append(H.cuboid_obstacle(*centre, *(size / 3)))
    problem = _with_cuboids(base, obs)
    assert problem.n_obstacles == 27 and problem.uses_scene
    bound = []
    set_obstacles = problem.robot.set_obstacles

    def recording(cuboids, Tcuboids):
        bound.append(len(cuboids))
        return set_obstacles(cuboids, Tcuboids)

    problem.robot.set_obstacles = recording
    try:
        res = _planner(problem, device_optimizer).generate_plan(problem)
    finally:
        del problem.robot.set_obstacles
    assert bound and max(bound) <= 8
    assert res.debug_info["scene_selection_rounds"] in (1, 2) and 1 <= len(res.debug_info["active_obstacles"]) <= 8
    lo, hi = H.box_corners([c for c, _ in obs], [T for _, T in obs])
    x = host(res.plan.q_path).astype(np.float64)
    ch = H.chain("panda")
    want_env = H.oracle32("panda").masks(x, lo, hi, ch.lo, ch.hi)["env_mask"].astype(bool)
    assert np.array_equal(host(res.plan.env_colliding_per_ts), want_env)
    assert res.plan.validity_flags()["env_collisions"] == (not want_env.any())
    assert not (res.plan.is_valid and want_env.any())
    print(f"27 sub-cuboids, device_optimizer={device_optimizer}: is_valid={res.plan.is_valid}, rounds={res.debug_info['scene_selection_rounds']}, "
          f"active={res.debug_info['active_obstacles']}, env-colliding waypoints={int(want_env.sum())}, flags={res.plan.validity_flags()}")  # fmt: skip
