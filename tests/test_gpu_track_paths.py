"""cppf_track_paths -- k candidate joint-space paths in one launch (csrc/kernels_track.h) -- and TrackingSeedProvider (pytest -m gpu).

Bars (the lean-parity test's language, tests/test_gpu_lean_parity.py):
  * Same algorithm as the stand-in: with S = 1, R = 0, no tolerances and LmIkSeedProvider's own starts, one launch runs the chain of
    fused launches the provider's loop issues.  Against that loop issued in the row shape (lm_pose_steps, SHAPE_ROW: the same device
    code) the candidates are bit-identical.  Against LmIkSeedProvider itself, whose launches of k rows take the four-lanes-per-row shape
    (kernels_quad.h; <= 1e-4 in scaled task space per step, the K = 1 floor of CPPF_SOLVER_AUTO), the median row agrees to 1e-4 rad; a
    track that has not converged at some waypoint may take another IK branch from there on under a rounding-level difference, so only
    >= 60 % of the rows are required on the same branch (< 1e-3 rad; measured 78 %), and on the rows converged on both sides
    (pos_err < 1e-4 m; 6 damped steps per waypoint leave most rows above that, so only a share of them) the agreement of the pose
    errors is that of q: bit-exact against the row-shape loop; against the quad-shape provider only the branch-level bars above (rows
    still converging differ by more than 1e-5 m in pose error, so that is not checked there).
  * Divergent lanes: segments of unequal length (T % S != 0) and the recovery ladder (lanes leave and re-enter LM blocks in a data-
    dependent pattern, the conditioning gate's cooperative fp64 re-solve runs on a non-prefix set of active lanes) are bit-exact
    against row-shape lm_pose_steps launches from the same starts, the ladder's random starts recomputed from the kernel's hash.
  * Segments and jumps: consecutive converged rows within a segment stay within max_jump unless the row carries CPPF_TRACK_JUMP --
    the ladder keeps its lowest-error attempt when none meets the bar, and flags it; the test checks that the flag is truthful.
  * Against the fp64 oracle (oracle64.lm_steps in a CPU loop over the waypoints, k = 32, T = 64): the same branch-level bars (measured
    75 % of the rows on the same branch, median 4e-6 rad), and pos_err_m / rot_err_rad are cppf_pose_error_metrics of the returned q
    to 1e-6.
  * Recovery ladder, segments, determinism, poisoning, robot coverage and the planner as the issue lists them (each test's docstring)."""

import dataclasses
import os

import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF = os.path.join(GOLDEN, "reference_files")
STANDIN = dict(lm_lambda=1e-2, alpha_position=3.5, alpha_rotation=0.35, n_restart=40, n_track=6)
TOL = dict(tol_pos_m=5e-5, tol_rot_rad=5e-4)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _fixture_problem(name):
    from cppflow_amd.data_type_utils import problem_from_arrays, problem_from_filename
    from cppflow_amd.robots import get_robot

    if name == "fetch_arm__s__truncated":
        return problem_from_filename(None, name, filepath_override=os.path.join(REF, name + ".yaml"),
                                     problems_dir=os.path.join(REF, "problems"), paths_dir=os.path.join(REF, "paths"), device=DEV)  # fmt: skip
    if name == "panda__1cube_first64":
        z = np.load(os.path.join(GOLDEN, "reference_paths.npz"))
        return problem_from_arrays(get_robot("panda"), z[name], device=DEV)
    return problem_from_filename(None, name, problems_dir=os.path.join(REF, "problems"), paths_dir=os.path.join(REF, "paths"), device=DEV)


def _standin_starts(problem, k, seed):
    """the [k, d] starts LmIkSeedProvider(seed) draws (planners.py)"""
    rb = problem.robot
    gen = torch.Generator().manual_seed(seed)
    lo = torch.tensor([l for l, _ in rb.actuated_joints_limits], dtype=torch.float32)
    hi = torch.tensor([u for _, u in rb.actuated_joints_limits], dtype=torch.float32)
    return (lo + (hi - lo) * (0.1 + 0.8 * torch.rand((k, rb.ndof), generator=gen))).to(DEV)


def _smooth_path(chain, oracle, T, seed):
    """a reachable target path: FK of a smooth joint-space path well inside the limits"""
    rng = np.random.RandomState(seed)
    lo, hi = np.asarray(chain.lo), np.asarray(chain.hi)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    a = mid + 0.3 * half * rng.uniform(-1, 1, size=lo.shape)
    b = np.clip(a + 0.3 * rng.uniform(-1, 1, size=lo.shape) * np.minimum(half, 1.0), lo, hi)
    s = 0.5 - 0.5 * np.cos(np.linspace(0, np.pi, T))[:, None]
    return H.f32(oracle.fk(H.f32(a + (b - a) * s)))


@pytest.mark.parametrize("name", ["fetch_arm__s__truncated", "panda__1cube_first64"])
def test_one_launch_matches_the_standin_loop(name):
    from cppflow_amd import _hip
    from cppflow_amd.planners import LmIkSeedProvider

    problem = _fixture_problem(name)
    rb, k, seed = problem.robot, 64, 5
    want = host(LmIkSeedProvider(seed=seed)(problem, k))
    q0 = _standin_starts(problem, k, seed)
    got = rb.track_paths(problem.target_path, k, n_segments=1, q0=q0, n_random_restarts=0, **STANDIN)
    torch.cuda.synchronize()
    x = host(got["x"])
    assert np.isfinite(x).all()
    # the provider's loop issued in the row shape: the same device code, bit for bit
    q, T = q0.clone(), problem.n_timesteps
    for t in range(T):
        q = rb.lm_pose_steps(q, problem.target_path[t : t + 1].contiguous(), STANDIN["lm_lambda"], 3.5, 0.35,
                             n_steps=40 if t == 0 else 6, clamp=True, shape=_hip.SHAPE_ROW)["x"]  # fmt: skip
        assert torch.equal(got["x"][:, t], q), t
    dq = np.abs(x - want).max(axis=2)  # [k, T]
    same = dq < 1e-3
    assert same.mean() >= 0.6, (same.mean(), np.quantile(dq, [0.5, 0.9, 0.99]))
    assert np.median(dq) < 1e-4, np.quantile(dq, [0.5, 0.9])
    # (the issue's "pose errors agree to 1e-5 m on rows converged on both sides" is carried by the bit-exact row-shape comparison
    # above -- q, hence pos_err, identical -- not checked against the quad-shape provider, whose iterates are still converging)
    # no tolerances: no convergence test, so no row climbs the ladder; the first row is a (given) fresh start
    st = host(got["status"]).astype(np.uint8)
    assert (st[:, 0] == 2).all() and (st[:, 1:] == 0).all()


def test_against_the_fp64_oracle_and_the_metrics_entry_point():
    from cppflow_amd.robots import get_robot

    name, k, T = "panda", 32, 64
    rb, o64, ch = get_robot(name), H.oracle64(name), H.chain(name)
    target = _smooth_path(ch, o64, T, seed=3)
    x0 = H.random_configs(name, k, seed=4, margin=0.2)
    got = rb.track_paths(torch.tensor(target, dtype=torch.float32, device=DEV), k, q0=torch.tensor(x0, dtype=torch.float32, device=DEV),
                         **STANDIN)  # fmt: skip
    torch.cuda.synchronize()
    x = host(got["x"])
    q, want = x0.copy(), np.empty_like(x)
    for t in range(T):
        q = o64.lm_steps(q, np.tile(target[t], (k, 1)), 40 if t == 0 else 6, STANDIN["lm_lambda"], 3.5, 0.35, solver=0)
        want[:, t] = q
    dq = np.abs(x - want).max(axis=2)
    assert (dq < 1e-3).mean() >= 0.6, np.quantile(dq, [0.5, 0.9, 0.99])
    assert np.median(dq) < 1e-4, np.quantile(dq, [0.5, 0.9])
    pe_o = np.stack([o64.pose_metrics_exact(want[:, t], np.tile(target[t], (k, 1)))[0] for t in range(T)], axis=1)
    conv = (pe_o < 1e-4) & (host(got["pos_err_m"]) < 1e-4)
    assert conv.mean() > 0.2 and np.abs(pe_o - host(got["pos_err_m"]))[conv].max() < 1e-5
    pe, re = rb.pose_error_metrics(got["x"].reshape(k * T, -1), torch.tensor(target, dtype=torch.float32, device=DEV))
    assert np.abs(host(pe).reshape(k, T) - host(got["pos_err_m"])).max() <= 1e-6
    assert np.abs(host(re).reshape(k, T) - host(got["rot_err_rad"])).max() <= 1e-6


def test_recovery_ladder_after_an_unreachable_waypoint():
    """Waypoint 32 of a reachable path is moved 3 m away: its rows are not converged; the rows after it climb the ladder (restarted or
    recovered) and the candidates converge again within three waypoints."""
    from cppflow_amd.robots import get_robot

    name, k, T, bad = "panda", 64, 64, 32
    rb, ch, o64 = get_robot(name), H.chain(name), H.oracle64(name)
    target = _smooth_path(ch, o64, T, seed=7)
    target[bad, 0] += 3.0
    got = rb.track_paths(torch.tensor(target, dtype=torch.float32, device=DEV), k, seed=1, n_random_restarts=3, **STANDIN, **TOL)
    torch.cuda.synchronize()
    st = host(got["status"]).astype(np.uint8)
    conv = (st & 1) != 0
    assert conv[:, :bad].mean() > 0.9, conv[:, :bad].mean()
    assert not conv[:, bad].any()
    ladder = (st[:, bad + 1] & (2 | 8)) != 0
    assert ladder.mean() >= 0.9, ladder.mean()
    assert conv[:, bad + 3 :].mean() > 0.9, conv[:, bad + 3 :].mean()
    # the kept attempt's flags are consistent with what is stored
    assert np.all(((st & 8) == 0) | ((st & 2) == 0))  # never both recovered by continuation and restarted


def test_segments_restart_and_keep_the_jump_bar():
    from cppflow_amd.robots import get_robot

    name, k, T, S = "fetch", 32, 64, 4
    rb, ch = get_robot(name), H.chain(name)
    target = _smooth_path(ch, H.oracle64(name), T, seed=11)
    bar_rad, bar_m = 0.3, 0.05
    got = rb.track_paths(torch.tensor(target, dtype=torch.float32, device=DEV), k, n_segments=S, seed=2, n_random_restarts=2,
                         max_jump_rad=bar_rad, max_jump_m=bar_m, **STANDIN, **TOL)  # fmt: skip
    torch.cuda.synchronize()
    st, x = host(got["status"]).astype(np.uint8), host(got["x"])
    starts = [(s * T) // S for s in range(S)]
    assert ((st[:, starts] & 2) != 0).all()
    pris = np.array([j in rb.prismatic_joint_idxs for j in range(rb.ndof)])
    bar = np.where(pris, bar_m, bar_rad)
    for t in range(1, T):
        if t in starts:
            continue
        ok = ((st[:, t] & 1) != 0) & ((st[:, t - 1] & 1) != 0) & ((st[:, t] & 4) == 0)
        jump = np.abs(x[:, t] - x[:, t - 1])
        assert (jump[ok] <= bar[None] + 1e-6).all(), t
        flagged = (st[:, t] & 4) != 0
        assert (jump[flagged] > bar[None]).any(axis=1).all(), t  # the flag means what it says
    assert ((st & 1) != 0).mean() > 0.8


def test_determinism_sentinels_and_poisoning():
    from cppflow_amd.robots import get_robot

    name, k, T = "fetch_arm", 40, 24
    rb, ch = get_robot(name), H.chain(name)
    tgt = torch.tensor(_smooth_path(ch, H.oracle64(name), T, seed=13), dtype=torch.float32, device=DEV)
    kw = dict(n_segments=3, seed=9, n_random_restarts=2, max_jump_rad=0.5, **STANDIN, **TOL)

    def nan_out():
        return {"x": torch.full((k, T, rb.ndof), float("nan"), device=DEV), "pos_err_m": torch.full((k, T), float("nan"), device=DEV),
                "rot_err_rad": torch.full((k, T), float("nan"), device=DEV), "status": torch.full((k, T), 0xFF, dtype=torch.uint8, device=DEV)}  # fmt: skip

    a = rb.track_paths(tgt, k, call_index=0, out=nan_out(), **kw)
    b = rb.track_paths(tgt, k, call_index=0, out=nan_out(), **kw)
    c = rb.track_paths(tgt, k, call_index=1, **kw)
    torch.cuda.synchronize()
    for key in ("x", "pos_err_m", "rot_err_rad", "status"):
        assert torch.equal(a[key], b[key]), key
    assert torch.isfinite(a["x"]).all() and torch.isfinite(a["pos_err_m"]).all() and torch.isfinite(a["rot_err_rad"]).all()
    assert (a["status"] != 0xFF).all()
    assert not torch.equal(a["x"], c["x"])
    # a non-finite q0 row poisons its lane (candidate 2, segment 1) and nothing else
    S = 3
    q0 = torch.tensor(H.random_configs(name, k * S, seed=3, margin=0.1), dtype=torch.float32, device=DEV)
    q0[2 * S + 1, 0] = float("nan")
    p = rb.track_paths(tgt, k, q0=q0, out=nan_out(), **kw)
    torch.cuda.synchronize()
    seg = slice(T // S, 2 * T // S)
    assert torch.isnan(p["x"][2, seg]).all() and torch.isnan(p["pos_err_m"][2, seg]).all() and (p["status"][2, seg] == 0).all()
    mask = torch.ones((k, T), dtype=torch.bool, device=DEV)
    mask[2, seg] = False
    assert torch.isfinite(p["x"][mask]).all() and (p["status"][mask] != 0xFF).all()


@pytest.mark.parametrize("which", ["panda", "fetch", "fetch_arm", "rtc"])
def test_robot_coverage(which, tmp_path, monkeypatch):
    from cppflow_amd.robot_model import canonicalize
    from cppflow_amd.robots import Robot, get_robot
    from oracle.oracle import Oracle

    if which == "rtc":
        monkeypatch.setenv("CPPF_CACHE_DIR", str(tmp_path))
        (tmp_path / "tmp").mkdir()
        monkeypatch.setenv("TMPDIR", str(tmp_path / "tmp"))
        spec = H.random_chain_spec(7, seed=31)
        rb, ch = Robot(spec), canonicalize(spec)
        assert rb.specialization() == 1000  # compiled for this description through hipRTC
        o64 = Oracle(ch, f32=False)
    else:
        rb, ch, o64 = get_robot(which), H.chain(which), H.oracle64(which)
        assert rb.specialization() >= 0
    k, T = 32, 32
    tgt = torch.tensor(_smooth_path(ch, o64, T, seed=17), dtype=torch.float32, device=DEV)
    got = rb.track_paths(tgt, k, n_segments=2, seed=4, n_random_restarts=2, **STANDIN, **TOL)
    torch.cuda.synchronize()
    st = host(got["status"]).astype(np.uint8)
    assert ((st & 1) != 0).mean() > 0.8, ((st & 1) != 0).mean()
    pe, re = rb.pose_error_metrics(got["x"].reshape(k * T, -1), tgt)
    assert np.abs(host(pe).reshape(k, T) - host(got["pos_err_m"])).max() <= 1e-6
    conv = (st & 1) != 0
    assert (host(got["pos_err_m"])[conv] < 5e-5 * 1.01).all()
    # the generic instantiation computes the same candidates as the specialised one
    rb.debug_set("force_generic", 1)
    try:
        gen = rb.track_paths(tgt, k, n_segments=2, seed=4, n_random_restarts=2, **STANDIN, **TOL)
        torch.cuda.synchronize()
    finally:
        rb.debug_set("force_generic", None)
    dq = (gen["x"] - got["x"]).abs().amax(dim=2)
    assert (dq < 1e-3).float().mean() > 0.9


SHORT = ["panda__1cube_mini", "fetch_arm__hello_mini", "fetch_arm__s__truncated"]


def test_planner_with_the_tracking_provider():
    from cppflow_amd.data_types import PlannerSettings
    from cppflow_amd.planners import CppFlowPlanner, LmIkSeedProvider, TrackingSeedProvider

    settings = PlannerSettings(k=175, tmax_sec=5.0, anytime_mode_enabled=False, do_rerun_if_large_dp_search_mjac=True, verbosity=0)
    for name in SHORT:
        problem = _fixture_problem(name)
        ref = CppFlowPlanner(settings, problem.robot, seed_provider=LmIkSeedProvider(seed=0)).generate_plan(problem)
        prov = TrackingSeedProvider(seed=0)
        res = CppFlowPlanner(settings, problem.robot, seed_provider=prov).generate_plan(problem)
        assert res.plan is not None and tuple(res.plan.q_path.shape) == (problem.n_timesteps, problem.robot.ndof)
        assert prov.n_calls >= 1 and tuple(prov.last["status"].shape) == (175 if prov.n_calls == 1 else 125, problem.n_timesteps)
        if ref.plan.is_valid:
            assert res.plan.is_valid, (name, res.plan.validity_flags())
    # initial_configuration: candidate 0 starts exactly there (a converged row of a first call, so the early-out leaves it untouched)
    problem = _fixture_problem("panda__1cube_mini")
    prov = TrackingSeedProvider(seed=1)
    first = prov(problem, 16)
    row = int(np.argmax((host(prov.last["status"][:, 0]).astype(np.uint8) & 1) != 0))
    assert (int(prov.last["status"][row, 0]) & 1) == 1
    q_init = first[row, 0].clone()
    p2 = dataclasses.replace(problem, initial_configuration=q_init[None])
    again = prov(p2, 16)
    assert torch.equal(again[0, 0], q_init)
    assert prov.n_calls == 2
    # another call draws other candidates
    assert not torch.equal(prov(problem, 16), first)


# ---- divergent lanes, bit for bit against row-shape launches ------------------------------------------------------------------------
_M32 = 0xFFFFFFFF


def _mix(h):
    """track_mix of csrc/kernels_track.h on uint64 arrays holding 32-bit values"""
    h = h & _M32
    h ^= h >> 16
    h = (h * 0x7FEB352D) & _M32
    h ^= h >> 15
    h = (h * 0x846CA68B) & _M32
    h ^= h >> 16
    return h


def _track_draw(ch, seed, call, i, s, t, attempt):
    """track_draw of csrc/kernels_track.h: [n, d] fp32 starts for candidate / segment / waypoint arrays i, s, t"""
    n = len(i)
    h = _mix(np.full(n, (seed ^ 0x5BD1E995) & _M32, dtype=np.uint64))
    for v in (np.uint64(call), np.asarray(i, np.uint64), np.asarray(s, np.uint64), np.asarray(t, np.uint64), np.uint64(attempt)):
        h = _mix(h ^ v)
    lo, hi = np.float32(ch.lo), np.float32(ch.hi)
    q = np.empty((n, ch.ndof), dtype=np.float32)
    for j in range(ch.ndof):
        hj = _mix(h ^ np.uint64(((j + 1) * 0x9E3779B9) & _M32))
        u = (hj >> np.uint64(8)).astype(np.float32) * np.float32(2.0**-24)
        q[:, j] = lo[j] + (hi[j] - lo[j]) * (np.float32(0.1) + np.float32(0.8) * u)
    return q


def _row_steps(rb, x, tgt_t, n):
    """one fused row-shape launch of n steps (what one LM block of the tracking kernel is)"""
    from cppflow_amd import _hip

    return rb.lm_pose_steps(x.contiguous(), tgt_t, STANDIN["lm_lambda"], 3.5, 0.35, n_steps=n, clamp=True, shape=_hip.SHAPE_ROW)["x"]


def test_unequal_segments_are_the_per_segment_loops_bit_for_bit():
    """T % S != 0: segments of 13, 13 and 14 waypoints, so on the last trip of the waypoint loop only every third lane is active.  No
    tolerances, no restarts, starts from q0: each segment is the chain of row-shape launches of its waypoints, bit for bit."""
    from cppflow_amd.robots import get_robot

    name, k, T, S = "panda", 64, 40, 3
    rb, ch = get_robot(name), H.chain(name)
    tgt = torch.tensor(_smooth_path(ch, H.oracle64(name), T, seed=23), dtype=torch.float32, device=DEV)
    q0 = torch.tensor(H.random_configs(name, k * S, seed=8, margin=0.1), dtype=torch.float32, device=DEV)
    got = rb.track_paths(tgt, k, n_segments=S, q0=q0, **STANDIN)
    for s in range(S):
        q = q0[s::S]
        for t in range((s * T) // S, ((s + 1) * T) // S):
            q = _row_steps(rb, q, tgt[t : t + 1], 40 if t == (s * T) // S else 6)
            assert torch.equal(got["x"][:, t], q), (s, t)
    pe, re = rb.pose_error_metrics(got["x"].reshape(k * T, -1), tgt)
    assert torch.equal(pe.reshape(k, T), got["pos_err_m"]) and torch.equal(re.reshape(k, T), got["rot_err_rad"])


def test_recovery_ladder_is_the_row_shape_attempts_bit_for_bit():
    """The ladder with a jump bar and one random restart, no tolerances: at every waypoint some lanes stop after the warm start, some
    continue it, some restart from a hashed random configuration (where the conditioning gate's fp64 re-solve fires) -- lanes leave and
    re-enter LM blocks in a data-dependent pattern.  Every stored row is, bit for bit, the row-shape launch of the attempt its status
    names (warm start n_track, continuation n_restart - n_track from it, restart n_restart from the kernel's own hashed start), and the
    ladder's rungs are taken exactly when the previous attempt jumped."""
    from cppflow_amd import _hip
    from cppflow_amd.robots import get_robot

    name, k, T, S, seed, call = "panda", 64, 40, 3, 7, 3
    rb, ch = get_robot(name), H.chain(name)
    tgt = torch.tensor(_smooth_path(ch, H.oracle64(name), T, seed=29), dtype=torch.float32, device=DEV)
    q0 = torch.tensor(H.random_configs(name, k * S, seed=9, margin=0.1), dtype=torch.float32, device=DEV)
    free = host(rb.track_paths(tgt, k, n_segments=S, q0=q0, **STANDIN)["x"])
    starts = {(s * T) // S for s in range(S)}
    steps = np.abs(np.diff(free, axis=1)).max(axis=2)[:, [t - 1 for t in range(1, T) if t not in starts]]
    bar = float(np.median(steps))  # about half of the warm starts jump by more
    got = rb.track_paths(tgt, k, n_segments=S, q0=q0, seed=seed, call_index=call, n_random_restarts=1, max_jump_rad=bar, **STANDIN)
    x, st = got["x"], host(got["status"]).astype(np.uint8)
    bar32 = np.float32(bar)

    def jumped(a, prev):
        return ~(np.abs(host(a).astype(np.float32) - host(prev).astype(np.float32)) <= bar32).all(axis=1)

    seg_of = lambda t: max(s for s in range(S) if (s * T) // S <= t)  # noqa: E731
    kinds = np.zeros((k, T), dtype=int)
    for t in range(T):
        s = seg_of(t)
        if t in starts:
            assert torch.equal(x[:, t], _row_steps(rb, q0[s::S], tgt[t : t + 1], 40)), t
            assert ((st[:, t] & _hip.TRACK_RESTARTED) != 0).all() and ((st[:, t] & _hip.TRACK_JUMP) == 0).all()
            continue
        prev = x[:, t - 1]
        a0 = _row_steps(rb, prev, tgt[t : t + 1], 6)
        a1 = _row_steps(rb, a0, tgt[t : t + 1], 34)
        start2 = _track_draw(ch, seed, call, np.arange(k), np.full(k, s), np.full(k, t), 1)
        a2 = _row_steps(rb, torch.tensor(start2, device=DEV), tgt[t : t + 1], 40)
        j = [jumped(a, prev) for a in (a0, a1, a2)]
        kind = np.where((st[:, t] & _hip.TRACK_RECOVERED) != 0, 1, np.where((st[:, t] & _hip.TRACK_RESTARTED) != 0, 2, 0))
        kinds[:, t] = kind
        for i in range(k):
            want = (a0, a1, a2)[kind[i]][i]
            assert torch.equal(x[i, t], want), (t, i, kind[i])
            assert bool(st[i, t] & _hip.TRACK_JUMP) == bool(j[kind[i]][i]), (t, i)
            if not j[0][i]:
                assert kind[i] == 0, (t, i)  # the warm start met the bar: no rung climbed
            elif not j[1][i]:
                assert kind[i] == 1, (t, i)  # the continuation met it
            elif not j[2][i]:
                assert kind[i] == 2, (t, i)  # the restart met it
    inner = [t for t in range(T) if t not in starts]
    # the ladder really diverged the lanes: at most waypoints some lanes stopped, some continued, some restarted
    mixed = sum(len(set(kinds[:, t])) == 3 for t in inner)
    assert mixed >= 3, mixed


def test_a_destroyed_handle_is_refused():
    """cppf_track_paths on a handle that cppf_robot_destroy has marked dead (kept allocated by a live batch, as in
    tests/test_gpu_round5.py): CPPF_ERR_INVALID with a message, nothing launched."""
    import ctypes
    import gc

    from cppflow_amd import _hip
    from cppflow_amd.robots import get_robot

    rb = get_robot("panda")
    x0, target = H.lm_problem("panda", 4, 64, seed=1)
    x0, target = torch.tensor(x0, dtype=torch.float32, device=DEV), torch.tensor(target, dtype=torch.float32, device=DEV)
    plan = rb.lm_batch_plan([dict(x=x0, target=target, x_out=torch.empty_like(x0))], 1e-6, 3.5, 0.35, n_steps=3)
    handle = rb._handle(torch.device(DEV))
    plan._keep[0] = None
    _hip.lib().cppf_robot_destroy(handle)
    rb._handles = {}
    del rb
    gc.collect()
    k, T = 4, 8
    outs = [torch.full((k, T, 7), 5.0, device=DEV), torch.full((k, T), 5.0, device=DEV), torch.full((k, T), 5.0, device=DEV),
            torch.full((k, T), 7, dtype=torch.uint8, device=DEV)]  # fmt: skip
    prm = _hip.TrackParams(1e-2, 3.5, 0.35, 40, 6, 0, 0.0, 0.0, 0.0, 0.0, 0, 0)
    rc = _hip.lib().cppf_track_paths(handle, target.data_ptr(), T, k, 1, ctypes.byref(prm), None, *[o.data_ptr() for o in outs], None)
    assert rc == _hip.CPPF_ERR_INVALID and "destroyed" in _hip.lib().cppf_last_error().decode()
    torch.cuda.synchronize()
    assert (outs[0] == 5.0).all() and (outs[3] == 7).all()  # nothing was launched
    del plan
    gc.collect()
