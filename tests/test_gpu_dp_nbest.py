"""cppf_dp_nbest on the MI355X: the N lowest-cost dp_search paths that are different from each other, out of the tables a finished
search has left (csrc/kernels_dp.h), and the planner that optimises them together.

  * Bit for bit against the NumPy restatement of the definition (tests/test_dp_nbest_abi.py), fed the DEVICE's own cost / memo tables
    (which tests/test_gpu_round2.py pins to the oracle bit for bit).  The kernel compares fp32 maxima with the threshold, the
    restatement fp64 ones: every case first asserts that no pairwise separation of two traced paths lies within 1e-4 rad of the
    threshold -- outside that band the two decisions cannot differ (an fp32 difference of two joint values below 16 rad, scaled by 5
    and wrapped, is within 1e-5 of the exact one).  With a threshold of 0 every compare is `x >= 0`: no band is needed.
  * Inputs: C clusters of candidates -- one common random walk, per cluster an offset of >= 2 rad (wrapped, after the prismatic
    scale) in one of two joints at every waypoint plus a small walk of its own, per candidate 0.01 rad of noise -- so that the
    traces of a cluster merge or stay within a few hundredths of a radian, and clusters stay apart.  Fetch's second offset joint is
    its prismatic one (0.45 m: 2.25 after the scale, 0.45 -- below the threshold -- without it).  Penalties of 100 / 1000 are
    sprinkled over random nodes of the candidates beyond the first of each cluster, so that a cluster never has to be left.
  * Shapes: every k in {1, 3, 64, 65, 175, 257, 300} x T in {1, 2, 5, 256} x N in {1, 4, k+3} x threshold in {0, 0.5} for both
    robots; C in {1, 3, 5} rotates over the (robot, k, T) grid (each k and each T meets each C)."""

import ctypes
import functools
import gc
import os

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import test_dp_nbest_abi as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REF = os.path.join(GOLDEN, "reference_files")
KS, TS, CS = (1, 3, 64, 65, 175, 257, 300), (1, 2, 5, 256), (1, 3, 5)
ROBOTS = ("panda", "fetch")
MIN_SEPS = (0.0, 0.5)
BAND = 1e-4


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def clusters_for(name, k, T):
    return CS[(KS.index(k) + TS.index(T) + ROBOTS.index(name)) % 3]


def cluster_candidates(name, k, T, C, seed):
    """(q [k,T,d] f32, ext [k,T] f32, cluster [k]) as the module docstring describes them"""
    ch = H.chain(name)
    d = ch.ndof
    rng = np.random.RandomState(seed)
    pris = [j for j in range(d) if ch.jtype[j] == 1]
    j1 = [j for j in range(d) if ch.jtype[j] == 0][1]  # a revolute joint: offsets -2, 0, 2
    j2 = pris[0] if pris else [j for j in range(d) if ch.jtype[j] == 0][2]  # offsets 0 / 2 rad, or 0 / 0.45 m on a prismatic joint
    step = np.where(np.asarray(ch.jtype) == 1, 0.004, 0.02)
    common = np.cumsum(rng.uniform(-1, 1, size=(T, d)) * step, axis=0)
    base = np.zeros((C, T, d))
    for c in range(C):
        own = np.cumsum(rng.uniform(-1, 1, size=(T, d)) * step * 0.25, axis=0)
        own[:, [j1, j2]] = 0.0
        base[c] = common + own
        base[c, :, j1] += 2.0 * (c % 3) - 2.0
        base[c, :, j2] += (0.45 if pris else 2.0) * (c // 3)
    cluster = np.arange(k) % C
    noise = np.where(np.asarray(ch.jtype) == 1, 0.002, 0.01)
    q = (base[cluster] + rng.uniform(-1, 1, size=(k, T, d)) * noise).astype(np.float32)
    ext = ((rng.rand(k, T) < 0.02) * 1000 + (rng.rand(k, T) < 0.03) * 100).astype(np.float32)
    ext[:C] = 0.0
    return q, ext, cluster


@pytest.fixture(scope="module")
def robots():
    from cppflow_amd.robots import get_robot

    return {name: get_robot(name) for name in ROBOTS}


_cache = {}


def searched(robots, name, k, T):
    """one search per (robot, k, T), shared by the tests and left unchanged: inputs, the device's tables, the traced paths' pairwise
    separations (fp64, on the device) and the cluster of every candidate"""
    key = (name, k, T)
    if key not in _cache:
        C = clusters_for(name, k, T)
        q, ext, cluster = cluster_candidates(name, k, T, C, seed=1000 * KS.index(k) + 10 * TS.index(T) + ROBOTS.index(name))
        qd, ed = dev(q), dev(ext)
        best_path, best_idx, costsT, memoT, ran = robots[name].dp_search(qd, ed, return_memo=True, return_method=True)
        assert int(best_idx[0]) >= 0, "the resident search timed out"
        idx = R.trace_all(host(memoT))
        paths = torch.tensor(R.traced_paths(q, idx), dtype=torch.float64, device=DEV)  # [k,T,d]
        scale = torch.tensor(R.joint_scale(name), dtype=torch.float64, device=DEV)
        seps = torch.empty((k, k), dtype=torch.float64, device=DEV)
        for a in range(k):
            dq = (paths - paths[a]) * scale
            seps[a] = (torch.remainder(dq + np.pi, 2 * np.pi) - np.pi).abs().amax(dim=(1, 2))
        _cache[key] = dict(q=q, ext=ext, cluster=cluster, C=C, qd=qd, ed=ed, best_path=best_path, best_idx=best_idx, costsT=costsT,
                           memoT=memoT, costs_h=host(costsT), memo_h=host(memoT), seps=host(seps), ran=ran)  # fmt: skip
    return _cache[key]


def check_against_restatement(name, s, n_paths, min_sep, got):
    paths, path_idx, path_cost, n_found = (host(t) for t in got)
    if min_sep > 0:  # a condition on the INPUTS: no decision of the kernel hangs on fp32 rounding
        off = s["seps"][~np.eye(len(s["seps"]), dtype=bool)]
        assert off.size == 0 or np.abs(off - min_sep).min() > BAND, np.abs(off - min_sep).min()
    acc, idx = R.nbest_greedy(s["q"], s["costs_h"], s["memo_h"], n_paths, min_sep, R.joint_scale(name))
    want_paths, want_idx, want_cost, want_n = R.nbest_outputs(s["q"], s["costs_h"], acc, idx, n_paths)
    assert int(n_found[0]) == want_n, (int(n_found[0]), want_n)
    assert np.array_equal(path_idx, want_idx)
    assert np.array_equal(path_cost.view(np.uint32), want_cost.view(np.uint32))
    assert np.array_equal(paths.view(np.uint32)[:want_n], want_paths.view(np.uint32)[:want_n])
    # paths = the gather of q by path_idx; the empty slots hold NaN, -1 and +inf
    T = s["q"].shape[1]
    for i in range(want_n):
        assert np.array_equal(paths[i], s["q"][path_idx[i], np.arange(T)])
    assert np.isnan(paths[want_n:]).all() and (path_idx[want_n:] == -1).all() and np.isposinf(path_cost[want_n:]).all()
    return acc


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", ROBOTS)
def test_selection_is_the_restatement_bit_for_bit_and_diverse(robots, name, k, T):
    rb, s = robots[name], searched(robots, name, k, T)
    C_present = min(s["C"], k)
    for n_paths in (1, 4, k + 3):
        for min_sep in MIN_SEPS:
            got = rb.dp_nbest(s["qd"], s["costsT"], s["memoT"], n_paths, min_sep)
            acc = check_against_restatement(name, s, n_paths, min_sep, got)
            # slot 0 is the search's own result
            assert torch.equal(got[0][0], s["best_path"]) and torch.equal(got[1][0], s["best_idx"])
            if min_sep == 0.0:
                assert len(acc) == min(n_paths, k)
            elif n_paths >= s["C"]:  # one path per cluster, no more
                assert len(acc) == C_present, (len(acc), C_present)
                assert len({int(s["cluster"][a]) for a in acc}) == C_present
    # the tables and the candidates were only read
    assert np.array_equal(host(s["costsT"]).view(np.uint32), s["costs_h"].view(np.uint32)) and np.array_equal(host(s["memoT"]), s["memo_h"])
    assert np.array_equal(host(s["qd"]), s["q"])


@pytest.mark.parametrize("name,k,T", [("panda", 175, 256), ("fetch", 64, 5), ("panda", 300, 5), ("fetch", 257, 2), ("panda", 3, 256)])
def test_slot_0_is_the_search_result_for_every_search_form(robots, name, k, T):
    rb, s = robots[name], searched(robots, name, k, T)
    for method in ("resident", "launches") + (("table",) if k <= 256 else ()):
        best_path, best_idx, costsT, memoT = rb.dp_search(s["qd"], s["ed"], method=method, return_memo=True)
        assert int(best_idx[0]) >= 0
        paths, path_idx, path_cost, n_found = rb.dp_nbest(s["qd"], costsT, memoT, 4, 0.5)
        assert int(n_found[0]) >= 1, method
        assert torch.equal(paths[0], best_path) and torch.equal(path_idx[0], best_idx), method
        assert float(path_cost[0]) == float(costsT[T - 1, int(best_idx[T - 1])])
        assert torch.equal(path_idx, rb.dp_nbest(s["qd"], s["costsT"], s["memoT"], 4, 0.5)[1]), method  # the forms leave the same tables


@pytest.mark.parametrize("name,k,T", [("panda", 175, 256), ("fetch", 300, 5)])
def test_timed_out_tables_give_no_paths(robots, name, k, T):
    """the resident search's flag bit set BY HAND in a copy of memoT[0] (no timeout is provoked): n_found = -1, every slot empty; the same
    copy without the bit gives the normal result"""
    rb, s = robots[name], searched(robots, name, k, T)
    memo = s["memoT"].clone()
    memo[0, 0] |= R.K_TIMED_OUT
    for n_paths, min_sep in ((1, 0.0), (4, 0.5), (k + 3, 0.5)):
        paths, path_idx, path_cost, n_found = rb.dp_nbest(s["qd"], s["costsT"], memo, n_paths, min_sep)
        assert int(n_found[0]) == -1
        assert bool(torch.isnan(paths).all()) and bool((path_idx == -1).all()) and bool(torch.isposinf(path_cost).all())
        check_against_restatement(name, dict(s, memo_h=host(memo)), n_paths, min_sep, (paths, path_idx, path_cost, n_found))
    memo[0, 0] &= ~R.K_TIMED_OUT
    check_against_restatement(name, s, 4, 0.5, rb.dp_nbest(s["qd"], s["costsT"], memo, 4, 0.5))


@pytest.mark.parametrize("name,k,T,n_paths", [("panda", 65, 5, 4), ("fetch", 175, 256, 4), ("panda", 300, 5, 303), ("fetch", 3, 2, 6)])
def test_memory_discipline(robots, name, k, T, n_paths):
    """outputs and workspace carved out of one poisoned arena with guard gaps: the gaps are intact afterwards, the inputs unchanged byte
    for byte, two runs give identical bytes (whatever the workspace held before), and a non-default stream gives the same result"""
    from cppflow_amd import _hip

    rb, s = robots[name], searched(robots, name, k, T)
    d = rb.ndof
    lib = _hip.lib()
    nbytes = ctypes.c_size_t(0)
    _hip.check(lib.cppf_dp_nbest_workspace_bytes(k, T, n_paths, ctypes.byref(nbytes)))
    inputs = [s["qd"], s["costsT"], s["memoT"]]
    before = [t.clone() for t in inputs]
    results = []
    for poison, stream in ((0xA5, None), (0x5A, None), (0xA5, torch.cuda.Stream(device=DEV))):
        arena = torch.full((8 << 20,), poison, dtype=torch.uint8, device=DEV)
        cursor, spans, bufs = 4096, [], {}
        for nm, nb in (("workspace", nbytes.value), ("paths", n_paths * T * d * 4), ("path_idx", n_paths * T * 4),
                       ("path_cost", n_paths * 4), ("n_found", 4)):  # fmt: skip
            start = (cursor + 255) // 256 * 256
            bufs[nm] = arena[start : start + nb]
            spans.append((start, start + nb))
            cursor = start + nb + 1024
        assert cursor + 4096 < arena.numel()
        torch.cuda.synchronize()
        st = (stream if stream is not None else torch.cuda.current_stream(DEV)).cuda_stream
        _hip.check(lib.cppf_dp_nbest(rb._handle(torch.device(DEV)), s["qd"].data_ptr(), s["costsT"].data_ptr(), s["memoT"].data_ptr(),
                                     k, T, n_paths, 0.5, 5.0, bufs["workspace"].data_ptr(), bufs["paths"].data_ptr(),
                                     bufs["path_idx"].data_ptr(), bufs["path_cost"].data_ptr(), bufs["n_found"].data_ptr(), st))  # fmt: skip
        torch.cuda.synchronize()
        mask = torch.ones(cursor + 4096, dtype=torch.bool, device=DEV)
        for a, b in spans:
            mask[a:b] = False
        assert bool((arena[: cursor + 4096][mask] == poison).all()), "a guard gap was written"
        results.append({nm: host(bufs[nm]).copy() for nm in ("paths", "path_idx", "path_cost", "n_found")})
        for t, b in zip(inputs, before):
            assert torch.equal(t.view(torch.int32), b.view(torch.int32))
    for r in results[1:]:
        for nm, v in r.items():
            assert np.array_equal(v, results[0][nm]), nm
    r0 = results[0]
    got = (torch.tensor(r0["paths"]).view(torch.float32).view(n_paths, T, d), torch.tensor(r0["path_idx"]).view(torch.int32).view(n_paths, T),
           torch.tensor(r0["path_cost"]).view(torch.float32), torch.tensor(r0["n_found"]).view(torch.int32))  # fmt: skip
    check_against_restatement(name, s, n_paths, 0.5, got)


def test_a_destroyed_handle_is_refused():
    """cppf_dp_nbest on a handle that cppf_robot_destroy has marked dead (kept allocated by a live batch, as in
    tests/test_gpu_track_paths.py): CPPF_ERR_INVALID with a message, nothing launched."""
    from cppflow_amd import _hip
    from cppflow_amd.robots import Robot
    from cppflow_amd.robot_zoo import ROBOT_SPECS

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
    k, T, N = 4, 8, 2
    f = lambda *shape: torch.full(shape, 5.0, device=DEV)  # noqa: E731
    i = lambda *shape: torch.full(shape, 7, dtype=torch.int32, device=DEV)  # noqa: E731
    q, costsT, memoT, ws, paths, pidx, pcost, nf = f(k, T, 7), f(T, k), i(T, k), i(1024), f(N, T, 7), i(N, T), f(N), i(1)
    rc = _hip.lib().cppf_dp_nbest(handle, q.data_ptr(), costsT.data_ptr(), memoT.data_ptr(), k, T, N, 0.5, 5.0, ws.data_ptr(),
                                  paths.data_ptr(), pidx.data_ptr(), pcost.data_ptr(), nf.data_ptr(), None)  # fmt: skip
    assert rc == _hip.CPPF_ERR_INVALID and "destroyed" in _hip.lib().cppf_last_error().decode()
    torch.cuda.synchronize()
    assert (paths == 5.0).all() and (pidx == 7).all() and (nf == 7).all()  # nothing was launched
    del plan
    gc.collect()


# ---- the planner ---------------------------------------------------------------------------------------------------------------------
PLANNER_PROBLEMS = ["panda__1cube_mini", "fetch_arm__hello_mini"]


@functools.lru_cache(maxsize=None)
def _fixture_problem(name):
    from cppflow_amd.data_type_utils import problem_from_filename

    return problem_from_filename(None, name, problems_dir=os.path.join(REF, "problems"), paths_dir=os.path.join(REF, "paths"), device=DEV)


def _planner(problem, **kw):
    from cppflow_amd.data_types import PlannerSettings
    from cppflow_amd.planners import CppFlowPlanner, TrackingSeedProvider

    settings = PlannerSettings(k=64, tmax_sec=60.0, anytime_mode_enabled=False, do_rerun_if_large_dp_search_mjac=False,
                               do_rerun_if_optimization_fails=False, verbosity=0)  # fmt: skip
    return CppFlowPlanner(settings, problem.robot, seed_provider=TrackingSeedProvider(seed=3), **kw)


@pytest.mark.parametrize("name", PLANNER_PROBLEMS)
def test_planner_with_one_search_path_is_the_planner_without_the_argument(name):
    problem = _fixture_problem(name)
    for device_optimizer in (True, False):
        want = _planner(problem, device_optimizer=device_optimizer).generate_plan(problem)
        got = _planner(problem, device_optimizer=device_optimizer, n_search_paths=1).generate_plan(problem)
        assert torch.equal(got.plan.q_path, want.plan.q_path)
        assert "n_search_paths" not in got.debug_info and got.plan.is_valid == want.plan.is_valid


@pytest.mark.parametrize("device_optimizer", [True, False])
@pytest.mark.parametrize("name", PLANNER_PROBLEMS)
def test_planner_optimises_the_search_paths_together(name, device_optimizer):
    """n_search_paths = 4: the plan is slice `optimized_path_index` of a direct run_lm_optimization over dp_search_nbest's paths for
    the same candidates (device loop: every trajectory on its own record; host loop: one shared decision), bit for bit"""
    from cppflow_amd.collision_detection import qpaths_batched_collisions
    from cppflow_amd.optimization import run_lm_optimization
    from cppflow_amd.planners import TrackingSeedProvider
    from cppflow_amd.search import dp_search, dp_search_nbest

    problem = _fixture_problem(name)
    assert problem.initial_configuration is None
    T = problem.n_timesteps
    res = _planner(problem, device_optimizer=device_optimizer, n_search_paths=4).generate_plan(problem)
    n, s = res.debug_info["n_search_paths"], res.debug_info["optimized_path_index"]
    assert 1 <= n <= 4 and 0 <= s < n and "n_optimization_steps" in res.debug_info
    # the same candidates, searched and optimised by hand
    qs = TrackingSeedProvider(seed=3)(problem, 64)
    self_viol, env_viol = qpaths_batched_collisions(problem, qs.contiguous())
    paths, path_cost, path_idx = dp_search_nbest(problem.robot, qs.contiguous(), self_viol, env_viol, 4, 0.5)
    assert paths.shape[0] == n and path_cost.shape == (n,) and path_idx.shape == (n, T)
    assert torch.equal(paths[0], dp_search(problem.robot, qs.contiguous(), self_viol, env_viol))
    assert bool((path_cost[1:] >= path_cost[:-1]).all())
    opt = run_lm_optimization(problem, paths.reshape(n * T, -1).contiguous(), tmax_sec=60.0, max_n_steps=20, return_if_valid_after_n_steps=0,
                              convergence_threshold=1e6, verbosity=0, parallel_count=n, per_trajectory=device_optimizer,
                              device_loop=device_optimizer)  # fmt: skip
    want_s = opt.parallel_seed_idx if 0 <= opt.parallel_seed_idx < n else 0
    assert s == want_s
    assert torch.equal(res.plan.q_path, opt.x_opt.detach()[s * T : (s + 1) * T])
    assert res.plan.is_valid == opt.is_valid
    assert res.debug_info["n_optimization_steps"] == opt.n_steps_taken


def test_more_than_one_search_path_needs_one_rank(monkeypatch):
    import torch.distributed as dist

    problem = _fixture_problem("panda__1cube_mini")
    planner = _planner(problem, n_search_paths=2)
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(AssertionError, match="more than one rank"):
        planner._run_pipeline(problem)
    with pytest.raises(AssertionError):
        _planner(problem, n_search_paths=0)
