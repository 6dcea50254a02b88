"""cppf_dp_nbest (the N lowest-cost dp_search paths that are different from each other, csrc/kernels_dp.h) at the C ABI: the two
prototypes, the argument checks -- all of which come before a device is touched, so a host-only handle serves -- and the NumPy
restatement of its definition that tests/test_gpu_dp_nbest.py holds the device against.  No GPU."""

import ctypes

import numpy as np
import pytest

from tests.test_abi import declared_functions

K_TIMED_OUT = 0x40000000  # the resident search's flag bit in memoT[0] (csrc/kernels_dp.h: kDpTimedOut)


# ---- the definition, restated (fp64) -----------------------------------------------------------------------------------------------
def trace_all(memoT):
    """idx [k,T]: idx[j,T-1] = j, idx[j,t-1] = memoT[t, idx[j,t]] -- dp_search's back-trace from EVERY terminal"""
    T, k = memoT.shape
    idx = np.zeros((k, T), dtype=np.int64)
    cur = np.arange(k)
    for t in range(T - 1, -1, -1):
        idx[:, t] = cur
        if t > 0:
            cur = memoT[t, cur].astype(np.int64)
    return idx


def terminal_order(costsT):
    """terminals by (cost, index) ascending; a cost that is not below +inf counts as +inf (dp_search's scan `c < best` never
    prefers such a terminal to an earlier one either), so order[0] is the terminal dp_search picks"""
    last = np.asarray(costsT[-1], dtype=np.float64)
    c = np.where(last < np.inf, last, np.inf)
    return np.lexsort((np.arange(c.size), c))


def traced_paths(q, idx):
    return np.asarray(q, dtype=np.float64)[idx, np.arange(idx.shape[1])]  # [k,T,d]


def sep_to_all(paths, a, scale):
    """sep(a, j) for every j: max over t and joints of |wrap(s (path_j - path_a))|"""
    dq = (paths - paths[a]) * scale
    return np.abs(np.remainder(dq + np.pi, 2 * np.pi) - np.pi).max(axis=(1, 2))


def nbest_greedy(q, costsT, memoT, n_paths, min_sep, scale):
    """the definition: trace all, order, accept a terminal when it is >= min_sep away from every path accepted before it.
    -> (terminals accepted, idx [k,T]); None for tables that carry the timed-out flag"""
    if int(memoT[0, 0]) & K_TIMED_OUT:
        return None, None
    idx = trace_all(memoT)
    paths = traced_paths(q, idx)
    accepted, seps = [], []  # seps[i] = sep(accepted[i], .) to every terminal
    for j in terminal_order(costsT):
        if len(accepted) == n_paths:
            break
        if all(s[j] >= min_sep for s in seps):
            accepted.append(int(j))
            # (a separation is >= 0 whatever it is: with min_sep = 0 no compare can fail and none needs the number)
            seps.append(sep_to_all(paths, j, scale) if min_sep > 0 else np.zeros(len(paths)))
    return accepted, idx


def nbest_rounds(q, costsT, memoT, n_paths, min_sep, scale):
    """the round form the kernel runs: accept the first terminal alive, kill every terminal closer than min_sep to it"""
    if int(memoT[0, 0]) & K_TIMED_OUT:
        return None, None
    idx = trace_all(memoT)
    paths = traced_paths(q, idx)
    order = terminal_order(costsT)
    alive = np.ones(len(order), dtype=bool)
    accepted = []
    for _ in range(n_paths):
        live = [j for j in order if alive[j]]
        if not live:
            break
        a = int(live[0])
        accepted.append(a)
        alive[a] = False
        if min_sep > 0:
            alive &= sep_to_all(paths, a, scale) >= min_sep
    return accepted, idx


def nbest_outputs(q, costsT, accepted, idx, n_paths):
    """(paths [N,T,d] f32, path_idx [N,T] i32, path_cost [N] f32, n_found) as the entry point documents them"""
    k, T, d = q.shape
    paths = np.full((n_paths, T, d), np.nan, dtype=np.float32)
    pidx = np.full((n_paths, T), -1, dtype=np.int32)
    cost = np.full(n_paths, np.inf, dtype=np.float32)
    if accepted is None:
        return paths, pidx, cost, -1
    for s, a in enumerate(accepted):
        pidx[s] = idx[a]
        paths[s] = q[idx[a], np.arange(T)]
        cost[s] = costsT[-1, a]
    return paths, pidx, cost, len(accepted)


def joint_scale(name, prismatic_scaling=5.0):
    from tests import helpers as H

    return np.where(np.asarray(H.chain(name).jtype) == 1, prismatic_scaling, 1.0)


def dp_tables(q, ext, scale):
    """costsT / memoT [T,k] by the recurrence of tests/test_host_logic.py (cppflow/search.py:55-97), prismatic joints scaled"""
    k, T, _ = q.shape
    costs = np.zeros((T, k))
    memo = np.zeros((T, k), dtype=np.int32)
    costs[0] = ext[:, 0]
    for t in range(1, T):
        for b in range(k):
            dq = np.abs(np.remainder((q[b, t] - q[:, t - 1]) * scale + np.pi, 2 * np.pi) - np.pi).max(axis=1)
            c = np.maximum(dq, costs[t - 1]) + ext[b, t]
            memo[t, b] = int(np.argmin(c))
            costs[t, b] = c[memo[t, b]]
    return costs, memo


# ---- the tests ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from cppflow_amd import _hip, build

    build.build()
    return _hip.lib()


def test_entry_points_are_declared_bound_and_exported(lib):
    from cppflow_amd import _hip

    for fn in ("cppf_dp_nbest", "cppf_dp_nbest_workspace_bytes"):
        assert fn in declared_functions() and fn in _hip.SIGNATURES and getattr(lib, fn) is not None
    res, args = _hip.SIGNATURES["cppf_dp_nbest"]
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert res is ci and args == [vp, vp, vp, vp, ci, ci, ci, cf, cf, vp, vp, vp, vp, vp, vp]
    res, args = _hip.SIGNATURES["cppf_dp_nbest_workspace_bytes"]
    assert res is ci and args == [ci, ci, ci, ctypes.POINTER(ctypes.c_size_t)]
    assert lib.cppf_abi_version() == 6  # additive: the ABI version stays


def _call(lib, h, **kw):
    buf = ctypes.c_void_p(0x1000)  # never dereferenced: every call here is refused before any launch
    a = dict(q=buf, costsT=buf, memoT=buf, k=5, T=4, n_paths=2, min_sep=0.5, scale=5.0, workspace=buf, paths=buf, path_idx=buf,
             path_cost=buf, n_found=buf)  # fmt: skip
    a.update(kw)
    return lib.cppf_dp_nbest(h, a["q"], a["costsT"], a["memoT"], a["k"], a["T"], a["n_paths"], a["min_sep"], a["scale"],
                             a["workspace"], a["paths"], a["path_idx"], a["path_cost"], a["n_found"], None)  # fmt: skip


def test_bad_arguments_are_refused_before_the_device_is_selected(lib):
    from cppflow_amd import _hip
    from cppflow_amd.robot_model import canonicalize
    from cppflow_amd.robot_zoo import ROBOT_SPECS

    assert _call(lib, None) == _hip.CPPF_ERR_INVALID and "NULL" in lib.cppf_last_error().decode()
    desc = _hip.chain_to_desc(canonicalize(ROBOT_SPECS["panda"]()))
    h = ctypes.c_void_p()
    assert lib.cppf_robot_create(ctypes.byref(desc), -12345, ctypes.byref(h)) == _hip.CPPF_OK, lib.cppf_last_error().decode()
    try:
        cases = [(dict(**{name: None}), "NULL") for name in ("q", "costsT", "memoT", "workspace", "paths", "path_idx", "path_cost", "n_found")]
        cases += [
            (dict(k=0), "k, T, n_paths"),
            (dict(T=0), "k, T, n_paths"),
            (dict(n_paths=0), "k, T, n_paths"),
            (dict(k=-3), "k, T, n_paths"),
            (dict(min_sep=-0.25), "min_separation"),
            (dict(min_sep=float("nan")), "min_separation"),
            (dict(min_sep=float("inf")), "min_separation"),
            (dict(workspace=ctypes.c_void_p(0x1004)), "aligned"),
            (dict(k=1 << 20, T=1 << 9), "k*T*d"),  # 2^29 * 7 joints
        ]
        for kw, word in cases:
            assert _call(lib, h, **kw) == _hip.CPPF_ERR_INVALID, kw
            assert word in lib.cppf_last_error().decode(), (kw, lib.cppf_last_error().decode())
        # (a destroyed handle: tests/test_gpu_dp_nbest.py, through a handle a live batch keeps allocated)
    finally:
        lib.cppf_robot_destroy(h)


def test_workspace_bytes_is_monotone_and_rejects_non_positive_sizes(lib):
    from cppflow_amd import _hip

    def nbytes(k, T, n):
        out = ctypes.c_size_t(0)
        assert lib.cppf_dp_nbest_workspace_bytes(k, T, n, ctypes.byref(out)) == _hip.CPPF_OK
        return out.value

    for n in (1, 4, 303):
        prev = 0
        for k in (1, 3, 64, 65, 175, 257, 300, 1024):
            assert nbytes(k, 256, n) >= prev
            prev = nbytes(k, 256, n)
        prev = 0
        for T in (1, 2, 5, 256, 1000):
            assert nbytes(300, T, n) >= prev
            prev = nbytes(300, T, n)
    assert nbytes(300, 256, 4) >= 4 * 300 * 256 and nbytes(300, 256, 4) % 16 == 0  # the traced indices of every terminal, at least
    out = ctypes.c_size_t(0)
    for k, T, n in ((0, 4, 1), (4, 0, 1), (4, 4, 0), (-1, 4, 1)):
        assert lib.cppf_dp_nbest_workspace_bytes(k, T, n, ctypes.byref(out)) == _hip.CPPF_ERR_INVALID, (k, T, n)
        assert lib.cppf_last_error().decode()
    assert lib.cppf_dp_nbest_workspace_bytes(4, 4, 1, None) == _hip.CPPF_ERR_INVALID


def test_restatement_reproduces_the_oracles_best_path_in_slot_0():
    from tests import helpers as H

    rng = np.random.RandomState(0)
    k, T = 9, 14
    for name, d in (("panda", 7), ("fetch", 8)):
        q = rng.uniform(-1, 1, size=(k, T, d)).astype(np.float32)
        ext = ((rng.rand(k, T) < 0.2) * 1000 + (rng.rand(k, T) < 0.2) * 100).astype(np.float32)
        scale = joint_scale(name)
        costsT, memoT = dp_tables(q.astype(np.float64), ext, scale)
        want_idx, want_costs = H.oracle64(name).dp_search(q, ext)
        np.testing.assert_allclose(costsT, want_costs.T, rtol=0, atol=1e-12)
        for form in (nbest_greedy, nbest_rounds):
            for n_paths, min_sep in ((1, 0.5), (4, 0.0), (4, 0.5), (k + 3, 0.0)):
                acc, idx = form(q, costsT, memoT, n_paths, min_sep, scale)
                paths, pidx, cost, n = nbest_outputs(q, costsT, acc, idx, n_paths)
                assert n >= 1 and (pidx[0] == want_idx).all() and (paths[0] == q[want_idx, np.arange(T)]).all()
                assert cost[0] == np.float32(want_costs[want_idx[-1], -1])
                if min_sep == 0.0:
                    assert n == min(n_paths, k)
                assert np.isnan(paths[n:]).all() and (pidx[n:] == -1).all() and np.isinf(cost[n:]).all()
    # the flag bit is not an index
    memo_flag = memoT.copy()
    memo_flag[0, 0] |= K_TIMED_OUT
    assert nbest_greedy(q, costsT, memo_flag, 2, 0.5, scale) == (None, None)
    assert nbest_outputs(q, costsT, None, None, 2)[3] == -1


def test_greedy_and_round_forms_agree_on_random_small_instances():
    """50 random tables (random back-pointers, so that traces merge at random depths; costs with ties, +inf and NaN among them) and
    candidates drawn from a few clusters so that both outcomes of the separation test occur"""
    rng = np.random.RandomState(1)
    n_killed = n_multi = 0
    for trial in range(50):
        k, T, d = rng.randint(1, 13), rng.randint(1, 9), rng.randint(1, 5)
        centres = rng.uniform(-3, 3, size=(rng.randint(1, 4), 1, d))
        q = (centres[rng.randint(0, len(centres), size=k)] + 0.1 * rng.randn(k, T, d)).astype(np.float32)
        memoT = rng.randint(0, k, size=(T, k)).astype(np.int32)
        costsT = rng.randint(0, 4, size=(T, k)).astype(np.float64)
        costsT[-1, rng.rand(k) < 0.1] = np.inf
        costsT[-1, rng.rand(k) < 0.05] = np.nan
        scale = np.where(rng.rand(d) < 0.3, 5.0, 1.0)
        for n_paths in (1, 3, k + 3):
            for min_sep in (0.0, 0.3, 1.0):
                g, _ = nbest_greedy(q, costsT, memoT, n_paths, min_sep, scale)
                r, _ = nbest_rounds(q, costsT, memoT, n_paths, min_sep, scale)
                assert g == r, (trial, n_paths, min_sep, g, r)
                assert len(set(g)) == len(g) and 1 <= len(g) <= min(n_paths, k)
                n_multi += len(g) > 1
                n_killed += min_sep > 0 and n_paths > k and len(g) < k
    assert n_killed > 10 and n_multi > 50  # the instances exercise both the kill and the keep
