"""Pinned end waypoints of the coupled LM step (cppf_lm_full_step_pinned: CPPF_PIN_FIRST / CPPF_PIN_LAST), on the MI355X.

A pinned end is a smaller free problem whose boundary term is a virtual-config row: with n_virtual_configs = 1,
alpha_virtual_configs = 1 and alpha_differencing_prismatic_scaling = 1 (the preset's value) the row beta wrap(x_t - xv_t),
beta = alpha_differencing, IS the differencing row to a fixed neighbour xv_t.  So the fp64 oracle -- untouched -- serves on the
reduced path:
    PIN_FIRST | PIN_LAST, virtual configs off on the device  ==  oracle(x[1:W-1], target[1:W-1], n_vq = 1, xv = [x_0 .. x_{W-1}])
    PIN_FIRST, n_vq = 1 and xv = NULL on the device          ==  oracle(x[1:], n_vq = 1, xv = [x_0 .. x_{W-1}]): the last waypoint's
                                                                 zero-residual row adds beta^2 on both sides
    PIN_LAST                                                 ==  the mirror image
Tolerance: the project's own for this step against this oracle, 2e-4 + 2e-3 step in joint space (tests/test_gpu_api.py:426), the
task-space form of :410-419 with the pose block."""

import ctypes

import numpy as np
import pytest
import torch

from cppflow_amd import _hip
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIRST, LAST = _hip.PIN_FIRST, _hip.PIN_LAST
SENTINEL = 0x7FC0BEEF


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def robots():
    from cppflow_amd.robots import get_robot

    return {n: get_robot(n) for n in ("panda", "fetch", "chain12")}


def _params(**kw):
    from cppflow_amd.lm_hyper_parameters import ALT_LOSS_V2_1_DIFF, OptimizationParameters

    d = dict(ALT_LOSS_V2_1_DIFF.__dict__)
    d.update(kw)
    pm = OptimizationParameters(**d)
    pm.virtual_configs = torch.tensor([])
    return pm


def _with(rb, switches, fn):
    try:
        for k, v in switches.items():
            rb.debug_set(k, v)
        return fn()
    finally:
        for k in switches:
            rb.debug_set(k, None)


def pinned_rows(pin, S, T):
    rows = ([s * T for s in range(S)] if pin & FIRST else []) + ([s * T + T - 1 for s in range(S)] if pin & LAST else [])
    return sorted(set(rows))


def pin_params(pin, **kw):
    """device parameters of the reduced-problem identity (module docstring) for this mask, and the oracle's"""
    assert _params().alpha_differencing_prismatic_scaling == 1.0  # the identity needs beta = alpha_differencing on every joint
    vq = dict(use_virtual_configs=True, n_virtual_configs=1, alpha_virtual_configs=1.0)
    device = _params(use_virtual_configs=False, **kw) if pin == (FIRST | LAST) else _params(**vq, **kw)
    return device, _params(**vq, **kw)


def reduced_oracle(o, x, target, pm_oracle, S, T, pin, lo, hi, banded=False):
    """the oracle's step on the free waypoints, the pinned ones held by virtual-config rows; returned on the full path (pinned
    rows = x)"""
    a, b = (1 if pin & FIRST else 0), (T - 1 if pin & LAST else T)
    x3 = x.reshape(S, T, -1)
    xr = np.ascontiguousarray(x3[:, a:b]).reshape(S * (b - a), -1)
    xv3 = x3[:, a:b].copy()  # a waypoint that is its own virtual twin: zero residual, beta^2 on the diagonal
    if pin & FIRST:
        xv3[:, 0] = x3[:, 0]
    if pin & LAST:
        xv3[:, -1] = x3[:, T - 1]
    want_r = o.lm_full_step(xr, np.ascontiguousarray(target[a:b]), pm_oracle, S, b - a, virtual_configs=xv3.reshape(xr.shape),
                            boxes_lo=lo, boxes_hi=hi, banded=banded)  # fmt: skip
    want = x3.copy()
    want[:, a:b] = want_r.reshape(S, b - a, -1)
    return want.reshape(S * T, -1)


_cases = {}


def coupled_case(name, S, T, pinned_collides=False, seed=7):
    """trajectories like test_coupled_lm_step_matches_dense_reference_order_oracle: S small perturbations of one smooth path that
    starts next to a colliding configuration (active collision rows); `pinned_collides`: waypoint 0 of trajectory 0 IS that
    configuration, exactly"""
    key = (name, S, T, pinned_collides, seed)
    if key not in _cases:
        rng = np.random.RandomState(seed)
        ch = H.chain(name)
        obs = H.PANDA_2CUBES if name in ("panda", "chain12") else [H.cuboid_obstacle(0.7, 0.1, 0.8, 0.3, 0.3, 0.3)]
        lo, hi = H.box_corners([c for c, _ in obs], [T_ for _, T_ in obs])
        cand = H.random_configs(name, 4000, seed=11)
        m = H.oracle64(name).masks(cand, lo, hi, None, None)
        hit = cand[np.flatnonzero((m["self_mask"] | m["env_mask"]) > 0)[0]]
        walk = 0.02 * rng.randn(T, ch.ndof)
        if pinned_collides:
            walk[0] = 0.0
        base = np.clip(hit[None, :] + np.cumsum(walk, axis=0), ch.lo, ch.hi)
        noise = 0.003 * rng.randn(S, T, ch.ndof)
        if pinned_collides:
            noise[0, 0] = 0.0
        x = H.f32(np.clip(base[None] + noise, ch.lo, ch.hi).reshape(S * T, ch.ndof))
        target = H.f32(H.oracle64(name).fk(H.f32(base)) + np.concatenate([0.002 * rng.randn(T, 3), np.zeros((T, 4))], axis=1))
        if pinned_collides:
            m0 = H.oracle64(name).masks(x[:1], lo, hi, None, None)
            assert (m0["self_mask"] | m0["env_mask"])[0] > 0, "waypoint 0 of trajectory 0 must collide"
        _cases[key] = (x, target, obs, lo, hi)
    return _cases[key]


# ---- the pinned step against the fp64 oracle on the reduced problem ---------------------------------------------------------------------
@pytest.mark.parametrize("pin", [FIRST | LAST, FIRST, LAST])
@pytest.mark.parametrize("name,pinned_collides,switches", [("panda", False, {}), ("panda", True, {}), ("fetch", False, {}),
                                                           ("chain12", False, {}), ("chain12", True, {"full_rows": 0})])  # fmt: skip
def test_pinned_step_equals_the_oracle_on_the_reduced_problem(robots, name, pinned_collides, switches, pin):
    """S = 3, T = 24; chain12 runs the sixteen-lanes-per-trajectory rows and (full_rows = 0) the one-lane elimination"""
    rb, o = robots[name], H.oracle64(name)
    S, T = 3, 24
    x, target, obs, lo, hi = coupled_case(name, S, T, pinned_collides)
    rb.set_obstacles([c for c, _ in obs], [T_ for _, T_ in obs])
    try:
        pm_dev, pm_orc = pin_params(pin)
        xd = dev(x)
        got_t = _with(rb, switches, lambda: rb.lm_full_step(xd, dev(target), pm_dev, pin=pin))
        free = host(_with(rb, switches, lambda: rb.lm_full_step(xd, dev(target), pm_dev)))
        rows = pinned_rows(pin, S, T)
        assert torch.equal(bits(got_t)[rows], bits(xd)[rows]), "a pinned row of x_out is not x_in bit for bit"
        got = host(got_t)
        want = reduced_oracle(o, x, target, pm_orc, S, T, pin, lo, hi)
        step = np.abs(want - x).max()
        tol = 2e-4 + 2e-3 * step
        err, moved = np.abs(got - want).max(), np.abs(free - x)[rows].max()
        print(f"{name} pin={pin} collides={pinned_collides} {switches}: step {step:.3g} tol {tol:.3g} |got - want| {err:.3g}; the free "
              f"step moves the pinned rows by {moved:.3g}, differs from the pinned one by {np.abs(free - got).max():.3g}")
        assert step > 1e-4
        assert moved > 10 * tol, "the case has no teeth: the unpinned step hardly moves the pinned rows"
        assert err < tol, (err, tol)
    finally:
        rb.set_obstacles([], [])


@pytest.mark.parametrize("pin", [FIRST | LAST, FIRST, LAST])
def test_pinned_step_with_the_pose_block_in_task_space(robots, pin):
    """the pose block on (rank-deficient blocks, one-lane elimination with floored Cholesky pivots): parity in task space on the
    well-conditioned rows, as tests/test_gpu_api.py:410-419.  Teeth: the UNPINNED step of the same parameters misses the task-space
    bound against the reduced oracle by more than a factor of two (fp64: 6.6e-3 .. 7.2e-3 against 2e-3, all of it in the pinned
    rows, whose pose correction the pin withholds), so a kernel that ignored the mask would fail here; the joint-space bound of
    3e-2 alone would not tell (PIN_LAST: the two steps differ by 2.2e-2)."""
    name = "panda"
    rb, o = robots[name], H.oracle64(name)
    S, T = 3, 24
    x, target, obs, lo, hi = coupled_case(name, S, T)
    rb.set_obstacles([c for c, _ in obs], [T_ for _, T_ in obs])
    try:
        kw = dict(use_pose=True, alpha_position=1.1, alpha_rotation=1.0, alpha_self_collision=0.05, alpha_env_collision=0.03, alpha_differencing=0.01)
        pm_dev, pm_orc = pin_params(pin, **kw)
        xd = dev(x)
        got_t = rb.lm_full_step(xd, dev(target), pm_dev, pin=pin)
        rows = pinned_rows(pin, S, T)
        assert torch.equal(bits(got_t)[rows], bits(xd)[rows])
        got, want = host(got_t), reduced_oracle(o, x, target, pm_orc, S, T, pin, lo, hi)
        Js = o.lm_step(x, H.stacked(target, S), lm_lambda=pm_dev.lm_lambda, alpha_position=pm_dev.alpha_position,
                       alpha_rotation=pm_dev.alpha_rotation)[1]  # fmt: skip
        ok = np.linalg.svd(Js, compute_uv=False)[:, -1] >= 2e-2
        assert ok.mean() > 0.5
        free = host(rb.lm_full_step(xd, dev(target), pm_dev))
        task = lambda a: np.abs(np.einsum("nij,nj->ni", Js, a - want))[ok].max()  # noqa: E731
        print(f"pose block pin={pin}: task-space |got - want| {task(got):.3g}, |free - want| {task(free):.3g}; joint space {np.abs(got - want)[ok].max():.3g}")
        assert ok[rows].all(), "the pinned rows must be among the well-conditioned ones"
        assert task(free) > 2 * 2e-3, "the case has no teeth: the unpinned step is within reach of the task-space bound"
        assert task(got) < 2e-3
        assert np.abs(got - want)[ok].max() < 3e-2
    finally:
        rb.set_obstacles([], [])


# ---- the preset (n_vq = 4) and arbitrary parameters against the reference's dense formulation, pinned columns deleted -------------------
@pytest.mark.parametrize("name,T,pin,kw", [
    ("panda", 24, FIRST, {}), ("panda", 24, LAST, {}), ("panda", 24, FIRST | LAST, {}), ("fetch", 24, FIRST, {}),
    ("panda", 24, FIRST, dict(alpha_self_collision=0.05, alpha_env_collision=0.03, alpha_differencing=0.01, alpha_differencing_prismatic_scaling=2.0,
                              alpha_virtual_configs=0.7, n_virtual_configs=3)),
    ("fetch", 24, FIRST | LAST, dict(alpha_differencing=0.01, alpha_differencing_prismatic_scaling=2.0, n_virtual_configs=2)),
    ("panda", 2, FIRST, dict(use_virtual_configs=False)), ("panda", 2, LAST, dict(use_virtual_configs=False)),
    ("fetch", 3, FIRST | LAST, dict(use_virtual_configs=False)),
])  # fmt: skip
def test_pinned_step_equals_the_dense_formulation_without_the_pinned_columns(robots, name, T, pin, kw):
    """LmResidualFns.get_r_and_J (the mirror of the reference's residual / Jacobian) on trajectory 0, fp64 solve of
    (J_f^T J_f + lambda I) delta_f = J_f^T r  with J_f = J without the columns of the pinned waypoints; T = 2 and 3: one free waypoint"""
    from cppflow_amd.optimization_utils import LmResidualFns

    rb = robots[name]
    S = 3
    x, target, obs, lo, hi = coupled_case(name, S, 24)
    d = rb.ndof
    x = np.ascontiguousarray(x.reshape(S, 24, d)[:, :T]).reshape(S * T, d)  # (the first T waypoints: next to the colliding start)
    target = target[:T]
    rb.set_obstacles([c for c, _ in obs], [T_ for _, T_ in obs])
    try:
        pm = _params(**kw)
        xd = dev(x)
        got_t = rb.lm_full_step(xd, dev(target), pm, pin=pin)  # virtual_configs = NULL: the current x, what the loop sets
        rows = pinned_rows(pin, S, T)
        assert torch.equal(bits(got_t)[rows], bits(xd)[rows])
        got = host(got_t)[:T]
        free = host(rb.lm_full_step(xd, dev(target), pm))[:T]
        x0 = dev(x[:T])
        pm.virtual_configs = x0
        Tc, cub = [torch.tensor(T_) for _, T_ in obs], [torch.tensor(c) for c, _ in obs]
        Jm, rm = LmResidualFns.get_r_and_J(pm, rb, x0, dev(target), Tcuboids=Tc, cuboids=cub)
        Jd, rd = Jm.get_J().double().cpu().numpy(), rm.get_r().double().cpu().numpy()
        assert Jd.shape[1] == T * d
        keep = np.ones(T * d, dtype=bool)
        if pin & FIRST:
            keep[:d] = False
        if pin & LAST:
            keep[(T - 1) * d :] = False
        Jf = Jd[:, keep]
        delta = np.zeros(T * d)
        delta[keep] = np.linalg.solve(Jf.T @ Jf + pm.lm_lambda * np.eye(Jf.shape[1]), Jf.T @ rd).reshape(-1)
        dense = x[:T] + delta.reshape(T, d)
        step = np.abs(dense - x[:T]).max()
        tol = 2e-4 + 2e-3 * step
        err = np.abs(got - dense).max()
        print(f"{name} T={T} pin={pin}: step {step:.3g} tol {tol:.3g} |got - dense| {err:.3g} |free - pinned| {np.abs(free - got).max():.3g}")
        assert step > 1e-4
        assert err < tol, (err, tol)
    finally:
        rb.set_obstacles([], [])


# ---- every elimination form, every boundary ------------------------------------------------------------------------------------------------
def _plain_step(rb, x, target, pm):
    """cppf_lm_full_step itself (the Python method goes through the pinned entry point)"""
    n, d, W = x.shape[0], rb.ndof, target.shape[0]
    prm = rb.full_params(pm)
    blocks = torch.empty(n * (d * (d + 1) // 2 + d), dtype=torch.float32, device=DEV)
    G = torch.empty(n * d * d, dtype=torch.float32, device=DEV)
    y, out = torch.empty(n * d, dtype=torch.float32, device=DEV), torch.empty_like(x)
    _hip.check(_hip.lib().cppf_lm_full_step(rb._handle(x.device), x.data_ptr(), target.data_ptr(), None, n // W, W, ctypes.byref(prm),
                                           blocks.data_ptr(), G.data_ptr(), y.data_ptr(), out.data_ptr(), None))  # fmt: skip
    torch.cuda.synchronize()
    return out


def _forms(d, T):
    """name -> switches.  Up to 8 joints: the parallel-in-time reduction (state in LDS split / in the workspace / in LDS one lane per
    waypoint; beyond 256 waypoints always the workspace) and the row-per-lane elimination; beyond: sixteen lanes per trajectory and
    the one-lane kernel.  (full_rows = 0 at up to 8 joints leaves the parallel-in-time form in charge at these sizes.)"""
    if d > 8:
        return {"default": {}, "one_lane": {"full_rows": 0}}
    return {"default": {}, "pcr_ws": {"pcr_lds": 0}, "pcr_one": {"pcr_lds": 1}, "pcr_split": {"pcr_lds": 2}, "pcr_full_rows0": {"full_rows": 0},
            "rows": {"pcr_max_rows": 0}}  # fmt: skip


@pytest.mark.parametrize("T", [1, 2, 3, 59, 256, 300])
@pytest.mark.parametrize("name", ["panda", "fetch", "chain12"])
def test_every_elimination_form_takes_the_pin_at_every_boundary(robots, name, T):
    rb, ch, o = robots[name], H.chain(name), H.oracle64(name)
    d = rb.ndof
    rng = np.random.RandomState(1000 + T)
    obs = H.PANDA_2CUBES
    rb.set_obstacles([c for c, _ in obs], [T_ for _, T_ in obs])
    lo, hi = H.box_corners([c for c, _ in obs], [T_ for _, T_ in obs])
    try:
        base = np.clip(rng.uniform(ch.lo, ch.hi)[None, :] * 0.5 + np.cumsum(0.03 * rng.randn(T, d), axis=0), ch.lo, ch.hi)
        target = H.f32(o.fk(H.f32(base)))
        for S in (1, 3, 11):
            x = H.f32(np.clip(base[None] + 0.01 * rng.randn(S, T, d), ch.lo, ch.hi).reshape(S * T, d))
            xd, td = dev(x), dev(target)
            for pin in (0, FIRST, LAST, FIRST | LAST):
                n_free = T - bin(pin).count("1") if T > 1 else (T if pin == 0 else 0)
                pm_dev, pm_orc = pin_params(pin) if (pin and T >= 9) else (_params(use_virtual_configs=T >= 9), None)
                rows = pinned_rows(pin, S, T)
                res = {}
                for form, sw in _forms(d, T).items():
                    out = torch.empty_like(xd)
                    bits(out).fill_(SENTINEL)
                    _with(rb, sw, lambda: rb.lm_full_step(xd, td, pm_dev, x_out=out, pin=pin))
                    assert torch.equal(bits(out)[rows], bits(xd)[rows]), (form, S, pin, "a pinned row is not x_in bit for bit")
                    assert bool(torch.isfinite(out).all()), (form, S, pin)
                    if n_free <= 0:
                        assert torch.equal(bits(out), bits(xd)), (form, S, pin, "no free waypoint: x_out must be x_in")
                    res[form] = host(out)
                if pin == 0:  # the new entry point without a mask IS the plain one
                    for form, sw in _forms(d, T).items():
                        plain = _with(rb, sw, lambda: _plain_step(rb, xd, td, pm_dev))
                        assert np.array_equal(host(plain), res[form]), (form, S)
                    continue
                # the forms among each other, under the bounds of test_coupled_step_parallel_in_time_equals_sequential_elimination
                if d <= 8:
                    step = np.abs(res["rows"] - x).max()
                    if T <= 256:
                        assert np.array_equal(res["pcr_one"], res["pcr_ws"]), (S, pin)
                    assert np.array_equal(res["default"], res["pcr_split" if T <= 256 else "pcr_ws"]), (S, pin)
                    assert np.array_equal(res["default"], res["pcr_full_rows0"]), (S, pin)
                    assert np.abs(res["default"] - res["pcr_ws"]).max() < 1e-6 + 1e-4 * np.abs(res["pcr_ws"] - x).max(), (S, pin)
                    assert np.abs(res["default"] - res["rows"]).max() < 1e-5 + 1e-3 * step, (S, pin, np.abs(res["default"] - res["rows"]).max(), step)
                else:
                    step = np.abs(res["one_lane"] - x).max()
                    assert np.abs(res["default"] - res["one_lane"]).max() < 1e-5 + 1e-3 * step, (S, pin)
                # ... and the banded fp64 oracle on the reduced problem at the long lengths
                if pm_orc is not None and S <= 3:
                    want = reduced_oracle(o, x, target, pm_orc, S, T, pin, lo, hi, banded=True)
                    ostep = np.abs(want - x).max()
                    for form in res:
                        err = np.abs(res[form] - want).max()
                        assert err < 2e-4 + 2e-3 * ostep, (form, S, pin, err, ostep)
    finally:
        rb.set_obstacles([], [])


def test_refusals_leave_the_output_untouched(robots):
    """the "satisfied" options and the one-wavefront cross-check kernel with a mask: CPPF_ERR_UNSUPPORTED, nothing launched"""
    rb = robots["panda"]
    S, T = 2, 24
    x, target, _, _, _ = coupled_case("panda", 3, T)
    xd, td = dev(x[: S * T]), dev(target)
    out = torch.empty_like(xd)
    bits(out).fill_(SENTINEL)
    with pytest.raises(RuntimeError):
        rb.lm_full_step(xd, td, _params(differencing_do_ignore_satisfied=True, differencing_ignore_satisfied_margin_deg=0.5, differencing_ignore_satisfied_margin_cm=0.5), x_out=out, pin=FIRST)
    with pytest.raises(RuntimeError):
        _with(rb, {"pcr_max_rows": 0, "full_rows": 0}, lambda: rb.lm_full_step(xd, td, _params(), x_out=out, pin=LAST))
    with pytest.raises(AssertionError):  # (CPPF_ERR_INVALID)
        rb.lm_full_step(xd, td, _params(), x_out=out, pin=4)
    torch.cuda.synchronize()
    assert bool((bits(out) == SENTINEL).all())
