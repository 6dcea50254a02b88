"""The pose residual (atan2_lm / asin_lm through pose_error<false>) and the pose metrics (pose_metrics) over the whole rotation group,
through entry points that already exist: no test kernels.  Sweep, reference, bars and exclusions: tests/pose_domain.py (its docstring
holds the derivations); the CPU side, which shows that a correct implementation meets the bars and that three small mutations do
not, is tests/test_pose_domain_model.py.

The first two tests print the device's maxima over the sweep (4 robots x 3 base configurations x 23 310 offsets) as a share of each bar,
absolute and relative (pytest -s).
"""

import os

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import pose_domain as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
UNIT = dict(lm_lambda=1e-6, alpha_position=1.0, alpha_rotation=1.0)  # the residual output is e * alpha: with 1.0 it is e itself, bit for bit
LM = dict(lm_lambda=1e-6, alpha_position=3.5, alpha_rotation=0.35)
RAD2DEG32 = np.float32(57.29577951308232087680)


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


@pytest.fixture(scope="module")
def robots():
    from cppflow_amd.robots import get_robot

    return {n: get_robot(n) for n in P.ROBOTS}


def _fmt(d):
    return "  ".join(f"{k}: {v['ratio']:.3f} of the bar, {v['abs']:.3e} abs, {v['rel']:.3e} rel" for k, v in d.items() if "ratio" in v)


@pytest.mark.parametrize("name", P.ROBOTS)
def test_residual_meets_the_bars_over_the_rotation_group(robots, name):
    """cppf_pose_errors over Omega from three base configurations, one launch of S = 1, W = |Omega| each: roll / pitch / yaw inside
    the derived bars (and inside the function budget on the device's own operands), the translation exact, every output finite."""
    for k in range(P.N_BASES):
        x, target = P.problem(name, k)
        e, _ = robots[name].pose_errors(dev(x), dev(target), want_current_poses=False)
        got = P.check_residual(host(e)[:, :, 0], P.sweep_reference(name, k), (name, k))
        print(f"\n{name} base {k}  {_fmt(got)}\n    on its own operands  {_fmt(got['function'])}")


@pytest.mark.parametrize("name", P.ROBOTS)
def test_metrics_meet_the_bars_over_the_rotation_group(robots, name):
    """cppf_pose_error_metrics over Omega: pos_err within 4 u relative, rot_err within 8 DELTA + 4 u rot above the floor and the floor
    constant itself below it; along each axis of the theta ladder rot_err does not decrease (within the bars of the two rungs)."""
    _, _, blocks = P.offsets()
    for k in range(P.N_BASES):
        x, target = P.problem(name, k)
        ref = P.sweep_reference(name, k)
        pe, re = robots[name].pose_error_metrics(dev(x), dev(target))
        pe, re = host(pe), host(re)
        got = P.check_metrics(pe, re, ref, (name, k))
        print(f"\n{name} base {k}  {_fmt(got)}")
        lad = re[blocks["ladder"]].reshape(P.N_LADDER_AXES, -1)
        bar = P.rot_bar(ref)[blocks["ladder"]].reshape(P.N_LADDER_AXES, -1)
        assert (lad[:, 1:] >= lad[:, :-1] - (bar[:, 1:] + bar[:, :-1])).all(), (name, k)
        assert (lad[:, :2] == P.FLOOR).all() and (lad[:, 3:] > P.FLOOR).all()  # theta = 0 and 0.99 floor; 1.01 floor and beyond


@pytest.mark.parametrize("name", P.ROBOTS)
def test_one_value_through_every_route(robots, name):
    """A 2 048-row subsample of Omega through every entry point that reports the residual or the metrics.

    Which routes share the device function (read from the code, asserted bit for bit here):
      e        pose_errors_kernel and the LAST iteration of the row-shape fused launch (lm_row_iterate<LEAD = false>) both run the
               canonical FK and pose_error<false>; the fused launch stores e * alpha (alpha = 1 here).  The robot-specialised and the
               generic (force_generic) kernels run the same arithmetic.  The quad shape forms its pitch as atan2_lm(sp, sqrt((1 - sp)(1 + sp)))
               in registers and REFUSES return_residual (tests/test_gpu_round2.py::test_quad_shape_refuses_what_it_cannot_produce): its
               residual is not observable at the boundary, so there is no quad route for e.
      metrics  pose_metrics_kernel, the fused launch's finish stage in the row shape (pose_metrics) and in the quad shape (the same operations
               in the same order, one row of R per lane), seed_validity_kernel and plan_metrics_seed (pose_metrics): for the same x the
               same bits.  The fused launches are compared at their own x_K, and meet the bars against the reference evaluated there.
               seed_validity / plan_metrics maxima are maxima of fp32(100 pe) and fp32(rad2deg re): exact.  The plan's means are fp32 sums of
               positive terms, W / 64 per lane, six butterfly levels and one division: (W / 64 + 7) 2^-24 relative.
    """
    from cppflow_amd import _hip

    rb = robots[name]
    idx = P.subsample(2048)
    xs, ts = P.problem(name, 1)
    x, target = xs[idx], ts[idx]
    W = len(idx)
    ref = P.reference(name, x, target)
    e0 = rb.pose_errors(dev(x), dev(target), want_current_poses=False)[0]
    P.check_residual(host(e0)[:, :, 0], ref, name)
    fused = rb.lm_pose_steps(dev(x), dev(target), n_steps=1, clamp=False, return_residual=True, shape=_hip.SHAPE_ROW, **UNIT)
    assert torch.equal(fused["e"], e0)
    try:
        rb.debug_set("force_generic", 1)
        assert torch.equal(rb.pose_errors(dev(x), dev(target), want_current_poses=False)[0], e0)
        g = rb.lm_pose_steps(dev(x), dev(target), n_steps=1, clamp=False, return_residual=True, shape=_hip.SHAPE_ROW, **UNIT)
        assert torch.equal(g["e"], e0) and torch.equal(g["x"], fused["x"])
    finally:
        rb.debug_set("force_generic", 0)
    # metrics
    pe0, re0 = rb.pose_error_metrics(dev(x), dev(target))
    P.check_metrics(host(pe0), host(re0), ref, name)
    shapes = [_hip.SHAPE_ROW] + ([_hip.SHAPE_QUAD] if rb.ndof >= 6 else [])
    for shape in shapes:
        r = rb.lm_pose_steps(dev(x), dev(target), n_steps=1, want_errors=True, shape=shape, **LM)
        xk = host(r["x"])
        assert np.isfinite(xk).all()
        pe_k, re_k = rb.pose_error_metrics(r["x"], dev(target))
        assert torch.equal(r["pos_err_m"], pe_k) and torch.equal(r["rot_err_rad"], re_k), shape
        P.check_metrics(host(r["pos_err_m"]), host(r["rot_err_rad"]), P.reference(name, xk, target), (name, shape))
    pc = (np.float32(100) * pe0.cpu().numpy()).astype(np.float32)
    rd = (RAD2DEG32 * re0.cpu().numpy()).astype(np.float32)
    sv = rb.seed_validity(dev(x), dev(target)).cpu().numpy()
    assert sv.shape == (1, 4) and sv[0, 0] == pc.max() and sv[0, 1] == rd.max()
    pm = rb.plan_metrics(dev(x), dev(target)).cpu().numpy()
    assert pm[0, 0] == pc.max() and pm[0, 2] == rd.max()
    bar = (W / 64 + 7) * 2.0**-24
    for col, v in ((1, pc), (3, rd)):
        mean = v.astype(np.float64).mean()
        assert abs(pm[0, col] - mean) <= bar * mean, (name, col, pm[0, col], mean)


def _sign_cases(name):
    idx = P.subsample(512, seed=2)
    xs, ts = P.problem(name, 1)
    cases = [("subsample", xs[idx], ts[idx])]
    if name == "fetch_arm":
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_paths.npz"))
        path = H.f32(z["fetch_arm__s__truncated"])
        assert path.shape == (59, 7)
        cases.append(("path", H.random_configs(name, 59, seed=5, margin=0.2), path))
    return cases


@pytest.mark.parametrize("name", P.ROBOTS)
def test_sign_of_the_target_quaternion_changes_no_bit(robots, name):
    """quat_to_mat is even in q (every term is a product of two components): q and -q are the same target to every kernel.
    pose_errors, pose_error_metrics, lm_pose_steps at K = 3 in both shapes (x, errors, masks) and one coupled step at S = 2."""
    from cppflow_amd import _hip
    from cppflow_amd.lm_hyper_parameters import ALT_LOSS_V2_1_DIFF, OptimizationParameters

    rb = robots[name]
    pm = OptimizationParameters(**{**ALT_LOSS_V2_1_DIFF.__dict__, "use_pose": True, "alpha_position": 1.1, "alpha_rotation": 1.0})
    pm.virtual_configs = torch.tensor([])
    for label, x1, target in _sign_cases(name):
        W = len(target)
        neg = target.copy()
        neg[:, 3:] = -neg[:, 3:]
        rng = np.random.RandomState(W)
        x = H.f32(np.concatenate([x1, np.clip(x1 + 0.05 * rng.randn(*x1.shape), H.chain(name).lo, H.chain(name).hi)]))  # S = 2
        out = []
        for t in (target, neg):
            o = {}
            o["e"] = rb.pose_errors(dev(x), dev(t), want_current_poses=False)[0]
            o["pe"], o["re"] = rb.pose_error_metrics(dev(x), dev(t))
            for shape in [_hip.SHAPE_ROW] + ([_hip.SHAPE_QUAD] if rb.ndof >= 6 else []):
                r = rb.lm_pose_steps(dev(x), dev(t), n_steps=3, want_errors=True, want_collisions=True, shape=shape, **LM)
                o.update({f"{shape}_{k}": v for k, v in r.items()})
            T = min(W, 64)
            xt = np.concatenate([x[:T], x[W : W + T]])
            o["coupled"] = rb.lm_full_step(dev(xt), dev(t[:T]), pm)
            out.append(o)
        assert set(out[0]) == set(out[1]) and len(out[0]) >= 10
        for k in out[0]:
            a, b = out[0][k], out[1][k]
            assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (name, label, k)  # bits: NaN-proof
        assert np.isfinite(host(out[0]["coupled"])).all()


@pytest.mark.parametrize("name", ("panda", "fetch"))
def test_nan_rows_stay_nan_and_touch_no_other_row(robots, name):
    """W = 65: the second wavefront holds one row.  A NaN in one row's x or target leaves that row NaN (where the quantity depends on
    the poisoned input) and every other row of the launch bit-identical to the clean launch."""
    rb = robots[name]
    idx = P.subsample(2048)[:: 2048 // 65][:65]
    xs, ts = P.problem(name, 1)
    x, target = xs[idx].copy(), ts[idx].copy()
    assert len(x) == 65
    e0 = rb.pose_errors(dev(x), dev(target), want_current_poses=False)[0].cpu().numpy()[:, :, 0]
    pe0, re0 = (t.cpu().numpy() for t in rb.pose_error_metrics(dev(x), dev(target)))
    assert np.isfinite(e0).all() and np.isfinite(pe0).all() and np.isfinite(re0).all()
    # (row, what is poisoned, which of e's components / pos / rot must be NaN)
    cases = [(3, "x", slice(0, 6), True, True), (64, "x", slice(0, 6), True, True), (10, "quat", slice(0, 3), False, True),
             (64, "quat", slice(0, 3), False, True), (63, "trans", slice(3, 4), True, False)]  # fmt: skip
    for row, what, nan_e, nan_pos, nan_rot in cases:
        xb, tb = x.copy(), target.copy()
        if what == "x":
            xb[row, int(np.flatnonzero(np.asarray(H.chain(name).jtype) == 0)[0])] = np.nan  # the first revolute joint
        elif what == "quat":
            tb[row, 4] = np.nan
        else:
            tb[row, 0] = np.nan
        e = rb.pose_errors(dev(xb), dev(tb), want_current_poses=False)[0].cpu().numpy()[:, :, 0]
        pe, re = (t.cpu().numpy() for t in rb.pose_error_metrics(dev(xb), dev(tb)))
        others = np.arange(65) != row
        assert np.array_equal(e[others], e0[others]) and np.array_equal(pe[others], pe0[others]) and np.array_equal(re[others], re0[others])
        assert np.isnan(e[row, nan_e]).all(), (name, row, what, e[row])
        keep = np.ones(6, dtype=bool)
        keep[nan_e] = False
        assert np.array_equal(e[row, keep], e0[row, keep]), (name, row, what)
        assert np.isnan(pe[row]) == nan_pos and (nan_pos or pe[row] == pe0[row]), (name, row, what, pe[row])
        assert np.isnan(re[row]) == nan_rot and (nan_rot or re[row] == re0[row]), (name, row, what, re[row])
