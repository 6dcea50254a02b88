"""The damped pose step on the device where the damping and the row weights decide it (pytest -m gpu): eight settings of (lambda,
alpha_position, alpha_rotation) from 1e-6 to 1 on chains of 3 .. 12 joints through the generic kernels, Panda and Fetch through the
generated tables and one run-time-specialised chain.  Inputs, references and bars: tests/pose_step_domain.py (its docstring holds the
derivations); tests/test_pose_step_domain_model.py shows on the CPU that a doubled lambda or exchanged weights move the reference step by
4 .. 40 times the loosest bar used here, so every form of the solve is pinned:

  one bare step (n_steps = 1, clamp off)      the canonical Cholesky (AUTO / F32), the gate's fp64 re-solve through LDS (AUTO), the whole-row
                                              fp64 solve (F64), the quad shape's solve and gate, the primal Cholesky (fewer than six joints)
  two steps in one launch (clamp on)          iteration 0 is the lean 2x2-block L D L^T with its damping floors on the determinants

With POSE_STEP_DOMAIN_RECORD=<file> in the environment the worst measured / bar per (robot, form, solver, setting) is written there when
the module is done (profiles/pose_step_domain.txt is such a run).
"""

import functools
import os

import numpy as np
import pytest
import torch

from tests import pose_step_domain as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RECORDS = {}  # (robot, form, solver, setting index) -> {which bar: worst measured / bar}
COLUMNS = ("max vs reference-order fp32", "well-conditioned rows", "well-conditioned rows, far targets", "row-wise 5 x F64 bar", "row-wise F64 bar",
           "two steps, row-wise K eps amp", "step length")  # fmt: skip


def dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device=DEV)


def host(t):
    return t.detach().cpu().numpy().astype(np.float64)


@pytest.fixture(scope="module", autouse=True)
def _write_records():
    yield
    path = os.environ.get("POSE_STEP_DOMAIN_RECORD")
    if path and RECORDS:
        with open(path, "w") as f:
            f.write("# worst measured / bar per (robot, form, solver, setting); bars: tests/pose_step_domain.py.  form row2 = two steps in one launch.\n")
            f.write("# columns: " + " | ".join(f"{i + 1} {c}" for i, c in enumerate(COLUMNS)) + "\n")
            f.write("# (7, the step-length bound, is a theorem's bound that rows with sigma ~ sqrt(lambda) attain: near 1 is expected there)\n")
            for (name, form, solver, k), r in sorted(RECORDS.items(), key=lambda kv: (D.CASES.index(kv[0][0]), kv[0][1:])):
                f.write(f"{name:8s} {form:5s} {solver:4s} {D.label(D.SETTINGS[k]):34s} " + " ".join(f"{r[c]:7.4f}" if c in r else "      -" for c in COLUMNS) + "\n")


def _record(name, form, solver, k, ratios):
    r = RECORDS.setdefault((name, form, solver, k), {})
    for what, ratio in ratios.items():
        r[what] = max(r.get(what, 0.0), float(ratio))


def _solvers():
    from cppflow_amd import _hip

    return (("auto", _hip.SOLVER_AUTO), ("f64", _hip.SOLVER_F64), ("f32", _hip.SOLVER_F32))


@functools.lru_cache(maxsize=None)
def _robot(name):
    from cppflow_amd.robots import Robot, get_robot

    c = D.case(name)
    if c.spec is None:
        return get_robot(name)
    return Robot(c.spec, specialize=(name == "rtc7"))  # (this chain's specialised module is the one tests/test_gpu_round2.py builds)


@functools.lru_cache(maxsize=None)
def _one_step(name):
    """{(setting index, form, solver): dict(x, and for the row shape J, e)} of one bare step, as float64 host arrays"""
    from cppflow_amd import _hip

    rb = _robot(name)
    x0, tgt, _ = D.problem(name)
    x0_d, tgt_d = dev(x0), dev(tgt)
    out = {}
    for k, setting in enumerate(D.SETTINGS):
        for sname, solver in _solvers():
            r = rb.lm_pose_steps(x0_d, tgt_d, n_steps=1, clamp=False, return_residual=True, shape=_hip.SHAPE_ROW, solver=solver, **D.lm_kwargs(setting))
            out[(k, "row", sname)] = dict(x=host(r["x"]), J=host(r["J"]), e=host(r["e"])[:, :, 0])
            if rb.ndof >= 6:
                r = rb.lm_pose_steps(x0_d, tgt_d, n_steps=1, clamp=False, shape=_hip.SHAPE_QUAD, solver=solver, **D.lm_kwargs(setting))
                out[(k, "quad", sname)] = dict(x=host(r["x"]))
    return out


def _ratios(name, sname, ts, ref, lam, rows=slice(None)):
    """measured / bar of one run for its solver's bars on `rows`; fewer than six joints: the primal fp32 solve, held to the AUTO bars"""
    if D.case(name).chain.ndof < 6 or sname == "auto":
        return D.auto_ratios(ts, ref, lam, rows)
    if sname == "f64":
        return D.f64_ratios(ts, ref, rows)
    far = np.zeros(len(ts), dtype=bool)
    far[D.problem(name)[2]["zero"]] = True
    return D.f32_ratios(ts, ref, far, rows)


def _report(bad):
    assert not bad, "\n".join(str(b) for b in bad)


@pytest.mark.parametrize("name", D.CASES)
def test_one_bare_step_against_the_oracle(name):
    """x, J and e of one bare step in every form and solver against the fp64 reference-order oracle, every row of the launch."""
    runs = _one_step(name)
    ndof = D.case(name).chain.ndof
    bad = []
    for (k, form, sname), got in runs.items():
        lam = D.SETTINGS[k][0]
        ref = D.reference(name, k)
        tag = (name, D.label(D.SETTINGS[k]), form, sname)
        if not np.isfinite(got["x"]).all():
            bad.append((tag, "not finite"))
            continue
        ratios = _ratios(name, sname, D.task_space(ref["Js"], got["x"] - ref["x64"]), ref, lam)
        _record(name, form, sname, k, ratios)
        bad += [(tag, what, r) for what, r in ratios.items() if not r <= 1.0]
        if form == "row":  # the project's bar of test_single_lm_step_matches_reference_order_oracle
            dJ, de = np.abs(got["J"] - ref["Js"]).max(), np.abs(got["e"] - ref["es"]).max()
            if not (dJ <= 1e-5 and de <= 1e-5):
                bad.append((tag, "J / e", dJ, de))
            if ndof < 6 and not np.array_equal(got["x"], runs[(k, "row", "auto")]["x"]):
                bad.append((tag, "fewer than six joints: the solver value must not change a bit"))
    _report(bad)


@pytest.mark.parametrize("name", D.CASES)
def test_step_length_is_bounded_by_the_damping_and_vanishes_on_the_solution(name):
    """|delta|_2 <= (|e_s|_2 + E) / (2 sqrt(lambda)) on every row of every block, form, solver and setting (what the damping exists for: the
    singular starts of the zero block at large lambda included; E, the rounding of a fp32 residual: tests/pose_step_domain.py); on the
    solution block the step is inside the bars of the one-step comparison."""
    runs = _one_step(name)
    x0, _, blocks = D.problem(name)
    bad = []
    for (k, form, sname), got in runs.items():
        lam = D.SETTINGS[k][0]
        ref = D.reference(name, k)
        tag = (name, D.label(D.SETTINGS[k]), form, sname)
        ratio = np.linalg.norm(got["x"] - x0, axis=1) / D.step_length_bound(ref["es_norm"], lam)
        _record(name, form, sname, k, {"step length": np.nanmax(ratio)})
        if not (ratio <= 1.0).all():
            bad.append((tag, "step length", np.nanmax(ratio), int(np.nanargmax(ratio))))
        on = _ratios(name, sname, D.task_space(ref["Js"], got["x"] - ref["x64"]), ref, lam, blocks["solution"])
        bad += [(tag, "solution block", what, r) for what, r in on.items() if not r <= 1.0]
    _report(bad)


@pytest.mark.parametrize("name", D.CASES)
def test_two_steps_in_one_launch_against_the_oracle(name):
    """n_steps = 2 with the clamp: iteration 0 is lean (six joints and more: the 2x2-block L D L^T with its lambda x a determinant floors).
    Calm rows against the oracle's two clamped steps at the lean bar K eps (1 + 2 |step| / sigma_min) of tests/test_gpu_lean_parity.py."""
    from cppflow_amd import _hip

    rb = _robot(name)
    x0, tgt, _ = D.problem(name)
    x0_d, tgt_d = dev(x0), dev(tgt)
    bad = []
    for k, setting in enumerate(D.SETTINGS):
        ref2 = D.reference_two_steps(name, k)
        calm = ref2["calm"]
        assert calm.mean() > 0.8, (name, D.label(setting), calm.mean())
        xs = {}
        for sname, solver in _solvers()[:2]:
            r = rb.lm_pose_steps(x0_d, tgt_d, n_steps=2, clamp=True, shape=_hip.SHAPE_ROW, solver=solver, **D.lm_kwargs(setting))
            x = xs[sname] = host(r["x"])
            tag = (name, D.label(setting), "two steps", sname)
            if not np.isfinite(x).all():
                bad.append((tag, "not finite"))
                continue
            eps = D.BAR64 if sname == "f64" and rb.ndof >= 6 else D.FLOOR32
            ratio = (D.task_space(ref2["J2"], x - ref2["x2"]) / D.two_step_bar(eps, ref2))[calm].max()
            _record(name, "row2", sname, k, {"two steps, row-wise K eps amp": ratio})
            if not ratio <= 1.0:
                bad.append((tag, "row-wise K eps amp", ratio))
        if rb.ndof < 6 and not np.array_equal(xs["auto"], xs["f64"]):
            bad.append((name, D.label(setting), "fewer than six joints: the solver value must not change a bit"))
    _report(bad)


@pytest.mark.parametrize("name", D.UNDER_SIX)
def test_unreachable_targets_with_fewer_than_six_joints(name):
    """The minimiser of an unreachable target depends on the weights to first order: the primal solve's row weights, block by itself."""
    runs = _one_step(name)
    rows = D.problem(name)[2]["unreachable"]
    bad = []
    for k, setting in enumerate(D.SETTINGS):
        ref = D.reference(name, k)
        ratios = D.auto_ratios(D.task_space(ref["Js"], runs[(k, "row", "auto")]["x"] - ref["x64"]), ref, setting[0], rows)
        bad += [(name, D.label(setting), what, r) for what, r in ratios.items() if not r <= 1.0]
    _report(bad)
