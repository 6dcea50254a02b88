"""CPU side of the damped-pose-step domain (tests/pose_step_domain.py; the GPU side is tests/test_gpu_pose_step_domain.py): the
conditions the GPU module's comparisons rest on, held with the oracle alone.

  * the reference-order solve fails on no row, and numpy's dense solve of the oracle's own J_s, e_s reproduces its step (1e-10);
  * at least 90 % of the seeded rows are calm (|x64 - x0|_inf < 1);
  * rounding J and e to fp32 alone moves the exactly solved step by <= 5e-6, a quarter of the fp64 bar: the bars are not used up
    before a kernel's solve has made its first rounding error;
  * VISIBILITY: at lambda >= 1e-2 a doubled lambda moves 90 % of the seeded rows by more than 4e-4 (four times the loosest bar) and
    exchanged weights, where they differ, by more than 4e-3 -- the faults the GPU module is written for cannot hide inside its bars;
  * the unreachable block is unreachable: a scaled residual >= 1e-2 is left after the oracle's step on >= 90 % of its rows;
  * two bars of the GPU module carry a term for what fp32 does before any kernel's solve: the step-length bound (the rounding of the
    residual) and the ungated fp32 solve on far targets (eps cond^2 |e_s|).  Both are shown necessary and sufficient with the oracle.
"""

import numpy as np
import pytest

from tests import pose_step_domain as D

SETTING_IDS = [D.label(s) for s in D.SETTINGS]


def test_inputs_are_deterministic_fp32_and_inside_the_limits():
    for name in D.CASES:
        c = D.case(name)
        x0, tgt, blocks = D.problem(name)
        d = c.chain.ndof
        assert x0.shape == (D.N_SEEDED + 128 + (64 if d < 6 else 0), d) and tgt.shape == (len(x0), 7)
        assert ("unreachable" in blocks) == (d < 6) and blocks["seeded"] == slice(0, D.N_SEEDED)
        assert np.array_equal(x0, x0.astype(np.float32).astype(np.float64)) and np.array_equal(tgt, tgt.astype(np.float32).astype(np.float64))
        assert (x0 >= c.chain.lo.astype(np.float32)).all() and (x0 <= c.chain.hi.astype(np.float32)).all()
        assert np.abs(np.linalg.norm(tgt[:, 3:], axis=1) - 1.0).max() < 1e-6
        assert np.array_equal(tgt[blocks["solution"]], tgt[: D.W]) and np.array_equal(tgt[blocks["zero"]], tgt[: D.W])
        # the solution block sits on its targets: the residual is the rounding of the target to fp32
        assert np.abs(c.o64.pose_errors(x0[blocks["solution"]], tgt[blocks["solution"]])[0]).max() < 1e-6
    assert [D.case(n).chain.ndof for n in D.CASES[:10]] == [3, 4, 5, 6, 7, 8, 9, 10, 11, 12]


@pytest.mark.parametrize("name", D.CASES)
def test_reference_step_is_solved_and_two_formulations_agree(name):
    x0, _, blocks = D.problem(name)
    # 1e-10 on every row of the ten chains (measured <= 3e-13).  A shipped robot's zero pose is EXACTLY singular (Fetch: cond(Js^T Js + 1e-6 I)
    # beyond 1e13), where two fp64 LU solves differ by cond x 2e-16 themselves: that block alone gets 1e-8 there (measured 7.4e-10).
    bar = np.full(len(x0), 1e-10)
    if name in D.NAMED:
        bar[blocks["zero"]] = 1e-8
    for k, (lam, _, _) in enumerate(D.SETTINGS):
        ref = D.reference(name, k)
        assert ref["fails"] == 0 and ref["fails32"] == 0, (name, D.label(D.SETTINGS[k]))
        ts = D.task_space(ref["Js"], x0 + D.dense_step(ref["Js"], ref["es"], lam) - ref["x64"])
        assert (ts <= bar).all(), (name, D.label(D.SETTINGS[k]), ts.max())
        # the step-length bound the GPU module asserts holds for the reference itself, without the fp32 slack
        dn = np.linalg.norm(ref["x64"] - x0, axis=1)
        assert (dn <= ref["es_norm"] / (2.0 * np.sqrt(lam)) * (1 + 1e-9) + 1e-12).all(), (name, D.label(D.SETTINGS[k]))


@pytest.mark.parametrize("name", D.CASES)
def test_seeded_rows_are_calm(name):
    seeded = D.problem(name)[2]["seeded"]
    for k in range(len(D.SETTINGS)):
        calm = D.reference(name, k)["calm"][seeded].mean()
        assert calm >= 0.9, (name, D.label(D.SETTINGS[k]), calm)


@pytest.mark.parametrize("name", D.CASES)
def test_fp32_rounding_of_the_inputs_takes_a_quarter_of_the_fp64_bar_at_most(name):
    """dense_step on the fp32 oracle's J and e against the fp64 oracle's step: what no solver can undo.  (The zero block's rows are singular
    starts with far targets: there the F64 bar carries its own perturbation term, which this floor is not compared with.)"""
    x0, _, blocks = D.problem(name)
    rows = np.r_[blocks["seeded"], blocks["solution"]] if "unreachable" not in blocks else np.r_[blocks["seeded"], blocks["solution"], blocks["unreachable"]]
    for k, (lam, _, _) in enumerate(D.SETTINGS):
        ref = D.reference(name, k)
        ts = D.task_space(ref["Js"], x0 + D.dense_step(ref["J32"], ref["e32"], lam) - ref["x64"])
        assert ts[rows].max() <= 5e-6, (name, D.label(D.SETTINGS[k]), ts[rows].max())
        assert (ts <= 0.25 * ref["bar64"]).all(), (name, D.label(D.SETTINGS[k]), (ts / ref["bar64"]).max())


@pytest.mark.parametrize("name", D.CASES)
def test_wrong_damping_and_exchanged_weights_are_visible(name):
    """A condition on the inputs, not a tolerance: if it fails for a chain, the chain gets another seed and the figures stay."""
    c = D.case(name)
    x0, tgt, blocks = D.problem(name)
    seeded = blocks["seeded"]
    for k, (lam, ap, ar) in enumerate(D.SETTINGS):
        if lam < 1e-2:
            continue
        ref = D.reference(name, k)
        x2 = c.o64.lm_step(x0[seeded], tgt[seeded], lm_lambda=2 * lam, alpha_position=ap, alpha_rotation=ar, solver=0)[0]
        moved = D.task_space(ref["Js"][seeded], x2 - ref["x64"][seeded])
        assert np.quantile(moved, 0.1) > D.VISIBLE_LAMBDA, (name, D.label(D.SETTINGS[k]), "2 lambda", np.quantile(moved, 0.1))
        if ap != ar:
            xs = c.o64.lm_step(x0[seeded], tgt[seeded], lm_lambda=lam, alpha_position=ar, alpha_rotation=ap, solver=0)[0]
            moved = D.task_space(ref["Js"][seeded], xs - ref["x64"][seeded])
            assert np.quantile(moved, 0.1) > D.VISIBLE_WEIGHTS, (name, D.label(D.SETTINGS[k]), "weights", np.quantile(moved, 0.1))


@pytest.mark.parametrize("name", D.UNDER_SIX)
def test_fewer_than_six_joints_weights_are_first_order_and_the_unreachable_block_is_unreachable(name):
    c = D.case(name)
    x0, tgt, blocks = D.problem(name)
    un, seeded = blocks["unreachable"], blocks["seeded"]
    for k, (lam, ap, ar) in enumerate(D.SETTINGS):
        ref = D.reference(name, k)
        left = c.o64.lm_step(ref["x64"][un], tgt[un], solver=0, **D.lm_kwargs(D.SETTINGS[k]))[2].reshape(-1, 6)
        share = (np.linalg.norm(left, axis=1) >= 1e-2).mean()
        assert share >= 0.9, (name, D.label(D.SETTINGS[k]), share)
        if ap != ar:  # overdetermined: exchanging the weights moves the step at ANY lambda (5e-4 and more on 90 % of the rows)
            xs = c.o64.lm_step(x0[seeded], tgt[seeded], lm_lambda=lam, alpha_position=ar, alpha_rotation=ap, solver=0)[0]
            moved = D.task_space(ref["Js"][seeded], xs - ref["x64"][seeded])
            assert np.quantile(moved, 0.1) > 4e-4, (name, D.label(D.SETTINGS[k]), np.quantile(moved, 0.1))


def test_step_length_bound_needs_the_residuals_own_rounding_and_holds_with_it():
    """The exactly solved step of the fp32 oracle's J and e -- what a perfect fp32 device returns -- against the step-length bound formed
    with the fp64 oracle's e_s: without the residual term it is exceeded (only on the solution block, where |e_s| ~ 1e-7 IS rounding; 3.6
    times at lambda = 1e-6), with it it holds on every row, and the residuals differ by less than the term (1e-5 per component)."""
    worst_without, worst_with = 0.0, 0.0
    for name in D.CASES:
        x0, _, blocks = D.problem(name)
        for k, (lam, _, _) in enumerate(D.SETTINGS):
            ref = D.reference(name, k)
            assert np.abs(ref["e32"] - ref["es"]).max() < 1e-5
            dn = np.linalg.norm(D.dense_step(ref["J32"], ref["e32"], lam), axis=1)
            without = dn / D.step_length_bound(ref["es_norm"], lam, residual_term=0.0)
            over = np.flatnonzero(without > 1.0)
            assert ((over >= blocks["solution"].start) & (over < blocks["solution"].stop)).all(), (name, D.label(D.SETTINGS[k]))
            worst_without = max(worst_without, without.max())
            worst_with = max(worst_with, (dn / D.step_length_bound(ref["es_norm"], lam)).max())
    assert worst_without > 2.0 and worst_with <= 1.0, (worst_without, worst_with)


def test_far_targets_take_the_reference_own_fp32_past_the_flat_bar_on_well_conditioned_rows():
    """The reference-order fp32 oracle on the zero block's rows with sigma_min >= 2e-2: beyond 1e-4 on several chains (1.3e-4 .. 2.1e-4),
    inside the project's far-target bar 1e-4 + 1e-6 cond^2 |e_s| everywhere."""
    beyond = 0
    for name in D.CASES:
        zero = D.problem(name)[2]["zero"]
        for k, (lam, _, _) in enumerate(D.SETTINGS):
            ref = D.reference(name, k)
            well = ref["smin"][zero] >= D.WELL
            if well.any():
                ts = ref["ts32"][zero][well]
                beyond += ts.max() > D.FLOOR32
                assert (ts <= D.bar_f32_far(ref)[zero][well]).all(), (name, D.label(D.SETTINGS[k]))
    assert beyond >= 4, beyond
