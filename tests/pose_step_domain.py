"""The damped pose step  delta = J^T (J J^T + lambda S^-2)^-1 e  where the damping and the row weights decide the result: the chains,
the inputs, two references and the bars.  Shared by tests/test_pose_step_domain_model.py (CPU) and tests/test_gpu_pose_step_domain.py.

WHY.  Every other single-step comparison of the suite runs at lambda = 1e-6 with weights (3.5, 0.35), (1, 1) or (1.1, 1).  There a
doubled lambda moves the step by 1e-7 .. 2e-6 in scaled task space at the median row and exchanged weights (seven joints and more) by
a few 1e-6: below every bar.  At lambda >= 1e-2 a doubled lambda moves 90 % of the rows by > 4e-4 and exchanged weights by > 4e-3,
and with fewer than six joints (the primal solve, overdetermined) the weights are first order at any lambda.  The model module asserts
those figures, so the GPU module's bars (<= 1e-4 where they matter) can tell a wrong damping or a wrong row weight from a right one.

INPUTS (`problem`).  Per chain one launch of
  seeded       512 rows = 8 seeds x 64 waypoints in the reference's construction (q* ~ U(limits), target = fp32(FK(q*)),
               x0 = clip(q* + 0.1 randn)), from RandomState(seed), fp32-representable
  solution      64 rows with x0 = q*                                   (zero residual up to the rounding of the target)
  zero          64 rows at the zero pose clamped into the limits + 1e-3 randn, against the same 64 targets (singular starts, far targets)
  unreachable   64 rows, fewer than six joints only: the first seed's x0 against targets displaced from FK(q*) by 5 cm along a random
               direction and by 0.1 rad about a random axis -- no configuration reaches them, so the minimiser itself depends on the weights
every row with its own target (the stacked form, W = n).

REFERENCES.  `reference` is the reference-order oracle (oracle/lmik_oracle.c: scaled primal normal equations, LU) in fp64 and in fp32;
`dense_step` states the same formulation in numpy, solve(Js^T Js + lambda I, Js^T es), independent of the oracle's solver.

BARS (scaled task space, ts = |J_s (x - x64)|_inf with the fp64 oracle's J_s; none of them fitted to a kernel's output).
  F64, >= 6 joints, every row     2e-5 + 2.5e-7 sigma_max |e_s|_inf / max(sigma_min, sqrt(lambda)).  At lambda = 1e-6 this is bar64 of
                                  tests/test_gpu_parity_allrows.py; the generalisation: the filter factor sigma^2 / (sigma^2 + lambda) is most
                                  sensitive to a relative change of sigma (2^-23 sigma_max / sigma, the last bits of the fp32 Jacobian)
                                  at sigma ~ sqrt(lambda), with slope ~ 1 / sqrt(lambda).
  AUTO                            max <= max(max of the reference-order fp32 oracle, 1e-4); <= 1e-4 where sigma_min >= 2e-2; row by row
                                  <= 5 x the F64 bar at lambda >= 1e-3 (well conditioned: nothing is flagged, or what is flagged is re-solved)
  F32                             <= 1e-4 where sigma_min >= 2e-2; on the zero block (far targets, |e_s| of several units) the project's
                                  bar for such rows, 1e-4 + 1e-6 (sigma_max / sigma_min)^2 |e_s|_inf (tests/test_gpu_parity_allrows.py,
                                  source "special"): an ungated fp32 solve is off by eps cond(A) |e_s| with cond(A) = cond(J_s)^2 --
                                  why the gate exists.  The reference's OWN fp32 arithmetic is at 1.3e-4 .. 2.1e-4 on those rows
                                  (asserted in the model module), so a flat 1e-4 there is not a statement about a kernel.
  fewer than six joints           the primal fp32 solve whatever the solver: the AUTO bars (sigma_min = the d-th singular value)
  step length, every row          |delta|_2 <= (|e_s|_2 + E) / (2 sqrt(lambda)) (1 + 1e-3) + 1e-6: sigma / (sigma^2 + lambda) <= 1 / (2 sqrt(lambda))
                                  for every singular value of J_s, whatever the conditioning.  e_s is the fp64 oracle's; the step is linear in
                                  the residual with that same norm, and a device's fp32 residual is within the project's 1e-5 per component of
                                  the oracle's (asserted on the returned e), so E = sqrt(6) 1e-5.  Without E the bound is a statement about
                                  the rounding of the residual, not about the damping: on the solution block |e_s| ~ 1e-7 is itself rounding,
                                  and the EXACTLY solved step of the fp32 oracle's J, e exceeds the E-free bound 3.6 times at lambda = 1e-6
                                  (asserted in the model module, where the bound with E holds for it on every row).
  two steps in one launch         K eps (1 + 2 |step| / sigma_min), K = 2, eps = 2e-5 (F64) / 1e-4 (AUTO): tests/test_gpu_lean_parity.py, DESIGN 5.2
The share of the bars that rounding J and e to fp32 alone takes is asserted (<= 5e-6) in the model module.
"""

import functools
import types

import numpy as np

from tests import helpers as H

GENERIC = ((3, 4), (4, 5), (5, 6), (6, 12), (7, 11), (8, 2), (9, 7), (10, 8), (11, 41), (12, 3))  # (ndof, seed of chain and inputs)
# six joints: seed 12 and not the suite's usual 0, on which the oracle itself keeps only 85 % of the rows calm at lambda = 1e-6
NAMED = {"panda": 17, "fetch": 18, "rtc7": 21}  # shipped robots (generated tables) and the run-time-specialised chain: seed of the inputs
CASES = tuple(f"chain{d}" for d, _ in GENERIC) + tuple(NAMED)
UNDER_SIX = tuple(f"chain{d}" for d, _ in GENERIC if d < 6)  # the primal solve; these launches carry the unreachable block
SETTINGS = ((1e-6, 3.5, 0.35), (1e-6, 1.0, 1.0), (1e-4, 4.0, 0.25), (1e-3, 3.5, 0.35), (1e-2, 1.0, 1.0), (1e-2, 0.25, 2.0),
            (1e-1, 1.0, 1.0), (1.0, 2.0, 0.5))  # (lambda, alpha_position, alpha_rotation)  # fmt: skip
S, W = 8, 64
N_SEEDED = S * W
WELL = 2e-2  # sigma_min(J_s) from which the fp32 solves carry the project's 1e-4
FLOOR32 = 1e-4
BAR64 = 2e-5
VISIBLE_LAMBDA, VISIBLE_WEIGHTS = 4e-4, 4e-3  # four times the loosest bar / forty times


def lm_kwargs(setting):
    lam, ap, ar = setting
    return dict(lm_lambda=lam, alpha_position=ap, alpha_rotation=ar)


def label(setting):
    return "lam=%g a_pos=%g a_rot=%g" % setting


@functools.lru_cache(maxsize=None)
def case(name):
    """spec (None for a shipped robot), canonical chain, both oracle builds and the seed of the inputs"""
    from cppflow_amd.robot_model import canonicalize
    from oracle.oracle import Oracle

    if name in ("panda", "fetch"):
        return types.SimpleNamespace(name=name, spec=None, chain=H.chain(name), o64=H.oracle64(name), o32=H.oracle32(name), seed=NAMED[name])
    ndof, seed = (7, NAMED[name]) if name == "rtc7" else next((d, s) for d, s in GENERIC if f"chain{d}" == name)
    spec = H.random_chain_spec(ndof, seed)
    ch = canonicalize(spec)
    return types.SimpleNamespace(name=name, spec=spec, chain=ch, o64=Oracle(ch, f32=False, threads=8), o32=Oracle(ch, f32=True, threads=8), seed=seed)


def _unit(rng, n):
    a = rng.randn(n, 3)
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def _quat_mul(a, b):
    """Hamilton product, w first"""
    aw, ax, ay, az = a.T
    bw, bx, by, bz = b.T
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=1)  # fmt: skip


@functools.lru_cache(maxsize=None)
def problem(name):
    """(x0 [n,d], target [n,7], blocks {name: slice}) as fp32-representable float64, read-only"""
    c = case(name)
    ch, d = c.chain, c.chain.ndof
    rng = np.random.RandomState(c.seed)
    q_star = H.f32(rng.uniform(ch.lo, ch.hi, size=(W, d)))
    pose = c.o64.fk(q_star)
    target = H.f32(pose)
    seeded = np.clip(q_star[None] + 0.1 * rng.randn(S, W, d), ch.lo, ch.hi).reshape(N_SEEDED, d)  # (the draws so far: helpers.lm_problem's)
    zero = np.clip(np.clip(np.zeros(d), ch.lo, ch.hi) + 1e-3 * rng.randn(W, d), ch.lo, ch.hi)
    xs, ts, blocks = [seeded, q_star, zero], [H.stacked(target, S), target, target], {}
    if d < 6:
        half = 0.5 * 0.1
        turn = np.concatenate([np.full((W, 1), np.cos(half)), np.sin(half) * _unit(rng, W)], axis=1)
        moved = np.concatenate([pose[:, :3] + 0.05 * _unit(rng, W), _quat_mul(turn, pose[:, 3:])], axis=1)
        xs.append(seeded[:W])
        ts.append(H.f32(moved))
    n = 0
    for nm, x in zip(("seeded", "solution", "zero", "unreachable"), xs):
        blocks[nm] = slice(n, n + len(x))
        n += len(x)
    x0, tgt = H.f32(np.concatenate(xs)), np.concatenate(ts)
    x0.setflags(write=False), tgt.setflags(write=False)
    return x0, tgt, blocks


def task_space(Js, dx):
    return np.abs(np.einsum("nij,nj->ni", Js, dx)).max(axis=1)


def dense_step(Js, es, lam):
    """the reference's formulation in fp64 numpy: solve(Js^T Js + lambda I, Js^T es), [n,d]"""
    Js, es = np.asarray(Js, dtype=np.float64), np.asarray(es, dtype=np.float64).reshape(len(Js), 6)
    A = np.einsum("nki,nkj->nij", Js, Js) + lam * np.eye(Js.shape[2])
    return np.linalg.solve(A, np.einsum("nki,nk->ni", Js, es)[..., None])[..., 0]


def sigmas(Js):
    """(sigma_min, sigma_max) of the scaled Jacobian; sigma_min is the min(6, d)-th singular value (the smallest that is not zero by shape)"""
    sv = np.linalg.svd(Js, compute_uv=False)
    return sv[:, -1], sv[:, 0]


@functools.lru_cache(maxsize=None)
def reference(name, k):
    """The oracles' one bare step of setting k on the whole launch (read-only arrays): x64, Js, es [n,6], fails, x32, J32, e32, smin, smax,
    step = |x64 - x0|_inf, calm = step < 1, bar64, ts32, es_norm = |e_s|_2"""
    c = case(name)
    x0, tgt, _ = problem(name)
    lam = SETTINGS[k][0]
    x64, Js, es, fails = c.o64.lm_step(x0, tgt, solver=0, **lm_kwargs(SETTINGS[k]))
    x32, J32, e32, fails32 = c.o32.lm_step(x0, tgt, solver=0, **lm_kwargs(SETTINGS[k]))
    es, e32 = es.reshape(len(x0), 6), e32.reshape(len(x0), 6)
    smin, smax = sigmas(Js)
    step = np.abs(x64 - x0).max(axis=1)
    r = dict(x64=x64, Js=Js, es=es, x32=x32, J32=J32, e32=e32, smin=smin, smax=smax, step=step, calm=step < 1.0,
             bar64=bar_f64(smin, smax, es, lam), ts32=task_space(Js, x32 - x64), es_norm=np.linalg.norm(es, axis=1))  # fmt: skip
    for v in r.values():
        v.setflags(write=False)
    r["fails"], r["fails32"] = int(fails), int(fails32)
    return r


@functools.lru_cache(maxsize=None)
def reference_two_steps(name, k):
    """The fp64 oracle's two clamped steps: x2, the scaled Jacobian there, steps = the larger of the two |step|_inf, smin over the three
    linearisation points, calm = both steps < 1"""
    c = case(name)
    x0, tgt, _ = problem(name)
    kw = lm_kwargs(SETTINGS[k])
    x1 = c.o64.lm_steps(x0, tgt, 1, solver=0, **kw)
    x2 = c.o64.lm_steps(x0, tgt, 2, solver=0, **kw)
    smin = reference(name, k)["smin"]
    for x in (x1, x2):
        J = c.o64.lm_step(x, tgt, solver=0, **kw)[1]
        smin = np.minimum(smin, sigmas(J)[0])
    steps = np.maximum(np.abs(x1 - x0).max(axis=1), np.abs(x2 - x1).max(axis=1))
    r = dict(x2=x2, J2=J, steps=steps, smin=smin, calm=steps < 1.0)
    for v in r.values():
        v.setflags(write=False)
    return r


# ---- bars ---------------------------------------------------------------------------------------------------------------------------
def bar_f64(smin, smax, es, lam):
    return BAR64 + 2.5e-7 * smax * np.abs(es).max(axis=1) / np.maximum(smin, np.sqrt(lam))


def auto_ratios(ts, ref, lam, rows=slice(None)):
    """measured / bar for the three AUTO bars on `rows` (module docstring); a bar that does not apply is left out"""
    ts, ts32, smin, bar64 = ts[rows], ref["ts32"][rows], ref["smin"][rows], ref["bar64"][rows]
    out = {"max vs reference-order fp32": ts.max() / max(ts32.max(), FLOOR32)}
    well = smin >= WELL
    if well.any():
        out["well-conditioned rows"] = ts[well].max() / FLOOR32
    if lam >= 1e-3:
        out["row-wise 5 x F64 bar"] = (ts / (5.0 * bar64)).max()
    return out


def f64_ratios(ts, ref, rows=slice(None)):
    return {"row-wise F64 bar": (ts[rows] / ref["bar64"][rows]).max()}


def bar_f32_far(ref):
    """the project's bar of an ungated fp32 solve on far targets (tests/test_gpu_parity_allrows.py, source "special"), for rows with sigma_min >= WELL"""
    return FLOOR32 + 1e-6 * (ref["smax"] / ref["smin"]) ** 2 * np.abs(ref["es"]).max(axis=1)


def f32_ratios(ts, ref, far, rows=slice(None)):
    """`far` [n] bool: the rows of the zero block"""
    well, far, ts = ref["smin"][rows] >= WELL, far[rows], ts[rows]
    out = {}
    if (well & ~far).any():
        out["well-conditioned rows"] = ts[well & ~far].max() / FLOOR32
    if (well & far).any():
        out["well-conditioned rows, far targets"] = (ts / bar_f32_far(ref)[rows])[well & far].max()
    return out


RESIDUAL_E = np.sqrt(6.0) * 1e-5  # |e_s(fp32) - e_s(fp64)|_2 at the project's 1e-5 per component


def step_length_bound(es_norm, lam, residual_term=RESIDUAL_E):
    return (es_norm + residual_term) / (2.0 * np.sqrt(lam)) * (1.0 + 1e-3) + 1e-6


def two_step_bar(eps, ref2):
    return 2 * eps * (1.0 + 2.0 * ref2["steps"] / np.maximum(ref2["smin"], 1e-6))
