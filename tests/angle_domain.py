"""sin / cos and the wrapped joint change over the whole angle domain: sincos_cw, sincos_pi<FOLD> and wrap_pi of csrc/lmik_device.h.
The probe chain, the row classes, numpy fp32 restatements, the fp64 references and the bars.  Shared by
tests/test_angle_domain_model.py (CPU) and tests/test_gpu_angle_domain.py (GPU).

A PROBE CHAIN.  `probe_spec`: one revolute joint about z at the origin, a fixed translation (1, 0, 0), six more coincident revolute
joints about z that every row holds at q = 0, a fixed tool at the same point.  The end-effector position is then (cos q, sin q, 0) of
the FIRST joint exactly as sincos_cw returned them: sincos_cw(0) = (0, 1), and a multiply-add by 0 or by +-1 is exact.  A row of the
sweep is [q, 0, 0, 0, 0, 0, 0], so one FK launch evaluates sincos_cw on thousands of angles through an entry point that already exists.

ROW CLASSES (`rows()`: {class: fp32 angles}; each at most MAX_ROWS = 16 384 and at least MIN_CLASS = 64 rows).
  half_pi    k pi/2 for |k| <= 64 and k = +-2^n while |q| < 2^20, each with its +-1 .. 3 fp32 neighbours (Cody-Waite cancellation)
  tiny       +-0, the three smallest subnormals of either sign, +-10^U(-40, -2)
  limits     every joint limit of every shipped robot with its +-1 .. 3 fp32 neighbours
  uniform    U(-4 pi, 4 pi)
  log        +-2^U(-20, 20): log-uniform magnitudes up to 2^20
  nonfinite  U(-4 pi, 4 pi) with +inf, -inf and NaN at NONFINITE_AT (inside otherwise finite wavefronts)

REFERENCES.  fp64 np.sin / np.cos of the fp32 input itself.  For the wrap: the fp32 remainder form `np.remainder(f32(dq) + f32(pi),
f32(2 pi)) - f32(pi)`, which the device must equal BIT FOR BIT (the device spells fmodf out as one exact +-2 pi step: Sterbenz), and
separately the fp64 wrap of the same fp32 input, for the accuracy statement only.

BARS.  1.25 x the maximum that the numpy restatement (sincos_pi) or the fp32 oracle's FK on the probe chain (sincos_cw) reaches against
fp64 over the classes, rounded up to two digits -- never anything a device returned; the margin covers the inputs between the sampled
ones and nothing else.  Each function is measured on the domain it is specified on: FOLD 0 on [-pi32, pi32], FOLD +1 / -1 on
[-pi32, 3 pi32] / [-3 pi32, pi32], FOLD 2 and sincos_cw on |q| <= 2^10, 2^16 and 2^20 separately.  The measured maxima (printed by
tests/test_angle_domain_model.py, recorded in profiles/angle_domain.txt):

                     |q| <= 2^10   2^16       2^20                         fold 0     fold +1    fold -1
  sincos_cw   abs    9.20e-8       9.20e-8    9.20e-8        sincos_pi     4.84e-7    6.43e-7    6.29e-7
   |s^2 + c^2 - 1|   1.27 u        1.30 u     1.35 u
  sincos_pi<2>       5.59e-7       6.53e-7    2.46e-6

These are maxima over the classes AND over `dense_rows()`, a CPU-only supplement of 2.1 M angles: the classes alone, 16 384 rows spread
to 2^20, give 8.7e-8 / 4.5e-7 / 4.9e-7 (sincos_cw / fold 0 / fold 2 below 2^16) and would set bars that denser sampling then exceeds.
The bars are therefore LOOSER than the classes alone would make them (sincos_cw 1.2e-7 for 1.1e-7, fold 0 6.1e-7 for 5.6e-7).
tests/test_angle_domain_model.py asserts that the constants below ARE 1.25 x what it measures, rounded up to two digits.
Every fused multiply-add of the restatements is rounded ONCE (the exact product and sum in fp64, rows on which a second rounding could
differ flagged), as the device rounds it.  4 M uniform angles and the 256 neighbours of +-pi32 give FOLD 0 4.85e-7 that way; a
figure of 5.05e-7 quoted for the same inputs could not be reproduced (separate multiplies and adds give 6.2e-7).
"""

import functools
import math

import numpy as np

from tests import helpers as H
from tests.pose_domain import _fma32_exact

U = 2.0**-23
MAX_ROWS, MIN_CLASS = 16384, 64
SEED = 31415
f32 = np.float32
PI32, TWO_PI32 = f32(3.14159265358979323846), f32(2) * f32(3.14159265358979323846)
RANGES = (2.0**10, 2.0**16, 2.0**20)
CW_DOMAIN = 2.0**22 * math.pi / 2  # beyond this the magic-number rounding of sincos_cw no longer holds the quadrant: unspecified

# ---- the bars (module docstring; tests/test_angle_domain_model.py::test_bars_are_the_recipe) ------------------------------------------
CW_BAR = {2.0**10: 1.2e-7, 2.0**16: 1.2e-7, 2.0**20: 1.2e-7}
CW_ORTHO_BAR_U = {2.0**10: 1.6, 2.0**16: 1.7, 2.0**20: 1.7}  # |s^2 + c^2 - 1| of sincos_cw in units of u = 2^-23
PI_BAR = {0: 6.1e-7, 1: 8.1e-7, -1: 7.9e-7}
PI2_BAR = {2.0**10: 7.0e-7, 2.0**16: 8.2e-7, 2.0**20: 3.1e-6}


def bar_of(measured):
    """1.25 x measured, rounded UP to two significant digits"""
    v = 1.25 * measured
    e = math.floor(math.log10(v)) - 1
    return float(f"{math.ceil(v / 10.0**e - 1e-9)}e{e}")


# ---- the probe chain --------------------------------------------------------------------------------------------------------------
PROBE_DOF = 7


def probe_spec():
    from cppflow_amd.robot_model import CapsuleSpec, JointSpec, RobotSpec

    big = (-4.0e6, 4.0e6)
    joints = [JointSpec("r0", "l0", (0, 0, 0), (0, 0, 0), (0, 0, 1), "revolute", big),
              JointSpec("arm", "larm", (1, 0, 0), (0, 0, 0), jtype="fixed")]  # fmt: skip
    joints += [JointSpec(f"r{i}", f"l{i}", (0, 0, 0), (0, 0, 0), (0, 0, 1), "revolute", (-1.0, 1.0)) for i in range(1, PROBE_DOF)]
    joints.append(JointSpec("tool", "tool", (0, 0, 0), (0, 0, 0), jtype="fixed"))
    caps = [CapsuleSpec("base", (0, 0, 0), (0, 0, 0.1), 0.01), CapsuleSpec(f"l{PROBE_DOF - 1}", (0, 0, 0), (0, 0, 0.1), 0.01)]
    return RobotSpec("angle_probe", "one angle read back through FK", "base", joints, caps, collision_pairs=[(0, 1)])


@functools.lru_cache(maxsize=None)
def probe_chain():
    from cppflow_amd.robot_model import canonicalize

    return canonicalize(probe_spec())


@functools.lru_cache(maxsize=None)
def probe_oracle(is_f32=True):
    from oracle.oracle import Oracle

    return Oracle(probe_chain(), f32=is_f32, threads=8)


def probe_rows(q):
    """[n] angles -> [n, PROBE_DOF] rows (float64 holding fp32 values)"""
    x = np.zeros((len(q), PROBE_DOF))
    x[:, 0] = np.asarray(q, dtype=np.float32)
    return x


# ---- the rows ---------------------------------------------------------------------------------------------------------------------
def neighbours(v, n=3):
    """[m] fp32 -> [m * (2 n + 1)]: every value with its +-1 .. n fp32 neighbours"""
    v = np.asarray(v, dtype=np.float32).reshape(-1)
    out, dn, up = [v], v, v
    for _ in range(n):
        dn, up = np.nextafter(dn, f32(-np.inf)), np.nextafter(up, f32(np.inf))
        out += [dn, up]
    return np.concatenate(out)


NONFINITE_AT = {5: np.inf, 70: -np.inf, 77: np.nan, 130: np.nan, 200: np.inf, 255: -np.inf}


def shipped_limits():
    from cppflow_amd.robot_zoo import ROBOT_SPECS

    lim = []
    for name in ROBOT_SPECS:
        ch = H.chain(name)
        rev = np.asarray(ch.jtype) == 0
        lim += [np.asarray(ch.lo)[rev], np.asarray(ch.hi)[rev]]
    return np.unique(np.concatenate(lim).astype(np.float32))


@functools.lru_cache(maxsize=None)
def rows():
    rng = np.random.RandomState(SEED)
    ks = list(range(-64, 65)) + [s * 2**n for n in range(7, 20) for s in (-1, 1)]
    sign = lambda n: rng.choice([-1.0, 1.0], size=n)  # noqa: E731
    tiny = np.concatenate([[0.0, -0.0], [s * m * 2.0**-149 for s in (-1, 1) for m in (1, 2, 3)], sign(4088) * 10.0 ** rng.uniform(-40, -2, 4088)])
    nonfinite = rng.uniform(-4 * np.pi, 4 * np.pi, 256)
    for i, v in NONFINITE_AT.items():
        nonfinite[i] = v
    out = dict(half_pi=neighbours(np.array(ks, dtype=np.float64) * (np.pi / 2)), tiny=tiny, limits=neighbours(shipped_limits()),
               uniform=rng.uniform(-4 * np.pi, 4 * np.pi, MAX_ROWS), log=sign(MAX_ROWS) * 2.0 ** rng.uniform(-20, 20, MAX_ROWS),
               nonfinite=nonfinite)  # fmt: skip
    out = {k: np.asarray(v, dtype=np.float32) for k, v in out.items()}
    for k, v in out.items():
        assert MIN_CLASS <= len(v) <= MAX_ROWS, (k, len(v))
        v.setflags(write=False)
    assert np.abs(out["half_pi"]).max() < 2.0**20 and np.abs(out["log"]).max() <= 2.0**20
    return out


DENSE_PER_RANGE = 1 << 19


@functools.lru_cache(maxsize=None)
def dense_rows():
    """CPU only (tests/test_angle_domain_model.py): what the bars are measured on IN ADDITION to the classes, because 16 384 rows
    spread to 2^20 leave the larger ranges thin.  U(-R, R) for R = 4 pi and the three RANGES, DENSE_PER_RANGE each; +-pi32 and +-3 pi32
    with +-1 .. 256 neighbours (where the alternating terms of sincos_pi cancel); 4096 random multiples of pi/2 below 2^20 with +-1 .. 8."""
    rng = np.random.RandomState(SEED + 2)
    parts = [rng.uniform(-r, r, DENSE_PER_RANGE) for r in (4 * np.pi,) + RANGES]
    parts.append(neighbours(np.array([s * m for s in (-1, 1) for m in (PI32, f32(3) * PI32)], dtype=np.float32), 256))
    parts.append(neighbours(rng.randint(-667543, 667544, 4096).astype(np.float64) * (np.pi / 2), 8))
    out = np.concatenate([np.asarray(p, dtype=np.float32) for p in parts])
    assert np.abs(out).max() <= 2.0**20
    out.setflags(write=False)
    return out


# ---- fp32 restatements, operation by operation (every fused multiply-add through _fma32_exact: value and "ambiguous") ----------------
CW_PIECES = (1.5703125, 4.837512969970703125e-4, 7.54978995489188e-8)
CW_SIN = (-1.9515295891e-4, 8.3321608736e-3, -1.6666654611e-1)
CW_COS = (2.443315711809948e-5, -1.388731625493765e-3, 4.166664568298827e-2)
MAGIC = f32(12582912.0)


class _Fma:
    """fused multiply-adds that remember on which rows one of them was ambiguous.  _fma32_exact flags every fp64 sum that sits on a
    tie between two fp32 neighbours; where that fp64 sum is EXACT (the error term of a TwoSum is 0: 1 - z / 2 is, every time) the tie
    is a real one, one rounding to nearest-even decides it on the device as here, and the row is not ambiguous."""

    def __init__(self, n):
        self.amb = np.zeros(n, dtype=bool)

    def __call__(self, a, b, c):
        a, b = np.broadcast_to(f32(a), self.amb.shape), np.broadcast_to(f32(b), self.amb.shape)
        r, t = _fma32_exact(a, b, c)
        p, c64 = a.astype(np.float64) * b.astype(np.float64), np.asarray(c, dtype=np.float64)
        s = p + c64
        bb = s - p
        inexact = ((p - (s - bb)) + (c64 - bb)) != 0
        self.amb |= t & inexact & np.isfinite(r)
        return r


def sincos_cw32(x, pieces=CW_PIECES, sin_c=CW_SIN, cos_c=CW_COS):
    """sincos_cw in numpy float32: (s, c, ambiguous)"""
    with np.errstate(all="ignore"):
        x = np.asarray(x, dtype=np.float32)
        fma = _Fma(x.shape)
        t = fma(x, f32(0.63661977236758134), np.broadcast_to(MAGIC, x.shape))
        k = t - MAGIC
        r = x
        for p in pieces:
            r = fma(-k, f32(p), r)
        z = r * r
        ps = fma(fma(f32(sin_c[0]), z, np.broadcast_to(f32(sin_c[1]), x.shape)), z, np.broadcast_to(f32(sin_c[2]), x.shape))
        sn = fma(r * z, ps, r)
        pc = fma(fma(f32(cos_c[0]), z, np.broadcast_to(f32(cos_c[1]), x.shape)), z, np.broadcast_to(f32(cos_c[2]), x.shape))
        cs = fma(z * z, pc, fma(f32(-0.5), z, np.broadcast_to(f32(1), x.shape)))
        ki = t.view(np.uint32)
        odd = (ki & np.uint32(1)).astype(bool)
        so = np.where(odd, cs, sn).view(np.uint32) ^ ((ki << np.uint32(30)) & np.uint32(0x80000000))
        co = np.where(odd, sn, cs).view(np.uint32) ^ (((ki + np.uint32(1)) << np.uint32(30)) & np.uint32(0x80000000))
        assert z.dtype == np.float32 and k.dtype == np.float32
        return so.view(np.float32), co.view(np.float32), fma.amb


PI_SIN = (-2.0696598213e-08, 2.7087969556e-06, -1.9817604334e-04, 8.3327908069e-03, -1.6666620970e-01, 9.9999994040e-01)
PI_COS = (1.7243808603e-09, -2.7078681342e-07, 2.4769848096e-05, -1.3887801906e-03, 4.1666489094e-02, -4.9999988079e-01)


def sincos_pi32(x, fold, sin_c=PI_SIN, cos_c=PI_COS, fold_ge=False):
    """sincos_pi<fold> in numpy float32: (s, c, ambiguous).  `fold_ge`: the mutant whose conditional turn compares >= / <= for > / <"""
    with np.errstate(all="ignore"):
        x = np.asarray(x, dtype=np.float32)
        fma = _Fma(x.shape)
        r = x
        if fold == 1:
            r = np.where((x >= PI32) if fold_ge else (x > PI32), x - TWO_PI32, x)
        elif fold == -1:
            r = np.where((x <= -PI32) if fold_ge else (x < -PI32), x + TWO_PI32, x)
        elif fold == 2:
            k = fma(x, f32(0.15915494309189535), np.broadcast_to(MAGIC, x.shape)) - MAGIC
            r = fma(-k, f32(1.9353071795864769e-3), fma(-k, f32(6.28125), x))
        else:
            assert fold == 0
        u = r * r
        ps, pc = np.broadcast_to(f32(sin_c[0]), x.shape), np.broadcast_to(f32(cos_c[0]), x.shape)
        for a, b in zip(sin_c[1:], cos_c[1:]):
            ps = fma(ps, u, np.broadcast_to(f32(a), x.shape))
            pc = fma(pc, u, np.broadcast_to(f32(b), x.shape))
        s = ps * r
        c = fma(pc, u, np.broadcast_to(f32(1), x.shape))
        assert r.dtype == np.float32 and s.dtype == np.float32
        return s, c, fma.amb


def fold_domain(fold):
    """(lo, hi) in fp32 of the interval sincos_pi<fold> is specified on (fk_joint's dispatch: lmik_device.h); None for the general fold"""
    return {0: (-PI32, PI32), 1: (-PI32, f32(3) * PI32), -1: (f32(-3) * PI32, PI32)}.get(fold)


def wrap_pi32(dq, ge_2pi=True, le_m2pi=True):
    """wrap_pi in numpy float32, both of its branches.  Mutants: `ge_2pi=False` compares x > 2 pi for x >= 2 pi, `le_m2pi=False`
    r < -2 pi for r <= -2 pi"""
    with np.errstate(all="ignore"):
        dq = np.asarray(dq, dtype=np.float32)
        x = dq + PI32
        near = np.abs(x) < f32(2) * TWO_PI32
        r = np.where((x >= TWO_PI32) if ge_2pi else (x > TWO_PI32), x - TWO_PI32, x)
        r = np.where((r <= -TWO_PI32) if le_m2pi else (r < -TWO_PI32), r + TWO_PI32, r)
        r = np.where(near, r, np.fmod(x, TWO_PI32))
        r = np.where(r < 0, r + TWO_PI32, r)
        out = r - PI32
        assert out.dtype == np.float32
        return out


def wrap_remainder32(dq):
    """the fp32 remainder form: what the device must return bit for bit"""
    with np.errstate(all="ignore"):
        dq = np.asarray(dq, dtype=np.float32)
        out = np.remainder(dq + PI32, TWO_PI32) - PI32
        assert out.dtype == np.float32
        return out


def wrap64(dq):
    """the fp64 wrap of the same fp32 input (for the accuracy statement only)"""
    with np.errstate(all="ignore"):
        dq = np.asarray(dq, dtype=np.float32).astype(np.float64)
        return np.remainder(dq + np.pi, 2 * np.pi) - np.pi


def same_bits32(a, b, zero_sign_free=False):
    """elementwise: the same fp32 bit pattern (any NaN equals any NaN; `zero_sign_free`: +0 equals -0)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    eq = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    return eq | ((a == 0) & (b == 0)) if zero_sign_free else eq


# ---- measuring against fp64 -----------------------------------------------------------------------------------------------------------
def errors(q, s, c):
    """(max(|s - sin q|, |c - cos q|), |s^2 + c^2 - 1| / u) per row, in fp64, from the fp32 input and outputs"""
    q64, s64, c64 = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (q, s, c))
    with np.errstate(all="ignore"):
        return np.maximum(np.abs(s64 - np.sin(q64)), np.abs(c64 - np.cos(q64))), np.abs(s64 * s64 + c64 * c64 - 1.0) / U


def finite_rows():
    """{class: finite fp32 angles}"""
    return {k: v[np.isfinite(v)] for k, v in rows().items()}


def check_cw(q, s, c, label=""):
    """asserts sincos_cw's bars on the finite rows q with results (s, c); returns {range: (max abs error, max ortho / u)}"""
    q = np.asarray(q, dtype=np.float32)
    err, ortho = errors(q, s, c)
    out = {}
    for rng in RANGES:
        m = np.abs(q) <= rng
        if not m.any():
            continue
        out[rng] = (float(err[m].max()), float(ortho[m].max()))
        i = int(np.flatnonzero(m)[err[m].argmax()])
        assert out[rng][0] <= CW_BAR[rng], (label, "sincos_cw", rng, "row", i, "q", float(q[i]), "error", out[rng][0], "bar", CW_BAR[rng])
        assert out[rng][1] <= CW_ORTHO_BAR_U[rng], (label, "sincos_cw orthonormality", rng, out[rng][1], CW_ORTHO_BAR_U[rng])
    return out


def check_pi(q, s, c, fold, label=""):
    """asserts sincos_pi<fold>'s bars on the rows of q inside the fold's domain; returns the measured maxima"""
    q = np.asarray(q, dtype=np.float32)
    err, _ = errors(q, s, c)
    if fold != 2:
        lo, hi = fold_domain(fold)
        m = (q >= lo) & (q <= hi)
        worst = float(err[m].max())
        assert worst <= PI_BAR[fold], (label, "sincos_pi", fold, "q", float(q[m][err[m].argmax()]), "error", worst, "bar", PI_BAR[fold])
        return worst
    out = {}
    for rng in RANGES:
        m = np.abs(q) <= rng
        out[rng] = float(err[m].max())
        assert out[rng] <= PI2_BAR[rng], (label, "sincos_pi<2>", rng, "q", float(q[m][err[m].argmax()]), "error", out[rng], "bar", PI2_BAR[rng])
    return out


# ---- the wrap classes (pairs (0, b): the difference is b itself) -----------------------------------------------------------------------
WRAP_NEIGHBOURS = 512


@functools.lru_cache(maxsize=None)
def wrap_rows():
    """{class: fp32 values b}.  k pi for |k| <= 9 with +-1 .. 512 neighbours (x == 2 pi, r == -2 pi, the 4 pi switch of the far branch
    from both sides) in two classes of at most MAX_ROWS rows, +-10^U(-40, -1), +-10^U(1, 8), +-0"""
    rng = np.random.RandomState(SEED + 1)
    sign = lambda n: rng.choice([-1.0, 1.0], size=n)  # noqa: E731
    mult = lambda ks: neighbours(np.array(ks, dtype=np.float64) * np.pi, WRAP_NEIGHBOURS)  # noqa: E731
    out = dict(k_pi_low=mult(range(-4, 5)), k_pi_high=mult([k for k in range(-9, 10) if abs(k) > 4]),
               small=sign(4096) * 10.0 ** rng.uniform(-40, -1, 4096), large=sign(4096) * 10.0 ** rng.uniform(1, 8, 4096),
               zero=np.tile([0.0, -0.0], 32))  # fmt: skip
    out = {k: np.asarray(v, dtype=np.float32) for k, v in out.items()}
    for k, v in out.items():
        assert MIN_CLASS <= len(v) <= MAX_ROWS, (k, len(v))
        v.setflags(write=False)
    return out


# ---- the lean polynomials where their folds switch (part b: tests/test_gpu_angle_domain.py; calm shares: test_angle_domain_model.py) ------
# Seven chains, one fold class each.  The five random 7-dof chains are H.random_chain_spec(7, seed) with every revolute limit overwritten;
# Fetch's continuous joints end at +-pi32 (the edge of FOLD = 0), Panda's sixth joint is the one shipped joint with FOLD = +1.
FOLD_CHAINS = {"fold0": (31, (-3.0, 3.0)), "fold+1": (32, (-1.0, 7.0)), "fold-1": (33, (-7.0, 1.0)), "fold2": (34, (-7.0, 7.0)),
               "fold2_wide": (35, (-20.0, 20.0)), "fetch": None, "panda": None}  # fmt: skip
RTC_FOLD_CHAINS = ("fold-1", "fold2_wide")  # the two that are also compiled for their own limits (hipRTC)
EDGE_CLASSES = ("limit", "inward", "pi", "turns")
EDGE_ROWS = 96  # per class
EDGE_NOISE = 0.02
TURNS = (1, 2, 3, 100)
LEAN_KS = (2, 3, 5)


def fold_spec(name):
    if FOLD_CHAINS[name] is None:
        from cppflow_amd.robot_zoo import ROBOT_SPECS

        return ROBOT_SPECS[name]()
    seed, lim = FOLD_CHAINS[name]
    spec = H.random_chain_spec(7, seed)
    spec.name = f"angle_{name}"
    for j in spec.joints:
        if j.jtype == "revolute":
            j.limits = lim
    return spec


@functools.lru_cache(maxsize=None)
def fold_chain(name):
    from cppflow_amd.robot_model import canonicalize

    return canonicalize(fold_spec(name))


@functools.lru_cache(maxsize=None)
def fold_oracle(name):
    from oracle.oracle import Oracle

    return Oracle(fold_chain(name), f32=False, threads=8)


@functools.lru_cache(maxsize=None)
def edge_problem(name):
    """Rows in H.lm_problem's construction (q* ~ U(limits), target = FK(q*), x0 = clamp(q* + EDGE_NOISE randn)) with one to three revolute
    joints per row put ON an edge value -- in q* too, so that the row starts next to its solution and its steps are small:
      limit   the limit itself                       inward  its 1 .. 3 fp32 neighbours inside
      pi      +-pi32 and its two neighbours on either side, where the limits allow
      turns   the limit plus 1, 2, 3 or 100 whole turns OUTSIDE it: the first iteration's any-angle form, then the clamp
    -> dict(x0, target [n,7], unturned [n,d] = x0 with the whole turns taken out again, cls [n] of str)"""
    ch, orc = fold_chain(name), fold_oracle(name)
    lo32, hi32 = np.asarray(ch.lo, dtype=np.float32), np.asarray(ch.hi, dtype=np.float32)
    lo, hi = lo32.astype(np.float64), hi32.astype(np.float64)
    rev = np.flatnonzero(np.asarray(ch.jtype) == 0)
    rng = np.random.RandomState(SEED + 10 + sorted(FOLD_CHAINS).index(name))
    pis = neighbours(np.array([PI32, -PI32], dtype=np.float32), 2)
    x0s, qs, uns, cls = [], [], [], []
    for c in EDGE_CLASSES:
        for r in range(EDGE_ROWS):
            q = rng.uniform(lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo))
            start = {}
            able = [j for j in rev if c != "pi" or ((pis >= lo32[j]) & (pis <= hi32[j])).any()]
            for j in rng.permutation(able)[: 1 + r % 3]:
                up = rng.randint(2) == 1
                edge = (hi32 if up else lo32)[j]
                if c == "inward":
                    for _ in range(1 + r % 3):
                        edge = np.nextafter(edge, lo32[j] if up else hi32[j])
                elif c == "pi":
                    ok = pis[(pis >= lo32[j]) & (pis <= hi32[j])]
                    edge = ok[rng.randint(len(ok))]
                q[j] = float(edge)
                start[j] = float(f32(float(edge) + (1 if up else -1) * 2 * np.pi * TURNS[r % 4])) if c == "turns" else float(edge)
            if not start:
                continue
            q = H.f32(q)
            x0 = H.f32(np.clip(q + EDGE_NOISE * rng.randn(ch.ndof), lo, hi))
            un = x0.copy()
            for j, v in start.items():
                x0[j], un[j] = v, q[j]
            x0s.append(x0), qs.append(q), uns.append(un), cls.append(c)
    x0, q = np.array(x0s), np.array(qs)
    out = dict(x0=x0, target=H.f32(orc.fk(q)), unturned=np.array(uns), cls=np.array(cls))
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def edge_trace(name, K):
    """the fp64 oracle's K clamped steps from x0: (xs, Js, es) of scripts/lean_parity_stats.oracle_trace, the largest step of each row --
    the first one taken from `unturned`, since a whole turn is no motion of the chain -- and calm = every step below 1 rad"""
    from scripts.lean_parity_stats import oracle_trace

    p = edge_problem(name)
    xs, Js, es = oracle_trace(fold_oracle(name), np.array(p["x0"]), np.array(p["target"]), K)
    moves = [np.abs(xs[1] - p["unturned"]).max(axis=1)] + [np.abs(xs[k + 1] - xs[k]).max(axis=1) for k in range(1, K)]
    steps = np.max(moves, axis=0)
    return xs, Js, es, steps, steps < 1.0
