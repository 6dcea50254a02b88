"""The pose residual and pose metrics over the whole rotation group: the sweep, a reference that sees what the device sees,
the derived bars, and a numpy fp32 restatement of the two hand-fitted angle functions.  Shared by tests/test_pose_domain_model.py
(CPU) and tests/test_gpu_pose_domain.py (GPU).

REFERENCE.  For fp32 x and fp32 target [n,7] everything the device's angle functions read is reproduced from fp32 values:
  R_cur, p_cur  the fp32 oracle's end-effector frame (link_frames(x)[:, ndof]); the device's FK is pinned bit-identical to that
                oracle by tests/test_gpu_parity.py::test_fk_bit_exact_vs_fp32_oracle
  R_t           quat_to_mat of lmik_device.h restated in numpy float32, operation by operation (it holds no fused multiply-add and
                the library is built with contraction off, so this is bit-exact by construction)
and from those fp32 arrays, in fp64: E = R_t R_cur^T, roll = atan2(E21, E22), pitch = asin(clamp(-E20)), yaw = atan2(E10, E00),
theta = atan2(|skew E| / 2, (tr E - 1) / 2) floored at the fp32 constant 8.94427191e-4, and the norm of the fp32 translation
difference.  The device may differ from this by two things only: the rounding of its dot3 (one multiply and two fused
multiply-adds on operands <= 1 in magnitude: DELTA = 3 * 2^-24 per entry of E) and the angle function's own error.

BARS (u = 2^-23; derived from the above, not from anything the device returned).
  roll, yaw   2 DELTA / hypot(y, x) + 4 u |ref| + 2.4e-7 [x < 0 or |y| > |x|]     (one ulp of pi for the fix-up subtractions and
              the fp32 value of pi).  The bracket is evaluated for every (y, x) the device may hold, i.e. within DELTA of the
              reference's: x < DELTA or |y| > |x| - 2 DELTA -- the device takes a fix-up whenever ITS operands say so.
  pitch       DELTA / sqrt(max(1 - sp^2, 2 DELTA)) + 4 u |ref| + 1.2e-7 [|sp| > 0.5 - DELTA]
  an angle whose reference is within its bar of +-pi is compared modulo 2 pi (the sign of a vanishing numerator is free)
  translation exact (one fp32 subtraction of identical operands)
  pos_err     4 u pos_ref (three roundings and a correctly rounded square root on identical operands)
  rot_err     8 DELTA + 4 u rot_ref above the floor; exactly the floor constant below it (either within the bar of the floor)
4 u for a function = the polynomials' documented error (1.6e-7 relative) plus the roundings of a degree-7 Horner evaluation and of
the Newton-refined reciprocal.

SECOND TIER (a tighter check on top, this module's own).  dot3 is a multiply and two explicit fused multiply-adds, so its fp32 result can
be reproduced exactly from the same fp32 operands (`dot3_32`: through fp64, where the product is exact; the rare row whose fp64 sum
sits on a tie between two fp32 neighbours is left out).  With the device's own operands known the DELTA terms drop out and the angle
must be inside the FUNCTION budget alone: 4 u |ref| + 2.4e-7 [fix-up] for atan2_lm, 4 u |ref| + 1.2e-7 [|sp| > 0.5] for asin_lm, exact
0 at a vanishing numerator, and exactly the fp32 value of +-pi/2 where the clamped sp is +-1 (z = 0, t = 0, fma(-2, 0, pi/2)).

EXCLUSIONS.  roll / yaw where hypot(y, x) < 1e-3 (gimbal lock: the angle is ill-defined), pitch where 1 - |sp| < 1e-6.  There the
tests assert what can still be said: finite outputs, the metrics inside their bars, and the pitch within sqrt(2 DELTA) + 4 u pi/2
of the REFERENCE pitch: |sqrt(a) - sqrt(b)| <= sqrt(|a - b|) with pi/2 - |asin(s)| ~ sqrt(2 (1 - |s|)) and |s_dev - s_ref| <= DELTA.
(Where the reference pitch is +-pi/2 itself that is "within sqrt(2 DELTA) + 4 u pi/2 of pi/2"; a row with 1 - |sp| = 9e-7 has a TRUE
pitch 1.3e-3 away from pi/2, more than that distance, so the statement is made about the reference and not about pi/2.)
"""

import functools

import numpy as np

from tests import helpers as H

U = 2.0**-23
DELTA = 3.0 * 2.0**-24
FLOOR32 = np.float32(8.94427191e-4)
FLOOR = float(FLOOR32)
PI_ULP, HALF_PI_ULP = 2.4e-7, 1.2e-7
GIMBAL_HYPOT, PITCH_MARGIN = 1e-3, 1e-6
ROBOTS = ("panda", "fetch", "fetch_arm", "chain12")
N_BASES = 3
f32 = np.float32


# ---- rotations (fp64; R = Rz(yaw) Ry(pitch) Rx(roll), the oracle's convention) ---------------------------------------------------
def rpy_to_mat(roll, pitch, yaw):
    roll, pitch, yaw = (np.asarray(a, dtype=np.float64) for a in (roll, pitch, yaw))
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    R = np.empty(roll.shape + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = -sp, cp * sr, cp * cr
    return R


def axis_angle_to_mat(axis, theta):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis, axis=-1, keepdims=True)
    theta = np.asarray(theta, dtype=np.float64)[..., None, None]
    K = np.zeros(axis.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -axis[..., 2], axis[..., 1], axis[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -axis[..., 0], -axis[..., 1], axis[..., 0]
    return np.eye(3) + np.sin(theta) * K + (1.0 - np.cos(theta)) * (K @ K)


def mat_to_quat64(R):
    """[n,3,3] -> unit quaternions [n,4] (w first), branch on the largest component"""
    m = R
    q4 = np.stack([1 + m[:, 0, 0] + m[:, 1, 1] + m[:, 2, 2], 1 + m[:, 0, 0] - m[:, 1, 1] - m[:, 2, 2],
                   1 - m[:, 0, 0] + m[:, 1, 1] - m[:, 2, 2], 1 - m[:, 0, 0] - m[:, 1, 1] + m[:, 2, 2]], axis=1)  # fmt: skip
    best = q4.argmax(axis=1)
    a, b, c = m[:, 2, 1] - m[:, 1, 2], m[:, 0, 2] - m[:, 2, 0], m[:, 1, 0] - m[:, 0, 1]
    d, e, f = m[:, 1, 0] + m[:, 0, 1], m[:, 0, 2] + m[:, 2, 0], m[:, 1, 2] + m[:, 2, 1]
    cand = np.stack([np.stack([q4[:, 0], a, b, c], 1), np.stack([a, q4[:, 1], d, e], 1),
                     np.stack([b, d, q4[:, 2], f], 1), np.stack([c, e, f, q4[:, 3]], 1)], axis=1)  # fmt: skip
    q = cand[np.arange(len(R)), best]
    return q / np.linalg.norm(q, axis=1, keepdims=True)


# ---- fp32 restatements, operation by operation ------------------------------------------------------------------------------------
def quat_to_mat32(q):
    """quat_to_mat of lmik_device.h: q [n,4] (w, x, y, z) float32 -> [n,9] float32, every operation rounded to fp32 in its order"""
    q = np.asarray(q)
    assert q.dtype == np.float32
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = f32(1), f32(2)
    R = np.empty((q.shape[0], 9), dtype=np.float32)
    R[:, 0] = one - two * (y * y + z * z)
    R[:, 1] = two * (x * y - w * z)
    R[:, 2] = two * (x * z + w * y)
    R[:, 3] = two * (x * y + w * z)
    R[:, 4] = one - two * (x * x + z * z)
    R[:, 5] = two * (y * z - w * x)
    R[:, 6] = two * (x * z - w * y)
    R[:, 7] = two * (y * z + w * x)
    R[:, 8] = one - two * (x * x + y * y)
    assert R.dtype == np.float32
    return R


def mat_to_quat32(R):
    """mat_to_quat of lmik_device.h / the fp32 oracle: R [n,9] float32 -> [n,4] float32"""
    R = np.asarray(R)
    assert R.dtype == np.float32
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = (R[:, i] for i in range(9))
    one, half = f32(1), f32(0.5)
    qa = np.stack([one + m00 + m11 + m22, one + m00 - m11 - m22, one - m00 + m11 - m22, one - m00 - m11 + m22], axis=1)
    best = np.zeros(len(R), dtype=np.int64)
    bv = qa[:, 0].copy()
    for i in (1, 2, 3):
        up = qa[:, i] > bv
        best[up], bv[up] = i, qa[up, i]
    d = np.sqrt(np.where(bv > 0, bv, f32(0)))
    inv = half / d
    hd = half * d
    a, b, c = (m21 - m12) * inv, (m02 - m20) * inv, (m10 - m01) * inv
    dd, e, f = (m10 + m01) * inv, (m02 + m20) * inv, (m12 + m21) * inv
    e2, f2 = (m20 + m02) * inv, (m21 + m12) * inv
    cand = np.stack([np.stack([hd, a, b, c], 1), np.stack([a, hd, dd, e], 1), np.stack([b, dd, hd, f], 1),
                     np.stack([c, e2, f2, hd], 1)], axis=1)  # fmt: skip
    out = cand[np.arange(len(R)), best]
    assert out.dtype == np.float32
    return out


def _fma32(a, b, c):
    """fp32 fused multiply-add through fp64: the product of two fp32 is exact in fp64; the sum is rounded to fp64, then to fp32"""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def _rcp32(x):
    return (1.0 / np.asarray(x, dtype=np.float64)).astype(np.float32)  # correctly rounded, as the Newton-refined v_rcp_f32 is


def _fma32_exact(a, b, c):
    """(fma(a, b, c) in fp32, ambiguous): through fp64 as `_fma32`; a row is ambiguous where the fp64 sum lies at (or within fp64
    rounding of) a tie between two fp32 neighbours, the one case in which rounding twice may differ from rounding once"""
    s64 = np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)
    r = s64.astype(np.float32)
    half = 0.5 * np.spacing(np.abs(r)).astype(np.float64)
    off, tol = np.abs(s64 - r.astype(np.float64)), 4 * np.spacing(np.abs(s64))
    return r, (np.abs(off - half) <= tol) | ((off > 0) & (np.abs(off - 0.5 * half) <= tol))  # (the second: below a power of two)


def dot3_32(a, b):
    """dot3 of lmik_device.h, fma(a2, b2, fma(a1, b1, a0 * b0)), on float32 [n,3] operands: (value float32 [n], ambiguous [n])"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32
    p = a[:, 0] * b[:, 0]
    s1, t1 = _fma32_exact(a[:, 1], b[:, 1], p)
    s2, t2 = _fma32_exact(a[:, 2], b[:, 2], s1)
    return s2, t1 | t2


ATAN_COEFFS = (0.002546269, -0.014814576, 0.040576745, -0.07317518, 0.10549001, -0.14178993, 0.19989419, -0.33332935)
ASIN_COEFFS = (0.04374494, 0.023150224, 0.04570716, 0.07493067, 0.16666822)
HALF_PI32, PI32 = f32(1.57079632679489661923), f32(3.14159265358979323846)


def atan2_lm32(y, x, coeffs=ATAN_COEFFS):
    """atan2_lm of kernels_chain.h in numpy float32 (reciprocal and square root correctly rounded)"""
    with np.errstate(all="ignore"):
        y, x = np.asarray(y, dtype=np.float32), np.asarray(x, dtype=np.float32)
        ax, ay = np.abs(x), np.abs(y)
        mx, mn = np.maximum(np.maximum(ax, ay), f32(1e-30)), np.minimum(ax, ay)
        a = mn * _rcp32(mx)
        s = a * a
        p = np.full_like(a, f32(coeffs[0]))
        for c in coeffs[1:]:
            p = _fma32(p, s, f32(c))
        r = _fma32(a * s, p, a)
        r = np.where(ay > ax, HALF_PI32 - r, r)
        r = np.where(x < 0, PI32 - r, r)
        return np.copysign(r, y).astype(np.float32)


def asin_lm32(x, half_pi=HALF_PI32):
    """asin_lm of kernels_chain.h in numpy float32"""
    with np.errstate(all="ignore"):
        x = np.asarray(x, dtype=np.float32)
        ax = np.abs(x)
        big = ax > f32(0.5)
        z = np.where(big, _fma32(f32(-0.5), ax, f32(0.5)), x * x)
        t = np.where(big, np.sqrt(z), ax)
        p = np.full_like(z, f32(ASIN_COEFFS[0]))
        for c in ASIN_COEFFS[1:]:
            p = _fma32(p, z, f32(c))
        r = _fma32(t * z, p, t)
        r = np.where(big, _fma32(f32(-2), r, half_pi), r)
        return np.copysign(r, x).astype(np.float32)


def atan2_budget(y, x, ref):
    """the function's own budget against fp64 atan2 of the same fp32 operands"""
    y, x = np.abs(np.asarray(y, dtype=np.float64)), np.asarray(x, dtype=np.float64)
    return 4 * U * np.abs(ref) + PI_ULP * ((x < 0) | (y > np.abs(x)))


def asin_budget(x, ref):
    return 4 * U * np.abs(ref) + HALF_PI_ULP * (np.abs(np.asarray(x, dtype=np.float64)) > 0.5)


def model_residual(ref, coeffs=ATAN_COEFFS, half_pi=HALF_PI32):
    """e [n,6] as the restated functions give it on the emulated operands: what a correct device returns, up to its 1-ulp square root"""
    return np.column_stack([atan2_lm32(*ref["dev_roll_yx"], coeffs=coeffs), asin_lm32(ref["dev_sp"], half_pi=half_pi),
                            atan2_lm32(*ref["dev_yaw_yx"], coeffs=coeffs), ref["e"][:, 3:]]).astype(np.float64)  # fmt: skip


# ---- the sweep -------------------------------------------------------------------------------------------------------------------
def _neighbours(v):
    v = f32(v)
    return [float(np.nextafter(v, f32(-np.inf))), float(v), float(np.nextafter(v, f32(np.inf)))]


def _unit(rng, n):
    a = rng.randn(n, 3)
    return a / np.linalg.norm(a, axis=1, keepdims=True)


THETA_LADDER = np.array([0.0, FLOOR * (1 - 1e-2), FLOOR, FLOOR * (1 + 1e-2)] + list(np.logspace(-3, 0, 13))
                        + [np.pi - 10.0**-k for k in (1, 2, 3, 4)] + [np.pi])  # ascending; the rungs next to the floor are 1 % = 8.9e-6 away, six bars  # fmt: skip
N_LADDER_AXES = 16


@functools.lru_cache(maxsize=None)
def offsets():
    """The offset set Omega: (R_off [n,3,3], delta [n,3], blocks) with blocks = {name: slice}; seeded, the same for every robot."""
    rng = np.random.RandomState(20240)
    Rs, blocks, n = [], {}, 0

    def add(name, R):
        nonlocal n
        Rs.append(R)
        blocks[name] = slice(n, n + len(R))
        n += len(R)

    # small rotations about x, y, z and three random axes, both signs, 1e-7 .. 1e-1 in 29 log steps; the exact zero offset
    axes = np.concatenate([np.eye(3), _unit(rng, 3)])
    mags = np.logspace(-7, -1, 29)
    ax = np.repeat(np.concatenate([axes, -axes]), len(mags), axis=0)
    add("small", axis_angle_to_mat(ax, np.tile(mags, 12)))
    add("zero", np.eye(3)[None])
    # the rpy grid: roll, yaw on [-pi, pi] with the ay > ax and x < 0 boundaries and their fp32 neighbours; pitch with the |sp| = 0.5
    # boundary, the approach to gimbal lock and gimbal lock itself
    ry = sorted(sum((_neighbours(s * v) for v in (np.pi / 4, np.pi / 2, 3 * np.pi / 4, np.pi) for s in (-1, 1)), [])
                + [0.0, -0.3, 0.3, -1.1, 1.1, -1.9, 1.9, -2.7, 2.7])  # fmt: skip
    pt = sorted(sum((_neighbours(s * np.pi / 6) for s in (-1, 1)), []) + [s * (np.pi / 2 - 10.0**-k) for k in (1, 2, 3, 4) for s in (-1, 1)]
                + [-np.pi / 2, np.pi / 2, 0.0])  # fmt: skip
    assert len(ry) == 33 and len(pt) == 17
    g = np.array(np.meshgrid(ry, pt, ry, indexing="ij")).reshape(3, -1).T
    lock = np.pi / 2 - np.abs(g[:, 1]) < 2e-3  # the deliberately constructed +-pi/2 pitch block: +-(pi/2 - 1e-3), +-(pi/2 - 1e-4), +-pi/2
    add("grid", rpy_to_mat(g[~lock, 0], g[~lock, 1], g[~lock, 2]))
    add("grid_lock", rpy_to_mat(g[lock, 0], g[lock, 1], g[lock, 2]))
    # Haar-random rotations (normalised Gaussian quaternions)
    q = rng.randn(4096, 4)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    add("haar", quat_to_mat32(q.astype(np.float32)).astype(np.float64).reshape(-1, 3, 3))
    # the theta ladder: axis-major, theta ascending along each axis
    lad_axes = np.repeat(_unit(rng, N_LADDER_AXES), len(THETA_LADDER), axis=0)
    add("ladder", axis_angle_to_mat(lad_axes, np.tile(THETA_LADDER, N_LADDER_AXES)))
    R = np.concatenate(Rs)
    # translations: a quarter of the rows none, the others a seeded direction of length 1e-7 .. 1 m
    length = 10.0 ** -rng.randint(0, 8, size=n).astype(np.float64)
    length[rng.randint(0, 4, size=n) == 0] = 0.0
    length[blocks["zero"]] = 0.0
    delta = _unit(rng, n) * length[:, None]
    R.setflags(write=False), delta.setflags(write=False)
    return R, delta, blocks


def base_config(name, k):
    """mid-range, one seeded random configuration, the zero pose clamped into the limits"""
    ch = H.chain(name)
    if k == 0:
        q = 0.5 * (ch.lo + ch.hi)
    elif k == 1:
        q = np.random.RandomState(7 + len(name)).uniform(ch.lo, ch.hi)
    else:
        q = np.clip(np.zeros(ch.ndof), ch.lo, ch.hi)
    return H.f32(q)


def ee_frame32(name, x):
    """(R [n,9], p [n,3]) float32: the fp32 oracle's end-effector frame"""
    fr = H.oracle32(name).link_frames(x)[:, H.chain(name).ndof]
    return fr[:, :9].astype(np.float32), fr[:, 9:].astype(np.float32)


@functools.lru_cache(maxsize=None)
def problem(name, k):
    """(x [n,d], target [n,7]) as fp32-representable float64: x = base configuration k in every row, target = offset applied to its pose"""
    R_off, delta, _ = offsets()
    q = base_config(name, k)
    R, p = ee_frame32(name, q[None])
    Rt = R_off @ R.astype(np.float64).reshape(3, 3)
    target = np.concatenate([p.astype(np.float64) + delta, mat_to_quat64(Rt)], axis=1)
    x, target = np.tile(q[None], (len(R_off), 1)), H.f32(target)
    x.setflags(write=False), target.setflags(write=False)
    return x, target


def reference(name, x, target):
    """dict of fp64 arrays: e [n,6], pos, rot, the operands the angle functions read (y/x of roll and yaw, sp), theta before the floor"""
    R, p = ee_frame32(name, x)
    tgt = np.asarray(target, dtype=np.float32)
    Rt32 = quat_to_mat32(tgt[:, 3:7]).reshape(-1, 3, 3)
    R32 = R.reshape(-1, 3, 3)
    Rt = Rt32.astype(np.float64)
    E = np.einsum("nai,nbi->nab", Rt, R.astype(np.float64).reshape(-1, 3, 3))  # E[a][b] = Rt row a . R row b
    # the operands of the device's angle functions themselves (module docstring, SECOND TIER): e20, e21, e22, e10, e00
    dv = {ab: dot3_32(Rt32[:, ab[0]], R32[:, ab[1]]) for ab in ((2, 0), (2, 1), (2, 2), (1, 0), (0, 0))}
    amb = np.column_stack([dv[2, 1][1] | dv[2, 2][1], dv[2, 0][1], dv[1, 0][1] | dv[0, 0][1]])
    sp32 = np.clip(-dv[2, 0][0], f32(-1), f32(1))
    sp = np.clip(-E[:, 2, 0], -1.0, 1.0)
    trans = (tgt[:, :3] - p).astype(np.float64)  # ONE fp32 subtraction
    assert (tgt[:, :3] - p).dtype == np.float32
    e = np.column_stack([np.arctan2(E[:, 2, 1], E[:, 2, 2]), np.arcsin(sp), np.arctan2(E[:, 1, 0], E[:, 0, 0]), trans])
    a = np.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], axis=1)
    theta = np.arctan2(0.5 * np.linalg.norm(a, axis=1), 0.5 * (np.trace(E, axis1=1, axis2=2) - 1.0))
    return dict(e=e, pos=np.linalg.norm(trans, axis=1), rot=np.maximum(theta, FLOOR), theta=theta, sp=sp,
                roll_yx=(E[:, 2, 1], E[:, 2, 2]), yaw_yx=(E[:, 1, 0], E[:, 0, 0]),
                dev_roll_yx=(dv[2, 1][0], dv[2, 2][0]), dev_yaw_yx=(dv[1, 0][0], dv[0, 0][0]), dev_sp=sp32, dev_ambiguous=amb)  # fmt: skip


@functools.lru_cache(maxsize=None)
def sweep_reference(name, k):
    x, target = problem(name, k)
    ref = reference(name, x, target)
    for v in ref.values():
        for a in v if isinstance(v, tuple) else (v,):
            a.setflags(write=False)
    return ref


# ---- bars and exclusions -----------------------------------------------------------------------------------------------------------
def atan2_bar(y, x, ref):
    fix = (x < DELTA) | (np.abs(y) > np.abs(x) - 2 * DELTA)
    with np.errstate(divide="ignore"):
        return 2 * DELTA / np.hypot(y, x) + 4 * U * np.abs(ref) + PI_ULP * fix


def pitch_bar(sp, ref):
    return DELTA / np.sqrt(np.maximum(1.0 - sp * sp, 2 * DELTA)) + 4 * U * np.abs(ref) + HALF_PI_ULP * (np.abs(sp) > 0.5 - DELTA)


def angle_bars(ref):
    """[n,3] bars of roll, pitch, yaw"""
    return np.column_stack([atan2_bar(*ref["roll_yx"], ref["e"][:, 0]), pitch_bar(ref["sp"], ref["e"][:, 1]),
                            atan2_bar(*ref["yaw_yx"], ref["e"][:, 2])])  # fmt: skip


def excluded(ref):
    """[n,3] bool: roll, pitch, yaw rows that cannot carry a tight bar"""
    return np.column_stack([np.hypot(*ref["roll_yx"]) < GIMBAL_HYPOT, 1.0 - np.abs(ref["sp"]) < PITCH_MARGIN,
                            np.hypot(*ref["yaw_yx"]) < GIMBAL_HYPOT])  # fmt: skip


EXCLUDED_PITCH_BAR = np.sqrt(2 * DELTA) + 4 * U * np.pi / 2


def angle_errors(got, ref, bars):
    """|got - ref| for the three angles [n,3]; roll / yaw rows whose reference is within the bar of +-pi are compared modulo 2 pi"""
    d = np.abs(got[:, :3] - ref["e"][:, :3])
    for c in (0, 2):
        wrap = np.pi - np.abs(ref["e"][:, c]) < bars[:, c]
        d[wrap, c] = np.minimum(d[wrap, c], np.abs(2 * np.pi - d[wrap, c]))
    return d


def pos_bar(ref):
    return 4 * U * ref["pos"]


def rot_bar(ref):
    return 8 * DELTA + 4 * U * ref["rot"]


def check_residual(got, ref, label=""):
    """Asserts the bars of the module docstring on e [n,6]; returns the measured maxima (dict) for reporting."""
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), label
    assert np.array_equal(got[:, 3:], ref["e"][:, 3:]), (label, "translation components are one fp32 subtraction: exact")
    bars, ex = angle_bars(ref), excluded(ref)
    d = angle_errors(got, ref, bars)
    out = {}
    for c, nm in enumerate(("roll", "pitch", "yaw")):
        ok = ~ex[:, c]
        ratio = d[ok, c] / bars[ok, c]
        i = np.flatnonzero(ok)[ratio.argmax()]
        rel = d[ok, c] / np.maximum(np.abs(ref["e"][ok, c]), 1e-300)
        out[nm] = dict(ratio=ratio.max(), abs=d[ok, c].max(), rel=rel[np.abs(ref["e"][ok, c]) > 0].max())
        assert ratio.max() <= 1.0, (label, nm, "row", int(i), "got", got[i, c], "want", ref["e"][i, c], "bar", bars[i, c])
    out["function"] = check_functions(got, ref, label)
    pe = ex[:, 1]
    if pe.any():
        dp = np.abs(got[pe, 1] - ref["e"][pe, 1])
        assert dp.max() <= EXCLUDED_PITCH_BAR, (label, "excluded pitch", dp.max())
    return out


def check_functions(got, ref, label=""):
    """SECOND TIER (module docstring): the three angles against fp64 functions of the device's OWN fp32 operands, on every row whose
    operands the emulation determines -- gimbal lock included, since nothing is ill-conditioned once the operands are known."""
    out = {}
    for c, key in ((0, "dev_roll_yx"), (2, "dev_yaw_yx")):
        y, x = ref[key]
        ok = ~ref["dev_ambiguous"][:, c] & (np.maximum(np.abs(x), np.abs(y)) >= f32(1e-30))
        want = np.arctan2(y.astype(np.float64), x.astype(np.float64))
        d = np.abs(got[:, c] - want)
        d = np.minimum(d, np.abs(2 * np.pi - d))
        ratio = (d / np.maximum(atan2_budget(y, x, want), 1e-300))[ok]
        assert ratio.max() <= 1.0, (label, "atan2_lm on its own operands", c, int(np.flatnonzero(ok)[ratio.argmax()]), ratio.max())
        nz = ok & (want != 0)
        out[key] = dict(ratio=ratio.max(), abs=d[ok].max(), rel=(d[nz] / np.abs(want[nz])).max())
        zero = ok & (y == 0) & (x > 0)
        assert (got[zero, c] == 0).all(), (label, "exact at 0")
    sp = ref["dev_sp"]
    ok = ~ref["dev_ambiguous"][:, 1]
    want = np.arcsin(sp.astype(np.float64))
    d = np.abs(got[:, 1] - want)
    ratio = (d / np.maximum(asin_budget(sp, want), 1e-300))[ok]
    assert ratio.max() <= 1.0, (label, "asin_lm on its own operand", int(np.flatnonzero(ok)[ratio.argmax()]), ratio.max())
    nz = ok & (want != 0)
    out["dev_sp"] = dict(ratio=ratio.max(), abs=d[ok].max(), rel=(d[nz] / np.abs(want[nz])).max())
    assert (got[ok & (sp == 0), 1] == 0).all(), (label, "exact at 0")
    for sgn in (-1.0, 1.0):  # exact at the clamp: z = 0, sqrt(0) = 0, fma(-2, 0, pi/2) = the fp32 value of pi/2
        at = ok & (sp == f32(sgn))
        assert (got[at, 1] == sgn * float(HALF_PI32)).all(), (label, "exact at the clamp", sgn)
    return out


def check_metrics(pe, re, ref, label=""):
    pe, re = np.asarray(pe, dtype=np.float64), np.asarray(re, dtype=np.float64)
    assert np.isfinite(pe).all() and np.isfinite(re).all(), label
    dpos = np.abs(pe - ref["pos"])
    assert (dpos <= pos_bar(ref)).all(), (label, "pos_err", int(np.argmax(dpos - pos_bar(ref))), dpos.max())
    bar = rot_bar(ref)
    drot = np.abs(re - ref["rot"])
    assert (drot <= bar).all(), (label, "rot_err", int(np.argmax(drot - bar)), drot.max())
    below = ref["theta"] < FLOOR - bar
    assert (re[below] == FLOOR).all(), (label, "below the floor the result is the floor constant itself")
    assert (re >= FLOOR).all(), label
    nz = ref["pos"] > 0
    return dict(pos=dict(ratio=(dpos[nz] / pos_bar(ref)[nz]).max(), abs=dpos.max(), rel=(dpos[nz] / ref["pos"][nz]).max()),
                rot=dict(ratio=(drot / bar).max(), abs=drot.max(), rel=(drot / ref["rot"]).max()))  # fmt: skip


def subsample(n_rows, seed=1):
    """a seeded subsample of Omega's row indices: 16 rows of every block (all of a smaller one), the rest drawn from the whole set"""
    _, _, blocks = offsets()
    rng = np.random.RandomState(seed)
    n_total = max(s.stop for s in blocks.values())
    idx = np.concatenate([rng.choice(np.arange(s.start, s.stop), size=min(16, s.stop - s.start), replace=False) for s in blocks.values()])
    rest = np.setdiff1d(np.arange(n_total), idx)
    return np.sort(np.concatenate([idx, rng.choice(rest, size=n_rows - len(idx), replace=False)]))
