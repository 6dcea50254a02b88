"""The two capsule distance functions (seg_seg_closest2 / seg_box_closest2 of csrc/lmik_device.h, restated line for line by
oracle/lmik_oracle.c) on degenerate geometry: a free capsule, the sweep, a reference that does not share the algorithm, the classes
and the bars.  Shared by tests/test_capsule_domain_model.py (CPU) and tests/test_gpu_capsule_domain.py (GPU).

A FREE CAPSULE.  `free_capsule_spec`: three prismatic joints along x, y, z (limits +-4), three coincident revolute joints about z, y, x
(limits +-7), a fixed tool; one capsule on the base, one on the last link, collision_pairs = [(0, 1)].  A row of q = [x y z yaw pitch
roll] is a pose of the moving capsule, so one launch tests thousands of segment pairs.  The moving segments lie along the last link's
x axis, centred on its origin: their world half-axis is L times the first column of Rz(yaw) Ry(pitch) Rx(roll).

REFERENCE.  Takes the fp32 end points the device itself uses (`oracle32.capsule_endpoints`, pinned bit-exact to the device's FK by
tests/test_gpu_parity.py) and minimises, in fp64, a convex function of ONE parameter: f(t) = distance from p(t) = p0 + t (p1 - p0) to
the box (one clamp per coordinate) or to the other segment (a projection and one clamp; the projection divides by the other segment's
squared length, 0 for a point).  Golden section on t in [0, 1], 200 iterations, the minimum over every point evaluated and both end
points.  No Gram determinant, no candidate list, no reciprocal of a half-axis component.

CLASSES (`classes`; each must hold >= MIN_CLASS rows, so that no comparison below is vacuous).
  parallel        both segments have a length and h1 x h2 = 0 exactly
  near_parallel   both have a length and sin^2(angle) < 2^-23 (the Gram determinant a e - b^2 is rounding noise; includes `parallel`)
  sphere_first / sphere_second / both_spheres   by the shape
  zero_ref        the reference distance is exactly 0
  h_zero          a component of the moving half-axis is exactly 0
  h_sq_subnormal  a component of the moving half-axis whose fp32 square is subnormal (0 < h_i^2 < 2^-126)
The half-axis is the device's own: the fp32 link rotation of the fp32 oracle times the link-frame half-axis, which has one non-zero
component, so the product is reproduced exactly.

BARS.  u = 2^-23, ext = the largest absolute coordinate among the row's end points (and box corners), scale = u (d_ref + ext).

  FIRST TIER, the form this sweep was set up to pin:
    segment-box, and segment-segment outside near_parallel:   |d - d_ref| <= KAPPA scale
    near_parallel:   -KAPPA scale <= d - d_ref <= sqrt(d_ref^2 + delta^2) - d_ref + KAPPA scale,  delta = KAPPA_P sqrt(u) min(|h1|, |h2|)
  with KAPPA, KAPPA_P = twice what the fp32 oracle needs on this sweep (the device must equal that oracle bit for bit, so the margin
  only has to cover a reseeded sweep).  MEASURED: the rows outside near_parallel need 1157.6 (segment-segment; segment-box alone 0.99),
  so KAPPA = 2320, and with that KAPPA the near_parallel rows need no delta at all: KAPPA_P = 0.  FINDING: this form does not describe
  the function.  (1) The loss of accuracy does not end at sin^2 = 2^-23: it decays as 1 / sin(angle) and is still 60 scale at
  sin^2 = 1e-4, which is where the 1157.6 comes from (a row at sin^2 = 2.6e-7: 3.1e-5 m at d_ref = 1.1e-5 m).  (2) Inside the class the
  overestimate is LINEAR in the misplacement, not of the form sqrt(d^2 + delta^2) - d: two near-parallel lines that converge change
  their distance by sin(angle) per unit length, so 7.1e-6 m is overestimated at d_ref = 1.19 m just as it would be at d_ref = 0; to
  fit the quadratic form there, KAPPA_P would have to be 577.  The first tier is kept as stated, with the constants its recipe gives;
  it still fails the sphere-second fault (0.2 m).  The second tier is the bound that has teeth.

  SECOND TIER, derived from the formula (KT, KS measured, the 2 is not):
    every row:            d - d_ref >= -KT scale                                    (no path underestimates)
    segment-box, and segment-segment with a sphere in the pair:   |d - d_ref| <= KT scale    (no Gram determinant: nothing cancels)
    both with a length:   d - d_ref <= KT scale + min(2 hmin sin(angle), KS u ext / sin(angle)),   hmin = min(|h1|, |h2|)
  The only ill-conditioned quantity is s, the parameter on the first segment, a quotient by the Gram determinant a e - b^2 =
  a e sin^2(angle), which is formed with an absolute error of about u a e.  t is then the exact projection of that point on the
  second line, so what is returned is the distance from a misplaced point of the first segment to the second LINE, and that distance
  changes by at most sin(angle) per unit length along the first segment.  The misplacement is at most the span of the shorter segment,
  2 hmin (beyond it t leaves [-1, 1] and s is recomputed from 1 / a without the determinant), and otherwise about u ext / sin^2(angle).
  Exactly parallel lines (sin = 0) lose nothing.  The worst case, where both terms of the min meet, is sqrt(2 hmin KS u ext):
  1.4e-4 m for half-lengths 0.2 and 0.5 at ext = 0.6, always an overestimate -- more clearance reported than there is.
  MEASURED (fp32 oracle, this sweep): max |d - d_ref| / scale on segment-box 0.99, with a sphere in the pair 0.83; the largest
  underestimate 0.83 scale; on the rows with two lengths max overshoot / (hmin sin) = 1.99 (the derived 2 is attained: s really lands
  anywhere on the shorter span) and max overshoot sin / (u ext) = 0.78.  KT = 2 and KS = 2: twice the measured maxima, rounded up.
tests/test_capsule_domain_model.py prints all of these (pytest -s); tests/test_gpu_capsule_domain.py prints the device's, which are
the same figures because the device returns the same bits.
"""

import functools

import numpy as np

from tests import helpers as H

U = 2.0**-23
KAPPA, KAPPA_P = 2320.0, 0.0  # first tier (module docstring)
KT, KS = 2.0, 2.0  # second tier
N_ROWS = 16384
MIN_CLASS = 64
SEED = 5150
f32 = np.float32

BASES = {"seg": ((-0.2, 0.0, 0.0), (0.2, 0.0, 0.0)), "sph": ((0.1, 0.0, 0.0), (0.1, 0.0, 0.0))}
MOVING = {"h15": ((-0.15, 0.0, 0.0), (0.15, 0.0, 0.0)), "h50": ((-0.5, 0.0, 0.0), (0.5, 0.0, 0.0)),
          "h02": ((-0.02, 0.0, 0.0), (0.02, 0.0, 0.0)), "sph": ((0.1, 0.05, 0.0), (0.1, 0.05, 0.0))}  # fmt: skip
SHAPES = tuple((b, m) for b in BASES for m in MOVING)
RADII = (0.03, 0.05)  # the one variant with radii: the mask-only threshold path then has hits to decide
RTC_SHAPES = (("seg", "h15"), ("seg", "sph"))  # the two shapes that also run specialised (hipRTC) kernels; the second has a sphere second

# axis-aligned boxes as world-frame corners (lo, hi); lattice-aligned (multiples of 1/16) where rows are meant to graze exactly
BOXES = {
    "cube": ((0.25, -0.125, 0.0), (0.5, 0.125, 0.25)),  # 25 cm
    "flat": ((-0.5, -0.5, -0.3125), (0.5, 0.5, -0.25)),
    "voxel": ((0.25, 0.0625, 0.125), (0.258, 0.0705, 0.133)),  # 8 mm
    "slab": ((-1.0, -1.0, -0.0625), (1.0, 1.0, 0.0625)),  # holds the segments that lie in the plane z = 0 near the origin
    "point": ((0.25, 0.125, -0.0625), (0.25, 0.125, -0.0625)),
}
SCENE_SIZE, SCENE_SLOT = 65, 37  # scene_env_collisions: the cube in slot 37 of a scene padded with far clutter to 65 cuboids


def free_capsule_spec(base, moving, radii=(0.0, 0.0)):
    from cppflow_amd.robot_model import CapsuleSpec, JointSpec, RobotSpec

    eye = ((1, 0, 0), (0, 1, 0), (0, 0, 1))
    joints = [JointSpec(f"p{n}", f"lp{n}", (0, 0, 0), (0, 0, 0), ax, "prismatic", (-4.0, 4.0)) for n, ax in zip("xyz", eye)]
    joints += [JointSpec(f"r{n}", f"lr{n}", (0, 0, 0), (0, 0, 0), ax, "revolute", (-7.0, 7.0)) for n, ax in zip("zyx", eye[::-1])]
    joints.append(JointSpec("tool", "tool", (0, 0, 0.125), (0, 0, 0), jtype="fixed"))
    caps = [CapsuleSpec("base", *BASES[base], radii[0]), CapsuleSpec("lrx", *MOVING[moving], radii[1])]
    return RobotSpec(f"free_{base}_{moving}", "a free capsule", "base", joints, caps, collision_pairs=[(0, 1)])


@functools.lru_cache(maxsize=None)
def chain(base, moving, radii=(0.0, 0.0)):
    from cppflow_amd.robot_model import canonicalize

    return canonicalize(free_capsule_spec(base, moving, radii))


@functools.lru_cache(maxsize=None)
def oracle(base, moving, is_f32=True, radii=(0.0, 0.0)):
    from oracle.oracle import Oracle

    return Oracle(chain(base, moving, radii), f32=is_f32, threads=8)


def box_obstacle(name):
    """(cuboid [6], Tcuboid [4,4]) with a zero translation: the library's corners t + c are then the fp32 values of BOXES[name]"""
    lo, hi = BOXES[name]
    T = np.zeros((4, 4), dtype=np.float32)
    T[:3, :3] = np.eye(3, dtype=np.float32)
    return np.array([*lo, *hi], dtype=np.float32), T


def box_corners(name):
    c, T = box_obstacle(name)
    lo, hi = H.box_corners([c], [T])
    return lo[0], hi[0]


def mask_boxes():
    """(lo, hi) [4,3] of the boxes the variant with radii is masked against: all but the slab, which holds the base capsule"""
    lo, hi = zip(*(box_corners(b) for b in BOXES if b != "slab"))
    return np.array(lo), np.array(hi)


@functools.lru_cache(maxsize=None)
def scene_corners():
    """(lo, hi) [65,3] fp32-valued float64: far clutter (6 .. 8 m from the origin; the rows stay within 2 m of it) around the cube"""
    rng = np.random.RandomState(SEED + 1)
    d = rng.randn(SCENE_SIZE, 3)
    centre = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(6.0, 8.0, (SCENE_SIZE, 1))
    half = rng.uniform(0.02, 0.3, (SCENE_SIZE, 3))
    lo, hi = H.f32(centre - half), H.f32(centre + half)
    lo[SCENE_SLOT], hi[SCENE_SLOT] = box_corners("cube")
    lo.setflags(write=False), hi.setflags(write=False)
    return lo, hi


# ---- the rows ---------------------------------------------------------------------------------------------------------------------
SPECIAL_ANGLES = (0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, np.pi / 4)


def _sign(rng, n):
    return rng.choice([-1.0, 1.0], size=n)


def _special_angles(rng, n):
    """one of SPECIAL_ANGLES in fp32: itself, one of its +-1 .. 3 fp32 neighbours (of 0: the smallest subnormals), or plus an offset of
    +-10^U(-30, -2) (next to 0 the squares of the half-axis components this gives are subnormal or zero; elsewhere it rounds away)"""
    v = np.asarray(rng.choice(SPECIAL_ANGLES, size=n), dtype=np.float32)
    kind = rng.randint(0, 3, size=n)
    steps = rng.randint(1, 4, size=n) * (kind == 1)
    toward = np.where(rng.randint(0, 2, size=n) == 0, -np.inf, np.inf).astype(np.float32)
    for k in (1, 2, 3):
        v = np.where(steps >= k, np.nextafter(v, toward), v)
    off = _sign(rng, n) * 10.0 ** rng.uniform(-30, -2, size=n)
    return np.where(kind == 2, v.astype(np.float64) + off, v.astype(np.float64))


def _lattice(rng, shape, span):
    """multiples of 1/16 within +-span/16 (they graze exactly), half of them plus +-10^U(-30, -3)"""
    lat = rng.randint(-span, span + 1, size=shape) / 16.0
    off = _sign(rng, shape) * 10.0 ** rng.uniform(-30, -3, size=shape)
    return np.where(rng.randint(0, 2, size=shape) == 0, lat, lat + off)


FAMILIES = (("special", 6144), ("special_far", 1536), ("collinear", 512), ("generic", 4096), ("near_parallel", 3584), ("parallel", 512))


@functools.lru_cache(maxsize=None)
def rows(seed=SEED):
    """(q [N_ROWS, 6] fp32-representable float64, family [N_ROWS] of str); seeded, the same for every shape"""
    rng = np.random.RandomState(seed)
    qs, fam = [], []
    for name, n in FAMILIES:
        q = np.zeros((n, 6))
        if name in ("special", "special_far"):
            q[:, :3] = _lattice(rng, (n, 3), 8 if name == "special" else 16)
            for j in (3, 4, 5):
                q[:, j] = _special_angles(rng, n)
        elif name == "collinear":  # on the base capsule's line, unrotated (roll does not move the x axis): overlaps, touches, gaps
            q[:, 0] = rng.randint(-12, 13, size=n) / 16.0
            q[:, 5] = _special_angles(rng, n)
        elif name == "generic":
            q[:, :3] = rng.uniform(-1.0, 1.0, size=(n, 3))
            q[:, 3:] = rng.uniform(-np.pi, np.pi, size=(n, 3))
        else:  # yaw in {0, +-pi} plus 10^U(-8, -2), a small pitch, small offsets; "parallel": yaw = pitch = 0 exactly
            q[:, 0] = rng.uniform(-0.8, 0.8, size=n)
            small = _sign(rng, (n, 2)) * 10.0 ** rng.uniform(-6, -1, size=(n, 2))
            q[:, 1:3] = np.where(rng.randint(0, 4, size=(n, 2)) == 0, rng.randint(-2, 3, size=(n, 2)) / 16.0, small)
            q[:, 5] = rng.uniform(-np.pi, np.pi, size=n)
            if name == "near_parallel":
                q[:, 3] = rng.choice([0.0, np.pi, -np.pi], size=n) + _sign(rng, n) * 10.0 ** rng.uniform(-8, -2, size=n)
                q[:, 4] = np.where(rng.randint(0, 4, size=n) == 0, 0.0, _sign(rng, n) * 10.0 ** rng.uniform(-8, -2, size=n))
        qs.append(q)
        fam += [name] * n
    q = H.f32(np.concatenate(qs))
    assert q.shape == (N_ROWS, 6) and np.abs(q[:, :3]).max() <= 1.0 + 1e-3 and np.abs(q[:, 3:]).max() < 7.0
    q.setflags(write=False)
    return q, np.array(fam)


# ---- the reference ----------------------------------------------------------------------------------------------------------------
GOLDEN_ITERATIONS = 200
_INVPHI = (np.sqrt(5.0) - 1.0) / 2.0


def golden_min(f, n):
    """min over t in [0, 1] of the convex f (vectorised over n rows): golden section, and the least value seen at any point, 0 and 1"""
    a, b = np.zeros(n), np.ones(n)
    c, d = b - _INVPHI * (b - a), a + _INVPHI * (b - a)
    fc, fd = f(c), f(d)
    best = np.minimum(np.minimum(f(a), f(b)), np.minimum(fc, fd))
    for _ in range(GOLDEN_ITERATIONS):
        left = fc <= fd  # the minimum lies in [a, d]; otherwise in [c, b]
        b, a = np.where(left, d, b), np.where(left, a, c)
        x = np.where(left, b - _INVPHI * (b - a), a + _INVPHI * (b - a))
        fx = f(x)
        best = np.minimum(best, fx)
        c, d, fc, fd = np.where(left, x, d), np.where(left, c, x), np.where(left, fx, fd), np.where(left, fc, fx)
    return best


def point_segment_distance(p, b0, b1):
    u = b1 - b0
    uu = (u * u).sum(axis=1)
    s = np.clip(((p - b0) * u).sum(axis=1) / np.where(uu > 0, uu, 1.0), 0.0, 1.0)  # (a point: u = 0, so s = 0)
    return np.linalg.norm(p - (b0 + s[:, None] * u), axis=1)


def ref_segment_segment(a0, a1, b0, b1):
    """fp64 distance between the segments a0-a1 and b0-b1, [n,3] each"""
    return golden_min(lambda t: point_segment_distance(a0 + t[:, None] * (a1 - a0), b0, b1), len(a0))


def ref_segment_box(a0, a1, lo, hi):
    def f(t):
        p = a0 + t[:, None] * (a1 - a0)
        return np.linalg.norm(p - np.clip(p, lo, hi), axis=1)

    return golden_min(f, len(a0))


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def geometry(moving):
    """what the device holds for the moving capsule at every row: fp32 end points [n,6] and the fp32 world half-axis [n,3]"""
    q, _ = rows()
    orc, ch = oracle("seg", moving), chain("seg", moving)
    ends = orc.capsule_endpoints(q)[:, 1]
    li = int(ch.cap_link[1])
    R = orc.link_frames(q)[:, li, :9].reshape(-1, 3, 3)
    h = (0.5 * (ch.cap_p1[1] - ch.cap_p0[1])).astype(np.float32).astype(np.float64)  # capsule_centred: rounded to fp32 once
    assert np.count_nonzero(h) <= 1  # R h is then ONE fp32 product per component (the two fused additions of an exact 0 change nothing)
    hw = (R @ h).astype(np.float32).astype(np.float64)
    ext = np.abs(ends).max(axis=1)
    assert (np.abs(0.5 * (ends[:, 3:] - ends[:, :3]) - hw).max(axis=1) <= U * ext).all()  # the same capsule, up to the rounding of c +- h
    return _frozen(dict(ends=ends, hw=hw))


@functools.lru_cache(maxsize=None)
def reference_ss(base, moving):
    """segment-segment reference of one shape over the rows: dict(d, ext, hmin, sin, both [with a length], near, parallel)"""
    g = geometry(moving)
    b0, b1 = (np.tile(H.f32(p), (N_ROWS, 1)) for p in BASES[base])
    a0, a1 = g["ends"][:, :3], g["ends"][:, 3:]
    h1, h2 = 0.5 * (b1 - b0), g["hw"]
    n1, n2 = (h1 * h1).sum(axis=1), (h2 * h2).sum(axis=1)
    cr = np.cross(h1, h2)
    both = (n1 > 0) & (n2 > 0)
    sin2 = (cr * cr).sum(axis=1) / np.where(both, n1 * n2, 1.0)
    ext = np.maximum(np.abs(g["ends"]).max(axis=1), max(np.abs(b0).max(), np.abs(b1).max()))
    return _frozen(dict(d=ref_segment_segment(a0, a1, b0, b1), ext=ext, hmin=np.sqrt(np.minimum(n1, n2)), both=both, sin=np.sqrt(sin2),
                        near=both & (sin2 < U), parallel=both & (cr == 0).all(axis=1)))  # fmt: skip


@functools.lru_cache(maxsize=None)
def reference_box(moving, box):
    g = geometry(moving)
    lo, hi = box_corners(box)
    ext = np.maximum(np.abs(g["ends"]).max(axis=1), max(np.abs(lo).max(), np.abs(hi).max()))
    return _frozen(dict(d=ref_segment_box(g["ends"][:, :3], g["ends"][:, 3:], lo, hi), ext=ext))


def classes(base, moving):
    """{class: bool [N_ROWS]} of one shape (module docstring)"""
    ref, hw = reference_ss(base, moving), geometry(moving)["hw"]
    all_rows = np.ones(N_ROWS, dtype=bool)
    s1, s2 = BASES[base][0] == BASES[base][1], MOVING[moving][0] == MOVING[moving][1]
    h32 = hw.astype(np.float32)
    sq = h32 * h32
    assert sq.dtype == np.float32
    return dict(parallel=ref["parallel"], near_parallel=ref["near"], sphere_first=all_rows & (s1 and not s2),
                sphere_second=all_rows & (s2 and not s1), both_spheres=all_rows & (s1 and s2), zero_ref=ref["d"] == 0,
                h_zero=(hw == 0).any(axis=1) & (not s2), h_sq_subnormal=((sq > 0) & (sq < np.finfo(np.float32).tiny)).any(axis=1))  # fmt: skip


# ---- bars -------------------------------------------------------------------------------------------------------------------------
def _allowance(d_ref, delta):
    return delta * delta / (np.sqrt(d_ref * d_ref + delta * delta) + d_ref + 1e-300)  # sqrt(d^2 + delta^2) - d without cancellation


def _gram_slack(ref):
    """min(2 hmin sin, KS u ext / sin) on the rows where both segments have a length, 0 elsewhere (and for a box)"""
    if "sin" not in ref:
        return np.zeros(len(ref["d"]))
    with np.errstate(divide="ignore"):
        return np.where(ref["both"], np.minimum(2.0 * ref["hmin"] * ref["sin"], KS * U * ref["ext"] / ref["sin"]), 0.0)


def measure(d, ref):
    """what the distances d [n] need of every constant of the module docstring, as a dict of maxima over the rows"""
    d = np.asarray(d, dtype=np.float64)
    n = len(d)
    near, both = ref.get("near", np.zeros(n, dtype=bool)), ref.get("both", np.zeros(n, dtype=bool))
    scale = U * (ref["d"] + ref["ext"])
    err = d - ref["d"]
    out = dict(kappa=float((np.abs(err) / scale)[~near].max()), under=float((-err / scale).max()), kappa_p=0.0, lin=0.0, ks=0.0,
               kt=float((np.abs(err) / scale)[~both].max()) if (~both).any() else 0.0)  # fmt: skip
    if near.any():
        over = np.maximum(err - KAPPA * scale, 0.0)[near]  # what is left for sqrt(d_ref^2 + delta^2) - d_ref to cover
        out["kappa_p"] = float((np.sqrt(over * (over + 2.0 * ref["d"][near])) / (np.sqrt(U) * ref["hmin"][near])).max())
    pos = both & (ref.get("sin", np.zeros(n)) > 0)
    if pos.any():
        over = np.maximum(err - KT * scale, 0.0)[pos]
        out["lin"] = float((over / (ref["hmin"] * ref["sin"])[pos]).max())
        out["ks"] = float((over * ref["sin"][pos] / (U * ref["ext"][pos])).max())
    return out


def check(d, ref, label="", tiers=(1, 2)):
    """asserts the bars of the module docstring on the distances d [n] of one shape (or of one moving capsule and one box)"""
    d = np.asarray(d, dtype=np.float64)
    assert d.shape == ref["d"].shape and np.isfinite(d).all(), label
    scale = U * (ref["d"] + ref["ext"])
    err = d - ref["d"]
    near = ref.get("near", np.zeros(len(d), dtype=bool))
    uppers = {1: KAPPA * scale + np.where(near, _allowance(ref["d"], KAPPA_P * np.sqrt(U) * ref.get("hmin", 0.0)), 0.0),
              2: KT * scale + _gram_slack(ref)}  # fmt: skip
    lowers = {1: -KAPPA * scale, 2: -KT * scale}
    for tier in tiers:
        i, j = int(np.argmin(err - lowers[tier])), int(np.argmax(err - uppers[tier]))
        assert (err >= lowers[tier]).all(), (label, "tier", tier, "underestimate, row", i, "got", d[i], "want", ref["d"][i], "bar", lowers[tier][i])
        assert (err <= uppers[tier]).all(), (label, "tier", tier, "overestimate, row", j, "got", d[j], "want", ref["d"][j], "bar", uppers[tier][j])


# ---- a restatement of the segment-segment formula (fp64 numpy), with the fault it used to have --------------------------------------
def seg_seg_restated(a0, a1, b0, b1, sphere_second_fix=True):
    """seg_seg_closest2 on centres and half-axes, parameters in [-1, 1]; `sphere_second_fix=False` is the formula as it was: s = 0
    (the first segment's centre) whenever the Gram determinant vanishes, also where the second capsule is a sphere"""
    def rcp(v):
        return np.where(v >= 2.0**-100, 1.0 / np.where(v >= 2.0**-100, v, 1.0), 0.0)

    c1, h1, c2, h2 = 0.5 * (a0 + a1), 0.5 * (a1 - a0), 0.5 * (b0 + b1), 0.5 * (b1 - b0)
    rr = c1 - c2
    a, e = (h1 * h1).sum(axis=1), (h2 * h2).sum(axis=1)
    ia, ie = rcp(a), rcp(e)
    b, c, f = (h1 * h2).sum(axis=1), (h1 * rr).sum(axis=1), (h2 * rr).sum(axis=1)
    s = np.clip((b * f - c * e) * rcp(a * e - b * b), -1.0, 1.0)
    t = (b * s + f) * ie
    s = np.where(t < -1, np.clip(-(b + c) * ia, -1.0, 1.0), np.where(t > 1, np.clip((b - c) * ia, -1.0, 1.0), s))
    if sphere_second_fix:
        s = np.where(ie == 0, np.clip(-c * ia, -1.0, 1.0), s)
    t = np.clip(t, -1.0, 1.0)
    return np.linalg.norm(rr + s[:, None] * h1 - t[:, None] * h2, axis=1)
