"""Emit csrc/robots_gen.h: compile-time tables of the shipped robots' canonical chains.

The heavy kernels are instantiated once per shipped robot with these tables as `static constexpr` data.  After full
unrolling every chain constant is a literal, so (a) the 0 / +-1 entries of the fixed transforms fold away (Panda's
joint frames differ by +-90 degree rolls: R*F becomes a signed column permutation, no arithmetic), (b) no constant
competes for SGPRs or is re-fetched through the scalar cache every LM iteration, (c) capsule end points are indexed by
compile-time ids and stay in VGPRs instead of LDS.  `cppf_robot_create` picks a table by exact comparison with the
description it is handed; anything else runs the generic (kernel-argument-driven) instantiation.

Run by cppflow_amd.build before hipcc; the output is committed so that a bare `hipcc` of csrc/ also works.
"""

import os

import numpy as np

from cppflow_amd.robot_model import CanonicalChain, canonicalize
from cppflow_amd.robot_zoo import ROBOT_SPECS

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "robots_gen.h")
ORDER = ["panda", "fetch", "fetch_arm", "chain12"]


def _f(v) -> str:
    """Exact fp32 literal (C99 hex float)."""
    v = float(np.float32(v))
    if v == 0.0:
        return "0.0f"
    if v == 1.0:
        return "1.0f"
    if v == -1.0:
        return "-1.0f"
    return v.hex() + "f"


def _arr(vals) -> str:
    return "{" + ", ".join(_f(v) for v in vals) + "}"


def sqrt_threshold(r) -> np.float32:
    """Smallest fp32 y with sqrt_rn(y) >= r: then for every fp32 d2 >= 0,  sqrtf(d2) - r < 0  <=>  d2 < y  exactly
    (correctly rounded sqrt is monotone).  Lets the mask-only kernels skip the square root without changing a single bit
    of the masks the sqrt-based definition (collision_detection.py:66-68: `min_dists < 0`) produces."""
    r = np.float32(r)
    if r <= 0:
        return np.float32(0.0)
    y = np.float32(r * r)
    while np.sqrt(y) >= r:
        y = np.nextafter(y, np.float32(0.0))
    while np.sqrt(y) < r:
        y = np.nextafter(y, np.float32(np.inf))
    return y


def cull_threshold(reach: float) -> np.float32:
    """Broad-phase threshold on a squared mid-point distance: (reach + 1 cm)^2 (1 + 1e-4), rounded up to fp32 (reach = half
    lengths + radii).  Conservative by construction -- see cull_far in csrc/kernels_collision.h."""
    y = (float(reach) + 0.01) ** 2 * (1.0 + 1e-4)
    f = np.float32(y)
    if float(f) < y:
        f = np.nextafter(f, np.float32(np.inf))
    return f


def inside_threshold(r) -> np.float32:
    """Certain-hit threshold on the squared distance of a capsule's CENTRE from a cuboid: max(r - 1 cm, 0)^2 (1 - 1e-4), rounded down
    to fp32 -- the mirror image of cull_threshold.  The segment contains its centre, so a centre closer than r - 1 cm puts the exact
    test 1 cm inside its threshold; r <= 1 cm gives 0 and `d2 < 0` never holds (env_item_undecided in csrc/kernels_collision.h)."""
    y = max(float(r) - 0.01, 0.0) ** 2 * (1.0 - 1e-4)
    f = np.float32(y)
    if float(f) > y:
        f = np.nextafter(f, np.float32(0.0))
    return f


def capsule_centred(cap_p0, cap_p1):
    """(centre, half-axis, |h|^2, 1 / |h|^2) of every capsule as the kernels use them: double arithmetic on the fp32 end points,
    each rounded to fp32 once -- c = 0.5 (p0 + p1), h = 0.5 (p1 - p0), a = (h0 h0 + h1 h1) + h2 h2 over the ROUNDED h, 1 / a (0 when a < 2^-100).
    The same four lines are in csrc/cppflow_hip.hip (capsule_centred) and oracle/lmik_oracle.c (orc_robot_create)."""
    p0 = np.asarray(cap_p0, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    p1 = np.asarray(cap_p1, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    c = (0.5 * (p0 + p1)).astype(np.float32)
    h = (0.5 * (p1 - p0)).astype(np.float32)
    hd = h.astype(np.float64)
    a = (hd[:, 0] * hd[:, 0] + hd[:, 1] * hd[:, 1]) + hd[:, 2] * hd[:, 2]
    ia = np.where(a >= 2.0**-100, 1.0 / np.maximum(a, 2.0**-100), 0.0)  # a zero-length capsule is a sphere: its parameter stays 0
    return c, h, a.astype(np.float32), ia.astype(np.float32), np.sqrt(a)


# ---- self pairs that can never touch inside the joint limits ----------------------------------------------------------------------
# pair_never[pi]: dist(seg_a, seg_b) - (r_a + r_b) >= CERT_MARGIN for EVERY q in [lo, hi], proved (not sampled) by branch and bound in
# float64 on the canonical chain.  1 cm is the slack the broad phase already relies on (cull_far in csrc/kernels_collision.h): with it
# the exact fp32 test of such a pair could only have said "no hit", so a mask-only launch whose rows are clamped to the limits drops
# the pair at compile time.  The distance of a pair depends on the joints between its two links only (joints 0 .. link_b for a base
# capsule); capsule a is at rest in its own link's frame, and when joint k alone moves by dq every point of capsule b moves by at
# most |dq| rho_k, rho_k = a bound on the point's distance from joint k's axis (1 per unit for a prismatic joint).  The distance of
# two segments is 1-Lipschitz in the displacement of one of them, so over a box of half-widths w about a centre c
#     dist(q) >= dist(c) - sum_k w_k rho_k.
# A box whose bound clears the margin is accepted, any other is halved along its widest (w rho) side; the search gives up -- the pair
# stays live -- on a centre below the margin, after CERT_MAX_BOXES boxes, or when more than CERT_MAX_DIMS joints lie between the links
# (the box count grows with the power of the dimension; generate() runs on every CPU test run and has to stay within seconds).
CERT_MARGIN = 0.01
CERT_SLACK = 1e-6  # float64 rounding of the chain and of the distance is below 1e-12; three digits of the margin are not worth arguing
CERT_MAX_DIMS = 4  # with 100 000 boxes: 1.8 s for the four shipped robots, 0.4 s of it Panda (12 of its 25 pairs certified)
CERT_MAX_BOXES = 100000


def _seg_point_dist2(p, a, d, dd):
    """squared distance of the points p [N, 3] from the segments a + u d, u in [0, 1] (dd = |d|^2, may be 0)"""
    u = np.clip(np.einsum("ij,ij->i", p - a, d) / np.where(dd > 0, dd, 1.0), 0.0, 1.0) * (dd > 0)
    e = p - (a + u[:, None] * d)
    return np.einsum("ij,ij->i", e, e)


def segment_distance(p1, q1, p2, q2):
    """Distance of the segments p1 q1 and p2 q2 ([N, 3] each, float64): the interior critical point where the segments are not
    parallel (Ericson 5.1.9), and the four end-point-to-segment distances, whichever is smallest -- the minimum is always one of them."""
    d1, d2, r = q1 - p1, q2 - p2, p1 - p2
    a, e = np.einsum("ij,ij->i", d1, d1), np.einsum("ij,ij->i", d2, d2)
    b, c, f = np.einsum("ij,ij->i", d1, d2), np.einsum("ij,ij->i", d1, r), np.einsum("ij,ij->i", d2, r)
    den = a * e - b * b
    ok = den > 1e-12 * np.maximum(a * e, 1e-300)
    s = np.clip(np.where(ok, (b * f - c * e) / np.where(ok, den, 1.0), 0.0), 0.0, 1.0)
    t = np.clip(np.where(e > 0, (b * s + f) / np.where(e > 0, e, 1.0), 0.0), 0.0, 1.0)
    g = (p1 + s[:, None] * d1) - (p2 + t[:, None] * d2)
    best = np.einsum("ij,ij->i", g, g)
    for v in (_seg_point_dist2(p1, p2, d2, e), _seg_point_dist2(q1, p2, d2, e), _seg_point_dist2(p2, p1, d1, a), _seg_point_dist2(q2, p1, d1, a)):
        best = np.minimum(best, v)
    return np.sqrt(best)


def pair_joints(ch: CanonicalChain, a: int, b: int):
    """(the capsule on the nearer link, the one on the farther link, the joints between them) of the pair (a, b)"""
    if ch.cap_link[a] > ch.cap_link[b]:
        a, b = b, a
    return a, b, list(range(int(ch.cap_link[a]) + 1, int(ch.cap_link[b]) + 1))


def _pair_clearance(ch: CanonicalChain, a: int, b: int, joints, q):
    """clearance of the pair at the configurations q [N, len(joints)] of the joints between its links (capsule a's link frame)"""
    n = q.shape[0]
    R = np.broadcast_to(np.eye(3), (n, 3, 3))
    p = np.zeros((n, 3))
    for i, j in enumerate(joints):
        F = ch.F[j]
        p = p + R @ F[9:12]
        R = R @ F[:9].reshape(3, 3)
        if ch.jtype[j] == 1:
            p = p + R[:, :, 2] * q[:, i : i + 1]
        else:
            cs, sn = np.cos(q[:, i]), np.sin(q[:, i])
            M = np.zeros((n, 3, 3))
            M[:, 0, 0], M[:, 0, 1], M[:, 1, 0], M[:, 1, 1], M[:, 2, 2] = cs, -sn, sn, cs, 1.0
            R = R @ M
    b0, b1 = p + R @ ch.cap_p0[b], p + R @ ch.cap_p1[b]
    a0, a1 = np.broadcast_to(ch.cap_p0[a], (n, 3)), np.broadcast_to(ch.cap_p1[a], (n, 3))
    return segment_distance(a0, a1, b0, b1) - (ch.cap_r[a] + ch.cap_r[b])


def pair_travel_bounds(ch: CanonicalChain, b: int, joints):
    """rho_k for each of `joints` (the last of them carries capsule b): how far a point of the capsule moves per unit of joint k"""
    reach = max(np.linalg.norm(ch.cap_p0[b]), np.linalg.norm(ch.cap_p1[b]))  # bound on |point| in the frame of the link
    rho = []
    for j in reversed(joints):
        rho.append(1.0 if ch.jtype[j] == 1 else reach)
        if ch.jtype[j] == 1:
            reach += max(abs(ch.lo[j]), abs(ch.hi[j]))
        reach += np.linalg.norm(ch.F[j][9:12])
    return np.array(rho[::-1])


def certify_pair(ch: CanonicalChain, a: int, b: int, margin: float = CERT_MARGIN, max_dims: int = CERT_MAX_DIMS,
                 max_boxes: int = CERT_MAX_BOXES) -> bool:
    """True only with a proof that the pair keeps `margin` of clearance over the whole joint box (see above); deterministic."""
    a, b, joints = pair_joints(ch, a, b)
    if not joints:  # same link: a constant
        return bool(_pair_clearance(ch, a, b, joints, np.zeros((1, 0)))[0] >= margin + CERT_SLACK)
    if len(joints) > max_dims or not np.all(ch.hi[joints] >= ch.lo[joints]):
        return False
    rho = pair_travel_bounds(ch, b, joints)
    c = 0.5 * (ch.lo[joints] + ch.hi[joints])[None]
    w = 0.5 * (ch.hi[joints] - ch.lo[joints])[None]
    done = 0
    while c.shape[0]:
        done += c.shape[0]
        if done > max_boxes:
            return False
        d = _pair_clearance(ch, a, b, joints, c)
        if np.any(d < margin + CERT_SLACK):
            return False
        open_ = d - (w * rho).sum(axis=1) < margin + CERT_SLACK
        c, w = c[open_], w[open_]
        k = np.argmax(w * rho, axis=1)
        rows = np.arange(c.shape[0])
        w[rows, k] *= 0.5
        lo_half, hi_half = c.copy(), c.copy()
        lo_half[rows, k] -= w[rows, k]
        hi_half[rows, k] += w[rows, k]
        c, w = np.concatenate([lo_half, hi_half]), np.concatenate([w, w])
    return True


def pair_never(ch: CanonicalChain):
    """the certificate of every pair of the chain, in pair order (the table's pair_never)"""
    return [certify_pair(ch, int(a), int(b)) for a, b in ch.pairs]


def emit_robot(name: str, ch: CanonicalChain) -> str:
    d, L, P = ch.ndof, ch.n_capsules, ch.n_pairs
    cname = "".join(p.capitalize() for p in name.split("_"))
    s = [f"struct {cname} {{"]
    s.append(f'    static constexpr const char* name = "{name}";')
    s.append(f"    static constexpr int D = {d}, L = {L}, P = {P};")
    s.append(f"    static constexpr uint32_t pris_mask = {sum(1 << j for j in range(d) if ch.jtype[j] == 1)}u;")
    s.append(f"    static constexpr float F[{d}][12] = {{")
    for j in range(d):
        s.append("        " + _arr(ch.F[j]) + ",")
    s.append("    };")
    s.append(f"    static constexpr float Fee[12] = {_arr(ch.F_ee)};")
    s.append(f"    static constexpr float lo[{d}] = {_arr(ch.lo)};")
    s.append(f"    static constexpr float hi[{d}] = {_arr(ch.hi)};")
    Lm, Pm = max(L, 1), max(P, 1)
    s.append(f"    static constexpr int cap_link[{Lm}] = {{" + ", ".join(str(int(v)) for v in (ch.cap_link if L else [0])) + "};")
    s.append(f"    static constexpr float cap_p0[{Lm}][3] = {{" + ", ".join(_arr(v) for v in (ch.cap_p0 if L else [[0, 0, 0]])) + "};")
    s.append(f"    static constexpr float cap_p1[{Lm}][3] = {{" + ", ".join(_arr(v) for v in (ch.cap_p1 if L else [[0, 0, 0]])) + "};")
    s.append(f"    static constexpr float cap_r[{Lm}] = {_arr(ch.cap_r if L else [0])};")
    cc, hh, aa, ia, half = capsule_centred(ch.cap_p0, ch.cap_p1) if L else (np.zeros((1, 3)), np.zeros((1, 3)), [0], [0], [])
    s.append(f"    static constexpr float cap_c[{Lm}][3] = {{" + ", ".join(_arr(v) for v in cc) + "};  // centre 0.5 (p0 + p1)")
    s.append(f"    static constexpr float cap_h[{Lm}][3] = {{" + ", ".join(_arr(v) for v in hh) + "};  // half-axis 0.5 (p1 - p0)")
    s.append(f"    static constexpr float cap_a[{Lm}] = {_arr(aa)};  // |h|^2")
    s.append(f"    static constexpr float cap_ia[{Lm}] = {_arr(ia)};  // 1 / |h|^2")
    r32 = ch.cap_r.astype(np.float32)
    pair_thr = [sqrt_threshold(np.float32(r32[a] + r32[b])) for a, b in ch.pairs] if P else [0]
    cap_thr = [sqrt_threshold(r) for r in r32] if L else [0]
    s.append(f"    static constexpr float pair_thr[{Pm}] = {_arr(pair_thr)};  // sqrt thresholds of r_a + r_b")
    s.append(f"    static constexpr float cap_thr[{Lm}] = {_arr(cap_thr)};  // sqrt thresholds of r")
    pair_cull = [cull_threshold(half[a] + half[b] + float(r32[a]) + float(r32[b])) for a, b in ch.pairs] if P else [0]
    cap_cull = [cull_threshold(half[c] + float(r32[c])) for c in range(L)] if L else [0]
    s.append(f"    static constexpr float pair_cull[{Pm}] = {_arr(pair_cull)};  // broad phase, pairs")
    s.append(f"    static constexpr float cap_cull[{Lm}] = {_arr(cap_cull)};  // broad phase, capsule vs cuboid")
    cap_in = [inside_threshold(r) for r in r32] if L else [0]
    cap_box = [cull_threshold(float(r)) for r in r32] if L else [0]
    s.append(f"    static constexpr float cap_in[{Lm}] = {_arr(cap_in)};  // certain hit: the centre within r - 1 cm of a cuboid")
    s.append(f"    static constexpr float cap_box[{Lm}] = {_arr(cap_box)};  // certain miss: the segment's bounding box beyond r + 1 cm")
    s.append(f"    static constexpr int pair_a[{Pm}] = {{" + ", ".join(str(int(v)) for v in (ch.pairs[:, 0] if P else [0])) + "};")
    s.append(f"    static constexpr int pair_b[{Pm}] = {{" + ", ".join(str(int(v)) for v in (ch.pairs[:, 1] if P else [0])) + "};")
    never = pair_never(ch) if P else [False]
    s.append(f"    static constexpr bool pair_never[{Pm}] = {{" + ", ".join("true" if v else "false" for v in never) + "};  // certified: never within 1 cm inside [lo, hi]")
    s.append("};")
    return "\n".join(s)


def generate() -> str:
    parts = [
        "// robots_gen.h -- GENERATED by cppflow_amd/gen_robots.py from cppflow_amd/robot_zoo.py; do not edit.",
        "// Canonical chains (cppflow_amd/robot_model.py) of the shipped robots as compile-time tables.",
        "#pragma once",
        "#include <stdint.h>",
        "",
        "namespace cppf {",
        "namespace gen {",
        "",
    ]
    names = []
    for name in ORDER:
        ch = canonicalize(ROBOT_SPECS[name]())
        parts.append(emit_robot(name, ch))
        parts.append("")
        names.append("".join(p.capitalize() for p in name.split("_")))
    parts.append(f"constexpr int kNumStaticRobots = {len(names)};")
    parts.append("}  // namespace gen")
    parts.append("}  // namespace cppf")
    parts.append("")
    parts.append("// X-macro over the generated robots: CPPF_FOR_EACH_STATIC_ROBOT(M) expands M(index, Type)")
    parts.append("#define CPPF_FOR_EACH_STATIC_ROBOT(M) \\")
    parts.append(" \\\n".join(f"    M({i}, ::cppf::gen::{n})" for i, n in enumerate(names)))
    parts.append("")
    return "\n".join(parts)


def write(force: bool = False) -> bool:
    text = generate()
    if not force and os.path.exists(OUT) and open(OUT).read() == text:
        return False
    with open(OUT, "w") as f:
        f.write(text)
    return True


if __name__ == "__main__":
    print(OUT, "written" if write() else "up to date")
