"""Soundness of the per-lane classification in front of the exact capsule-cuboid test of the mask-only collision stage
(env_item_undecided, csrc/kernels_collision.h), on the CPU: every item a rule decides must get the bit the exact test would have
given it.  The exact test is the fp32 oracle's segment-box function (oracle/lmik_oracle.c: seg_box_closest), which the parity tests
hold bit-equal to the device's seg_box_dist2; `distance - r < 0` there is `d2 < cap_thr` on the device (gen_robots.sqrt_threshold).

The rules, mirrored here in float32 numpy with the device's operation order (C, H: the capsule's centre and half-axis; e = C - clamp(C,
lo, hi) per axis; pd = fma(ez, ez, fma(ey, ey, ex ex))):
  rule 2   pd > cap_cull[c]                      certain miss (the bounding sphere, as before)
  rule 3   pd < cap_in[c]                        certain hit  (the centre within r - 1 cm)
  rule 4   lb > cap_box[c], lb = |g|^2 with g_i = max(|e_i| - |H_i|, 0)      certain miss (the segment's bounding box beyond r + 1 cm)
The thresholds of the shipped robots are read from the GENERATED table csrc/robots_gen.h (and must equal what gen_robots computes);
those of the extra capsules below come from the same gen_robots functions.

A FREE CAPSULE per (half length, radius), as in tests/capsule_domain.py: three prismatic and three revolute joints, the capsule along
one axis of the last link, centred on its origin.  The oracle's own fp32 centre is then the link origin and its half-axis one column
of the link's rotation times the fp32 half length -- one product per component, reproduced exactly (and checked against the oracle's
end points) -- so the mirror classifies the very numbers the exact test reads.  The half length of a shipped capsule is rounded to fp32 for this (at most 1 ulp from the value cap_cull
was computed from, against a margin of 1 cm).

Per shipped robot: every capsule x (16 384 random rows + 4 608 adversarial rows) x 8 cuboids: 1.5 to 2.2 million items, at least
1 179 648 of them random.  Adversarial
rows: H = 0 comes from the extra sphere; segments along x (H_y = H_z = 0) and in the plane z = const (H_z = 0); centres inside a
cuboid; an end point, or the centre, placed off a face, an edge or a corner at r (1 + d), d within +-1e-6, and at r +- 1 cm (1 + d) and
(half + r + 1 cm)(1 + d); cuboids 4 mm thin, of zero thickness and 8 mm small.  Extra capsules: radii 0, 5 mm, 9.9 mm and exactly 1 cm
(rule 3 must never fire), a sphere, and a 6 m capsule.

Shares (measured with this file's seed; the assertions are set below them so that a rule that stops firing fails): over the random rows
of the shipped robots rule 2 decides 87.5 - 93.6 % of the items, rule 3 3.1 - 5.9 %, and rule 4 40.7 - 44.1 % of what rules 2 and 3
leave (panda 91.4 / 4.0 / 41.8, fetch and fetch_arm 87.5 / 5.9 / 44.1, chain12 93.6 / 3.1 / 40.7)."""

import functools
import re

import numpy as np
import pytest

from cppflow_amd import gen_robots
from tests import helpers as H

f32, f64 = np.float32, np.float64
N_RANDOM, N_ADV_EACH = 16384, 512
SEED = 7411
# extra capsules (half length, radius): small radii, a sphere, a very long capsule
EXTRA = [(0.1, 0.0), (0.1, 0.005), (0.05, 0.0099), (0.1, 0.01), (0.0, 0.06), (3.0, 0.05)]
MIN_SHARE = {2: 0.80, 3: 0.025, 4: 0.35}  # of the random items; rule 4: of the items rules 2 and 3 leave undecided


def table(name, field):
    """one float array of the generated table of a shipped robot, parsed from csrc/robots_gen.h"""
    cname = "".join(p.capitalize() for p in name.split("_"))
    body = open(gen_robots.OUT).read().split(f"struct {cname} {{")[1].split("\n};")[0]
    vals = re.search(rf"static constexpr float {field}\[\d+\] = \{{([^}}]*)\}}", body).group(1)
    return np.array([float.fromhex(v.strip()[:-1]) for v in vals.split(",")], dtype=f32)


def thresholds(half, r):
    """(cap_thr, cap_cull, cap_in, cap_box) of a capsule as gen_robots computes them"""
    r = f32(r)
    return (gen_robots.sqrt_threshold(r), gen_robots.cull_threshold(float(half) + float(r)), gen_robots.inside_threshold(r),
            gen_robots.cull_threshold(float(r)))


@functools.lru_cache(maxsize=None)
def free_capsule(half, r):
    """(chain, fp32 oracle) of a free capsule of half length fp32(half) along x and radius r"""
    from cppflow_amd.robot_model import CapsuleSpec, JointSpec, RobotSpec, canonicalize
    from oracle.oracle import Oracle

    eye = ((1, 0, 0), (0, 1, 0), (0, 0, 1))
    joints = [JointSpec(f"p{n}", f"lp{n}", (0, 0, 0), (0, 0, 0), ax, "prismatic", (-8.0, 8.0)) for n, ax in zip("xyz", eye)]
    joints += [JointSpec(f"r{n}", f"lr{n}", (0, 0, 0), (0, 0, 0), ax, "revolute", (-7.0, 7.0)) for n, ax in zip("zyx", eye[::-1])]
    joints.append(JointSpec("tool", "tool", (0, 0, 0.125), (0, 0, 0), jtype="fixed"))
    h = float(f32(half))
    caps = [CapsuleSpec("base", (-0.01, 0, 0), (0.01, 0, 0), 0.0), CapsuleSpec("lrx", (-h, 0.0, 0.0), (h, 0.0, 0.0), float(r))]
    ch = canonicalize(RobotSpec(f"free_{half}_{r}", "a free capsule", "base", joints, caps, collision_pairs=[(0, 1)]))
    return ch, Oracle(ch, f32=True, threads=8)


@functools.lru_cache(maxsize=None)
def boxes():
    """(lo, hi) [8, 3], fp32-valued: four random cuboids, a 4 mm plate, one of zero thickness, a large one, an 8 mm voxel"""
    rng = np.random.RandomState(SEED)
    centre = rng.uniform(-0.4, 0.4, (8, 3))
    half = rng.uniform(0.02, 0.3, (8, 3))
    half[4, 1] = 0.002
    half[5, 2] = 0.0
    half[6] = 0.35
    half[7] = 0.004
    lo, hi = H.f32(centre - half), H.f32(centre + half)
    assert (lo[5, 2] == hi[5, 2]) and (hi[4, 1] - lo[4, 1] < 0.01)
    lo.setflags(write=False), hi.setflags(write=False)
    return lo, hi


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _box_feature(rng, n, lo, hi, kind):
    """n points on a face / an edge / a corner of the box with a unit direction in the feature's normal cone"""
    k = {"face": 1, "edge": 2, "corner": 3}[kind]
    F = rng.uniform(lo, hi, (n, 3))
    nrm = np.zeros((n, 3))
    for i in range(n):
        axes = rng.choice(3, size=k, replace=False)
        side = rng.randint(0, 2, size=k)
        F[i, axes] = np.where(side, hi[axes], lo[axes])
        nrm[i, axes] = np.where(side, 1.0, -1.0) * rng.uniform(0.2, 1.0, size=k)
    return F, _unit(nrm)


def world_half_axis(half, r, q):
    """the oracle's own fp32 world half-axis at the rows q (module docstring)"""
    ch, orc = free_capsule(float(half), float(r))
    h = gen_robots.capsule_centred(ch.cap_p0, ch.cap_p1)[1][1].astype(f64)  # the link-frame half-axis, rounded to fp32 once
    assert np.count_nonzero(h) <= 1  # R h is then ONE fp32 product per component (fused additions of an exact 0 change nothing)
    R = orc.link_frames(q)[:, int(ch.cap_link[1]), :9].reshape(-1, 3, 3)
    return (R @ h).astype(f32).astype(f64)


def rows_for(half, r):
    """q [N, 6] (fp32-valued) of a capsule: random rows first (N_RANDOM), then the adversarial ones"""
    rng = np.random.RandomState(SEED + 1)
    lo, hi = boxes()
    half, r = float(f32(half)), float(f32(r))
    q = [np.concatenate([rng.uniform(-0.7, 0.7, (N_RANDOM, 3)), rng.uniform(-np.pi, np.pi, (N_RANDOM, 3))], axis=1)]
    n = N_ADV_EACH
    # segments along x, and in a plane z = const; centres inside a cuboid
    a = np.zeros((n, 6))
    a[:, :3] = rng.uniform(-0.7, 0.7, (n, 3))
    b = a.copy()
    b[:, :3] = rng.uniform(-0.7, 0.7, (n, 3))
    b[:, 3] = rng.uniform(-np.pi, np.pi, n)
    c = np.zeros((n, 6))
    k = rng.randint(0, 8, n)
    c[:, :3] = rng.uniform(lo[k], hi[k])
    c[:, 3:] = rng.uniform(-np.pi, np.pi, (n, 3))
    q += [a, b, c]
    # grazing: the end point nearest the feature (or the centre) at a chosen distance from a face / an edge / a corner
    rel = np.array([0.0, 1e-7, -1e-7, 3e-7, -3e-7, 1e-6, -1e-6, 1e-3, -1e-3])
    for kind in ("face", "edge", "corner"):
        for centre_only in (False, True):
            ang = rng.uniform(-np.pi, np.pi, (n, 3))
            ang[rng.rand(n) < 0.3] = 0.0  # (a share of them along x: the end-point construction is then exact)
            k = rng.choice([0, 1, 4, 5, 7], size=n)
            F, nrm = np.zeros((n, 3)), np.zeros((n, 3))
            for i in range(n):
                F[i : i + 1], nrm[i : i + 1] = _box_feature(rng, 1, lo[k[i]], hi[k[i]], kind)
            hv = world_half_axis(half, r, H.f32(np.concatenate([np.zeros((n, 3)), ang], axis=1)))
            d = 1.0 + rng.choice(rel, size=n)
            if centre_only:
                dist = np.where(rng.rand(n) < 0.5, max(r - 0.01, 0.0), half + r + 0.01) * d
                C = F + dist[:, None] * nrm
            else:
                dist = rng.choice([r, r + 0.01, max(r - 0.01, 0.0)], size=n) * d
                s = -np.sign((hv * nrm).sum(axis=1))
                C = F + dist[:, None] * nrm - s[:, None] * hv
            q.append(np.concatenate([C, ang], axis=1))
    q = H.f32(np.concatenate(q))
    assert np.abs(q[:, :3]).max() < 8.0
    return q


def fma32(a, b, c):
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def classify(C, Hh, lo, hi, cull, cin, cbox):
    """the device's three comparisons on fp32 arrays C, Hh [n, 3] against one cuboid: (rule 2, rule 3, rule 4) as bool [n]"""
    e = C - np.clip(C, lo.astype(f32), hi.astype(f32))
    assert e.dtype == f32
    pd = fma32(e[:, 2], e[:, 2], fma32(e[:, 1], e[:, 1], e[:, 0] * e[:, 0]))
    g = np.maximum(np.abs(e) - np.abs(Hh), f32(0.0))
    lb = fma32(g[:, 2], g[:, 2], fma32(g[:, 1], g[:, 1], g[:, 0] * g[:, 0]))
    return pd > cull, pd < cin, lb > cbox


def sweep(half, r, thr):
    """every (row, cuboid) item of one capsule: counts per rule over the random rows, and the disagreements with the exact test"""
    ch, orc = free_capsule(float(half), float(r))
    q = rows_for(half, r)
    li = int(ch.cap_link[1])
    frames = orc.link_frames(q)[:, li]
    C = frames[:, 9:12].astype(f32)
    Hh = world_half_axis(half, r, q).astype(f32)
    ends = orc.capsule_endpoints(q)[:, 1]
    assert np.array_equal((C - Hh).astype(f64), ends[:, :3]) and np.array_equal((C + Hh).astype(f64), ends[:, 3:])  # the oracle's own capsule
    if h32_nonzero := bool(Hh.any()):  # the axis-parallel rows are what they are meant to be: two, and one, exact zeros in H
        zeros = (Hh == 0).sum(axis=1)
        assert (zeros == 2).sum() >= N_ADV_EACH // 2 and (zeros == 1).sum() >= N_ADV_EACH // 2, ((zeros == 2).sum(), (zeros == 1).sum())
    assert h32_nonzero == (float(f32(half)) > 0)
    _, cull, cin, cbox = thr
    lo, hi = boxes()
    counts = np.zeros(5)  # random items; decided by rule 2, rule 3, left to rule 4, decided by rule 4
    bad = []
    for o in range(lo.shape[0]):
        hit = orc.env_dists(q, lo[o], hi[o])[:, 1] < 0  # == d2 < cap_thr (sqrt_threshold)
        r2, r3, r4 = classify(C, Hh, lo[o], hi[o], cull, cin, cbox)
        for rule, decided, says_hit in ((2, r2, False), (3, r3, True), (4, r4, False)):
            wrong = np.flatnonzero(decided & (hit != says_hit))
            bad += [(rule, o, int(i)) for i in wrong[:4]]
        assert not (r2 & r3).any()
        if float(r) <= 0.01:
            assert not r3.any(), "rule 3 fired for a radius of at most 1 cm"
        rnd = slice(0, N_RANDOM)
        left = ~r2[rnd] & ~r3[rnd]
        counts += [N_RANDOM, r2[rnd].sum(), r3[rnd].sum(), left.sum(), (left & r4[rnd]).sum()]
    return counts, bad, q.shape[0] * lo.shape[0]


@pytest.mark.parametrize("name", gen_robots.ORDER)
def test_every_decided_item_gets_the_exact_tests_bit(name):
    ch = H.chain(name)
    half = gen_robots.capsule_centred(ch.cap_p0, ch.cap_p1)[4]
    r32 = ch.cap_r.astype(f32)
    gen = {k: table(name, k) for k in ("cap_thr", "cap_cull", "cap_in", "cap_box")}
    total, items = np.zeros(5), 0
    for c in range(ch.n_capsules):
        thr = tuple(gen[k][c] for k in ("cap_thr", "cap_cull", "cap_in", "cap_box"))
        assert thr == thresholds(half[c], r32[c]), (name, c, "the generated table is not what gen_robots computes")
        counts, bad, n = sweep(half[c], r32[c], thr)
        assert not bad, (name, c, "rule, cuboid, row:", bad[:8])
        total += counts
        items += n
    assert total[0] >= 1_000_000  # random items
    share = {2: total[1] / total[0], 3: total[2] / total[0], 4: total[4] / total[3]}
    print(name, items, "items; shares of the random items decided by rule 2 / 3 / 4 (of the rest):", {k: round(v, 4) for k, v in share.items()})
    for rule, least in MIN_SHARE.items():
        assert share[rule] >= least, (name, rule, share[rule])


@pytest.mark.parametrize("half,r", EXTRA)
def test_extra_capsules(half, r):
    """radii of at most 1 cm (rule 3 never fires: asserted in sweep), a sphere (H = 0), a 6 m capsule"""
    thr = thresholds(float(f32(half)), r)
    if r <= 0.01:
        assert thr[2] == 0.0
    counts, bad, _ = sweep(half, r, thr)
    assert not bad, (half, r, "rule, cuboid, row:", bad[:8])
    # each rule that can fire for this capsule does (the 6 m capsule's bounding sphere holds every random row: rule 4 does its work)
    assert (half > 1.0 or counts[1] > 0) and (r <= 0.01 or counts[2] > 0) and (half == 0.0 or counts[4] > 0)
