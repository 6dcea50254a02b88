#!/usr/bin/env python3
"""CPU census: what do the two prunings of the fused launch's mask-only collision stage remove on a given set of rows?

    python scripts/prune_census.py DIR/x.npy [robot]          (x.npy from `python bench.py --dump-outputs DIR`: the launch's own x_out)

Per row (a wavefront's 64 consecutive rows share every broad-phase decision, so "executed" counts a test for all 64 when any of them
is within reach):
  * self pairs certified never to touch inside the limits (Table::pair_never): their bounding-sphere tests (one each, always) and the
    exact tests the wavefront executed for them;
  * capsules that cannot reach any cuboid (a restatement of csrc/obstacle_reach.h): their point-box tests (one per cuboid, always); an
    exact test is never executed for such a capsule -- that is what the bit says.
Predicted VALU per row with the source-level costs the project uses for these functions (7 per sphere test, 55 per exact
segment-segment test, 10 per point-box test); capsule end points from the fp32 CPU oracle."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cppflow_amd import gen_robots  # noqa: E402
from cppflow_amd.problems_synthetic import PANDA_2CUBES_OBSTACLES  # noqa: E402
from oracle import oracle  # noqa: E402

oracle.build()
from tests import helpers as H  # noqa: E402

SPHERE, EXACT, POINT_BOX = 7, 55, 10
x = np.load(sys.argv[1]).astype(np.float64)
name = sys.argv[2] if len(sys.argv) > 2 else "panda"
ch = H.chain(name)
x = x.reshape(-1, ch.ndof)
x = x[: x.shape[0] // 64 * 64]
never = np.array(gen_robots.pair_never(ch))
r, half = ch.cap_r, np.linalg.norm(ch.cap_p1 - ch.cap_p0, axis=-1) / 2
ep = np.asarray(H.oracle32(name).capsule_endpoints(x))
c = 0.5 * (ep[..., :3] + ep[..., 3:])
inside = bool(((x >= ch.lo) & (x <= ch.hi)).all())

executed = np.zeros(len(ch.pairs))
for pi, (a, b) in enumerate(ch.pairs):
    near = ((c[:, a] - c[:, b]) ** 2).sum(-1) <= float(gen_robots.cull_threshold(half[a] + half[b] + r[a] + r[b]))
    executed[pi] = near.reshape(-1, 64).any(1).mean()
boxes = [(np.array(o[:3]) - np.array(o[3:]) / 2, np.array(o[:3]) + np.array(o[3:]) / 2) for o in PANDA_2CUBES_OBSTACLES]
origin = ch.F[0][9:12]
dead, env_executed = [], 0.0
for k in range(ch.n_capsules):
    l = int(ch.cap_link[k])
    on_axis0 = l == 0 and ch.jtype[0] == 0 and not ch.cap_p0[k][:2].any() and not ch.cap_p1[k][:2].any()  # on a revolute joint 0's axis
    if l < 0 or on_axis0:
        m = (ch.cap_p0[k] + ch.cap_p1[k]) / 2
        if on_axis0:
            m = ch.F[0][9:12] + ch.F[0][:9].reshape(3, 3)[:, 2] * m[2]
        live = any(((m - np.clip(m, lo, hi)) ** 2).sum() <= float(gen_robots.cull_threshold(half[k] + r[k])) for lo, hi in boxes)
    else:
        reach = sum(np.linalg.norm(ch.F[j][9:12]) for j in range(1, l + 1)) + sum(max(abs(ch.lo[j]), abs(ch.hi[j])) for j in range(l + 1) if ch.jtype[j] == 1)
        reach += max(np.linalg.norm(ch.cap_p0[k]), np.linalg.norm(ch.cap_p1[k])) + r[k] + 0.01
        live = any(np.linalg.norm(origin - np.clip(origin, lo, hi)) <= reach for lo, hi in boxes)
    for lo, hi in boxes:
        e = c[:, k] - np.clip(c[:, k], lo, hi)
        near = (e**2).sum(-1) <= float(gen_robots.cull_threshold(half[k] + r[k]))
        env_executed += near.reshape(-1, 64).any(1).mean()
        assert live or not near.any(), (k, "a dead capsule within broad-phase reach")
    if not live:
        dead.append(k)

print(f"{name}: {x.shape[0]} rows, all inside the joint limits: {inside}")
print(f"self pairs: {len(ch.pairs)}, exact tests executed per row {executed.sum():.3f}; certified {int(never.sum())} "
      f"{[tuple(int(v) for v in p) for p in ch.pairs[never]]}, exact tests executed per row on those {executed[never].sum():.3f}")
print(f"(capsule, cuboid) items: {ch.n_capsules * len(boxes)}, exact tests executed per row {env_executed:.3f}; capsules that reach no cuboid {dead}")
saved_self = never.sum() * SPHERE + executed[never].sum() * EXACT
saved_env = len(dead) * len(boxes) * POINT_BOX
print(f"predicted VALU per row removed: self {saved_self:.0f} ({int(never.sum())} x {SPHERE} + {executed[never].sum():.3f} x {EXACT}), "
      f"env {saved_env:.0f} ({len(dead)} x {len(boxes)} x {POINT_BOX}), together {saved_self + saved_env:.0f}")

# ---- per-lane classification in front of the exact capsule-cuboid test (env_item_undecided, csrc/kernels_collision.h) ------------------
# The stage as it runs: capsules outermost, the capsules that reach no cuboid skipped; per capsule first every cuboid is classified,
# then the exact test runs for the cuboids some lane of the wavefront is still undecided for, and stops once every lane that was
# undecided for this capsule is hit.  An executed test ORs its bit into all 64 lanes.  Rules: 1 a lane whose env bit is set stops
# asking; 3 the centre within r - 1 cm is a hit; 4 the segment's bounding box beyond r + 1 cm is a miss; ideal: only lanes whose exact
# clearance is within +-1 cm ask.  Rules 3 and 4 are evaluated only for the items some lane is within reach of and not yet hit
# (`surviving items`; a certain hit lies within reach, so rule 3 loses nothing by that), and cost their VALU there alone.
SEG_BOX, RULE3, RULE4 = 175, 2, 12
live_caps = [k for k in range(ch.n_capsules) if k not in dead]
hv = 0.5 * (ep[..., 3:] - ep[..., :3])
clear = np.stack([np.asarray(H.oracle32(name).env_dists(x, lo, hi)) for lo, hi in boxes], axis=-1)  # [rows, L, O]: distance - r
r32 = ch.cap_r.astype(np.float32)
cull = [float(gen_robots.cull_threshold(half[k] + float(r32[k]))) for k in range(ch.n_capsules)]
cin = [float(gen_robots.inside_threshold(r32[k])) for k in range(ch.n_capsules)]
cbox = [float(gen_robots.cull_threshold(float(r32[k]))) for k in range(ch.n_capsules)]


def wave_any(m):
    return np.repeat(m.reshape(-1, 64).any(1), 64)


def lane_census(rules):
    hit = np.zeros(x.shape[0], dtype=bool)
    tests = surviving = 0.0
    for k in live_caps:
        und = []
        for o, (lo, hi) in enumerate(boxes):
            e = c[:, k] - np.clip(c[:, k], lo, hi)
            pd = (e**2).sum(-1)
            if rules == "ideal":
                hit |= clear[:, k, o] < -0.01
                und.append((np.abs(clear[:, k, o]) <= 0.01) & ~hit)
                continue
            u = pd <= cull[k]
            if 1 in rules:
                u &= ~hit
            ask = wave_any(u)
            if 3 in rules or 4 in rules:
                surviving += ask.mean()
            if 3 in rules:
                hit |= ask & (pd < cin[k])
                u &= ~hit
            if 4 in rules:
                gap = np.maximum(np.abs(e) - np.abs(hv[:, k]), 0.0)
                u &= ~(ask & ((gap**2).sum(-1) > cbox[k]))
            und.append(u)
        open_ = np.logical_or.reduce(und)
        for o in range(len(boxes)):
            run = wave_any(und[o])
            if rules:  # (today's stage has no early stop)
                run &= wave_any(open_ & ~hit)
            tests += run.mean()
            hit |= run & (clear[:, k, o] < 0)
    assert np.array_equal(hit, (clear[:, live_caps] < 0).any((1, 2))), "the classification changed a mask bit"
    return tests, surviving


items = len(live_caps) * len(boxes)
print(f"\nexact capsule-cuboid tests per row by rule ({items} live items per row; {SEG_BOX} VALU per exact test, {RULE3} per surviving item for rule 3, "
      f"{RULE4} per surviving item for rule 4):")
base_tests = None
for label, rules in (("today", ()), ("rule 1", (1,)), ("rules 1+3", (1, 3)), ("rules 1+4", (1, 4)), ("rules 1+3+4", (1, 3, 4)), ("ideal 1 cm bound", "ideal")):
    t, s = lane_census(rules)
    base_tests = t if base_tests is None else base_tests
    added = ((RULE3 if 3 in rules else 0) + (RULE4 if 4 in rules else 0)) * s if rules != "ideal" else 0.0
    print(f"  {label:18s} tests per row {t:.3f}   surviving items per row {s:.3f}   predicted net VALU per row {(t - base_tests) * SEG_BOX + added:+.0f}")
