"""What the mask-only collision stage of the fused launch skips because it is known before a row runs (CPU side):

  * Table::pair_never (cppflow_amd/gen_robots.py: certify_pair) -- self pairs PROVED to keep 1 cm of clearance over the whole joint
    box.  Checked against the fp64 oracle on samples and corners, and on synthetic chains the certificate must refuse.
  * the capsule reach bits of cppf_set_obstacles (csrc/obstacle_reach.h), through a host-only entry compiled here with g++."""

import ctypes
import functools
import itertools
import os
import subprocess

import numpy as np
import pytest

from cppflow_amd import gen_robots
from tests import helpers as H

ROBOTS = gen_robots.ORDER
MARGIN = 0.01
N_SAMPLES = 200_000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def certified(name):
    return gen_robots.pair_never(H.chain(name))


@functools.lru_cache(maxsize=None)
def sampled_clearance(name):
    """minimum over N_SAMPLES uniform in-limit configurations of every pair's signed distance (fp64 oracle) -> [P]"""
    return H.oracle64(name).self_dists(H.random_configs(name, N_SAMPLES, seed=77)).min(axis=0)


@pytest.mark.parametrize("name", ROBOTS)
def test_certified_pairs_keep_their_margin(name):
    ch = H.chain(name)
    never = certified(name)
    smin = sampled_clearance(name)
    mid = 0.5 * (ch.lo + ch.hi)
    for pi, (a, b) in enumerate(ch.pairs):
        if not never[pi]:
            continue
        assert smin[pi] >= MARGIN, (name, int(a), int(b), smin[pi])
        joints = gen_robots.pair_joints(ch, int(a), int(b))[2]
        assert 1 <= len(joints) <= gen_robots.CERT_MAX_DIMS
        corners = np.tile(mid, (2 ** len(joints), 1))
        corners[:, joints] = np.array(list(itertools.product(*[(ch.lo[j], ch.hi[j]) for j in joints])))
        cmin = H.oracle64(name).self_dists(corners)[:, pi].min()
        assert cmin >= MARGIN, (name, int(a), int(b), cmin)


def test_panda_pairs():
    """the two pairs whose bounding spheres always overlap are certified; (2, 6) comes within half a centimetre and is not"""
    ch = H.chain("panda")
    pairs = [tuple(int(v) for v in p) for p in ch.pairs]
    never = dict(zip(pairs, certified("panda")))
    assert never[(1, 3)] and never[(3, 5)]
    assert not never[(2, 6)]
    assert sampled_clearance("panda")[pairs.index((2, 6))] < MARGIN
    assert sum(never.values()) >= 2


def _synthetic(z_gap, angle):
    """tests/helpers.two_capsule_chain: three coincident joints about z (|q_j| <= 1, so the last link turns by -3 .. 3 rad), a short
    radial capsule on the last link 0.2 above the origin and one on the base `z_gap` above where the first passes at `angle`.
    Radii are 0: the clearance is the distance of the segments, min over the box = z_gap (reached where q0 + q1 + q2 = angle)."""
    c, s = np.cos(angle), np.sin(angle)
    moving = ((0.1, 0.0, 0.2), (0.15, 0.0, 0.2))
    fixed = ((0.15 * c, 0.15 * s, 0.2 + z_gap), (0.25 * c, 0.25 * s, 0.2 + z_gap))
    return H.two_capsule_chain(fixed, moving)


def test_certificate_refuses_what_it_must():
    touching = _synthetic(0.0, 3.0)  # reached in ONE corner of the box only: q = (1, 1, 1)
    assert H.f32(touching.hi).sum() >= 3.0 - 1e-6
    assert not gen_robots.certify_pair(touching, 0, 1)
    near = _synthetic(0.005, 0.5)
    assert not gen_robots.certify_pair(near, 0, 1)
    clear = _synthetic(0.03, 0.5)
    assert gen_robots.certify_pair(clear, 0, 1)
    # the distances are what the construction says (fp64 oracle, along the line q0 = q1 = q2)
    from oracle.oracle import Oracle

    t = np.linspace(-1.0, 1.0, 6001)[:, None] * np.ones((1, 3))
    for chain, want in ((touching, 0.0), (near, 0.005), (clear, 0.03)):
        got = Oracle(chain, f32=False).self_dists(t)[:, 0].min()
        assert abs(got - want) < 2e-4, (got, want)
    # and nothing is certified over more joints than the cap
    assert not gen_robots.certify_pair(clear, 0, 1, max_dims=2)


def test_generate_is_deterministic():
    assert gen_robots.generate() == gen_robots.generate()


# ---- capsule reach bits -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reach_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("reach") / "libreach.so")
    src = os.path.join(ROOT, "tests", "native", "obstacle_reach_host.cpp")
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", out, src], check=True)
    lib = ctypes.CDLL(out)
    lib.cppf_test_capsule_reach.restype = None
    return lib


def world_fixed(ch, k):
    """a capsule of the base, or one of link 0 whose axis lies on a revolute joint 0's axis: the same place in every row"""
    on_axis = ch.cap_link[k] == 0 and ch.jtype[0] == 0 and not ch.cap_p0[k][:2].any() and not ch.cap_p1[k][:2].any()
    return ch.cap_link[k] < 0 or on_axis


def reach_bits(lib, name, lo, hi):
    from cppflow_amd import _hip

    ch = H.chain(name)
    desc = _hip.chain_to_desc(ch)
    cc, _, _, _, half = gen_robots.capsule_centred(ch.cap_p0, ch.cap_p1)
    r32 = ch.cap_r.astype(np.float32)
    cap_c = np.ascontiguousarray(cc, dtype=np.float32)
    cap_cull = np.array([gen_robots.cull_threshold(half[c] + float(r32[c])) for c in range(ch.n_capsules)], dtype=np.float32)
    lo32, hi32 = np.ascontiguousarray(lo, dtype=np.float32), np.ascontiguousarray(hi, dtype=np.float32)
    any_, lim = ctypes.c_uint32(), ctypes.c_uint32()
    fp = ctypes.POINTER(ctypes.c_float)
    lib.cppf_test_capsule_reach(ctypes.byref(desc), cap_c.ctypes.data_as(fp), cap_cull.ctypes.data_as(fp), int(lo32.shape[0]),
                                lo32.ctypes.data_as(fp), hi32.ctypes.data_as(fp), ctypes.byref(any_), ctypes.byref(lim))
    return any_.value, lim.value


@pytest.mark.parametrize("name", ROBOTS)
def test_capsules_without_a_reach_bit_stay_clear(reach_lib, name):
    """Random cubes about the boundary of each capsule's reach, on both sides of it: a capsule whose bit is clear keeps more than
    1 cm from every cuboid of the set on 100 000 random in-limit configurations (fp64 oracle); the any-row bit is only ever clear for
    a capsule that does not move (`world_fixed`)."""
    ch = H.chain(name)
    L = ch.n_capsules
    x = H.random_configs(name, 100_000, seed=5)
    rng = np.random.RandomState(11)
    o = ch.F[0][9:12]
    dead_seen, live_seen = 0, 0
    for trial in range(8):
        c = rng.randint(L)
        # roughly the capsule's reach from the origin of joint 0's frame, then a cube whose near face sits within +-6 cm of it
        l = int(ch.cap_link[c])
        far = sum(np.linalg.norm(ch.F[j][9:12]) for j in range(1, l + 1)) + sum(max(abs(ch.lo[j]), abs(ch.hi[j])) for j in range(l + 1) if ch.jtype[j] == 1)
        far += max(np.linalg.norm(ch.cap_p0[c]), np.linalg.norm(ch.cap_p1[c])) + ch.cap_r[c]
        axis, sign, h = rng.randint(3), rng.choice([-1.0, 1.0]), rng.uniform(0.05, 0.2)
        centre = o + rng.uniform(-0.05, 0.05, 3)
        centre[axis] = o[axis] + sign * (far + h + rng.uniform(-0.06, 0.06))
        boxes_lo, boxes_hi = [centre - h], [centre + h]
        if trial % 2:  # a second cube far away from everything
            boxes_lo.append(o + 10.0), boxes_hi.append(o + 10.5)
        lo, hi = H.f32(np.array(boxes_lo)), H.f32(np.array(boxes_hi))
        any_, lim = reach_bits(reach_lib, name, lo, hi)
        assert lim & ~any_ == 0 and any_ < (1 << L)
        clear = np.min([H.oracle64(name).env_dists(x, lo[k], hi[k]) for k in range(lo.shape[0])], axis=0).min(axis=0)  # [L]
        for k in range(L):
            if not world_fixed(ch, k):
                assert (any_ >> k) & 1
            if not (lim >> k) & 1:
                assert clear[k] - MARGIN > 0, (name, trial, k, clear[k])
                dead_seen += 1
            else:
                live_seen += 1
    assert dead_seen > 0 and live_seen > 0
    # no cuboids: nothing is live inside the limits (any row: the moving capsules are never decided); a cuboid around everything: all are
    moving = sum(1 << k for k in range(L) if not world_fixed(ch, k))
    assert reach_bits(reach_lib, name, np.zeros((0, 3)), np.zeros((0, 3))) == (moving, 0)
    assert reach_bits(reach_lib, name, np.full((1, 3), -5.0), np.full((1, 3), 5.0)) == ((1 << L) - 1, (1 << L) - 1)
