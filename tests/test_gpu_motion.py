"""The motion between waypoints on the MI355X: cppf_motion_clearance (csrc/kernels_motion.h) against its definition
(include/cppflow_hip.h), restated here on the fp32 oracle's per-pair and per-(capsule, cuboid) clearances.

Paths (make_paths): a start drawn inside the joint limits, then steps uniform in +-amp per joint with amp cycling through 0.03 rad
(the planner's spacing), 0.15 and 0.45 rad (a sparse path), a fifth of that on prismatic joints, clipped 0.05 inside the limits.
Scenes: the polar recipe of tests/test_gpu_scene.py, 70 cuboids per robot, a scene of O cuboids is the first O of them.  The seeds
(SEEDS) were picked with the oracle so that every robot's cases hold certified, hit and undecided transitions
(test_the_cases_hold_every_verdict asserts it on the device's answer).

Guard band.  The kernel decides  (c_i + c_{i+1}) - lambda / M > 1e-6  in fp32; the restatement evaluates the same expression in fp64 on
the same fp32 clearances, table and |b - a|.  The two differ by the rounding of at most d fmaf's in lambda (<= d 2^-24 lambda, lambda
< 8 m: 6e-6 at d = 12) and of the sum and difference (2^-23 of < 1 m): decisions whose fp64 margin is more than 1e-5 m off the
threshold must agree, and at most 1 % of all decisions may lie inside that band."""

import ctypes
import dataclasses
import functools
import gc
import os

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_gpu_scene import polar_cuboids

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_files")
ROBOTS = ("panda", "fetch", "generic7", "chain12")
RADII = {"panda": (0.30, 0.95), "chain12": (0.30, 0.95), "fetch": (0.50, 1.15), "generic7": (0.30, 0.95)}
SEEDS = {"panda": 11, "fetch": 12, "generic7": 13, "chain12": 14}
# (S, W, level, n_obs): every S in {1, 3}, W in {2, 5, 12}, level in {0, 3, 6} (65, 9 and 2 nodes per transition: no multiple of 64),
# n_obs in {0, 2, 70} (no scene, one part-filled tile, a second tile)
CASES = ((1, 2, 0, 0), (1, 2, 6, 2), (3, 5, 3, 70), (3, 12, 6, 70), (1, 12, 3, 2), (3, 2, 0, 70), (1, 5, 6, 0), (3, 12, 0, 2))
REACH = 0.05
BAND, SLACK = 1e-5, 1e-6
INF = np.float32(np.inf)
CERT, HIT = 1, 2


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.int32)


@functools.lru_cache(maxsize=None)
def chain(name):
    if name == "generic7":  # a description that matches no generated table: the generic kernel, general joint axes, a prismatic joint
        from cppflow_amd.robot_model import canonicalize

        return canonicalize(H.random_chain_spec(7, seed=21))
    return H.chain(name)


@functools.lru_cache(maxsize=None)
def oracle(name):
    from oracle.oracle import Oracle

    return Oracle(chain(name), f32=True, threads=8)


@functools.lru_cache(maxsize=None)
def robot(name):
    from cppflow_amd.robot_zoo import ROBOT_SPECS
    from cppflow_amd.robots import Robot

    if name == "generic7":
        return Robot(H.random_chain_spec(7, seed=21), specialize=False)
    return Robot(ROBOT_SPECS[name]())


@functools.lru_cache(maxsize=None)
def rho(name):
    return robot(name).motion_travel_table().astype(np.float64)


@functools.lru_cache(maxsize=None)
def boxes(name):
    lo, hi, _ = polar_cuboids(RADII[name], 70, np.random.default_rng(SEEDS[name]))
    return lo, hi


def make_paths(name, S, W, seed):
    ch = chain(name)
    rng = np.random.RandomState(seed)
    lo, hi = ch.lo + 0.05, ch.hi - 0.05
    scale = np.where(np.asarray(ch.jtype) == 1, 0.2, 1.0)
    q = np.zeros((S, W, ch.ndof))
    q[:, 0] = rng.uniform(lo, hi, size=(S, ch.ndof))
    for t in range(1, W):
        amp = np.array([(0.03, 0.15, 0.45)[(t + s) % 3] for s in range(S)])[:, None]
        q[:, t] = np.clip(q[:, t - 1] + rng.uniform(-1, 1, size=(S, ch.ndof)) * amp * scale, lo, hi)
    return q.astype(np.float32)


def lerp_nodes(q, level):
    """the definition's nodes in fp64 (exact but for the final rounding): [S, W-1, M+1, d]"""
    M = 1 << level
    a, b = q[:, :-1, None, :].astype(np.float64), q[:, 1:, None, :].astype(np.float64)
    d32 = (q[:, 1:] - q[:, :-1]).astype(np.float64)[:, :, None, :]  # (the subtraction in fp32)
    f = (np.arange(M + 1) / M)[None, None, :, None]
    x = a + f * d32
    x[:, :, 0], x[:, :, M] = a[:, :, 0], b[:, :, 0]
    return x


@dataclasses.dataclass
class Restated:
    min_clear: np.ndarray  # [S, W-1] f32, exact
    hit_node: np.ndarray  # [S, W-1] i32, exact
    must_certify: np.ndarray  # bool [S, W-1]: every decision clearly passes, inside the limits, not hit
    must_not_certify: np.ndarray  # bool [S, W-1]: some decision clearly fails, or outside the limits, or hit
    n_decisions: int
    n_in_band: int
    node_clear: np.ndarray  # [S, W-1, M+1] f32: min(min_self, min_env untruncated) per node


def restate(name, q, nodes, lo, hi, level, reach):
    """the definition in fp64 on the fp32 oracle's clearances at the DEVICE's nodes"""
    ch, orc, M = chain(name), oracle(name), 1 << level
    S, W, d = q.shape
    x = nodes.reshape(-1, d).astype(np.float64)
    n, shape = x.shape[0], (S, W - 1, M + 1)
    cs = orc.self_dists(x).reshape(shape + (-1,))  # [S, W-1, M+1, P]
    O = lo.shape[0]
    ce = np.stack([orc.env_dists(x, lo[o].astype(np.float64), hi[o].astype(np.float64)) for o in range(O)], axis=1) if O else np.zeros((n, 0, orc.n_caps))
    ce = ce.reshape(shape + (O, orc.n_caps))
    assert np.array_equal(cs.astype(np.float32).astype(np.float64), cs) and np.array_equal(ce.astype(np.float32).astype(np.float64), ce)
    min_self = cs.min(axis=-1) if cs.shape[-1] else np.full(shape, np.inf)
    min_env_all = ce.reshape(shape + (-1,)).min(axis=-1) if ce.size else np.full(shape, np.inf)
    min_env = np.where(min_env_all < np.float32(reach), min_env_all, np.inf)
    node_clear = np.minimum(min_self, min_env_all)
    neg = node_clear < 0
    hit_node = np.where(neg.any(axis=-1), neg.argmax(axis=-1), -1).astype(np.int32)
    # travel bounds: |b - a| in fp32, the handle's table
    r = rho(name)
    dq = np.abs(q[:, 1:] - q[:, :-1]).astype(np.float64)  # [S, W-1, d]
    link = np.asarray(ch.cap_link)
    lam_c = dq @ r  # [S, W-1, L]
    lam_p = np.zeros((S, W - 1, len(ch.pairs)))
    for p, (c1, c2) in enumerate(np.asarray(ch.pairs)):
        if link[c1] > link[c2]:
            c1, c2 = c2, c1
        js = np.arange(d)
        sel = (js > link[c1]) & (js <= link[c2])
        lam_p[:, :, p] = dq[:, :, sel] @ r[sel, c2]
    reach64 = float(np.float32(reach))
    cet = np.minimum(ce, reach64)
    dec_self = cs[:, :, :-1] + cs[:, :, 1:] - lam_p[:, :, None, :] / M - SLACK  # [S, W-1, M, P]
    dec_env = cet[:, :, :-1] + cet[:, :, 1:] - lam_c[:, :, None, None, :] / M - SLACK  # [S, W-1, M, O, L]
    dec = np.concatenate([dec_self.reshape(S, W - 1, -1), dec_env.reshape(S, W - 1, -1)], axis=-1)
    inside = ((q >= ch.lo.astype(np.float32)) & (q <= ch.hi.astype(np.float32))).all(axis=-1)
    inside = inside[:, :-1] & inside[:, 1:]
    hit = hit_node >= 0
    clearly_pass = (dec > BAND).all(axis=-1)
    clearly_fail = (dec < -BAND).any(axis=-1)
    return Restated(
        min_clear=np.minimum(min_self, min_env).min(axis=-1).astype(np.float32), hit_node=hit_node,
        must_certify=clearly_pass & inside & ~hit, must_not_certify=clearly_fail | ~inside | hit,
        n_decisions=int(dec.size), n_in_band=int((np.abs(dec) <= BAND).sum()), node_clear=node_clear.astype(np.float32),
    )  # fmt: skip


def run(name, q, lo, hi, level, reach=REACH, want=("status", "min_clear", "hit_node", "nodes")):
    got = robot(name).motion_clearance(dev(q), dev(lo).reshape(-1, 3), dev(hi).reshape(-1, 3), level=level, reach=reach, want=want)
    torch.cuda.synchronize()
    return {k: host(v) for k, v in got.items()}


@functools.lru_cache(maxsize=None)
def case(name, S, W, level, n_obs):
    """one launch and its restatement, shared by the tests below: (q, lo, hi, device outputs, Restated)"""
    q = make_paths(name, S, W, SEEDS[name] + 100 * S + W)
    lo, hi = (a[:n_obs] for a in boxes(name))
    got = run(name, q, lo, hi, level)
    return q, lo, hi, got, restate(name, q, got["nodes"], lo, hi, level, REACH)


def check_against_restatement(got, want, ctx):
    status = got["status"]
    assert not ((status & CERT != 0) & (status & HIT != 0)).any() and (status <= 3).all(), ctx
    assert np.array_equal(bits(got["min_clear"]), bits(want.min_clear)), ctx
    assert np.array_equal(got["hit_node"], want.hit_node), ctx
    assert np.array_equal(status & HIT != 0, want.hit_node >= 0), ctx
    cert = status & CERT != 0
    assert not (want.must_certify & ~cert).any(), (ctx, "a transition every decision of which clearly passes was not certified")
    assert not (want.must_not_certify & cert).any(), (ctx, "a transition with a clearly failing decision was certified")
    assert want.n_in_band <= 0.01 * max(want.n_decisions, 1), (ctx, want.n_in_band, want.n_decisions)


# ---- 1. nodes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,W,level,n_obs", CASES)
@pytest.mark.parametrize("name", ROBOTS)
def test_nodes(name, S, W, level, n_obs):
    q, _, _, got, _ = case(name, S, W, level, n_obs)
    M = 1 << level
    nodes = got["nodes"]
    assert nodes.shape == (S, W - 1, M + 1, q.shape[2]) and nodes.dtype == np.float32
    assert np.array_equal(bits(nodes[:, :, 0]), bits(q[:, :-1])) and np.array_equal(bits(nodes[:, :, M]), bits(q[:, 1:]))
    want = lerp_nodes(q, level)
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert (np.abs(nodes.astype(np.float64) - want) <= ulp).all()
    if level >= 1:  # i / M = 1 / 2 and an fp32 step: the midpoint is the correctly rounded one
        mid = (q[:, :-1].astype(np.float64) + 0.5 * (q[:, 1:] - q[:, :-1]).astype(np.float64)).astype(np.float32)
        assert np.array_equal(bits(nodes[:, :, M // 2]), bits(mid))


# ---- 2. / 3. clearances bit for bit, the verdict against the fp64 restatement -------------------------------------------------------------
@pytest.mark.parametrize("S,W,level,n_obs", CASES)
@pytest.mark.parametrize("name", ROBOTS)
def test_clearances_bit_for_bit_and_verdict_against_the_restatement(name, S, W, level, n_obs):
    q, lo, hi, got, want = case(name, S, W, level, n_obs)
    check_against_restatement(got, want, (name, S, W, level, n_obs))
    # the existing launches on the returned nodes: min_self of cppf_collision_masks, min_env of cppf_scene_env_collisions at the same reach
    rb = robot(name)
    nd = dev(got["nodes"]).reshape(1, -1, q.shape[2]).contiguous()
    rb.set_obstacles([], [])
    m_self = host(rb.collision_masks(nd, want_min_dists=True, only=("self",))["min_self"]).reshape(got["nodes"].shape[:3])
    m_env = host(rb.scene_env_collisions(nd, dev(lo).reshape(-1, 3), dev(hi).reshape(-1, 3), reach=REACH, want=("env_mask", "min_env"))["min_env"])
    node_min = np.minimum(m_self, m_env.reshape(m_self.shape))
    assert np.array_equal(bits(got["min_clear"]), bits(node_min.min(axis=-1)))
    neg = node_min < 0
    assert np.array_equal(got["hit_node"], np.where(neg.any(axis=-1), neg.argmax(axis=-1), -1))


def test_the_cases_hold_every_verdict():
    """what the seeds were picked for, on the device's answer: per robot certified, hit and undecided transitions all occur, and
    certificates are issued against cuboids within reach (min_clear below the reach) as well as far from everything"""
    for name in ROBOTS:
        st = np.concatenate([case(name, *c)[3]["status"].reshape(-1) for c in CASES])
        mc = np.concatenate([case(name, *c)[3]["min_clear"].reshape(-1) for c in CASES])
        n_cert, n_hit, n_und = int((st == CERT).sum()), int((st == HIT).sum()), int((st == 0).sum())
        band = sum(case(name, *c)[4].n_in_band for c in CASES), sum(case(name, *c)[4].n_decisions for c in CASES)
        print(f"{name}: {st.size} transitions: certified {n_cert}, hit {n_hit}, undecided {n_und}; certified with min_clear < reach "
              f"{int(((st == CERT) & (mc < REACH)).sum())}; decisions inside the guard band {band[0]} of {band[1]}")  # fmt: skip
        assert n_cert > 0 and n_hit > 0 and n_und > 0, name
        assert ((st == CERT) & (mc < REACH)).any(), name


# ---- 4. soundness ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROBOTS)
def test_no_certified_transition_touches_anything_in_a_1025_sample_sweep(name):
    orc = oracle(name)
    n_checked = 0
    for c in CASES:
        q, lo, hi, got, _ = case(name, *c)
        cert = np.argwhere(got["status"] & CERT != 0)
        if not len(cert):
            continue
        f = (np.arange(1025) / 1024)[None, :, None]
        a = np.stack([q[s, t] for s, t in cert]).astype(np.float64)[:, None, :]
        b = np.stack([q[s, t + 1] for s, t in cert]).astype(np.float64)[:, None, :]
        x = H.f32((a + f * (b - a)).reshape(-1, q.shape[2]))
        worst = orc.self_dists(x).min(axis=1) if orc.n_pairs else np.full(x.shape[0], np.inf)
        for o in range(lo.shape[0]):
            worst = np.minimum(worst, orc.env_dists(x, lo[o].astype(np.float64), hi[o].astype(np.float64)).min(axis=1))
        assert (worst > 0).all(), (name, c, float(worst.min()))
        n_checked += len(cert)
    assert n_checked > 0


# ---- 5. the case this exists for ----------------------------------------------------------------------------------------------------------
VOXEL_SEED, VOXEL_T = 6, 2


def voxel_case():
    """(q [1, 5, 7], lo, hi [3, 3] = PANDA_2CUBES + the voxel, the midpoint configuration, the hand capsule's index)"""
    ch, orc = chain("panda"), oracle("panda")
    rng = np.random.RandomState(VOXEL_SEED)
    q = np.zeros((1, 5, 7), dtype=np.float32)
    q[0, 0] = [0.0, -0.4, 0.0, -2.0, 0.0, 1.6, 0.8]
    for t in range(1, 5):
        q[0, t] = q[0, t - 1] + np.float32(0.3) * rng.choice([-1.0, 1.0], 7).astype(np.float32)
    q = np.clip(q, ch.lo.astype(np.float32) + np.float32(0.05), ch.hi.astype(np.float32) - np.float32(0.05))
    mid = (q[0, VOXEL_T].astype(np.float64) + 0.5 * (q[0, VOXEL_T + 1] - q[0, VOXEL_T]).astype(np.float64)).astype(np.float32)
    hand = ch.n_capsules - 1
    assert "hand" in ch.cap_names[hand]
    ends = orc.capsule_endpoints(mid[None].astype(np.float64))[0, hand]
    centre = 0.5 * (ends[:3] + ends[3:])
    lo0, hi0 = H.box_corners([c for c, _ in H.PANDA_2CUBES], [T for _, T in H.PANDA_2CUBES])
    vlo, vhi = H.box_corners(*zip(H.cuboid_obstacle(*centre, 0.02, 0.02, 0.02)))
    return q, np.concatenate([lo0, vlo]).astype(np.float32), np.concatenate([hi0, vhi]).astype(np.float32), mid, hand


def test_a_voxel_between_two_clear_waypoints():
    """a 2 cm cube on the hand capsule's centre at the midpoint of one transition of a sparse Panda path (steps of 0.3 rad per
    joint): both neighbouring waypoints are clear of it, the waypoint masks call the path collision-free, the motion check finds it"""
    name, t_hit = "panda", VOXEL_T
    ch, orc, rb = chain(name), oracle(name), robot(name)
    q, lo, hi, mid, hand = voxel_case()
    # the oracle: every waypoint is clear of everything (of the voxel in particular), the midpoint is inside it
    way = orc.masks(q[0].astype(np.float64), lo.astype(np.float64), hi.astype(np.float64), ch.lo, ch.hi)
    assert not way["self_mask"].any() and not way["env_mask"].any()
    d_voxel = orc.env_dists(q[0].astype(np.float64), lo[2].astype(np.float64), hi[2].astype(np.float64)).min(axis=1)
    assert (d_voxel[[t_hit, t_hit + 1]] > 0.02).all(), d_voxel
    assert orc.env_dists(mid[None].astype(np.float64), lo[2].astype(np.float64), hi[2].astype(np.float64))[0, hand] < 0
    # the existing masks: collision-free
    qd = dev(q)
    rb.set_obstacles([], [])
    assert not bool(rb.scene_env_collisions(qd, dev(lo), dev(hi), want=("env_mask",))["env_mask"].any())
    assert not bool(rb.collision_masks(qd, only=("self",))["self_mask"].any())
    for level in (1, 3, 6):
        M = 1 << level
        got = run(name, q, lo, hi, level)
        want = restate(name, q, got["nodes"], lo, hi, level, REACH)
        assert got["status"][0, t_hit] == HIT and got["hit_node"][0, t_hit] == want.hit_node[0, t_hit] >= 0, (level, got)
        assert want.node_clear[0, t_hit, M // 2] < 0 and got["hit_node"][0, t_hit] <= M // 2
        if level == 1:
            assert got["hit_node"][0, t_hit] == 1
        assert got["min_clear"][0, t_hit] < 0
        check_against_restatement(got, want, ("voxel", level))
    got0 = run(name, q, lo, hi, 0)
    assert got0["status"][0, t_hit] == 0 and got0["hit_node"][0, t_hit] == -1  # level 0: neither hit nor certified
    without = run(name, q, lo[:2], hi[:2], 6)
    assert without["status"][0, t_hit] == CERT, without
    print("voxel case: status with the voxel", run(name, q, lo, hi, 6)["status"], "without", without["status"])


# ---- 6. culling cannot change a verdict ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROBOTS)
def test_culling_cannot_change_a_verdict(name):
    S, W, level, n_obs = 3, 12, 6, 70
    q, lo, hi, got, _ = case(name, S, W, level, n_obs)
    _, _, far = polar_cuboids((2.5, 3.5), 60, np.random.default_rng(1))
    flo, fhi = H.box_corners([c for c, _ in far], [T for _, T in far])
    for lo2, hi2 in ((lo, hi), (np.concatenate([lo, flo.astype(np.float32)]), np.concatenate([hi, fhi.astype(np.float32)]))):
        fin = run(name, q, lo2, hi2, level, reach=REACH, want=("status", "min_clear", "hit_node"))
        unc = run(name, q, lo2, hi2, level, reach=float("inf"), want=("status", "min_clear", "hit_node"))
        cert = fin["status"] & CERT != 0
        assert np.array_equal(unc["status"][cert], fin["status"][cert])
        assert np.array_equal(unc["status"] & HIT, fin["status"] & HIT) and np.array_equal(unc["hit_node"], fin["hit_node"])
        # far clutter changes nothing at all at the finite reach
        assert np.array_equal(fin["status"], got["status"]) and np.array_equal(fin["hit_node"], got["hit_node"])
        assert np.array_equal(bits(fin["min_clear"]), bits(got["min_clear"]))
    assert (got["status"] & CERT != 0).any()


# ---- 7. / 8. a stationary transition, a waypoint outside the limits ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROBOTS)
def test_stationary_transitions_and_waypoints_outside_the_limits(name):
    ch, orc = chain(name), oracle(name)
    lo, hi = (a[:70] for a in boxes(name))
    x = H.random_configs(name, 24, seed=9, margin=0.05) if name != "generic7" else H.f32(
        np.random.RandomState(9).uniform(ch.lo + 0.05, ch.hi - 0.05, size=(24, ch.ndof)))  # fmt: skip
    q = np.repeat(x.astype(np.float32)[:, None, :], 2, axis=1)  # [24, 2, d], a == b
    clear = orc.self_dists(x).min(axis=1) if orc.n_pairs else np.full(24, np.inf)
    for o in range(70):
        clear = np.minimum(clear, orc.env_dists(x, lo[o].astype(np.float64), hi[o].astype(np.float64)).min(axis=1))
    assert (clear > 1e-6).any() and (clear < 0).any() and not ((clear >= 0) & (clear <= 1e-6)).any()  # (nothing within the slack of 0)
    for level in (0, 6):
        got = run(name, q, lo, hi, level, want=("status", "hit_node"))
        assert np.array_equal(got["status"][:, 0] == CERT, clear > 0), (name, level)
        assert np.array_equal(got["status"][:, 0] == HIT, clear < 0) and np.array_equal(got["hit_node"][:, 0] == 0, clear < 0)
    # 8. the same stationary transitions with one joint of one waypoint 0.01 beyond a limit: never certified, whichever end
    free = np.flatnonzero(clear > 0.02)
    assert len(free) >= 2
    for end in (0, 1):
        for side in (0, 1):
            qo = q[free].copy()
            j = (end + 2 * side) % ch.ndof
            qo[:, end, j] = np.float32(ch.hi[j]) + np.float32(0.01) if side else np.float32(ch.lo[j]) - np.float32(0.01)
            got = run(name, qo, lo[:0], hi[:0], 6, want=("status",))
            assert not (got["status"] & CERT).any(), (name, end, side)
    # ON a limit is inside: stationary at the limit, certified exactly when the (self) clearance there is positive
    qi = q[free].copy()
    qi[:, :, 0], qi[:, :, ch.ndof - 1] = np.float32(ch.hi[0]), np.float32(ch.lo[ch.ndof - 1])
    on = orc.self_dists(qi[:, 0].astype(np.float64)).min(axis=1) if orc.n_pairs else np.full(len(free), np.inf)
    assert not ((on >= 0) & (on <= 1e-6)).any()
    ok = run(name, qi, lo[:0], hi[:0], 0, want=("status",))
    assert np.array_equal(ok["status"][:, 0] == CERT, on > 0), name


# ---- 9. hygiene ------------------------------------------------------------------------------------------------------------------------------
def run_in_arena(rb, q, lo, hi, level, reach, poison, stream=None):
    """the entry point with outputs and workspace carved out of one poisoned arena with guard gaps -> dict of host arrays"""
    from cppflow_amd import _hip

    lib = _hip.lib()
    S, W, d = q.shape
    M, O, n_tr = 1 << level, lo.shape[0], S * (W - 1)
    nbytes = ctypes.c_size_t(0)
    _hip.check(lib.cppf_motion_workspace_bytes(S, W, ctypes.byref(nbytes)))
    arena = torch.full((1 << 21,), poison, dtype=torch.uint8, device=DEV)
    cursor, spans, bufs = 4096, [], {}
    sizes = (("workspace", nbytes.value), ("status", n_tr), ("min_clear", 4 * n_tr), ("hit_node", 4 * n_tr), ("nodes", 4 * n_tr * (M + 1) * d))
    for nm, nb in sizes:
        start = (cursor + 255) // 256 * 256
        bufs[nm] = arena[start : start + nb]
        spans.append((start, start + nb))
        cursor = start + nb + 1024
    assert cursor + 4096 < arena.numel()
    torch.cuda.synchronize()
    st = (stream if stream is not None else torch.cuda.current_stream(DEV)).cuda_stream
    _hip.check(lib.cppf_motion_clearance(rb._handle(torch.device(DEV)), q.data_ptr(), S, W, level, lo.data_ptr(), hi.data_ptr(), O, reach,
                                         bufs["status"].data_ptr(), bufs["min_clear"].data_ptr(), bufs["hit_node"].data_ptr(),
                                         bufs["nodes"].data_ptr(), bufs["workspace"].data_ptr(), nbytes.value, st))  # fmt: skip
    torch.cuda.synchronize()
    keep = torch.ones(cursor + 4096, dtype=torch.bool, device=DEV)
    for a, b in spans:
        keep[a:b] = False
    assert bool((arena[: cursor + 4096][keep] == poison).all()), "a guard gap was written"
    return {nm: host(bufs[nm]).copy() for nm, _ in sizes[1:]}


@pytest.mark.parametrize("name,S,W,level,n_obs", [("panda", 3, 12, 6, 70), ("fetch", 3, 5, 3, 70), ("generic7", 1, 2, 6, 2), ("chain12", 3, 2, 0, 70)])
def test_memory_discipline_and_determinism(name, S, W, level, n_obs):
    rb = robot(name)
    q, lo, hi, got, _ = case(name, S, W, level, n_obs)
    qd, lod, hid = dev(q), dev(lo).reshape(-1, 3), dev(hi).reshape(-1, 3)
    before = [t.clone() for t in (qd, lod, hid)]
    runs = [run_in_arena(rb, qd, lod, hid, level, REACH, 0xA5), run_in_arena(rb, qd, lod, hid, level, REACH, 0x5A),
            run_in_arena(rb, qd, lod, hid, level, REACH, 0xA5, torch.cuda.Stream(device=DEV))]  # fmt: skip
    for r in runs[1:]:
        for nm, v in r.items():
            assert np.array_equal(v, runs[0][nm]), nm
    for t, b in zip((qd, lod, hid), before):
        assert torch.equal(t.view(torch.int32), b.view(torch.int32))
    r = runs[0]
    assert np.array_equal(r["status"], got["status"].reshape(-1)) and np.array_equal(r["min_clear"].view(np.int32), bits(got["min_clear"]).reshape(-1))
    assert np.array_equal(r["hit_node"].view(np.int32), got["hit_node"].reshape(-1)) and np.array_equal(r["nodes"].view(np.int32), bits(got["nodes"]).reshape(-1))


@pytest.mark.parametrize("name", ROBOTS)
def test_permuted_paths_give_permuted_outputs_and_the_generic_form_agrees(name):
    rb = robot(name)
    S, W, level, n_obs = 3, 12, 6, 70
    q, lo, hi, got, _ = case(name, S, W, level, n_obs)
    perm = [2, 0, 1]
    shuf = run(name, q[perm], lo, hi, level)
    for nm in got:
        assert np.array_equal(shuf[nm].view(np.uint8), np.ascontiguousarray(got[nm][perm]).view(np.uint8)), nm
    if name == "generic7":
        assert rb.specialization() == -1
        return
    assert rb.specialization() >= 0  # a generated table
    rb.debug_set("force_generic", 1)
    try:
        gen = [run(name, q, lo, hi, level), run(name, *case(name, 3, 5, 3, 70)[:3], 3)]
    finally:
        rb.debug_set("force_generic", None)
    for g, base in zip(gen, (got, case(name, 3, 5, 3, 70)[3])):
        for nm in base:
            assert np.array_equal(g[nm].view(np.uint8), base[nm].view(np.uint8)), nm


def test_a_handle_specialised_at_run_time_is_served_by_the_generic_form():
    from cppflow_amd.robots import Robot

    rtc = Robot(H.random_chain_spec(7, seed=21), specialize=True)
    assert rtc.specialization() == 1000
    q, lo, hi, got, _ = case("generic7", 3, 5, 3, 70)
    a = rtc.motion_clearance(dev(q), dev(lo), dev(hi), level=3, reach=REACH, want=("status", "min_clear", "hit_node", "nodes"))
    for nm in got:
        assert np.array_equal(host(a[nm]).view(np.uint8), got[nm].view(np.uint8)), nm


def test_graph_capture_replays_the_call():
    rb = robot("panda")
    q, lo, hi, want, _ = case("panda", 3, 12, 6, 70)
    qd, lod, hid = dev(q), dev(lo), dev(hi)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    g = torch.cuda.CUDAGraph()
    keys = ("status", "min_clear", "hit_node", "nodes")
    with torch.cuda.stream(side):
        rb.motion_clearance(qd, lod, hid, level=6, reach=REACH, want=keys)  # (warm: the allocator's pool, the handle)
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            got = rb.motion_clearance(qd, lod, hid, level=6, reach=REACH, want=keys)
    for _ in range(2):
        for v in got.values():
            v.view(torch.uint8).fill_(0x77)
        g.replay()
        torch.cuda.synchronize()
        for nm in keys:
            assert np.array_equal(host(got[nm]).view(np.uint8), want[nm].view(np.uint8)), nm


def test_a_destroyed_handle_is_refused():
    """on a handle that cppf_robot_destroy has marked dead (kept allocated by a live batch): CPPF_ERR_INVALID, nothing launched"""
    from cppflow_amd import _hip
    from cppflow_amd.robot_zoo import ROBOT_SPECS
    from cppflow_amd.robots import Robot

    rb = Robot(ROBOT_SPECS["panda"]())
    x0, target = H.lm_problem("panda", 4, 64, seed=1)
    x0, target = dev(x0), dev(target)
    plan = rb.lm_batch_plan([dict(x=x0, target=target, x_out=torch.empty_like(x0))], 1e-6, 3.5, 0.35, n_steps=3)
    handle = rb._handle(torch.device(DEV))
    plan._keep[0] = None
    _hip.lib().cppf_robot_destroy(handle)
    rb._handles = {}
    del rb
    gc.collect()
    q = dev(make_paths("panda", 3, 5, 1))
    status = torch.full((12,), 7, dtype=torch.uint8, device=DEV)
    ws = torch.full((1 << 12,), 7, dtype=torch.uint8, device=DEV)
    rc = _hip.lib().cppf_motion_clearance(handle, q.data_ptr(), 3, 5, 6, None, None, 0, 0.05, status.data_ptr(), None, None, None,
                                          ws.data_ptr(), ws.numel(), None)  # fmt: skip
    assert rc == _hip.CPPF_ERR_INVALID and "destroyed" in _hip.lib().cppf_last_error().decode()
    torch.cuda.synchronize()
    assert bool((status == 7).all()) and bool((ws == 7).all())  # nothing was launched
    del plan
    gc.collect()


# ---- 10. the planner ---------------------------------------------------------------------------------------------------------------------------
def test_the_planner_reports_the_certificate_and_returns_the_same_plan():
    from cppflow_amd.data_type_utils import problem_from_filename
    from cppflow_amd.data_types import PlannerSettings
    from cppflow_amd.planners import CppFlowPlanner, TrackingSeedProvider

    problem = problem_from_filename(None, "panda__1cube_mini", problems_dir=os.path.join(REF, "problems"), paths_dir=os.path.join(REF, "paths"),
                                    device=DEV)  # fmt: skip
    settings = PlannerSettings(k=175, tmax_sec=60.0, anytime_mode_enabled=False, do_rerun_if_large_dp_search_mjac=False,
                               do_rerun_if_optimization_fails=False, verbosity=0)  # fmt: skip
    plain = CppFlowPlanner(settings, problem.robot, seed_provider=TrackingSeedProvider(seed=0)).generate_plan(problem)
    res = CppFlowPlanner(settings, problem.robot, seed_provider=TrackingSeedProvider(seed=0), certify_motion_level=6).generate_plan(problem)
    keys = ("motion_certified", "motion_hit_transitions", "motion_undecided_transitions")
    assert all(k in res.debug_info for k in keys) and not any(k in plain.debug_info for k in keys)
    assert torch.equal(res.plan.q_path, plain.plan.q_path) and res.plan.is_valid == plain.plan.is_valid
    assert {k: v for k, v in res.debug_info.items() if k not in keys} == plain.debug_info
    mc = problem.motion_clearance(res.plan.q_path, level=6)
    T = problem.n_timesteps
    assert mc.certified.shape == (1, T - 1) and mc.min_clear.dtype == torch.float32 and mc.hit_node.dtype == torch.int32
    assert res.debug_info["motion_certified"] == bool(mc.all_certified[0]) == (not res.debug_info["motion_hit_transitions"] and not res.debug_info["motion_undecided_transitions"])
    assert res.debug_info["motion_hit_transitions"] == torch.nonzero(mc.hit[0]).flatten().tolist()
    assert bool(mc.any_hit[0]) == bool(res.debug_info["motion_hit_transitions"])
    if res.plan.is_valid:  # a valid plan's waypoints are collision-free: nodes 0 and M of every transition are not hit
        assert not bool(((mc.hit_node == 0) | (mc.hit_node == 64)).any())
    print(f"planner: is_valid={res.plan.is_valid} motion_certified={res.debug_info['motion_certified']} "
          f"hit={res.debug_info['motion_hit_transitions']} undecided={res.debug_info['motion_undecided_transitions']}")  # fmt: skip
