"""Adaptive bisection of the motion test on the MI355X: cppf_motion_resolve (csrc/kernels_motion_resolve.h) against its definition
(include/cppflow_hip.h), restated here breadth first on the fp32 oracle's per-pair and per-(capsule, cuboid) clearances.

Paths, scenes, seeds and robots are those of tests/test_gpu_motion.py (imported).  Cases are (S, W, n_obs, start_level, max_depth,
max_frontier).

Guard band, as in tests/test_gpu_motion.py.  The kernel decides  (c_i + c_{i+1}) - lambda 2^-L > 1e-6  in fp32; the restatement
evaluates the same expression in fp64 on the same fp32 clearances, table and |b - a|.  A transition is AMBIGUOUS when any decision
on its breadth-first path has an fp64 margin within 1e-5 of the threshold: such a transition is checked for invariants only, every
other one must match in every output, and at most 10 % of a robot's transitions may be ambiguous.

Nodes are formed exactly: i 2^-L (b - a) is exact in fp64, the sum with a is rounded once to fp32 -- the fp64 sum's error (TwoSum)
decides the rare case in which the fp64 sum is a tie of the fp32 grid."""

import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_gpu_motion import (BAND, CERT, DEV, HIT, REACH, REF, ROBOTS, SEEDS, SLACK, bits, boxes, chain, dev, host, make_paths, oracle,
                                   rho, robot, voxel_case)  # fmt: skip
from tests.test_gpu_motion import run as run_uniform

pytestmark = pytest.mark.gpu

OVF = 4
CASES = ((1, 2, 0, 0, 16, 512), (3, 12, 70, 0, 16, 512), (3, 12, 70, 6, 16, 512), (3, 5, 2, 3, 5, 512), (3, 12, 70, 0, 3, 512),
         (3, 12, 70, 0, 16, 8), (3, 12, 20, 2, 12, 64))  # fmt: skip
# Random waypoints of these scenes are mostly hit AT a waypoint or not at all; one more case per robot -- (3, 12, 70, 0, 16, 512) on
# paths from a seed picked with the oracle -- holds a transition that is HIT strictly between two clear waypoints.
HIT_SEEDS = {"panda": 2, "fetch": 6, "generic7": 4, "chain12": 1}
KEYS = ("status", "depth", "hit_num", "min_clear", "n_tested")
DTYPES = {"status": np.uint8, "depth": np.int32, "hit_num": np.int32, "min_clear": np.float32, "n_tested": np.int32}


def paths(name, S, W, seed=None):
    return make_paths(name, S, W, SEEDS[name] + 100 * S + W if seed is None else seed)  # (None: as `case` of tests/test_gpu_motion.py)


def cases_of(name):
    return CASES + ((3, 12, 70, 0, 16, 512, HIT_SEEDS[name]),)


def scene(name, n_obs):
    return tuple(a[:n_obs] for a in boxes(name))


def run(name, q, lo, hi, start_level, max_depth, max_frontier, reach=REACH, decided=None, want=KEYS, rb=None):
    got = (rb or robot(name)).motion_resolve(dev(q), dev(lo).reshape(-1, 3), dev(hi).reshape(-1, 3), start_level=start_level,
                                             max_depth=max_depth, max_frontier=max_frontier, reach=reach, decided=decided, want=want)  # fmt: skip
    torch.cuda.synchronize()
    return {k: host(v) for k, v in got.items()}


def same_bytes(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in KEYS)


# ---- the definition, restated ------------------------------------------------------------------------------------------------------------
def exact_nodes(a32, b32, L, i):
    """node (L, i[n]) between a32 and b32 [n, d]: fl32(a + i 2^-L (b - a)) with ONE rounding, a and b themselves at the ends"""
    a = a32.astype(np.float64)
    d = (b32 - a32).astype(np.float64)  # (the subtraction in fp32)
    p = (i.astype(np.float64) / float(1 << L))[:, None] * d  # exact: 17 bits x 24 bits
    s = a + p
    bb = s - a
    err = (a - (s - bb)) + (p - bb)  # TwoSum: a + p == s + err exactly
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    other = np.where(r64 > s, np.nextafter(r, np.float32(-np.inf)), np.nextafter(r, np.float32(np.inf)))
    tie = (r64 != s) & (np.abs(s - r64) == np.abs(other.astype(np.float64) - s)) & (err != 0)
    r = np.where(tie, np.where(err > 0, np.maximum(r, other), np.minimum(r, other)), r).astype(np.float32)
    r[i == 0] = a32[i == 0]
    r[i == (1 << L)] = b32[i == (1 << L)]
    return r


class Clearances:
    """the fp32 oracle's clearances at the nodes of one (robot, paths, scene), evaluated once per node whatever case asks for it"""

    def __init__(self, name, q, lo, hi):
        self.orc, (S, W, d) = oracle(name), q.shape
        self.a, self.b = q[:, :-1].reshape(-1, d), q[:, 1:].reshape(-1, d)
        self.lo, self.hi = lo.astype(np.float64), hi.astype(np.float64)
        self.cache = {}

    @staticmethod
    def canonical(tr, L, i):
        while L > 0 and i % 2 == 0:  # (L, i) and (L+1, 2i) are the same bits
            L, i = L - 1, i // 2
        return tr, L, i

    def get(self, keys):
        """[(tr, L, i)] -> (self [n, P], env [n, O * L]) in fp64, every value an fp32"""
        keys = [self.canonical(*k) for k in keys]
        miss = sorted({k for k in keys if k not in self.cache})
        for L in sorted({k[1] for k in miss}):
            ks = [k for k in miss if k[1] == L]
            tr, i = np.array([k[0] for k in ks]), np.array([k[2] for k in ks])
            x = exact_nodes(self.a[tr], self.b[tr], L, i).astype(np.float64)
            cs = self.orc.self_dists(x) if self.orc.n_pairs else np.zeros((len(ks), 0))
            ce = [self.orc.env_dists(x, self.lo[o], self.hi[o]) for o in range(self.lo.shape[0])]
            ce = np.stack(ce, axis=1).reshape(len(ks), -1) if ce else np.zeros((len(ks), 0))
            assert np.array_equal(cs.astype(np.float32).astype(np.float64), cs) and np.array_equal(ce.astype(np.float32).astype(np.float64), ce)
            for n, k in enumerate(ks):
                self.cache[k] = (cs[n], ce[n])
        return np.stack([self.cache[k][0] for k in keys]), np.stack([self.cache[k][1] for k in keys])


@functools.lru_cache(maxsize=None)
def clearances(name, S, W, n_obs, seed=None):
    return Clearances(name, paths(name, S, W, seed), *scene(name, n_obs))


def travel_bounds(name, q):
    """(lambda_p [S (W-1), P], lambda_c [S (W-1), L], inside [S (W-1)]) in fp64 from the handle's table and the fp32 |b - a|"""
    ch, r = chain(name), rho(name)
    S, W, d = q.shape
    dq = np.abs(q[:, 1:] - q[:, :-1]).astype(np.float64).reshape(-1, d)
    link = np.asarray(ch.cap_link)
    lam_p = np.zeros((dq.shape[0], len(ch.pairs)))
    for p, (c1, c2) in enumerate(np.asarray(ch.pairs)):
        if link[c1] > link[c2]:
            c1, c2 = c2, c1
        sel = (np.arange(d) > link[c1]) & (np.arange(d) <= link[c2])
        lam_p[:, p] = dq[:, sel] @ r[sel, c2]
    inside = ((q >= ch.lo.astype(np.float32)) & (q <= ch.hi.astype(np.float32))).all(axis=-1)
    return lam_p, dq @ r, (inside[:, :-1] & inside[:, 1:]).reshape(-1)


def restate(name, q, store, n_obs, start_level, max_depth, max_frontier, reach=REACH):
    """steps 1 .. 7 of the definition per transition -> dict of [S, W-1] arrays (KEYS, `ambiguous`, `frontier`: the largest |F|)"""
    S, W, _ = q.shape
    n_tr, n_caps = S * (W - 1), oracle(name).n_caps
    lam_p, lam_c, inside = travel_bounds(name, q)
    reach64 = float(np.float32(reach))
    out = {k: np.zeros(n_tr, dtype=DTYPES[k]) for k in KEYS}
    out["ambiguous"], out["frontier"] = np.zeros(n_tr, dtype=bool), np.zeros(n_tr, dtype=np.int64)
    for tr in range(n_tr):
        L, F, tested, minc, status, hit_num, amb = start_level, np.arange(1 << start_level), 0, np.float32(np.inf), 0, -1, False
        while True:
            out["frontier"][tr] = max(out["frontier"][tr], len(F))
            if len(F) > max_frontier:
                status = OVF
                break
            tested += len(F)
            nodes = np.union1d(F, F + 1)
            cs, ce = store.get([(tr, L, int(i)) for i in nodes])
            m_self = cs.min(axis=1) if cs.shape[1] else np.full(len(nodes), np.inf)
            m_env = ce.min(axis=1) if ce.shape[1] else np.full(len(nodes), np.inf)
            minc = min(minc, np.float32(np.minimum(m_self, np.where(m_env < reach64, m_env, np.inf)).min()))
            neg = np.minimum(m_self, m_env) < 0
            if neg.any():
                status, hit_num = HIT, int(nodes[neg.argmax()])
                break
            if not inside[tr]:
                break
            left, right = np.searchsorted(nodes, F), np.searchsorted(nodes, F + 1)
            cet = np.minimum(ce, reach64)
            scale = 1.0 / (1 << L)
            dec = [cs[left] + cs[right] - lam_p[tr][None, :] * scale - SLACK,
                   cet[left] + cet[right] - np.tile(lam_c[tr], n_obs)[None, :] * scale - SLACK]  # fmt: skip
            if n_obs > 0:  # a cuboid beyond reach at both ends, present or not: the kernel's once-per-capsule test
                dec.append(np.broadcast_to(2 * reach64 - lam_c[tr] * scale - SLACK, (len(F), n_caps)))
            dec = np.concatenate(dec, axis=1)
            amb = amb or bool((np.abs(dec) <= BAND).any())
            failing = F[~(dec > 0).all(axis=1)]
            if not len(failing):
                status = CERT
                break
            if L == max_depth:
                break
            F, L = np.stack([2 * failing, 2 * failing + 1], axis=1).reshape(-1), L + 1
        for k, v in (("status", status), ("depth", L), ("hit_num", hit_num), ("min_clear", minc), ("n_tested", tested), ("ambiguous", amb)):
            out[k][tr] = v
    return {k: v.reshape(S, W - 1) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def case(name, S, W, n_obs, start_level, max_depth, max_frontier, seed=None):
    """one launch and its restatement, shared by the tests below: (q, lo, hi, device outputs, restated)"""
    q = paths(name, S, W, seed)
    lo, hi = scene(name, n_obs)
    got = run(name, q, lo, hi, start_level, max_depth, max_frontier)
    return q, lo, hi, got, restate(name, q, clearances(name, S, W, n_obs, seed), n_obs, start_level, max_depth, max_frontier)


def check_invariants(got, start_level, max_depth, ctx):
    st = got["status"]
    assert np.isin(st, (0, CERT, HIT, OVF)).all(), ctx  # never CERTIFIED and HIT together, OVERFLOW alone
    assert ((got["depth"] >= start_level) & (got["depth"] <= max_depth)).all(), ctx
    assert np.array_equal(got["hit_num"] >= 0, st == HIT) and (got["hit_num"] <= (1 << got["depth"])).all(), ctx
    assert (got["n_tested"] >= (1 << start_level)).all(), ctx


# ---- 1. start_level == max_depth is the uniform test -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROBOTS)
def test_equals_the_uniform_test_when_the_depth_is_the_start_level(name):
    q = paths(name, 3, 12)
    for n_obs in (0, 2, 70):
        lo, hi = scene(name, n_obs)
        for L in (0, 3, 6):
            uni = run_uniform(name, q, lo, hi, L, want=("status", "min_clear", "hit_node"))
            got = run(name, q, lo, hi, L, L, 1 << L)
            ctx = (name, n_obs, L)
            assert np.array_equal(got["status"], uni["status"]), ctx
            assert np.array_equal(bits(got["min_clear"]), bits(uni["min_clear"])), ctx
            assert np.array_equal(got["hit_num"], uni["hit_node"]), ctx
            assert (got["n_tested"] == 1 << L).all() and (got["depth"] == L).all(), ctx  # (every waypoint is inside the limits)


# ---- 2. against the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROBOTS)
def test_restated_nodes_are_the_uniform_kernels_nodes(name):
    q = paths(name, 3, 12)
    S, W, d = q.shape
    a, b = q[:, :-1].reshape(-1, d), q[:, 1:].reshape(-1, d)
    lo, hi = scene(name, 0)
    for L in range(7):
        nodes = run_uniform(name, q, lo, hi, L, want=("status", "nodes"))["nodes"].reshape(S * (W - 1), (1 << L) + 1, d)
        for i in range((1 << L) + 1):
            assert np.array_equal(bits(exact_nodes(a, b, L, np.full(len(a), i))), bits(nodes[:, i])), (name, L, i)


@pytest.mark.parametrize("k", range(len(CASES) + 1))
@pytest.mark.parametrize("name", ROBOTS)
def test_against_the_restatement(name, k):
    c = cases_of(name)[k]
    (S, W, n_obs, start_level, max_depth, max_frontier), ctx = c[:6], (name,) + c
    _, _, _, got, want = case(name, *c)
    check_invariants(got, start_level, max_depth, ctx)
    sure = ~want["ambiguous"]
    print(f"{ctx}: {sure.size} transitions, {int((~sure).sum())} ambiguous, largest frontier {int(want['frontier'].max())}, "
          f"tests per transition {got['n_tested'].mean():.1f}, deepest {int(got['depth'].max())}")  # fmt: skip
    for k in ("status", "depth", "hit_num", "n_tested"):
        assert np.array_equal(got[k][sure], want[k][sure]), (ctx, k, got[k], want[k], sure)
    assert np.array_equal(bits(got["min_clear"])[sure], bits(want["min_clear"])[sure]), ctx
    if max_frontier == 512:
        assert want["frontier"].max() <= 154, ctx  # (what the cases were laid out for: 512 never overflows)


@pytest.mark.parametrize("name", ROBOTS)
def test_few_transitions_are_ambiguous(name):
    amb = np.concatenate([case(name, *c)[4]["ambiguous"].reshape(-1) for c in cases_of(name)])
    print(f"{name}: {int(amb.sum())} of {amb.size} transitions are ambiguous")
    assert amb.sum() <= 0.10 * amb.size, name


# ---- 3. every outcome occurs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROBOTS)
def test_the_cases_hold_every_outcome(name):
    seen = dict(certified_deeper=0, hit_deeper=0, floor=0, overflow=0)
    for c in cases_of(name):
        got, start_level, max_depth = case(name, *c)[3], c[3], c[4]
        st, dp = got["status"], got["depth"]
        seen["certified_deeper"] += int(((st == CERT) & (dp > start_level)).sum())
        seen["hit_deeper"] += int(((st == HIT) & (dp > start_level)).sum())
        seen["floor"] += int(((st == 0) & (dp == max_depth)).sum())
        seen["overflow"] += int((st == OVF).sum())
    print(name, seen)
    assert all(v > 0 for v in seen.values()), (name, seen)


# ---- 4. the case this exists for -------------------------------------------------------------------------------------------------------------
def test_resolve_certifies_what_level_6_leaves_undecided():
    q, lo, hi, got, _ = case("fetch", 3, 12, 70, 6, 16, 512)
    uni = run_uniform("fetch", q, lo, hi, 6, want=("status",))["status"]
    found = (uni == 0) & (got["status"] == CERT) & (got["depth"] > 6)
    print("fetch (3, 12, 70): undecided at level 6:", np.argwhere(uni == 0).tolist(), "certified at depths", got["depth"][found].tolist())
    assert found.any()
    assert np.array_equal(got["status"][uni != 0], uni[uni != 0])  # what level 6 decides stays decided the same way


@pytest.mark.parametrize("name", ROBOTS)
def test_nothing_stays_undecided_from_one_interval_down_to_depth_16(name):
    for n_obs in (70, 2):
        q = paths(name, 3, 12)
        got = case(name, 3, 12, 70, 0, 16, 512)[3] if n_obs == 70 else run(name, q, *scene(name, 2), 0, 16, 512)
        assert np.isin(got["status"], (CERT, HIT)).all(), (name, n_obs, got["status"], got["depth"])


# ---- 5. the voxel ------------------------------------------------------------------------------------------------------------------------------
def test_a_voxel_between_two_clear_waypoints():
    from tests.test_gpu_motion import VOXEL_T

    q, lo, hi, _, _ = voxel_case()
    got = run("panda", q, lo, hi, 0, 16, 512)
    assert got["status"][0, VOXEL_T] == HIT and got["depth"][0, VOXEL_T] >= 1, got
    assert got["hit_num"][0, VOXEL_T] / 2.0 ** got["depth"][0, VOXEL_T] <= 0.5 and got["min_clear"][0, VOXEL_T] < 0
    uni = run_uniform("panda", q, lo, hi, 0, want=("status", "hit_node"))
    assert uni["status"][0, VOXEL_T] == 0 and uni["hit_node"][0, VOXEL_T] == -1  # one interval sees nothing there
    without = run("panda", q, lo[:2], hi[:2], 0, 16, 512)
    assert without["status"][0, VOXEL_T] == CERT, without


# ---- 6. the prefix property --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROBOTS)
def test_a_deeper_floor_changes_nothing_that_ended_above_it(name):
    shallow, deep = case(name, 3, 12, 70, 0, 3, 512)[3], case(name, 3, 12, 70, 0, 16, 512)[3]
    ended = np.isin(shallow["status"], (CERT, HIT))
    assert ended.any() and (~ended).any() and (shallow["depth"][~ended] == 3).all()
    for k in KEYS:
        assert np.array_equal(shallow[k][ended].view(np.uint8), deep[k][ended].view(np.uint8)), (name, k)
    assert (deep["depth"][~ended] > 3).all() and (deep["n_tested"][~ended] > shallow["n_tested"][~ended]).all()


# ---- 7. soundness ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROBOTS)
def test_no_certified_transition_touches_anything_in_a_1025_sample_sweep(name):
    orc = oracle(name)
    certified = {}  # one sweep per (paths, scene): the transitions any case certified
    for c in cases_of(name):
        cert = case(name, *c)[3]["status"] == CERT
        key = c[:3] + c[6:]
        certified[key] = certified.get(key, False) | cert
    n_checked = 0
    for (S, W, n_obs, *seed), cert in certified.items():
        q, (lo, hi) = paths(name, S, W, *seed), scene(name, n_obs)
        cert = np.argwhere(cert)
        if not len(cert):
            continue
        f = (np.arange(1025) / 1024)[None, :, None]
        a = np.stack([q[s, t] for s, t in cert]).astype(np.float64)[:, None, :]
        b = np.stack([q[s, t + 1] for s, t in cert]).astype(np.float64)[:, None, :]
        x = H.f32((a + f * (b - a)).reshape(-1, q.shape[2]))
        worst = orc.self_dists(x).min(axis=1) if orc.n_pairs else np.full(x.shape[0], np.inf)
        for o in range(n_obs):
            worst = np.minimum(worst, orc.env_dists(x, lo[o].astype(np.float64), hi[o].astype(np.float64)).min(axis=1))
        assert (worst > 0).all(), (name, S, W, n_obs, float(worst.min()))
        n_checked += len(cert)
    assert n_checked > 0


# ---- 8. decided ----------------------------------------------------------------------------------------------------------------------------------
SENTINEL = 0x6B


def run_raw(rb, q, lo, hi, start_level, max_depth, max_frontier, bufs, decided_ptr, work, stream=None):
    """the entry point itself on caller-made buffers (uint8 views)"""
    from cppflow_amd import _hip

    S, W, _ = q.shape
    st = (stream if stream is not None else torch.cuda.current_stream(DEV)).cuda_stream
    _hip.check(_hip.lib().cppf_motion_resolve(rb._handle(torch.device(DEV)), q.data_ptr(), S, W, start_level, max_depth, max_frontier,
                                              lo.data_ptr(), hi.data_ptr(), lo.shape[0], REACH, decided_ptr, bufs["status"].data_ptr(),
                                              bufs["depth"].data_ptr(), bufs["hit_num"].data_ptr(), bufs["min_clear"].data_ptr(),
                                              bufs["n_tested"].data_ptr(), work.data_ptr(), work.numel(), st))  # fmt: skip
    torch.cuda.synchronize()


def workspace_bytes(S, W, max_frontier):
    from cppflow_amd import _hip

    nbytes = ctypes.c_size_t(0)
    _hip.check(_hip.lib().cppf_motion_resolve_workspace_bytes(S, W, max_frontier, ctypes.byref(nbytes)))
    return nbytes.value


@pytest.mark.parametrize("name,level", (("fetch", 6), ("generic7", 3)))
def test_decided_transitions_are_skipped_and_nothing_of_theirs_is_written(name, level):
    """`decided` = the uniform test's status at `level` (6 leaves nothing undecided on generic7's paths; 3 does), aliased to status"""
    rb = robot(name)
    q, lo, hi, full, _ = case(name, 3, 12, 70, level, 16, 512)
    S, W, _ = q.shape
    n_tr = S * (W - 1)
    qd, lod, hid = dev(q), dev(lo).reshape(-1, 3), dev(hi).reshape(-1, 3)
    uni = run_uniform(name, q, lo, hi, level, want=("status",))["status"].reshape(-1)
    assert (uni != 0).any() and (uni == 0).any()
    work = torch.empty(workspace_bytes(S, W, 512), dtype=torch.uint8, device=DEV)
    sizes = {k: n_tr * np.dtype(DTYPES[k]).itemsize for k in KEYS}
    bufs = {k: torch.full((sizes[k],), SENTINEL, dtype=torch.uint8, device=DEV) for k in KEYS}
    bufs["status"].copy_(dev(uni, torch.uint8))
    run_raw(rb, qd, lod, hid, level, 16, 512, bufs, bufs["status"].data_ptr(), work)  # decided IS status
    out = {k: host(bufs[k]).view(DTYPES[k]) for k in KEYS}
    skip = uni != 0
    assert np.array_equal(out["status"][skip], uni[skip])
    for k in KEYS[1:]:
        assert (out[k][skip].view(np.uint8) == SENTINEL).all(), k  # every byte kept
    for k in KEYS:
        assert np.array_equal(out[k][~skip].view(np.uint8), full[k].reshape(-1)[~skip].view(np.uint8)), k
    # the Python form completes a status in place
    st = dev(uni, torch.uint8).reshape(S, W - 1)
    res = rb.motion_resolve(qd, lod, hid, start_level=level, max_depth=16, decided=st)
    assert res["status"].data_ptr() == st.data_ptr() and np.array_equal(host(st), full["status"])
    # all-ones: nothing is written at all
    bufs = {k: torch.full((sizes[k],), SENTINEL, dtype=torch.uint8, device=DEV) for k in KEYS}
    ones = torch.ones(n_tr, dtype=torch.uint8, device=DEV)
    run_raw(rb, qd, lod, hid, 0, 16, 512, bufs, ones.data_ptr(), work)
    assert all(bool((bufs[k] == SENTINEL).all()) for k in KEYS) and bool((ones == 1).all())


# ---- 9. a stationary transition, a waypoint outside the limits -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ROBOTS)
def test_stationary_transitions_and_waypoints_outside_the_limits(name):
    ch, orc = chain(name), oracle(name)
    lo, hi = scene(name, 70)
    x = H.random_configs(name, 24, seed=9, margin=0.05) if name != "generic7" else H.f32(
        np.random.RandomState(9).uniform(ch.lo + 0.05, ch.hi - 0.05, size=(24, ch.ndof)))  # fmt: skip
    q = np.repeat(x.astype(np.float32)[:, None, :], 2, axis=1)  # [24, 2, d], a == b
    clear = orc.self_dists(x).min(axis=1) if orc.n_pairs else np.full(24, np.inf)
    for o in range(70):
        clear = np.minimum(clear, orc.env_dists(x, lo[o].astype(np.float64), hi[o].astype(np.float64)).min(axis=1))
    assert (clear > 1e-6).any() and (clear < 0).any() and not ((clear >= 0) & (clear <= 1e-6)).any()  # (nothing within the slack of 0)
    for start_level in (0, 3):
        got = run(name, q, lo, hi, start_level, 16, 512)
        assert np.array_equal(got["status"][:, 0] == CERT, clear > 1e-6), (name, start_level)
        assert np.array_equal(got["status"][:, 0] == HIT, clear < 0) and np.array_equal(got["hit_num"][:, 0] == 0, clear < 0)
        assert (got["depth"] == start_level).all() and (got["n_tested"] == 1 << start_level).all()
    free = np.flatnonzero(clear > 0.02)
    assert len(free) >= 2
    for start_level in (0, 2):
        for end in (0, 1):
            for side in (0, 1):
                qo = q[free].copy()
                j = (end + 2 * side) % ch.ndof
                qo[:, end, j] = np.float32(ch.hi[j]) + np.float32(0.01) if side else np.float32(ch.lo[j]) - np.float32(0.01)
                got = run(name, qo, lo[:0], hi[:0], start_level, 16, 512)
                assert not (got["status"] & CERT).any(), (name, end, side)
                assert (got["n_tested"] == 1 << start_level).all() and (got["depth"] == start_level).all(), (name, end, side)


# ---- 10. hygiene -------------------------------------------------------------------------------------------------------------------------------------
def run_in_arena(rb, q, lo, hi, start_level, max_depth, max_frontier, poison, stream=None):
    """the entry point with outputs and workspace carved out of one poisoned arena with guard gaps -> dict of host arrays"""
    S, W, _ = q.shape
    n_tr = S * (W - 1)
    arena = torch.full((1 << 21,), poison, dtype=torch.uint8, device=DEV)
    cursor, spans, bufs = 4096, [], {}
    sizes = (("workspace", workspace_bytes(S, W, max_frontier)),) + tuple((k, n_tr * np.dtype(DTYPES[k]).itemsize) for k in KEYS)
    for nm, nb in sizes:
        start = (cursor + 255) // 256 * 256
        bufs[nm] = arena[start : start + nb]
        spans.append((start, start + nb))
        cursor = start + nb + 1024
    assert cursor + 4096 < arena.numel()
    torch.cuda.synchronize()
    run_raw(rb, q, lo, hi, start_level, max_depth, max_frontier, bufs, None, bufs["workspace"], stream)
    keep = torch.ones(cursor + 4096, dtype=torch.bool, device=DEV)
    for a, b in spans:
        keep[a:b] = False
    assert bool((arena[: cursor + 4096][keep] == poison).all()), "a guard gap was written"
    return {k: host(bufs[k]).copy().view(DTYPES[k]) for k in KEYS}


@pytest.mark.parametrize("name,c", [("panda", CASES[1]), ("fetch", CASES[6]), ("generic7", CASES[5]), ("chain12", CASES[3])])
def test_memory_discipline_and_determinism(name, c):
    rb = robot(name)
    q, lo, hi, got, _ = case(name, *c)
    qd, lod, hid = dev(q), dev(lo).reshape(-1, 3), dev(hi).reshape(-1, 3)
    before = [t.clone() for t in (qd, lod, hid)]
    runs = [run_in_arena(rb, qd, lod, hid, *c[3:], 0xA5), run_in_arena(rb, qd, lod, hid, *c[3:], 0x5A),
            run_in_arena(rb, qd, lod, hid, *c[3:], 0xA5, torch.cuda.Stream(device=DEV))]  # fmt: skip
    for r in runs:
        assert same_bytes(r, {k: got[k].reshape(-1) for k in KEYS}), (name, c)
    for t, b in zip((qd, lod, hid), before):
        assert torch.equal(t.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("name", ROBOTS)
def test_permuted_paths_give_permuted_outputs_and_the_generic_form_agrees(name):
    rb = robot(name)
    c = CASES[1]
    q, lo, hi, got, _ = case(name, *c)
    perm = [2, 0, 1]
    assert same_bytes(run(name, q[perm], lo, hi, *c[3:]), {k: got[k][perm] for k in KEYS})
    if name == "generic7":
        assert rb.specialization() == -1
        return
    assert rb.specialization() >= 0  # a generated table
    rb.debug_set("force_generic", 1)
    try:
        gen = [run(name, *case(name, *cc)[:3], *cc[3:]) for cc in (c, CASES[6])]
    finally:
        rb.debug_set("force_generic", None)
    assert same_bytes(gen[0], got) and same_bytes(gen[1], case(name, *CASES[6])[3])


def test_a_handle_specialised_at_run_time_is_served_by_the_generic_form():
    from cppflow_amd.robots import Robot

    rtc = Robot(H.random_chain_spec(7, seed=21), specialize=True)
    assert rtc.specialization() == 1000
    for c in (CASES[1], CASES[6]):
        q, lo, hi, got, _ = case("generic7", *c)
        assert same_bytes(run("generic7", q, lo, hi, *c[3:], rb=rtc), got), c


def test_graph_capture_replays_the_call():
    rb = robot("panda")
    q, lo, hi, want, _ = case("panda", *CASES[1])
    qd, lod, hid = dev(q), dev(lo), dev(hi)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        rb.motion_resolve(qd, lod, hid)  # (warm: the allocator's pool, the handle)
        side.synchronize()
        with torch.cuda.graph(g, stream=side):
            got = rb.motion_resolve(qd, lod, hid)
    for v in got.values():
        v.view(torch.uint8).fill_(0x77)
    g.replay()
    torch.cuda.synchronize()
    assert same_bytes({k: host(v) for k, v in got.items()}, want)


# ---- 11. the planner ---------------------------------------------------------------------------------------------------------------------------
def test_the_planner_resolves_its_certificate_and_returns_the_same_plan():
    from cppflow_amd.data_type_utils import problem_from_filename
    from cppflow_amd.data_types import PlannerSettings
    from cppflow_amd.planners import CppFlowPlanner, TrackingSeedProvider

    problem = problem_from_filename(None, "panda__1cube_mini", problems_dir=os.path.join(REF, "problems"), paths_dir=os.path.join(REF, "paths"),
                                    device=DEV)  # fmt: skip
    settings = PlannerSettings(k=175, tmax_sec=60.0, anytime_mode_enabled=False, do_rerun_if_large_dp_search_mjac=False,
                               do_rerun_if_optimization_fails=False, verbosity=0)  # fmt: skip

    def plan(**kw):
        return CppFlowPlanner(settings, problem.robot, seed_provider=TrackingSeedProvider(seed=0), **kw).generate_plan(problem)

    plain, level, res = plan(), plan(certify_motion_level=3), plan(certify_motion_level=3, certify_motion_depth=12)
    new = ("motion_resolve_depth", "motion_tests_per_transition")
    keys = ("motion_certified", "motion_hit_transitions", "motion_undecided_transitions") + new
    assert all(k in res.debug_info for k in keys) and not any(k in level.debug_info for k in new)
    assert torch.equal(res.plan.q_path, plain.plan.q_path) and res.plan.is_valid == plain.plan.is_valid
    assert {k: v for k, v in res.debug_info.items() if k not in keys} == plain.debug_info
    assert set(res.debug_info["motion_undecided_transitions"]) <= set(level.debug_info["motion_undecided_transitions"])
    assert 3 <= res.debug_info["motion_resolve_depth"] <= 12 and res.debug_info["motion_tests_per_transition"] >= 8
    mc = problem.motion_clearance(res.plan.q_path, level=3, resolve_depth=12)
    T = problem.n_timesteps
    assert mc.certified.shape == (1, T - 1) and mc.depth.dtype == torch.int32 and mc.n_tested.dtype == torch.int32 and mc.overflow.dtype == torch.bool
    assert res.debug_info["motion_resolve_depth"] == int(mc.depth.max())
    assert res.debug_info["motion_undecided_transitions"] == torch.nonzero(mc.undecided[0]).flatten().tolist()
    assert not bool((mc.overflow & (mc.certified | mc.hit)).any())
    hp = mc.hit_param
    assert bool((torch.isnan(hp) == ~mc.hit).all()) and bool(((hp[mc.hit] >= 0) & (hp[mc.hit] <= 1)).all())
    print(f"planner: undecided at level 3 {level.debug_info['motion_undecided_transitions']}, resolved to depth 12 "
          f"{res.debug_info['motion_undecided_transitions']}; deepest {res.debug_info['motion_resolve_depth']}, "
          f"{res.debug_info['motion_tests_per_transition']:.1f} tests per transition")  # fmt: skip
