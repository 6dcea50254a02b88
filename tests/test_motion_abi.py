"""cppf_motion_clearance / cppf_motion_workspace_bytes / cppf_motion_rho (the motion between waypoints, csrc/kernels_motion.h) at the
C ABI: the prototypes, every refusal -- all decided before a device is selected, so a host-only handle serves -- the travel-bound
table against hand-computed values, and the planner keyword's default.  No GPU.  (The destroyed handle: tests/test_gpu_motion.py.)"""

import ctypes
import inspect

import numpy as np
import pytest

from tests import helpers as H
from tests.test_abi import declared_functions

NO_DEVICE = -12345


@pytest.fixture(scope="module")
def lib():
    from cppflow_amd import _hip, build

    build.build()
    return _hip.lib()


def test_entry_points_are_declared_bound_and_exported(lib):
    import re

    from cppflow_amd import _hip
    from tests.test_abi import HEADER

    for fn in ("cppf_motion_clearance", "cppf_motion_workspace_bytes", "cppf_motion_rho"):
        assert fn in declared_functions() and fn in _hip.SIGNATURES and getattr(lib, fn) is not None
    vp, ci, cf, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    res, args = _hip.SIGNATURES["cppf_motion_clearance"]
    assert res is ci and args == [vp, vp, ci, ci, ci, vp, vp, ci, cf, vp, vp, vp, vp, vp, sz, vp]
    res, args = _hip.SIGNATURES["cppf_motion_workspace_bytes"]
    assert res is ci and args == [ci, ci, ctypes.POINTER(sz)]
    text = open(HEADER).read()
    assert re.search(r"int cppf_motion_clearance\(const cppf_robot\* robot, const float\* q, int S, int W, int level, const float\* box_lo, "
                     r"const float\* box_hi,\s+int n_obs, float reach_m, uint8_t\* status, float\* min_clear, int32_t\* hit_node, "
                     r"float\* nodes, void\* workspace,\s+size_t workspace_bytes, void\* stream\);", text)  # fmt: skip
    assert int(re.search(r"#define CPPF_MOTION_MAX_LEVEL (\d+)", text).group(1)) == 6 == _hip.MOTION_MAX_LEVEL
    assert int(re.search(r"#define CPPF_MOTION_CERTIFIED (\d+)", text).group(1)) == 1 == _hip.MOTION_CERTIFIED
    assert int(re.search(r"#define CPPF_MOTION_HIT (\d+)", text).group(1)) == 2 == _hip.MOTION_HIT
    assert lib.cppf_abi_version() == 6  # additive: the ABI version stays


def _host_handle(lib, chain):
    from cppflow_amd import _hip

    desc = _hip.chain_to_desc(chain)
    h = ctypes.c_void_p()
    assert lib.cppf_robot_create(ctypes.byref(desc), NO_DEVICE, ctypes.byref(h)) == _hip.CPPF_OK, lib.cppf_last_error().decode()
    return h


def _nbytes(lib, S, W):
    from cppflow_amd import _hip

    out = ctypes.c_size_t(0)
    assert lib.cppf_motion_workspace_bytes(S, W, ctypes.byref(out)) == _hip.CPPF_OK, lib.cppf_last_error().decode()
    return out.value


def _call(lib, h, **kw):
    buf = ctypes.c_void_p(0x1000)  # never dereferenced: every call here is refused before any launch
    a = dict(q=buf, S=3, W=5, level=6, box_lo=buf, box_hi=buf, n_obs=9, reach=0.05, status=buf, min_clear=buf, hit_node=buf, nodes=buf,
             workspace=buf, workspace_bytes=1 << 30)  # fmt: skip
    a.update(kw)
    return lib.cppf_motion_clearance(h, a["q"], a["S"], a["W"], a["level"], a["box_lo"], a["box_hi"], a["n_obs"], a["reach"], a["status"],
                                     a["min_clear"], a["hit_node"], a["nodes"], a["workspace"], a["workspace_bytes"], None)  # fmt: skip


def test_bad_arguments_are_refused_before_the_device_is_selected(lib):
    from cppflow_amd import _hip

    assert _call(lib, None) == _hip.CPPF_ERR_INVALID and "NULL" in lib.cppf_last_error().decode()
    h = _host_handle(lib, H.chain("panda"))
    try:
        need = _nbytes(lib, 3, 5)
        cases = [(dict(**{name: None}), "NULL") for name in ("q", "status", "box_lo", "box_hi", "workspace")]
        cases += [
            (dict(level=-1), "level"),
            (dict(level=7), "level"),
            (dict(W=1), "W < 2"),
            (dict(W=0), "W < 2"),
            (dict(W=-3), "W < 2"),
            (dict(S=-1), "S < 0"),
            (dict(S=1 << 15, W=1 << 12), "2^31"),
            (dict(n_obs=-1), "n_obs"),
            (dict(n_obs=4097), "n_obs"),
            (dict(reach=-0.01), "reach"),
            (dict(reach=float("nan")), "reach"),
            (dict(reach=float("-inf")), "reach"),
            (dict(workspace_bytes=need - 1), "workspace"),
            (dict(workspace_bytes=0), "workspace"),
            (dict(workspace=ctypes.c_void_p(0x1004)), "aligned"),
        ]
        for kw, word in cases:
            assert _call(lib, h, **kw) == _hip.CPPF_ERR_INVALID, kw
            assert word in lib.cppf_last_error().decode(), (kw, lib.cppf_last_error().decode())
        # the optional outputs and an empty scene are not refusals: with everything else in order the call gets as far as selecting
        # the device, which a host-only handle does not have (any code but CPPF_ERR_INVALID)
        for kw in (dict(min_clear=None, hit_node=None, nodes=None), dict(n_obs=0, box_lo=None, box_hi=None), dict(reach=float("inf")),
                   dict(level=0), dict(W=2)):  # fmt: skip
            assert _call(lib, h, **kw) != _hip.CPPF_ERR_INVALID, (kw, lib.cppf_last_error().decode())
        assert lib.cppf_motion_rho(h, None) == _hip.CPPF_ERR_INVALID
        assert lib.cppf_motion_rho(None, ctypes.cast(ctypes.c_void_p(0x1000), ctypes.POINTER(ctypes.c_float))) == _hip.CPPF_ERR_INVALID
    finally:
        lib.cppf_robot_destroy(h)


def test_workspace_bytes(lib):
    from cppflow_amd import _hip

    prev = 0
    for S, W in ((0, 2), (1, 2), (1, 5), (3, 12), (8, 256), (175, 25)):
        b = _nbytes(lib, S, W)
        assert b % 16 == 0 and b >= 12 * S * (W - 1) and b > 0 and b >= prev  # three 32-bit words per transition
        prev = b
    out = ctypes.c_size_t(0)
    for S, W in ((-1, 4), (4, 1), (4, 0)):
        assert lib.cppf_motion_workspace_bytes(S, W, ctypes.byref(out)) == _hip.CPPF_ERR_INVALID, (S, W)
        assert lib.cppf_last_error().decode()
    assert lib.cppf_motion_workspace_bytes(4, 4, None) == _hip.CPPF_ERR_INVALID


def _rho(lib, chain):
    from cppflow_amd import _hip
    from cppflow_amd.robot_model import MAX_CAPSULES, MAX_DOF

    h = _host_handle(lib, chain)
    try:
        rho = np.full((MAX_DOF, MAX_CAPSULES), -1.0, dtype=np.float32)
        assert lib.cppf_motion_rho(h, _hip.fptr(rho)) == _hip.CPPF_OK
    finally:
        lib.cppf_robot_destroy(h)
    assert (rho[chain.ndof :] == 0).all() and (rho[:, chain.n_capsules :] == 0).all()
    return rho[: chain.ndof, : chain.n_capsules]


def rho_fp64(chain):
    """the definition of include/cppflow_hip.h restated in fp64 on the canonical chain (the fp32 values a handle is created from)"""
    F = np.asarray(chain.F, dtype=np.float32).astype(np.float64)
    lo, hi = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (chain.lo, chain.hi))
    p0, p1 = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (chain.cap_p0, chain.cap_p1))
    r = np.asarray(chain.cap_r, dtype=np.float32).astype(np.float64)
    rho = np.zeros((chain.ndof, chain.n_capsules))
    for c in range(chain.n_capsules):
        l = int(chain.cap_link[c])
        for j in range(l + 1):
            if chain.jtype[j] == 1:
                rho[j, c] = 1.0
                continue
            s = max(np.linalg.norm(p0[c]), np.linalg.norm(p1[c])) + r[c]
            for i in range(j + 1, l + 1):
                s += np.linalg.norm(F[i, 9:12])
                if chain.jtype[i] == 1:
                    s += max(abs(lo[i]), abs(hi[i]))
            rho[j, c] = s
    return rho


def _rounded_up(got, want):
    """got (fp32) is `want` (fp64) rounded UP: never below, and less than one fp32 step above"""
    got64 = got.astype(np.float64)
    below = np.nextafter(got, np.float32(-np.inf)).astype(np.float64)
    return bool((got64 >= want).all() and ((below < want) | (got64 == want)).all())


def test_travel_bounds_of_the_two_capsule_chain_by_hand(lib):
    """three coincident revolute joints (no offsets), a capsule on the base and one on the last link with end points at distance
    0.5 and 0.25 of the link's origin, radius 0: rho = 0.5 under every joint for the moving capsule, 0 for the base capsule"""
    chain = H.two_capsule_chain(((0.0, 0.0, 0.0), (1.0, 0.0, 0.0)), ((0.3, 0.0, 0.4), (0.0, 0.0, 0.25)))
    assert chain.ndof == 3 and list(chain.cap_link) == [-1, 2] and not np.asarray(chain.F)[:, 9:12].any()
    rho = _rho(lib, chain)
    assert (rho[:, 0] == 0).all()
    # |(0.3, 0, 0.4)| in the fp32 end points is 0.5 to within an fp32 step; the table is rounded up from the fp64 value
    assert np.allclose(rho[:, 1], 0.5, rtol=0, atol=1e-7) and (rho[:, 1] >= np.float32(0.5) - np.float32(6e-8)).all()
    assert _rounded_up(rho, rho_fp64(chain))


def test_travel_bounds_of_fetch_and_of_a_prismatic_joint_in_mid_chain(lib):
    chain = H.chain("fetch")
    assert chain.jtype[0] == 1 and not chain.jtype[1:].any()  # the torso lift, then seven revolute joints
    rho = _rho(lib, chain)
    moving = np.asarray(chain.cap_link) >= 0
    assert moving.any() and (~moving).any()
    assert (rho[0, moving] == 1.0).all() and (rho[0, ~moving] == 0.0).all()  # a prismatic joint moves every point as far as itself
    for c in range(chain.n_capsules):
        l = int(chain.cap_link[c])
        assert (rho[l + 1 :, c] == 0).all()  # joints behind the link
        if l >= 1:
            assert (np.diff(rho[1 : l + 1, c]) <= 0).all() and rho[l, c] > 0  # nearer joints, shorter arms
    assert _rounded_up(rho, rho_fp64(chain))
    # by hand, Fetch's gripper capsule under the wrist roll joint: only the capsule's own extent
    c = chain.n_capsules - 1
    l = int(chain.cap_link[c])
    by_hand = max(np.linalg.norm(np.float32(chain.cap_p0[c]).astype(np.float64)), np.linalg.norm(np.float32(chain.cap_p1[c]).astype(np.float64))) + float(np.float32(chain.cap_r[c]))
    assert abs(float(rho[l, c]) - by_hand) <= 1.2e-7 * by_hand and float(rho[l, c]) >= by_hand
    # a prismatic joint between a revolute joint and the capsule adds its largest excursion: a 3-joint chain R - P - R by hand
    from cppflow_amd.robot_model import CapsuleSpec, JointSpec, RobotSpec, canonicalize

    joints = [JointSpec("j0", "l0", (0, 0, 0.5), (0, 0, 0), (0, 0, 1), "revolute", (-1.0, 1.0)),
              JointSpec("j1", "l1", (0, 0, 0.25), (0, 0, 0), (0, 0, 1), "prismatic", (-0.125, 0.375)),
              JointSpec("j2", "l2", (0, 0, 0.125), (0, 0, 0), (0, 0, 1), "revolute", (-1.0, 1.0))]  # fmt: skip
    spec = RobotSpec("rpr", "R-P-R", "base", joints, [CapsuleSpec("base", (0, 0, 0), (0, 0, 0.1), 0.0625), CapsuleSpec("l2", (0, 0, 0), (0, 0, 0.5), 0.0625)],
                     collision_pairs=[(0, 1)])  # fmt: skip
    rpr = canonicalize(spec)
    assert list(rpr.jtype) == [0, 1, 0] and list(rpr.cap_link) == [-1, 2]
    got = _rho(lib, rpr)
    #               |t_1|  |t_2|   max|limit|  extent  radius
    assert got[0, 1] == np.float32(0.25 + 0.125 + 0.375 + 0.5 + 0.0625)
    assert got[1, 1] == 1.0 and got[2, 1] == np.float32(0.5 + 0.0625) and (got[:, 0] == 0).all()


def test_the_planner_keyword_is_off_by_default():
    from cppflow_amd.data_types import MotionClearance, PlannerSettings, Problem
    from cppflow_amd.planners import CppFlowPlanner, Planner

    assert inspect.signature(Planner.__init__).parameters["certify_motion_level"].default is None
    settings = PlannerSettings(k=4, tmax_sec=1.0, anytime_mode_enabled=False)
    planner = CppFlowPlanner(settings, object())
    assert planner._certify_motion_level is None
    assert CppFlowPlanner(settings, object(), certify_motion_level=6)._certify_motion_level == 6
    with pytest.raises(AssertionError):
        CppFlowPlanner(settings, object(), certify_motion_level=7)
    sig = inspect.signature(Problem.motion_clearance).parameters
    assert sig["level"].default == 6 and sig["reach_m"].default == 0.05
    assert {"certified", "hit", "min_clear", "hit_node"} <= {f for f in MotionClearance.__dataclass_fields__}
    from cppflow_amd.robots import Robot

    sig = inspect.signature(Robot.motion_clearance).parameters
    assert sig["level"].default == 6 and sig["reach"].default == 0.05
