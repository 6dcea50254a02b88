"""cppf_motion_resolve / cppf_motion_resolve_workspace_bytes (adaptive bisection of the motion test, csrc/kernels_motion_resolve.h) at
the C ABI: the prototypes and constants, every refusal -- all decided before a device is selected, so a host-only handle serves --
the workspace size, and the defaults of the new Python keywords.  No GPU."""

import ctypes
import inspect
import re

import pytest

from tests import helpers as H
from tests.test_abi import HEADER, declared_functions
from tests.test_motion_abi import _host_handle

WS_MESSAGE = "cppf_motion_resolve_workspace_bytes"


@pytest.fixture(scope="module")
def lib():
    from cppflow_amd import _hip, build

    build.build()
    return _hip.lib()


def test_entry_points_are_declared_bound_and_exported(lib):
    from cppflow_amd import _hip

    for fn in ("cppf_motion_resolve", "cppf_motion_resolve_workspace_bytes"):
        assert fn in declared_functions() and fn in _hip.SIGNATURES and getattr(lib, fn) is not None
    vp, ci, cf, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    res, args = _hip.SIGNATURES["cppf_motion_resolve"]
    assert res is ci and args == [vp, vp, ci, ci, ci, ci, ci, vp, vp, ci, cf, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    res, args = _hip.SIGNATURES["cppf_motion_resolve_workspace_bytes"]
    assert res is ci and args == [ci, ci, ci, ctypes.POINTER(sz)]
    text = open(HEADER).read()
    assert re.search(r"int cppf_motion_resolve_workspace_bytes\(int S, int W, int max_frontier, size_t\* bytes\);", text)
    assert re.search(r"int cppf_motion_resolve\(const cppf_robot\* robot, const float\* q, int S, int W, int start_level, int max_depth, "
                     r"int max_frontier,\s+const float\* box_lo, const float\* box_hi, int n_obs, float reach_m, const uint8_t\* decided,\s+"
                     r"uint8_t\* status, int32_t\* depth, int32_t\* hit_num, float\* min_clear, int32_t\* n_tested,\s+"
                     r"void\* workspace, size_t workspace_bytes, void\* stream\);", text)  # fmt: skip
    assert int(re.search(r"#define CPPF_MOTION_RESOLVE_MAX_DEPTH (\d+)", text).group(1)) == 16 == _hip.MOTION_RESOLVE_MAX_DEPTH
    assert int(re.search(r"#define CPPF_MOTION_RESOLVE_MAX_FRONTIER (\d+)", text).group(1)) == 4096 == _hip.MOTION_RESOLVE_MAX_FRONTIER
    assert int(re.search(r"#define CPPF_MOTION_OVERFLOW (\d+)", text).group(1)) == 4 == _hip.MOTION_OVERFLOW
    # what the uniform test pins stays as it was
    assert int(re.search(r"#define CPPF_MOTION_MAX_LEVEL (\d+)", text).group(1)) == 6 == _hip.MOTION_MAX_LEVEL
    assert (_hip.MOTION_CERTIFIED, _hip.MOTION_HIT) == (1, 2)
    assert lib.cppf_abi_version() == 6  # additive: the ABI version stays


def _nbytes(lib, S, W, F):
    from cppflow_amd import _hip

    out = ctypes.c_size_t(0)
    assert lib.cppf_motion_resolve_workspace_bytes(S, W, F, ctypes.byref(out)) == _hip.CPPF_OK, lib.cppf_last_error().decode()
    return out.value


def _call(lib, h, **kw):
    buf = ctypes.c_void_p(0x1000)  # never dereferenced: every call here is refused before any launch
    a = dict(q=buf, S=3, W=5, start_level=0, max_depth=16, max_frontier=512, box_lo=buf, box_hi=buf, n_obs=9, reach=0.05, decided=buf,
             status=buf, depth=buf, hit_num=buf, min_clear=buf, n_tested=buf, workspace=buf, workspace_bytes=1 << 30)  # fmt: skip
    a.update(kw)
    return lib.cppf_motion_resolve(h, a["q"], a["S"], a["W"], a["start_level"], a["max_depth"], a["max_frontier"], a["box_lo"], a["box_hi"],
                                   a["n_obs"], a["reach"], a["decided"], a["status"], a["depth"], a["hit_num"], a["min_clear"],
                                   a["n_tested"], a["workspace"], a["workspace_bytes"], None)  # fmt: skip


def test_bad_arguments_are_refused_before_the_device_is_selected(lib):
    from cppflow_amd import _hip

    assert _call(lib, None) == _hip.CPPF_ERR_INVALID and "NULL" in lib.cppf_last_error().decode()
    h = _host_handle(lib, H.chain("panda"))
    try:
        need = _nbytes(lib, 3, 5, 512)
        cases = [(dict(**{name: None}), "NULL") for name in ("q", "status", "box_lo", "box_hi", "workspace")]
        cases += [
            (dict(start_level=-1), "start_level"),
            (dict(start_level=7, max_depth=7), "start_level"),
            (dict(start_level=3, max_depth=2), "max_depth"),
            (dict(max_depth=17), "max_depth"),
            (dict(max_depth=-1), "max_depth"),
            (dict(max_frontier=0), "max_frontier"),
            (dict(start_level=4, max_frontier=15), "max_frontier"),
            (dict(max_frontier=4097), "max_frontier"),
            (dict(W=1), "W < 2"),
            (dict(W=0), "W < 2"),
            (dict(W=-3), "W < 2"),
            (dict(S=-1), "S < 0"),
            (dict(S=1 << 20, W=1 << 12), "2^31"),
            (dict(n_obs=-1), "n_obs"),
            (dict(n_obs=4097), "n_obs"),
            (dict(reach=-0.01), "reach"),
            (dict(reach=float("nan")), "reach"),
            (dict(reach=float("-inf")), "reach"),
            (dict(workspace_bytes=need - 1), WS_MESSAGE),
            (dict(workspace_bytes=0), WS_MESSAGE),
            (dict(workspace=ctypes.c_void_p(0x1004)), "aligned"),
        ]
        for kw, word in cases:
            assert _call(lib, h, **kw) == _hip.CPPF_ERR_INVALID, kw
            assert word in lib.cppf_last_error().decode(), (kw, lib.cppf_last_error().decode())
        # the optional outputs, no `decided`, an empty scene and the ends of every range are not refusals: with everything else in
        # order the call gets as far as selecting the device, which a host-only handle does not have (any code but CPPF_ERR_INVALID)
        for kw in (dict(depth=None, hit_num=None, min_clear=None, n_tested=None), dict(decided=None), dict(n_obs=0, box_lo=None, box_hi=None),
                   dict(reach=float("inf")), dict(start_level=6, max_depth=6, max_frontier=64), dict(start_level=0, max_depth=0, max_frontier=1),
                   dict(max_frontier=4096), dict(W=2), dict(workspace_bytes=need)):  # fmt: skip
            assert _call(lib, h, **kw) != _hip.CPPF_ERR_INVALID, (kw, lib.cppf_last_error().decode())
    finally:
        lib.cppf_robot_destroy(h)


def test_workspace_bytes(lib):
    from cppflow_amd import _hip

    shapes = ((0, 2, 1), (1, 2, 1), (1, 2, 8), (1, 5, 8), (3, 5, 8), (3, 12, 64), (3, 12, 512), (8, 256, 512), (8, 256, 4096))
    prev = 0
    for S, W, F in shapes:
        b = _nbytes(lib, S, W, F)
        assert b % 16 == 0 and b > 0 and b >= prev, (S, W, F, b)
        prev = b
    # monotone in each argument by itself
    for lo, hi in (((3, 12, 64), (4, 12, 64)), ((3, 12, 64), (3, 13, 64)), ((3, 12, 64), (3, 12, 65))):
        assert _nbytes(lib, *lo) <= _nbytes(lib, *hi)
    assert _nbytes(lib, 3, 12, 64) < _nbytes(lib, 6, 12, 64) and _nbytes(lib, 3, 12, 64) < _nbytes(lib, 3, 23, 64)
    assert _nbytes(lib, 3, 12, 64) < _nbytes(lib, 3, 12, 128)
    out = ctypes.c_size_t(0)
    for S, W, F in ((-1, 4, 8), (4, 1, 8), (4, 0, 8), (4, 4, 0), (4, 4, -1), (4, 4, 4097)):
        assert lib.cppf_motion_resolve_workspace_bytes(S, W, F, ctypes.byref(out)) == _hip.CPPF_ERR_INVALID, (S, W, F)
        assert lib.cppf_last_error().decode()
    assert lib.cppf_motion_resolve_workspace_bytes(4, 4, 8, None) == _hip.CPPF_ERR_INVALID


def test_the_new_keywords_and_their_defaults():
    from cppflow_amd.data_types import MotionClearance, PlannerSettings, Problem
    from cppflow_amd.planners import CppFlowPlanner, Planner
    from cppflow_amd.robots import Robot

    sig = inspect.signature(Robot.motion_resolve).parameters
    assert list(sig)[1:] == ["q", "box_lo", "box_hi", "start_level", "max_depth", "max_frontier", "reach", "decided", "want"]
    assert (sig["start_level"].default, sig["max_depth"].default, sig["max_frontier"].default, sig["reach"].default) == (0, 16, 512, 0.05)
    assert sig["decided"].default is None and tuple(sig["want"].default) == ("status", "depth", "hit_num", "min_clear", "n_tested")
    sig = inspect.signature(Problem.motion_clearance).parameters
    assert list(sig)[1:] == ["q_paths", "level", "reach_m", "resolve_depth"]
    assert sig["level"].default == 6 and sig["reach_m"].default == 0.05 and sig["resolve_depth"].default is None
    fields = MotionClearance.__dataclass_fields__
    assert all(fields[f].default is None for f in ("depth", "n_tested", "overflow")) and isinstance(MotionClearance.hit_param, property)
    assert inspect.signature(Planner.__init__).parameters["certify_motion_depth"].default is None
    settings = PlannerSettings(k=4, tmax_sec=1.0, anytime_mode_enabled=False)
    assert CppFlowPlanner(settings, object())._certify_motion_depth is None
    assert CppFlowPlanner(settings, object(), certify_motion_level=3)._certify_motion_depth is None
    p = CppFlowPlanner(settings, object(), certify_motion_level=3, certify_motion_depth=12)
    assert (p._certify_motion_level, p._certify_motion_depth) == (3, 12)
    assert CppFlowPlanner(settings, object(), certify_motion_level=6, certify_motion_depth=6)._certify_motion_depth == 6
    assert CppFlowPlanner(settings, object(), certify_motion_level=0, certify_motion_depth=16)._certify_motion_depth == 16
    for kw in (dict(certify_motion_depth=12), dict(certify_motion_level=3, certify_motion_depth=2), dict(certify_motion_level=3, certify_motion_depth=17)):
        with pytest.raises(AssertionError):
            CppFlowPlanner(settings, object(), **kw)


def test_hit_param_of_a_motion_clearance():
    import torch

    from cppflow_amd.data_types import MotionClearance

    z = torch.zeros((1, 3), dtype=torch.bool)
    hit_node = torch.tensor([[-1, 3, 0]], dtype=torch.int32)
    uniform = MotionClearance(certified=z, hit=z, min_clear=torch.zeros(1, 3), hit_node=hit_node, level=3, reach_m=0.05)
    assert uniform.depth is None and uniform.n_tested is None and uniform.overflow is None
    got = uniform.hit_param
    assert torch.isnan(got[0, 0]) and got[0, 1] == 0.375 and got[0, 2] == 0.0
    resolved = MotionClearance(certified=z, hit=z, min_clear=torch.zeros(1, 3), hit_node=hit_node, level=3, reach_m=0.05,
                               depth=torch.tensor([[3, 5, 9]], dtype=torch.int32))  # fmt: skip
    got = resolved.hit_param
    assert torch.isnan(got[0, 0]) and got[0, 1] == 3 / 32 and got[0, 2] == 0.0
