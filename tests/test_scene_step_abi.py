"""cppf_lm_full_step_scene (the coupled LM step on a whole obstacle scene) at the C ABI and in the Python keywords: the prototype,
every CPPF_ERR_INVALID refusal -- all decided before a device is selected, so a host-only handle serves -- and the refusal of
`device_loop=True` together with `scene_in_step=True`.  No GPU."""

import ctypes
import inspect

import pytest

from tests.test_abi import declared_functions
from tests.test_optloop_abi import _params


@pytest.fixture(scope="module")
def lib():
    from cppflow_amd import _hip, build

    build.build()
    return _hip.lib()


@pytest.fixture()
def handle(lib):
    from cppflow_amd import _hip
    from cppflow_amd.robot_model import canonicalize
    from cppflow_amd.robot_zoo import ROBOT_SPECS

    desc = _hip.chain_to_desc(canonicalize(ROBOT_SPECS["panda"]()))
    h = ctypes.c_void_p()
    assert lib.cppf_robot_create(ctypes.byref(desc), -12345, ctypes.byref(h)) == _hip.CPPF_OK, lib.cppf_last_error().decode()
    yield h
    lib.cppf_robot_destroy(h)


BUF = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is refused before any launch


FULL_STEP_ENTRY_POINTS = ("cppf_lm_full_step", "cppf_lm_full_step_pinned", "cppf_lm_full_step_scene")


def _call(lib, h, entry="cppf_lm_full_step_scene", **kw):
    """one coupled step through `entry` with everything in order but `kw` (the plain step takes no pin, only the scene step cuboids)"""
    P = _params()
    a = dict(x_in=BUF, target=BUF, virtual_configs=None, S=3, W=24, params=ctypes.byref(P.diff), pin=0, box_lo=BUF, box_hi=BUF, n_obs=9,
             blocks=BUF, G=BUF, y=BUF, x_out=ctypes.c_void_p(0x2000))  # fmt: skip
    a.update(kw)
    head = [h, a["x_in"], a["target"], a["virtual_configs"], a["S"], a["W"], a["params"]]
    mid = {"cppf_lm_full_step": [], "cppf_lm_full_step_pinned": [a["pin"]],
           "cppf_lm_full_step_scene": [a["pin"], a["box_lo"], a["box_hi"], a["n_obs"]]}[entry]  # fmt: skip
    return getattr(lib, entry)(*head, *mid, a["blocks"], a["G"], a["y"], a["x_out"], None)


def test_the_entry_point_is_declared_bound_and_exported(lib):
    from cppflow_amd import _hip
    from tests.test_abi import HEADER

    fn = "cppf_lm_full_step_scene"
    assert fn in declared_functions() and fn in _hip.SIGNATURES and getattr(lib, fn) is not None
    vp, ci = ctypes.c_void_p, ctypes.c_int
    res, args = _hip.SIGNATURES[fn]
    assert res is ci and args == [vp, vp, vp, vp, ci, ci, ctypes.POINTER(_hip.FullParams), ci, vp, vp, ci, vp, vp, vp, vp, vp]
    # the pinned step's list with (box_lo, box_hi, n_obs) between the mask and the workspaces
    pinned = _hip.SIGNATURES["cppf_lm_full_step_pinned"][1]
    assert args == pinned[:8] + [vp, vp, ci] + pinned[8:]
    assert lib.cppf_abi_version() == 6  # additive: the ABI version stays
    assert ctypes.sizeof(_hip.FullParams) == 92  # no public struct changed
    text = " ".join(open(HEADER).read().split())
    assert "int n_obs, float* work_blocks, float* work_G, float* work_y, float* x_out, void* stream);" in text


def test_bad_arguments_are_refused_before_the_device_is_selected(lib, handle):
    from cppflow_amd import _hip

    assert _call(lib, None) == _hip.CPPF_ERR_INVALID and "NULL" in lib.cppf_last_error().decode()
    cases = [(dict(**{name: None}), "NULL") for name in ("x_in", "target", "params", "box_lo", "box_hi", "blocks", "G", "y", "x_out")]
    cases += [
        (dict(n_obs=-1), "n_obs"),
        (dict(n_obs=4097), "n_obs"),
        (dict(pin=-1), "pin_mask"),
        (dict(pin=4), "pin_mask"),
        (dict(pin=1 << 20), "pin_mask"),
        (dict(S=-1), "S < 0"),
        (dict(W=0), "W < 1"),
    ]
    for kw, word in cases:
        assert _call(lib, handle, **kw) == _hip.CPPF_ERR_INVALID, kw
        assert word in lib.cppf_last_error().decode(), (kw, lib.cppf_last_error().decode())
    # box_lo / box_hi may be NULL with n_obs = 0 -- and only then: with S = 0 and everything else in order the call passes every
    # argument check (it ends at selecting the device of a host-only handle, or returns at once: nothing is launched either way)
    assert _call(lib, handle, box_lo=None, box_hi=None, n_obs=0, S=0) != _hip.CPPF_ERR_INVALID
    assert _call(lib, handle, box_lo=None, box_hi=None, n_obs=1, S=0) == _hip.CPPF_ERR_INVALID


@pytest.mark.parametrize("entry", FULL_STEP_ENTRY_POINTS)
def test_every_entry_point_refuses_what_the_step_refuses_before_the_device_is_selected(lib, handle, entry):
    """the step's one plan checks for all three: each fault alone is CPPF_ERR_INVALID on a handle whose device cannot be selected"""
    from cppflow_amd import _hip
    from tests.test_optloop_abi import FULL_STEP_VALUE_CASES

    cases = [(dict(**{name: None}), "NULL") for name in ("x_in", "target", "blocks", "G", "y", "x_out")]
    cases += [(dict(x_out=BUF), "alias"), (dict(W=8), "n_virtual_configs")]  # 2 * 4 virtual configs need more than 8 waypoints
    for fields, word in FULL_STEP_VALUE_CASES:
        P = _params(**{"diff_" + k: v for k, v in fields.items()})
        cases.append((dict(params=ctypes.byref(P.diff)), word))
    for kw, word in cases:
        assert _call(lib, handle, entry, **kw) == _hip.CPPF_ERR_INVALID, (kw, lib.cppf_last_error().decode())
        assert word in lib.cppf_last_error().decode(), (kw, lib.cppf_last_error().decode())
    # with everything in order the call passes every check and ends where the device would be selected: nothing was launched
    assert _call(lib, handle, entry) == _hip.CPPF_ERR_HIP, lib.cppf_last_error().decode()
    assert "device" in lib.cppf_last_error().decode()


def test_the_pinned_steps_unsupported_cases_are_kept(lib, handle):
    from cppflow_amd import _hip

    Q = _params(diff_differencing_mode=1)
    assert _call(lib, handle, params=ctypes.byref(Q.diff), pin=1) == _hip.CPPF_ERR_UNSUPPORTED
    assert "satisfied" in lib.cppf_last_error().decode()


def test_python_keywords_exist_and_default_to_off():
    from cppflow_amd.optimization import run_lm_optimization
    from cppflow_amd.planners import Planner
    from cppflow_amd.robots import Robot

    assert inspect.signature(Robot.lm_full_step).parameters["scene"].default is None
    assert inspect.signature(run_lm_optimization).parameters["scene_in_step"].default is False
    assert inspect.signature(Planner.__init__).parameters["scene_optimizer"].default is False


def test_the_planner_refuses_the_combination_at_construction():
    from cppflow_amd.data_types import PlannerSettings
    from cppflow_amd.planners import CppFlowPlanner

    settings = PlannerSettings(k=175, tmax_sec=3.0, anytime_mode_enabled=False, verbosity=0)
    with pytest.raises(AssertionError, match="scene_optimizer"):
        CppFlowPlanner(settings, object(), device_optimizer=True, scene_optimizer=True)
    assert CppFlowPlanner(settings, object(), scene_optimizer=True)._scene_optimizer is True


def test_the_device_loop_refuses_the_scene_step_before_touching_the_gpu():
    """the refusal comes first of all: not one argument is looked at, so placeholders serve and no device is needed"""
    from cppflow_amd.optimization import run_lm_optimization

    class Untouchable:
        def __getattr__(self, name):
            raise RuntimeError(f"run_lm_optimization looked at .{name} before refusing")

    with pytest.raises(AssertionError, match="scene_in_step"):
        run_lm_optimization(Untouchable(), Untouchable(), tmax_sec=None, max_n_steps=20, return_if_valid_after_n_steps=0,
                            convergence_threshold=1e6, device_loop=True, scene_in_step=True)  # fmt: skip
