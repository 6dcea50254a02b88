"""Pinned end waypoints (CPPF_PIN_FIRST / CPPF_PIN_LAST) at the C ABI and in the Python keywords: the two entry points
(cppf_lm_full_step_pinned, cppf_lm_optimize_enqueue_pinned), the constants, and the refusals -- all of which come before a device is
selected, so a host-only handle serves.  No GPU."""

import ctypes
import dataclasses
import inspect
import re

import pytest

from tests.test_abi import HEADER, declared_functions
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


def _full_step(lib, h, P, pin, S=3, W=24):
    return lib.cppf_lm_full_step_pinned(h, BUF, BUF, None, S, W, ctypes.byref(P.diff), pin, BUF, BUF, BUF, ctypes.c_void_p(0x2000), None)


def _enqueue(lib, h, P, pin, S=3, W=24, n=1):
    return lib.cppf_lm_optimize_enqueue_pinned(h, BUF, BUF, S, W, ctypes.byref(P), pin, BUF, BUF, n, None)


def test_entry_points_and_constants_are_declared_bound_and_exported(lib):
    from cppflow_amd import _hip

    for fn in ("cppf_lm_full_step_pinned", "cppf_lm_optimize_enqueue_pinned"):
        assert fn in declared_functions() and fn in _hip.SIGNATURES and getattr(lib, fn) is not None
    assert lib.cppf_abi_version() == 6  # additive: the ABI version stays
    text = open(HEADER).read()
    for name, val in (("CPPF_PIN_FIRST", _hip.PIN_FIRST), ("CPPF_PIN_LAST", _hip.PIN_LAST)):
        assert re.search(rf"#define {name} {val}\b", text), name
    assert (_hip.PIN_FIRST, _hip.PIN_LAST) == (1, 2)
    # no public struct changed
    assert ctypes.sizeof(_hip.FullParams) == 92 and ctypes.sizeof(_hip.OptloopParams) == 160


def test_a_mask_outside_0_to_3_is_invalid_on_a_host_only_handle(lib, handle):
    from cppflow_amd import _hip

    for pin in (-1, 4, 7, 1 << 20):
        assert _full_step(lib, handle, _params(), pin) == _hip.CPPF_ERR_INVALID, pin
        assert "pin_mask" in lib.cppf_last_error().decode()
        assert _enqueue(lib, handle, _params(), pin) == _hip.CPPF_ERR_INVALID, pin
        assert "pin_mask" in lib.cppf_last_error().decode()
    # ... and so is a NULL handle / NULL params with a valid non-zero mask: checked before anything else is touched
    P = _params()
    assert lib.cppf_lm_full_step_pinned(None, BUF, BUF, None, 3, 24, ctypes.byref(P.diff), 1, BUF, BUF, BUF, BUF, None) == _hip.CPPF_ERR_INVALID
    assert lib.cppf_lm_full_step_pinned(handle, BUF, BUF, None, 3, 24, None, 1, BUF, BUF, BUF, BUF, None) == _hip.CPPF_ERR_INVALID


@pytest.mark.parametrize("pin", [1, 2, 3])
def test_the_satisfied_row_options_are_refused_with_a_pin(lib, handle, pin):
    from cppflow_amd import _hip

    for kw in (dict(diff_differencing_mode=1), dict(diff_differencing_mode=2, diff_differencing_scale_down=0.5),
               dict(diff_use_pose=1, diff_pose_do_scale_down_satisfied=1, diff_pose_scale_down=0.5)):  # fmt: skip
        assert _full_step(lib, handle, _params(**kw), pin) == _hip.CPPF_ERR_UNSUPPORTED, kw
        assert "satisfied" in lib.cppf_last_error().decode()
    assert _enqueue(lib, handle, _params(diff_differencing_mode=1), pin) == _hip.CPPF_ERR_UNSUPPORTED


@pytest.mark.parametrize("pin", [1, 2, 3])
def test_an_invalid_value_is_invalid_with_a_pin_too(lib, handle, pin):
    """the value checks come before what a pin does not combine with: a "satisfied" option out of range is CPPF_ERR_INVALID, not
    CPPF_ERR_UNSUPPORTED -- on the step and, for what the device loop's own refusals let through, on the loop"""
    from cppflow_amd import _hip
    from tests.test_optloop_abi import FULL_STEP_VALUE_CASES

    for fields, word in FULL_STEP_VALUE_CASES:
        P = _params(**{"diff_" + k: v for k, v in fields.items()})
        assert _full_step(lib, handle, P, pin) == _hip.CPPF_ERR_INVALID, (fields, lib.cppf_last_error().decode())
        assert word in lib.cppf_last_error().decode(), (fields, lib.cppf_last_error().decode())
        if "differencing_mode" not in fields:  # (the loop refuses weighted differencing rows as unsupported, whatever their values)
            assert _enqueue(lib, handle, P, pin) == _hip.CPPF_ERR_INVALID, (fields, lib.cppf_last_error().decode())
            assert word in lib.cppf_last_error().decode(), (fields, lib.cppf_last_error().decode())
    assert _full_step(lib, handle, _params(), pin, W=8) == _hip.CPPF_ERR_INVALID and "n_virtual_configs" in lib.cppf_last_error().decode()
    # with everything in order the pinned step passes every check and ends where the device would be selected
    assert _full_step(lib, handle, _params(), pin) == _hip.CPPF_ERR_HIP, lib.cppf_last_error().decode()


def test_the_one_wavefront_cross_check_kernel_refuses_a_pin(lib, handle):
    """full_rows = 0 beyond the parallel-in-time form's sizes resolves to full_solve_wave_kernel, which takes no pin"""
    from cppflow_amd import _hip

    keys = _hip.TUNE_KEYS
    try:
        assert lib.cppf_debug_set(handle, keys["full_rows"], 0) == _hip.CPPF_OK
        assert lib.cppf_debug_set(handle, keys["pcr_max_rows"], 0) == _hip.CPPF_OK
        assert _full_step(lib, handle, _params(), 1) == _hip.CPPF_ERR_UNSUPPORTED
        assert "one-wavefront" in lib.cppf_last_error().decode()
    finally:
        for k in ("full_rows", "pcr_max_rows"):
            assert lib.cppf_debug_set(handle, keys[k], _hip.TUNE_DEFAULT) == _hip.CPPF_OK


def test_enqueue_with_a_pin_keeps_the_plain_refusals_and_zero_iterations_are_ok(lib, handle):
    from cppflow_amd import _hip

    assert _enqueue(lib, handle, _params(), 1, n=0) == _hip.CPPF_OK
    assert _enqueue(lib, handle, _params(), 3, W=8) == _hip.CPPF_ERR_INVALID  # 2 * 4 virtual configs need more than 8 waypoints
    assert _enqueue(lib, handle, _params(diff_use_pose=1), 1) == _hip.CPPF_ERR_UNSUPPORTED


def test_python_keywords_exist_and_default_to_off():
    from cppflow_amd.optimization import OptimizationProblem, _pinned_rows, run_lm_optimization
    from cppflow_amd.planners import Planner
    from cppflow_amd.robots import Robot

    assert inspect.signature(Robot.lm_full_step).parameters["pin"].default == 0
    assert inspect.signature(Robot.lm_optimize_enqueue).parameters["pin"].default == 0
    sig = inspect.signature(run_lm_optimization).parameters
    assert sig["pin_first"].default is False and sig["pin_last"].default is False
    assert inspect.signature(Planner.__init__).parameters["pin_initial_configuration"].default is False
    f = {x.name: x for x in dataclasses.fields(OptimizationProblem)}
    assert f["pin_mask"].default == 0 and list(f)[-1] == "pin_mask"  # defaulted and last: positional constructors keep working
    # every combination of pin_first / pin_last is served, so run_lm_optimization has none to reject; the row bookkeeping of the
    # host loop: rows of the pinned waypoints of S stacked trajectories
    assert _pinned_rows(0, 3, 5, "cpu") is None
    assert _pinned_rows(1, 3, 5, "cpu").tolist() == [0, 5, 10]
    assert _pinned_rows(2, 3, 5, "cpu").tolist() == [4, 9, 14]
    assert _pinned_rows(3, 2, 5, "cpu").tolist() == [0, 4, 5, 9]
    assert _pinned_rows(3, 2, 1, "cpu").tolist() == [0, 1]  # W = 1: first and last are the same row
    with pytest.raises(AssertionError):
        _pinned_rows(4, 1, 5, "cpu")
