"""cppf_lm_optimize_enqueue (the alternating LM optimiser loop decided on the device, csrc/kernels_optloop.h) at the C ABI: header /
binding agreement of the three structs and of the constants, and the argument checks -- all of which come before a device is
touched, so a host-only handle serves.  No GPU."""

import ctypes
import re

import pytest

from tests.test_abi import HEADER, declared_functions


@pytest.fixture(scope="module")
def lib():
    from cppflow_amd import _hip, build

    build.build()
    return _hip.lib()


def _struct_fields(name):
    """field names of `typedef struct <name> { ... } <name>;` in the header, in order (comments stripped, arrays as name)"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = decl.split(None, 1)[1]
        out += [re.sub(r"\[.*\]", "", n.strip()) for n in names.split(",")]
    return out


def test_entry_points_are_declared_bound_and_exported(lib):
    from cppflow_amd import _hip

    for fn in ("cppf_lm_optimize_enqueue", "cppf_lm_optimize_workspace_bytes", "cppf_lm_optimize_control_bytes"):
        assert fn in declared_functions() and fn in _hip.SIGNATURES and getattr(lib, fn) is not None
    assert lib.cppf_abi_version() == 6  # additive: the ABI version stays


def test_struct_layouts_and_constants_agree_with_the_header():
    from cppflow_amd import _hip

    for cname, cls in (("cppf_optloop_record", _hip.OptloopRecord), ("cppf_optloop_trace", _hip.OptloopTrace),
                       ("cppf_optloop_params", _hip.OptloopParams)):  # fmt: skip
        assert _struct_fields(cname) == [f[0] for f in cls._fields_], cname
    assert ctypes.sizeof(_hip.OptloopRecord) == 64 and ctypes.sizeof(_hip.OptloopTrace) == 16
    # 3 floats, cppf_full_params (23 words), cppf_constraints (6 words), 6 int32, one double (8-aligned at 152)
    assert ctypes.sizeof(_hip.FullParams) == 92 and ctypes.sizeof(_hip.Constraints) == 24
    assert ctypes.sizeof(_hip.OptloopParams) == 160 and _hip.OptloopParams.convergence_threshold.offset == 152
    assert _hip.OptloopRecord.mode.offset == 0  # the launch gate reads a record's first word
    text = open(HEADER).read()
    for name, val in (("CPPF_OPT_MODE_POSE", _hip.OPT_MODE_POSE), ("CPPF_OPT_MODE_DIFF", _hip.OPT_MODE_DIFF),
                      ("CPPF_OPT_MODE_DONE", _hip.OPT_MODE_DONE),
                      ("CPPF_OPT_ON_POSE_VALID_DIFFERENCING", _hip.OPT_ON_POSE_VALID["differencing"]),
                      ("CPPF_OPT_ON_POSE_VALID_STOP", _hip.OPT_ON_POSE_VALID["stop"]),
                      ("CPPF_OPT_ON_POSE_VALID_CONTINUE", _hip.OPT_ON_POSE_VALID["continue"])):  # fmt: skip
        assert re.search(rf"#define {name} {val}\b", text), name
    # the initial control block: every record leads with a pose step
    w = _hip.optloop_initial_control(3, 5)
    assert w.size == 3 * 16 + 3 * 5 * 4
    r = _hip.OptloopRecord.from_buffer_copy(w[16:32].tobytes())
    assert (r.mode, r.pose_pos_valid, r.pose_rot_valid, r.last_valid_idx, r.n_steps, r.is_valid) == (_hip.OPT_MODE_POSE, 1, 0, -1, 0, 0)
    assert _hip.optloop_flags(-1) is None and _hip.optloop_flags(0b10_01_1011) == (True, True, False, True, False, True)


def _params(**kw):
    from cppflow_amd import _hip
    from cppflow_amd.lm_hyper_parameters import ALT_LOSS_V2_1_DIFF
    from cppflow_amd.robots import Robot

    P = _hip.OptloopParams()
    P.pose_lm_lambda, P.pose_alpha_position, P.pose_alpha_rotation = 1e-6, 3.5, 0.35
    P.diff = Robot.full_params(ALT_LOSS_V2_1_DIFF)
    P.constraints = _hip.Constraints(0.01, 0.1, 3.0, 2.0, 0, 0)
    P.max_n_steps, P.return_if_valid_after_n_steps, P.trace_capacity, P.convergence_threshold = 20, 15, 20, 0.3
    for k, v in kw.items():
        if k.startswith("diff_"):
            setattr(P.diff, k[5:], v)
        else:
            setattr(P, k, v)
    return P


# what a coupled step refuses by the values in its cppf_full_params, whichever entry point takes them (this file, test_pin_abi.py,
# test_scene_step_abi.py): (fields, word in the message)
FULL_STEP_VALUE_CASES = [
    (dict(lm_lambda=0.0), "lm_lambda"),
    (dict(differencing_mode=3), "differencing_mode"),
    (dict(differencing_mode=2, differencing_scale_down=1.5), "scale-down"),
    (dict(pose_do_scale_down_satisfied=1, pose_scale_down=2.0), "scale-down"),
]


def test_null_robot_is_refused_with_a_message(lib):
    from cppflow_amd import _hip

    P = _params()
    n = ctypes.c_size_t(0)
    assert lib.cppf_lm_optimize_enqueue(None, None, None, 1, 16, ctypes.byref(P), None, None, 1, None) == _hip.CPPF_ERR_INVALID
    assert "NULL" in lib.cppf_last_error().decode()
    assert lib.cppf_lm_optimize_workspace_bytes(None, 1, 16, ctypes.byref(n)) == _hip.CPPF_ERR_INVALID
    assert lib.cppf_lm_optimize_control_bytes(1, None, ctypes.byref(n)) == _hip.CPPF_ERR_INVALID


def test_bad_arguments_are_refused_before_any_launch_and_sizes_are_as_documented(lib):
    from cppflow_amd import _hip
    from cppflow_amd.robot_model import canonicalize
    from cppflow_amd.robot_zoo import ROBOT_SPECS

    desc = _hip.chain_to_desc(canonicalize(ROBOT_SPECS["panda"]()))
    h = ctypes.c_void_p()
    assert lib.cppf_robot_create(ctypes.byref(desc), -12345, ctypes.byref(h)) == _hip.CPPF_OK, lib.cppf_last_error().decode()
    try:
        buf = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is refused before any launch
        cases = [
            (dict(), dict(x=None), "NULL"),
            (dict(), dict(target=None), "NULL"),
            (dict(), dict(workspace=None), "NULL"),
            (dict(), dict(control=None), "NULL"),
            (dict(), dict(workspace=ctypes.c_void_p(0x1004)), "aligned"),
            (dict(), dict(S=0), "S / W"),
            (dict(), dict(W=0), "S / W"),
            (dict(), dict(n=-1), "n_iterations"),
            (dict(max_n_steps=0), dict(), "max_n_steps"),
            (dict(return_if_valid_after_n_steps=-2), dict(), "return_if_valid_after_n_steps"),
            (dict(on_pose_valid=3), dict(), "on_pose_valid"),
            (dict(per_trajectory=2), dict(), "per_trajectory"),
            (dict(trace_capacity=-1), dict(), "trace_capacity"),
            (dict(convergence_threshold=-1.0), dict(), "convergence_threshold"),
            (dict(pose_lm_lambda=0.0), dict(), "lm_lambda"),
            (dict(pose_alpha_position=0.0), dict(), "alpha_position"),
            (dict(diff_lm_lambda=0.0), dict(), "lm_lambda"),
            (dict(), dict(W=8), "n_virtual_configs"),  # 2 * 4 virtual configs need more than 8 waypoints
            # (without a pose block the step never reads the factor; refused before the pose step's launch all the same)
            (dict(diff_pose_do_scale_down_satisfied=1, diff_pose_scale_down=2.0), dict(), "scale-down"),
        ]
        for pkw, akw, word in cases:
            a = dict(x=buf, target=buf, S=1, W=16, workspace=buf, control=buf, n=1)
            a.update(akw)
            P = _params(**pkw)
            rc = lib.cppf_lm_optimize_enqueue(h, a["x"], a["target"], a["S"], a["W"], ctypes.byref(P), a["workspace"], a["control"], a["n"], None)
            assert rc == _hip.CPPF_ERR_INVALID, (pkw, akw, rc)
            assert word in lib.cppf_last_error().decode(), (pkw, akw, lib.cppf_last_error().decode())
        # what has no gated kernel is refused as unsupported, not run some other way
        for pkw, akw in ((dict(diff_use_pose=1), dict()), (dict(diff_differencing_mode=1), dict()), (dict(), dict(S=64, W=512))):
            a = dict(S=1, W=16)
            a.update(akw)
            P = _params(**pkw)
            rc = lib.cppf_lm_optimize_enqueue(h, buf, buf, a["S"], a["W"], ctypes.byref(P), buf, buf, 1, None)
            assert rc == _hip.CPPF_ERR_UNSUPPORTED, (pkw, akw, rc, lib.cppf_last_error().decode())
        # ... and so is a coupled step that would resolve to an elimination without a gate (neither the parallel-in-time nor the
        # row-per-lane form): the choice depends on S, W, ndof and the handle's tuning only, so it is refused up front as well --
        # on this host-only handle, i.e. before the device is selected, let alone the pose step launched
        keys = _hip.TUNE_KEYS
        try:
            assert lib.cppf_debug_set(h, keys["full_rows"], 0) == _hip.CPPF_OK
            for tune, a in (({"pcr_max_rows": 0}, dict(S=1, W=16)), ({"pcr_max_rows": 0}, dict(S=3, W=200)), ({}, dict(S=1, W=600)),
                            ({"pcr_max_rows": 100}, dict(S=2, W=64))):  # fmt: skip
                for k, v in tune.items():
                    assert lib.cppf_debug_set(h, keys[k], v) == _hip.CPPF_OK
                P = _params()
                rc = lib.cppf_lm_optimize_enqueue(h, buf, buf, a["S"], a["W"], ctypes.byref(P), buf, buf, 1, None)
                assert rc == _hip.CPPF_ERR_UNSUPPORTED, (tune, a, rc, lib.cppf_last_error().decode())
                assert "elimination" in lib.cppf_last_error().decode()
                assert lib.cppf_debug_set(h, keys["pcr_max_rows"], _hip.TUNE_DEFAULT) == _hip.CPPF_OK
        finally:
            for k in ("full_rows", "pcr_max_rows"):
                assert lib.cppf_debug_set(h, keys[k], _hip.TUNE_DEFAULT) == _hip.CPPF_OK
        # zero iterations: nothing to do, nothing touched
        P = _params()
        assert lib.cppf_lm_optimize_enqueue(h, buf, buf, 1, 16, ctypes.byref(P), buf, buf, 0, None) == _hip.CPPF_OK
        # sizes: control = C records of 16 words + C * trace_capacity rows of 4 words; the workspace leads with the S*W*d snapshot
        n = ctypes.c_size_t(0)
        assert lib.cppf_lm_optimize_control_bytes(8, ctypes.byref(_params()), ctypes.byref(n)) == _hip.CPPF_OK
        assert n.value == 4 * (16 + 20 * 4)
        assert lib.cppf_lm_optimize_control_bytes(8, ctypes.byref(_params(per_trajectory=1)), ctypes.byref(n)) == _hip.CPPF_OK
        assert n.value == 8 * 4 * (16 + 20 * 4)
        assert lib.cppf_lm_optimize_workspace_bytes(h, 2, 100, ctypes.byref(n)) == _hip.CPPF_OK
        d, rows = 7, 200
        floats = 2 * rows * d + rows * (d * (d + 1) // 2 + d) + rows * d * d + rows * d + 2 * 16 + 2 * (((rows + 3) // 4 + 3) // 4 * 4)
        assert n.value == 4 * floats and n.value % 16 == 0
        assert lib.cppf_lm_optimize_workspace_bytes(h, 0, 100, ctypes.byref(n)) == _hip.CPPF_ERR_INVALID
    finally:
        lib.cppf_robot_destroy(h)


def test_new_header_is_part_of_the_build_id_and_the_planner_switch_defaults_off():
    import inspect

    from cppflow_amd import build
    from cppflow_amd.optimization import run_lm_alternating_loss, run_lm_optimization
    from cppflow_amd.planners import Planner

    assert "kernels_optloop.h" in build.HEADERS
    for fn in (run_lm_optimization, run_lm_alternating_loss):
        sig = inspect.signature(fn).parameters
        assert sig["device_loop"].default is False and sig["sync_every"].default is None and sig["per_trajectory"].default is False
    assert inspect.signature(Planner.__init__).parameters["device_optimizer"].default is False
