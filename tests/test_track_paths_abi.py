"""cppf_track_paths (one-launch tracking IK, csrc/kernels_track.h) at the C ABI and TrackingSeedProvider's argument checks: no GPU.

A NULL robot or target is refused with CPPF_ERR_INVALID and a message before anything is launched; the provider validates its
arguments when it is constructed."""

import ctypes

import pytest

from tests.test_abi import HEADER, declared_functions


@pytest.fixture(scope="module")
def lib():
    from cppflow_amd import _hip, build

    build.build()
    return _hip.lib()


def _params(**kw):
    from cppflow_amd import _hip

    p = dict(lm_lambda=1e-2, alpha_position=3.5, alpha_rotation=0.35, n_restart=40, n_track=6, n_random_restarts=0, tol_pos_m=0.0,
             tol_rot_rad=0.0, max_jump_rad=0.0, max_jump_m=0.0, seed=0, call_index=0)  # fmt: skip
    p.update(kw)
    return _hip.TrackParams(**p)


def test_track_paths_is_declared_and_exported(lib):
    from cppflow_amd import _hip

    assert "cppf_track_paths" in declared_functions()
    assert "cppf_track_paths" in _hip.SIGNATURES
    assert lib.cppf_track_paths is not None
    text = open(HEADER).read()
    for name, bit in (("CPPF_TRACK_CONVERGED", _hip.TRACK_CONVERGED), ("CPPF_TRACK_RESTARTED", _hip.TRACK_RESTARTED),
                      ("CPPF_TRACK_JUMP", _hip.TRACK_JUMP), ("CPPF_TRACK_RECOVERED", _hip.TRACK_RECOVERED)):  # fmt: skip
        assert f"#define {name} {bit} " in text
    # 3 floats, 3 int32, 4 floats, 2 uint32
    assert ctypes.sizeof(_hip.TrackParams) == 48


def test_null_robot_is_refused_with_a_message(lib):
    from cppflow_amd import _hip

    prm = _params()
    rc = lib.cppf_track_paths(None, None, 16, 4, 1, ctypes.byref(prm), None, None, None, None, None, None)
    assert rc == _hip.CPPF_ERR_INVALID
    assert "NULL" in lib.cppf_last_error().decode()


def test_null_target_and_bad_arguments_are_refused_with_a_message(lib):
    """A host-only handle (no device is touched: cppf_robot_create's validation path) -- every argument check comes before a launch."""
    from cppflow_amd import _hip
    from cppflow_amd.robot_model import canonicalize
    from cppflow_amd.robot_zoo import ROBOT_SPECS

    desc = _hip.chain_to_desc(canonicalize(ROBOT_SPECS["panda"]()))
    h = ctypes.c_void_p()
    rc = lib.cppf_robot_create(ctypes.byref(desc), -12345, ctypes.byref(h))  # kNoDevice: the host-only mode
    assert rc == _hip.CPPF_OK, lib.cppf_last_error().decode()
    try:
        buf = ctypes.c_void_p(0x1000)  # never dereferenced: the call is refused before any launch
        cases = [
            (dict(), dict(target=None), "target"),
            (dict(), dict(S=0), "S"),
            (dict(), dict(S=17), "S"),
            (dict(n_restart=0), dict(), "n_restart"),
            (dict(n_track=0), dict(), "n_track"),
            (dict(n_random_restarts=-1), dict(), "n_random_restarts"),
            (dict(max_jump_rad=-1.0), dict(), "max_jump"),
            (dict(tol_pos_m=1e-4), dict(), "tolerances"),
            (dict(lm_lambda=0.0), dict(), "lm_lambda"),
            (dict(), dict(q_out=None), "q_out"),
        ]
        for pkw, akw, word in cases:
            a = dict(target=buf, T=16, k=4, S=1, q_out=buf)
            a.update(akw)
            prm = _params(**pkw)
            rc = lib.cppf_track_paths(h, a["target"], a["T"], a["k"], a["S"], ctypes.byref(prm), None, a["q_out"], buf, buf, buf, None)
            assert rc == _hip.CPPF_ERR_INVALID, (pkw, akw)
            assert word in lib.cppf_last_error().decode(), (pkw, akw, lib.cppf_last_error().decode())
    finally:
        lib.cppf_robot_destroy(h)
    # (a destroyed handle: tests/test_gpu_track_paths.py, through a handle a live batch keeps allocated)


def test_tracking_seed_provider_validates_without_a_gpu():
    from cppflow_amd.planners import LmIkSeedProvider, Planner, TrackingSeedProvider

    p = TrackingSeedProvider(seed=3, n_segments=4)
    assert p.n_calls == 0 and p.last is None and p.n_segments == 4
    assert TrackingSeedProvider().n_segments is None and TrackingSeedProvider().waypoints_per_segment == 35
    for bad in (dict(n_segments=0), dict(waypoints_per_segment=0), dict(damping=0.0), dict(n_restart_steps=0), dict(n_track_steps=0), dict(n_random_restarts=-1),
                dict(tol_pos_m=1e-4, tol_rot_rad=0.0), dict(tol_pos_m=-1.0, tol_rot_rad=-1.0), dict(max_jump_rad=-0.1),
                dict(init_width=-1.0)):  # fmt: skip
        with pytest.raises(AssertionError):
            TrackingSeedProvider(**bad)
    # the planner's default provider is unchanged
    import inspect

    assert "LmIkSeedProvider()" in inspect.getsource(Planner.__init__)
    assert callable(LmIkSeedProvider())


def test_tracking_kernel_header_is_part_of_the_build_id_and_of_hiprtc():
    from cppflow_amd import build

    assert "kernels_track.h" in build.HEADERS and "kernels_track.h" in build.EMBEDDED
    import os

    src = open(os.path.join(build.CSRC, "rtc_specialize.h")).read()
    assert "track_kernel<cppf::StaRobot<cppf::gen::Custom>>" in src and '#include \\"kernels_track.h\\"' in src
