"""cppf_scene_env_collisions / cppf_scene_workspace_bytes (obstacle scenes, csrc/kernels_scene.h) at the C ABI: the prototypes and
every refusal -- all of which are decided before a device is selected, so a host-only handle serves.  No GPU.  (The destroyed
handle: tests/test_gpu_scene.py, through a handle a live batch keeps allocated.)"""

import ctypes

import pytest

from tests.test_abi import declared_functions


@pytest.fixture(scope="module")
def lib():
    from cppflow_amd import _hip, build

    build.build()
    return _hip.lib()


def test_entry_points_are_declared_bound_and_exported(lib):
    import re

    from cppflow_amd import _hip
    from cppflow_amd import scene
    from tests.test_abi import HEADER

    for fn in ("cppf_scene_env_collisions", "cppf_scene_workspace_bytes"):
        assert fn in declared_functions() and fn in _hip.SIGNATURES and getattr(lib, fn) is not None
    vp, ci, cf, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
    res, args = _hip.SIGNATURES["cppf_scene_env_collisions"]
    assert res is ci and args == [vp, vp, ci, ci, vp, vp, ci, cf, vp, vp, vp, vp, vp, sz, vp]
    res, args = _hip.SIGNATURES["cppf_scene_workspace_bytes"]
    assert res is ci and args == [ci, ci, ctypes.POINTER(sz)]
    text = open(HEADER).read()
    assert int(re.search(r"#define CPPF_MAX_SCENE_OBSTACLES (\d+)", text).group(1)) == 4096 == _hip.MAX_SCENE_OBSTACLES
    assert scene.MAX_SCENE_OBSTACLES == 4096
    assert int(re.search(r"#define CPPF_MAX_OBSTACLES (\d+)", text).group(1)) == 8  # the handle's own limit is untouched
    assert lib.cppf_abi_version() == 6  # additive: the ABI version stays


def _nbytes(lib, n, O):
    from cppflow_amd import _hip

    out = ctypes.c_size_t(0)
    assert lib.cppf_scene_workspace_bytes(n, O, ctypes.byref(out)) == _hip.CPPF_OK, lib.cppf_last_error().decode()
    return out.value


def _call(lib, h, **kw):
    buf = ctypes.c_void_p(0x1000)  # never dereferenced: every call here is refused before any launch
    a = dict(q=buf, S=3, W=5, box_lo=buf, box_hi=buf, n_obs=9, reach=0.05, env_mask=buf, min_env=buf, nearest_obs=buf, obs_min=buf,
             workspace=buf, workspace_bytes=None)  # fmt: skip
    a.update(kw)
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = 1 << 30
    return lib.cppf_scene_env_collisions(h, a["q"], a["S"], a["W"], a["box_lo"], a["box_hi"], a["n_obs"], a["reach"], a["env_mask"],
                                         a["min_env"], a["nearest_obs"], a["obs_min"], a["workspace"], a["workspace_bytes"], None)  # fmt: skip


def test_bad_arguments_are_refused_before_the_device_is_selected(lib):
    from cppflow_amd import _hip
    from cppflow_amd.robot_model import canonicalize
    from cppflow_amd.robot_zoo import ROBOT_SPECS

    assert _call(lib, None) == _hip.CPPF_ERR_INVALID and "NULL" in lib.cppf_last_error().decode()
    desc = _hip.chain_to_desc(canonicalize(ROBOT_SPECS["panda"]()))
    h = ctypes.c_void_p()
    assert lib.cppf_robot_create(ctypes.byref(desc), -12345, ctypes.byref(h)) == _hip.CPPF_OK, lib.cppf_last_error().decode()
    try:
        need = _nbytes(lib, 15, 9)
        cases = [(dict(**{name: None}), "NULL") for name in ("q", "env_mask", "box_lo", "box_hi", "workspace")]
        cases += [
            (dict(n_obs=-1), "n_obs"),
            (dict(n_obs=4097), "n_obs"),
            (dict(S=-1), "S / W"),
            (dict(W=-2), "S / W"),
            (dict(S=1 << 16, W=1 << 16), "2^31"),
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
    finally:
        lib.cppf_robot_destroy(h)


def test_workspace_bytes(lib):
    from cppflow_amd import _hip

    for O in (0, 1, 8, 9, 4096):
        prev = 0
        for n in (0, 1, 63, 64, 65, 300, 44800):
            b = _nbytes(lib, n, O)
            assert b >= prev and b % 16 == 0 and b >= 8 * n + 4 * O and b > 0  # a 64-bit key per row, a 32-bit key per cuboid
            prev = b
    out = ctypes.c_size_t(0)
    for n, O in ((-1, 4), (4, -1), (4, 4097)):
        assert lib.cppf_scene_workspace_bytes(n, O, ctypes.byref(out)) == _hip.CPPF_ERR_INVALID, (n, O)
        assert lib.cppf_last_error().decode()
    assert lib.cppf_scene_workspace_bytes(4, 4, None) == _hip.CPPF_ERR_INVALID
