"""The capsule distance functions on degenerate geometry, on the device, through entry points that already exist: no test kernels.
Sweep, classes, reference and bars: tests/capsule_domain.py (its docstring holds the derivations and the measured figures); the CPU side
is tests/test_capsule_domain_model.py.

16 384 rows per shape; the generic kernels for all eight shapes, the run-time-specialised (hipRTC) ones for two, one of them with a
sphere second.  Every distance the library reports must equal the fp32 oracle BIT FOR BIT on the whole sweep -- the first parity check in
which rcp_rn's "0 below 2^-100" rule, the v_med3 clamps, fminf / fmaxf on +-inf and subnormal products are in play on the chip -- and
must meet the bars against the fp64 golden-section reference directly, so that nothing here rests on the oracle alone.
"""

import numpy as np
import pytest
import torch

from tests import capsule_domain as C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = [(s, False) for s in C.SHAPES] + [(s, True) for s in C.RTC_SHAPES]
ENV_CASES = [c for c in CASES if c[0][0] == "seg"]  # (the base capsule does not move: one base is enough against the boxes)
VARIANT = (("seg", "h15"), False)


def _id(case):
    (base, moving), rtc = case
    return f"{base}-{moving}-{'rtc' if rtc else 'generic'}"


def dev(a, dtype=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def same_bits(got, want):
    """got (device fp32 tensor) == want (the fp32 oracle's values as float64), bit for bit"""
    got, want32 = np.ascontiguousarray(host(got)), np.ascontiguousarray(np.asarray(want).astype(np.float32))
    assert got.dtype == np.float32 and np.array_equal(want32.astype(np.float64), np.asarray(want, dtype=np.float64))
    return got.shape == want32.shape and np.array_equal(got.view(np.int32), want32.view(np.int32))


_ROBOTS = {}


def robot(case, radii=(0.0, 0.0)):
    from cppflow_amd.robots import Robot

    key = (case, radii)
    if key not in _ROBOTS:
        (base, moving), rtc = case
        rb = Robot(C.free_capsule_spec(base, moving, radii), specialize=rtc)
        assert rb.specialization(DEV) == (1000 if rtc else -1), (case, rb.specialization(DEV))  # (a failed hipRTC build only warns)
        _ROBOTS[key] = rb
    return _ROBOTS[key]


@pytest.fixture(scope="module")
def q():
    return dev(C.rows()[0])


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_self_distances_equal_the_oracle_and_meet_the_bars(q, case):
    (base, moving), _ = case
    rb, ref = robot(case), C.reference_ss(base, moving)
    want = C.oracle(base, moving).self_dists(C.rows()[0])
    got = rb.self_collision_distances(q)
    m = C.measure(host(got)[:, 0].astype(np.float64), ref)
    print(_id(case), {k: round(v, 3) for k, v in m.items()})
    assert same_bits(got, want), (case, int((host(got).astype(np.float64) != want).sum()), "rows differ from the fp32 oracle")
    C.check(host(got)[:, 0], ref, case)
    J, dist = rb.self_collision_distances_jacobian(q, return_distances=True)
    assert same_bits(dist, want) and torch.isfinite(J).all(), case


@pytest.mark.parametrize("case", ENV_CASES, ids=_id)
def test_env_distances_equal_the_oracle_and_meet_the_bars(q, case):
    (base, moving), _ = case
    rb = robot(case)
    for box in C.BOXES:
        cub, T = C.box_obstacle(box)
        want = C.oracle(base, moving).env_dists(C.rows()[0], *C.box_corners(box))
        got = rb.env_collision_distances(q, cub, T)
        assert same_bits(got, want), (case, box, int((host(got).astype(np.float64) != want).any(axis=1).sum()), "rows differ")
        C.check(host(got)[:, 1], C.reference_box(moving, box), (case, box))
        J, dist = rb.env_collision_distances_jacobian(q, cub, T, return_distances=True)
        assert same_bits(dist, want) and torch.isfinite(J).all(), (case, box)


def _masks_case(q, case, radii):
    """against every box but the slab (which holds the base capsule: the minimum over the capsules would be 0 in every row)"""
    (base, moving), _ = case
    rb = robot(case, radii)
    lo, hi = C.mask_boxes()
    obs = [(np.array([*l, *h], dtype=np.float32), C.box_obstacle("cube")[1]) for l, h in zip(lo, hi)]
    rb.set_obstacles([c for c, _ in obs], [T for _, T in obs])
    want = C.oracle(base, moving, True, radii).masks(C.rows()[0], lo, hi)
    full = rb.collision_masks(q.reshape(1, C.N_ROWS, 6), want_min_dists=True)
    for k in ("min_self", "min_env", "ext_cost"):
        assert same_bits(full[k].reshape(-1), want[k]), (case, radii, k)
    lean = rb.collision_masks(q.reshape(1, C.N_ROWS, 6))  # the mask-only launch: squared distances against squared thresholds
    for k in ("self_mask", "env_mask", "jlim_mask"):
        assert np.array_equal(host(full[k]).reshape(-1), want[k].astype(bool)), (case, radii, k)
        assert torch.equal(lean[k], full[k]), (case, radii, k, "mask-only launch")
    for k, v in (("self_mask", "min_self"), ("env_mask", "min_env")):  # ... equal to the sign of the minima
        assert torch.equal(lean[k], full[v] < 0), (case, radii, k)
    assert torch.equal(lean["ext_cost"], full["ext_cost"])
    base_min = C.oracle(base, moving, True, radii).env_dists(C.rows()[0][:1], lo[0], hi[0])[0, 0]  # (the cube is the base capsule's nearest)
    assert (want["min_env"] < base_min).sum() >= 512, (case, "rows in which the moving capsule decides the minimum")
    return want


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_masks_and_minima_equal_the_oracle(q, case):
    _masks_case(q, case, (0.0, 0.0))


def test_masks_of_the_variant_with_radii(q):
    """radii 0.03 / 0.05: both signs occur (tests/test_capsule_domain_model.py), so the mask-only threshold path has hits to decide"""
    want = _masks_case(q, VARIANT, C.RADII)
    assert want["self_mask"].sum() >= C.MIN_CLASS and want["env_mask"].sum() >= C.MIN_CLASS


@pytest.mark.parametrize("case", ENV_CASES, ids=_id)
def test_scene_minimum_equals_the_oracle(q, case):
    """scene_env_collisions with the cube in slot 37 of a 65-cuboid scene (two tiles of the scene launch): min_env and the mask"""
    (base, moving), _ = case
    lo, hi = C.scene_corners()
    want = C.oracle(base, moving).masks(C.rows()[0], lo, hi)
    got = robot(case).scene_env_collisions(q, dev(lo), dev(hi), want=("env_mask", "min_env", "nearest_obs"))
    assert same_bits(got["min_env"], want["min_env"]), case
    assert np.array_equal(host(got["env_mask"]), want["env_mask"].astype(bool))
    assert (host(got["nearest_obs"]) == C.SCENE_SLOT).all()  # (the clutter is farther than the cube from every row)
    base_min = C.oracle(base, moving).env_dists(C.rows()[0][:1], lo[C.SCENE_SLOT], hi[C.SCENE_SLOT])[0, 0]
    assert (want["min_env"] < base_min).sum() >= 512, (case, "rows in which the moving capsule decides the minimum")


@pytest.mark.parametrize("rtc", [False, True], ids=["generic", "rtc"])
def test_gradient_of_a_segment_sphere_pair(q, rtc):
    """sphere second: the device's d(distance)/dq against the fp64 oracle's analytic gradient (equal to central differences:
    tests/test_capsule_domain_model.py) on the rows away from contact.  The gradient is the unit normal (c1 - c2) / d times a lever of
    at most 2 ext; c1 - c2 carries about 4 u ext of fp32 rounding per component, so the bar is 16 u ext (1 + ext) / d per row:
    1.6e-4 at d = 0.05, ext = 1.6 (a gradient through the first segment's centre instead of the closest point is off by tenths)."""
    case = (("seg", "sph"), rtc)
    x = C.rows()[0]
    d64, g64 = C.oracle("seg", "sph", False).self_dists_grads(x)
    J = host(robot(case).self_collision_distances_jacobian(q)).astype(np.float64)
    ok = d64[:, 0] > 0.05
    bar = 16 * C.U * C.reference_ss("seg", "sph")["ext"] * (1 + C.reference_ss("seg", "sph")["ext"]) / np.maximum(d64[:, 0], 0.05)
    err = np.abs(J[:, 0] - g64[:, 0]).max(axis=1)
    print("rows", int(ok.sum()), "max gradient error", err[ok].max(), "max share of the bar", (err / bar)[ok].max())
    assert ok.sum() > 15000 and np.abs(g64[ok]).max() > 0.9 and (err[ok] <= bar[ok]).all(), (err / bar)[ok].max()
