"""CPU side of the capsule-distance sweep (tests/capsule_domain.py; its docstring holds the classes, the reference, the bars and the
measured figures): both oracle builds against the fp64 golden-section reference on every shape, every box and every row; the class
counts that keep the comparison from being vacuous; the constants against what the fp32 oracle needs; and a restatement of the
segment-segment formula whose old form (s = 0 whenever the Gram determinant vanishes) must fail where the second capsule is a sphere.

Measured on this sweep with the fp32 oracle (pytest -s prints them): first tier kappa 1157.6 (segment-segment outside near_parallel),
0.99 (segment-box), kappa_p 0 given KAPPA = 2320; second tier kt 0.99, largest underestimate 0.83, overshoot / (hmin sin) 1.99,
overshoot sin / (u ext) 0.78.  The fp64 oracle needs 0.56 of u (d_ref + ext) everywhere: what is left is the rounding of c +- h to the
fp32 end points the reference reads.
"""

import numpy as np
import pytest
import torch

from tests import capsule_domain as C
from tests import helpers as H


def _self(base, moving, is_f32):
    return C.oracle(base, moving, is_f32).self_dists(C.rows()[0])[:, 0]


def _env(moving, box, is_f32):
    lo, hi = C.box_corners(box)
    return C.oracle("seg", moving, is_f32).env_dists(C.rows()[0], lo, hi)


def test_no_class_of_the_sweep_is_empty():
    """every class of the module docstring holds >= 64 rows, in every shape it can occur in; no row is left out of any comparison"""
    q, fam = C.rows()
    assert q.shape == (C.N_ROWS, 6) and np.array_equal(H.f32(q), q) and {f for f, _ in C.FAMILIES} == set(fam)
    counts = {s: {k: int(v.sum()) for k, v in C.classes(*s).items()} for s in C.SHAPES}
    for (base, moving), n in counts.items():
        print(base, moving, n)
        if base == "seg" and moving != "sph":
            assert n["parallel"] >= C.MIN_CLASS and n["near_parallel"] - n["parallel"] >= C.MIN_CLASS, (base, moving, n)
            assert n["zero_ref"] >= C.MIN_CLASS, (base, moving, n)
        else:
            assert n["parallel"] == 0 and n["near_parallel"] == 0
        if moving != "sph":
            assert n["h_zero"] >= C.MIN_CLASS and n["h_sq_subnormal"] >= C.MIN_CLASS, (base, moving, n)
    assert counts["sph", "h15"]["sphere_first"] == counts["seg", "sph"]["sphere_second"] == counts["sph", "sph"]["both_spheres"] == C.N_ROWS
    assert sum(n["sphere_first"] > 0 for n in counts.values()) == 3 and sum(n["sphere_second"] > 0 for n in counts.values()) == 1
    for box in ("cube", "flat", "slab"):  # (a voxel and a point are hit exactly by a handful of rows only)
        for moving in C.MOVING:
            assert int((C.reference_box(moving, box)["d"] == 0).sum()) >= C.MIN_CLASS, (moving, box)
    # joint values next to 0 that are subnormal themselves, and lattice positions that graze exactly
    assert ((q[:, 3:] != 0) & (np.abs(q[:, 3:]) < np.finfo(np.float32).tiny)).sum() >= C.MIN_CLASS
    assert (q[:, :3] * 16 == np.round(q[:, :3] * 16)).all(axis=1).sum() >= C.MIN_CLASS


def test_segment_segment_meets_the_bars_in_both_builds():
    worst = {}
    for base, moving in C.SHAPES:
        ref = C.reference_ss(base, moving)
        for is_f32 in (True, False):
            d = _self(base, moving, is_f32)
            C.check(d, ref, (base, moving, is_f32))
            for k, v in C.measure(d, ref).items():
                worst[is_f32, k] = max(worst.get((is_f32, k), 0.0), v)
    print({f"{'fp32' if f else 'fp64'} {k}": round(v, 3) for (f, k), v in worst.items()})
    # the constants are twice what the fp32 oracle needs here, no less (and `lin` is derived: s spans at most the shorter segment)
    assert 2 * worst[True, "kappa"] <= C.KAPPA and 2 * worst[True, "kappa_p"] <= C.KAPPA_P
    assert 2 * worst[True, "kt"] <= C.KT and 2 * worst[True, "under"] <= C.KT and 2 * worst[True, "ks"] <= C.KS and worst[True, "lin"] <= 2.0
    # the exact arithmetic of the same formula has nothing to lose: the fp64 build is inside the plain bar on every row
    assert worst[False, "kappa"] <= 1.0 and worst[False, "lin"] == 0.0


def test_segment_box_meets_the_bars_in_both_builds():
    worst = {True: 0.0, False: 0.0}
    for moving in C.MOVING:
        for box in C.BOXES:
            ref = C.reference_box(moving, box)
            for is_f32 in (True, False):
                d = _env(moving, box, is_f32)
                C.check(d[:, 1], ref, (moving, box, is_f32))
                worst[is_f32] = max(worst[is_f32], C.measure(d[:, 1], ref)["kt"])
                assert (d[:, 0] == d[0, 0]).all()  # (the base capsule does not move)
    print("segment-box, max |d - d_ref| / (u (d_ref + ext)): fp32", round(worst[True], 3), " fp64", round(worst[False], 3))
    assert 2 * worst[True] <= C.KT and worst[False] <= 1.0


def _base_ends(base):
    return tuple(np.tile(H.f32(p), (C.N_ROWS, 1)) for p in C.BASES[base])


def test_the_old_formula_fails_where_the_second_capsule_is_a_sphere():
    """the bars have teeth: the restated formula passes every shape, and with s = 0 on a vanishing determinant (the formula as it was)
    it fails the sphere-second shape, in either tier, and no other; oracle/ref_torch.py is given the same rows"""
    from oracle import ref_torch

    for base, moving in C.SHAPES:
        ends, ref = C.geometry(moving)["ends"], C.reference_ss(base, moving)
        b0, b1 = _base_ends(base)
        C.check(C.seg_seg_restated(b0, b1, ends[:, :3], ends[:, 3:]), ref, (base, moving, "restated"))
        old = C.seg_seg_restated(b0, b1, ends[:, :3], ends[:, 3:], sphere_second_fix=False)
        if (base, moving) == ("seg", "sph"):
            for tier in (1, 2):
                with pytest.raises(AssertionError, match="overestimate"):
                    C.check(old, ref, tiers=(tier,))
            assert (old - ref["d"]).max() > 0.1  # up to the half-length of the first segment, 0.2 m
        else:
            C.check(old, ref, (base, moving, "old formula"))
        t = [torch.tensor(a, dtype=torch.float64) for a in (b0, b1, ends[:, :3], ends[:, 3:])]
        C.check(ref_torch._segment_segment_distance(*t).numpy(), ref, (base, moving, "ref_torch"))


def test_the_oracle_gradient_of_a_segment_sphere_pair_equals_central_differences():
    """sphere second: d(distance)/dq of the fp64 oracle (the closest points it differentiates through moved with the fix) against
    central differences of step eps.  Away from contact the distance is C^1 with a curvature of at most 1 / d that jumps where a clamp
    takes hold, so a central difference is within eps / d of the gradient: 2e-5 for d > 0.05 (a gradient through the wrong closest
    point is off by tenths)"""
    q = C.rows()[0][::16]
    orc = C.oracle("seg", "sph", False)
    d, g = orc.self_dists_grads(q)
    assert np.array_equal(d, orc.self_dists(q))
    eps = 1e-6
    fd = np.stack([(orc.self_dists(q + eps * e)[:, 0] - orc.self_dists(q - eps * e)[:, 0]) / (2 * eps) for e in np.eye(6)], axis=1)
    ok = d[:, 0] > 0.05
    assert ok.sum() > 900 and np.abs(g[ok, 0]).max() > 0.9
    assert np.abs(g[ok, 0] - fd[ok]).max() < eps / 0.05, np.abs(g[ok, 0] - fd[ok]).max()


def test_masks_of_the_variant_with_radii_have_hits_to_decide():
    """radii 0.03 (base) / 0.05 (moving): the masks of the fp32 oracle are the sign of its minima, and both signs occur among the rows"""
    q = C.rows()[0]
    lo, hi = C.mask_boxes()
    m = C.oracle("seg", "h15", True, C.RADII).masks(q, lo, hi)
    assert np.array_equal(m["self_mask"], m["min_self"] < 0) and np.array_equal(m["env_mask"], m["min_env"] < 0)
    for k in ("self_mask", "env_mask"):
        assert C.MIN_CLASS <= m[k].sum() <= C.N_ROWS - C.MIN_CLASS, (k, m[k].sum())
    print("self-colliding", m["self_mask"].mean(), "env-colliding", m["env_mask"].mean())
