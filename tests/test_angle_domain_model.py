"""CPU side of the angle-domain sweep (tests/angle_domain.py; the GPU side is tests/test_gpu_angle_domain.py).

  * The probe chain reads sincos_cw back exactly: the fp32 oracle's FK position on it IS the numpy restatement's (cos, sin), bit for bit,
    on every row whose restatement is not ambiguous (<= 0.1 % of each class).
  * The measured maxima of sincos_cw (fp32 oracle) and sincos_pi<FOLD> (numpy) against fp64, each on the domain it is specified on, and
    the bars of tests/angle_domain.py as 1.25 x those maxima (pytest -s prints them; profiles/angle_domain.txt holds them).
  * Mutants: the bars fail a dropped Cody-Waite piece, a coefficient of sincos_cw off by 1e-6 relative, a coefficient of sincos_pi off
    by 1e-7 absolute, a missing fold and `x >= 2 pi` made `>` in wrap_pi.  Two neighbouring changes are NOT faults and are pinned as
    such: `r <= -2 pi` made `<` is the same function (r == -2 pi then takes the `r < 0` step to the same 0), and FOLD = +1 comparing
    `>=` changes one input, x == pi32, whose reduced argument -pi32 is as valid as +pi32 (the sine changes sign at a magnitude below
    the bar).
  * Every edge class of the fold-boundary chains (part b of the GPU module) is at least half calm, from the fp64 oracle alone.
  * wrap_pi restated == the fp32 remainder form on every class, inside [-pi32, pi32].
"""

import numpy as np
import pytest

from tests import angle_domain as A


@pytest.fixture(scope="module")
def measured():
    """the maxima over the finite rows of every class and the dense CPU-only supplement"""
    q = np.concatenate(list(A.finite_rows().values()) + [A.dense_rows()])
    pose = A.probe_oracle(True).fk(A.probe_rows(q))
    err, ortho = A.errors(q, pose[:, 1], pose[:, 0])
    out = dict(q=q, cw={r: (err[np.abs(q) <= r].max(), ortho[np.abs(q) <= r].max()) for r in A.RANGES}, pi={}, pi2={})
    for fold in (0, 1, -1):
        lo, hi = A.fold_domain(fold)
        m = (q >= lo) & (q <= hi)
        s, c, _ = A.sincos_pi32(q[m], fold)
        out["pi"][fold] = A.errors(q[m], s, c)[0].max()
    s, c, _ = A.sincos_pi32(q, 2)
    e2 = A.errors(q, s, c)[0]
    out["pi2"] = {r: e2[np.abs(q) <= r].max() for r in A.RANGES}
    return out


def test_classes():
    rows = A.rows()
    assert set(rows) == {"half_pi", "tiny", "limits", "uniform", "log", "nonfinite"}
    for k, v in list(rows.items()) + list(A.wrap_rows().items()):
        assert v.dtype == np.float32 and A.MIN_CLASS <= len(v) <= A.MAX_ROWS, (k, len(v))
    assert np.isfinite(np.concatenate([v for k, v in rows.items() if k != "nonfinite"])).all()
    nf = rows["nonfinite"]
    assert (~np.isfinite(nf)).sum() == len(A.NONFINITE_AT) and np.isnan(nf).sum() == 2 and np.isfinite(nf).sum() >= A.MIN_CLASS
    assert A.PI32 in rows["limits"] and -A.PI32 in rows["limits"]  # Fetch's continuous joints: the edge of FOLD = 0
    assert np.signbit(rows["tiny"][1]) and rows["tiny"][1] == 0 and np.abs(rows["tiny"][2:8]).max() < 1e-44
    assert np.abs(rows["half_pi"]).max() > 2.0**19
    w = A.wrap_rows()
    x = np.concatenate(list(w.values())) + A.PI32
    for edge in (A.TWO_PI32, -A.TWO_PI32, 2 * A.TWO_PI32, -2 * A.TWO_PI32):  # x == 2 pi, r == -2 pi, the far switch: hit and straddled
        assert (x < edge).any() and (x > edge).any(), edge
        # (no fp32 dq has dq + pi32 == -2 pi32: the one candidate, the fp32 value of -3 pi, lands on a tie that rounds to the even
        # neighbour, and 2 pi32's last bit is odd.  That select boundary is reachable only from its two sides.)
        assert (x == edge).any() == (edge != -A.TWO_PI32), edge


@pytest.mark.parametrize("cls", ["half_pi", "tiny", "limits", "uniform", "log", "nonfinite"])
def test_probe_chain_reads_sincos_cw_back(cls):
    """position = (cos q, sin q, 0) exactly as sincos_cw returns them: the fp32 oracle on the probe chain against the restatement"""
    q = A.finite_rows()[cls]
    pose = A.probe_oracle(True).fk(A.probe_rows(q))
    s, c, amb = A.sincos_cw32(q)
    assert amb.sum() <= 1e-3 * len(q), (cls, int(amb.sum()))
    ok = ~amb
    assert ok.sum() >= A.MIN_CLASS
    assert A.same_bits32(pose[:, 0], c, zero_sign_free=True)[ok].all() and A.same_bits32(pose[:, 1], s, zero_sign_free=True)[ok].all()
    assert (pose[:, 2] == 0).all()
    A.check_cw(q, pose[:, 1], pose[:, 0], cls)


def test_probe_chain_nonfinite_and_signed_zero():
    q = A.rows()["nonfinite"]
    pose = A.probe_oracle(True).fk(A.probe_rows(q))
    bad = ~np.isfinite(q)
    assert np.isnan(pose[bad, :2]).all() and np.isfinite(pose[~bad]).all()
    s, c, _ = A.sincos_cw32(np.array([-0.0, 0.0], dtype=np.float32))
    assert not np.signbit(s).any() and (s == 0).all() and (c == 1).all()  # sincos_cw(-0.0) gives s = +0


def test_bars_are_the_recipe(measured):
    """every bar IS 1.25 x the measured maximum of the oracle / restatement, rounded up to two digits"""
    print()
    for r in A.RANGES:
        e, o = measured["cw"][r]
        print(f"sincos_cw     |q| <= 2^{int(np.log2(r))}: max abs error {e:.3e} (bar {A.CW_BAR[r]:.1e}), |s^2 + c^2 - 1| {o:.3f} u (bar {A.CW_ORTHO_BAR_U[r]})")
        assert A.bar_of(e) == A.CW_BAR[r] and A.bar_of(o) == A.CW_ORTHO_BAR_U[r], (r, e, o)
    for fold in (0, 1, -1):
        e = measured["pi"][fold]
        print(f"sincos_pi<{fold:+d}> on its interval: max abs error {e:.3e} (bar {A.PI_BAR[fold]:.1e})")
        assert A.bar_of(e) == A.PI_BAR[fold], (fold, e)
    for r in A.RANGES:
        e = measured["pi2"][r]
        print(f"sincos_pi<2>  |q| <= 2^{int(np.log2(r))}: max abs error {e:.3e} (bar {A.PI2_BAR[r]:.1e})")
        assert A.bar_of(e) == A.PI2_BAR[r], (r, e)


def test_beyond_the_documented_domain():
    """just inside 2^22 pi/2 the quadrant still holds (1e-6); beyond it the result is no rotation: what the header says, no more"""
    q = np.array([0.99 * A.CW_DOMAIN, 1e7, 1e10], dtype=np.float32)
    s, c, _ = A.sincos_cw32(q)
    err, _ = A.errors(q, s, c)
    print("\nsincos_cw at 0.99 * 2^22 pi/2, 1e7, 1e10: error", err)
    assert err[0] < 2e-6 and err[1] > 1.0 and err[2] > 1e3


def _cw_fails(q, **mutant):
    s, c, _ = A.sincos_cw32(q, **mutant)
    with pytest.raises(AssertionError):
        A.check_cw(q, s, c, str(mutant))


def test_bars_pass_the_restatements_and_fail_their_mutants(measured):
    q = measured["q"]
    s, c, _ = A.sincos_cw32(q)
    A.check_cw(q, s, c, "restated")
    _cw_fails(q, pieces=A.CW_PIECES[:2])  # the third Cody-Waite piece dropped
    # one coefficient off by 1e-6 relative: the sine's -1/6, either way (1.4e-7 / 1.6e-7).  The same relative change of a higher
    # coefficient moves no result by an ulp (the cosine's 1/24: 1.07e-7, inside the bar); those only the bit-for-bit comparison with
    # the fp32 oracle on the device sees.
    for sg in (1, -1):
        _cw_fails(q, sin_c=A.CW_SIN[:2] + (A.CW_SIN[2] * (1 + sg * 1e-6),))
    for fold in (0, 1, -1, 2):
        s, c, _ = A.sincos_pi32(q, fold)
        A.check_pi(q, s, c, fold, "restated")
        for coeffs in ("sin_c", "cos_c"):  # the leading coefficient of either polynomial off by 1e-7 absolute
            base = dict(sin_c=A.PI_SIN, cos_c=A.PI_COS)[coeffs]
            s, c, _ = A.sincos_pi32(q, fold, **{coeffs: base[:-1] + (base[-1] + 1e-7,)})
            with pytest.raises(AssertionError):
                A.check_pi(q, s, c, fold, coeffs)
    for fold in (1, -1):  # the conditional turn missing: FOLD = 0's code on FOLD = +-1's interval
        s, c, _ = A.sincos_pi32(q, 0)
        with pytest.raises(AssertionError):
            A.check_pi(q, s, c, fold, "no fold")


def test_fold_comparing_ge_is_not_a_fault(measured):
    """FOLD = +1 with `x >= pi` for `x > pi` (and -1 likewise) changes exactly the inputs x == +-pi32: the reduced argument becomes
    -+pi32, as valid an argument of the polynomials; the sine changes sign at a magnitude below the bar and every bar still holds."""
    q = measured["q"]
    for fold, at in ((1, A.PI32), (-1, -A.PI32)):
        s, c, _ = A.sincos_pi32(q, fold)
        sm, cm, _ = A.sincos_pi32(q, fold, fold_ge=True)
        diff = ~(A.same_bits32(s, sm) & A.same_bits32(c, cm))
        assert diff.any() and (q[diff] == at).all() and A.same_bits32(cm, c).all() and (sm[diff] == -s[diff]).all()
        assert np.abs(s[diff]).max() < 0.5 * A.PI_BAR[fold]
        A.check_pi(q, sm, cm, fold, "fold_ge")


def test_wrap_restated_equals_the_remainder_form():
    print()
    for k, b in list(A.wrap_rows().items()) + list(A.rows().items()):
        got, want = A.wrap_pi32(b), A.wrap_remainder32(b)
        assert A.same_bits32(got, want).all(), k
        fin = np.isfinite(b)
        assert np.isnan(got[~fin]).all() and (np.abs(got[fin]) <= A.PI32).all(), k
        on = (int((got == A.PI32).sum()), int((got == -A.PI32).sum()))
        print(f"wrap class {k}: {len(b)} rows, {on[0]} land exactly on +pi32, {on[1]} on -pi32")
        if k.startswith("k_pi"):
            assert on[0] + on[1] >= 1, k
        # accuracy (a statement, not a bar of the device): against the fp64 wrap of the same input, modulo the seam, one rounding of
        # dq + pi, one of the 2 pi step and the fp32 values of pi and 2 pi: 4 ulp of max(|dq|, 2 pi) for |dq| < 30
        small = fin & (np.abs(b) < 30)
        d = np.abs(got[small].astype(np.float64) - A.wrap64(b[small]))
        d = np.minimum(d, np.abs(2 * np.pi - d))
        assert (d <= 4 * A.U * np.maximum(np.abs(b[small]), 2 * np.pi)).all(), (k, d.max())
    # dq = -pi - tiny rounds to +pi: the one way to the closed upper end
    below = np.nextafter(-A.PI32, np.float32(-np.inf))
    assert A.wrap_pi32(below) == A.wrap_remainder32(below)


def test_wrap_mutants():
    b = np.concatenate(list(A.wrap_rows().values()))
    want = A.wrap_remainder32(b)
    assert not A.same_bits32(A.wrap_pi32(b, ge_2pi=False), want).all()  # x == 2 pi stays 2 pi and leaves as +pi for -pi
    # `r <= -2 pi` made `<` is the SAME function: r == -2 pi is negative, so the `r < 0` step adds the same 2 pi; asserted as found
    assert A.same_bits32(A.wrap_pi32(b, le_m2pi=False), want).all()


@pytest.mark.parametrize("name", list(A.FOLD_CHAINS))
def test_edge_classes_of_the_fold_chains_are_calm(name):
    """the condition of the K-step comparison on the device: per class >= 64 rows, at least half of them calm at every K -- computed from
    the fp64 oracle alone; rows that start whole turns outside the limits count their first step without the turns"""
    p, ch = A.edge_problem(name), A.fold_chain(name)
    lo, hi = np.asarray(ch.lo, dtype=np.float32), np.asarray(ch.hi, dtype=np.float32)
    assert ((p["unturned"] >= lo) & (p["unturned"] <= hi)).all()
    turned = p["cls"] == "turns"
    assert (np.abs(p["x0"] - p["unturned"]).max(axis=1)[turned] > 6.0).all() and np.array_equal(p["x0"][~turned], p["unturned"][~turned])
    assert ((p["x0"] > hi) | (p["x0"] < lo)).any(axis=1)[turned].all()
    on = (p["x0"] == hi) | (p["x0"] == lo)
    assert on.any(axis=1)[p["cls"] == "limit"].all()
    if name != "fold0":  # [-3, 3] holds no +-pi32
        assert (np.abs(np.abs(p["x0"]) - A.PI32) < 1e-6).any(axis=1)[p["cls"] == "pi"].all()
    for K in A.LEAN_KS:
        calm = A.edge_trace(name, K)[4]
        for c in A.EDGE_CLASSES:
            m = p["cls"] == c
            assert (not m.any() and (name, c) == ("fold0", "pi")) or (m.sum() >= A.MIN_CLASS and calm[m].mean() >= 0.5), (name, K, c)
