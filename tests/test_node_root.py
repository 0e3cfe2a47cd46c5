"""The frozen-node root finder (node_visit, vic_profile.hpp) as a unit, against an arbitrary-precision root of the
reference's node residual (tests/node_cases.py) on a battery of edge cases: soils from expt 4 to 40 and bubble 2 to 80 cm,
roots just below 0 C, at the kink where the ice content reaches zero, deep cold and at the +-50.25 K edge of the
reference's search, starts from T0, far away, subnormal and at or above 0 C, and node 1's cold-nose residual.

Bounds, with r the exact root and tol(T) = 2 * 3e-8 |T| + 1e-7 (root_brent.c:274):
  * the oracle and the device's Brent mode: within 2 tol of a sign change; ERROR exactly when none lies in range;
  * the device's Newton mode: within NODE_NEWTON_TOL = 1e-8 K, and within 1e-9 K + 1e-12 |r| on the curved branch of the
    freezing curve (|r| >= 1e-4 K, 1e-6 K from a kink; the accept rule claims 1e-11 K there); failed exactly when no root
    lies in range (roots within 1e-6 K of the range's edge are not judged); where node 1's residual has its cold-nose
    variant below the smooth root, the result equals the Brent mode's bit for bit (the replay);
  * closed-form updates (oldT >= 0): a few roundings of the largest term of the numerator, and the oracle's bits.
"""
import math

import numpy as np
import pytest

from tests import node_cases as nc


@pytest.fixture(scope="module")
def battery():
    X, n1, ex, lb = nc.make_battery()
    return X, n1, ex, lb, nc.references(X, n1, ex)


def _report(name, worst):
    print("%s worst |T - r| per class: %s" % (name, ", ".join("%s %.3e" % kv for kv in sorted(worst.items()))))


# ------------------------------------------------------------------------------------------------ CPU
def test_battery_covers_every_class(battery):
    """The battery cannot thin out quietly: a minimum count per class, and the cold-nose sets it promises."""
    X, n1, ex, lb, refs = battery
    cnt = nc.count_classes(lb)
    for kind, values, least in (("expt", nc.EXPTS, 100), ("bubble", nc.BUBBLES, 150), ("ratio", nc.RATIOS, 100),
                                ("ice0", nc.ICE0S, 200), ("root", nc.ROOTS, 80), ("start", nc.STARTS, 80), ("nose", nc.NOSES, 40)):
        for v in values:
            assert cnt.get((kind, v), 0) >= least, (kind, v, cnt.get((kind, v), 0))
    for e in (False, True):
        assert (ex == e).sum() >= 400
        assert ((ex == e) & n1).sum() >= 100
    nose = [r for r, l in zip(refs, lb) if l["nose"] and "roots" in r]
    assert sum(len(r["roots"]) > 1 for r in nose) >= 5                       # several sign changes below Thi
    single_above = 0
    for r, l, c, e in zip(refs, lb, X, ex):
        if l["nose"] and "roots" in r and len(r["roots"]) == 1 and r["roots"][0] >= nc.nose_interval(c, e)[1]:
            single_above += 1
    assert single_above >= 20                                                # one sign change at or above Thi
    assert sum(1 for r in refs if "roots" in r and not r["roots"]) >= 40     # no root in range
    assert (X[:, nc.IOLDT] == -1e-310).sum() >= 50 and (X[:, nc.IOLDT] >= 0).sum() >= 100
    assert cnt.get(("start", "kink_side"), 0) >= 80                          # Newton steps from the curved side across the kink


def test_oracle_node_root_against_mpmath(oracle_lib, battery):
    """vicorc_node_root (the oracle's Brent iteration on the reference's residual) within 2 tol of the exact root, ERROR
    exactly outside the range: pins the arbitrary-precision reference and the generator before a GPU is involved."""
    X, n1, ex, lb, refs = battery
    T, F = nc.run_groups(lambda rows, a, b: oracle_lib.oracle_node_root(rows, int(a), b), X, n1, ex)
    bad, worst = nc.check(X, n1, ex, lb, refs, T, F, "brent")
    _report("oracle", worst)
    assert not bad, "\n".join(bad[:20])


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def model():
    return nc.hook_model()


@pytest.fixture(scope="module")
def hook(battery, model):
    m = model
    X, n1, ex, lb, refs = battery
    brent = nc.run_groups(nc.device_fn(m, newton=False), X, n1, ex)
    newton = nc.run_groups(nc.device_fn(m, newton=True), X, n1, ex)
    return m, brent, newton


@pytest.mark.gpu
def test_newton_node_root(battery, hook):
    X, n1, ex, lb, refs = battery
    _, brent, newton = hook
    bad, worst = nc.check(X, n1, ex, lb, refs, newton[0], newton[1], "newton", brent)
    _report("device newton", worst)
    assert not bad, "\n".join(bad[:20])


@pytest.mark.gpu
def test_brent_node_root_and_oracle(oracle_lib, battery, hook):
    X, n1, ex, lb, refs = battery
    _, brent, _ = hook
    bad, worst = nc.check(X, n1, ex, lb, refs, brent[0], brent[1], "brent")
    _report("device brent", worst)
    assert not bad, "\n".join(bad[:20])
    To, Fo = nc.run_groups(lambda rows, a, b: oracle_lib.oracle_node_root(rows, int(a), b), X, n1, ex)
    assert np.array_equal(brent[1], Fo), np.flatnonzero(brent[1] != Fo)[:20]
    closed = X[:, nc.IOLDT] >= 0
    assert np.array_equal(brent[0][closed], To[closed]) and np.array_equal(hook[2][0][closed], To[closed])


@pytest.mark.gpu
def test_node_root_lane_independence(battery, hook):
    """Natural order, a seeded permutation, and each case alone among padding lanes: the same bits per case."""
    X, n1, ex, lb, refs = battery
    m, brent, newton = hook
    perm = np.random.default_rng(7).permutation(len(X))
    inv = np.argsort(perm)
    for newton_mode, ref in ((False, brent), (True, newton)):
        fn = nc.device_fn(m, newton_mode)
        Tp, Fp = nc.run_groups(fn, X[perm], n1[perm], ex[perm])
        assert np.array_equal(Tp[inv], ref[0]) and np.array_equal(Fp[inv], ref[1])
        for i in range(len(X)):
            T1, F1 = fn(X[i:i + 1], n1[i], ex[i])
            assert T1[0] == ref[0][i] or (np.isnan(T1[0]) and np.isnan(ref[0][i])), (newton_mode, i)
            assert F1[0] == ref[1][i], (newton_mode, i)


def _ulp_err(got, want):
    """|got - want| in units of the last place of want (mpf)."""
    import mpmath
    w = float(want)
    return float(abs(mpmath.mpf(got) - want) / np.spacing(abs(w))) if w != 0 else abs(got) / np.spacing(0.0)


@pytest.mark.gpu
def test_math_ids_against_mpmath(model):
    """ln_pos, pow_pos, pow_pos_approx, rcp_refined (vic_math.hpp) against mpmath; the measured worst values are printed
    (the accuracy of v_rcp_f64 and v_log_f32 on gfx950 is not documented)."""
    import mpmath
    from vic_amd.abi import C
    m = model
    rng = np.random.default_rng(11)
    eps = 2.0 ** -52
    # ln_pos: <= 1 ulp; dense at 1 +- k eps, at 2^k +- 1 ulp, at sqrt(1/2) +- 1 ulp; exactly 0 at 1
    x = [1.0] + [1.0 + k * eps for k in range(-64, 65)] + [math.ldexp(1.0, k) for k in range(-1020, 997, 7)]
    x += [np.nextafter(math.ldexp(1.0, k), np.inf) for k in range(-1020, 997, 7)] + [np.nextafter(math.ldexp(1.0, k), 0) for k in range(-1020, 997, 7)]
    s = math.sqrt(0.5)
    x += [s, np.nextafter(s, 0), np.nextafter(s, 1), 2 * s, np.nextafter(2 * s, 0), np.nextafter(2 * s, 2)]
    x += list(10.0 ** rng.uniform(-300, 300, 4000)) + list(rng.uniform(0.5, 2.0, 4000))
    x = np.array(x)
    got = m.debug_pure(C["VICGPU_PURE_LN_POS"], x[:, None])
    assert got[0] == 0.0
    worst = max(_ulp_err(g, mpmath.log(mpmath.mpf(v))) for g, v in zip(got, x) if v != 1.0)
    print("ln_pos worst %.3f ulp over %d inputs" % (worst, len(x)))
    assert worst <= 1.0
    # pow_pos: the freezing curve's range, x = -Lf T / 273.16 / (g bubble / 100) for T in [-1e-12, -100], bubble 2-80 cm
    xs = (3.337e5 * 10.0 ** rng.uniform(-12, 2, 6000) / 273.16 / (9.81 * rng.uniform(2, 80, 6000) / 100.))
    ys = -2.0 / (rng.uniform(4, 40, 6000) - 3.0)
    got = m.debug_pure(C["VICGPU_PURE_POW_POS"], np.stack([xs, ys], 1))
    wr = 0.0
    for g, a, b in zip(got, xs, ys):
        want = mpmath.power(mpmath.mpf(a), mpmath.mpf(b))
        rel = float(abs(mpmath.mpf(g) / want - 1))
        # exp(v) with v = y ln_pos(x): ln_pos errs by <= 1 ulp of ln x (<= 2^-52 relative) and the product rounds once
        # (2^-53), a relative error of v that exp turns into |v| * 3 * 2^-53; the library exp adds <= 1 ulp (2 * 2^-53).
        # (2 + |v|) 2^-53 leaves out ln's own ulp: measured on gfx950, the worst case is 1.13 x that.
        bound = (2 + 3 * abs(b * math.log(a))) * 2.0 ** -53
        wr = max(wr, rel / bound)
        assert rel <= bound, (a, b, g)
    print("pow_pos worst %.3f of its bound (2 + 3 |y ln x|) 2^-53" % wr)
    # pow_pos corner cases (0, inf, NaN, negative): the library pow's special values bit for bit; finite results of a negative
    # base, and the bases at the ends of ln_pos's range, within the bound above
    cx = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -1.0, -2.5, 1e300, 2e300, 5e-324, 1.0])
    cy = np.array([-0.4, 0.5, 2.0, -1.0])
    xy = np.array([(a, b) for a in cx for b in cy])
    got = m.debug_pure(C["VICGPU_PURE_POW_POS"], xy)
    with np.errstate(all="ignore"):
        want = np.power(xy[:, 0], xy[:, 1])
    special = ~np.isfinite(want) | (want == 0) | ~np.isfinite(xy[:, 0]) | (xy[:, 0] == 0)
    same = (got.view(np.int64) == want.view(np.int64)) | (np.isnan(got) & np.isnan(want))
    assert same[special].all(), xy[special & ~same]
    for g, w, (a, b) in zip(got[~special], want[~special], xy[~special]):
        v = abs(b * math.log(abs(a)))
        assert abs(g / w - 1) <= (2 + 3 * v) * 2.0 ** -53, (a, b, g, w)
    # pow_pos_approx over the freezing curve's range (bound below); never NaN; 0 / inf where the float under-/overflows
    got = m.debug_pure(C["VICGPU_PURE_POW_POS_APPROX"], np.stack([xs, ys], 1))
    assert not np.isnan(got).any()
    want = np.array([float(mpmath.power(mpmath.mpf(a), mpmath.mpf(float(np.float32(b))))) for a, b in zip(xs, ys)])
    fin = (want > 1e-37) & (want < 1e37)
    rel = np.abs(got[fin] / want[fin] - 1)
    # Not 1e-6 flat: everything is single precision.  (float)x errs by 2^-24 relative (|y| 2^-24 after the power), v_log_f32
    # by ~1 ulp of log2 x and the product y log2 x rounds once, an absolute error of v = y log2 x up to 1.5 |v| 2^-23 that exp2
    # turns into ln2 1.5 |v| 2^-23 relative, and v_exp_f32 adds ~1 ulp: (3 + |y| + 3 ln2 |v|) 2^-24.  |v| reaches ~60 on this
    # range (expt 4, T = -100 K), i.e. ~5e-6.  The predictor only picks the start of the double-precision iteration.
    v = np.abs(ys[fin] * np.log2(xs[fin]))
    bound = (3 + np.abs(ys[fin]) + 3 * math.log(2) * v) * 2.0 ** -24
    print("pow_pos_approx worst rel %.3e, %.3f of its bound, over %d inputs in float range" % (rel.max(), (rel / bound).max(), fin.sum()))
    assert (rel <= bound).all()
    ext = m.debug_pure(C["VICGPU_PURE_POW_POS_APPROX"], np.array([[1e-30, 5.0], [1e30, 5.0], [1e-30, -5.0], [1e30, -5.0]]))
    assert ext[0] == 0.0 and ext[1] == np.inf and ext[2] == np.inf and ext[3] == 0.0, ext
    # rcp_refined over the normal range.  r = r0 + r0 (1 - d r0) with e0 = 1 - d r0 the seed's error: the exact value of that
    # expression is (1 - e0^2) / d, the inner fma is exact to 2^-53 e0 and the outer one rounds once, so the relative error is
    # <= e0^2 + 2^-53 (1 + e0).  2^-50 would need e0 <= 2^-25.5 from v_rcp_f64, whose accuracy is not documented; with a
    # single-precision-class seed (e0 <= 2^-24) the bound is 2^-48 + 2^-53.  Production only scales Newton steps with it.
    d = np.concatenate([10.0 ** rng.uniform(-300, 300, 6000), -10.0 ** rng.uniform(-300, 300, 2000), [1.0, 3.0, -7.0]])
    got = m.debug_pure(C["VICGPU_PURE_RCP_REFINED"], d[:, None])
    rel = np.array([float(abs(mpmath.mpf(g) * mpmath.mpf(v) - 1)) for g, v in zip(got, d)])
    print("rcp_refined worst rel %.3e (%.3f x 2^-52)" % (rel.max(), rel.max() / eps))
    assert rel.max() <= 2.0 ** -48 + 2.0 ** -53
    # Subnormal inputs: production never passes one.  ln_pos / pow_pos see -T * kappa with |T| >= 1e-310 K times kappa >= 150
    # (normal); pow_pos_approx and rcp_refined take floats of the iterate and the Newton denominator S x + Y Eu, whose
    # smallest magnitude is S * 1e-310 with S >= 1e3.  Recorded only:
    sub = np.array([5e-324, 1e-310, 2.2e-308])
    print("subnormal: ln_pos %s, rcp_refined %s, pow_pos_approx(x, -0.4) %s" % (
        m.debug_pure(C["VICGPU_PURE_LN_POS"], sub[:, None]), m.debug_pure(C["VICGPU_PURE_RCP_REFINED"], sub[:, None]),
        m.debug_pure(C["VICGPU_PURE_POW_POS_APPROX"], np.stack([sub, np.full(3, -0.4)], 1))))

