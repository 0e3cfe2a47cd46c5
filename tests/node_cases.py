"""The frozen-node root find as a unit: an arbitrary-precision reference of the reference's node residual and a battery of
edge cases in the layout of vicgpu_debug_node_root / vicorc_node_root (include/vicgpu.h VICGPU_NODE_NIN).

The residual is soil_thermal_eqn.c with maximum_unfrozen_water (soil_conduction.c:830-863) and both clamps, evaluated with
mpmath at 50 digits on the double inputs of a case.  Its sign changes in [T0 - 50.25, T0 + 50.25] (SOIL_DT + MAXTRIES * TSTEP,
root_brent.c:183-248) are found exactly: the residual is continuous and decreasing in T, except at node 1 with
|TL - TU| > 5 K, where the cold-nose variant drops the flux term ft1 = B (TL - TU) on an interval Tb < T < Thi; there it is
decreasing on each of the three pieces, so every sign change is either inside a piece (bisection) or a jump at a piece end.

The cases derive A-E from physical inputs with the reference's formulas (frozen_soil.c:161-212): heat capacity, conductivity,
node spacing or the EXP_TRANS geometry, and time step; the neighbour temperature TL (or T0 for the cold-nose classes) is then
solved so that the root lands where the class puts it.
"""
import math

import mpmath
import numpy as np

mp = mpmath.mp
mp.dps = 50

LF = 3.337e5
ICE_DENSITY = 917.0
SOIL_DT = 0.25
ROOT_RANGE = SOIL_DT + 5 * 10.0           # MAXTRIES * TSTEP
NODE_NEWTON_TOL = 1e-8                    # vic_profile.hpp: the last Newton step
NIN = 14
IA, IB, IC, ID, IE, IT0, IICE0, IMOIST, IMM, IBUB, IEXPT, ITL, ITU, IOLDT = range(NIN)

EXPTS = (4.0, 6.0, 10.0, 16.0, 25.0, 40.0)
BUBBLES = (2.0, 8.0, 30.0, 80.0)
RATIOS = (1e-6, 0.3, 0.99, 1.0)            # moist / max_moist
ICE0S = ("zero", "partial", "moist")
ROOTS = ("near0", "kink", "kink_lo", "kink_hi", "kink_cross", "curved", "deep", "bound_in", "bound_out", "positive")
STARTS = ("T0", "far", "other_side", "tiny", "subnormal", "root", "nonneg")
NOSES = ("nose_single", "nose_several", "nose_edge")


def tol(T):
    """Brent's stopping tolerance of the frozen-node root finds (root_brent.c:274)."""
    return 2 * 3e-8 * np.abs(T) + 1e-7


def _kap(bub):
    return mpmath.mpf(LF) / mpmath.mpf("273.16") / (mpmath.mpf("9.81") * mpmath.mpf(bub) / 100)


def ice_mp(T, moist, mm, bub, expt):
    T = mpmath.mpf(T)
    if T >= 0:
        return mpmath.mpf(0)
    u = mpmath.mpf(mm) * mpmath.power(-T * _kap(bub), -2 / (mpmath.mpf(expt) - 3))
    u = min(max(u, mpmath.mpf(0)), mpmath.mpf(mm))
    ice = mpmath.mpf(moist) - u
    return min(max(ice, mpmath.mpf(0)), mpmath.mpf(mm))


def _terms(c, T, exp_trans):
    A, B, C, D, E, T0, ice0 = (mpmath.mpf(float(c[i])) for i in (IA, IB, IC, ID, IE, IT0, IICE0))
    TL, TU = mpmath.mpf(float(c[ITL])), mpmath.mpf(float(c[ITU]))
    ice = ice_mp(T, c[IMOIST], c[IMM], c[IBUB], c[IEXPT])
    ft1 = B * (TL - TU)
    if not exp_trans:
        ft2 = C * (TL - T) - D * (T - TU)
    else:
        ft2 = C * (TL - 2 * T + TU) - D * (TL - TU)
    g = -A * (T - T0) + ft1 + ft2 + E * (ice - ice0)
    return g, ft1, ft2


def residual(c, T, node1, exp_trans):
    """soil_thermal_eqn.c:47-131 at T (an mpf), for the case row c."""
    T = mpmath.mpf(T)
    g, ft1, ft2 = _terms(c, T, exp_trans)
    TL, TU = float(c[ITL]), float(c[ITU])
    if node1 and abs(TL - TU) > 5 and T < TL and T < TU and ft1 < 0 and ft2 > 0 and abs(ft1) > abs(ft2):
        return g - ft1
    return g


def nose_interval(c, exp_trans):
    """(Tb, Thi) of the cold-nose interval in exact arithmetic (vic_profile.hpp:201-213), or None when ft1 >= 0."""
    B, C, D = (mpmath.mpf(float(c[i])) for i in (IB, IC, ID))
    TL, TU = mpmath.mpf(float(c[ITL])), mpmath.mpf(float(c[ITU]))
    ft1 = B * (TL - TU)
    if not ft1 < 0:
        return None
    Thi = min(TL, TU)
    if not exp_trans:
        Tb = (C * TL + D * TU + ft1) / (C + D)
    else:
        num = C * (TL + TU) - D * (TL - TU)
        Thi = min(Thi, num / (2 * C))
        Tb = (num + ft1) / (2 * C)
    return Tb, Thi


def _bisect(f, lo, hi, flo):
    """f(lo) has the sign of flo and f(hi) the other one: the sign change to 1e-15 K (plus 60 digits of headroom)."""
    lo, hi = mpmath.mpf(lo), mpmath.mpf(hi)
    while hi - lo > mpmath.mpf("1e-16") * max(1, abs(lo)) and hi - lo > mpmath.mpf("1e-18"):
        mid = (lo + hi) / 2
        fm = f(mid)
        if (fm > 0) == (flo > 0) and fm != 0:
            lo = mid
        else:
            hi = mid
    return (lo + hi) / 2


def sign_changes(c, node1, exp_trans, lo, hi):
    """Every sign change of the residual in [lo, hi] (mpf list, ascending)."""
    f = lambda T: residual(c, T, node1, exp_trans)
    lo, hi = mpmath.mpf(lo), mpmath.mpf(hi)
    cuts = []
    TL, TU = float(c[ITL]), float(c[ITU])
    if node1 and abs(TL - TU) > 5:
        iv = nose_interval(c, exp_trans)
        if iv is not None and iv[0] < iv[1]:
            cuts = [b for b in iv if lo < b < hi]
    eps = mpmath.mpf("1e-40")
    ends = [lo] + cuts + [hi]
    roots = []
    prev_right = None
    for k in range(len(ends) - 1):
        a, b = ends[k], ends[k + 1]
        fa = f(a if k == 0 else a + eps * max(1, abs(a)))
        fb = f(b if k == len(ends) - 2 else b - eps * max(1, abs(b)))
        if prev_right is not None and (prev_right > 0) != (fa > 0):
            roots.append(a)                       # a jump across zero at a piece end
        if fa == 0:
            roots.append(a)
        elif (fa > 0) != (fb > 0) and fb != 0:
            roots.append(_bisect(f, a, b, fa))
        prev_right = fb
    return sorted(set(roots))


def smooth_root(c, exp_trans, half=1000.0):
    """The root of the residual without its cold-nose variant (decreasing): the unique sign change in T0 -+ half, or None."""
    T0 = float(c[IT0])
    r = sign_changes(c, False, exp_trans, T0 - half, T0 + half)
    return r[0] if r else None


def reference(cases, node1, exp_trans):
    """Per case: dict(roots=[sign changes in T0 -+ 50.25], smooth=root of the smooth residual, kinks=[T where ice(T) has a
    kink], closed=N/S when oldT >= 0)."""
    out = []
    for c in cases:
        T0 = float(c[IT0])
        d = {}
        if c[IOLDT] >= 0:
            A, B, C, D, E, ice0 = (mpmath.mpf(float(c[i])) for i in (IA, IB, IC, ID, IE, IICE0))
            TL, TU, T0m = mpmath.mpf(float(c[ITL])), mpmath.mpf(float(c[ITU])), mpmath.mpf(T0)
            if not exp_trans:
                d["closed"] = (A * T0m + B * (TL - TU) + C * TL + D * TU - E * ice0) / (A + C + D)
                d["scale"] = float((abs(A * T0m) + abs(B * (TL - TU)) + abs(C * TL) + abs(D * TU) + abs(E * ice0)) / (A + C + D))
            else:
                d["closed"] = (A * T0m + B * (TL - TU) + C * (TL + TU) - D * (TL - TU) - E * ice0) / (A + 2 * C)
                d["scale"] = float((abs(A * T0m) + abs(B * (TL - TU)) + abs(C * (TL + TU)) + abs(D * (TL - TU)) + abs(E * ice0)) / (A + 2 * C))
            out.append(d)
            continue
        d["roots"] = sign_changes(c, node1, exp_trans, T0 - ROOT_RANGE, T0 + ROOT_RANGE)
        d["smooth"] = smooth_root(c, exp_trans)
        kap = _kap(c[IBUB])
        Yinv = -(mpmath.mpf(c[IEXPT]) - 3) / 2
        d["kinks"] = [mpmath.mpf(0), -1 / kap]
        if c[IMOIST] > 0:
            d["kinks"].append(-mpmath.power(mpmath.mpf(float(c[IMOIST])) / mpmath.mpf(float(c[IMM])), Yinv) / kap)
        out.append(d)
    return out


# ------------------------------------------------------------------------------------------------ the battery
def _coefficients(rng, exp_trans, dt, kratio=None):
    """A..E of a node from physical inputs (frozen_soil.c:161-212): Cs, kappa of the node and its neighbours, geometry."""
    Cs = rng.uniform(1.0e6, 3.5e6)
    k = math.exp(rng.uniform(math.log(0.1), math.log(3.0)))
    if kratio is None:
        kup, kdn = k * rng.uniform(0.7, 1.4), k * rng.uniform(0.7, 1.4)
    else:
        kup, kdn = k * kratio[0], k * kratio[1]
    B = (kup - kdn) * dt
    if not exp_trans:
        be = math.exp(rng.uniform(math.log(0.02), math.log(2.0)))      # node spacing above, below
        ga = math.exp(rng.uniform(math.log(0.02), math.log(2.0)))
        al = be + ga
        A = Cs * al * al
        C = 2 * dt * k * al / ga
        D = 2 * dt * k * al / be
        E = ICE_DENSITY * LF * al * al
    else:
        Dp = rng.uniform(2.0, 10.0)
        Nn = int(rng.integers(5, 21))
        Bexp = math.log(Dp + 1.) / (Nn - 1)
        j = int(rng.integers(1, Nn - 1))
        z1 = math.exp(Bexp * j)                                        # Zsum_node[j] + 1
        A = 4 * Bexp * Bexp * Cs * z1 * z1
        C = 4 * dt * k
        D = 2 * dt * k * Bexp
        E = 4 * Bexp * Bexp * ICE_DENSITY * LF * z1 * z1
    return A, B, C, D, E


def kink_T(moist, mm, bub, expt):
    """Where ice(T) reaches zero: u(T) = moist (for moist = max_moist: where u stops being clipped)."""
    return float(-mpmath.power(mpmath.mpf(moist) / mpmath.mpf(mm), -(mpmath.mpf(expt) - 3) / 2) / _kap(bub))


def _solve_TL(row, r, exp_trans):
    """TL such that the smooth residual vanishes at r (None when TL's coefficient is too small to steer it)."""
    A, B, C, D, E, T0, ice0 = (mpmath.mpf(row[i]) for i in (IA, IB, IC, ID, IE, IT0, IICE0))
    TU = mpmath.mpf(row[ITU])
    rm = mpmath.mpf(r)
    ice = ice_mp(rm, row[IMOIST], row[IMM], row[IBUB], row[IEXPT])
    coef = B + C if not exp_trans else B + C - D
    if not coef > 0.2 * C:
        return None
    if not exp_trans:
        rhs = A * (rm - T0) + B * TU + C * rm + D * (rm - TU) - E * (ice - ice0)
    else:
        rhs = A * (rm - T0) + B * TU - C * (TU - 2 * rm) + D * TU - E * (ice - ice0)
    return float(rhs / coef)


def _solve_T0(row, r, exp_trans):
    """T0 such that the smooth residual vanishes at r."""
    A, B, C, D, E, ice0 = (mpmath.mpf(row[i]) for i in (IA, IB, IC, ID, IE, IICE0))
    TL, TU, rm = mpmath.mpf(row[ITL]), mpmath.mpf(row[ITU]), mpmath.mpf(r)
    ice = ice_mp(rm, row[IMOIST], row[IMM], row[IBUB], row[IEXPT])
    ft2 = C * (TL - rm) - D * (rm - TU) if not exp_trans else C * (TL - 2 * rm + TU) - D * (TL - TU)
    return float(rm - (B * (TL - TU) + ft2 + E * (ice - ice0)) / A)


def _water(rng, ratio, ice0cls):
    mm = rng.uniform(0.3, 0.55) if rng.random() < 0.85 else rng.uniform(20.0, 200.0)   # mm/mm, or mm (frozen_compat layers)
    moist = ratio * mm
    ice0 = {"zero": 0.0, "partial": moist * rng.uniform(0.05, 0.95), "moist": moist}[ice0cls]
    return moist, mm, ice0


def _target_root(rng, cls, moist, mm, bub, expt):
    if cls == "near0":
        return -10 ** rng.uniform(-9, -4)
    if cls in ("kink", "kink_lo", "kink_hi"):
        Tk = kink_T(moist, mm, bub, expt)
        if not -45.0 < Tk < -1e-9:
            return None
        if cls == "kink":
            return Tk
        rel = 10 ** rng.uniform(-12, -5)
        return Tk * (1 + rel) if cls == "kink_lo" else Tk * (1 - rel)
    if cls == "kink_cross":
        # the root 1e-7 to 1e-5 K on the ice-free side of the kink, the start on the curved side (start "kink_side"): the
        # Newton steps taken from the curved branch end past the kink, where the accept rule's kink guard must refuse them
        Tk = kink_T(moist, mm, bub, expt)
        if not -45.0 < Tk < -1e-3:
            return None
        return Tk + 10 ** rng.uniform(-7, -5)
    if cls == "curved":
        return -math.exp(rng.uniform(math.log(1e-3), math.log(30.0)))
    if cls == "deep":
        return rng.uniform(-50.0, -30.0)
    if cls in ("bound_in", "bound_out"):
        return -math.exp(rng.uniform(math.log(0.5), math.log(20.0)))
    if cls == "positive":
        return rng.uniform(0.0, 3.0)
    raise ValueError(cls)


def _start(rng, cls, T0, r):
    return {"T0": T0, "far": r - 40.0, "other_side": -rng.uniform(0.1, 5.0), "tiny": -1e-300, "subnormal": -1e-310,
            "root": r, "nonneg": rng.choice([0.0, rng.uniform(0.0, 3.0)])}[cls]


def make_battery(n_plain=1000, n_nose=150, seed=20261015):
    """Rows [n][NIN] and their labels: node1, exp_trans (bool arrays) and per case a dict of class names
    (soil: expt, bubble; water: ratio, ice0; root; start; nose)."""
    rng = np.random.default_rng(seed)
    rows, node1, expt_, labels = [], [], [], []
    i = 0
    while len(rows) < n_plain:
        i += 1
        exp_trans = bool(i % 2)
        dt = 3600.0 if rng.random() < 0.5 else 86400.0
        expt, bub = float(rng.choice(EXPTS)), float(rng.choice(BUBBLES))
        ratio, ice0cls = float(rng.choice(RATIOS)), str(rng.choice(ICE0S))
        rcls = ROOTS[len(rows) % len(ROOTS)]
        scls = "other_side" if rcls == "positive" else STARTS[(len(rows) // len(ROOTS)) % len(STARTS)]
        if scls == "other_side" and rcls != "positive":
            scls = "T0"
        if rcls == "kink_cross":
            scls = "kink_side"
        moist, mm, ice0 = _water(rng, ratio, ice0cls)
        r = _target_root(rng, rcls, moist, mm, bub, expt)
        if r is None:
            continue
        A, B, C, D, E = _coefficients(rng, exp_trans, dt)
        if rcls == "bound_in":
            T0 = r + rng.choice([-1.0, 1.0]) * (ROOT_RANGE - 1e-3)
        elif rcls == "bound_out":
            T0 = r + rng.choice([-1.0, 1.0]) * (ROOT_RANGE + 1e-3)
        else:
            T0 = r + rng.uniform(-3.0, 3.0)
        row = [A, B, C, D, E, T0, ice0, moist, mm, bub, expt, 0.0, r + rng.uniform(-3.0, 3.0), 0.0]
        TL = _solve_TL(row, r, exp_trans)
        if TL is None:
            continue
        row[ITL] = TL
        if scls == "kink_side":
            row[IOLDT] = kink_T(moist, mm, bub, expt) - 10 ** rng.uniform(-8, -4)
        else:
            row[IOLDT] = _start(rng, scls, T0, r)
        rows.append(row); node1.append(bool(rng.random() < 0.25)); expt_.append(exp_trans)
        labels.append(dict(expt=expt, bubble=bub, ratio=ratio, ice0=ice0cls, root=rcls, start=scls, nose=None, target=r))
    j = 0
    while len(rows) < n_plain + n_nose:
        j += 1
        exp_trans = bool(j % 2)
        dt = 3600.0 if rng.random() < 0.5 else 86400.0
        expt, bub = float(rng.choice(EXPTS)), float(rng.choice(BUBBLES))
        ratio, ice0cls = float(rng.choice(RATIOS[1:])), str(rng.choice(ICE0S))
        ncls = NOSES[len(rows) % len(NOSES)]
        moist, mm, ice0 = _water(rng, ratio, ice0cls)
        # ft1 = B (TL - TU) < 0 with TL < TU - 5: the conductivity grows downwards
        A, B, C, D, E = _coefficients(rng, exp_trans, dt, kratio=(rng.uniform(1.5, 3.0), rng.uniform(0.3, 0.7)))
        TL = -rng.uniform(1.0, 25.0)
        TU = TL + rng.uniform(5.5, 20.0)
        row = [A, B, C, D, E, 0.0, ice0, moist, mm, bub, expt, TL, TU, 0.0]
        iv = nose_interval(row, exp_trans)
        if iv is None or not iv[0] < iv[1]:
            continue
        Tb, Thi = float(iv[0]), float(iv[1])
        if ncls == "nose_single":
            r = Thi + rng.uniform(1e-4, 3.0)                     # the smooth root at or above Thi: one sign change
        elif ncls == "nose_several":
            r = Tb - rng.uniform(0.05, 0.9) * abs(B * (TL - TU)) / (A + C + D)   # below Tb, close enough for g + |ft1| > 0 at Tb:
            #                                                                       sign changes at r, at Tb and above
        else:
            r = Thi - 10 ** rng.uniform(-7, -3.5)                # just below Thi: the replay decision's margin
        if not r < 0:
            continue
        T0 = _solve_T0(row, r, exp_trans)
        if not abs(T0 - r) < 45.0:
            continue
        row[IT0] = T0
        row[IOLDT] = float(rng.choice([T0, r, r - 5.0])) if T0 < 0 else r
        rows.append(row); node1.append(True); expt_.append(exp_trans)
        labels.append(dict(expt=expt, bubble=bub, ratio=ratio, ice0=ice0cls, root=None, start=None, nose=ncls, target=r))
    return np.array(rows), np.array(node1), np.array(expt_), labels


def count_classes(labels):
    """{(kind, value): number of cases}."""
    cnt = {}
    for lb in labels:
        for k in ("expt", "bubble", "ratio", "ice0", "root", "start", "nose"):
            if lb[k] is not None:
                cnt[(k, lb[k])] = cnt.get((k, lb[k]), 0) + 1
    return cnt


# ------------------------------------------------------------------------------------------------ checks
def check(cases, node1, exp_trans, labels, refs, T, failed, mode, other=None):
    """Violations of the bounds (list of strings) and the worst error per class for the results T / failed of one
    root finder on the battery.  mode: "newton" (the device's Newton solver), "brent" (device Brent, or the oracle).
    other: for "newton", the device's Brent-mode results (T, failed): the cold-nose replay must equal them bit for bit."""
    bad, worst = [], {}

    def note(cls, err):
        worst[cls] = max(worst.get(cls, 0.0), err)

    for i, (c, ref) in enumerate(zip(cases, refs)):
        lb = labels[i]
        cls = lb["nose"] or lb["root"]
        tag = "case %d (%s, start %s, node1 %d, exp %d)" % (i, cls, lb["start"], node1[i], exp_trans[i])
        if "closed" in ref:
            # N is a sum of terms that cancel: a few roundings of the largest of them, over S
            err = abs(T[i] - float(ref["closed"]))
            note("closed", err / ref["scale"])
            if failed[i] or not err <= 8 * 2.0 ** -53 * ref["scale"]:
                bad.append("%s: closed form %r vs %s, failed %d" % (tag, T[i], mpmath.nstr(ref["closed"], 17), failed[i]))
            continue
        T0 = float(c[IT0])
        roots = [float(r) for r in ref["roots"]]
        sm = ref["smooth"]
        near_bound = sm is not None and abs(abs(float(sm) - T0) - ROOT_RANGE) < 1e-6
        nose_iv = nose_interval(c, exp_trans[i]) if (node1[i] and abs(c[ITL] - c[ITU]) > 5) else None
        several = len(roots) > 1
        # the replay decision of the Newton solver (vic_profile.hpp:201-213) in exact arithmetic
        replay = None
        if nose_iv is not None and nose_iv[0] < nose_iv[1] and sm is not None:
            d = float(sm - nose_iv[1]) - 1e-6
            replay = None if abs(d) < 1e-8 else d < 0
        if mode == "newton" and replay:
            if other is not None and not (T[i] == other[0][i] and failed[i] == other[1][i]):
                bad.append("%s: cold-nose replay %r / %d differs from the Brent mode's %r" % (tag, T[i], failed[i], other[0][i]))
            mode_i = "brent"
        else:
            mode_i = mode
        if mode_i == "brent":
            if not roots:
                if not failed[i]:
                    bad.append("%s: no sign change in range, got %r" % (tag, T[i]))
                continue
            if failed[i]:
                bad.append("%s: failed, sign changes at %s" % (tag, roots))
                continue
            err = min(abs(T[i] - r) for r in roots)
            r0 = min(roots, key=lambda r: abs(T[i] - r))
            note(cls, err)
            if not err <= 2 * tol(r0):
                bad.append("%s: |T - r| = %.3e > 2 tol (T %r, roots %s)" % (tag, err, T[i], roots))
            continue
        # Newton
        if near_bound:
            continue
        if several and replay is None:
            continue                                           # a borderline replay decision: either answer is right
        if not roots:
            if not failed[i]:
                bad.append("%s: no root in range, got %r" % (tag, T[i]))
            continue
        if failed[i]:
            bad.append("%s: failed, root %r in range" % (tag, roots))
            continue
        r = roots[0]
        err = abs(T[i] - r)
        note(cls, err)
        if not err <= NODE_NEWTON_TOL:
            bad.append("%s: |T - r| = %.3e > 1e-8 (T %r, r %r)" % (tag, err, T[i], r))
        kink_d = min(abs(r - float(k)) for k in ref["kinks"])
        if r <= -1e-4 and kink_d >= 1e-6 and r < float(ref["kinks"][-1]):
            note(cls + "/curved", err)
            if not err <= 1e-9 + 1e-12 * abs(r):
                bad.append("%s: curved branch |T - r| = %.3e > 1e-9 + 1e-12 |r| (T %r, r %r)" % (tag, err, T[i], r))
    return bad, worst


def run_groups(fn, cases, node1, exp_trans):
    """fn(rows, node1, exp_trans) -> (T, failed) called once per (node1, exp_trans) group; results in case order."""
    T = np.zeros(len(cases)); F = np.zeros(len(cases), bool)
    for a in (False, True):
        for b in (False, True):
            m = (node1 == a) & (exp_trans == b)
            if m.any():
                T[m], F[m] = fn(cases[m], a, b)
    return T, F


def device_fn(model, newton):
    """The device hook as a run_groups function."""
    from vic_amd.abi import C

    def fn(rows, node1, exp_trans):
        mode = (C["VICGPU_NODE_NODE1"] if node1 else 0) | (C["VICGPU_NODE_NEWTON"] if newton else 0) | \
               (C["VICGPU_NODE_EXP_TRANS"] if exp_trans else 0)
        return model.debug_node_root(mode, rows)
    return fn


def references(cases, node1, exp_trans):
    return [reference(cases[i:i + 1], node1[i], exp_trans[i])[0] for i in range(len(cases))]


def hook_model():
    """A one-cell FROZEN_SOIL domain: the context vicgpu_debug_node_root needs (the hook reads nothing from it)."""
    from vic_amd import abi, domain
    from vic_amd.api import Model
    opt = abi.default_options(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=10, frozen_compat=0)
    return Model(domain.make_domain(1, opt))
