"""The battery of tests/test_brent.py: root finds that pin the device's Brent state machines (vic_math.hpp Brent and
BrentLean) to the reference's RootBrent::root_brent (root_brent.c:97-337), evaluation by evaluation.

A case is a bracket (lower, upper) and a residual.  Residuals are of two kinds:
  * functions of x built from + - * / and comparisons only, at brackets shaped like the model's call sites: (T0 - 1, 0)
    with the upper end exactly 0 (the ground surface under snow), 0.5 (T0 + Tair) +- 1 (the bare ground surface), T +- 5
    (snow pack, glacier), (T - 5, 0) (the canopy) and T0 +- 0.25 (a frozen soil node); temperatures around 300 as well,
    where the tolerance is dominated by 2 MACHEPS |b|.  Where the exact root is known, `mp_root` holds it (mpmath; a
    tuple where the function has several);
  * scripted residuals: the k-th value of a script whatever x is (then, past the script, a function of x).  They reach
    states no smooth function reaches: ties of the swap and bisection tests, a step of exactly tol, an interval of
    exactly 2 tol, subnormal values in the main loop, ERROR values at a chosen evaluation.  Traces of real solves of the
    oracle's model runs are scripted residuals too (`record_traces`).

Every case is run through `transcribe`, a plain-Python transcription of root_brent.c:97-337 that labels each path it
takes; test_battery_covers_every_path holds a minimum count per label, so the battery cannot thin out quietly.  The
transcription is checked bit for bit against the reference (tests/golden/brent_traces.npz, tests/test_brent.py).

Excluded, because the reference itself is undefined there:
  * NaN or inf residuals;
  * |fb| below about 1.5e-162 when the main loop starts: fb * fc = fb^2 underflows to 0, the test at root_brent.c:258
    fails and root_brent.c:264-274 reads c, d and e, which nothing has set (uninitialised locals).

The longest main loop: the reference fails after MAXITER = 1000 main-loop evaluations, and no case reaches that, so the
battery does not pin that exit (`i >= MAXITER` in Brent::advance and BrentLean::advance; a mutation there goes
unnoticed).  An estimate, not a proof, of why no residual reaches it at the model's brackets: each step either bisects
or moves by at least tol toward c, and an interpolation step is accepted only while it is smaller than half the step
before last (root_brent.c:305); so between two bisections lie at most about 2 log2(W / tol) steps, and the bisections
halve W.  For W = 100-110 K (the widest the five expansions give at these call sites) and tol = 1e-7 K that is about
log2(W / tol)^2 ~ 900-930 evaluations, whatever the residual returns -- a thin margin to 1000.  A residual must also keep
most steps short without letting the bracket collapse; the battery's adversarial script (`adversarial_script`) reaches
about 250.
"""
import math

import numpy as np

MAXTRIES, MAXITER = 5, 1000                     # root_brent.c:32-36
MACHEPS, TTOL, TSTEP = 3e-8, 1e-7, 10.0
ERROR = -999.0
UNDEFINED_FB = 1.5e-162                         # fb * fb underflows to 0 below this


class Undefined(Exception):
    """The reference reads uninitialised variables on this input (see the module docstring)."""


def _div(x, y):
    """IEEE division (Python raises on a zero divisor)."""
    if y != 0:
        return x / y
    if x != x or x == 0:
        return math.nan
    return math.copysign(math.inf, x) * math.copysign(1.0, y)


class Run:
    """What one transcribed root find did: xs / fs (every residual request in order and the value given), result,
    failed, the device's counters at return (i, j, k, which_err), labels (the paths taken) and, per main-loop
    evaluation, the branch that chose its abscissa and the relative margin of the acceptance tests (branch, margin)."""
    __slots__ = ("xs", "fs", "result", "failed", "i", "j", "k", "which_err", "labels", "steps", "nmain", "state")

    def __init__(self):
        self.xs, self.fs, self.labels, self.steps = [], [], set(), []
        self.result, self.failed, self.i, self.j, self.k, self.which_err, self.nmain = ERROR, True, 0, 0, 0, 0, 0
        self.state = None


def transcribe(lower, upper, f, macheps=MACHEPS, ttol=TTOL):
    """root_brent.c:97-337, step by step, with the counters named as in vic_math.hpp's Brent (k: the halvings of the
    current bisection search, j: the expansions, i: the main-loop evaluations).  f(x) -> float."""
    R = Run()
    L = R.labels

    def ev(x):
        fx = float(f(x))
        R.xs.append(x)
        R.fs.append(fx)
        return fx

    def done(result, label):
        R.result, R.failed = result, result == ERROR
        L.add(label)
        L.add("fail" if R.failed else "success")
        return R

    a, b = lower, upper
    if a == b:
        L.add("equal_bounds")
    fa = ev(a)
    fb = ev(b)
    which_err = 0
    if fa == ERROR and fb == ERROR:                                               # :129-132
        return done(ERROR, "err_both")
    last_bad = last_good = 0.0
    if fa == ERROR or fb == ERROR:                                                # :136-177
        if fa == ERROR:
            which_err, last_bad, last_good = -1, a, b
            L.add("err_a")
        else:
            which_err, last_good, last_bad = 1, a, b
            L.add("err_b")
        R.which_err = which_err
        c = 0.5 * (last_bad + last_good)
        fc = ev(c)
        R.k = 0
        while fc == ERROR and R.k < MAXITER:
            last_bad = c
            c = 0.5 * (last_bad + last_good)
            fc = ev(c)
            R.k += 1
        if fc == ERROR:
            L.add("search0_exhausted")
            return done(ERROR, "search0_fail")
        L.add({0: "search0_0", 1: "search0_1", 2: "search0_2"}.get(R.k, "search0_many" if R.k >= 40 else "search0_some"))
        if which_err == -1:
            a, fa = c, fc
        else:
            b, fb = c, fc
    R.j = 0
    while fa * fb >= 0 and R.j < MAXTRIES:                                        # :183-243
        if fa * fb == 0:
            L.add("zero_at_end" if (fa == 0 or fb == 0) else "underflow_product")
        if which_err == 0:
            a -= TSTEP
            b += TSTEP
            fa = ev(a)
            fb = ev(b)
        else:
            if which_err == -1:
                b += TSTEP
                fb = ev(b)
                if fb == ERROR:
                    return done(ERROR, "exp_one_fail_up")
                last_good = a
            else:
                a -= TSTEP
                fa = ev(a)
                if fa == ERROR:
                    return done(ERROR, "exp_one_fail_down")
                last_good = b
            c = 0.5 * (last_good + last_bad)
            fc = ev(c)
            R.k = 0
            L.add("search1")
            while fc == ERROR and R.k < MAXITER:
                last_bad = c
                c = 0.5 * (last_bad + last_good)
                fc = ev(c)
                R.k += 1
                L.add("search1_halving")
            if fc == ERROR:
                L.add("search1_exhausted")
                return done(ERROR, "search1_fail")
            if which_err == -1:
                a, fa = c, fc
            else:
                b, fb = c, fc
        R.j += 1
    if fa * fb >= 0:                                                              # :244-248
        if fa * fb == 0:
            L.add("zero_at_end" if (fa == 0 or fb == 0) else "underflow_product")
        return done(ERROR, "expand_fail")
    L.add("bracketed" if R.j == 0 and which_err == 0 else "expand_%d" % R.j)

    if abs(fb) < UNDEFINED_FB:
        raise Undefined("|fb| = %g at main-loop entry" % abs(fb))
    fc = fb
    c = d = e = math.nan                                                         # never read: fb * fc > 0 here
    R.i = 0
    while R.i < MAXITER:                                                          # :256-332
        if fb * fc > 0:
            c, fc = a, fa
            d = b - a
            e = d
        if abs(fc) < abs(fb):
            a, b, c = b, c, b
            fa, fb, fc = fb, fc, fb
            L.add("swap")
        elif abs(fc) == abs(fb):
            L.add("swap_tie")
        tol = 2 * macheps * abs(b) + ttol
        if 2 * macheps * abs(b) > 10 * ttol:
            L.add("tol_rel")
        m = 0.5 * (c - b)
        if abs(m) <= tol or fb == 0:
            if fb == 0:
                L.add("stop_fb0")
            if abs(m) == tol:
                L.add("stop_m_eq")
            return done(b, "stop_m" if abs(m) <= tol else "stop_fb")
        margin = math.inf
        if abs(e) < tol or abs(fa) <= abs(fb):
            branch = "bisect"
            L.add("bisect_e" if abs(e) < tol else ("bisect_fa_tie" if abs(fa) == abs(fb) else "bisect_fa"))
            d = m
            e = d
        else:
            s = fb / fa
            if a == c:
                L.add("secant")
                p = 2 * m * s
                q = 1 - s
            else:
                L.add("iqi")
                q = fa / fc
                r = fb / fc
                p = s * (2 * m * q * (q - r) - (b - a) * (r - 1))
                q = (q - 1) * (r - 1) * (s - 1)
            if p > 0:
                q = -q
            else:
                p = -p
            s = e
            e = d
            t1l, t1r = 2 * p, 3 * m * q - abs(tol * q)
            t2l, t2r = p, abs(0.5 * s * q)
            t1, t2 = t1l < t1r, t2l < t2r
            margin = min(_rel(t1l, t1r), _rel(t2l, t2r))
            if t1 and t2:
                branch = "accept"
                d = _div(p, q)
            else:
                branch = "reject"
                L.add("reject_t1" if not t1 else "reject_t2")
                if not t1 and t2:
                    L.add("reject_t1_only")
                d = m
                e = d
            L.add(branch)
        a = b
        fa = fb
        if abs(d) > tol:
            b += d
        else:
            L.add("step_tol")
            if abs(d) == tol:
                L.add("step_tol_eq")
            b += tol if m > 0 else -tol
        R.steps.append((branch, margin))
        fb = ev(b)
        R.state = (a, b, c)
        if fb == ERROR:
            L.add("main_err_first" if R.i == 0 else ("main_err_late" if R.i >= 5 else "main_err_early"))
            R.nmain = R.i + 1
            return done(ERROR, "main_err")
        if fb != 0 and abs(fb) < 2.2250738585072014e-308:
            L.add("subnormal_main")
        R.i += 1
        R.nmain = R.i
    return done(ERROR, "maxiter")


def _rel(l, r):
    """Relative distance of the two sides of an acceptance test."""
    den = max(abs(l), abs(r))
    return abs(l - r) / den if den > 0 else 0.0


# ------------------------------------------------------------------------------------------------ residuals
class Script:
    """The k-th value of `vals` at the k-th call, whatever x is; past the script, tail(x) (None: ERROR)."""

    def __init__(self, vals, tail=None):
        self.vals, self.tail, self.k = [float(v) for v in vals], tail, 0

    def __call__(self, x):
        k = self.k
        self.k += 1
        if k < len(self.vals):
            return self.vals[k]
        return self.tail(x) if self.tail is not None else ERROR


def lin(r, s):
    return lambda x: s * (x - r)


def cubic(r1, r2, r3, s):
    return lambda x: s * (x - r1) * (x - r2) * (x - r3)


def cubic_expanded(p, q):
    return lambda x: x * x * x + p * x + q


def rational(r, w):
    return lambda x: (x - r) / (w + (x - r) * (x - r))


def triple(r, s):
    return lambda x: s * (x - r) * (x - r) * (x - r)


def jump(r, lo, hi):
    return lambda x: lo if x < r else hi


def clamp(r, s, w):
    def f(x):
        v = s * (x - r)
        return w if v > w else (-w if v < -w else v)
    return f


def balance(Ta, sw, h):
    """An energy balance shaped like the surface one: sw - eps sigma (T + 273.15)^4 - h (T - Ta)."""
    def f(x):
        t = x + 273.15
        return sw - 5.67e-8 * 0.97 * (t * t) * (t * t) - h * (x - Ta)
    return f


def err_below(e, g):
    return lambda x: ERROR if x < e else g(x)


def err_above(e, g):
    return lambda x: ERROR if x > e else g(x)


def err_outside(lo, hi, g):
    return lambda x: ERROR if (x < lo or x > hi) else g(x)


def err_near(r, w, g):
    return lambda x: ERROR if (x - r < w and r - x < w) else g(x)


def _mp_root(f_mp, lo, hi):
    import mpmath
    mpmath.mp.prec = 200
    return float(mpmath.findroot(f_mp, (mpmath.mpf(lo), mpmath.mpf(hi)), solver="anderson"))


# ------------------------------------------------------------------------------------------------ the battery
class Case:
    """src: for a recorded trace, (index into TRACE_RUNS, the solve's running number in that run); else (-1, -1)."""
    __slots__ = ("cls", "lower", "upper", "make", "mp_root", "src")

    def __init__(self, cls, lower, upper, make, mp_root=None, src=(-1, -1)):
        self.cls, self.lower, self.upper, self.make, self.mp_root, self.src = cls, float(lower), float(upper), make, mp_root, src


def _brackets(rng, n):
    """n brackets shaped like the model's call sites: (name, lower, upper, centre)."""
    out = []
    shapes = ("snow", "surf", "pack", "canopy", "node", "hot")
    for k in range(n):
        s = shapes[k % len(shapes)]
        T0 = float(np.round(rng.uniform(-30, 25), 3))
        if s == "snow":
            T0 = -abs(T0)
            out.append((s, T0 - 1.0, 0.0))
        elif s == "surf":
            Ta = float(np.round(rng.uniform(-25, 30), 2))
            mid = 0.5 * (T0 + Ta)
            out.append((s, mid - 1.0, mid + 1.0))
        elif s == "pack":
            out.append((s, T0 - 5.0, T0 + 5.0))
        elif s == "canopy":
            T0 = -abs(T0)
            out.append((s, T0 - 5.0, 0.0))
        elif s == "node":
            out.append((s, T0 - 0.25, T0 + 0.25))
        else:
            T0 = float(np.round(rng.uniform(280, 320), 3))
            out.append((s, T0 - 5.0, T0 + 5.0))
    return out


def function_cases(rng):
    """Residual functions of x with a known root (mp_root) inside the bracket or 1 to 5 expansions away, or none."""
    import mpmath
    cases = []
    for shape, lo, hi in _brackets(rng, 650):
        w = hi - lo
        kind = rng.integers(0, 8)
        where = rng.integers(0, 10)                         # 0-5: inside; 6-8: n expansions away; 9: beyond reach
        if where <= 5:
            r = lo + w * float(rng.uniform(0.02, 0.98))
            nexp = 0
        elif where <= 8:
            nexp = int(rng.integers(1, 6))
            side = 1 if rng.integers(0, 2) else -1
            r = (hi + TSTEP * (nexp - 1) + float(rng.uniform(0.1, 9.9))) if side > 0 else (lo - TSTEP * (nexp - 1) - float(rng.uniform(0.1, 9.9)))
        else:
            side = 1 if rng.integers(0, 2) else -1
            r = hi + 55.0 + float(rng.uniform(0, 20)) if side > 0 else lo - 55.0 - float(rng.uniform(0, 20))
            nexp = 6
        r = float(np.round(r, 6))
        sgn = 1.0 if rng.integers(0, 2) else -1.0
        if kind == 0:
            s = sgn * float(10 ** rng.uniform(-3, 3))
            cases.append(Case("fn_lin", lo, hi, (lambda r=r, s=s: lin(r, s)), r if nexp < 6 else None))
        elif kind == 1:
            r2, r3 = r + 60.0 + float(rng.uniform(0, 30)), r - 60.0 - float(rng.uniform(0, 30))
            s = sgn * float(10 ** rng.uniform(-4, 0))
            cases.append(Case("fn_cubic", lo, hi, (lambda r=r, r2=r2, r3=r3, s=s: cubic(r, r2, r3, s)), (r, r2, r3)))
        elif kind == 2:
            # x^3 + p x + q with one real root r: p > 0, q = -(r^3 + p r)
            p = float(np.round(rng.uniform(0.5, 50), 3))
            q = -(r * r * r + p * r)
            root = None
            if nexp < 6:          # the real one of the three
                root = float(min(mpmath.polyroots([1, 0, mpmath.mpf(p), mpmath.mpf(q)], extraprec=300), key=lambda z: abs(z.imag)).real)
            cases.append(Case("fn_cubic_expanded", lo, hi, (lambda p=p, q=q: cubic_expanded(p, q)), root))
        elif kind == 3:
            wd = float(10 ** rng.uniform(-2, 2))
            cases.append(Case("fn_rational", lo, hi, (lambda r=r, wd=wd: rational(r, wd)), r if nexp < 6 else None))
        elif kind == 4:
            s = sgn * float(10 ** rng.uniform(-2, 2))
            cases.append(Case("fn_triple", lo, hi, (lambda r=r, s=s: triple(r, s)), r if nexp < 6 else None))
        elif kind == 5:
            lo_v, hi_v = -float(10 ** rng.uniform(-3, 3)), float(10 ** rng.uniform(-3, 3))
            cases.append(Case("fn_jump", lo, hi, (lambda r=r, a=lo_v, b=hi_v: jump(r, a, b)), r if nexp < 6 else None))
        elif kind == 6:
            s, wd = sgn * float(10 ** rng.uniform(-1, 3)), float(10 ** rng.uniform(-2, 1))
            cases.append(Case("fn_flat", lo, hi, (lambda r=r, s=s, wd=wd: clamp(r, s, wd)), r if nexp < 6 else None))
        else:
            if shape == "hot":
                continue
            Ta = float(np.round(rng.uniform(-25, 30), 2))
            h = float(np.round(rng.uniform(1, 40), 3))
            sw = 5.67e-8 * 0.97 * (r + 273.15) ** 4 + h * (r - Ta)
            sw = float(np.round(sw, 6))

            def fm(x, Ta=Ta, h=h, sw=sw):
                import mpmath as mp
                t = x + mp.mpf(273.15)
                return mp.mpf(sw) - mp.mpf(5.67e-8) * mp.mpf(0.97) * t ** 4 - mp.mpf(h) * (x - mp.mpf(Ta))
            root = _mp_root(fm, r - 1, r + 1) if nexp < 6 else None
            cases.append(Case("fn_balance", lo, hi, (lambda Ta=Ta, sw=sw, h=h: balance(Ta, sw, h)), root))
    # the bracket ends themselves: an exact zero at an end, and lower == upper
    for shape, lo, hi in _brackets(rng, 60):
        r = lo if rng.integers(0, 2) else hi
        s = float(10 ** rng.uniform(-2, 2))
        cases.append(Case("fn_zero_at_end", lo, hi, (lambda r=r, s=s: lin(r, s)), r))
    for shape, lo, hi in _brackets(rng, 30):
        r = lo + float(rng.uniform(-30, 30))
        cases.append(Case("fn_equal_bounds", lo, lo, (lambda r=r: lin(r, 1.0)), r if abs(r - lo) < 45 else None))
    # fa * fb underflows to +-0 although the signs differ: expansion, then failure (or success once the values grow)
    for shape, lo, hi in _brackets(rng, 30):
        r = lo + (hi - lo) * float(rng.uniform(0.2, 0.8))
        s = float(10 ** rng.uniform(-172, -166))
        cases.append(Case("fn_underflow_product", lo, hi, (lambda r=r, s=s: lin(r, s)), None))
    return cases


def error_cases(rng):
    """Residuals that return ERROR (-999) on part of the line: the bisection searches and the failures around them."""
    cases = []
    for shape, lo, hi in _brackets(rng, 240):
        w = hi - lo
        kind = int(rng.integers(0, 8))
        r = lo + w * float(rng.uniform(0.6, 0.9))
        g = (lambda r=r: lin(r, 3.0))
        if kind == 0:       # ERROR at a, the search finds the valid side after n halvings (n = 1, 2, ~50)
            n = int(rng.choice([1, 2, 3, 50]))
            e = hi - w / 2.0 ** (n + 1) - w / 2.0 ** (n + 3)
            cases.append(Case("err_a_search", lo, hi, (lambda e=e, g=g: err_below(e, g())), None))
        elif kind == 1:     # ERROR at b
            n = int(rng.choice([1, 2, 3, 50]))
            r = lo + w * float(rng.uniform(0.1, 0.4))
            e = lo + w / 2.0 ** (n + 1) + w / 2.0 ** (n + 3)
            cases.append(Case("err_b_search", lo, hi, (lambda e=e, r=r: err_above(e, lin(r, 2.0))), None))
        elif kind == 2:     # ERROR at both ends
            cases.append(Case("err_both", lo, hi, (lambda lo=lo, hi=hi, g=g: err_outside(lo + 1e-3, hi - 1e-3, g())), None))
        elif kind == 3:     # ERROR at a, no sign change in range: the upper end moves, and hits ERROR (EXP_ONE failure)
            e = lo + 0.3 * w
            top = hi + TSTEP * int(rng.integers(0, 4)) + 5.0
            cases.append(Case("err_exp_one_up", lo, hi, (lambda e=e, top=top: err_outside(e, top, lambda x: x * x + 1.0)), None))
        elif kind == 4:     # ERROR at b, the lower end moves down into ERROR
            e = hi - 0.3 * w
            bot = lo - TSTEP * int(rng.integers(0, 4)) - 5.0
            cases.append(Case("err_exp_one_down", lo, hi, (lambda e=e, bot=bot: err_outside(bot, e, lambda x: x * x + 1.0)), None))
        elif kind == 5:     # ERROR at a, root above the range: the upper end moves, the search below runs (SEARCH1)
            e = lo + 0.3 * w
            r = hi + TSTEP * int(rng.integers(0, 4)) + float(rng.uniform(1, 9))
            cases.append(Case("err_search1_up", lo, hi, (lambda e=e, r=r: err_below(e, lin(r, 1.5))), r))
        elif kind == 6:     # ERROR at b, root below: the lower end moves
            e = hi - 0.3 * w
            r = lo - TSTEP * int(rng.integers(0, 4)) - float(rng.uniform(1, 9))
            cases.append(Case("err_search1_down", lo, hi, (lambda e=e, r=r: err_above(e, lin(r, -0.7))), r))
        else:               # ERROR close to the root: the main loop runs into it
            wd = float(10 ** rng.uniform(-6, -2))
            r = lo + w * float(rng.uniform(0.2, 0.8))
            cases.append(Case("err_main", lo, hi, (lambda r=r, wd=wd: err_near(r + wd / 3, wd, cubic(r, r + 70, r - 80, 0.01))), None))
    # a residual of exactly -999.0 where a number was meant ((x - lo) - 999 at x = lo, negative at the upper end as well):
    # the reference reads it as ERROR and searches toward the upper end; read as a number it would expand the bracket
    for k in range(12):
        lo = -float(k)
        cases.append(Case("err_minus999_number", lo, lo + 500.0 + k, (lambda lo=lo: (lambda x: (x - lo) - 999.0)), None))
    return cases


def _state_script(rng):
    """A random script from a small alphabet (ties, zeros, subnormals, ERROR) followed by a function tail."""
    alpha = [1.0, -1.0, 2.0, -2.0, 0.5, -0.5, 3.0, -3.0, 1e-3, -1e-3, 0.0, 4e-310, -4e-310, 1e-170, -1e-170, 1e200, -1e200,
             ERROR, 0.25, -0.25]
    p = np.array([8, 8, 6, 6, 6, 6, 3, 3, 3, 3, 2, 2, 2, 1, 1, 1, 1, 2, 3, 3], dtype=float)
    n = int(rng.integers(3, 14))
    vals = [alpha[i] for i in rng.choice(len(alpha), size=n, p=p / p.sum())]
    return vals


def script_cases(rng, count=380):
    cases = []
    for shape, lo, hi in _brackets(rng, count):
        vals = _state_script(rng)
        r = lo + (hi - lo) * float(rng.uniform(0.1, 0.9))
        tail = int(rng.integers(0, 3))
        cases.append(Case("script_random", lo, hi, (lambda vals=vals, r=r, tail=tail: Script(vals, [lin(r, 1.0), cubic(r, r + 40, r - 50, 0.001), None][tail])), None))
    return cases


def _tie_scripts():
    """Hand-made scripts for exact ties and long searches."""
    out = []
    # |fc| == |fb| and |fa| == |fb| at the first iteration
    for lo, hi in ((-1.0, 1.0), (-5.0, 0.0), (295.0, 305.0), (-0.25, 0.25)):
        out.append(("script_tie", lo, hi, [1.0, -1.0], None))
        out.append(("script_tie", lo, hi, [-2.0, 2.0, 1.0], None))
        out.append(("script_tie", lo, hi, [-2.0, 1.0, 1.0, -0.5, 0.5], None))
    # SEARCH0 exhausted: every request after the valid end returns ERROR; the same for SEARCH1 after an expansion
    out.append(("script_search0_exhausted", -5.0, 5.0, [ERROR, 1.0] + [ERROR] * 1001, None))
    out.append(("script_search0_exhausted", -1.0, 0.0, [2.0, ERROR] + [ERROR] * 1001, None))
    out.append(("script_search1_exhausted", -5.0, 5.0, [ERROR, 1.0, ERROR, 2.0, 3.0] + [ERROR] * 1001, None))
    out.append(("script_search1_exhausted", 280.0, 290.0, [1.0, ERROR, 1.5, 2.0, 2.5] + [ERROR] * 1001, None))
    # SEARCH1 with halvings, then success
    out.append(("script_search1", -5.0, 5.0, [ERROR, 1.0, ERROR, 2.0, 3.0, ERROR, ERROR, 0.5, -1.0], "lin"))
    out.append(("script_search1", -5.0, 5.0, [2.0, ERROR, ERROR, 1.0, 3.0, ERROR, 0.5, -2.0], "lin"))
    # ERROR in the main loop: the first evaluation and a late one
    out.append(("script_main_err", -5.0, 5.0, [1.0, -1.0, ERROR], None))
    out.append(("script_main_err", -5.0, 5.0, [-3.0, 2.0, 1.0, 0.5, -0.1, 0.05, 0.01, -0.001, 0.0001, ERROR], None))
    # exact zeros in the main loop, subnormal values in the main loop
    out.append(("script_fb0", -5.0, 5.0, [1.0, -1.0, 0.0], None))
    out.append(("script_fb0", -5.0, 5.0, [1.0, -1.0, 0.5, -0.2, 0.0], None))
    for v in (4e-310, -4e-310, 5e-324, 2.2250738585072e-308):
        out.append(("script_subnormal", -5.0, 5.0, [-1.0, 1.0, v, -v, v / 2], "lin"))
        out.append(("script_subnormal", -1.0, 0.0, [2.0, -1.0, -1e-3, v, 1e-300], "lin"))
    return out


def tie_cases():
    cases = []
    for cls, lo, hi, vals, tail in _tie_scripts():
        r = 0.5 * (lo + hi)
        t = lin(r, 1.0) if tail == "lin" else None
        cases.append(Case(cls, lo, hi, (lambda vals=vals, t=t: Script(vals, t)), None))
    return cases


def step_tol_eq_cases():
    """A secant step of exactly tol (root_brent.c:321: |d| == tol takes the +-tol branch).  With fa at the lower end and
    fb = -1 at the upper one, the first step is |d| = 2 |m| / (fa + 1); fa is searched over the doubles next to
    2 |m| / tol - 1 until the step equals tol bit for bit."""
    cases = []
    for lo, hi in ((-1.0, 1.0), (-5.0, 0.0), (-0.25, 0.25), (0.0, 2.0), (290.0, 300.0), (-3.0, 7.0), (-30.0, -20.0),
                   (-1.5, 0.0), (12.0, 22.0)):
        tol = 2 * MACHEPS * abs(hi) + TTOL
        fa = 2 * abs(0.5 * (lo - hi)) / tol - 1.0
        for k in range(4000):
            v = fa + (k // 2 if k % 2 == 0 else -(k // 2 + 1)) * math.ulp(fa)
            tail = lin(0.5 * (lo + hi), -1.0)
            R = transcribe(lo, hi, Script([v, -1.0], tail))
            if "step_tol_eq" in R.labels:
                cases.append(Case("script_step_tol_eq", lo, hi, (lambda v=v, tail=tail: Script([v, -1.0], tail)), None))
                break
    return cases


def m_eq_tol_cases():
    """An interval of exactly 2 tol around b (root_brent.c:276: |m| == tol stops): c = b +- 2 tol for the first twelve b
    of a grid (0 and small multiples of 2^-24, where c - b is exact more often than not) where that is exact."""
    cases = []
    grid = [0.0] + [math.ldexp(k, -24) * sg for k in range(1, 4000) for sg in (1.0, -1.0)]
    for b in grid:
        if len(cases) >= 12:
            break
        tol = 2 * MACHEPS * abs(b) + TTOL
        for sg in (1.0, -1.0):
            c = b + sg * 2 * tol
            if 0.5 * (c - b) == sg * tol:
                cases.append(Case("script_m_eq_tol", c, b, (lambda sg=sg: Script([2.0 * sg, -sg], None)), None))
    return cases


def adversarial_script(lo, hi, frac=1.0 / 64, nmax=MAXITER + 100):
    """A script that keeps the main loop going: every value has the sign of the one before (so c stays where it is) and
    its size, one of a few, makes the next step the longest the acceptance test takes that is still below frac |c - b|."""
    vals = [-1.0, 1.0]
    mags = [float(v) for v in np.geomspace(1e-14, 0.999, 90)]
    while True:
        R = transcribe(lo, hi, Script(vals, None))
        if "main_err" not in R.labels or len(R.xs) <= len(vals) or R.nmain >= nmax:
            break
        a, b, c = R.state
        best = None
        for mg in mags:
            v = vals[-1] * mg
            Rt = transcribe(lo, hi, Script(vals + [v], None))
            if "main_err" not in Rt.labels or len(Rt.xs) != len(vals) + 2 or Rt.steps[-1][0] != "accept":
                continue
            st = abs(Rt.xs[-1] - Rt.xs[-2])
            if st <= abs(c - b) * frac and (best is None or st > best[0]):
                best = (st, v)
        vals.append(vals[-1] * 0.5 if best is None else best[1])
    return vals


def make_battery(seed=20261016, recorded=None):
    """All cases (list of Case).  recorded: the scripts of recorded_scripts(), appended as scripted cases."""
    rng = np.random.default_rng(seed)
    cases = function_cases(rng) + error_cases(rng) + script_cases(rng) + tie_cases() + step_tol_eq_cases() + m_eq_tol_cases()
    for cls, lo, hi, fs, src in recorded or ():
        cases.append(Case(cls, lo, hi, (lambda fs=fs: Script(fs, None)), None, src))
    return cases


def recorded_scripts():
    """The scripted cases that take long to make (make_golden_brent.py stores them in the fixture; tests read them from
    there): the oracle's traces and two adversarial main loops.  [(cls, lower, upper, script, src)]."""
    out = [("trace_" + kind, lo, hi, fs, src) for kind, lo, hi, fs, src in record_traces()]
    for lo, hi in ((-50.0, 50.0), (-5.0, 5.0)):
        out.append(("script_long", lo, hi, adversarial_script(lo, hi), (-1, -1)))
    return out


def run_battery(cases, long_cap=6):
    """Runs every case through the transcription.  Cases on which the reference is undefined are dropped, and so are the
    generated cases with more than 300 evaluations (exhausted searches) past the first long_cap of them.
    Returns (kept cases, runs)."""
    keep, runs = [], []
    nlong = 0
    for c in cases:
        try:
            R = transcribe(c.lower, c.upper, c.make())
        except Undefined:
            continue
        if any(not math.isfinite(v) for v in R.fs):
            continue
        if len(R.fs) > 300 and not c.cls.startswith(("script_", "trace_")):
            nlong += 1
            if nlong > long_cap:
                continue
        keep.append(c)
        runs.append(R)
    return keep, runs


def pack(cases, runs):
    """Arrays of the fixture: bounds [n][2], off [n+1], fs, xs, result, failed, cls (names), trace_src [n][2]."""
    off = np.zeros(len(runs) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(R.fs) for R in runs])
    return dict(bounds=np.array([[c.lower, c.upper] for c in cases], dtype=np.float64), off=off,
                fs=np.array([v for R in runs for v in R.fs], dtype=np.float64),
                xs=np.array([v for R in runs for v in R.xs], dtype=np.float64),
                result=np.array([R.result for R in runs], dtype=np.float64),
                failed=np.array([R.failed for R in runs], dtype=bool),
                cls=np.array([c.cls for c in cases]), trace_src=np.array([c.src for c in cases], dtype=np.int32))


# ------------------------------------------------------------------------------------------------ the fixture
RECORDED = ("trace_surf", "trace_node", "script_long")


def load_fixture():
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "brent_traces.npz"))
    return {k: g[k] for k in g.files}


def fixture_recorded(g):
    """The recorded scripts of the fixture, as make_battery takes them."""
    out = []
    for i, cls in enumerate(g["cls"]):
        if str(cls) in RECORDED:
            o0, o1 = g["off"][i], g["off"][i + 1]
            out.append((str(cls), float(g["bounds"][i, 0]), float(g["bounds"][i, 1]), [float(v) for v in g["fs"][o0:o1]],
                        tuple(int(v) for v in g["trace_src"][i])))
    return out


def fixture_battery(g):
    """The battery the fixture was made from: (cases, transcribed runs)."""
    return run_battery(make_battery(recorded=fixture_recorded(g)))


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def check_full(g, runs, xreq, out, idx=None):
    """Brent's replay (vicgpu_debug_root_brent mode 0) against the fixture, for the cases idx (default: all, in order):
    every abscissa, the count, no overrun, result, failure, and the transcription's counters.  Returns the problems."""
    bad = []
    idx = range(len(runs)) if idx is None else idx
    pos = 0
    for row, i in enumerate(idx):
        o0, o1 = g["off"][i], g["off"][i + 1]
        n = o1 - o0
        x = xreq[pos:pos + n]
        pos += n
        R = runs[i]
        exp = [n, 1, float(g["failed"][i]), g["result"][i], R.i, R.j, R.k, R.which_err, 0]
        if not same_bits(x, g["xs"][o0:o1]):
            k = int(np.flatnonzero(x.view(np.int64) != g["xs"][o0:o1].view(np.int64))[0])
            bad.append("case %d (%s): abscissa %d: %r != %r" % (i, g["cls"][i], k, x[k], g["xs"][o0 + k]))
        elif not same_bits(out[row], exp):
            bad.append("case %d (%s): out %s != %s" % (i, g["cls"][i], list(out[row]), exp))
    return bad


LEAN_STEP_REL = 1e-12          # the battery's largest difference is 6.2e-13 of the step


def check_lean(g, runs, xreq, out, idx):
    """BrentLean's replay (mode 1) of ERROR-free cases: the abscissae equal the reference's up to the first divergence; at
    that one the reference accepted an interpolation step and the two steps agree to LEAN_STEP_REL of the step (the
    common denominator rounds differently where the residuals nearly cancel) beyond 4 ulp of b + d, or the reference's
    acceptance test was a near-tie (relative margin < 1e-14); without a divergence the count, result and failure are
    the same.  Returns (problems, divergences [(case, evaluation, kind, |difference| / step beyond the 4 ulp)])."""
    bad, div = [], []
    pos = 0
    for row, i in enumerate(idx):
        o0, o1 = g["off"][i], g["off"][i + 1]
        n = o1 - o0
        x, xr = xreq[pos:pos + n], g["xs"][o0:o1]
        pos += n
        R = runs[i]
        used = int(out[row][0])
        m = min(used, n)
        ne = np.flatnonzero(x[:m].view(np.int64) != xr[:m].view(np.int64))
        if ne.size == 0:
            if not (used == n and out[row][1] == 1 and out[row][2] == g["failed"][i] and same_bits(out[row][3], g["result"][i])
                    and out[row][8] == 0):
                bad.append("case %d (%s): lean out %s, reference n %d result %r failed %d" % (
                    i, g["cls"][i], list(out[row]), n, g["result"][i], g["failed"][i]))
            continue
        k = int(ne[0])
        s = k - (n - len(R.steps))              # the main-loop step that chose abscissa k
        if s < 0:
            bad.append("case %d (%s): lean differs at evaluation %d, before the main loop" % (i, g["cls"][i], k))
            continue
        branch, margin = R.steps[s]
        step = abs(xr[k] - xr[k - 1])
        rel = max(0.0, abs(x[k] - xr[k]) - 4 * math.ulp(xr[k])) / step
        if branch == "accept" and rel <= LEAN_STEP_REL:
            div.append((i, k, "step", rel))
        elif margin < 1e-14:
            div.append((i, k, "tie", rel))
        else:
            bad.append("case %d (%s): lean differs at evaluation %d (step %d, %s, margin %.3e): %r != %r" % (
                i, g["cls"][i], k, s, branch, margin, x[k], xr[k]))
    return bad, div


LEAN_RANGE = (1e-100, 1e100)


def lean_cases(g):
    """The ERROR-free cases (no value of exactly -999, which BrentLean reads as a number) whose nonzero residuals lie
    within LEAN_RANGE: BrentLean's common denominator multiplies three residuals (fa fc^2), which overflows or underflows
    outside it where the reference's quotients do not.  The node residual (W/m^2) stays far inside."""
    out = []
    for i in range(len(g["cls"])):
        f = np.abs(g["fs"][g["off"][i]:g["off"][i + 1]])
        nz = f[f > 0]
        if not np.any(g["fs"][g["off"][i]:g["off"][i + 1]] == ERROR) and not np.any((nz < LEAN_RANGE[0]) | (nz > LEAN_RANGE[1])):
            out.append(i)
    return out


def gather(g, idx):
    """bounds, fvals, off of the cases idx, in that order."""
    b = g["bounds"][list(idx)]
    parts = [g["fs"][g["off"][i]:g["off"][i + 1]] for i in idx]
    off = np.zeros(len(parts) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(p) for p in parts])
    return b, (np.concatenate(parts) if parts else np.zeros(0)), off


TRACE_RUNS = (("stress_fallback_frozen", 20), ("deep_spikes_n50", 1), ("quick_solve", 12), ("ar_410", 24))


def record_solves(name, nsteps):
    """Every root find of the oracle's run of scenario `name` (tests/scenarios.py, tests/deep_scenarios.py) over nsteps
    steps, recorded through vicorc_set_brent_recorder and keyed by the solve's running number, so that the node solves a
    surface residual runs inside one evaluation do not mix with the surface solve.  Returns, in the order the solves
    started: [(solve, kind, lower, upper, macheps, ttol, xs, fs)], kind "node" for the frozen-node residual, "surf" for
    the others (ground surface, snow pack, canopy, glacier)."""
    import ctypes
    from oracle import pyref
    from tests import scenarios, deep_scenarios
    from vic_amd import init_state
    lib = ctypes.CDLL(pyref.oracle_lib_path())
    REC = ctypes.CFUNCTYPE(None, ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                           ctypes.c_double, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_void_p)
    lib.vicorc_set_brent_recorder.restype = None
    lib.vicorc_set_brent_recorder.argtypes = [REC, ctypes.c_void_p]
    lib.vicorc_node_residual.restype = ctypes.c_void_p
    node_fn = lib.vicorc_node_residual()
    solves = {}

    def rec(solve, fn, lower, upper, macheps, ttol, k, x, fx, _):
        if k == 0:
            assert solve not in solves
            solves[solve] = ("node" if fn == node_fn else "surf", lower, upper, macheps, ttol, [], [])
        e = solves[solve]
        assert len(e[5]) == k and (e[1], e[2]) == (lower, upper)
        e[5].append(x)
        e[6].append(fx)
    cb = REC(rec)
    lib.vicorc_set_brent_recorder(cb, None)
    try:
        deep = name in deep_scenarios.DEEP_BRANCHES
        sp, d, f, sf, dmy = (deep_scenarios if deep else scenarios).build(name, nsteps)
        sd0, si0 = init_state.initial_state(d, f[0])
        if deep:
            deep_scenarios.start_state(sp, sd0)
        orc = pyref.OracleModel(d)
        orc.set_state(sd0, si0)
        for s in range(nsteps):
            orc.step(f[s], sf[s], dmy[s], nthreads=1)
        orc.close()
    finally:
        lib.vicorc_set_brent_recorder(REC(0), None)
    return [(k,) + tuple(solves[k]) for k in sorted(solves)]


def record_traces(per_kind=200):
    """per_kind surface-type and per_kind frozen-node solves of the oracle's runs of TRACE_RUNS (record_solves), each
    checked to replay through the transcription with the abscissae recorded for it: the unusual ones first (ERROR
    values, failures, long runs), then an even spread of the rest.  Returns [(kind, lower, upper, fs, (run, solve))]."""
    pool = {"surf": [], "node": []}
    for r, (name, nsteps) in enumerate(TRACE_RUNS):
        for solve, kind, lo, hi, macheps, ttol, xs, fs in record_solves(name, nsteps):
            if (macheps, ttol) != (MACHEPS, TTOL):
                continue
            R = transcribe(lo, hi, Script(fs, None))
            assert R.xs == xs and R.fs == fs, (name, solve, kind)
            pool[kind].append((kind, lo, hi, fs, (r, solve)))
    out = []
    for kind in ("surf", "node"):
        sel = pool[kind]
        odd = [s for s in sel if ERROR in s[3] or len(s[3]) > 14]
        rest = [s for s in sel if not (ERROR in s[3] or len(s[3]) > 14)]
        take = odd[:per_kind // 2]
        stride = max(1, len(rest) // max(1, per_kind - len(take)))
        take += rest[::stride][:per_kind - len(take)]
        out += take
    return out


def count_labels(runs, cases):
    cnt = {}
    for c, R in zip(cases, runs):
        for l in R.labels:
            cnt[l] = cnt.get(l, 0) + 1
        cnt["cls:" + c.cls] = cnt.get("cls:" + c.cls, 0) + 1
    return cnt
