"""The per-column ensemble transform solved and applied on the device (vicgpu_member_transform_solve / _set / _get / _apply,
include/vicgpu.h).  The apply against the library's own vicgpu_mix_cells with the lists of domain.member_transform, bit for
bit, NaNs by position; the solve against the header's formulas evaluated with mpmath at 50 digits and with numpy's eigh.  Run by
tests/test_member_transform.py with VICGPU_LIB pointing at the unsanitized host build (SAN=none tools/hostemu/build.sh);
tests/test_member_transform_gpu.py imports the functions for the GPU.
    python tools/hostemu/check_member_transform.py apply       set a random T: apply == mix_cells, all columns and a shuffled
                                                               subset, two staging budgets, 4 x 35, 16 x 9 and 64 x 2; what a
                                                               call leaves alone; the same with the T a solve left
    python tools/hostemu/check_member_transform.py accuracy    the solve against mpmath and numpy; column sums
    python tools/hostemu/check_member_transform.py guarantees  (a) to (d) of the header
    python tools/hostemu/check_member_transform.py midrun      FROZEN_SOIL as one chunk and as two, right behind a two-step vicgpu_step
    python tools/hostemu/check_member_transform.py errors      every error return, each leaving every table and the transform as it was
    python tools/hostemu/check_member_transform.py refusals    the n-th allocation refused, for every n
    python tools/hostemu/check_member_transform.py endtoend    FULL_ENERGY + FROZEN_SOIL, 4 x 12: steps, solve from the SWE, apply, derive, steps
Each prints "member transform <name>: problems: none" (or the list) and exits with 1 when there are any."""
import ctypes
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import check_copy_cells as cc
import check_mix_cells as cm
import check_state_update as su
import check_update_params as cu
from vic_amd import abi, domain
from vic_amd.abi import C
from vic_amd.api import Model, VicGpuError, load_library

same, differing, same_nan = cc.same, cc.differing, cm.same_nan
model, clone = cu.model, cu.clone
CAP, NODES = C["VICGPU_DERIVE_CAP_MOIST"], C["VICGPU_DERIVE_NODES"]
SWEEPS = "VICGPU_TRANSFORM_SWEEPS"
SHAPES = ((4, 35), (16, 9), (64, 2))          # members x base columns


@functools.lru_cache(maxsize=None)
def ens(M, ncol):
    """The domain of check_mix_cells (cells of 6 or 9 HRUs) as M members of ncol base columns; 4 x 35 is its own case."""
    return cc.quickflux(ncol=ncol, M=M)


def started(E, stage_mb=None, steps=0):
    m = cc.start(model(E, clone(E.D), stage_mb=stage_mb), E)
    if steps:
        m.dist_prec(0, steps, sync=False)
    return m


# ------------------------------------------------------------------------------------------------ observations and yardsticks
def observations(M, ncol, seed, infl="mixed"):
    """(obs_off, hx, yobs, rinv, infl): the observation counts cycle through 0, 1, 3, 40 (from column 1 on; column 0 has 3
    observations whose rinv are all 0), rinv spans 1e-6 .. 1e6 with every seventh entry exactly 0, infl is 1, 1, 1.1, 1.1, 1, ...."""
    rng = np.random.default_rng(seed)
    counts = np.array([3] + [(40, 0, 1, 3)[j % 4] for j in range(ncol - 1)])
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    nobs = int(off[-1])
    truth = rng.normal(size=nobs)
    hx = truth[:, None] + rng.normal(size=(nobs, M)) * rng.uniform(0.1, 2.0, size=(nobs, 1))
    yobs = truth + 0.3 * rng.normal(size=nobs)
    rinv = 10.0 ** rng.uniform(-6, 6, size=nobs)
    rinv[::7] = 0.0
    rinv[off[0]:off[1]] = 0.0
    rinv[[rinv.argmax(), rinv.argmin()]] = [1e6, 0.0]
    rinv[np.flatnonzero(rinv)[0]] = 1e-6
    rho = None if infl is None else np.where((np.arange(ncol) // 2) % 2 == 0, 1.0, 1.1) if infl == "mixed" else np.full(ncol, float(infl))
    return off, np.ascontiguousarray(hx), yobs, rinv, rho


def np_transform(M, hx, yobs, rinv, rho):
    """The header's formulas for one column in plain float64, the eigendecomposition by numpy's eigh."""
    hx = hx.reshape(-1, M)
    ybar = hx.sum(axis=1) / M
    Y = hx - ybar[:, None]
    d = yobs - ybar
    RY = rinv[:, None] * Y
    A = RY.T @ Y + ((M - 1) / rho) * np.eye(M)
    A = 0.5 * (A + A.T)
    g = RY.T @ d
    lam, U = np.linalg.eigh(A)
    wbar = U @ ((U.T @ g) / lam)
    Wa = (U * np.sqrt((M - 1) / lam)) @ U.T
    W = Wa + wbar[:, None]
    return W + (1.0 - W.sum(axis=0))[None, :] / M


def mp_transform(M, hx, yobs, rinv, rho):
    """The same with mpmath at 50 digits, rounded to float64 at the end."""
    import mpmath as mp
    with mp.workdps(50):
        hx = hx.reshape(-1, M)
        n = hx.shape[0]
        H = [[mp.mpf(float(v)) for v in r] for r in hx]
        A = mp.matrix(M, M)
        g = mp.matrix(M, 1)
        for p in range(n):
            ybar = mp.fsum(H[p]) / M
            Y = [v - ybar for v in H[p]]
            r, d = mp.mpf(float(rinv[p])), mp.mpf(float(yobs[p])) - ybar
            if r == 0:
                continue
            for a in range(M):
                ry = r * Y[a]
                g[a] += ry * d
                for b in range(M):
                    A[a, b] += ry * Y[b]
        for a in range(M):
            A[a, a] += mp.mpf(M - 1) / mp.mpf(float(rho))
        lam, U = mp.eigsy(A)
        z = U.T * g
        for i in range(M):
            z[i] /= lam[i]
        wbar = U * z
        S = mp.matrix(M, M)
        for a in range(M):
            for i in range(M):
                S[a, i] = U[a, i] * mp.sqrt((M - 1) / lam[i])
        Wa = S * U.T
        T = np.zeros((M, M))
        for b in range(M):
            col = [Wa[a, b] + wbar[a] for a in range(M)]
            corr = (1 - mp.fsum(col)) / M
            for a in range(M):
                T[a, b] = float(col[a] + corr)
    return T


def closed_form(M, rho):
    s = np.sqrt(np.float64(rho))
    return s * np.eye(M) + (1.0 - s) / M


def column(case, j):
    off, hx, yobs, rinv, rho = case
    return hx[off[j]:off[j + 1]], yobs[off[j]:off[j + 1]], rinv[off[j]:off[j + 1]], 1.0 if rho is None else float(rho[j])


def solve(m, M, case):
    return m.member_transform_solve(M, *case)


# ------------------------------------------------------------------------------------------------ 1. apply == mix
def twin(m, E, rows, T, cols, bad, what):
    """apply(rows, cols) on model m against mix_cells with the lists of member_transform on the same state; returns the state
    after the apply.  m holds the transform T."""
    D = E.D
    sd0, si0 = m.get_state()
    t0 = su.full_tables(m)
    m.member_transform_apply(rows, cols)
    t1 = su.full_tables(m)
    m.set_state(sd0, si0)
    m.mix_cells(rows, *domain.member_transform(E.M, E.ncol, T, cols))
    want = m.get_state()[0]
    m.set_state(t1["sd"], si0)
    if not same_nan(want, t1["sd"]):
        with np.errstate(all="ignore"):
            n = int((~((want == t1["sd"]) | (np.isnan(want) & np.isnan(t1["sd"])))).sum())
        bad.append("%s: %d words differ from mix_cells" % (what, n))
    if same_nan(sd0, t1["sd"]):
        bad.append("%s: the call changed nothing" % what)
    bad += ["%s: %s changed" % (what, k) for k in differing(t0, t1) if k != "sd"]
    listed = np.arange(E.ncol) if cols is None else np.asarray(cols)
    hd = cu.hrus_of(D, (np.arange(E.M)[:, None] * E.ncol + listed[None, :]).reshape(-1))
    rest = np.setdiff1d(np.arange(D.nhru), hd)
    other = np.setdiff1d(np.arange(sd0.shape[0]), rows)
    if not same(sd0[:, rest], t1["sd"][:, rest]) or not same(sd0[other], t1["sd"][other]):
        bad.append("%s: unlisted SD rows or columns changed" % what)
    return t1["sd"]


def check_apply(log=print, shapes=SHAPES):
    bad = []
    for M, ncol in shapes:
        E = ens(M, ncol)
        D = E.D
        rows = cm.mix_rows(D)
        rng = np.random.default_rng(31 + M)
        T = rng.normal(size=(ncol, M, M))
        T[0, 1, 2] = 0.0                                     # a zero weight still reads its operand
        subset = rng.permutation(ncol)[:max(1, (2 * ncol) // 3)].astype(np.int32)
        if (M, ncol) == (4, 35) and (D.nhru != 924 or len(rows) != 11 or (np.diff(subset) > 0).all()):
            bad.append("the case: %d HRUs, %d rows, subset %s" % (D.nhru, len(rows), subset))
        kept = []
        for stage in ((None, "0") if M != 64 else (None,)):
            m = started(E, stage, steps=1 if M == 4 else 0)
            if M == 4:                                       # a NaN row takes part (SD_GLAC_CUM_MASS_BALANCE starts as NaN)
                if not np.isnan(m.get_state()[0][C["SD_GLAC_CUM_MASS_BALANCE"]]).any():
                    bad.append("the case: no NaN in the listed rows")
            m.member_transform_set(T)
            if not same(m.member_transform_get(), T):
                bad.append("%d x %d: get does not return what set stored" % (M, ncol))
            what = "%d x %d, stage %s" % (M, ncol, stage or "default")
            kept.append(twin(m, E, rows, T, None, bad, what + ", all columns"))
            twin(m, E, rows, T, subset, bad, what + ", %d shuffled columns" % len(subset))
            if stage is None:                                # ... and with the transform a solve leaves
                case = observations(M, ncol, 40 + M)
                info = solve(m, M, case)
                Ts = m.member_transform_get()
                if (info < 0).any() or Ts.shape != T.shape or not np.isfinite(Ts).all():
                    bad.append("%s: the solve: info %s" % (what, info))
                twin(m, E, rows, Ts, None, bad, what + ", the solved T")
                back = np.arange(ncol - 1, 0, -1, dtype=np.int32)[:max(1, ncol // 2)]      # column 0 has no information
                twin(m, E, rows[:3], Ts, back, bad, what + ", the solved T on the last columns, descending")
            m.close()
        if len(kept) == 2 and not same_nan(kept[0], kept[1]):
            bad.append("%d x %d: one row per pass gives other bits than the default budget" % (M, ncol))
    log("member transform apply: %s, differing: %s" % (", ".join("%d x %d" % s for s in shapes), bad or "none"), flush=True)
    return bad


# ------------------------------------------------------------------------------------------------ 2. accuracy of the solve
@functools.lru_cache(maxsize=None)
def yardsticks(M, ncol, seed):
    """(case, sample columns, their mpmath transforms, numpy's transforms of every column): computed once."""
    case = observations(M, ncol, seed)
    counts = np.diff(case[0])
    sample = []
    for n in (0, 1, 3, 40):                                  # of every observation count; one column at 64 members
        js = np.flatnonzero(counts == n)[1 if n == 3 else 0:]
        sample += js[:2 if M == 4 else 1].tolist()
    if M == 64:
        sample = [int(np.flatnonzero(counts == 40)[0])]
    Tmp = {j: mp_transform(M, *column(case, j)) for j in sample}
    Tnp = np.stack([np_transform(M, *column(case, j)) for j in range(ncol)])
    return case, sample, Tmp, Tnp


def check_accuracy(log=print, shapes=SHAPES):
    """max |T_dev - T_mp| <= bound on the sample, max |T_dev - T_np| <= bound on the rest, bound = 16 x max(the deviation of the
    numpy evaluation from mpmath on the sample, 64 ulp of max |T|); every column of T sums to 1 within 4 M ulp of its largest
    entry (the sum taken exactly)."""
    import math
    bad = []
    for M, ncol in shapes:
        E = ens(M, ncol)
        case, sample, Tmp, Tnp = yardsticks(M, ncol, 50 + M)
        m = started(E)
        info = solve(m, M, case)
        T = m.member_transform_get()
        m.close()
        if (info < 0).any():
            bad.append("%d members: not converged: info %s" % (M, info))
        tmax = max(np.abs(Tmp[j]).max() for j in sample)
        dev_np = max(np.abs(Tnp[j] - Tmp[j]).max() for j in sample)
        bound = 16 * max(dev_np, 64 * np.spacing(tmax))
        dev = max(np.abs(T[j] - Tmp[j]).max() for j in sample)
        rest = [j for j in range(ncol) if j not in sample]
        dev_rest = max([np.abs(T[j] - Tnp[j]).max() for j in rest] or [0.0])
        worst = 0.0
        for j in range(ncol):
            for b in range(M):
                ulps = abs(math.fsum(T[j, :, b]) - 1.0) / np.spacing(np.abs(T[j, :, b]).max())
                worst = max(worst, ulps)
        log("member transform accuracy: %d members, %d columns (%d against mpmath), sweeps %d..%d: numpy - mpmath %.3g, device - mpmath %.3g, "
            "device - numpy on the rest %.3g, bound %.3g; column sums off by at most %.1f ulp (allowed %d)"
            % (M, ncol, len(sample), info.min(), info.max(), dev_np, dev, dev_rest, bound, worst, 4 * M), flush=True)
        if not dev <= bound:
            bad.append("%d members: device - mpmath %.3g > %.3g" % (M, dev, bound))
        if not dev_rest <= bound:
            bad.append("%d members: device - numpy %.3g > %.3g" % (M, dev_rest, bound))
        if not worst <= 4 * M:
            bad.append("%d members: a column of T sums to 1 within %.1f ulp only" % (M, worst))
    return bad


# ------------------------------------------------------------------------------------------------ 3. the guarantees
def check_guarantees(log=print):
    bad = []
    M, ncol = 16, 9
    E = ens(M, ncol)
    case = observations(M, ncol, 61)
    off, hx, yobs, rinv, rho = case
    counts = np.diff(off)
    m = started(E)
    rows = cm.mix_rows(E.D)
    # (a) two runs
    info1 = solve(m, M, case); T1 = m.member_transform_get()
    info2 = solve(m, M, case); T2 = m.member_transform_get()
    if not same(T1, T2) or not same(info1, info2):
        bad.append("(a) two runs differ")
    # (b) a column alone: every other column loses its observations
    for j in (1, 4):
        keep = np.zeros(len(yobs), bool); keep[off[j]:off[j + 1]] = True
        alone = np.zeros(ncol, np.int64); alone[j] = counts[j]
        off1 = np.concatenate([[0], np.cumsum(alone)]).astype(np.int32)
        infoj = m.member_transform_solve(M, off1, hx[keep], yobs[keep], rinv[keep], rho)
        Tj = m.member_transform_get()
        if not same(Tj[j], T1[j]) or infoj[j] != info1[j]:
            bad.append("(b) column %d alone differs from the same column among others" % j)
        others = [k for k in range(ncol) if k != j]
        if not all(same(Tj[k], closed_form(M, rho[k])) for k in others):
            bad.append("(b) the emptied columns are not the closed form")
    # (c) no observation (count 0) and all rinv == 0 (column 0), rho 1 and 1.1
    quiet = [0] + np.flatnonzero(counts == 0).tolist()
    if {float(rho[j]) for j in quiet} != {1.0, 1.1} or not (rinv[off[0]:off[1]] == 0).all() or counts[0] == 0:
        bad.append("the case: the quiet columns %s, rho %s" % (quiet, rho[quiet]))
    for j in quiet:
        if not same(T1[j], closed_form(M, rho[j])) or info1[j] != 0:
            bad.append("(c) column %d is not the closed form (info %d)" % (j, info1[j]))
        if rho[j] == 1.0 and not same(T1[j], np.eye(M)):
            bad.append("(c) column %d with rho 1 is not the identity" % j)
    for infl in (None, np.ones(ncol)):
        info = m.member_transform_solve(M, np.zeros(ncol + 1, np.int32), np.zeros((0, M)), np.zeros(0), np.zeros(0), infl)
        if not same(m.member_transform_get(), np.broadcast_to(np.eye(M), (ncol, M, M))) or info.any():
            bad.append("(c) no observation at all, infl %s: not the identity" % ("NULL" if infl is None else "1"))
        before = m.get_state()[0]
        m.member_transform_apply(rows[np.isfinite(before[rows]).all(axis=1)])
        if not same(before, m.get_state()[0]):
            bad.append("(c) applying the identity changed finite rows")
    m.close()
    # (d) the sweep cap
    os.environ[SWEEPS] = "1"
    try:
        m = started(E)
    finally:
        os.environ.pop(SWEEPS, None)
    dense = np.flatnonzero(counts == 40)
    # diagonal columns in the same call: all members equal (sums of small multiples of 1/2 are exact), so Y == 0 and A is
    # diagonal although rinv > 0; they take the general path and end after a sweep that rotates nothing.  Their T is the closed
    # form up to the roundings of (M - 1) / rho, the two square roots, their product and the column sum: 64 ulp of 1 is ample
    diag = [j for j in range(1, ncol) if counts[j] in (1, 3)]
    hxd, rinvd = hx.copy(), rinv.copy()
    for j in diag:
        hxd[off[j]:off[j + 1]] = 0.5 * (1 + j)
        rinvd[off[j]:off[j + 1]] = 4.0
    info = m.member_transform_solve(M, off, hxd, yobs, rinvd, rho)
    T = m.member_transform_get()
    m.close()
    for j in dense:
        if info[j] != -1 or not same(T[j], np.eye(M)):
            bad.append("(d) the dense column %d under a cap of one sweep: info %d" % (j, info[j]))
    for j in quiet:
        if info[j] != 0 or not same(T[j], closed_form(M, rho[j])):
            bad.append("(d) the quiet column %d did not converge under the cap" % j)
    if len(diag) < 3 or not len(dense):
        bad.append("the case: diagonal columns %s, dense %s" % (diag, dense))
    for j in diag:
        if info[j] != 0 or np.abs(T[j] - closed_form(M, rho[j])).max() > 64 * np.spacing(1.0):
            bad.append("(d) the diagonal column %d: info %d" % (j, info[j]))
    log("member transform guarantees: info %s; problems: %s" % (info1.tolist(), bad or "none"), flush=True)
    return bad


# ------------------------------------------------------------------------------------------------ 4. mid-run
def check_midrun(log=print, chunks="2"):
    """The frozen pair of check_mix_cells.check_midrun: steps, apply, steps with no synchronize in between, against the same run
    with mix_cells at that point.  State, fluxes and records."""
    os.environ["VICGPU_CHUNKS"] = chunks
    try:
        E = cc.ensemble(dict(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=10, Nband=2, frozen_compat=0), 5, 2, 2, 2 + 2 * cc.R, 330, glacier=True)
        Nn = E.D.opt.Nnode
        rows = np.array([C["SD_MOIST0"], C["SD_MOIST1"], C["SD_MOIST2"], C["SD_SNOW_SWQ"]] + [abi.sd_node(C["SDN_T"], n, Nn) for n in (1, 2, 3)], np.int32)
        T = np.array([[0.7, 0.4], [0.3, 0.6]])[None] + 0.01 * np.arange(E.ncol)[:, None, None] * np.array([[1, -1], [-1, 1]])
        a, b, n = cc.model(E), cc.model(E), cc.model(E)
        a.member_transform_set(T)
        a.dist_prec(0, 2, sync=False)
        a.member_transform_apply(rows)
        ra = cc.run_records(a, 2, 2)
        b.dist_prec(0, 2, sync=False)
        b.mix_cells(rows, *domain.member_transform(E.M, E.ncol, T))
        rb = cc.run_records(b, 2, 2)
        n.dist_prec(0, 2)
        rn = cc.run_records(n, 2, 2)
        ta, tb, tn = (cc.tables(x) for x in (a, b, n))
        for x in (a, b, n):
            x.close()
        bad = ["after the steps: " + k for k in differing(tb, ta)]
        if not same(ra, rb):
            bad.append("the records after the apply")
        if same(tb["sd"], tn["sd"]) or same(rb, rn) or not np.isfinite(rb).all() or not np.isfinite(tb["cell_out"]).all():
            bad.append("the run with the transform does not differ from the run without, or is not finite")
    finally:
        os.environ.pop("VICGPU_CHUNKS", None)
    log("member transform midrun (chunks %s): %d columns, differing: %s" % (chunks, E.ncol, bad or "none"), flush=True)
    return bad


# ------------------------------------------------------------------------------------------------ 5. errors and refusals
def _lib():
    lib = load_library()
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    I = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)
    F = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    PI = lambda a: None if a is None else a.ctypes.data_as(ip)
    PF = lambda a: None if a is None else a.ctypes.data_as(dp)

    def c_solve(h, M, ncol, off, hx, yobs, rinv, infl, info=None):
        a = [I(off), F(hx), F(yobs), F(rinv), F(infl)]
        return lib.vicgpu_member_transform_solve(h, M, ncol, PI(a[0]), PF(a[1]), PF(a[2]), PF(a[3]), PF(a[4]), None if info is None else PI(info))

    def c_set(h, M, ncol, T):
        T = F(T)
        return lib.vicgpu_member_transform_set(h, M, ncol, PF(T))

    def c_get(h, sizes=True, T=None):
        M, n = ctypes.c_int(-7), ctypes.c_int(-7)
        rc = lib.vicgpu_member_transform_get(h, ctypes.byref(M) if sizes else None, ctypes.byref(n) if sizes else None, PF(T))
        return rc, M.value, n.value

    def c_apply(h, rows, cols, nrow=None, n=None):
        r, c = I(rows), I(cols)
        nrow = (len(r) if r is not None else 0) if nrow is None else nrow
        n = (len(c) if c is not None else 0) if n is None else n
        return lib.vicgpu_member_transform_apply(h, nrow, PI(r), n, PI(c))

    return lib, c_solve, c_set, c_get, c_apply


def null_handle_returns():
    """The four entries on a null handle, with arguments that are otherwise fine and with nothing to do: [(what, got, want)]."""
    _, c_solve, c_set, c_get, c_apply = _lib()
    ARG = C["VICGPU_ERR_ARG"]
    M = 2
    return [("solve, null handle", c_solve(None, M, 1, [0, 1], np.ones((1, M)), [0.0], [1.0], None), ARG),
            ("solve, null handle, no observation", c_solve(None, M, 1, [0, 0], None, None, None, None), ARG),
            ("set, null handle", c_set(None, M, 1, np.eye(M)[None]), ARG),
            ("get, null handle", c_get(None)[0], ARG),
            ("apply, null handle", c_apply(None, [0], [0]), ARG),
            ("apply, null handle, nothing to do", c_apply(None, None, None), ARG)]


def error_returns(log=print):
    """Every VICGPU_ERR_ARG / VICGPU_ERR_STATE return of the header, each followed by a comparison of all tables and of the stored
    transform; then the calls that follow work.  All of them are refused on the host before any launch."""
    lib, c_solve, c_set, c_get, c_apply = _lib()
    ARG, ST, OK = C["VICGPU_ERR_ARG"], C["VICGPU_ERR_STATE"], 0
    checks = list(null_handle_returns())
    E = cc.quickflux()
    D = E.D
    M, ncol, nsd = E.M, E.ncol, abi.sd_nrow(D.opt.Nnode)
    odd = 2 * ncol + 3               # member 2, base column 3: its second HRU gets another vegetation class
    D.hru_iparams[C["HPI_VEG_CLASS"], D.cell_hru_list[D.cell_hru_offset[odd] + 1]] += 1
    off, hx, yobs, rinv, rho = observations(M, ncol, 71)
    nobs = len(yobs)
    T0 = np.random.default_rng(72).normal(size=(ncol, M, M))
    R = [C["SD_MOIST0"], C["SD_SNOW_SWQ"]]
    fresh = ctypes.c_void_p()
    assert lib.vicgpu_create(ctypes.byref(D.opt), 0, ctypes.byref(fresh)) == 0
    checks.append(("solve, no domain", c_solve(fresh, M, ncol, off, hx, yobs, rinv, rho), ST))
    checks.append(("set, no domain", c_set(fresh, M, ncol, T0), ST))
    checks.append(("get, no domain", c_get(fresh)[0], ST))
    checks.append(("apply, no domain", c_apply(fresh, R, [0]), ST))
    checks.append(("apply, no domain, nothing to do", c_apply(fresh, None, None), ST))
    checks.append(("solve, no domain, nmember 1", c_solve(fresh, 1, ncol, off, hx, yobs, rinv, rho), ARG))
    lib.vicgpu_destroy(fresh)
    m = cc.start(Model(D), E)
    m.dist_prec(0, 1)
    checks.append(("get without a transform", c_get(m.h)[0], ST))
    checks.append(("get without a transform, sizes only", c_get(m.h, T=None)[0], ST))
    checks.append(("apply without a transform", c_apply(m.h, R, [0, 1]), ST))
    checks.append(("apply without a transform, nothing to do", c_apply(m.h, None, None), ST))
    m.member_transform_set(T0)
    t0 = su.full_tables(m)
    inf, nan = float("inf"), float("nan")

    def bent(a, i, v):
        a = np.array(a, dtype=np.float64)
        a.reshape(-1)[i] = v
        return a

    S = lambda **kw: c_solve(m.h, kw.get("M", M), kw.get("ncol", ncol), kw.get("off", off), kw.get("hx", hx), kw.get("yobs", yobs), kw.get("rinv", rinv),
                             kw.get("infl", rho))
    down = off.copy(); down[5] = down[4] - 1
    cases = [
        ("solve: nmember 1", lambda: S(M=1)),
        ("solve: nmember 65", lambda: S(M=65)),
        ("solve: nmember 0", lambda: S(M=0)),
        ("solve: ncol 0", lambda: S(ncol=0)),
        ("solve: ncol -1", lambda: S(ncol=-1)),
        ("solve: nmember * ncol != ncell", lambda: S(ncol=ncol - 1)),
        ("solve: nmember 2, ncol 2 * ncol + 1", lambda: S(M=2, ncol=2 * ncol + 1)),
        ("solve: null obs_off", lambda: S(off=None)),
        ("solve: null hx", lambda: S(hx=None)),
        ("solve: null yobs", lambda: S(yobs=None)),
        ("solve: null rinv", lambda: S(rinv=None)),
        ("solve: obs_off[0] != 0", lambda: S(off=off + 1)),
        ("solve: decreasing offsets", lambda: S(off=down)),
        ("solve: a NaN hx", lambda: S(hx=bent(hx, 5, nan))),
        ("solve: an infinite hx in the last entry", lambda: S(hx=bent(hx, hx.size - 1, inf))),
        ("solve: a NaN yobs", lambda: S(yobs=bent(yobs, 2, nan))),
        ("solve: an infinite yobs", lambda: S(yobs=bent(yobs, nobs - 1, -inf))),
        ("solve: a NaN rinv", lambda: S(rinv=bent(rinv, 0, nan))),
        ("solve: an infinite rinv", lambda: S(rinv=bent(rinv, 1, inf))),
        ("solve: rinv < 0", lambda: S(rinv=bent(rinv, nobs - 1, -1e-300))),
        ("solve: infl 0", lambda: S(infl=bent(rho, 0, 0.0))),
        ("solve: infl < 0", lambda: S(infl=bent(rho, ncol - 1, -1.0))),
        ("solve: a NaN infl", lambda: S(infl=bent(rho, 3, nan))),
        ("solve: an infinite infl", lambda: S(infl=bent(rho, 3, inf))),
        ("set: nmember 1", lambda: c_set(m.h, 1, ncol, T0)),
        ("set: nmember 65", lambda: c_set(m.h, 65, ncol, T0)),
        ("set: ncol 0", lambda: c_set(m.h, M, 0, T0)),
        ("set: nmember * ncol != ncell", lambda: c_set(m.h, M, ncol + 1, np.zeros((ncol + 1, M, M)))),
        ("set: null T", lambda: c_set(m.h, M, ncol, None)),
        ("set: a NaN weight", lambda: c_set(m.h, M, ncol, bent(T0, 7, nan))),
        ("set: an infinite weight in the last entry", lambda: c_set(m.h, M, ncol, bent(T0, T0.size - 1, inf))),
        ("apply: nrow < 0", lambda: c_apply(m.h, R, [0], nrow=-1)),
        ("apply: n < 0", lambda: c_apply(m.h, R, [0], n=-1)),
        ("apply: null rows", lambda: c_apply(m.h, None, [0], nrow=2)),
        ("apply: null cols, n != ncol", lambda: c_apply(m.h, R, None, n=ncol - 1)),
        ("apply: row == nrows", lambda: c_apply(m.h, [0, nsd], [0])),
        ("apply: row < 0", lambda: c_apply(m.h, [-1], [0])),
        ("apply: a row listed twice", lambda: c_apply(m.h, [2, 1, 2], [0])),
        ("apply: column == ncol", lambda: c_apply(m.h, R, [0, ncol])),
        ("apply: column < 0", lambda: c_apply(m.h, R, [-1])),
        ("apply: a column listed twice", lambda: c_apply(m.h, R, [4, 1, 4])),
        ("apply: a member's vegetation class differs", lambda: c_apply(m.h, R, [1, 3])),
        ("apply: ... with all columns", lambda: c_apply(m.h, R, None, n=ncol)),
    ]
    for w, f in cases:
        checks.append((w, f(), ARG))
        checks.append((w + ": tables", differing(t0, su.full_tables(m)) or "unchanged", "unchanged"))
        checks.append((w + ": the stored transform", same(m.member_transform_get(), T0), True))
    for w, f in [("apply: nrow == 0", lambda: c_apply(m.h, [], [0, 1])), ("apply: n == 0", lambda: c_apply(m.h, R, [])),
                 ("apply: nrow == 0, null lists", lambda: c_apply(m.h, None, None)), ("apply: n == 0, null cols", lambda: c_apply(m.h, R, None)),
                 ("apply: nrow == 0, lists that would be refused", lambda: c_apply(m.h, [], [4, 4]))]:
        checks.append((w, f(), OK))
    checks.append(("tables after the no-ops", differing(t0, su.full_tables(m)) or "unchanged", "unchanged"))
    checks.append(("get: sizes only", c_get(m.h), (OK, M, ncol)))
    checks.append(("get: no sizes asked", c_get(m.h, sizes=False)[0], OK))
    for w, f, words in [("the odd member", lambda: m.member_transform_apply(R, [1, 3]), ("column 3", "member 2", "vegetation")),
                        ("a row", lambda: m.member_transform_apply([1, 1]), ("listed twice",)),
                        ("an observation", lambda: m.member_transform_solve(M, off, bent(hx, M * 4 + 1, nan), yobs, rinv, rho), ("observation 4", "hx"))]:
        try:
            f()
            checks.append(("Model raises for " + w, False, True))
        except VicGpuError as e:
            checks.append(("Model names %s: %s" % (w, e), all(x in str(e) for x in words), True))
    # the calls that follow work; the odd column may be left out
    cols = [j for j in range(ncol) if j != 3]
    checks.append(("the apply that follows", c_apply(m.h, R, cols), OK))
    t1 = su.full_tables(m)
    checks.append(("... changed SD alone", differing(t0, t1), ["sd"]))
    m.set_state(t0["sd"], t0["si"])
    m.mix_cells(R, *domain.member_transform(M, ncol, T0, cols))
    checks.append(("... as mix_cells does", same_nan(m.get_state()[0], t1["sd"]), True))
    info = np.full(ncol, -9, np.int32)
    checks.append(("the solve that follows", c_solve(m.h, M, ncol, off, hx, yobs, rinv, None, info), OK))
    checks.append(("... fills info", bool((info >= 0).all()), True))
    checks.append(("... with a null info", c_solve(m.h, M, ncol, off, hx, yobs, rinv, rho), OK))
    checks.append(("... replaced the transform", same(m.member_transform_get(), T0), False))
    m.close()
    failed = [(w, got, want) for w, got, want in checks if got != want]
    for w, got, want in failed:
        log("member transform return: %s gave %s, want %s" % (w, got, want), flush=True)
    log("member transform errors: %d checks, failed: %d" % (len(checks), len(failed)), flush=True)
    return ["%s gave %s" % (w, got) for w, got, _ in failed], len(checks)


def check_refusals(log=print):
    """solve, set and apply under a runtime that refuses the n-th allocation, n = 1, 2, ...: VICGPU_ERR_HIP, no live runtime object
    added, every table and the stored transform as they were, until the call gets through -- which leaves nothing behind but,
    for solve and set, the transform that replaces the old one."""
    lib, c_solve, c_set, c_get, c_apply = _lib()
    lib.hostemu_live_objects.restype = ctypes.c_longlong
    lib.hostemu_refuse_alloc.argtypes = [ctypes.c_longlong]
    E = cc.quickflux()
    M, ncol = E.M, E.ncol
    rows = np.array([C["SD_MOIST0"], C["SD_MOIST1"], C["SD_SNOW_SWQ"]], np.int32)
    case = observations(M, ncol, 81)
    T0 = np.random.default_rng(82).normal(size=(ncol, M, M))
    bad, counts = [], {}
    m = started(E, steps=1)
    m.member_transform_set(T0)
    for name, call, changes in [("apply", lambda: c_apply(m.h, rows, np.arange(ncol)), ["sd"]), ("set", lambda: c_set(m.h, M, ncol, T0 + 1.0), []),
                                ("solve", lambda: c_solve(m.h, M, ncol, *case), [])]:
        t0, kept = su.full_tables(m), m.member_transform_get()
        before = lib.hostemu_live_objects()
        for n in range(1, 20):
            lib.hostemu_refuse_alloc(n)
            rc = call()
            lib.hostemu_refuse_alloc(0)
            if rc == 0:
                break
            if rc != C["VICGPU_ERR_HIP"] or lib.hostemu_live_objects() != before or differing(t0, su.full_tables(m)) or not same(m.member_transform_get(), kept):
                bad.append("%s, allocation %d refused: code %d, %d objects more, changed %s" % (name, n, rc, lib.hostemu_live_objects() - before,
                                                                                                differing(t0, su.full_tables(m))))
        counts[name] = n - 1
        if lib.hostemu_live_objects() != before:
            bad.append("%s: %d objects left by the call that got through" % (name, lib.hostemu_live_objects() - before))
        if differing(t0, su.full_tables(m)) != changes:
            bad.append("%s: the call that got through changed %s" % (name, differing(t0, su.full_tables(m))))
        if (name != "apply") == same(m.member_transform_get(), kept):
            bad.append("%s: the stored transform after the call that got through" % name)
    m.close()
    if counts != {"apply": 2, "set": 1, "solve": 3}:         # lists and stage; the transform; ints, observations and the transform
        bad.append("refusals %s" % counts)
    log("member transform refusals: %s refused; problems: %s" % (counts, bad or "none"), flush=True)
    return bad


# ------------------------------------------------------------------------------------------------ 6. end to end
def check_endtoend(log=print):
    """4 members x 12 columns, FULL_ENERGY + FROZEN_SOIL: steps, hx = the cells' snow water equivalent, solve, apply on the SWE and
    the three moisture rows, derive_soil_state(CAP_MOIST | NODES), more steps: no cell error flag, finite outputs, and the state
    after the apply equal to the mix_cells twin."""
    E = cc.ensemble(dict(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=10, Nband=2, frozen_compat=0), 12, 4, 2, 2 + 2 * cc.R, 330)
    D, M, ncol = E.D, E.M, E.ncol
    rows = np.array([C["SD_SNOW_SWQ"], C["SD_MOIST0"], C["SD_MOIST1"], C["SD_MOIST2"]], np.int32)
    bad = []
    m = cc.model(E)
    m.dist_prec(0, 2, sync=False)
    swq = m.get_state_rows(np.array([C["SD_SNOW_SWQ"]], np.int32))[0]
    cell = D.hru_iparams[C["HPI_CELL"]]
    per_cell = np.bincount(cell, weights=swq, minlength=D.ncell)
    hx = np.ascontiguousarray(per_cell.reshape(M, ncol).T)                       # one observation per column: [ncol][M]
    yobs = hx.mean(axis=1) * 1.1 + 0.001
    rinv = np.full(ncol, 1.0 / max(float(hx.var(axis=1).mean()), 1e-8))
    info = m.member_transform_solve(M, np.arange(ncol + 1, dtype=np.int32), hx, yobs, rinv, np.full(ncol, 1.05))
    T = m.member_transform_get()
    if (info < 0).any() or np.abs(T.sum(axis=1) - 1).max() > 1e-13 or same(T, np.broadcast_to(np.eye(M), T.shape)):
        bad.append("the solve: info %s" % info)
    twin(m, E, rows, T, None, bad, "end to end")
    try:
        m.derive_soil_state(CAP | NODES)
    except VicGpuError as e:
        bad.append("derive_soil_state: %s" % e)
    rec = cc.run_records(m, 2, 2)
    t = cc.tables(m)
    m.close()
    if t["cell_err"].any():
        bad.append("cell error flags %s" % np.unique(t["cell_err"]))
    if not np.isfinite(rec).all() or not np.isfinite(t["cell_out"]).all() or not np.isfinite(t["sd"][rows]).all():
        bad.append("outputs after the analysis are not finite")
    log("member transform endtoend: %d x %d, sweeps %s; problems: %s" % (M, ncol, info.tolist(), bad or "none"), flush=True)
    return bad


if __name__ == "__main__":
    cmd = sys.argv[1]
    if cmd == "errors":
        problems, _ = error_returns()
    else:
        both_chunkings = lambda: check_midrun(chunks="1") + check_midrun(chunks="2")
        problems = {"apply": check_apply, "accuracy": check_accuracy, "guarantees": check_guarantees, "midrun": both_chunkings,
                    "refusals": check_refusals, "endtoend": check_endtoend}[cmd]()
    print("member transform %s: problems: %s" % (cmd, problems or "none"), flush=True)
    sys.exit(1 if problems else 0)
