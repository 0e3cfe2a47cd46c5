"""Raw forcing expanded and perturbed per column on the device (vicgpu_prefetch_forcing_perturbed, include/vicgpu.h).  The
reference side of every comparison is never the entry under test: it is the same library's vicgpu_prefetch_forcing_raw, fed the
ncol-wide table numpy builds as raw[..., col_src] * mul[..., col_group] + add[..., col_group] (two roundings, like the
contract), and the oracle's derivation of that table where the oracle is built.  Run by tests/test_forcing_perturb.py with
VICGPU_LIB pointing at the unsanitized host build (SAN=none tools/hostemu/build.sh); tests/test_forcing_perturb_gpu.py calls
the same functions on a GPU.
    python tools/hostemu/check_forcing_perturb.py table <nsrc> <M>     the derived table bit for bit: member-major, scrambled and
                                                                        group-per-column lists, the oracle, no perturbation
    python tools/hostemu/check_forcing_perturb.py mapped                with a forcing map in force: cells -> 60 columns -> 20 sources
    python tools/hostemu/check_forcing_perturb.py run <shape> <nsrc> <M>    daily | hourly: steps through both entries
    python tools/hostemu/check_forcing_perturb.py stream <nsrc> <M>     chunks prefetched behind the steps, entry kinds alternating
    python tools/hostemu/check_forcing_perturb.py group <nsrc> <M> <nshard>
    python tools/hostemu/check_forcing_perturb.py errors                every error return of the contract
    python tools/hostemu/check_forcing_perturb.py refusals              the n-th allocation refused, for every n (host build only)"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import check_forcing_map as cfm
from vic_amd import abi, domain, init_state
from vic_amd.abi import C
from vic_amd.api import Group, Model, load_library

SEED = 20261020
MIN_WIND = 0.4
NPERT = C["VICGPU_NPERT"]
RAWV = ("VIC_RAW_AIR_TEMP", "VIC_RAW_PREC", "VIC_RAW_PRESSURE_KPA", "VIC_RAW_VP_KPA", "VIC_RAW_SHORTWAVE", "VIC_RAW_LONGWAVE", "VIC_RAW_WIND")
SHAPES = {
    # name: options, tiles, start day, steps.  daily: NF = 8, so the NR slot and the sub-step stride; hourly: NF = 1, NR = 0
    "daily": (dict(FULL_ENERGY=0, dt=24, snow_step=3), 2, 60, 3),
    "hourly": (dict(FULL_ENERGY=1, Nband=3), 2, 100, 4),
}


# ------------------------------------------------------------------------------------------------ cases
def raw_of(opt, f, seed=3):
    """Hourly raw forcing whose T and prec are the synthetic derived table's (check_forcing_map.raw_case's construction): some
    vapour pressures above saturation, some winds below the floor."""
    rng = np.random.default_rng(seed)
    n, ncol = f.shape[0], f.shape[-1]
    raw = np.zeros((n, C["VIC_NRAW"], opt.dt, ncol))
    hours = lambda v: np.repeat(f[:, C[v], :opt.NF], opt.snow_step, axis=1)
    raw[:, C["VIC_RAW_AIR_TEMP"]] = hours("VIC_F_AIR_TEMP")
    raw[:, C["VIC_RAW_PREC"]] = hours("VIC_F_PREC") / opt.snow_step
    raw[:, C["VIC_RAW_PRESSURE_KPA"]] = hours("VIC_F_PRESSURE") * 1e-3
    raw[:, C["VIC_RAW_VP_KPA"]] = hours("VIC_F_VP") * 1e-3 * rng.uniform(0.5, 1.6, raw[:, 0].shape)
    raw[:, C["VIC_RAW_SHORTWAVE"]] = hours("VIC_F_SHORTWAVE"); raw[:, C["VIC_RAW_LONGWAVE"]] = hours("VIC_F_LONGWAVE")
    raw[:, C["VIC_RAW_WIND"]] = hours("VIC_F_WIND") * rng.uniform(0.0, 1.2, raw[:, 0].shape)
    return raw


def case(shape, nsrc, M):
    """(D, raw [..][nsrc], f [..][nsrc] the unperturbed derived table, dmy): M members of identical parameters on nsrc source
    columns, member-major, so whatever splits the members comes from the perturbation alone.  The daily shape is
    check_forcing_map.raw_case's: dt = 24, snow_step = 3, 3 steps from day 60."""
    kw, ntile, doy, nsteps = SHAPES[shape]
    os.environ.pop("VICGPU_CHUNKS", None)
    opt = abi.default_options(**kw)
    base = domain.make_domain(nsrc, opt, ntile=ntile)
    f, _, dmy = domain.make_forcing(base, 0, nsteps, start_doy=doy)
    if shape == "daily":
        D1, _, raw, dmy, _ = cfm.raw_case(nsrc, 1)       # member 0 of its ensemble: MAX_SNOW_TEMP 0.5
        D, _ = domain.tile_members(D1, M)
    else:
        raw = raw_of(opt, f)
        D, _ = domain.tile_members(base, M)
    return D, raw, f, dmy


def noise(nsteps, ngroup, seed=SEED):
    """pert [nsteps][VICGPU_NPERT][ngroup]: exp(N(0, 0.5)) on precipitation, N(0, 2 K) on air temperature, and every other
    variable perturbed too (vapour pressure up to 30 % up, so that some vpd is clipped that was not; wind down to 20 %, so that
    more winds are floored); group 1 has a precipitation multiplier of exactly 0 in step 1."""
    rng = np.random.default_rng(seed)
    p = np.zeros((nsteps, NPERT, ngroup))
    p[:, 0::2] = 1.0
    mul = lambda v: p[:, abi.pert_mul(C[v])]
    add = lambda v: p[:, abi.pert_add(C[v])]
    mul("VIC_RAW_PREC")[:] = np.exp(rng.normal(0.0, 0.5, (nsteps, ngroup)))
    add("VIC_RAW_AIR_TEMP")[:] = rng.normal(0.0, 2.0, (nsteps, ngroup))
    mul("VIC_RAW_SHORTWAVE")[:] = np.exp(rng.normal(0.0, 0.2, (nsteps, ngroup)))
    add("VIC_RAW_LONGWAVE")[:] = rng.normal(0.0, 10.0, (nsteps, ngroup))
    mul("VIC_RAW_VP_KPA")[:] = rng.uniform(0.9, 1.3, (nsteps, ngroup))
    add("VIC_RAW_PRESSURE_KPA")[:] = rng.normal(0.0, 0.5, (nsteps, ngroup))
    mul("VIC_RAW_WIND")[:] = rng.uniform(0.2, 1.2, (nsteps, ngroup))
    add("VIC_RAW_WIND")[:] = rng.normal(0.0, 0.05, (nsteps, ngroup))
    if ngroup > 1 and nsteps > 1:
        mul("VIC_RAW_PREC")[1, 1] = 0.0
    return np.ascontiguousarray(p)


def lists(kind, ncol, nsrc, ngroup, seed=SEED):
    """(col_src, col_group) [ncol].  member-major: tile / repeat.  scrambled: a fixed-seed random assignment with repeats, source
    nsrc // 2 and group ngroup // 2 used by nobody.  blocked: consecutive columns share a source, as on a grid finer than its
    forcing grid -- a shard's source range then starts past source 0."""
    M = ncol // nsrc
    if kind == "member-major":
        return (np.ascontiguousarray(np.tile(np.arange(nsrc, dtype=np.int32), M)),
                np.ascontiguousarray(np.repeat(np.arange(ngroup, dtype=np.int32), ncol // ngroup)))
    rng = np.random.default_rng(seed + 1)
    used = np.array([g for g in range(ngroup) if g != ngroup // 2], dtype=np.int32)
    grp = used[rng.integers(0, len(used), ncol)]
    if kind == "blocked":
        src = (np.arange(ncol) * nsrc // ncol).astype(np.int32)
    else:
        free = nsrc // 2
        useds = np.array([c for c in range(nsrc) if c != free], dtype=np.int32)
        src = useds[rng.integers(0, len(useds), ncol)]
        assert len(np.unique(src)) < ncol and free not in src
    assert ngroup // 2 not in grp
    return np.ascontiguousarray(src), np.ascontiguousarray(grp)


def expand(raw, col_src, col_group, pert):
    """numpy's ncol-wide table of the x' = (x * mul) + add, each operation rounded once; pert None: the values verbatim."""
    ncol = len(col_src) if col_src is not None else raw.shape[-1]
    x = raw if col_src is None else raw[..., col_src]
    if pert is None:
        return np.ascontiguousarray(x)
    g = np.arange(ncol) if col_group is None else col_group
    mul = pert[:, 0::2][:, :, None, :][..., g]
    add = pert[:, 1::2][:, :, None, :][..., g]
    prod = x * mul
    return np.ascontiguousarray(prod + add)


def derived(m, nsteps):
    fs = [m.get_forcing(s) for s in range(nsteps)]
    return np.stack([x[0] for x in fs]), np.stack([x[1] for x in fs])


def stage_both(D, raw, dmy, col_src, col_group, pert, cell_col=None, ncol=None):
    """((F, S) of vicgpu_prefetch_forcing_raw on numpy's table, (F, S) of the entry under test, numpy's table)."""
    xp = expand(raw, col_src, col_group, pert)
    out = []
    for new in (False, True):
        m = Model(D)
        if cell_col is not None:
            m.set_forcing_map(cell_col, ncol)
        if new:
            m.prefetch_forcing_perturbed(raw, dmy, col_src, col_group, pert, min_wind_speed=MIN_WIND, plapse=True)
        else:
            m.prefetch_forcing_raw(xp, dmy, min_wind_speed=MIN_WIND, plapse=True)
        m.swap_forcing()
        out.append(derived(m, raw.shape[0]))
        m.close()
    return out[0], out[1], xp


def same_table(what, ref, got, bad):
    if ref[0].shape != got[0].shape or not np.array_equal(ref[0], got[0]):
        bad.append("%s: derived rows differ from the replicated call's" % what)
    if not np.array_equal(ref[1], got[1]):
        bad.append("%s: flags differ from the replicated call's" % what)


EXACT = ("VIC_F_AIR_TEMP", "VIC_F_PREC", "VIC_F_PRESSURE", "VIC_F_DENSITY", "VIC_F_SHORTWAVE", "VIC_F_LONGWAVE", "VIC_F_WIND")


def against_oracle(what, oracle, D, xp, sides, bad):
    """Both sides against the oracle's derivation of numpy's table: the flags and the seven rows without a transcendental exactly,
    vp / vpd to the 1e-11 relative (floor 1e-6) of check_forcing_map.run_raw."""
    fo, so = oracle.OracleModel(D).derive_forcing(xp, min_wind=MIN_WIND, plapse=1)
    exact = [C[v] for v in EXACT]
    for side, (F, S) in sides:
        if not np.array_equal(so, S):
            bad.append("%s, %s: flags differ from the oracle's" % (what, side))
        if not np.array_equal(fo[:, exact], F[:, exact]):
            bad.append("%s, %s: rows differ from the oracle's" % (what, side))
        rel = np.abs(fo - F) / np.maximum(np.maximum(np.abs(fo), np.abs(F)), 1e-6)
        if not rel.max() < 1e-11:
            bad.append("%s, %s: vp / vpd off the oracle's by %.3g" % (what, side, rel.max()))


# ------------------------------------------------------------------------------------------------ comparisons
def run_table(nsrc, M, oracle=None):
    """Comparisons 1 and 2.  Returns (problems, facts): facts counts what keeps the case from passing empty."""
    D, raw, f, dmy = case("daily", nsrc, M)
    nsteps, ncol = raw.shape[0], D.ncell
    bad, facts = [], {}
    rawM = np.ascontiguousarray(np.tile(raw, (1, 1, 1, M)))
    plain = None
    for kind in ("member-major", "scrambled", "per-column"):
        ngroup = ncol if kind == "per-column" else M + 1 if kind == "scrambled" else M
        src, grp = lists("scrambled" if kind == "scrambled" else "member-major", ncol, nsrc, M + 1 if kind == "scrambled" else M)
        if kind == "per-column":
            grp = None
        pert = noise(nsteps, ngroup)
        ref, got, xp = stage_both(D, raw, dmy, src, grp, pert)
        same_table(kind, ref, got, bad)
        if oracle is not None:
            against_oracle(kind, oracle, D, xp, (("replicated", ref), ("perturbed", got)), bad)
        if kind == "member-major":
            # the unperturbed table of the same columns, through the reference side only
            m = Model(D); m.prefetch_forcing_raw(rawM, dmy, min_wind_speed=MIN_WIND, plapse=True); m.swap_forcing()
            plain = derived(m, nsteps); m.close()
            S = ref[1].reshape(nsteps, D.opt.NR + 1, M, nsrc)
            facts["flags_split"] = int((S.max(axis=2) != S.min(axis=2)).sum())          # members of identical parameters apart
            facts["flags"] = int(S[:, :, 0].size)
            vpd, vpd0 = ref[0][:, C["VIC_F_VPD"]], plain[0][:, C["VIC_F_VPD"]]
            facts["vpd_newly_clipped"] = int(((vpd == 0) & (vpd0 > 0)).sum())
            facts["wind_floored"] = int((xp[:, C["VIC_RAW_WIND"]] < MIN_WIND).sum())
            facts["wind_floored_unperturbed"] = int((rawM[:, C["VIC_RAW_WIND"]] < MIN_WIND).sum())
            facts["prec_mul_zero"] = int((pert[:, abi.pert_mul(C["VIC_RAW_PREC"])] == 0.0).sum())
            facts["oracle"] = oracle is not None
    # comparison 2: no perturbation
    src, grp = lists("member-major", ncol, nsrc, M)
    m = Model(D); m.prefetch_forcing_perturbed(raw, dmy, src, None, None, min_wind_speed=MIN_WIND, plapse=True); m.swap_forcing()
    same_table("pert NULL, member-major col_src", plain, derived(m, nsteps), bad); m.close()
    m = Model(D); m.prefetch_forcing_perturbed(rawM, dmy, None, None, None, min_wind_speed=MIN_WIND, plapse=True); m.swap_forcing()
    same_table("both lists NULL", plain, derived(m, nsteps), bad); m.close()
    ident = np.zeros((nsteps, NPERT, M)); ident[:, 0::2] = 1.0
    for what, r in (("identity pert", raw), ("identity pert, no negative zero", np.abs(raw) * np.where(raw < 0, -1.0, 1.0) + 0.0)):
        rM = np.ascontiguousarray(np.tile(r, (1, 1, 1, M)))
        a = Model(D); a.prefetch_forcing_raw(rM, dmy, min_wind_speed=MIN_WIND, plapse=True); a.swap_forcing()
        want = derived(a, nsteps); a.close()
        b = Model(D); b.prefetch_forcing_perturbed(r, dmy, src, grp, ident, min_wind_speed=MIN_WIND, plapse=True); b.swap_forcing()
        got = derived(b, nsteps); b.close()
        if what == "identity pert":
            if not ((want[0] == got[0]).all() and (want[1] == got[1]).all()):
                bad.append("identity pert: not equal under ==")
        else:
            assert not np.signbit(r[r == 0]).any()
            same_table(what, want, got, bad)
    return bad, facts


def facts_missing(facts):
    """The conditions that keep comparison 1 from passing empty."""
    miss = []
    if facts["flags_split"] < 1:
        miss.append("no flag differs between members of identical parameters")
    if facts["vpd_newly_clipped"] < 1:
        miss.append("no vpd is clipped on the perturbed table where the unperturbed one is not")
    if facts["wind_floored"] < 1:
        miss.append("no wind is floored")
    if facts["prec_mul_zero"] < 1:
        miss.append("no precipitation multiplier of exactly 0")
    return miss


def run_mapped(oracle=None):
    """Comparison 3: 120 cells -> 60 forcing columns (a scrambled forcing map) -> 20 sources, 2 groups.  The members' parameters
    differ (check_forcing_map.perturb), so the flags are per cell."""
    nsrc, M, ncol = 20, 6, 60
    D1, raw, f, dmy = case("daily", nsrc, 1)
    D, _ = domain.tile_members(D1, M)
    cfm.perturb(D, nsrc, M)
    cell_col = cfm.scrambled_map(D.ncell, ncol)
    src, grp = lists("scrambled", ncol, nsrc, 3)          # groups 0 and 2 used, group 1 not
    pert = noise(raw.shape[0], 3)
    ref, got, xp = stage_both(D, raw, dmy, src, grp, pert, cell_col, ncol)
    bad = []
    if got[0].shape != (raw.shape[0], C["VIC_NFORCE"], D.opt.NR + 1, ncol):
        bad.append("shape of the mapped table %s" % (got[0].shape,))
    same_table("mapped", ref, got, bad)
    if oracle is not None:      # the oracle derives per cell: its table is numpy's, gathered through the map
        xc = np.ascontiguousarray(xp[..., cell_col])
        sides = [(w, (np.ascontiguousarray(F[..., cell_col]), S)) for w, (F, S) in (("replicated", ref), ("perturbed", got))]
        against_oracle("mapped", oracle, D, xc, sides, bad)
    split = cfm.flags_split(got[1], cell_col, ncol)
    return bad, split


def start(m, D, f0, R):
    sd0, si0 = init_state.initial_state(D, f0)
    m.set_state(sd0, si0)
    m.put_data_config(R)
    m.put_data_init()
    return m


def steps(m, n):
    m.dist_prec(0, 1)
    if n > 1:
        m.dist_prec(1, n - 1)


def run_steps(shape, nsrc, M):
    """Comparison 4: every table a run leaves, through the new entry and through the replicated call."""
    D, raw, f, dmy = case(shape, nsrc, M)
    n, ncol = raw.shape[0], D.ncell
    src, grp = lists("member-major", ncol, nsrc, M)
    pert = noise(n, M)
    xp = expand(raw, src, grp, pert)
    f0 = np.ascontiguousarray(np.tile(f[0], (1, 1, M)))
    a = start(Model(D), D, f0, n)
    a.prefetch_forcing_raw(xp, dmy, min_wind_speed=MIN_WIND, plapse=True); a.swap_forcing()
    steps(a, n)
    want = cfm.tables(a, n); a.close()
    b = start(Model(D), D, f0, n)
    b.prefetch_forcing_perturbed(raw, dmy, src, grp, pert, min_wind_speed=MIN_WIND, plapse=True); b.swap_forcing()
    steps(b, n)
    got = cfm.tables(b, n); b.close()
    bad = cfm.differing(want, got)
    members_differ = not np.array_equal(want["accum"][:, :nsrc], want["accum"][:, nsrc:2 * nsrc])
    ok = not want["errors"].any() and bool(np.isfinite(want["out_agg"]).all()) and bool(want["out_agg"].any())
    return bad, members_differ, ok


def run_stream(nsrc, M):
    """Comparison 5: three one-step chunks with prefetch(k + 1) issued before step(k) against one chunk of all three, every chunk
    by the new entry ("nnn") and with vicgpu_prefetch_forcing_raw taking some of them, so that a slot's buffers pass from one
    entry kind to the other and back (a slot takes every second chunk)."""
    D, raw, f, dmy = case("daily", nsrc, M)
    n, ncol = raw.shape[0], D.ncell
    src, grp = lists("member-major", ncol, nsrc, M)
    pert = noise(n, M)
    xp = expand(raw, src, grp, pert)
    f0 = np.ascontiguousarray(np.tile(f[0], (1, 1, M)))
    one = start(Model(D), D, f0, n)
    one.prefetch_forcing_perturbed(raw, dmy, src, grp, pert, min_wind_speed=MIN_WIND, plapse=True); one.swap_forcing()
    one.dist_prec(0, n)
    want = cfm.tables(one, n); one.close()
    wf, ws = want.pop("forcing"), want.pop("snowflag")
    bad = []
    for pattern in ("nnn", "nrr", "rnn", "rnr"):
        m = start(Model(D), D, f0, n)

        def prefetch(k):
            s = slice(k, k + 1)
            if pattern[k] == "n":
                m.prefetch_forcing_perturbed(raw[s], dmy[s], src, grp, pert[s], min_wind_speed=MIN_WIND, plapse=True)
            else:
                m.prefetch_forcing_raw(xp[s], dmy[s], min_wind_speed=MIN_WIND, plapse=True)
        prefetch(0); m.swap_forcing()
        for k in range(n):
            if k + 1 < n:
                prefetch(k + 1)
            m.dist_prec(0, 1, sync=False)
            if k + 1 < n:
                m.swap_forcing()
        m.synchronize()
        got = cfm.tables(m, 1); m.close()
        gf, gs = got.pop("forcing"), got.pop("snowflag")
        d = cfm.differing(want, got)
        if not (np.array_equal(gf[0], wf[n - 1]) and np.array_equal(gs[0], ws[n - 1])):
            d.append("last chunk's forcing")
        if d:
            bad.append("%s: %s" % (pattern, d))
    ok = not want["errors"].any() and bool(want["out_agg"].any())
    return bad, ok


def run_group(nsrc, M, devices, kind):
    """Comparison 6: a group of len(devices) shards against one context, both through the new entry; the group reads its raw
    table straight from pinned memory (the pitched copies of a shard's source range)."""
    D, raw, f, dmy = case("hourly", nsrc, M)
    n, ncol = raw.shape[0], D.ncell
    src, grp = lists(kind, ncol, nsrc, M + 1 if kind != "member-major" else M)
    pert = noise(n, M + 1 if kind != "member-major" else M)
    fc = expand(f[:1], src, None, None)[0]           # every column starts from its source's unperturbed forcing
    one = start(Model(D), D, fc, n)
    one.prefetch_forcing_perturbed(raw, dmy, src, grp, pert, min_wind_speed=MIN_WIND, plapse=True); one.swap_forcing()
    steps(one, n)
    want = cfm.tables(one, n); one.close()
    g = start(Group(D, devices=devices), D, fc, n)
    bounds = g.shard_bounds()
    rp = g.pinned(raw.shape); rp[:] = raw
    g.prefetch_forcing_perturbed(rp, dmy, src, grp, pert, min_wind_speed=MIN_WIND, plapse=True); g.swap_forcing()
    steps(g, n)
    got = cfm.tables(g, n); g.close()
    return [k for k in got if not np.array_equal(want[k], got[k], equal_nan=True)], bounds


def errors():
    """Comparison 7: every VICGPU_ERR_ARG / VICGPU_ERR_STATE of the contract; after them the current and the staged chunk are
    what they were -- the steps give the results of a model that never saw a refused call."""
    lib = load_library()
    ARG, STATE, OK = C["VICGPU_ERR_ARG"], C["VICGPU_ERR_STATE"], 0
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    checks = []
    want = lambda what, got, code: checks.append((what, got, code))
    nsrc, M = 5, 3
    D, raw, f, dmy = case("daily", nsrc, M)
    n, ncol = raw.shape[0], D.ncell
    src, grp = lists("member-major", ncol, nsrc, M)
    pert = noise(n, M)
    I = lambda a: None if a is None else a.ctypes.data_as(ip)
    Dd = lambda a: None if a is None else a.ctypes.data_as(dp)

    def call(h, fn=lib.vicgpu_prefetch_forcing_perturbed, nsteps=n, ns=nsrc, r=raw, s=src, ng=M, g=grp, p=pert, d=dmy):
        return fn(h, nsteps, ns, Dd(r), I(s), ng, I(g), Dd(p), I(d), MIN_WIND, 1)
    for name, fn in (("ctx", lib.vicgpu_prefetch_forcing_perturbed), ("group", lib.vicgpu_group_prefetch_forcing_perturbed)):
        want(name + ": null handle", call(None, fn), ARG)
    h = ctypes.c_void_p()
    want("create", lib.vicgpu_create(ctypes.byref(D.opt), 0, ctypes.byref(h)), OK)
    want("before a domain", call(h), STATE)
    lib.vicgpu_destroy(h)
    f0 = np.ascontiguousarray(np.tile(f[0], (1, 1, M)))
    ref = start(Model(D), D, f0, n)
    m = start(Model(D), D, f0, n)
    for x in (ref, m):
        x.prefetch_forcing_perturbed(raw, dmy, src, grp, pert, min_wind_speed=MIN_WIND, plapse=True); x.swap_forcing()
        x.prefetch_forcing_perturbed(raw[1:], dmy[1:], src, grp, pert[1:], min_wind_speed=MIN_WIND, plapse=True)      # staged
    badm = dmy.copy(); badm[1, C["VIC_DMY_MONTH"]] = 13
    hi = src.copy(); hi[7] = nsrc
    lo = src.copy(); lo[0] = -1
    ghi = grp.copy(); ghi[-1] = M
    glo = grp.copy(); glo[3] = -1
    pnan = pert.copy(); pnan[2, 5, 1] = np.nan
    pinf = pert.copy(); pinf[0, 0, 0] = np.inf
    wide = np.ascontiguousarray(np.tile(raw, (1, 1, 1, M)))
    percol = noise(n, ncol)

    def refused():
        yield "null raw", call(m.h, r=None)
        yield "null dmy", call(m.h, d=None)
        yield "nsteps 0", call(m.h, nsteps=0)
        yield "nsteps < 0", call(m.h, nsteps=-2)
        yield "nsrc 0", call(m.h, ns=0)
        yield "month 13", call(m.h, d=badm)
        yield "col_src NULL with nsrc != ncol", call(m.h, s=None)
        yield "col_src entry == nsrc", call(m.h, s=hi)
        yield "negative col_src entry", call(m.h, s=lo)
        yield "ngroup < 0", call(m.h, ng=-1)
        yield "ngroup > 0 with pert NULL", call(m.h, p=None)
        yield "pert with ngroup 0", call(m.h, ng=0, g=None)
        yield "col_group NULL with ngroup neither 0 nor ncol", call(m.h, g=None)
        yield "col_group entry == ngroup", call(m.h, g=ghi)
        yield "negative col_group entry", call(m.h, g=glo)
        yield "col_group with ngroup 0", call(m.h, ng=0, p=None)
        yield "NaN in pert", call(m.h, p=pnan)
    for what, rc in refused():
        want(what, rc, ARG)
    msg = lib.vicgpu_last_error(m.h).decode()
    want("last_error names step 2, row 5, group 1 (%s)" % msg, int("step 2" in msg and "row 5" in msg and "group 1" in msg), 1)
    want("infinity in pert", call(m.h, p=pinf), ARG)
    msg = lib.vicgpu_last_error(m.h).decode()
    want("last_error names step 0, row 0, group 0 (%s)" % msg, int("step 0" in msg and "row 0" in msg and "group 0" in msg), 1)
    # the current chunk, then the staged one, are what they were
    for x in (ref, m):
        x.dist_prec(0, 1)
    for what, rc in refused():
        want(what + " (again)", rc, ARG)
    for x in (ref, m):
        x.swap_forcing(); x.dist_prec(0, 2)
    d = cfm.differing(cfm.tables(ref, 2), cfm.tables(m, 2))
    want("tables after the refused calls differ in %s" % d, len(d), 0)
    # legal edge forms
    want("both lists NULL, nsrc == ncol", call(m.h, ns=ncol, r=wide, s=None, ng=0, g=None, p=None), OK)
    want("a group per column", call(m.h, ng=ncol, g=None, p=percol), OK)
    want("col_src only", call(m.h, ng=0, g=None, p=None), OK)
    want("swap", lib.vicgpu_swap_forcing(m.h), OK)
    want("step", lib.vicgpu_step(m.h, 0, 1), OK)
    want("synchronize", lib.vicgpu_synchronize(m.h), OK)
    ref.close(); m.close()
    # the group: checked on the whole domain before any shard uploads
    g = Group(D, devices=[0, 0])
    gcall = lambda **kw: call(g.h, lib.vicgpu_group_prefetch_forcing_perturbed, **kw)
    want("group: null raw", gcall(r=None), ARG)
    want("group: col_src entry == nsrc", gcall(s=hi), ARG)
    want("group: col_group entry == ngroup", gcall(g=ghi), ARG)
    want("group: NaN in pert", gcall(p=pnan), ARG)
    gmsg = lib.vicgpu_group_last_error(g.h).decode()
    want("group: last_error names the entry (%s)" % gmsg, int("step 2" in gmsg and "row 5" in gmsg and "group 1" in gmsg), 1)
    want("group: month 13", gcall(d=badm), ARG)
    want("group: step before a chunk", lib.vicgpu_group_step(g.h, 0, 1), STATE)
    want("group: the call", gcall(), OK)
    want("group: swap", lib.vicgpu_group_swap_forcing(g.h), OK)
    g.close()
    failed = [(w, got, c) for w, got, c in checks if got != c]
    for w, got, c in failed:
        print("forcing perturb error return: %s gave %d, want %d" % (w, got, c), flush=True)
    print("hostemu forcing perturb errors: %d checks, failed: %d" % (len(checks), len(failed)), flush=True)
    return 1 if failed else 0


def refusals():
    """Comparison 8: vicgpu_prefetch_forcing_perturbed with the n-th allocation refused (hostemu_refuse_alloc), n = 1, 2, ...:
    VICGPU_ERR_HIP and the count of live runtime objects where it was, until the call gets through -- first into an empty slot,
    then with a chunk current and the slot's buffers too small (a longer chunk); the chunk in force stays usable."""
    lib = load_library()
    lib.hostemu_live_objects.restype = ctypes.c_longlong
    lib.hostemu_refuse_alloc.argtypes = [ctypes.c_longlong]
    live0 = lib.hostemu_live_objects()
    nsrc, M = 5, 3
    D, raw, f, dmy = case("daily", nsrc, M)
    n, ncol = raw.shape[0], D.ncell
    src, grp = lists("member-major", ncol, nsrc, M)
    pert = noise(n, M)
    f0 = np.ascontiguousarray(np.tile(f[0], (1, 1, M)))
    ref = start(Model(D), D, f0, n)
    m = start(Model(D), D, f0, n)
    bad, counts = [], []

    def through(what, lo, hi):
        before = lib.hostemu_live_objects()
        for k in range(1, 30):
            lib.hostemu_refuse_alloc(k)
            try:
                m.prefetch_forcing_perturbed(raw[lo:hi], dmy[lo:hi], src, grp, pert[lo:hi], min_wind_speed=MIN_WIND, plapse=True)
                rc = 0
            except Exception as e:
                rc = C["VICGPU_ERR_HIP"] if "(%d)" % C["VICGPU_ERR_HIP"] in str(e) else -99
            finally:
                lib.hostemu_refuse_alloc(0)
            if rc == 0:
                counts.append((k - 1, lib.hostemu_live_objects() - before))
                return
            if rc != C["VICGPU_ERR_HIP"] or lib.hostemu_live_objects() != before:
                bad.append("%s, allocation %d refused: code %d, %d objects more" % (what, k, rc, lib.hostemu_live_objects() - before))
        bad.append("%s: still refused at allocation 30" % what)
    through("empty slot", 0, 1)
    ref.prefetch_forcing_perturbed(raw[0:1], dmy[0:1], src, grp, pert[0:1], min_wind_speed=MIN_WIND, plapse=True)
    for x in (ref, m):
        x.swap_forcing(); x.dist_prec(0, 1)
    through("other slot", 1, 2)            # refused calls with a chunk current: it stays usable
    ref.prefetch_forcing_perturbed(raw[1:2], dmy[1:2], src, grp, pert[1:2], min_wind_speed=MIN_WIND, plapse=True)
    for x in (ref, m):
        x.swap_forcing(); x.dist_prec(0, 1)
    through("first slot again, two steps where it holds one", 1, 3)      # every buffer that depends on nsteps grows
    ref.prefetch_forcing_perturbed(raw[1:3], dmy[1:3], src, grp, pert[1:3], min_wind_speed=MIN_WIND, plapse=True)
    for x in (ref, m):
        x.dist_prec(0, 1)                  # still the old chunk
        x.swap_forcing(); x.dist_prec(1, 1)
    d = cfm.differing(cfm.tables(ref, 2), cfm.tables(m, 2))
    if d:
        bad.append("tables differ from a model that saw no refusal: %s" % d)
    if counts != [(7, 7), (7, 7), (5, 0)]:      # rows, flags, raw, factors, two lists, staging; the lists do not depend on nsteps
        bad.append("refusals and objects owned per call: %s" % counts)
    ref.close(); m.close()
    left = lib.hostemu_live_objects() - live0
    if left:
        bad.append("%d objects left after close" % left)
    print("hostemu forcing perturb refusals: %s refused / owned; problems: %s" % (counts, bad or "none"), flush=True)
    return 1 if bad else 0


def main(argv):
    cmd = argv[0]
    from oracle import pyref
    oracle = pyref if pyref.have_oracle() else None
    if cmd == "table":
        bad, facts = run_table(int(argv[1]), int(argv[2]), oracle)
        miss = facts_missing(facts)
        print("forcing perturb table: %s; missing: %s; problems: %s" % (facts, miss or "none", bad or "none"), flush=True)
        return 1 if bad or miss else 0
    if cmd == "mapped":
        bad, split = run_mapped(oracle)
        print("forcing perturb mapped: flags apart within a column: %d, oracle: %s, problems: %s" % (split, oracle is not None, bad or "none"), flush=True)
        return 1 if bad else 0
    if cmd == "run":
        bad, members_differ, ok = run_steps(argv[1], int(argv[2]), int(argv[3]))
        print("forcing perturb run %s: members differ: %s, clean run: %s, differing: %s" % (argv[1], members_differ, ok, bad or "none"), flush=True)
        return 1 if bad or not members_differ or not ok else 0
    if cmd == "stream":
        bad, ok = run_stream(int(argv[1]), int(argv[2]))
        print("forcing perturb stream: clean run: %s, differing: %s" % (ok, bad or "none"), flush=True)
        return 1 if bad or not ok else 0
    if cmd == "group":
        nsrc, M, ns = int(argv[1]), int(argv[2]), int(argv[3])
        rc = 0
        for kind in ("member-major", "scrambled", "blocked"):
            bad, bounds = run_group(nsrc, M, [0] * ns, kind)
            print("forcing perturb group %s lists: shards at %s, differing: %s" % (kind, bounds.tolist(), bad or "none"), flush=True)
            if bad:
                rc = 1
        return rc
    return {"errors": errors, "refusals": refusals}[cmd]()


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
