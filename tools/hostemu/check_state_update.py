"""Model state read and changed in place and its dependent soil rows re-derived (vicgpu_get_state_rows / vicgpu_update_state /
vicgpu_derive_soil_state, the int forms and the group forms, include/vicgpu.h).  The derive is pinned to the reference's own
tables (tests/golden/*.npz: the state after initialize_model_state and the stepped states) and to the numpy restatement
(vic_amd/init_state.py, np_derive below) at a tolerance the caller passes; gather, scatter, the moisture cap, ordering, the
untouched tables and the group are compared bit for bit.  Run by tests/test_state_update.py with VICGPU_LIB pointing at the
unsanitized host build (SAN=none tools/hostemu/build.sh); tests/test_state_update_gpu.py imports the functions for the GPU.
    python tools/hostemu/check_state_update.py initial       derive(NODES | LAYERS | FRONTS) against sd0 / si0 of every fixture
    python tools/hostemu/check_state_update.py stepped       derive(NODES | LAYERS) against every recorded step; a 14-node domain
    python tools/hostemu/check_state_update.py selfcheck     after three steps derive(NODES) leaves the node blocks as they are
    python tools/hostemu/check_state_update.py cap           CAP_MOIST bit for bit; GLACIER_DYNAMICS is refused
    python tools/hostemu/check_state_update.py rows          get / SET / ADD / ints, four list shapes, two staging budgets; continuation
    python tools/hostemu/check_state_update.py midrun        FROZEN_SOIL as one chunk and as two, right behind a two-step vicgpu_step
    python tools/hostemu/check_state_update.py errorpath     nodes that end above the bottom layer: VICGPU_CELLERR_NODES for that cell
    python tools/hostemu/check_state_update.py zeroarea      HPD_CV = 0: empty node blocks, nothing else
    python tools/hostemu/check_state_update.py untouched     what a call must leave alone
    python tools/hostemu/check_state_update.py errors        every error return, each leaving every table as it was
    python tools/hostemu/check_state_update.py refusals      the n-th allocation refused, for every n
    python tools/hostemu/check_state_update.py group         3 shards on device 0 next to one context
Each prints "state update <name>: problems: none" (or the list) and exits with 1 when there are any."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import check_copy_cells as cc
import check_update_params as cu
from vic_amd import abi, domain, init_state
from vic_amd.abi import C
from vic_amd.api import Group, Model, VicGpuError, load_library

same, differing = cc.same, cc.differing
model, clone = cu.model, cu.clone
CAP, NODES, LAYERS, FRONTS = C["VICGPU_DERIVE_CAP_MOIST"], C["VICGPU_DERIVE_NODES"], C["VICGPU_DERIVE_LAYERS"], C["VICGPU_DERIVE_FRONTS"]
SET, ADD = C["VICGPU_STATE_SET"], C["VICGPU_STATE_ADD"]
INT_MIN = -2147483648
CPU_TOL = 1e-12              # what tests/test_domain.py holds the numpy restatement to
WRONG_D, WRONG_I = 1e30, 7   # what the rows a derive must produce hold before it


def rel_diff(a, b, floor):
    """tests/util.py rel_diff: relative with an absolute floor, NaN == NaN"""
    a = np.asarray(a, dtype=float); b = np.asarray(b, dtype=float)
    with np.errstate(all="ignore"):
        d = np.abs(a - b) / np.maximum(floor, np.maximum(np.abs(a), np.abs(b)))
    d = np.where(np.isnan(a) & np.isnan(b), 0.0, d)
    return np.where(np.isnan(d), np.inf, d)


def worst(ref, got):
    d = rel_diff(ref, got, 1e-12)
    return float(d.max()) if d.size else 0.0


# ------------------------------------------------------------------------------------------------ rows and the numpy restatement
def node_rows(Nn, fields=("SDN_MOIST", "SDN_ICE", "SDN_KAPPA", "SDN_CS")):
    return np.array([abi.sd_node(C[f], n, Nn) for f in fields for n in range(Nn)], np.int32)


def layer_rows(prefix):
    return np.array([C[prefix + "0"] + l for l in range(3)], np.int32)


FRONT_SI = np.array([C["SI_NFROST"], C["SI_NTHAW"]], np.int32)
FRONT_FX = np.array([C["FX_FDEPTH0"] + f for f in range(3)] + [C["FX_TDEPTH0"] + f for f in range(3)], np.int32)


def live_hrus(D):
    """HPD_CV > 0 and CPB_AREAFRACT > 0 in the HRU's band (initialize_model_state.c:692-694)"""
    Nn, Nb = D.opt.Nnode, D.opt.Nband
    cell, band = D.hru_iparams[C["HPI_CELL"]], D.hru_iparams[C["HPI_BAND"]]
    area = np.stack([D.cell_params[abi.cp_band(C["CPB_AREAFRACT"], b, Nn, Nb)] for b in range(Nb)])[band, cell]
    return (D.hru_dparams[C["HPD_CV"]] > 0) & (area > 0)


def np_fronts(opt, cp, cell, T):
    """find_0_degree_fronts (soil_conduction.c:775-828): counts and depths, NaN where there is no front"""
    Nn, nh = opt.Nnode, T.shape[1]
    Z = init_state._node(cp, "CPN_ZSUM", cell, Nn)
    nthaw = np.zeros(nh, np.int32); nfrost = np.zeros(nh, np.int32)
    td = np.full((3, nh), np.nan); fd = np.full((3, nh), np.nan)
    hid = np.arange(nh)
    for n in range(Nn - 2, -1, -1):
        th = (T[n] > 0) & (T[n + 1] <= 0) & (nthaw < 3)
        fr = ~th & (T[n] < 0) & (T[n + 1] >= 0) & (nfrost < 3)
        with np.errstate(all="ignore"):
            v = (0 - T[n]) / (T[n + 1] - T[n]) * (Z[n + 1] - Z[n]) + Z[n]
        td[np.minimum(nthaw, 2)[th], hid[th]] = v[th]
        fd[np.minimum(nfrost, 2)[fr], hid[fr]] = v[fr]
        nthaw = nthaw + th; nfrost = nfrost + fr
    return nfrost.astype(np.int32), nthaw.astype(np.int32), fd, td


def np_derive(D, sd, si, fx, what, hrus=None):
    """vicgpu_derive_soil_state restated with numpy: (sd, si, fx) after the call.  The cap is the reference's four lines
    (initialize_model_state.c:405-432); the other stages are the functions of vic_amd/init_state.py."""
    sd, si, fx = sd.copy(), si.copy(), fx.copy()
    opt, cp = D.opt, D.cell_params
    Nn = opt.Nnode
    cell = D.hru_iparams[C["HPI_CELL"]]
    listed = np.zeros(D.nhru, bool)
    listed[np.arange(D.nhru) if hrus is None else np.asarray(hrus)] = True
    mo, ic = layer_rows("SD_MOIST"), layer_rows("SD_ICE")
    if what & CAP:
        mm = init_state._layer(cp, "CPL_MAX_MOIST", cell)
        moist, ice = sd[mo], sd[ic]
        over = moist > mm
        with np.errstate(all="ignore"):
            ice = np.where(over, ice * (mm / moist), ice)
        moist = np.where(over, mm, moist)
        ice = np.where(ice > moist, moist, ice)
        sd[np.ix_(mo, listed)] = moist[:, listed]
        sd[np.ix_(ic, listed)] = ice[:, listed]
    live = live_hrus(D)
    on = listed & live
    T = np.stack([sd[abi.sd_node(C["SDN_T"], n, Nn)] for n in range(Nn)])
    moist = sd[mo]
    if what & NODES:
        blocks = init_state.distribute_node_moisture_properties(opt, cp, cell, T, moist)
        for f, b in zip(("SDN_MOIST", "SDN_ICE", "SDN_KAPPA", "SDN_CS"), blocks):
            r = node_rows(Nn, (f,))
            sd[np.ix_(r, on)] = b[:, on]
            sd[np.ix_(r, listed & ~live)] = 0.0
    if what & LAYERS:
        if opt.QUICK_FLUX:
            lice, lT = init_state.estimate_layer_ice_content_quick_flux(opt, cp, cell, T[0], T[1], moist)
        else:
            lice, lT = init_state.estimate_layer_ice_content(opt, cp, cell, T, moist)
        sd[np.ix_(ic, on)] = lice[:, on]
        sd[np.ix_(layer_rows("SD_LAYER_T"), on)] = lT[:, on]
    if (what & FRONTS) and not opt.QUICK_FLUX:
        fs = on & (cp[C["CP_FS_ACTIVE"]][cell] != 0)
        nfrost, nthaw, fd, td = np_fronts(opt, cp, cell, T)
        si[C["SI_NFROST"], fs] = nfrost[fs]; si[C["SI_NTHAW"], fs] = nthaw[fs]
        fx[np.ix_(FRONT_FX[:3], fs)] = fd[:, fs]
        fx[np.ix_(FRONT_FX[3:], fs)] = td[:, fs]
    return sd, si, fx


def spoil(D, sd, si, fx, layers=True, fronts=True, ice=True):
    """The rows the stages produce, filled with a recognisable wrong value."""
    sd, si, fx = sd.copy(), si.copy(), fx.copy()
    sd[node_rows(D.opt.Nnode)] = WRONG_D
    if layers:
        sd[layer_rows("SD_LAYER_T")] = WRONG_D
        if ice:
            sd[layer_rows("SD_ICE")] = WRONG_D
    if fronts:
        si[FRONT_SI] = WRONG_I
        fx[FRONT_FX] = WRONG_D
    return sd, si, fx


def frozen_pair(nsteps=4):
    """FROZEN_SOIL, 10 nodes, 2 bands, glacier HRUs, 5 base cells x 2 members (chunk boundary = member boundary)"""
    return cc.ensemble(dict(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=10, Nband=2, frozen_compat=0), 5, 2, 2, nsteps, 330, glacier=True)


def begin(m, E):
    m.set_forcing_map(E.cell_col, E.ncol)
    m.set_state(E.sd0, E.si0)
    m.push_forcing(E.f, E.sf, E.dmy)
    return m


def full_tables(m, put=True):
    t = cc.tables(m, put=put)
    t["cp"], t["hpd"] = m.get_cell_params(), m.get_hru_params()
    return t


# ------------------------------------------------------------------------------------------------ 1. the reference's initial state
def check_initial(log=print, tol=CPU_TOL):
    """Every fixture: sd0 / si0 in, the produced rows spoiled, derive(all, NODES | LAYERS | FRONTS), and back to sd0 / si0; the
    front depths against np_fronts.  Rows no stage produces for the fixture's options keep the spoiling value, every other
    row its bits."""
    from tests.golden_util import golden_names, load_golden
    bad, top = [], 0.0
    for name in golden_names():
        D, z = load_golden(name)
        sd0, si0 = np.ascontiguousarray(z["sd0"]), np.ascontiguousarray(z["si0"].astype(np.int32))
        m = Model(D)
        fx0 = m.get_fluxes()
        sdw, siw, fxw = spoil(D, sd0, si0, fx0)
        m.set_state(sdw, siw); m.set_fluxes(fxw)
        m.derive_soil_state(NODES | LAYERS | FRONTS)
        sd, si = m.get_state(); fx = m.get_fluxes()
        m.close()
        live = live_hrus(D)
        want_sd = sdw.copy()
        prod = np.concatenate([node_rows(D.opt.Nnode), layer_rows("SD_ICE"), layer_rows("SD_LAYER_T")])
        want_sd[np.ix_(prod, live)] = sd0[np.ix_(prod, live)]
        want_sd[np.ix_(node_rows(D.opt.Nnode), ~live)] = 0.0
        _, want_si, want_fx = np_derive(D, sd0, siw, fxw, FRONTS)
        fs = live & (D.cell_params[C["CP_FS_ACTIVE"]][D.hru_iparams[C["HPI_CELL"]]] != 0) & (not D.opt.QUICK_FLUX)
        ref_si = siw.copy(); ref_si[np.ix_(FRONT_SI, fs)] = si0[np.ix_(FRONT_SI, fs)]
        rest = np.setdiff1d(np.arange(sd.shape[0]), prod)
        w = max(worst(want_sd, sd), worst(want_fx, fx))
        top = max(top, w)
        p = []
        if not w < tol:
            p.append("worst relative difference %.3e" % w)
        if not np.array_equal(si, ref_si) or not np.array_equal(si, want_si):
            p.append("SI rows differ from si0")
        if not same(sd[rest], sd0[rest]):
            p.append("SD rows no stage produces changed")
        if (sd[np.ix_(prod, live)] == WRONG_D).any():
            p.append("a produced row still holds the spoiling value")
        log("state update initial %s: Nnode %d, %d HRUs (%d live, %d with fronts): worst %.3e %s" % (name, D.opt.Nnode, D.nhru, live.sum(), fs.sum(), w, p or ""), flush=True)
        bad += ["%s: %s" % (name, x) for x in p]
    log("state update initial: worst over the fixtures %.3e (bound %.1e)" % (top, tol), flush=True)
    return bad


# ------------------------------------------------------------------------------------------------ 2. the reference's stepped states
def check_stepped(log=print, tol=CPU_TOL):
    """Every fixture with FULL_ENERGY or FROZEN_SOIL, every recorded step: the node blocks and SD_LAYER_T0..2 spoiled,
    derive(all, NODES | LAYERS), against the reference's own rows (SD_ICE is not compared: runoff changes it afterwards).
    Then a 14-node, 3-band domain (the middle node bound) after two steps against np_derive."""
    from tests.golden_util import golden_names, load_golden
    bad, top = [], 0.0
    for name in golden_names():
        D, z = load_golden(name)
        if not (D.opt.FULL_ENERGY or D.opt.FROZEN_SOIL):
            continue
        m = Model(D)
        fx0 = m.get_fluxes()
        live = live_hrus(D)
        rows = np.concatenate([node_rows(D.opt.Nnode), layer_rows("SD_LAYER_T")])
        w = 0.0
        for k in range(z["states_d"].shape[0]):
            sdk, sik = np.ascontiguousarray(z["states_d"][k]), np.ascontiguousarray(z["states_i"][k].astype(np.int32))
            sdw, siw, _ = spoil(D, sdk, sik, fx0, fronts=False, ice=False)
            m.set_state(sdw, siw)
            m.derive_soil_state(NODES | LAYERS)
            sd, si = m.get_state()
            w = max(w, worst(sdk[np.ix_(rows, live)], sd[np.ix_(rows, live)]))
            if not np.array_equal(si, sik):
                bad.append("%s step %d: an SI row changed" % (name, k))
        m.close()
        top = max(top, w)
        if not w < tol:
            bad.append("%s: worst relative difference %.3e" % (name, w))
        log("state update stepped %s: Nnode %d (bound %d), %d steps: worst %.3e" % (name, D.opt.Nnode, 10 if D.opt.Nnode == 10 else 24 if D.opt.Nnode <= 24 else 50,
                                                                                   z["states_d"].shape[0], w), flush=True)
    # the middle bound
    opt = abi.default_options(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=14, Nband=3, frozen_compat=0)
    D = domain.make_domain(12, opt, ntile=2)
    f, sf, dmy = domain.make_forcing(D, 0, 2, start_doy=330)
    sd0, si0 = init_state.initial_state(D, f[0])
    m = Model(D)
    m.set_state(sd0, si0); m.push_forcing(f, sf, dmy)
    m.dist_prec(0, 2)
    sd, si = m.get_state(); fx = m.get_fluxes()
    if same(sd, sd0):
        bad.append("n14: the steps changed nothing")
    sdw, siw, fxw = spoil(D, sd, si, fx)
    m.set_state(sdw, siw); m.set_fluxes(fxw)
    m.derive_soil_state(NODES | LAYERS | FRONTS)
    got = m.get_state() + (m.get_fluxes(),)
    m.close()
    want = np_derive(D, sdw, siw, fxw, NODES | LAYERS | FRONTS)
    w = max(worst(want[0], got[0]), worst(want[2], got[2]))
    top = max(top, w)
    if not w < tol or not np.array_equal(want[1], got[1]) or (got[0] == WRONG_D).any():
        bad.append("n14: worst %.3e, SI equal %s, spoiled left %s" % (w, np.array_equal(want[1], got[1]), (got[0] == WRONG_D).any()))
    log("state update stepped n14 (synthetic, bound 24): %d HRUs: worst %.3e" % (D.nhru, w), flush=True)
    log("state update stepped: worst over the fixtures %.3e (bound %.1e)" % (top, tol), flush=True)
    return bad


# ------------------------------------------------------------------------------------------------ 3. the device against itself
def check_selfcheck(log=print, tol=CPU_TOL):
    E = frozen_pair()
    m = begin(model(E, clone(E.D)), E)
    m.dist_prec(0, 3)
    t0 = full_tables(m, put=False)
    m.derive_soil_state(NODES)
    t1 = full_tables(m, put=False)
    m.close()
    live = live_hrus(E.D)
    rows = node_rows(E.D.opt.Nnode)
    a, b = t0["sd"][np.ix_(rows, live)], t1["sd"][np.ix_(rows, live)]
    w = worst(a, b)
    bad = [] if w < tol else ["the node blocks moved by %.3e" % w]
    rest = np.setdiff1d(np.arange(t0["sd"].shape[0]), rows)
    if not same(t0["sd"][rest], t1["sd"][rest]) or [k for k in differing(t0, t1) if k != "sd"]:
        bad.append("other rows or tables changed: %s" % differing(t0, t1))
    if same(t0["sd"], E.sd0) or not (t0["sd"][node_rows(E.D.opt.Nnode, ("SDN_ICE",))] > 0).any():
        bad.append("the steps left no node ice to reproduce")
    log("state update selfcheck: %d live HRUs, node blocks after derive(NODES) bit for bit: %s (worst %.3e)" % (live.sum(), "yes" if same(a, b) else "no", w), flush=True)
    return bad


# ------------------------------------------------------------------------------------------------ 4. the moisture cap
def cap_case(E):
    """Listed: members 1 and 2.  Their ice rows are set to 30 % of the moisture; then increments that push every third listed
    HRU above CPL_MAX_MOIST in layer 0, every sixth also in layer 2."""
    D = E.D
    hrus = cu.hrus_of(D, cu.member_cells(E, [1, 2]))
    mm = init_state._layer(D.cell_params, "CPL_MAX_MOIST", D.hru_iparams[C["HPI_CELL"]])[:, hrus]
    moist = E.sd0[np.ix_(layer_rows("SD_MOIST"), hrus)]
    k = np.arange(len(hrus))
    inc = np.full((3, len(hrus)), 0.75)
    inc[0, k % 3 == 0] = (mm[0] - moist[0] + 3.25)[k % 3 == 0]
    inc[2, k % 6 == 0] = (mm[2] - moist[2] + 11.5)[k % 6 == 0]
    return hrus, np.ascontiguousarray(0.3 * moist), np.ascontiguousarray(inc)


def check_cap(log=print):
    E = cc.quickflux()
    D = E.D
    hrus, ice, inc = cap_case(E)
    m = cc.start(model(E, clone(D)), E)
    t0 = full_tables(m)
    m.update_state(layer_rows("SD_ICE"), ice, hrus)
    m.update_state(layer_rows("SD_MOIST"), inc, hrus, mode=ADD)
    m.derive_soil_state(CAP, hrus)
    t1 = full_tables(m)
    m.close()
    sd = E.sd0.copy()
    sd[np.ix_(layer_rows("SD_ICE"), hrus)] = ice
    sd[np.ix_(layer_rows("SD_MOIST"), hrus)] = sd[np.ix_(layer_rows("SD_MOIST"), hrus)] + inc
    over = (sd[np.ix_(layer_rows("SD_MOIST"), hrus)] > init_state._layer(D.cell_params, "CPL_MAX_MOIST", D.hru_iparams[C["HPI_CELL"]])[:, hrus])
    want, _, _ = np_derive(D, sd, E.si0, t0["flux"], CAP, hrus)
    bad = []
    if not same(want, t1["sd"]):
        bad.append("the capped rows differ from the reference's four lines in %d words" % (want != t1["sd"]).sum())
    n_over = int(over.any(axis=0).sum())
    if not (len(hrus) // 3 <= n_over <= len(hrus) // 3 + 1) or not (over.sum(axis=0) == 2).any() or same(want, sd):
        bad.append("the case: %d of %d listed HRUs above the maximum" % (n_over, len(hrus)))
    if not (want[np.ix_(layer_rows("SD_ICE"), hrus)][over] > 0).all():
        bad.append("the case: no ice to rescale")
    rest = np.setdiff1d(np.arange(D.nhru), hrus)
    if not same(t1["sd"][:, rest], t0["sd"][:, rest]) or [k for k in differing(t0, t1) if k != "sd"]:
        bad.append("HRUs that were not listed, or other tables, changed: %s" % differing(t0, t1))
    # GLACIER_DYNAMICS: refused, nothing changed
    G = cc.ensemble(dict(FULL_ENERGY=1, Nband=3, GLACIER_DYNAMICS=1), 5, 2, 2, 1, 80, glacier=True)
    g = begin(model(G, clone(G.D)), G)
    g0 = full_tables(g, put=False)
    rc = g.lib.vicgpu_derive_soil_state(g.h, 0, None, CAP | NODES)
    rc2 = g.lib.vicgpu_derive_soil_state(g.h, G.D.nhru, None, CAP)
    if (rc, rc2) != (C["VICGPU_ERR_UNSUPPORTED"],) * 2 or differing(g0, full_tables(g, put=False)):
        bad.append("GLACIER_DYNAMICS: codes %d, %d, changed %s" % (rc, rc2, differing(g0, full_tables(g, put=False))))
    g.derive_soil_state(NODES)                       # the other stages stay available
    g.close()
    log("state update cap: %d listed HRUs, %d capped (%d in two layers), differing: %s" % (len(hrus), n_over, (over.sum(axis=0) == 2).sum(), bad or "none"), flush=True)
    return bad


# ------------------------------------------------------------------------------------------------ 5. gather / scatter
def row_lists(D):
    Nn = D.opt.Nnode
    sdr = np.array([C["SD_SNOW_SWQ"], C["SD_MOIST2"], C["SD_MOIST0"], abi.sd_node(C["SDN_T"], 1, Nn), C["SD_GLAC_CUM_MASS_BALANCE"], C["SD_WDEW"],
                    abi.sd_node(C["SDN_CS"], Nn - 1, Nn), C["SD_MOIST1"], C["SD_SNOW_DEPTH"], 0, abi.sd_nrow(Nn) - 1], np.int32)      # 11 rows: two tiles
    sir = np.array([C["SI_SNOW_LAST_SNOW"], abi.si_nrow(Nn) - 1, C["SI_SNOW_SNOW"], 0, C["SI_NTHAW"]], np.int32)
    first = lambda r: r[np.sort(np.unique(r, return_index=True)[1])]               # in this order, no row twice
    return first(sdr), first(sir)


def hru_lists(D):
    rng = np.random.default_rng(11)
    return {"wave": np.arange(64, 192, dtype=np.int32), "ragged": np.arange(7, 7 + 209, dtype=np.int32),
            "permuted": rng.permutation(D.nhru)[:300].astype(np.int32), "dense": None}


def check_rows(log=print):
    E = cc.quickflux()
    D = E.D
    sdr, sir = row_lists(D)
    bad = []
    if D.nhru != 924:
        bad.append("the ensemble has %d HRUs, not 924" % D.nhru)
    if not (E.si0[C["SI_SNOW_LAST_SNOW"]] == INT_MIN).any() or not np.isnan(E.sd0[C["SD_GLAC_CUM_MASS_BALANCE"]]).any():
        bad.append("the case: no INT_MIN or no NaN in the initial state")
    rng = np.random.default_rng(3)
    for stage in (None, "0"):
        m = cc.start(model(E, clone(D), stage_mb=stage), E)
        m.dist_prec(0, 1, sync=False)
        sd, si = None, None
        for name, hrus in hru_lists(D).items():
            cols = np.arange(D.nhru) if hrus is None else hrus
            sd, si = m.get_state()
            p = []
            if not same(m.get_state_rows(sdr, hrus), sd[np.ix_(sdr, cols)]):
                p.append("get")
            if not same(m.get_state_rows(sir, hrus, ints=True), si[np.ix_(sir, cols)]):
                p.append("get ints")
            v = rng.normal(size=(len(sdr), len(cols))) * 10.0 ** rng.integers(-3, 4, size=(len(sdr), 1))
            v[4, ::5] = np.nan; v[0, 1::7] = -0.0
            m.update_state(sdr, v, hrus)
            sd[np.ix_(sdr, cols)] = v
            if not same(m.get_state()[0], sd):
                p.append("SET")
            a = rng.normal(size=v.shape)
            m.update_state(sdr, a, hrus, mode=ADD)
            sd[np.ix_(sdr, cols)] = sd[np.ix_(sdr, cols)] + a
            if not same(m.get_state()[0], sd):
                p.append("ADD")
            iv = rng.integers(-5, 1 << 20, size=(len(sir), len(cols))).astype(np.int32)
            iv[0, ::3] = INT_MIN; iv[-1, ::4] = 2147483647
            m.update_state(sir, iv, hrus, ints=True)
            si[np.ix_(sir, cols)] = iv
            got = m.get_state()
            if not same(got[1], si) or not same(got[0], sd):
                p.append("SET ints")
            if not same(m.get_state_rows(sdr, hrus), sd[np.ix_(sdr, cols)]) or not same(m.get_state_rows(sir, hrus, ints=True), iv):
                p.append("get after the updates")
            log("state update rows (stage %s) %s: %d x %d and %d x %d, differing: %s" % (stage or "default", name, len(sdr), len(cols), len(sir), len(cols), p or "none"), flush=True)
            bad += ["stage %s, %s: %s" % (stage or "default", name, x) for x in p]
        m.close()
    # continuation: SET of final values through the device against the same edit through set_state
    hrus = hru_lists(D)["permuted"]
    rows = np.array([C["SD_MOIST0"], C["SD_MOIST1"], C["SD_MOIST2"], C["SD_SNOW_SWQ"], C["SD_SNOW_DEPTH"]], np.int32)
    v = E.sd0[np.ix_(rows, hrus)] * np.array([0.9, 0.95, 0.97, 1.5, 1.5])[:, None]
    irows = np.array([C["SI_SNOW_LAST_SNOW"]], np.int32)
    iv = np.full((1, len(hrus)), 2, np.int32)
    out = []
    for how in ("host", "device", "none"):
        m = cc.start(model(E, clone(D)), E)
        if how == "host":
            sd, si = m.get_state()
            sd[np.ix_(rows, hrus)] = v; si[np.ix_(irows, hrus)] = iv
            m.set_state(sd, si)
        elif how == "device":
            m.update_state(rows, v, hrus)
            m.update_state(irows, iv, hrus, ints=True)
        rec = cu.records(m, 0, 2, cu.all_names(m))
        out.append((cc.tables(m), rec))
        m.close()
    d = differing(out[0][0], out[1][0]) + ([] if same(out[0][1], out[1][1]) else ["the records"])
    if same(out[0][1], out[2][1]) or not np.isfinite(out[0][1][np.isfinite(out[2][1])]).all():
        d.append("the records with and without the edit do not differ, or are not finite")
    log("state update rows continuation: %d record rows, differing: %s" % (out[0][1].shape[1], d or "none"), flush=True)
    return bad + ["continuation: " + x for x in d]


# ------------------------------------------------------------------------------------------------ 6. mid-run
def check_midrun(log=print, chunks="2"):
    """The frozen pair: an update and a derive of HRUs on both sides of the chunk boundary right behind a two-step vicgpu_step
    that was not waited for; two more steps.  The expected path waits, edits the state on the host and derives then."""
    os.environ["VICGPU_CHUNKS"] = chunks
    try:
        E = frozen_pair()
        D = E.D
        hrus = cu.hrus_of(D, np.array([1, 3, 4, 5, 8], np.int32))
        Nn = D.opt.Nnode
        mrows = layer_rows("SD_MOIST")
        trows = np.array([abi.sd_node(C["SDN_T"], n, Nn) for n in (1, 2, 3)], np.int32)
        inc = np.tile(np.array([[4.0], [-6.0], [5000.0]]), (1, len(hrus)))      # layer 2 goes above its maximum
        dT = np.tile(np.array([[-0.8], [-0.5], [0.3]]), (1, len(hrus)))
        what = CAP | NODES | LAYERS | FRONTS
        a, b, n = (begin(model(E, clone(D)), E) for _ in range(3))
        a.dist_prec(0, 2, sync=False)
        a.update_state(mrows, inc, hrus, mode=ADD)
        a.update_state(trows, dT, hrus, mode=ADD)
        a.derive_soil_state(what, hrus)
        a.dist_prec(2, 2)
        b.dist_prec(0, 2)
        b.synchronize()
        sd, si = b.get_state()
        sd[np.ix_(mrows, hrus)] = sd[np.ix_(mrows, hrus)] + inc
        sd[np.ix_(trows, hrus)] = sd[np.ix_(trows, hrus)] + dT
        b.set_state(sd, si)
        b.derive_soil_state(what, hrus)
        mid = b.get_state()[0]
        b.dist_prec(2, 2)
        n.dist_prec(0, 4)
        ta, tb, tn = (cc.tables(x, put=False) for x in (a, b, n))
        for x in (a, b, n):
            x.close()
        bad = ["after the steps: " + k for k in differing(tb, ta)]
        if same(tb["sd"], tn["sd"]) or not np.isfinite(tb["cell_out"]).all():
            bad.append("the run with the update does not differ from the run without, or is not finite")
        mm = init_state._layer(D.cell_params, "CPL_MAX_MOIST", D.hru_iparams[C["HPI_CELL"]])
        if not (mid[C["SD_MOIST2"], hrus] == mm[2, hrus]).all() or same(mid[node_rows(Nn)][:, hrus], sd[node_rows(Nn)][:, hrus]):
            bad.append("the derive did not cap layer 2 or left the node blocks")
        cell = D.hru_iparams[C["HPI_CELL"], hrus]
        if not ((cell < E.ncol).any() and (cell >= E.ncol).any()):
            bad.append("the listed HRUs lie on one side of the chunk boundary")
    finally:
        os.environ.pop("VICGPU_CHUNKS", None)
    log("state update midrun (chunks %s): %d HRUs, differing: %s" % (chunks, len(hrus), bad or "none"), flush=True)
    return bad


# ------------------------------------------------------------------------------------------------ 7. the ERROR return of the reference
def check_errorpath(log=print, tol=CPU_TOL):
    E = frozen_pair()
    D = clone(E.D)
    Nn = D.opt.Nnode
    c = 6
    zr = np.array([abi.cp_node(C["CPN_ZSUM"], n, Nn) for n in range(Nn)], np.int32)
    Z = D.cell_params[zr, c]
    bottom = sum(D.cell_params[abi.cp_layer(C["CPL_DEPTH"], l), c] for l in range(3))
    m = begin(model(E, D), E)
    if Z[Nn - 2] < bottom:           # the deepest node alone
        m.update_cell_params(zr[-1:], np.array([[0.5 * (Z[Nn - 2] + bottom)]]), [c])
    else:                            # the deepest node drags the others along: the profile keeps its shape
        m.update_cell_params(zr, (Z * (0.95 * bottom / Z[-1]))[:, None], [c])
    fx0 = m.get_fluxes()
    sdw, siw, fxw = spoil(D, E.sd0, E.si0, fx0, fronts=False)
    m.set_state(sdw, siw)
    t0 = full_tables(m, put=False)
    m.derive_soil_state(LAYERS)
    t1 = full_tables(m, put=False)
    flags = m.get_cell_errors()
    m.reset_accum()
    cleared = m.get_cell_errors()
    m.close()
    bad = []
    want_flags = np.zeros(D.ncell, np.int32); want_flags[c] = C["VICGPU_CELLERR_NODES"]
    if not np.array_equal(flags, want_flags):
        bad.append("cell flags %s" % flags.tolist())
    if cleared.any():
        bad.append("vicgpu_reset_accum left %s" % cleared.tolist())
    cell = D.hru_iparams[C["HPI_CELL"]]
    live = live_hrus(D)
    rows = np.concatenate([layer_rows("SD_ICE"), layer_rows("SD_LAYER_T")])
    others = live & (cell != c)
    want = np_derive(E.D, sdw, siw, fx0, LAYERS)[0]              # the members start from perturbed moisture: not sd0's layer rows
    w = worst(want[np.ix_(rows, others)], t1["sd"][np.ix_(rows, others)])
    if not w < tol:
        bad.append("the other cells' layer rows: worst %.3e" % w)
    mine = live & (cell == c)
    fail = t1["sd"][np.ix_(rows, mine)]
    # layers 0 and 1 are computed, the failing layer 2 takes zeros
    if (fail[[0, 1, 3, 4]] == WRONG_D).any() or (fail[[2, 5]] != 0).any() or not mine.any():
        bad.append("the failing cell's rows: %s" % fail.tolist())
    rest = np.setdiff1d(np.arange(t0["sd"].shape[0]), rows)
    if not same(t0["sd"][rest], t1["sd"][rest]) or sorted(differing(t0, t1)) != ["cell_err", "sd"]:
        bad.append("changed: %s" % differing(t0, t1))
    log("state update errorpath: cell %d of %d flagged, the others' worst %.3e, differing: %s" % (c, D.ncell, w, bad or "none"), flush=True)
    return bad


# ------------------------------------------------------------------------------------------------ 8. HRUs without area
def check_zeroarea(log=print):
    E = frozen_pair()
    D = clone(E.D)
    m = begin(model(E, D), E)
    dead = np.array([0, 7, E.base.nhru + 3, D.nhru - 1], np.int32)
    m.update_hru_params([C["HPD_CV"]], np.zeros((1, len(dead))), dead)
    fx0 = m.get_fluxes()
    sdw, siw, fxw = spoil(D, E.sd0, E.si0, fx0)
    m.set_state(sdw, siw); m.set_fluxes(fxw)
    m.derive_soil_state(NODES | LAYERS | FRONTS)
    sd, si = m.get_state(); fx = m.get_fluxes()
    m.close()
    nr = node_rows(D.opt.Nnode)
    lr = np.concatenate([layer_rows("SD_ICE"), layer_rows("SD_LAYER_T")])
    bad = []
    if (sd[np.ix_(nr, dead)] != 0).any():
        bad.append("the node blocks are not empty")
    if not (sd[np.ix_(lr, dead)] == WRONG_D).all() or not (si[np.ix_(FRONT_SI, dead)] == WRONG_I).all() or not (fx[np.ix_(FRONT_FX, dead)] == WRONG_D).all():
        bad.append("layer or front rows of the HRUs without area were written")
    alive = np.setdiff1d(np.arange(D.nhru), dead)
    if (sd[np.ix_(np.concatenate([nr, lr]), alive)] == WRONG_D).any() or (si[np.ix_(FRONT_SI, alive)] == WRONG_I).any():
        bad.append("the other HRUs were not derived")
    log("state update zeroarea: %d HRUs without area, differing: %s" % (len(dead), bad or "none"), flush=True)
    return bad


# ------------------------------------------------------------------------------------------------ 9. untouched, errors, refusals, group
def check_untouched(log=print):
    """A mid-run update and derive with put_data, records, cell groups, a forcing map and a retire mask in force."""
    E = cc.quickflux()
    D = E.D
    m = cc.start(model(E, clone(D)), E)
    m.records_config(cc.OUT, depth=2)
    m.records_set_groups(np.arange(0, D.ncell + 1, E.ncol, dtype=np.int32), np.arange(D.ncell, dtype=np.int32))
    m.set_retire_on_error(C["VICGPU_CELLERR_REFERENCE"])
    valid = np.ones(D.ncell, np.int32); valid[2 * E.ncol + 3] = 0
    m.dist_prec(0, 2)
    m.set_cell_valid(valid)

    def snapshot():
        t = full_tables(m)
        t["forcing"], t["snowflag"] = m.get_forcing(3)
        t["map"] = m.get_forcing_map()[1]
        return t, (m.lib.vicgpu_records_nrow(m.h), m.records_ncol(), m.records_get_groups(), m.get_forcing_map()[0])

    t0, cfg0 = snapshot()
    hrus, ice, inc = cap_case(E)
    rows = np.concatenate([layer_rows("SD_MOIST"), [C["SD_SNOW_SWQ"]]]).astype(np.int32)
    v = np.vstack([inc, np.full((1, len(hrus)), 0.01)])
    m.update_state(rows, v, hrus, mode=ADD)
    m.update_state([C["SI_SNOW_SNOW"]], np.ones((1, len(hrus)), np.int32), hrus, ints=True)
    m.derive_soil_state(CAP | NODES | LAYERS | FRONTS, hrus)
    t1, cfg1 = snapshot()
    bad = [k + " changed" for k in differing(t0, t1) if k not in ("sd", "si")]
    if cfg0 != cfg1:
        bad.append("the configuration changed: %s -> %s" % (cfg0, cfg1))
    rest = np.setdiff1d(np.arange(D.nhru), hrus)
    produced = np.concatenate([rows, node_rows(D.opt.Nnode), layer_rows("SD_ICE"), layer_rows("SD_LAYER_T")])
    other = np.setdiff1d(np.arange(t0["sd"].shape[0]), produced)
    if not same(t0["sd"][:, rest], t1["sd"][:, rest]) or not same(t0["sd"][other], t1["sd"][other]):
        bad.append("SD entries that were neither listed nor produced changed")
    irest = np.setdiff1d(np.arange(t0["si"].shape[0]), [C["SI_SNOW_SNOW"]])
    if not same(t0["si"][:, rest], t1["si"][:, rest]) or not same(t0["si"][irest], t1["si"][irest]):
        bad.append("SI entries that were not listed changed (QUICK_FLUX: no front rows)")
    if same(t0["sd"][np.ix_(produced, hrus)], t1["sd"][np.ix_(produced, hrus)]):
        bad.append("nothing was updated")
    rec = m.run_records(2, 1)
    rec.wait()
    if rec.out.shape[-1] != E.M or not np.isfinite(rec.out).all() or not rec.out.any():
        bad.append("the record after the update")
    del rec
    m.close()
    log("state update untouched: differing: %s" % (bad or "none"), flush=True)
    return bad


def error_returns(log=print):
    """Every VICGPU_ERR_ARG / _STATE / _UNSUPPORTED return of the header, each followed by a comparison of all tables.  All of
    them are refused on the host before any launch."""
    lib = load_library()
    ARG, ST, UNS, OK = C["VICGPU_ERR_ARG"], C["VICGPU_ERR_STATE"], C["VICGPU_ERR_UNSUPPORTED"], 0
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    i32 = lambda x: np.asarray(x, dtype=np.int32)
    E = cc.quickflux()
    D = clone(E.D)
    nh = D.nhru
    checks = []

    def call(fn, kind, h, rows, cols, values=0.5, nrow=None, n=None, mode=SET):
        """kind: 'd' (double values), 'i' (int values), 'dm' (double values and a mode)"""
        r = None if rows is None else i32(rows)
        c = None if cols is None else i32(cols)
        nrow = (len(r) if r is not None else 0) if nrow is None else nrow
        n = (len(c) if c is not None else 0) if n is None else n
        size = max(nrow, 1) * max(n, 1)
        if values is None:
            v = None
        elif kind == "i":
            v = np.full(size, 3, np.int32).ctypes.data_as(ip)
        else:
            v = np.full(size, float(values)).ctypes.data_as(dp)
        args = [h, nrow, r.ctypes.data_as(ip) if r is not None else None, n, c.ctypes.data_as(ip) if c is not None else None, v]
        return fn(*(args + [mode] if kind == "dm" else args))

    def derive(fn, h, cols, what, n=None):
        c = None if cols is None else i32(cols)
        n = (len(c) if c is not None else 0) if n is None else n
        return fn(h, n, c.ctypes.data_as(ip) if c is not None else None, what)

    def entries(prefix):
        g = lambda name: getattr(lib, prefix + name)
        return [(g("get_state_rows"), "d", abi.sd_nrow(D.opt.Nnode), "get_state_rows"), (g("get_state_rows_i"), "i", abi.si_nrow(D.opt.Nnode), "get_state_rows_i"),
                (g("update_state"), "dm", abi.sd_nrow(D.opt.Nnode), "update_state"), (g("update_state_i"), "i", abi.si_nrow(D.opt.Nnode), "update_state_i")], g("derive_soil_state")

    def every_case(tag, prefix, h, tables):
        t0 = tables()
        row_entries, dv = entries(prefix)
        cases = []
        for fn, kind, nrows, name in row_entries:
            cs = [
                ("null rows", lambda fn=fn, kind=kind: call(fn, kind, h, None, [1], nrow=1), ARG),
                ("null values", lambda fn=fn, kind=kind: call(fn, kind, h, [1], [1], values=None), ARG),
                ("nrow < 0", lambda fn=fn, kind=kind: call(fn, kind, h, [1], [1], nrow=-1), ARG),
                ("n < 0", lambda fn=fn, kind=kind: call(fn, kind, h, [1], [1], n=-1), ARG),
                ("row == nrows", lambda fn=fn, kind=kind, nrows=nrows: call(fn, kind, h, [0, nrows], [1]), ARG),
                ("row < 0", lambda fn=fn, kind=kind: call(fn, kind, h, [-1], [1]), ARG),
                ("a row listed twice", lambda fn=fn, kind=kind: call(fn, kind, h, [2, 1, 2], [1]), ARG),
                ("HRU == nhru", lambda fn=fn, kind=kind: call(fn, kind, h, [1], [0, nh]), ARG),
                ("HRU < 0", lambda fn=fn, kind=kind: call(fn, kind, h, [1], [3, -1]), ARG),
                ("an HRU listed twice", lambda fn=fn, kind=kind: call(fn, kind, h, [1], [5, 70, 5]), ARG),
                ("... after legal rows and HRUs", lambda fn=fn, kind=kind: call(fn, kind, h, [0, 1, 2], [0, 1, 2, nh, 1]), ARG),
                ("no list, n == nhru - 1", lambda fn=fn, kind=kind: call(fn, kind, h, [1], None, n=nh - 1), ARG),
                ("no list, n == nhru + 1", lambda fn=fn, kind=kind: call(fn, kind, h, [1], None, n=nh + 1), ARG),
                ("no list, n == 1", lambda fn=fn, kind=kind: call(fn, kind, h, [1], None, n=1), ARG),
            ]
            if kind == "dm":
                cs += [("mode 2", lambda fn=fn: call(fn, "dm", h, [1], [1], mode=2), ARG), ("mode -1", lambda fn=fn: call(fn, "dm", h, [1], [1], mode=-1), ARG),
                       ("mode 2, nothing to do", lambda fn=fn: call(fn, "dm", h, [], [], mode=2), ARG)]
            cases += [("%s%s: %s" % (tag, name, w), f, want) for w, f, want in cs]
        cases += [("%sderive: %s" % (tag, w), f, want) for w, f, want in [
            ("what == 0", lambda: derive(dv, h, [1], 0), ARG),
            ("what == 16", lambda: derive(dv, h, [1], 16), ARG),
            ("an unknown bit beside known ones", lambda: derive(dv, h, [1], NODES | 32), ARG),
            ("what < 0", lambda: derive(dv, h, [1], -1), ARG),
            ("what == 0, nothing to do", lambda: derive(dv, h, [], 0), ARG),
            ("n < 0", lambda: derive(dv, h, [1], NODES, n=-1), ARG),
            ("HRU == nhru", lambda: derive(dv, h, [0, nh], NODES), ARG),
            ("HRU < 0", lambda: derive(dv, h, [-1], NODES), ARG),
            ("an HRU listed twice", lambda: derive(dv, h, [5, 70, 5], CAP | NODES | LAYERS | FRONTS), ARG),
            ("no list, n == nhru - 1", lambda: derive(dv, h, None, NODES, n=nh - 1), ARG),
            ("no list, n == nhru + 1", lambda: derive(dv, h, None, CAP, n=nh + 1), ARG),
        ]]
        for w, f, want in cases:
            checks.append((w, f(), want))
            checks.append((w + ": tables", differing(t0, tables()) or "unchanged", "unchanged"))
        for fn, kind, _, name in row_entries:
            for w, f in [("nrow == 0", lambda: call(fn, kind, h, [], [1, 2])), ("n == 0", lambda: call(fn, kind, h, [1, 2], [])),
                         ("nrow == 0, null rows and values", lambda: call(fn, kind, h, None, [1], values=None)),
                         ("n == 0, null list", lambda: call(fn, kind, h, [1], None, n=0))]:
                checks.append(("%s%s: %s" % (tag, name, w), f(), OK))
        checks.append((tag + "derive: n == 0", derive(dv, h, [], NODES), OK))
        checks.append((tag + "derive: n == 0, null list", derive(dv, h, None, CAP | FRONTS, n=0), OK))
        checks.append((tag + "tables after the no-ops", differing(t0, tables()) or "unchanged", "unchanged"))

    for prefix in ("vicgpu_", "vicgpu_group_"):
        row_entries, dv = entries(prefix)
        for fn, kind, _, name in row_entries:
            checks.append((prefix + name + ": null handle", call(fn, kind, None, [1], [1]), ARG))
            checks.append((prefix + name + ": null handle, nothing to do", call(fn, kind, None, [], []), ARG))
        checks.append((prefix + "derive: null handle", derive(dv, None, [1], NODES), ARG))
    fresh = ctypes.c_void_p()
    assert lib.vicgpu_create(ctypes.byref(D.opt), 0, ctypes.byref(fresh)) == 0
    row_entries, dv = entries("vicgpu_")
    for fn, kind, _, name in row_entries:
        checks.append(("no domain: " + name, call(fn, kind, fresh, [1], [1]), ST))
        checks.append(("no domain: %s, nothing to do" % name, call(fn, kind, fresh, [], []), ST))
    checks += [("no domain: derive", derive(dv, fresh, [1], NODES), ST), ("no domain: derive, what == 0", derive(dv, fresh, [1], 0), ARG)]
    lib.vicgpu_destroy(fresh)
    m = cc.start(model(E, D), E)
    m.dist_prec(0, 1)
    every_case("", "vicgpu_", m.h, lambda: full_tables(m))
    for w, f in [("Model.update_state", lambda: m.update_state([1, 1], np.zeros((2, 1)), [0])), ("Model.get_state_rows", lambda: m.get_state_rows([1, 1], [0])),
                 ("Model.derive_soil_state", lambda: m.derive_soil_state(NODES, [4, 4]))]:
        try:
            f()
            checks.append((w + " raises", False, True))
        except VicGpuError as e:
            checks.append((w + " raises with the rule", "listed twice" in str(e), True))
    m.close()
    # CAP_MOIST with GLACIER_DYNAMICS
    G = cc.ensemble(dict(FULL_ENERGY=1, Nband=3, GLACIER_DYNAMICS=1), 5, 2, 2, 1, 80, glacier=True)
    for cls, kw, tag in ((Model, {}, ""), (Group, dict(devices=[0, 0]), "group: ")):
        g = begin(model(G, clone(G.D), cls=cls, **kw), G)
        t0 = full_tables(g, put=False)
        dvg = g.lib.vicgpu_derive_soil_state
        checks += [(tag + "GLACIER_DYNAMICS: CAP_MOIST", derive(dvg, g.h, None, CAP, n=G.D.nhru), UNS), (tag + "GLACIER_DYNAMICS: CAP_MOIST | NODES, listed", derive(dvg, g.h, [0, 1], CAP | NODES), UNS),
                   (tag + "GLACIER_DYNAMICS: CAP_MOIST, nothing to do", derive(dvg, g.h, [], CAP), UNS), (tag + "GLACIER_DYNAMICS: what == 0 comes first", derive(dvg, g.h, [1], 0), ARG),
                   (tag + "GLACIER_DYNAMICS: tables", differing(t0, full_tables(g, put=False)) or "unchanged", "unchanged"),
                   (tag + "GLACIER_DYNAMICS: NODES | LAYERS", derive(dvg, g.h, [0, 1], NODES | LAYERS), OK)]
        g.close()
    # the group
    g = cc.start(model(E, clone(E.D), cls=Group, devices=[0, 0, 0]), E)
    every_case("group: ", "vicgpu_group_", g.h, lambda: full_tables(g))
    fresh = ctypes.c_void_p()
    dev = i32([0, 0])
    assert lib.vicgpu_group_create(ctypes.byref(D.opt), 2, dev.ctypes.data_as(ip), ctypes.byref(fresh)) == 0
    row_entries, dv = entries("vicgpu_group_")
    for fn, kind, _, name in row_entries:
        checks.append(("group: no domain: " + name, call(fn, kind, fresh, [1], [1]), ST))
    checks.append(("group: no domain: derive", derive(dv, fresh, [1], NODES), ST))
    lib.vicgpu_group_destroy(fresh)
    g.close()
    failed = [(w, got, want) for w, got, want in checks if got != want]
    for w, got, want in failed:
        log("state update return: %s gave %s, want %s" % (w, got, want), flush=True)
    log("state update errors: %d checks, failed: %d" % (len(checks), len(failed)), flush=True)
    return ["%s gave %s" % (w, got) for w, got, _ in failed], len(checks)


def check_refusals(log=print):
    """The five entries under a runtime that refuses their n-th allocation, n = 1, 2, ...: VICGPU_ERR_HIP, no live runtime object
    added and every table as it was, until the call gets through -- which leaves no object behind either."""
    lib = load_library()
    lib.hostemu_live_objects.restype = ctypes.c_longlong
    lib.hostemu_refuse_alloc.argtypes = [ctypes.c_longlong]
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    E = cc.quickflux()
    hrus, ice, inc = cap_case(E)
    rows = layer_rows("SD_MOIST")
    irows = np.array([C["SI_SNOW_SNOW"], C["SI_SNOW_MELTING"]], np.int32)
    iv = np.ones((2, len(hrus)), np.int32)
    out_d, out_i = np.zeros_like(inc), np.zeros_like(iv)
    R = lambda a: a.ctypes.data_as(ip)
    calls = {
        "get_state_rows": (lambda h: lib.vicgpu_get_state_rows(h, 3, R(rows), len(hrus), R(hrus), out_d.ctypes.data_as(dp)), []),
        "get_state_rows_i": (lambda h: lib.vicgpu_get_state_rows_i(h, 2, R(irows), len(hrus), R(hrus), R(out_i)), []),
        "update_state": (lambda h: lib.vicgpu_update_state(h, 3, R(rows), len(hrus), R(hrus), inc.ctypes.data_as(dp), ADD), ["sd"]),
        "update_state_i": (lambda h: lib.vicgpu_update_state_i(h, 2, R(irows), len(hrus), R(hrus), R(iv)), ["si"]),
        "derive_soil_state": (lambda h: lib.vicgpu_derive_soil_state(h, len(hrus), R(hrus), CAP | NODES | LAYERS), ["sd"]),
    }
    bad, counts = [], []
    m = cc.start(model(E, clone(E.D)), E)
    m.dist_prec(0, 1)
    for name, (fn, changes) in calls.items():
        t0 = full_tables(m)
        before = lib.hostemu_live_objects()
        for n in range(1, 20):
            lib.hostemu_refuse_alloc(n)
            rc = fn(m.h)
            lib.hostemu_refuse_alloc(0)
            if rc == 0:
                break
            if rc != C["VICGPU_ERR_HIP"] or lib.hostemu_live_objects() != before or differing(t0, full_tables(m)):
                bad.append("%s, allocation %d refused: code %d, %d objects more, changed %s" % (name, n, rc, lib.hostemu_live_objects() - before, differing(t0, full_tables(m))))
        counts.append(n - 1)
        if lib.hostemu_live_objects() != before:
            bad.append("%s: %d objects left by the call that got through" % (name, lib.hostemu_live_objects() - before))
        if differing(t0, full_tables(m)) != changes:
            bad.append("%s: the call that got through changed %s" % (name, differing(t0, full_tables(m))))
    m.close()
    if counts != [2, 2, 2, 2, 1]:                          # the lists and the stage; the derive's list
        bad.append("refusals %s" % counts)
    log("state update refusals: %s refused; problems: %s" % (" + ".join(str(c) for c in counts), bad or "none"), flush=True)
    return bad


def check_group(log=print, devices=(0, 0, 0)):
    """Three shards on one device next to one context, behind a step: all five entries, the listed get with columns that
    interleave the shards, then a record on both."""
    E = cc.quickflux()
    D = E.D
    bad = []
    one, g = (cc.start(model(E, clone(D), **kw), E) for kw in ({}, dict(cls=Group, devices=list(devices))))
    bounds = g.shard_bounds()
    shard = lambda h: np.searchsorted(bounds, D.hru_iparams[C["HPI_CELL"], h], side="right") - 1
    hrus, ice, inc = cap_case(E)
    rng = np.random.default_rng(5)
    weave = rng.permutation(D.nhru)[:401].astype(np.int32)
    sh = shard(weave)
    if len(set(sh.tolist())) != len(devices) or (np.diff(sh) != 0).sum() < 100:
        bad.append("the listed columns do not interleave the shards")
    if len(set(shard(hrus).tolist())) < 2:
        bad.append("the updated HRUs lie in one shard")
    sdr, sir = row_lists(D)
    v = rng.normal(size=(len(sdr), len(weave)))
    iv = rng.integers(0, 9, size=(len(sir), len(weave))).astype(np.int32)
    got = {}
    for name, m in (("one", one), ("group", g)):
        m.dist_prec(0, 1, sync=False)
        m.update_state(layer_rows("SD_ICE"), ice, hrus)
        m.update_state(layer_rows("SD_MOIST"), inc, hrus, mode=ADD)
        m.derive_soil_state(CAP | NODES | LAYERS | FRONTS, hrus)
    ro, rg = cc.run_records(one, 1, 1), cc.run_records(g, 1, 1)                        # the run goes on from the update, on both
    if not same(ro, rg) or not np.isfinite(ro).all() or not ro.any():
        bad.append("the record after the update and the derive")
    for name, m in (("one", one), ("group", g)):
        m.update_state(sdr, v, weave, mode=ADD)
        m.update_state(sir, iv, weave, ints=True)
        m.update_state([C["SD_WDEW"]], np.full((1, D.nhru), 0.01), mode=ADD)         # dense
        m.derive_soil_state(NODES | LAYERS)                                            # dense
        got[name] = (m.get_state_rows(sdr, weave), m.get_state_rows(sir, weave, ints=True), m.get_state_rows(sdr), m.get_state_rows(sir, ints=True))
    tg, t1 = cc.tables(g), cc.tables(one)
    bad += differing(tg, {k: t1[k] for k in tg})
    for k, what in enumerate(("listed get", "listed get, ints", "dense get", "dense get, ints")):
        if not same(got["one"][k], got["group"][k]):
            bad.append(what)
    if not same(got["group"][0], tg["sd"][np.ix_(sdr, weave)]) or not same(got["group"][3], tg["si"][sir]):
        bad.append("the group's get differs from its get_state")
    if same(t1["sd"], E.sd0):
        bad.append("nothing was updated")
    one.close(); g.close()
    log("state update group: bounds %s, differing: %s" % (bounds.tolist(), bad or "none"), flush=True)
    return bad


# ------------------------------------------------------------------------------------------------ 10. a larger case
def check_large(log=print, stage_mb=None, tol=CPU_TOL):
    """4 members x 2 000 cells x 6 HRUs (QUICK_FLUX): 12 rows of three members set, added to and read back, then a derive over
    all 48 000 HRUs against np_derive."""
    E = cc.ensemble(dict(FULL_ENERGY=1, Nband=3), 2000, 4, 2, 1, 80)
    D = E.D
    hrus = cu.hrus_of(D, cu.member_cells(E, [1, 2, 3]))
    Nn = D.opt.Nnode
    rows = np.concatenate([layer_rows("SD_MOIST"), layer_rows("SD_ICE"), [C["SD_SNOW_SWQ"], C["SD_SNOW_DEPTH"], C["SD_WDEW"], C["SD_TSURF"], C["SD_SNOW_SURF_TEMP"]],
                           [abi.sd_node(C["SDN_T"], 0, Nn)]]).astype(np.int32)
    rng = np.random.default_rng(9)
    m = begin(model(E, clone(D), stage_mb), E)
    sd, si = E.sd0.copy(), E.si0.copy()
    v = sd[np.ix_(rows, hrus)] * rng.uniform(0.8, 1.3, size=(len(rows), len(hrus)))
    v[11] = rng.uniform(-6.0, 4.0, size=len(hrus))
    a = rng.uniform(0.0, 0.4, size=v.shape); a[9:] = 0.0
    m.update_state(rows, v, hrus)
    m.update_state(rows, a, hrus, mode=ADD)
    sd[np.ix_(rows, hrus)] = v + a
    bad = []
    if len(rows) != 12 or len(hrus) != 36000:
        bad.append("the case: %d rows x %d HRUs" % (len(rows), len(hrus)))
    if not same(m.get_state_rows(rows, hrus), sd[np.ix_(rows, hrus)]) or not same(m.get_state()[0], sd):
        bad.append("update or get")
    fx = m.get_fluxes()
    m.derive_soil_state(CAP | NODES | LAYERS | FRONTS)
    got = m.get_state()
    m.close()
    want = np_derive(D, sd, si, fx, CAP | NODES | LAYERS | FRONTS)
    # SD_LAYER_T1..2 of the quick-flux form are CP_AVG_TEMP minus a product of the same size (soil_conduction.c:655-659); among
    # 8 000 distinct cells some land within 0.01 C of zero, where the last-ulp differences of exp between the device, glibc and
    # numpy are 1e-12 of the result and 1e-15 of its terms.  Those rows are measured against a floor of 1 C, the size of the
    # terms; every other row as in the fixture comparisons.
    lt = layer_rows("SD_LAYER_T")
    other = np.setdiff1d(np.arange(sd.shape[0]), lt)
    w = max(worst(want[0][other], got[0][other]), float(rel_diff(want[0][lt], got[0][lt], 1.0).max()))
    if not w < tol or not np.array_equal(want[1], got[1]) or same(want[0], sd):
        bad.append("the derive: worst %.3e" % w)
    log("state update large (stage %s MB): %d rows x %d HRUs, derive over %d HRUs: worst %.3e, differing: %s" % (stage_mb or "default", len(rows), len(hrus), D.nhru, w, bad or "none"), flush=True)
    return bad


if __name__ == "__main__":
    cmd = sys.argv[1]
    if cmd == "errors":
        problems, _ = error_returns()
    else:
        both_chunkings = lambda: check_midrun(chunks="1") + check_midrun(chunks="2")
        problems = {"initial": check_initial, "stepped": check_stepped, "selfcheck": check_selfcheck, "cap": check_cap, "rows": check_rows, "midrun": both_chunkings,
                    "errorpath": check_errorpath, "zeroarea": check_zeroarea, "untouched": check_untouched, "refusals": check_refusals, "group": check_group,
                    "large": check_large}[cmd]()
    print("state update %s: problems: %s" % (cmd, problems or "none"), flush=True)
    sys.exit(1 if problems else 0)
