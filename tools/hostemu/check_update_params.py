"""Cell and HRU parameters updated in place (vicgpu_update_cell_params / vicgpu_update_hru_params and their group forms,
include/vicgpu.h) against a second model that takes the updated tables through vicgpu_set_domain.  Every comparison is bit
for bit.  Run by tests/test_update_params.py with VICGPU_LIB pointing at the unsanitized host build (SAN=none
tools/hostemu/build.sh); tests/test_update_params_gpu.py imports the functions for the GPU.
    python tools/hostemu/check_update_params.py start        members 1 and 3 updated before the run: listed, dense, one row per pass
    python tools/hostemu/check_update_params.py derived      the soil-conductivity rows of cell 0 follow its updated soil rows
    python tools/hostemu/check_update_params.py treeline     HPD_CV and CPB_ABOVETREELINE, before and after put_data_config
    python tools/hostemu/check_update_params.py midrun       FROZEN_SOIL as one chunk and as two, right behind a two-step vicgpu_step
    python tools/hostemu/check_update_params.py untouched    what a call must leave alone
    python tools/hostemu/check_update_params.py errors       every error return, each leaving every table as it was
    python tools/hostemu/check_update_params.py refusals     the n-th allocation refused, for every n
    python tools/hostemu/check_update_params.py group        3 shards on device 0 next to one context
Each prints "update params <name>: problems: none" (or the list) and exits with 1 when there are any."""
import copy
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import check_copy_cells as cc
from vic_amd import abi
from vic_amd.abi import C
from vic_amd.api import Group, Model, VicGpuError, load_library

R = cc.R
STAGE = cc.STAGE
same, differing = cc.same, cc.differing
TREE_OUT = ["OUT_SWE", "OUT_EVAP", "OUT_SNOW_DEPTH_BAND"]


def clone(D):
    """The domain with parameter tables of its own: Model.update_*_params keeps the tables of its domain in step."""
    d = copy.copy(D)
    d.cell_params = D.cell_params.copy()
    d.hru_dparams = D.hru_dparams.copy()
    return d


def model(E, D, stage_mb=None, cls=Model, **kw):
    """A model of domain D (the staging budget is read when the domain is set); nothing else is set yet."""
    os.environ.pop(STAGE, None)
    if stage_mb is not None:
        os.environ[STAGE] = stage_mb
    m = cls(D, **kw)
    os.environ.pop(STAGE, None)
    return m


def member_cells(E, members):
    return np.concatenate([m * E.ncol + np.arange(E.ncol) for m in members]).astype(np.int32)


def hrus_of(D, cells):
    off, lst = D.cell_hru_offset, D.cell_hru_list
    return np.concatenate([lst[off[c]:off[c + 1]] for c in cells]).astype(np.int32)


def soil_rows():
    rows = [C["CP_B_INFILT"], C["CP_DS"]]
    for f in ("CPL_DEPTH", "CPL_MAX_MOIST", "CPL_QUARTZ", "CPL_BULK_DENSITY"):
        rows += [abi.cp_layer(C[f], l) for l in range(3)]
    return np.array(rows, np.int32)


def generation(D, cells, k=1.0):
    """New values of the soil rows for `cells`: (rows, values [nrow][n]), every cell its own factor."""
    rows = soil_rows()
    v = D.cell_params[np.ix_(rows, cells)].copy()
    w = 1.0 + 0.05 * k * (1 + np.arange(len(cells)) % 4)            # 1.05 .. 1.20
    v[0] *= 1.3 * w; v[1] *= 0.7 / w
    v[2:5] *= w; v[5:8] *= w * 0.97                                 # depth; max_moist with the new depth and porosity
    v[8:11] *= 0.8; v[11:14] *= 0.97
    return rows, np.ascontiguousarray(v)


def root_update(D, cells):
    """New root fractions for the HRUs of `cells`: (rows, hrus, values [3][n])"""
    hrus = hrus_of(D, cells)
    rows = np.array([C["HPD_ROOT0"], C["HPD_ROOT1"], C["HPD_ROOT2"]], np.int32)
    v = np.empty((3, len(hrus)))
    v[0], v[1], v[2] = np.float32(0.25), np.float32(0.55), np.float32(0.20)
    return rows, hrus, v


def applied(D, cell_updates=(), hru_updates=()):
    """A clone of D with the updates written into its tables by numpy: what vicgpu_set_domain takes on the expected path."""
    d = clone(D)
    for rows, cols, v in cell_updates:
        d.cell_params[np.ix_(rows, cols)] = v
    for rows, cols, v in hru_updates:
        d.hru_dparams[np.ix_(rows, cols)] = v
    return d


def all_names(m):
    return [n for n, _, _ in m.output_list()]


def records(m, step0, nrec, names):
    m.records_config(names, depth=2)
    rec = m.run_records(step0, nrec)
    rec.wait()
    out = rec.out.copy()
    del rec
    return out


def params_held(m, D):
    """the getters against the tables of D"""
    bad = []
    if not same(m.get_cell_params(), D.cell_params):
        bad.append("get_cell_params differs from the updated table")
    if not same(m.get_hru_params(), D.hru_dparams):
        bad.append("get_hru_params differs from the updated table")
    if not same(m.dom.cell_params, D.cell_params) or not same(m.dom.hru_dparams, D.hru_dparams):
        bad.append("the model's host tables were not kept in step")
    return bad


# ------------------------------------------------------------------------------------------------ 1. from the start
def start_case(E=None):
    E = E or cc.quickflux()
    cells = member_cells(E, [1, 3])
    cu = generation(E.D, cells)
    hr, hh, hv = root_update(E.D, member_cells(E, [1]))
    E.up_cells, E.up_cell = cells, (cu[0], cells, cu[1])
    E.up_hru = (hr, hh, hv)
    E.mixed = applied(E.D, [E.up_cell], [E.up_hru])
    return E


def run_start(E, how, log=print):
    """how: 'listed', 'dense', 'row_per_pass' (listed, VICGPU_COPY_STAGE_MB=0), 'set_domain' (the expected path), 'none' (no
    update).  Returns (tables, records of all variables, problems)."""
    bad = []
    if how == "set_domain":
        m = model(E, clone(E.mixed))
    else:
        m = model(E, clone(E.D), stage_mb="0" if how == "row_per_pass" else None)
        if how in ("listed", "row_per_pass"):
            rows, cells, v = E.up_cell
            m.update_cell_params(rows, v, cells)
            rows, hrus, v = E.up_hru
            m.update_hru_params(rows, v, hrus)
        elif how == "dense":
            m.update_cell_params(np.arange(E.mixed.cell_params.shape[0]), E.mixed.cell_params)
            m.update_hru_params(np.arange(C["HPD_NROW"]), E.mixed.hru_dparams)
        if how != "none":
            bad += params_held(m, E.mixed)
    cc.start(m, E)
    rec = records(m, 0, 2, all_names(m))
    t = cc.tables(m)
    m.close()
    return t, rec, bad


def check_start(log=print):
    E = start_case()
    bad = []
    if len(E.up_cells) != 70:
        bad.append("the update lists %d cells, not 70" % len(E.up_cells))
    want_t, want_r, _ = run_start(E, "set_domain")
    none_t, none_r, _ = run_start(E, "none")
    for m in (1, 3):
        c = slice(m * E.ncol, (m + 1) * E.ncol)
        if same(want_r[..., c], none_r[..., c]):
            bad.append("member %d: the records with and without the update do not differ" % m)
    for m in (0, 2):
        c = slice(m * E.ncol, (m + 1) * E.ncol)
        if not same(want_r[..., c], none_r[..., c]):
            bad.append("member %d: its records changed although it was not updated" % m)
    if not (np.isfinite(want_r[np.isfinite(none_r)]).all() and want_r.any()):
        bad.append("the expected records are not finite or all zero")
    for how in ("listed", "dense", "row_per_pass"):
        t, r, b = run_start(E, how)
        d = b + differing(want_t, t) + ([] if same(r, want_r) else ["the records"])
        log("update params start %s: %d cells x %d HRUs, %d record rows, differing: %s" % (how, E.D.ncell, E.D.nhru, r.shape[1], d or "none"), flush=True)
        bad += ["%s: %s" % (how, x) for x in d]
    return bad


# ------------------------------------------------------------------------------------------------ 2. derived rows, directly
def check_derived(log=print):
    E = cc.quickflux()
    m = model(E, clone(E.D))
    D = m.dom
    rng = np.random.default_rng(5)
    n = 96
    moist = rng.uniform(0.0, 0.45, n)
    moist[:4] = 0.0
    Wu = np.where(rng.uniform(size=n) < 0.5, moist, moist * rng.uniform(0.05, 1.0, n))
    fields = ("CPL_SOIL_DENS_MIN", "CPL_BULK_DENS_MIN", "CPL_QUARTZ", "CPL_SOIL_DENSITY", "CPL_BULK_DENSITY", "CPL_ORGANIC")

    def derived(l):
        b = np.zeros((n, 10)); b[:, 0] = moist; b[:, 1] = Wu; b[:, 2] = l
        return m.debug_pure(C["VICGPU_PURE_SOIL_CONDUCTIVITY_DERIVED"], b)

    def direct(l):
        a = np.zeros((n, 10)); a[:, 0] = moist; a[:, 1] = Wu
        for j, f in enumerate(fields):
            a[:, 2 + j] = D.cell_params[abi.cp_layer(C[f], l), 0]
        return m.debug_pure(C["VICGPU_PURE_SOIL_CONDUCTIVITY"], a)

    bad = []
    before = [derived(l) for l in range(3)]
    rows = np.array([abi.cp_layer(C[f], l) for f in fields for l in range(3)], np.int32)
    v = D.cell_params[rows, 0].copy().reshape(-1, 1)
    new = {"CPL_QUARTZ": (0.15, 0.45, 0.85), "CPL_ORGANIC": (0.12, 0.05, 0.0), "CPL_BULK_DENSITY": (1350.0, 1480.0, 1570.0),
           "CPL_BULK_DENS_MIN": (1420.0, 1500.0, 1590.0), "CPL_SOIL_DENSITY": (2500.0, 2600.0, 2685.0), "CPL_SOIL_DENS_MIN": (2650.0, 2660.0, 2700.0)}
    for j, f in enumerate(fields):
        v[3 * j:3 * j + 3, 0] = new[f]
    m.update_cell_params(rows, v, [0])
    for l in range(3):
        got, want = derived(l), direct(l)
        if not same(got, want):
            bad.append("layer %d: the derived rows do not follow the updated soil rows" % l)
        if same(got, before[l]):
            bad.append("layer %d: the derived conductivity did not change" % l)
        if not np.isfinite(want).all():
            bad.append("layer %d: the conductivity is not finite" % l)
    # cell 1, not listed, keeps the caller's rows
    cp = m.get_cell_params()
    if not same(cp[:, 1:], E.D.cell_params[:, 1:]) or not same(cp[rows, 0], v[:, 0]):
        bad.append("the table after the update")
    m.close()
    log("update params derived: differing: %s" % (bad or "none"), flush=True)
    return bad


# ------------------------------------------------------------------------------------------------ 3. tree line
def treeline_case():
    """The quickflux ensemble with the top band above the tree line in a third of the base cells (every member), and two
    updates: HPD_CV of member 1's top-band HRUs (half of the overstory HRU's fraction goes to the band's first open HRU: the
    band's sum stays), and CPB_ABOVETREELINE of member 3's cells flipped."""
    E = cc.quickflux()
    D = E.D
    Nn, Nb = D.opt.Nnode, D.opt.Nband
    top = Nb - 1
    atl_row = abi.cp_band(C["CPB_ABOVETREELINE"], top, Nn, Nb)
    D.cell_params[atl_row, (np.arange(D.ncell) % E.ncol) % 3 == 0] = 1.0
    over = D.veglib[D.hru_iparams[C["HPI_VEG_INDEX"]], C["VL_OVERSTORY"]] != 0
    band = D.hru_iparams[C["HPI_BAND"]]
    hrus, vals = [], []
    for c in member_cells(E, [1]):
        h = hrus_of(D, [c])
        h = h[band[h] == top]
        ho, hn = h[over[h]], h[~over[h]]
        assert len(ho) >= 1 and len(hn) >= 1
        delta = 0.5 * D.hru_dparams[C["HPD_CV"], ho[0]]
        hrus += [ho[0], hn[0]]
        vals += [D.hru_dparams[C["HPD_CV"], ho[0]] - delta, D.hru_dparams[C["HPD_CV"], hn[0]] + delta]
    E.tree_overstory = bool(over[band == top].any())
    E.up_hru = (np.array([C["HPD_CV"]], np.int32), np.array(hrus, np.int32), np.array(vals)[None, :])
    cells = member_cells(E, [3])
    E.up_cell = (np.array([atl_row], np.int32), cells, (1.0 - D.cell_params[atl_row, cells])[None, :])
    E.mixed = applied(D, [E.up_cell], [E.up_hru])
    return E


def run_treeline(E, how):
    """how: 'before' / 'after' vicgpu_put_data_config, 'set_domain', 'none'"""
    m = model(E, clone(E.mixed if how == "set_domain" else E.D))

    def update():
        rows, hrus, v = E.up_hru
        m.update_hru_params(rows, v, hrus)            # the first call: tree rows of the owners of the listed HRUs
        rows, cells, v = E.up_cell
        m.update_cell_params(rows, v, cells)          # the second call: tree rows of the listed cells

    if how == "before":
        update()
    cc.start(m, E)
    if how == "after":
        update()
    m.put_data_init()                                 # the bookkeeping starts from the HRU fractions in force, on every path
    bad = params_held(m, E.mixed) if how in ("before", "after") else []
    rec = records(m, 0, 2, TREE_OUT)
    t = cc.tables(m)
    m.close()
    return t, rec, bad


def check_treeline(log=print):
    E = treeline_case()
    bad = [] if E.tree_overstory else ["no overstory HRU in the top band"]
    want_t, want_r, _ = run_treeline(E, "set_domain")
    _, none_r, _ = run_treeline(E, "none")
    for m in (1, 3):
        c = slice(m * E.ncol, (m + 1) * E.ncol)
        if same(want_r[..., c], none_r[..., c]):
            bad.append("member %d: the records with and without the update do not differ" % m)
    if not (np.isfinite(want_r).all() and want_r.any()):
        bad.append("the expected records are not finite or all zero")
    for how in ("before", "after"):
        t, r, b = run_treeline(E, how)
        d = b + differing(want_t, t) + ([] if same(r, want_r) else ["the records"])
        log("update params treeline %s put_data_config: differing: %s" % (how, d or "none"), flush=True)
        bad += ["%s: %s" % (how, x) for x in d]
    return bad


# ------------------------------------------------------------------------------------------------ 4. mid-run, finite differences
def check_midrun(log=print, chunks="2"):
    """FROZEN_SOIL, 10 nodes, 2 bands, glacier HRUs, 5 base cells x 2 members (chunk boundary = member boundary): cells on both
    sides of the boundary are updated right behind a two-step vicgpu_step that was not waited for; two more steps follow.
    The expected path makes the change through the host: state and fluxes out, vicgpu_set_domain, state, fluxes and forcing in."""
    os.environ["VICGPU_CHUNKS"] = chunks
    try:
        E = cc.ensemble(dict(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=10, Nband=2, frozen_compat=0), 5, 2, 2, 4, 330, glacier=True)
        D = E.D
        glac = D.hru_iparams[C["HPI_IS_GLACIER"]] != 0
        if not glac.any():
            return ["no glacier HRU in the domain"]
        cells = np.array([1, 3, 4, 5, 8], np.int32)
        rows, v = generation(D, cells, k=0.4)
        # the glacier retreats in the listed cells: a fifth of every glacier HRU's fraction goes to the other HRU of its band
        hrus, vals = [], []
        band = D.hru_iparams[C["HPI_BAND"]]
        for c in cells:
            h = hrus_of(D, [c])
            for g in h[glac[h]]:
                o = [x for x in h if band[x] == band[g] and not glac[x]][0]
                delta = 0.2 * D.hru_dparams[C["HPD_CV"], g]
                hrus += [g, o]
                vals += [D.hru_dparams[C["HPD_CV"], g] - delta, D.hru_dparams[C["HPD_CV"], o] + delta]
        up_hru = (np.array([C["HPD_CV"]], np.int32), np.array(hrus, np.int32), np.array(vals)[None, :])
        mixed = applied(D, [(rows, cells, v)], [up_hru])
        keys = ("sd", "si", "flux", "cell_out")

        def begin(m):
            m.set_forcing_map(E.cell_col, E.ncol)
            m.set_state(E.sd0, E.si0)
            m.push_forcing(E.f, E.sf, E.dmy)

        a, b, n = model(E, clone(D)), model(E, clone(D)), model(E, clone(D))
        for m in (a, b, n):
            begin(m)
        a.dist_prec(0, 2, sync=False)
        a.update_cell_params(rows, v, cells)
        a.update_hru_params(up_hru[0], up_hru[2], up_hru[1])
        a.dist_prec(2, 2)
        b.dist_prec(0, 2)
        sd, si = b.get_state()
        fx = b.get_fluxes()
        b.set_domain(clone(mixed))
        b.set_forcing_map(E.cell_col, E.ncol)
        b.set_state(sd, si)
        b.set_fluxes(fx)
        b.push_forcing(E.f, E.sf, E.dmy)
        b.dist_prec(2, 2)
        n.dist_prec(0, 4)
        ta, tb, tn = cc.tables(a, put=False), cc.tables(b, put=False), cc.tables(n, put=False)
        bad = ["after the steps: " + k for k in keys if not same(ta[k], tb[k])]
        bad += params_held(a, mixed)
        if same(tb["sd"], tn["sd"]):
            bad.append("the run with the update does not differ from the run without")
        if not np.isfinite(tb["cell_out"]).all():
            bad.append("the expected cell outputs are not finite")
        for m in (a, b, n):
            m.close()
    finally:
        os.environ.pop("VICGPU_CHUNKS", None)
    log("update params midrun (chunks %s): differing: %s" % (chunks, bad or "none"), flush=True)
    return bad


# ------------------------------------------------------------------------------------------------ 5. untouched
def check_untouched(log=print):
    """Around a mid-run update with put_data, records and cell groups configured: every table the contract names as untouched,
    the configuration, and the columns of the parameter tables that are not listed."""
    E = start_case()
    bad = []
    m = model(E, clone(E.D))
    cc.start(m, E)
    m.records_config(cc.OUT, depth=2)
    off = np.arange(0, E.D.ncell + 1, E.ncol, dtype=np.int32)           # a group per member
    m.records_set_groups(off, np.arange(E.D.ncell, dtype=np.int32))
    valid = np.ones(E.D.ncell, np.int32)
    valid[2 * E.ncol + 3] = 0
    m.dist_prec(0, 2)
    m.set_cell_valid(valid)

    def snapshot():
        t = cc.tables(m)
        t["forcing"], t["snowflag"] = m.get_forcing(3)
        t["hpi"] = m.dom.hru_iparams.copy()
        t["map"] = m.get_forcing_map()[1]
        cfg = (m.lib.vicgpu_records_nrow(m.h), m.records_ncol(), m.records_get_groups(), m.get_forcing_map()[0])
        return t, cfg, m.get_cell_params(), m.get_hru_params()

    t0, cfg0, cp0, hpd0 = snapshot()
    rows, cells, v = E.up_cell
    m.update_cell_params(rows, v, cells)
    hr, hh, hv = E.up_hru
    m.update_hru_params(hr, hv, hh)
    t1, cfg1, cp1, hpd1 = snapshot()
    bad += [k + " changed" for k in differing(t0, t1)]
    if cfg0 != cfg1:
        bad.append("the records configuration, the groups or the forcing map changed: %s -> %s" % (cfg0, cfg1))
    if m.lib.vicgpu_put_data_init(m.h) != 0:
        bad.append("the put_data configuration is gone")
    rest_c = np.setdiff1d(np.arange(E.D.ncell), cells)
    rest_r = np.setdiff1d(np.arange(cp0.shape[0]), rows)
    if not same(cp0[:, rest_c], cp1[:, rest_c]) or not same(cp0[rest_r], cp1[rest_r]):
        bad.append("cell parameters that were not listed changed")
    if not same(cp1[np.ix_(rows, cells)], v) or same(cp0[np.ix_(rows, cells)], v):
        bad.append("the listed cell parameters do not hold the new values")
    rest_h = np.setdiff1d(np.arange(E.D.nhru), hh)
    rest_hr = np.setdiff1d(np.arange(C["HPD_NROW"]), hr)
    if not same(hpd0[:, rest_h], hpd1[:, rest_h]) or not same(hpd0[rest_hr], hpd1[rest_hr]):
        bad.append("HRU parameters that were not listed changed")
    if not same(hpd1[np.ix_(hr, hh)], hv) or same(hpd0[np.ix_(hr, hh)], hv):
        bad.append("the listed HRU parameters do not hold the new values")
    # the run goes on: a record over the groups
    rec = m.run_records(2, 1)
    rec.wait()
    if rec.out.shape[-1] != E.M or not np.isfinite(rec.out).all() or not rec.out.any():
        bad.append("the record after the update")
    del rec
    m.close()
    log("update params untouched: differing: %s" % (bad or "none"), flush=True)
    return bad


# ------------------------------------------------------------------------------------------------ 6. errors
def error_returns(log=print):
    """Every VICGPU_ERR_ARG / VICGPU_ERR_STATE return of the header, each followed by a comparison of all tables.  All of them
    are refused on the host before any launch."""
    lib = load_library()
    ARG, ST, OK = C["VICGPU_ERR_ARG"], C["VICGPU_ERR_STATE"], 0
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    i32 = lambda x: np.asarray(x, dtype=np.int32)

    def call(fn, h, rows, cols, values=0.5, nrow=None, n=None):
        r = None if rows is None else i32(rows)
        c = None if cols is None else i32(cols)
        nrow = (len(r) if r is not None else 0) if nrow is None else nrow
        n = (len(c) if c is not None else 0) if n is None else n
        v = None if values is None else np.full(max(nrow, 1) * max(n, 1), float(values))
        return fn(h, nrow, r.ctypes.data_as(ip) if r is not None else None, n, c.ctypes.data_as(ip) if c is not None else None,
                  v.ctypes.data_as(dp) if v is not None else None)

    E = cc.quickflux()
    D = clone(E.D)
    nc, nh, ncp, nhp = D.ncell, D.nhru, D.cell_params.shape[0], C["HPD_NROW"]
    checks = []

    def every_case(tag, uc, uh, h, tables):
        t0 = tables()
        cases = []
        for fn, name, nrows, ncols in ((uc, "cell", ncp, nc), (uh, "hru", nhp, nh)):
            cases += [
                ("null rows", lambda: call(fn, h, None, [1], nrow=1), ARG),
                ("null values", lambda: call(fn, h, [1], [1], values=None), ARG),
                ("nrow < 0", lambda: call(fn, h, [1], [1], nrow=-1), ARG),
                ("n < 0", lambda: call(fn, h, [1], [1], n=-1), ARG),
                ("row == nrows", lambda: call(fn, h, [0, nrows], [1]), ARG),
                ("row < 0", lambda: call(fn, h, [-1], [1]), ARG),
                ("a row listed twice", lambda: call(fn, h, [2, 1, 2], [1]), ARG),
                ("column == ncol", lambda: call(fn, h, [1], [0, ncols]), ARG),
                ("column < 0", lambda: call(fn, h, [1], [3, -1]), ARG),
                ("a column listed twice", lambda: call(fn, h, [1], [5, 70, 5]), ARG),
                ("... after legal rows and columns", lambda: call(fn, h, [0, 1, 2], [0, 1, 2, 140, 1]), ARG),
                ("no list, n == ncol - 1", lambda: call(fn, h, [1], None, n=ncols - 1), ARG),
                ("no list, n == ncol + 1", lambda: call(fn, h, [1], None, n=ncols + 1), ARG),
                ("no list, n == 1", lambda: call(fn, h, [1], None, n=1), ARG),
            ]
            cases = [("%s%s: %s" % (tag, name, w), f, want) if not w.startswith(tag) else (w, f, want) for w, f, want in cases]
        for w, f, want in cases:
            checks.append((w, f(), want))
            d = differing(t0, tables())
            checks.append((w + ": tables", d or "unchanged", "unchanged"))
        noops = [("nrow == 0", lambda fn: call(fn, h, [], [1, 2])), ("n == 0", lambda fn: call(fn, h, [1, 2], [])),
                 ("nrow == 0, null rows and values", lambda fn: call(fn, h, None, [1], values=None)),
                 ("n == 0, null list", lambda fn: call(fn, h, [1], None, n=0))]
        for w, f in noops:
            for fn, name in ((uc, "cell"), (uh, "hru")):
                checks.append(("%s%s: %s" % (tag, name, w), f(fn), OK))
        checks.append((tag + "tables after the no-ops", differing(t0, tables()) or "unchanged", "unchanged"))

    def full_tables(m):
        def f():
            t = cc.tables(m)
            t["cp"], t["hpd"] = m.get_cell_params(), m.get_hru_params()
            return t
        return f

    uc, uh, gc, gh = lib.vicgpu_update_cell_params, lib.vicgpu_update_hru_params, lib.vicgpu_get_cell_params, lib.vicgpu_get_hru_params
    for fn in (uc, uh):
        checks.append(("null handle", call(fn, None, [1], [1]), ARG))
        checks.append(("null handle, nothing to do", call(fn, None, [], []), ARG))
    buf = np.zeros(8)
    checks += [("get_cell_params: null handle", gc(None, buf.ctypes.data_as(dp)), ARG), ("get_hru_params: null handle", gh(None, buf.ctypes.data_as(dp)), ARG)]
    fresh = ctypes.c_void_p()
    assert lib.vicgpu_create(ctypes.byref(D.opt), 0, ctypes.byref(fresh)) == 0
    checks += [("no domain: cell", call(uc, fresh, [1], [1]), ST), ("no domain: hru", call(uh, fresh, [1], [1]), ST),
               ("no domain: nothing to do", call(uc, fresh, [], []), ST),
               ("no domain: get_cell_params", gc(fresh, buf.ctypes.data_as(dp)), ST), ("no domain: get_hru_params", gh(fresh, buf.ctypes.data_as(dp)), ST)]
    lib.vicgpu_destroy(fresh)
    m = model(E, D)
    cc.start(m, E)
    m.dist_prec(0, 1)
    checks += [("get_cell_params: null table", gc(m.h, None), ARG), ("get_hru_params: null table", gh(m.h, None), ARG)]
    every_case("", uc, uh, m.h, full_tables(m))
    try:
        m.update_cell_params([1, 1], np.zeros((2, 1)), [0])
        checks.append(("Model.update_cell_params raises", False, True))
    except VicGpuError as e:
        checks.append(("Model.update_cell_params raises with the rule", "listed twice" in str(e), True))
    checks.append(("... and leaves the host table", same(m.dom.cell_params, E.D.cell_params), True))
    m.close()
    # the group
    g = model(E, clone(E.D), cls=Group, devices=[0, 0, 0])
    cc.start(g, E)
    guc, guh = lib.vicgpu_group_update_cell_params, lib.vicgpu_group_update_hru_params
    for fn in (guc, guh):
        checks.append(("group: null handle", call(fn, None, [1], [1]), ARG))
    checks += [("group: get_cell_params null handle", lib.vicgpu_group_get_cell_params(None, buf.ctypes.data_as(dp)), ARG),
               ("group: get_hru_params null table", lib.vicgpu_group_get_hru_params(g.h, None), ARG)]
    every_case("group: ", guc, guh, g.h, full_tables(g))
    fresh = ctypes.c_void_p()
    dev = i32([0, 0])
    assert lib.vicgpu_group_create(ctypes.byref(D.opt), 2, dev.ctypes.data_as(ip), ctypes.byref(fresh)) == 0
    checks += [("group: no domain", call(guc, fresh, [1], [1]), ST), ("group: no domain, hru", call(guh, fresh, [1], [1]), ST),
               ("group: no domain, getter", lib.vicgpu_group_get_cell_params(fresh, buf.ctypes.data_as(dp)), ST)]
    lib.vicgpu_group_destroy(fresh)
    g.close()
    failed = [(w, got, want) for w, got, want in checks if got != want]
    for w, got, want in failed:
        log("update params return: %s gave %s, want %s" % (w, got, want), flush=True)
    log("update params errors: %d checks, failed: %d" % (len(checks), len(failed)), flush=True)
    return ["%s gave %s" % (w, got) for w, got, _ in failed], len(checks)


def check_refusals(log=print):
    """The update entries under a runtime that refuses their n-th allocation, n = 1, 2, ...: VICGPU_ERR_HIP, no live runtime
    object added and every table as it was, until the call gets through -- which leaves no object behind either."""
    lib = load_library()
    lib.hostemu_live_objects.restype = ctypes.c_longlong
    lib.hostemu_refuse_alloc.argtypes = [ctypes.c_longlong]
    ip, dp = ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double)
    E = start_case()
    bad, counts = [], {}
    for name in ("cell", "hru"):
        m = model(E, clone(E.D))
        cc.start(m, E)
        m.dist_prec(0, 1)
        rows, cols, v = E.up_cell if name == "cell" else (E.up_hru[0], E.up_hru[1], E.up_hru[2])
        rows, cols, v = np.ascontiguousarray(rows, np.int32), np.ascontiguousarray(cols, np.int32), np.ascontiguousarray(v)
        fn = lib.vicgpu_update_cell_params if name == "cell" else lib.vicgpu_update_hru_params

        def tables():
            t = cc.tables(m)
            t["cp"], t["hpd"] = m.get_cell_params(), m.get_hru_params()
            return t

        t0 = tables()
        before = lib.hostemu_live_objects()
        for n in range(1, 20):
            lib.hostemu_refuse_alloc(n)
            rc = fn(m.h, len(rows), rows.ctypes.data_as(ip), len(cols), cols.ctypes.data_as(ip), v.ctypes.data_as(dp))
            lib.hostemu_refuse_alloc(0)
            if rc == 0:
                break
            if rc != C["VICGPU_ERR_HIP"] or lib.hostemu_live_objects() != before or differing(t0, tables()):
                bad.append("%s, allocation %d refused: code %d, %d objects more, changed %s"
                           % (name, n, rc, lib.hostemu_live_objects() - before, differing(t0, tables())))
        counts[name] = n - 1
        if lib.hostemu_live_objects() != before:
            bad.append("%s: %d objects left by the call that got through" % (name, lib.hostemu_live_objects() - before))
        if differing(t0, tables()) != ["cp" if name == "cell" else "hpd"]:
            bad.append("%s: the call that got through changed %s" % (name, differing(t0, tables())))
        m.close()
    if counts != {"cell": 2, "hru": 2}:                    # the lists and the stage
        bad.append("refusals %s" % counts)
    log("update params refusals: %d + %d refused; problems: %s" % (counts["cell"], counts["hru"], bad or "none"), flush=True)
    return bad


# ------------------------------------------------------------------------------------------------ 7. group
def check_group(log=print, devices=(0, 0, 0)):
    """Three shards on one device next to one context, behind a step: the listed update of members 1 and 3 and of member 1's
    HRUs (cells and HRUs of every shard), then the dense update back to a third table; every table and the getters equal, then
    a record on both."""
    E = start_case()
    bad = []
    one, g = model(E, clone(E.D)), model(E, clone(E.D), cls=Group, devices=list(devices))
    bounds = g.shard_bounds()
    shard = lambda c: np.searchsorted(bounds, c, side="right") - 1
    if len(set(shard(E.up_cells).tolist())) != len(devices):
        bad.append("the listed cells do not reach every shard")
    if len(set(shard(E.D.hru_iparams[C["HPI_CELL"], E.up_hru[1]]).tolist())) < 2:
        bad.append("the listed HRUs lie in one shard")
    others = member_cells(E, [0, 2])
    rows, v = generation(E.mixed, others, k=0.5)
    third = applied(E.mixed, [(rows, others, v)])
    for m in (one, g):
        cc.start(m, E)
        m.dist_prec(0, 1, sync=False)
        rows, cells, v = E.up_cell
        m.update_cell_params(rows, v, cells)
        rows, hrus, v = E.up_hru
        m.update_hru_params(rows, v, hrus)

    def compare(when, want):
        tg, t1 = cc.tables(g), cc.tables(one)
        d = [when + ": " + k for k in differing(tg, {k: t1[k] for k in tg})]
        d += [when + ": group: " + x for x in params_held(g, want)] + [when + ": context: " + x for x in params_held(one, want)]
        return d

    bad += compare("after the listed update", E.mixed)
    ro, rg = cc.run_records(one, 1, 1), cc.run_records(g, 1, 1)
    if not same(ro, rg):
        bad.append("the record after the listed update")
    for m in (one, g):
        m.update_cell_params(np.arange(third.cell_params.shape[0]), third.cell_params)
        m.update_hru_params(np.arange(C["HPD_NROW"]), third.hru_dparams)
    bad += compare("after the dense update", third)
    ro2, rg2 = cc.run_records(one, 1 + R, 1), cc.run_records(g, 1 + R, 1)
    if not same(ro2, rg2):
        bad.append("the record after the dense update")
    if not (np.isfinite(ro).all() and ro.any() and np.isfinite(ro2).all()):
        bad.append("the context's records are not finite or all zero")
    one.close(); g.close()
    log("update params group: bounds %s, differing: %s" % (bounds.tolist(), bad or "none"), flush=True)
    return bad


# ------------------------------------------------------------------------------------------------ 8. a larger case
def check_large(log=print, stage_mb=None):
    """4 members x 2 000 cells (QUICK_FLUX, 6 HRUs a cell): all CP rows of three members, against vicgpu_set_domain: the
    tables, the derived rows through a step, and the getters."""
    E = cc.ensemble(dict(FULL_ENERGY=1, Nband=3), 2000, 4, 2, 1, 80)
    cells = member_cells(E, [1, 2, 3])
    rows = np.arange(E.D.cell_params.shape[0], dtype=np.int32)
    v = E.D.cell_params[:, cells].copy()
    sr, sv = generation(E.D, cells)
    v[sr] = sv
    mixed = applied(E.D, [(rows, cells, v)])
    a, b = model(E, clone(E.D), stage_mb), model(E, clone(mixed))
    a.update_cell_params(rows, v, cells)
    bad = params_held(a, mixed)
    for m in (a, b):
        m.set_forcing_map(E.cell_col, E.ncol)
        m.set_state(E.sd0, E.si0)
        m.push_forcing(E.f, E.sf, E.dmy)
        m.dist_prec(0, 1)
    ta, tb = cc.tables(a, put=False), cc.tables(b, put=False)
    bad += differing(tb, ta)
    if not np.isfinite(tb["cell_out"]).all() or same(tb["sd"], E.sd0):
        bad.append("the step of the expected path")
    a.close(); b.close()
    log("update params large (stage %s MB): %d rows x %d cells, differing: %s" % (stage_mb or "default", len(rows), len(cells), bad or "none"), flush=True)
    return bad


if __name__ == "__main__":
    cmd = sys.argv[1]
    if cmd == "errors":
        problems, _ = error_returns()
    else:
        both_chunkings = lambda: check_midrun(chunks="1") + check_midrun(chunks="2")
        problems = {"start": check_start, "derived": check_derived, "treeline": check_treeline, "midrun": both_chunkings, "untouched": check_untouched,
                    "refusals": check_refusals, "group": check_group, "large": check_large}[cmd]()
    print("update params %s: problems: %s" % (cmd, problems or "none"), flush=True)
    sys.exit(1 if problems else 0)
