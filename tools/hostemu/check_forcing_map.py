"""The forcing map (vicgpu_set_forcing_map, include/vicgpu.h): an ensemble of M members on `ncol` shared forcing columns
against the same ensemble with the forcing replicated per cell.  Run by tests/test_forcing_map.py with VICGPU_LIB pointing at
the unsanitized host build (SAN=none tools/hostemu/build.sh); tests/test_forcing_map_gpu.py calls the same functions on a GPU.
    python tools/hostemu/check_forcing_map.py run <case> <ncol> <M>
        context A: identity map, forcing replicated along the cell axis; context B: mapped, ncol-wide forcing; from the same
        state, state, fluxes, accumulators, cell outputs, error flags, balance, output data (plain and aggregated), the
        forcing read back (B's columns gathered through the map) and, for the glacier case, the mass-balance fit must be
        bit-identical -- once with the member-major map of domain.tile_members, once with a scrambled map
    python tools/hostemu/check_forcing_map.py raw <ncol> <M>
        vicgpu_prefetch_forcing_raw mapped against replicated, and both against the oracle's derivation
    python tools/hostemu/check_forcing_map.py records <ncol> <M>      run_records with a map against the loop with a map
    python tools/hostemu/check_forcing_map.py group <ncol> <M> <nshard>  a group against one context, both maps
    python tools/hostemu/check_forcing_map.py errors                  every error and lifetime return the header lists
    python tools/hostemu/check_forcing_map.py refusals                the n-th allocation refused, for every n (host build only)"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from vic_amd import abi, domain, init_state
from vic_amd.abi import C
from vic_amd.api import Group, Model, load_library

# forcing echoes (read through the column), the cell's own precipitation, per-band, per-layer and summed variables
OUT = ["OUT_AIR_TEMP", "OUT_PREC", "OUT_REL_HUMID", "OUT_SWE_BAND", "OUT_RUNOFF", "OUT_SOIL_MOIST", "OUT_WIND", "OUT_QAIR"]

CASES = {
    # name: options, tiles, start day, steps, VICGPU_CHUNKS, glacier top band
    "full_energy": (dict(FULL_ENERGY=1, Nband=3), 2, 100, 4, None, False),
    "waterbalance_daily": (dict(FULL_ENERGY=0, dt=24, snow_step=3), 2, 60, 3, None, False),       # NF = 8: the NR slot, the sub-step stride
    "frozen": (dict(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=10, Nband=2, frozen_compat=0), 2, 330, 2, None, False),
    "frozen_chunks": (dict(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=10, Nband=2, frozen_compat=0), 2, 330, 2, "2", False),
    "glacier": (dict(FULL_ENERGY=1, Nband=2), 2, 120, 3, None, True),
}
MAX_SNOW_TEMP = (0.5, 3.0, 1.5)


def perturb(D, ncol, M):
    """Per-member parameters, so that members differ in their results and in their snowflags."""
    Nn, Nb = D.opt.Nnode, D.opt.Nband
    cp = D.cell_params
    for m in range(M):
        s = slice(m * ncol, (m + 1) * ncol)
        cp[C["CP_B_INFILT"], s] *= 1.0 + 0.2 * m
        cp[C["CP_DS"], s] *= 1.0 + 0.3 * m
        cp[C["CP_MAX_SNOW_TEMP"], s] = MAX_SNOW_TEMP[m % 3]
        for b in range(Nb):
            cp[abi.cp_band(C["CPB_TFACTOR"], b, Nn, Nb), s] += 0.4 * m


def scrambled_map(ncell, ncol, seed=20261019):
    """A fixed-seed random assignment of cells to columns: repeats, no order, and column ncol // 2 used by nobody."""
    rng = np.random.default_rng(seed)
    free = ncol // 2
    used = np.array([c for c in range(ncol) if c != free], dtype=np.int32)
    m = used[rng.integers(0, len(used), ncell)]
    assert len(np.unique(m)) < ncell and free not in m
    return np.ascontiguousarray(m)


MAPS = ("member-major", "scrambled")


def build(name, ncol, M, kind):
    """(D, cell_col, f [..][ncol], fA [..][ncell] replicated, sf [..][ncell], dmy, sd0, si0) of a case.  kind: the map --
    "member-major" (domain.tile_members), "scrambled", or "blocked" (consecutive cells share a column, as on a model grid
    finer than its forcing grid: a shard's columns then start past column 0)."""
    kw, ntile, doy, nsteps, chunks, glacier = CASES[name]
    if chunks:
        os.environ["VICGPU_CHUNKS"] = chunks
    else:
        os.environ.pop("VICGPU_CHUNKS", None)
    opt = abi.default_options(**kw)
    base = domain.make_domain(ncol, opt, ntile=ntile, glacier_top_band=glacier)
    f, _, dmy = domain.make_forcing(base, 0, nsteps, start_doy=doy)
    D, cell_col = domain.tile_members(base, M)
    perturb(D, ncol, M)
    if kind != "member-major":
        cell_col = scrambled_map(D.ncell, ncol) if kind == "scrambled" else np.ascontiguousarray((np.arange(D.ncell) * ncol // D.ncell).astype(np.int32))
        fA = np.ascontiguousarray(f[..., cell_col])
    else:
        fA = np.ascontiguousarray(np.tile(f, (1, 1, 1, M)))
    sf = domain.make_snowflag(D, f, cell_col)
    sd0, si0 = init_state.initial_state(D, fA[0])
    if glacier:
        sd0[C["SD_GLAC_CUM_MASS_BALANCE"], D.hru_iparams[C["HPI_IS_GLACIER"]] != 0] = 0.0
    return D, cell_col, f, fA, sf, dmy, sd0, si0


def tables(m, nsteps, glacier=False, cell_col=None):
    """Every table a run leaves; the forcing read back comes gathered through cell_col."""
    grp = isinstance(m, Group)
    r = {}
    r["sd"], r["si"] = m.get_state()
    r["flux"] = m.get_fluxes()
    r["errors"] = m.get_cell_errors()
    r["balance"] = m.get_balance()
    r["out_agg_f32"] = m.get_outputs(OUT, reset=False)
    if not grp:
        r["accum"] = m.get_accum()
        r["cell_out"] = m.get_cell_outputs()
        r["out_data"] = m.get_output_data(OUT, aggregated=False)
        r["out_agg"] = m.get_output_data(OUT, aggregated=True)
        fs = [m.get_forcing(s) for s in range(nsteps)]
        r["forcing"] = np.stack([x[0] if cell_col is None else x[0][..., cell_col] for x in fs])
        r["snowflag"] = np.stack([x[1] for x in fs])
    if glacier:
        r["fit"] = m.glacier_mass_balance_fit(reset=True)
        r["sd_after_fit"] = m.get_state()[0]
    return r


def start(m, sd0, si0, R, cell_col=None, ncol=None):
    m.set_state(sd0, si0)
    m.put_data_config(R)
    m.put_data_init()
    if cell_col is not None:
        m.set_forcing_map(cell_col, ncol)      # after the put_data configuration: the map leaves it alone
    return m


def run_steps(m, f, sf, dmy):
    m.push_forcing(f, sf, dmy)
    m.dist_prec(0, 1)
    if f.shape[0] > 1:
        m.dist_prec(1, f.shape[0] - 1)


def flags_split(sf, cell_col, ncol):
    """(step, sub-step, column) at which the cells of one column do not all have the same flag: where a flag read through the
    column instead of the cell would be another one."""
    lo = np.full(sf.shape[:2] + (ncol,), 1, dtype=np.int64)
    hi = np.zeros(sf.shape[:2] + (ncol,), dtype=np.int64)
    for c, col in enumerate(cell_col):
        lo[..., col] = np.minimum(lo[..., col], sf[..., c])
        hi[..., col] = np.maximum(hi[..., col], sf[..., c])
    return int((hi > lo).sum())


def differing(a, b):
    return [k for k in a if not np.array_equal(a[k], b[k], equal_nan=True)]


def run_case(name, ncol, M, kind):
    """The names of the tables in which the mapped run differs from the replicated one, and what the run was worth: the
    members differ from each other, nothing failed, and the number of flags that differ within a column."""
    D, cell_col, f, fA, sf, dmy, sd0, si0 = build(name, ncol, M, kind)
    glacier = CASES[name][5]
    a = start(Model(D), sd0, si0, f.shape[0])
    run_steps(a, fA, sf, dmy)
    want = tables(a, f.shape[0], glacier)
    a.close()
    b = start(Model(D), sd0, si0, f.shape[0], cell_col, ncol)
    assert b.get_forcing_map()[0] == ncol and np.array_equal(b.get_forcing_map()[1], cell_col)
    run_steps(b, f, sf, dmy)
    got = tables(b, f.shape[0], glacier, cell_col)
    b.close()
    bad = differing(want, got)
    # members differ: with the member-major map the cells j and ncol + j are one base cell on one column under two parameter sets
    members_differ = not np.array_equal(want["accum"][:, :ncol], want["accum"][:, ncol:2 * ncol])
    ok = not want["errors"].any() and bool(np.isfinite(want["out_agg"]).all()) and bool(want["out_agg"].any())
    return bad, members_differ, ok, flags_split(sf, cell_col, ncol)


def raw_case(ncol, M, min_wind=0.4):
    """dt = 24, snow_step = 3 from day 60, three steps: raw forcing whose T and prec are the synthetic table's, so that the
    members' flags differ where the table says they do."""
    opt = abi.default_options(FULL_ENERGY=0, dt=24, snow_step=3)
    base = domain.make_domain(ncol, opt, ntile=2)
    nsteps = 3
    f, _, dmy = domain.make_forcing(base, 0, nsteps, start_doy=60)
    rng = np.random.default_rng(3)
    raw = np.zeros((nsteps, C["VIC_NRAW"], opt.dt, ncol))
    hours = lambda v: np.repeat(f[:, C[v], :opt.NF], opt.snow_step, axis=1)          # the sub-step value in each of its hours
    raw[:, C["VIC_RAW_AIR_TEMP"]] = hours("VIC_F_AIR_TEMP")
    raw[:, C["VIC_RAW_PREC"]] = hours("VIC_F_PREC") / opt.snow_step
    raw[:, C["VIC_RAW_PRESSURE_KPA"]] = hours("VIC_F_PRESSURE") * 1e-3
    raw[:, C["VIC_RAW_VP_KPA"]] = hours("VIC_F_VP") * 1e-3 * rng.uniform(0.5, 1.6, raw[:, 0].shape)      # some above saturation
    raw[:, C["VIC_RAW_SHORTWAVE"]] = hours("VIC_F_SHORTWAVE"); raw[:, C["VIC_RAW_LONGWAVE"]] = hours("VIC_F_LONGWAVE")
    raw[:, C["VIC_RAW_WIND"]] = hours("VIC_F_WIND") * rng.uniform(0.0, 1.2, raw[:, 0].shape)             # some below the floor
    D, cell_col = domain.tile_members(base, M)
    perturb(D, ncol, M)
    return D, cell_col, raw, dmy, min_wind


def run_raw(ncol, M, oracle=None):
    """(problems, flags that differ between members of one column, flags in all).  oracle: oracle.pyref, or None to leave that
    comparison out."""
    D, cell_col, raw, dmy, min_wind = raw_case(ncol, M)
    nsteps = raw.shape[0]
    rawA = np.ascontiguousarray(np.tile(raw, (1, 1, 1, M)))
    a = Model(D)
    a.prefetch_forcing_raw(rawA, dmy, min_wind_speed=min_wind, plapse=True); a.swap_forcing()
    fa = [a.get_forcing(s) for s in range(nsteps)]
    a.close()
    b = Model(D)
    b.set_forcing_map(cell_col, ncol)
    b.prefetch_forcing_raw(raw, dmy, min_wind_speed=min_wind, plapse=True); b.swap_forcing()
    fb = [b.get_forcing(s) for s in range(nsteps)]
    b.close()
    FA, SA = np.stack([x[0] for x in fa]), np.stack([x[1] for x in fa])
    FB, SB = np.stack([x[0] for x in fb]), np.stack([x[1] for x in fb])
    bad = []
    if FB.shape != (nsteps, C["VIC_NFORCE"], D.opt.NR + 1, ncol):
        bad.append("shape of the mapped table %s" % (FB.shape,))
    elif not np.array_equal(FA, FB[..., cell_col]):
        bad.append("derived rows differ from the replicated run's")
    if not np.array_equal(SA, SB):
        bad.append("flags differ from the replicated run's")
    if oracle is not None:
        fo, so = oracle.OracleModel(D).derive_forcing(rawA, min_wind=min_wind, plapse=1)
        exact = [C[v] for v in ("VIC_F_AIR_TEMP", "VIC_F_PREC", "VIC_F_PRESSURE", "VIC_F_DENSITY", "VIC_F_SHORTWAVE", "VIC_F_LONGWAVE", "VIC_F_WIND")]
        for what, F, S in (("replicated", FA, SA), ("mapped", FB[..., cell_col] if not bad else FA, SB)):
            if not np.array_equal(so, S):
                bad.append("%s flags differ from the oracle's" % what)
            if not np.array_equal(fo[:, exact], F[:, exact]):      # no transcendental on these rows: bit for bit
                bad.append("%s rows differ from the oracle's" % what)
            rel = np.abs(fo - F) / np.maximum(np.maximum(np.abs(fo), np.abs(F)), 1e-6)
            if not rel.max() < 1e-11:                              # vp / vpd go through exp: a few ulp of svp
                bad.append("%s vp / vpd off the oracle's by %.3g" % (what, rel.max()))
        if not ((fo[:, C["VIC_F_VPD"]] == 0).any() and (raw[:, C["VIC_RAW_WIND"]] < min_wind).any()):
            bad.append("no clipped vpd or no floored wind in the table")
    per_member = SB.reshape(nsteps, D.opt.NR + 1, M, ncol)
    split = int((per_member.max(axis=2) != per_member.min(axis=2)).sum())      # (step, sub-step, column) with members apart
    return bad, split, int(per_member[:, :, 0].size)


def run_records(ncol, M, depth=2, R=2, nrec=2):
    """vicgpu_run_records with a map against vicgpu_step + vicgpu_get_outputs(reset) + vicgpu_get_cell_errors with a map."""
    kw, ntile, doy = CASES["full_energy"][:3]
    os.environ.pop("VICGPU_CHUNKS", None)
    opt = abi.default_options(**kw)
    base = domain.make_domain(ncol, opt, ntile=ntile)
    f, _, dmy = domain.make_forcing(base, 0, R * nrec, start_doy=doy)
    D, _ = domain.tile_members(base, M)
    perturb(D, ncol, M)
    cell_col = scrambled_map(D.ncell, ncol)
    sf = domain.make_snowflag(D, f, cell_col)
    sd0, si0 = init_state.initial_state(D, np.ascontiguousarray(f[0][..., cell_col]))
    a = start(Model(D), sd0, si0, R, cell_col, ncol)
    a.push_forcing(f, sf, dmy)
    out, err = [], []
    for k in range(nrec):
        a.dist_prec(k * R, R, sync=False)
        out.append(a.get_outputs(OUT, reset=True))
        err.append(a.get_cell_errors())
    want = tables(a, R * nrec, cell_col=cell_col)
    want["records"], want["record_errors"] = np.stack(out), np.stack(err)
    a.close()
    b = start(Model(D), sd0, si0, R, cell_col, ncol)
    b.records_config(OUT, depth=depth)          # the map has left the put_data configuration in place
    b.push_forcing(f, sf, dmy)
    rec = b.run_records(0, nrec, errors=True)
    rec.wait()
    got = tables(b, R * nrec, cell_col=cell_col)
    got["records"], got["record_errors"] = rec.out.copy(), rec.errors.copy()
    del rec
    b.close()
    return differing(want, got), bool(want["records"].any() and np.isfinite(want["records"]).all())


def run_group(name, ncol, M, devices, kind):
    """A group of len(devices) shards against one context, both with the map."""
    D, cell_col, f, fA, sf, dmy, sd0, si0 = build(name, ncol, M, kind)
    one = start(Model(D), sd0, si0, f.shape[0], cell_col, ncol)
    run_steps(one, f, sf, dmy)
    want = tables(one, f.shape[0])
    one.close()
    g = start(Group(D, devices=devices), sd0, si0, f.shape[0], cell_col, ncol)
    assert g.get_forcing_map()[0] == ncol and np.array_equal(g.get_forcing_map()[1], cell_col)
    bounds = g.shard_bounds()
    fp = g.pinned(f.shape); fp[:] = f             # the pitched copies straight from pinned memory
    run_steps(g, fp, sf, dmy)
    got = tables(g, f.shape[0])
    g.close()
    return [k for k in got if not np.array_equal(want[k], got[k], equal_nan=True)], bounds


def errors():
    lib = load_library()
    ARG, STATE, OK = C["VICGPU_ERR_ARG"], C["VICGPU_ERR_STATE"], 0
    ip = ctypes.POINTER(ctypes.c_int)
    checks = []

    def want(what, got, code):
        checks.append((what, got, code))

    n = ctypes.c_int(-7)
    one = np.zeros(1, dtype=np.int32)
    for pre in ("vicgpu_", "vicgpu_group_"):
        want(pre + "set_forcing_map(NULL)", getattr(lib, pre + "set_forcing_map")(None, 1, one.ctypes.data_as(ip)), ARG)
        want(pre + "get_forcing_map(NULL)", getattr(lib, pre + "get_forcing_map")(None, ctypes.byref(n), None), ARG)
    ncol, M = 5, 3
    D, cell_col, f, fA, sf, dmy, sd0, si0 = build("full_energy", ncol, M, "member-major")
    # before a domain: a context that has none yet
    h = ctypes.c_void_p()
    want("create", lib.vicgpu_create(ctypes.byref(D.opt), 0, ctypes.byref(h)), OK)
    want("set_forcing_map before a domain", lib.vicgpu_set_forcing_map(h, ncol, cell_col.ctypes.data_as(ip)), STATE)
    want("identity before a domain", lib.vicgpu_set_forcing_map(h, 0, None), STATE)
    want("get_forcing_map before a domain", lib.vicgpu_get_forcing_map(h, ctypes.byref(n), None), STATE)
    lib.vicgpu_destroy(h)
    m = Model(D)
    m.set_state(sd0, si0)
    setmap = lambda k, cc: lib.vicgpu_set_forcing_map(m.h, k, cc.ctypes.data_as(ip) if cc is not None else None)

    def getmap():
        got = np.full(D.ncell, -1, dtype=np.int32)
        rc = lib.vicgpu_get_forcing_map(m.h, ctypes.byref(n), got.ctypes.data_as(ip))
        return rc, n.value, got
    ident = np.arange(D.ncell, dtype=np.int32)
    want("get_forcing_map of a fresh domain", getmap()[0], OK)
    want("a fresh domain has ncell columns", getmap()[1], D.ncell)
    want("... and the identity map", int(np.array_equal(getmap()[2], ident)), 1)
    want("get_forcing_map(ncol NULL)", lib.vicgpu_get_forcing_map(m.h, None, None), ARG)
    want("get_forcing_map(cell_col NULL)", lib.vicgpu_get_forcing_map(m.h, ctypes.byref(n), None), OK)
    want("set_forcing_map", setmap(ncol, cell_col), OK)
    want("ncol after set", getmap()[1], ncol)
    want("map after set", int(np.array_equal(getmap()[2], cell_col)), 1)
    want("step before a chunk was pushed", lib.vicgpu_step(m.h, 0, 1), STATE)
    m.ncol = ncol                      # the map was set behind the Model's back: its shape checks follow
    m.push_forcing(f, sf, dmy)
    want("step on the pushed chunk", lib.vicgpu_step(m.h, 0, 1), OK)
    # refused maps leave the map and the chunk in force
    bad = cell_col.copy(); bad[7] = ncol
    want("entry == ncol", setmap(ncol, bad), ARG)
    bad = cell_col.copy(); bad[0] = -1
    want("negative entry", setmap(ncol, bad), ARG)
    want("ncol 0 with a map", setmap(0, cell_col), ARG)
    want("negative ncol", setmap(-3, cell_col), ARG)
    want("NULL with a foreign ncol", setmap(ncol, None), ARG)
    want("ncol after refused maps", getmap()[1], ncol)
    want("map after refused maps", int(np.array_equal(getmap()[2], cell_col)), 1)
    want("step after refused maps", lib.vicgpu_step(m.h, 1, 1), OK)
    want("synchronize", lib.vicgpu_synchronize(m.h), OK)
    # a new map drops the chunk
    want("a wider map", setmap(ncol + 2, cell_col), OK)
    want("step after a new map", lib.vicgpu_step(m.h, 0, 1), STATE)
    m.ncol = ncol + 2
    wide = np.concatenate([f, f[..., :2]], axis=-1)
    m.push_forcing(wide, sf, dmy)
    want("step after the push", lib.vicgpu_step(m.h, 0, 1), OK)
    # NULL restores the identity
    want("NULL (ncol 0)", setmap(0, None), OK)
    want("identity has ncell columns", getmap()[1], D.ncell)
    want("identity map", int(np.array_equal(getmap()[2], ident)), 1)
    want("step after the identity", lib.vicgpu_step(m.h, 0, 1), STATE)
    want("NULL (ncol ncell)", setmap(D.ncell, None), OK)
    m.ncol = D.ncell
    m.push_forcing(fA, sf, dmy)
    want("step on replicated forcing", lib.vicgpu_step(m.h, 0, 1), OK)
    # vicgpu_set_domain restores the identity
    want("set_forcing_map again", setmap(ncol, cell_col), OK)
    m.set_domain(D)
    want("ncol after set_domain", getmap()[1], D.ncell)
    want("map after set_domain", int(np.array_equal(getmap()[2], ident)), 1)
    want("step after set_domain", lib.vicgpu_step(m.h, 0, 1), STATE)
    m.close()
    # the group
    g = Group(D, devices=[0, 0])
    gset = lambda k, cc: lib.vicgpu_group_set_forcing_map(g.h, k, cc.ctypes.data_as(ip) if cc is not None else None)
    bad = cell_col.copy(); bad[-1] = ncol
    want("group: entry == ncol", gset(ncol, bad), ARG)
    want("group: ncol 0 with a map", gset(0, cell_col), ARG)
    want("group: set_forcing_map", gset(ncol, cell_col), OK)
    want("group: ncol", g.get_forcing_map()[0], ncol)
    want("group: step before a chunk", lib.vicgpu_group_step(g.h, 0, 1), STATE)
    want("group: NULL", gset(0, None), OK)
    want("group: identity", int(np.array_equal(g.get_forcing_map()[1], ident) and g.get_forcing_map()[0] == D.ncell), 1)
    g.close()
    failed = [(w, got, c) for w, got, c in checks if got != c]
    for w, got, c in failed:
        print("forcing map error return: %s gave %d, want %d" % (w, got, c), flush=True)
    print("hostemu forcing map errors: %d checks, failed: %d" % (len(checks), len(failed)), flush=True)
    return 1 if failed else 0


def refusals():
    """vicgpu_set_forcing_map with the n-th allocation refused (hostemu_refuse_alloc), n = 1, 2, ...: VICGPU_ERR_HIP, the count of
    live runtime objects where it was and the map in force unchanged, until the call gets through; the identity releases what
    it then owns."""
    lib = load_library()
    lib.hostemu_live_objects.restype = ctypes.c_longlong
    lib.hostemu_refuse_alloc.argtypes = [ctypes.c_longlong]
    live0 = lib.hostemu_live_objects()
    D, cell_col, f, fA, sf, dmy, sd0, si0 = build("full_energy", 5, 3, "scrambled")
    m = Model(D)
    m.set_state(sd0, si0)
    ip = ctypes.POINTER(ctypes.c_int)
    bad = []
    before = lib.hostemu_live_objects()
    n = 0
    for n in range(1, 20):
        lib.hostemu_refuse_alloc(n)
        rc = lib.vicgpu_set_forcing_map(m.h, 5, cell_col.ctypes.data_as(ip))
        lib.hostemu_refuse_alloc(0)
        if rc == 0:
            break
        if rc != C["VICGPU_ERR_HIP"] or lib.hostemu_live_objects() != before or m.get_forcing_map()[0] != D.ncell:
            bad.append("allocation %d refused: code %d, %d objects more, ncol %d" % (n, rc, lib.hostemu_live_objects() - before, m.get_forcing_map()[0]))
    owned = lib.hostemu_live_objects() - before
    if n != 3 or owned != 2:         # the map and the HRU row were refused once each
        bad.append("%d refusals, %d objects owned" % (n - 1, owned))
    m.ncol = 5
    m.push_forcing(f, sf, dmy)
    m.dist_prec(0, 1)
    slots = lib.hostemu_live_objects() - before - owned      # the forcing slot the push has filled, which outlives a map
    m.set_forcing_map(None)
    if lib.hostemu_live_objects() - before != slots:
        bad.append("%d objects left by the identity" % (lib.hostemu_live_objects() - before - slots))
    m.close()
    left = lib.hostemu_live_objects() - live0
    if left:
        bad.append("%d objects left after close" % left)
    print("hostemu forcing map refusals: %d refused, then through owning %d objects; problems: %s" % (n - 1, owned, bad or "none"), flush=True)
    return 1 if bad else 0


def main(argv):
    cmd = argv[0]
    if cmd == "run":
        name, ncol, M = argv[1], int(argv[2]), int(argv[3])
        rc = 0
        for kind in MAPS:
            bad, members_differ, ok, split = run_case(name, ncol, M, kind)
            print("forcing map %s %s map, %d columns x %d members: members differ: %s, clean run: %s, flags apart within a column: %d, differing: %s"
                  % (name, kind, ncol, M, members_differ, ok, split, bad or "none"), flush=True)
            if bad or not members_differ or not ok:
                rc = 1
        return rc
    if cmd == "raw":
        from oracle import pyref
        bad, split, nflag = run_raw(int(argv[1]), int(argv[2]), pyref if pyref.have_oracle() else None)
        print("forcing map raw: %d of %d (step, sub-step, column) with members' flags apart, oracle: %s, problems: %s"
              % (split, nflag, pyref.have_oracle(), bad or "none"), flush=True)
        return 1 if bad or split < 1 else 0
    if cmd == "records":
        bad, ok = run_records(int(argv[1]), int(argv[2]))
        print("forcing map records: finite and non-zero: %s, differing: %s" % (ok, bad or "none"), flush=True)
        return 1 if bad or not ok else 0
    if cmd == "group":
        ncol, M, ns = int(argv[1]), int(argv[2]), int(argv[3])
        rc = 0
        for kind in MAPS + ("blocked",):
            bad, bounds = run_group("full_energy", ncol, M, [0] * ns, kind)
            print("forcing map group %s map: shards at %s, differing: %s" % (kind, bounds.tolist(), bad or "none"), flush=True)
            if bad:
                rc = 1
        return rc
    return {"errors": errors, "refusals": refusals}[cmd]()


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
