"""Model state copied between cells on the device (vicgpu_copy_cells / vicgpu_group_copy_cells, include/vicgpu.h) against the
same assignment made through the host: get_state / get_fluxes, the columns permuted with numpy, set_state / set_fluxes.  Every
comparison is bit for bit.  Run by tests/test_copy_cells.py with VICGPU_LIB pointing at the unsanitized host build
(SAN=none tools/hostemu/build.sh); tests/test_copy_cells_gpu.py imports the functions for the GPU.
    python tools/hostemu/check_copy_cells.py patterns        fan-out, rotation, resample, swap, rotation with one row per pass
    python tools/hostemu/check_copy_cells.py frozen          FROZEN_SOIL as two chunks, pairs across the chunk boundary
    python tools/hostemu/check_copy_cells.py continuation    STATE | BALANCE: the destination's later records are the source's
    python tools/hostemu/check_copy_cells.py untouched       what a call must leave alone; a retired destination
    python tools/hostemu/check_copy_cells.py errors          every error return, each leaving every table as it was
    python tools/hostemu/check_copy_cells.py refusals        the n-th allocation refused, for every n
    python tools/hostemu/check_copy_cells.py group           3 shards on device 0 next to one context
Each prints "copy cells <name>: problems: none" (or the list) and exits with 1 when there are any."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from vic_amd import abi, domain, init_state
from vic_amd.abi import C
from vic_amd.api import Group, Model, VicGpuError, load_library

STATE, BALANCE = C["VICGPU_COPY_STATE"], C["VICGPU_COPY_BALANCE"]
OUT = ["OUT_SWE_BAND", "OUT_RUNOFF", "OUT_SURF_TEMP", "OUT_SOIL_MOIST", "OUT_DELSOILMOIST", "OUT_WATER_ERROR", "OUT_SWE", "OUT_BASEFLOW"]
R = 3                        # steps per output record
STAGE = "VICGPU_COPY_STAGE_MB"


class Ensemble:
    pass


def _perturb_state(E):
    """Every member its own initial state: drier soil and a deeper snow pack with the member index."""
    member = E.D.hru_iparams[C["HPI_CELL"]] // E.ncol
    for m in range(1, E.M):
        cols = member == m
        for r in ("SD_MOIST0", "SD_MOIST1", "SD_MOIST2"):
            E.sd0[C[r], cols] *= 1.0 - 0.06 * m
        E.sd0[C["SD_SNOW_SWQ"], cols] += 0.015 * m
        E.sd0[C["SD_SNOW_DEPTH"], cols] += 0.06 * m
        E.sd0[C["SD_SNOW_DENSITY"], cols] = 250.0
        E.sd0[C["SD_SNOW_COVERAGE"], cols] = 1.0
        E.sd0[C["SD_SNOW_SURF_TEMP"], cols] = -1.0 - 0.5 * m
        E.si0[C["SI_SNOW_SNOW"], cols] = 1


def ensemble(kw, ncol, M, ntile, nsteps, doy, ragged=False, glacier=False):
    """M members of `ncol` base cells over the same forcing columns (domain.tile_members), every member from another state.
    ragged: the base cells keep 2 or 3 tiles (every fifth cell the third), so their HRU counts differ."""
    E = Ensemble()
    opt = abi.default_options(**kw)
    base = domain.make_domain(ncol, opt, ntile=ntile, glacier_top_band=glacier)
    if ragged:
        cell = base.hru_iparams[C["HPI_CELL"]]
        tile = (np.arange(base.nhru) // base.ncell) // opt.Nband
        domain.drop_hrus(base, (tile == ntile - 1) & (cell % 5 != 0))
    E.f, _, E.dmy = domain.make_forcing(base, 0, nsteps, start_doy=doy)
    E.D, E.cell_col = domain.tile_members(base, M)
    E.ncol, E.M, E.base = ncol, M, base
    E.sf = domain.make_snowflag(E.D, E.f, E.cell_col)
    E.sd0, E.si0 = init_state.initial_state(E.D, np.ascontiguousarray(E.f[0][..., E.cell_col]))
    _perturb_state(E)
    return E


def quickflux(nsteps=1 + 2 * R, ncol=35, M=4):
    """QUICK_FLUX, 3 bands, 35 base cells of 6 or 9 HRUs (231 HRUs a member: more than 64, no multiple of 64), 4 members."""
    return ensemble(dict(FULL_ENERGY=1, Nband=3), ncol, M, 3, nsteps, 80, ragged=True)


def members(E, pairs):
    """(dst, src) cell lists of the member pairs [(dst member, src member)]."""
    j = np.arange(E.ncol)
    dst = np.concatenate([d * E.ncol + j for d, _ in pairs])
    src = np.concatenate([s * E.ncol + j for _, s in pairs])
    return dst.astype(np.int32), src.astype(np.int32)


def patterns(E):
    """name -> (dst, src, VICGPU_COPY_STAGE_MB or None)"""
    nine = [c for c in range(E.ncol) if c % 5 == 0]          # base cells with the third tile
    a, b = E.ncol + nine[0], E.ncol + nine[1]                # two cells of equal structure inside member 1
    return {
        "fanout": members(E, [(1, 0), (2, 0), (3, 0)]) + (None,),
        "rotation": members(E, [(1, 0), (2, 1), (3, 2), (0, 3)]) + (None,),
        "resample": members(E, [(0, 0), (1, 0), (2, 2), (3, 2)]) + (None,),
        "swap": (np.array([a, b], np.int32), np.array([b, a], np.int32), None),
        "rotation_row_per_pass": members(E, [(1, 0), (2, 1), (3, 2), (0, 3)]) + ("0",),
    }


def start(m, E, put=True):
    m.set_forcing_map(E.cell_col, E.ncol)
    m.set_state(E.sd0, E.si0)
    if put:
        m.put_data_config(R)
        m.put_data_init()
    m.push_forcing(E.f, E.sf, E.dmy)
    return m


def model(E, stage_mb=None, cls=Model, put=True, **kw):
    """A model of the ensemble; the staging budget is read when the domain is set."""
    os.environ.pop(STAGE, None)
    if stage_mb is not None:
        os.environ[STAGE] = stage_mb
    m = start(cls(E.D, **kw), E, put)
    os.environ.pop(STAGE, None)
    return m


def hru_columns(D, dst, src):
    """The HRU columns of the cell pairs, paired by position in cell_hru_list order."""
    off, lst = D.cell_hru_offset, D.cell_hru_list
    hd = np.concatenate([lst[off[d]:off[d + 1]] for d in dst]) if len(dst) else np.zeros(0, np.int64)
    hs = np.concatenate([lst[off[s]:off[s + 1]] for s in src]) if len(src) else np.zeros(0, np.int64)
    return hd, hs


def host_copy(m, dst, src):
    """The same assignment through the host (all sources read before any destination is written)."""
    hd, hs = hru_columns(m.dom, dst, src)
    sd, si = m.get_state()
    fx = m.get_fluxes()
    sd[:, hd], si[:, hd], fx[:, hd] = sd[:, hs], si[:, hs], fx[:, hs]
    m.set_state(sd, si)
    m.set_fluxes(fx)


def tables(m, put=True):
    r = {}
    r["sd"], r["si"] = m.get_state()
    r["flux"] = m.get_fluxes()
    r["cell_err"] = m.get_cell_errors()
    r["valid"] = m.get_cell_valid()
    if put:
        r["balance"] = m.get_balance()
    if not isinstance(m, Group):
        r["accum"] = m.get_accum()
        r["cell_out"] = m.get_cell_outputs()
        if put:
            r["out_data"] = m.get_output_data(OUT)
            r["out_agg"] = m.get_output_data(OUT, aggregated=True)
    return r


def same(a, b):
    """bit for bit: integer tables as they are, floating-point tables through their unsigned views"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind == "f":
        u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        return bool(np.array_equal(a.view(u), b.view(u)))
    return bool(np.array_equal(a, b))


def differing(a, b):
    return [k for k in a if not same(a[k], b[k])]


def members_differ(E, t):
    """the members' state columns are not copies of each other"""
    hpm = E.base.nhru
    lst = E.D.cell_hru_list.reshape(E.M, hpm)          # member-major: member m's HRUs in the base's CSR order
    return all(not same(t["sd"][:, lst[0]], t["sd"][:, lst[m]]) for m in range(1, E.M))


def run_records(m, step0, nrec):
    out = []
    for k in range(nrec):
        m.dist_prec(step0 + k * R, R, sync=False)
        out.append(m.get_outputs(OUT, reset=True))
    return np.stack(out)


def run_pattern(E, dst, src, stage_mb, pre=1, log=print, name=""):
    """Device path on one model, host path on a second one: the tables right after the copy, then two records on both.
    Returns (problems, the device path's tables after the copy)."""
    bad = []
    a, b = model(E, stage_mb), model(E)
    if pre:
        a.dist_prec(0, pre, sync=False)
        b.dist_prec(0, pre)
    if not members_differ(E, tables(b)):
        bad.append("the members do not differ before the copy")
    a.copy_cells(dst, src)                   # queued behind the step; the read-backs wait for it
    host_copy(b, dst, src)
    ta, tb = tables(a), tables(b)
    bad += ["after the copy: " + k for k in differing(tb, ta)]
    ra, rb = run_records(a, pre, 2), run_records(b, pre, 2)
    ua, ub = tables(a), tables(b)
    bad += ["after two records: " + k for k in differing(ub, ua)]
    if not same(ra, rb):
        bad.append("the records after the copy")
    if not (np.isfinite(rb).all() and rb.any()):
        bad.append("the host path's records are not finite or all zero")
    a.close(); b.close()
    log("copy cells %s: %d pairs, %d cells x %d HRUs, differing: %s" % (name, len(dst), E.D.ncell, E.D.nhru, bad or "none"), flush=True)
    return bad, ta


def check_patterns(log=print):
    E = quickflux()
    bad, kept = [], {}
    for name, (dst, src, mb) in patterns(E).items():
        b, kept[name] = run_pattern(E, dst, src, mb, log=log, name=name)
        bad += ["%s: %s" % (name, x) for x in b]
    bad += ["one row per pass gives other bits than the default budget: " + k for k in differing(kept["rotation"], kept["rotation_row_per_pass"])]
    return bad


def check_frozen(log=print, chunks="2"):
    """FROZEN_SOIL, 10 nodes, 2 bands, glacier HRUs, 5 base cells x 2 members as two chunks (boundary = member boundary): a
    direct call and a staged one, both with pairs across the boundary, right behind a two-step vicgpu_step."""
    os.environ["VICGPU_CHUNKS"] = chunks
    try:
        E = ensemble(dict(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=10, Nband=2, frozen_compat=0), 5, 2, 2, 2 + 2 * R, 330, glacier=True)
        if not E.D.hru_iparams[C["HPI_IS_GLACIER"]].any():
            return ["no glacier HRU in the domain"]
        a, b = model(E), model(E)
        a.dist_prec(0, 2, sync=False)
        b.dist_prec(0, 2)
        bad = [] if members_differ(E, tables(b)) else ["the members do not differ before the copy"]
        calls = [(np.array([6, 2], np.int32), np.array([1, 7], np.int32)),                      # direct, both ways across
                 (np.array([5, 0, 8, 3], np.int32), np.array([0, 5, 8, 9], np.int32))]          # a swap across, an identity pair, 3 <- 9
        for dst, src in calls:
            a.copy_cells(dst, src)
            host_copy(b, dst, src)
        bad += ["after the copies: " + k for k in differing(tables(b), tables(a))]
        ra, rb = run_records(a, 2, 2), run_records(b, 2, 2)
        bad += ["after two records: " + k for k in differing(tables(b), tables(a))]
        if not same(ra, rb):
            bad.append("the records after the copies")
        if not (np.isfinite(rb).all() and rb.any()):
            bad.append("the host path's records are not finite or all zero")
        a.close(); b.close()
    finally:
        os.environ.pop("VICGPU_CHUNKS", None)
    log("copy cells frozen (chunks %s): differing: %s" % (chunks, bad or "none"), flush=True)
    return bad


def check_continuation(log=print):
    """Member 1 <- member 0 with STATE | BALANCE at a record boundary: from then on member 1's records are member 0's, all
    variables, through vicgpu_run_records.  With STATE alone the PB columns of member 1 stay as they were."""
    E = quickflux(nsteps=4 * R)
    bad = []
    m = model(E)
    names = [n for n, _, _ in m.output_list()]
    m.records_config(names, depth=2)
    rec = m.run_records(0, 2)
    rec.wait()
    before = rec.out.copy()
    del rec
    c0, c1 = slice(0, E.ncol), slice(E.ncol, 2 * E.ncol)
    if same(before[..., c0], before[..., c1]):
        bad.append("the members' records before the copy do not differ")
    pb0 = m.get_balance()
    if same(pb0[:, c0], pb0[:, c1]):
        bad.append("the members' balance columns before the copy do not differ")
    dst, src = members(E, [(1, 0)])
    m.copy_cells(dst, src, STATE | BALANCE)
    pb = m.get_balance()
    if not same(pb[:, c1], pb[:, c0]) or not same(pb[:, c0], pb0[:, c0]) or not same(pb[:, 2 * E.ncol:], pb0[:, 2 * E.ncol:]):
        bad.append("balance columns after STATE | BALANCE")
    rec = m.run_records(2 * R, 2)
    rec.wait()
    after = rec.out.copy()
    del rec
    eq = (after[..., c0].view(np.uint32) == after[..., c1].view(np.uint32))
    if not eq.all():
        rows = sorted(set(np.nonzero(~eq)[1].tolist()))
        bad.append("later records of member 1 differ from member 0's in rows %s" % rows[:12])
    if not np.isfinite(after[..., c0][np.isfinite(before[..., c0])]).all() or not after.any():
        bad.append("the later records are not finite or all zero")
    m.close()
    # STATE alone
    m = model(E)
    m.dist_prec(0, R)
    pb0 = m.get_balance()
    m.copy_cells(dst, src, STATE)
    if not same(m.get_balance(), pb0):
        bad.append("STATE alone changed balance columns")
    m.close()
    log("copy cells continuation: %d variables, differing: %s" % (len(names), bad or "none"), flush=True)
    return bad


def check_untouched(log=print):
    """Across a call: the flags, the validity table (a retired destination stays retired and its columns still take the copy),
    CA / CO, the output values and aggregates, the forcing map and the records configuration; the columns of cells in no pair
    in every table."""
    E = quickflux()
    bad = []
    a, b = model(E), model(E)
    dst, src = members(E, [(2, 0), (0, 2)])                  # members 1 and 3 are in no pair
    valid = np.ones(E.D.ncell, np.int32)
    retired = 2 * E.ncol + 3
    valid[retired] = 0
    for m in (a, b):
        m.dist_prec(0, 2)                                    # aggregates and accumulators hold something
        m.set_cell_valid(valid)
    a.records_config(OUT, depth=2)
    cfg = (a.lib.vicgpu_records_nrow(a.h), a.records_ncol(), a.records_get_groups(), a.get_forcing_map()[0], a.get_forcing_map()[1].copy())
    t0 = tables(a)
    a.copy_cells(dst, src, STATE | BALANCE)
    host_copy(b, dst, src)
    t1, tb = tables(a), tables(b)
    for k in ("cell_err", "valid", "accum", "cell_out", "out_data", "out_agg"):
        if not same(t0[k], t1[k]):
            bad.append(k + " changed")
    if t1["valid"][retired] != 0:
        bad.append("the retired destination is valid again")
    for k in ("sd", "si", "flux"):
        if not same(t1[k], tb[k]):
            bad.append(k + " differs from the host path (the retired destination takes the copy)")
    hd, _ = hru_columns(E.D, dst, src)
    rest_h = np.setdiff1d(np.arange(E.D.nhru), hd)
    rest_c = np.setdiff1d(np.arange(E.D.ncell), dst)
    for k in ("sd", "si", "flux"):
        if not same(t0[k][:, rest_h], t1[k][:, rest_h]):
            bad.append(k + ": columns of cells in no pair changed")
        if same(t0[k][:, hd], t1[k][:, hd]):
            bad.append(k + ": the destination columns did not change")
    if not same(t0["balance"][:, rest_c], t1["balance"][:, rest_c]):
        bad.append("balance: columns of cells in no pair changed")
    now = (a.lib.vicgpu_records_nrow(a.h), a.records_ncol(), a.records_get_groups(), a.get_forcing_map()[0], a.get_forcing_map()[1])
    if cfg[:4] != now[:4] or not np.array_equal(cfg[4], now[4]):
        bad.append("the records configuration or the forcing map changed")
    a.close(); b.close()
    log("copy cells untouched: differing: %s" % (bad or "none"), flush=True)
    return bad


def error_returns(log=print):
    """Every VICGPU_ERR_ARG / VICGPU_ERR_STATE return of the header, each leaving every table as it was.  All of them are
    refused on the host before any launch."""
    lib = load_library()
    ARG, ST, OK = C["VICGPU_ERR_ARG"], C["VICGPU_ERR_STATE"], 0
    ip = ctypes.POINTER(ctypes.c_int)
    checks = []
    i32 = lambda x: np.asarray(x, dtype=np.int32)

    def call(h, dst, src, what=STATE, n=None, fn=lib.vicgpu_copy_cells):
        d, s = (None if dst is None else i32(dst)), (None if src is None else i32(src))
        n = (len(d) if d is not None else 0) if n is None else n
        return fn(h, n, d.ctypes.data_as(ip) if d is not None else None, s.ctypes.data_as(ip) if s is not None else None, what)

    E = quickflux()
    # one cell's vegetation class differs at one position: member 1, base cell 3, its second HRU
    D = E.D
    odd = E.ncol + 3
    h = D.cell_hru_list[D.cell_hru_offset[odd] + 1]
    D.hru_iparams[C["HPI_VEG_CLASS"], h] += 1
    m = Model(D)
    checks.append(("no domain state is needed for a null handle", call(None, [1], [0]), ARG))
    fresh = ctypes.c_void_p()
    assert lib.vicgpu_create(ctypes.byref(D.opt), 0, ctypes.byref(fresh)) == 0
    checks.append(("no domain", call(fresh, [1], [0]), ST))
    lib.vicgpu_destroy(fresh)
    start(m, E, put=False)
    m.dist_prec(0, 1)
    t0 = tables(m, put=False)
    nc = D.ncell
    checks += [
        ("null lists with n > 0", call(m.h, None, None, n=2), ARG),
        ("null dst", call(m.h, None, [0], n=1), ARG),
        ("null src", call(m.h, [0], None, n=1), ARG),
        ("n < 0", call(m.h, [1], [0], n=-1), ARG),
        ("dst == ncell", call(m.h, [nc], [0]), ARG),
        ("dst < 0", call(m.h, [-1], [0]), ARG),
        ("src == ncell", call(m.h, [0], [nc]), ARG),
        ("src < 0", call(m.h, [0], [-1]), ARG),
        ("a repeated destination", call(m.h, [1, 40, 1], [0, 5, 36]), ARG),
        ("a destination repeated by an identity pair", call(m.h, [1, 1], [1, 36]), ARG),
        ("what == 0", call(m.h, [36], [1], what=0), ARG),
        ("unknown bits", call(m.h, [36], [1], what=4), ARG),
        ("unknown bits next to known ones", call(m.h, [36], [1], what=STATE | 8), ARG),
        ("HRU counts differ (a 9-HRU and a 6-HRU cell)", call(m.h, [0], [1]), ARG),
        ("vegetation class differs at one position", call(m.h, [3, odd], [E.ncol + 4, 3 + 2 * E.ncol]), ARG),
        ("... in a later pair, after legal ones", call(m.h, [1, 2, 3 + 2 * E.ncol], [36, 37, odd]), ARG),
        ("BALANCE without a put_data configuration", call(m.h, [36], [1], what=STATE | BALANCE), ST),
        ("BALANCE alone without a put_data configuration", call(m.h, [36], [1], what=BALANCE), ST),
    ]
    if not differing(t0, tables(m, put=False)):
        checks.append(("tables after the refused calls", "unchanged", "unchanged"))
    else:
        checks.append(("tables after the refused calls", differing(t0, tables(m, put=False)), "unchanged"))
    checks += [
        ("n == 0", call(m.h, None, None, n=0), OK),
        ("identity pairs only", call(m.h, [5, 6], [5, 6]), OK),
        ("the odd cell onto itself", call(m.h, [odd], [odd]), OK),
    ]
    checks.append(("tables after the no-ops", differing(t0, tables(m, put=False)) or "unchanged", "unchanged"))
    try:
        m.copy_cells([0], [1])
        checks.append(("Model.copy_cells raises", False, True))
    except VicGpuError as e:
        checks.append(("Model.copy_cells raises with the rule", "number of HRUs" in str(e), True))
    m.close()
    # the group
    g = start(Group(D, devices=[0, 0, 0]), E, put=False)
    gc = lib.vicgpu_group_copy_cells
    g0 = tables(g, put=False)
    checks += [
        ("group: null handle", call(None, [1], [0], fn=gc), ARG),
        ("group: null lists", call(g.h, None, None, n=1, fn=gc), ARG),
        ("group: n < 0", call(g.h, [1], [0], n=-2, fn=gc), ARG),
        ("group: cell out of range", call(g.h, [nc], [0], fn=gc), ARG),
        ("group: repeated destination", call(g.h, [1, 1], [0, 36], fn=gc), ARG),
        ("group: what == 0", call(g.h, [36], [1], what=0, fn=gc), ARG),
        ("group: incompatible pair across shards", call(g.h, [odd + 2 * E.ncol], [odd], fn=gc), ARG),
        ("group: BALANCE without put_data", call(g.h, [36], [1], what=BALANCE, fn=gc), ST),
        ("group: n == 0", call(g.h, None, None, n=0, fn=gc), OK),
    ]
    checks.append(("group: tables after the refused calls", differing(g0, tables(g, put=False)) or "unchanged", "unchanged"))
    fresh = ctypes.c_void_p()
    dev = i32([0, 0])
    assert lib.vicgpu_group_create(ctypes.byref(D.opt), 2, dev.ctypes.data_as(ip), ctypes.byref(fresh)) == 0
    checks.append(("group: no domain", call(fresh, [1], [0], fn=gc), ST))
    lib.vicgpu_group_destroy(fresh)
    g.close()
    failed = [(w, got, want) for w, got, want in checks if got != want]
    for w, got, want in failed:
        log("copy cells return: %s gave %s, want %s" % (w, got, want), flush=True)
    log("copy cells errors: %d checks, failed: %d" % (len(checks), len(failed)), flush=True)
    return ["%s gave %s" % (w, got) for w, got, _ in failed], len(checks)


def check_refusals(log=print):
    """vicgpu_copy_cells under a runtime that refuses its n-th allocation, n = 1, 2, ...: VICGPU_ERR_HIP, no live runtime object
    added and every table as it was, until the call gets through -- which leaves no object behind either."""
    lib = load_library()
    lib.hostemu_live_objects.restype = ctypes.c_longlong
    lib.hostemu_refuse_alloc.argtypes = [ctypes.c_longlong]
    ip = ctypes.POINTER(ctypes.c_int)
    E = quickflux()
    bad, counts = [], {}
    for name, pairs in (("direct", [(1, 0), (2, 0)]), ("staged", [(1, 0), (0, 1)])):
        m = model(E)
        m.dist_prec(0, 1)
        dst, src = members(E, pairs)
        t0 = tables(m)
        before = lib.hostemu_live_objects()
        for n in range(1, 20):
            lib.hostemu_refuse_alloc(n)
            rc = lib.vicgpu_copy_cells(m.h, len(dst), dst.ctypes.data_as(ip), src.ctypes.data_as(ip), STATE | BALANCE)
            lib.hostemu_refuse_alloc(0)
            if rc == 0:
                break
            if rc != C["VICGPU_ERR_HIP"] or lib.hostemu_live_objects() != before or differing(t0, tables(m)):
                bad.append("%s, allocation %d refused: code %d, %d objects more, changed %s"
                           % (name, n, rc, lib.hostemu_live_objects() - before, differing(t0, tables(m))))
        counts[name] = n - 1
        if lib.hostemu_live_objects() != before:
            bad.append("%s: %d objects left by the call that got through" % (name, lib.hostemu_live_objects() - before))
        if not differing(t0, tables(m)):
            bad.append("%s: the call that got through copied nothing" % name)
        m.close()
    if counts != {"direct": 1, "staged": 2}:               # the pairs; the pairs and the stage
        bad.append("refusals %s" % counts)
    log("copy cells refusals: %d + %d refused; problems: %s" % (counts["direct"], counts["staged"], bad or "none"), flush=True)
    return bad


def check_group(log=print, devices=(0, 0, 0)):
    """A group of three shards on one device next to one context: fan-out, rotation and resample with STATE | BALANCE, behind a
    step; every table equal, then a record on both."""
    E = quickflux()
    bad = []
    for name in ("fanout", "rotation", "resample"):
        dst, src, _ = patterns(E)[name]
        one, g = model(E), model(E, cls=Group, devices=list(devices))
        bounds = g.shard_bounds()
        shard = lambda c: np.searchsorted(bounds, c, side="right") - 1
        if not (shard(dst) != shard(src)).any():
            bad.append(name + ": no pair crosses a shard boundary")
        for m in (one, g):
            m.dist_prec(0, 1)
            m.copy_cells(dst, src, STATE | BALANCE)
        tg, t1 = tables(g), tables(one)
        d = differing(tg, {k: t1[k] for k in tg})
        ro, rg = run_records(one, 1, 1), run_records(g, 1, 1)
        tg, t1 = tables(g), tables(one)
        d += ["after a record: " + k for k in differing(tg, {k: t1[k] for k in tg})]
        if not same(ro, rg):
            d.append("the record after the copy")
        if not (np.isfinite(ro).all() and ro.any()):
            d.append("the context's record is not finite or all zero")
        one.close(); g.close()
        log("copy cells group %s: bounds %s, differing: %s" % (name, bounds.tolist(), d or "none"), flush=True)
        bad += ["%s: %s" % (name, x) for x in d]
    return bad


def check_large(log=print, stage_mb=None):
    """4 members x 2 000 cells (QUICK_FLUX, 6 HRUs a cell): the rotation, against the host path right after the copy."""
    E = ensemble(dict(FULL_ENERGY=1, Nband=3), 2000, 4, 2, 1, 80)
    dst, src = members(E, [(1, 0), (2, 1), (3, 2), (0, 3)])
    a, b = model(E, stage_mb, put=False), model(E, put=False)
    a.copy_cells(dst, src)
    host_copy(b, dst, src)
    ta, tb = tables(a, put=False), tables(b, put=False)
    bad = differing(tb, ta)
    if same(ta["sd"], E.sd0):
        bad.append("the copy changed nothing")
    a.close(); b.close()
    log("copy cells large (stage %s MB): %d HRUs, differing: %s" % (stage_mb or "default", E.D.nhru, bad or "none"), flush=True)
    return bad


if __name__ == "__main__":
    cmd = sys.argv[1]
    if cmd == "errors":
        problems, _ = error_returns()
    else:
        problems = {"patterns": check_patterns, "frozen": check_frozen, "continuation": check_continuation, "untouched": check_untouched,
                    "refusals": check_refusals, "group": check_group, "large": check_large}[cmd]()
    print("copy cells %s: problems: %s" % (cmd, problems or "none"), flush=True)
    sys.exit(1 if problems else 0)
