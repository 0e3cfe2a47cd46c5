"""Cell validity (vicgpu_set_retire_on_error / vicgpu_set_cell_valid / vicgpu_get_cell_valid, include/vicgpu.h): what the
reference driver does with cell.isValid and CONTINUEONERROR (vicNl.c:429, 521, 545-559), decided on the device.

The checks live here and take the domain size as an argument: tests/test_cell_valid.py runs them on tiny domains through the
unsanitized host build of the library (SAN=none tools/hostemu/build.sh, VICGPU_LIB pointing at it) in a child process,
    python tools/hostemu/check_cell_valid.py <case> [<case> ...]        cases: CPU_CASES below, errors
and tests/test_cell_valid_gpu.py imports them and runs them on the GPU at sizes that fill a wave and leave a tail.

Every retirement check runs three models from the same initial state on the `stress` forcing of tests/scenarios.py (60000
W/m2 of shortwave at steps 5, 12, ... on the cells c % 3 == 1, TFALLBACK = 0: the ground-surface root finder returns ERROR):
  X  retire mask 0                              one dist_prec(s, 1) at a time, every table read back after every step
  Y  retire mask VICGPU_CELLERR_REFERENCE       the same
  Z  the same mask                              records_config + run_records(0, 4): retirement in the middle of one call
All comparisons are bit for bit (np.array_equal, NaN == NaN)."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from vic_amd import abi, domain, init_state   # noqa: E402
from vic_amd.abi import C                     # noqa: E402

# the list of tests/test_records_gpu.py: out of table order, every aggregation type and element kind
OUT = ["OUT_SWE_BAND", "OUT_RUNOFF", "OUT_SURF_TEMP", "OUT_SOIL_MOIST", "OUT_AERO_RESIST", "OUT_SWE"]
R, NREC = 4, 4
NSTEPS = R * NREC
FAIL = 5                              # the first step of the stress forcing
HRU_TABLES = ("sd", "si", "flux")     # tables whose columns are HRUs; every other one has a column per cell

MONOLITH = dict(FULL_ENERGY=1, TFALLBACK=0, Nband=3)
FROZEN = dict(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=10, Nband=2, frozen_compat=0, TFALLBACK=0)


def eq(a, b):
    return np.array_equal(a, b, equal_nan=True)


def make_case(kw, ncell, doy, glacier=False, stress=True, nsteps=NSTEPS):
    opt = abi.default_options(**kw)
    d = domain.make_domain(ncell, opt, ntile=2, glacier_top_band=glacier)
    f, sf, dmy = domain.make_forcing(d, 0, nsteps, start_doy=doy)
    if stress:
        # the `stress` tweak of tests/scenarios.py
        sw = C["VIC_F_SHORTWAVE"]
        cells = np.arange(d.ncell) % 3 == 1
        for s in range(5, nsteps, 7):
            f[s, sw][:, cells] = 60000.0
    sd0, si0 = init_state.initial_state(d, f[0])
    if glacier:
        sd0[C["SD_GLAC_CUM_MASS_BALANCE"], d.hru_iparams[C["HPI_IS_GLACIER"]] != 0] = 0.0
    return d, f, sf, dmy, sd0, si0


def start(m, f, sf, dmy, sd0, si0, mask=0, invalid=None):
    m.set_retire_on_error(mask)
    m.set_state(sd0, si0)
    m.put_data_config(R)
    if invalid is not None:
        m.set_cell_valid(~invalid)
    m.put_data_init()
    m.push_forcing(f, sf, dmy)
    return m


def snap(m, single=True):
    r = {}
    r["sd"], r["si"] = m.get_state()
    r["flux"] = m.get_fluxes()
    r["errors"] = m.get_cell_errors()
    r["balance"] = m.get_balance()
    r["agg"] = m.get_outputs(OUT, reset=False)
    if single:                        # entries without a group form
        r["cell_out"] = m.get_cell_outputs()
        r["accum"] = m.get_accum()
    return r


def stepwise(m, nsteps=NSTEPS, single=True):
    """One dist_prec(s, 1) at a time: (snapshot after every step, validity after every step, records, flag words per record)."""
    snaps, valid, recs, errs = [], [], [], []
    for s in range(nsteps):
        m.dist_prec(s, 1)
        snaps.append(snap(m, single))
        valid.append(m.get_cell_valid())
        if (s + 1) % R == 0:
            recs.append(m.get_outputs(OUT, reset=True))
            errs.append(m.get_cell_errors())
    return snaps, valid, np.stack(recs), np.stack(errs)


def cols(d, name, table, cells):
    """The columns of `table` that belong to the cells of the boolean mask `cells`."""
    return table[..., cells[d.hru_iparams[C["HPI_CELL"]]] if name in HRU_TABLES else cells]


def differing(d, a, b, cells=None, skip=()):
    """Names of the tables of snapshot a that differ from b (on the columns of `cells` when given)."""
    assert sorted(a) == sorted(b)
    if cells is None:
        return [k for k in a if k not in skip and not eq(a[k], b[k])]
    return [k for k in a if k not in skip and not eq(cols(d, k, a[k], cells), cols(d, k, b[k], cells))]


def failing_cells(d, f, sf, dmy, sd0, si0, x_snaps):
    """The cells of the stress forcing, after the proof that the inputs do what the test needs: run X flags exactly them after
    step FAIL and no cell before it, and so does the CPU oracle."""
    from oracle.pyref import OracleModel
    bad = np.arange(d.ncell) % 3 == 1
    assert bad.any() and not bad.all()
    assert not x_snaps[FAIL - 1]["errors"].any(), "run X has flags before step %d" % FAIL
    assert np.array_equal(x_snaps[FAIL]["errors"] != 0, bad), ("run X flags after step %d" % FAIL, x_snaps[FAIL]["errors"])
    assert (x_snaps[FAIL]["errors"][bad] & C["VICGPU_CELLERR_REFERENCE"]).all()
    orc = OracleModel(d)
    orc.set_state(sd0, si0)
    for s in range(FAIL + 1):
        _, _, eo = orc.step(f[s], sf[s], dmy[s])
        want = bad if s == FAIL else np.zeros(d.ncell, dtype=bool)
        assert np.array_equal(eo != 0, want), ("oracle flags at step %d" % s, eo)
    orc.close()
    return bad


def check_retirement(make, kw, ncell, doy, glacier=False):
    """Assertions 1 to 6 of the header on one domain.  make(d) -> Model."""
    d, f, sf, dmy, sd0, si0 = make_case(kw, ncell, doy, glacier)
    hru_cell = d.hru_iparams[C["HPI_CELL"]]
    x = start(make(d), f, sf, dmy, sd0, si0, 0)
    xs, xv, xrec, xerr = stepwise(x)
    bad = failing_cells(d, f, sf, dmy, sd0, si0, xs)
    assert all(v.all() for v in xv), "a cell became invalid with mask 0"
    y = start(make(d), f, sf, dmy, sd0, si0, C["VICGPU_CELLERR_REFERENCE"])
    ys, yv, yrec, yerr = stepwise(y)
    y_final = snap(y)
    # 1: through the failing step Y is X
    for s in range(FAIL + 1):
        assert not differing(d, xs[s], ys[s]), ("step %d" % s, differing(d, xs[s], ys[s]))
        assert yv[s].all() == (s < FAIL)
    # 2: retired from the next step on, decided on the device
    for s in range(FAIL, NSTEPS):
        assert np.array_equal(yv[s], (~bad).astype(np.int32)), ("validity after step %d" % s, yv[s])
    froze = ys[FAIL]
    assert xs[FAIL + 7]["errors"][bad].all() and eq(xs[FAIL + 7]["errors"], xs[FAIL]["errors"])      # step 12 fails again in X
    for s in range(FAIL + 1, NSTEPS):
        # 3: the other cells never notice
        assert not differing(d, xs[s], ys[s], ~bad), ("valid cells, step %d" % s, differing(d, xs[s], ys[s], ~bad))
        # 4: nothing of a retired cell changes (its aggregates: assertion 5)
        assert not differing(d, froze, ys[s], bad, skip=("agg",)), ("retired cells, step %d" % s, differing(d, froze, ys[s], bad, skip=("agg",)))
        assert (ys[s]["accum"][C["CA_NSTEPS"], bad] == FAIL + 1).all()
        assert differing(d, xs[s], ys[s], bad), "step %d: run X did not move on the retired cells" % s
        agg = ys[s]["agg"][:, bad]
        assert eq(agg, froze["agg"][:, bad]) if s < 2 * R else not agg.any(), "aggregates of retired cells, step %d" % s
    # 5: the records
    assert eq(yrec[0], xrec[0])
    assert eq(yrec[1][:, bad], froze["agg"][:, bad]) and yrec[1][:, bad].any()
    assert not yrec[2:][:, :, bad].any(), "records 2 and 3 of retired cells are not 0.0"
    assert eq(yrec[:, :, ~bad], xrec[:, :, ~bad]) and eq(yerr[:, ~bad], xerr[:, ~bad])
    assert eq(yerr[1:, bad], np.broadcast_to(froze["errors"][bad], yerr[1:, bad].shape))
    if glacier:
        # the accumulated mass balance of a retired cell stays, the fit gives it the default equation and resets nothing
        isg = d.hru_iparams[C["HPI_IS_GLACIER"]] != 0
        cum = C["SD_GLAC_CUM_MASS_BALANCE"]
        assert isg.any() and xs[-1]["sd"][cum, isg].any()
        eqx, eqy = x.glacier_mass_balance_fit(reset=True), y.glacier_mass_balance_fit(reset=True)
        assert eq(eqy[:, bad], np.broadcast_to(np.array([[0.0], [0.0], [0.0], [-1.0]]), eqy[:, bad].shape)), eqy[:, bad]
        assert eq(eqy[:, ~bad], eqx[:, ~bad]) and (eqx[C["GMB_FIT_ERROR"], ~bad] >= 0).all() and (eqx[C["GMB_FIT_ERROR"], bad] >= 0).all()
        sdx, sdy = x.get_state()[0], y.get_state()[0]
        assert eq(sdy[:, bad[hru_cell]], froze["sd"][:, bad[hru_cell]]), "the fit touched a retired cell"
        assert eq(sdy[:, ~bad[hru_cell]], sdx[:, ~bad[hru_cell]]) and not sdy[cum, isg & ~bad[hru_cell]].any()
    x.close()
    # 6: retirement in the middle of one call
    z = start(make(d), f, sf, dmy, sd0, si0, C["VICGPU_CELLERR_REFERENCE"])
    z.records_config(OUT, depth=2)
    rec = z.run_records(0, NREC, errors=True)
    rec.wait()
    assert eq(rec.out, yrec), "run_records differs from the stepwise records"
    assert eq(rec.errors, yerr)
    del rec
    assert np.array_equal(z.get_cell_valid(), yv[-1])
    got = snap(z)
    assert not differing(d, y_final, got), differing(d, y_final, got)
    y.close()
    z.close()
    return int(bad.sum())


def check_host_validity(make, ncell=70):
    """The host's own isValid on the monolithic kernel without stress, mask 0: every 5th cell is invalid before put_data_init."""
    kw = dict(FULL_ENERGY=1, TFALLBACK=0, Nband=3)
    n = 2 * R
    d, f, sf, dmy, sd0, si0 = make_case(kw, ncell, 80, stress=False, nsteps=n + 1)
    off = np.arange(d.ncell) % 5 == 0
    a = start(make(d), f, sf, dmy, sd0, si0)
    a_first = snap(a)
    as_, _, arec, _ = stepwise(a, n)
    a.close()
    assert not as_[-1]["errors"].any()
    b = start(make(d), f, sf, dmy, sd0, si0, invalid=off)
    assert np.array_equal(b.get_cell_valid(), (~off).astype(np.int32))
    first = snap(b)
    assert eq(first["sd"], sd0) and eq(first["si"], si0) and not first["flux"].any()
    assert not first["balance"][:, off].any() and first["balance"][:, ~off].any(), "put_data_init on an invalid cell"
    assert not differing(d, a_first, first, ~off)
    bs, bv, brec, _ = stepwise(b, n)
    for s in range(n):
        assert np.array_equal(bv[s], (~off).astype(np.int32))
        assert not differing(d, first, bs[s], off), ("invalid cells, step %d" % s, differing(d, first, bs[s], off))
        assert not differing(d, as_[s], bs[s], ~off), ("valid cells, step %d" % s, differing(d, as_[s], bs[s], ~off))
    assert not brec[:, :, off].any() and eq(brec[:, :, ~off], arec[:, :, ~off]) and arec[:, :, off].any()
    # valid again: the cells resume from the tables as they stand
    b.set_cell_valid(np.ones(d.ncell, dtype=np.int32))
    assert b.get_cell_valid().all()
    sd1, si1 = b.get_state()
    fx1 = b.get_fluxes()
    b.dist_prec(n, 1)
    fresh = make(d)
    fresh.set_state(sd1, si1)
    fresh.set_fluxes(fx1)
    fresh.push_forcing(f, sf, dmy)
    fresh.dist_prec(n, 1)
    got, want = b.get_state(), fresh.get_state()
    assert eq(got[0], want[0]) and eq(got[1], want[1]) and eq(b.get_fluxes(), fresh.get_fluxes())
    hru_off = off[d.hru_iparams[C["HPI_CELL"]]]
    assert not eq(got[0][:, hru_off], sd1[:, hru_off]), "the cells did not resume"
    assert (b.get_accum()[C["CA_NSTEPS"]] == np.where(off, 1, n + 1)).all()
    b.close()
    fresh.close()
    return int(off.sum())


def check_group(make_group, make, ncell=70):
    """The monolithic stress case on a group of three shards against one context: validity table, records, final tables."""
    d, f, sf, dmy, sd0, si0 = make_case(MONOLITH, ncell, 80)
    mask = C["VICGPU_CELLERR_REFERENCE"]
    y = start(make(d), f, sf, dmy, sd0, si0, mask)
    ys, yv, yrec, yerr = stepwise(y, single=False)
    bad = np.arange(d.ncell) % 3 == 1
    assert np.array_equal(yv[-1], (~bad).astype(np.int32)) and yv[FAIL - 1].all()
    g = start(make_group(d), f, sf, dmy, sd0, si0, mask)
    assert g.get_cell_valid().all()
    g.dist_prec(0, R)                 # the first record stepwise, the other three in one call
    first = g.get_outputs(OUT, reset=True)
    g.records_config(OUT, depth=2)
    rec = g.run_records(R, NREC - 1, errors=True)
    rec.wait()
    assert eq(first, yrec[0]) and eq(rec.out, yrec[1:]) and eq(rec.errors, yerr[1:])
    del rec
    assert np.array_equal(g.get_cell_valid(), yv[-1])
    want, got = snap(y, single=False), snap(g, single=False)
    assert not differing(d, want, got), differing(d, want, got)
    # the group's table is in the caller's cell order, whatever the shard boundaries
    keep = np.arange(d.ncell) % 2 == 0
    g.set_cell_valid(keep)
    assert np.array_equal(g.get_cell_valid(), keep.astype(np.int32))
    y.close()
    g.close()
    return int(bad.sum())


def check_errors(make):
    """Every error return the header lists, and what the table and the mask survive."""
    from vic_amd.api import load_library
    lib = load_library()
    ARG, STATE, OK = C["VICGPU_ERR_ARG"], C["VICGPU_ERR_STATE"], 0
    ip = ctypes.POINTER(ctypes.c_int)
    checks = []

    def want(what, got, code):
        checks.append((what, got, code))

    d, f, sf, dmy, sd0, si0 = make_case(MONOLITH, 7, 80)
    one = np.ones(d.ncell, dtype=np.int32)
    p = one.ctypes.data_as(ip)
    for pre in ("vicgpu_", "vicgpu_group_"):
        want(pre + "set_retire_on_error(NULL)", getattr(lib, pre + "set_retire_on_error")(None, 0), ARG)
        want(pre + "set_cell_valid(NULL)", getattr(lib, pre + "set_cell_valid")(None, p), ARG)
        want(pre + "get_cell_valid(NULL)", getattr(lib, pre + "get_cell_valid")(None, p), ARG)
    # before a domain is set
    h = ctypes.c_void_p()
    assert lib.vicgpu_create(ctypes.byref(d.opt), 0, ctypes.byref(h)) == 0
    want("set_cell_valid before set_domain", lib.vicgpu_set_cell_valid(h, p), STATE)
    want("get_cell_valid before set_domain", lib.vicgpu_get_cell_valid(h, p), STATE)
    want("set_retire_on_error before set_domain", lib.vicgpu_set_retire_on_error(h, C["VICGPU_CELLERR_SOLVER"]), OK)
    lib.vicgpu_destroy(h)
    g = ctypes.c_void_p()
    dev = np.zeros(2, dtype=np.int32)
    assert lib.vicgpu_group_create(ctypes.byref(d.opt), 2, dev.ctypes.data_as(ip), ctypes.byref(g)) == 0
    want("group_set_cell_valid before set_domain", lib.vicgpu_group_set_cell_valid(g, p), STATE)
    want("group_get_cell_valid before set_domain", lib.vicgpu_group_get_cell_valid(g, p), STATE)
    want("group_set_retire_on_error before set_domain", lib.vicgpu_group_set_retire_on_error(g, 0), OK)
    want("group_set_retire_on_error(16)", lib.vicgpu_group_set_retire_on_error(g, 16), ARG)
    want("group_set_cell_valid(null table)", lib.vicgpu_group_set_cell_valid(g, None), ARG)
    want("group_get_cell_valid(null table)", lib.vicgpu_group_get_cell_valid(g, None), ARG)
    lib.vicgpu_group_destroy(g)
    m = make(d)
    want("set_cell_valid(null table)", lib.vicgpu_set_cell_valid(m.h, None), ARG)
    want("get_cell_valid(null table)", lib.vicgpu_get_cell_valid(m.h, None), ARG)
    for bad_mask in (16, -1, 1 << 30, 15 | 32):
        want("set_retire_on_error(%d)" % bad_mask, lib.vicgpu_set_retire_on_error(m.h, bad_mask), ARG)
    for mask in (0, 1, 2, 4, 8, 15, C["VICGPU_CELLERR_REFERENCE"]):
        want("set_retire_on_error(%d)" % mask, lib.vicgpu_set_retire_on_error(m.h, mask), OK)
    # the mask is the context's and survives vicgpu_set_domain, which makes every cell valid again; vicgpu_set_state and
    # vicgpu_reset_accum leave the table alone, vicgpu_reset_accum still clears the flags
    off = np.arange(d.ncell) % 2 == 1
    m.set_cell_valid(~off)
    m.set_domain(d)
    want("all valid after set_domain", int(m.get_cell_valid().all()), 1)
    start(m, f, sf, dmy, sd0, si0, mask=C["VICGPU_CELLERR_REFERENCE"])
    m.set_domain(d)
    m.set_state(sd0, si0)
    m.push_forcing(f, sf, dmy)
    m.dist_prec(0, FAIL + 2)
    retired = np.arange(d.ncell) % 3 == 1
    want("the mask survives set_domain", int(np.array_equal(m.get_cell_valid(), (~retired).astype(np.int32))), 1)
    m.set_state(sd0, si0)
    m.reset_accum()
    want("set_state and reset_accum keep the table", int(np.array_equal(m.get_cell_valid(), (~retired).astype(np.int32))), 1)
    want("reset_accum clears the flags", int(m.get_cell_errors().any()), 0)
    m.close()
    failed = [(w, g_, c) for w, g_, c in checks if g_ != c]
    for w, g_, c in failed:
        print("cell validity error return: %s gave %d, want %d" % (w, g_, c), flush=True)
    assert not failed, failed
    return len(checks)


# ---- the tiny domains of the CPU suite (host build of the library): name -> (what, VICGPU_CHUNKS)
def _cpu_model(d):
    from vic_amd.api import Model
    return Model(d)


def _cpu_group(d):
    from vic_amd.api import Group
    return Group(d, devices=[0, 0, 0])


CPU_CASES = {
    "monolith": (lambda: check_retirement(_cpu_model, MONOLITH, 7, 80), None),
    "frozen_chunks": (lambda: check_retirement(_cpu_model, FROZEN, 5, 330), "2"),
    "host_validity": (lambda: check_host_validity(_cpu_model, 7), None),
    "group": (lambda: check_group(_cpu_group, _cpu_model, 7), None),
    "errors": (lambda: check_errors(_cpu_model), None),
}


def main(names):
    rc = 0
    for name in names:
        fn, chunks = CPU_CASES[name]
        if chunks:
            os.environ["VICGPU_CHUNKS"] = chunks
        else:
            os.environ.pop("VICGPU_CHUNKS", None)
        try:
            n = fn()
            print("hostemu cell validity %s: ok (%d)" % (name, n), flush=True)
        except AssertionError as e:
            print("hostemu cell validity %s: FAILED: %s" % (name, e), flush=True)
            rc = 1
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
