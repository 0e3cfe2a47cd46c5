"""Who owns the runtime objects of the host layer (vic_amd/csrc/vic_host.hpp), through the sanitizer build of the library.
Run by tests/test_hostemu_sanitizers.py with the ASan runtime preloaded and VICGPU_LIB pointing at the host build:
    python tools/hostemu/check_lifecycle.py lifecycle
        per option set: create -> state -> put_data -> forcing from pinned memory -> 2 steps -> every read-back (none may
        change the number of live runtime objects) -> a second vicgpu_set_domain on the same handle (must compute what a
        fresh context computes, bit for bit) -> close (the count is back where it was before create)
    python tools/hostemu/check_lifecycle.py refusals
        on the frozen 10-node case: every call that allocates is given a runtime that refuses its n-th allocation
        (hostemu_refuse_alloc), n = 1, 2, ... until the call gets through.  Every refused call returns VICGPU_ERR_HIP and
        leaves the object count where it was; the first call that gets through computes what an undisturbed context does
The domain is 5 cells x 2 tiles, 2 steps, VICGPU_CHUNKS=2."""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
os.environ["VICGPU_CHUNKS"] = "2"
from tests import brent_cases as bc
from tests import node_cases as nc
from vic_amd import abi, domain, init_state
from vic_amd.abi import C
from vic_amd.api import Model, VicGpuError, _d, load_library

FROZEN = dict(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=10, Nband=2, frozen_compat=0)
CASES = {
    # name: option overrides, glacier top band
    "quickflux": (dict(FULL_ENERGY=1), False),
    "frozen_glacier": (FROZEN, True),
    "implicit": (dict(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=5, IMPLICIT=1, frozen_compat=0), False),
}
OUT = ["OUT_RUNOFF", "OUT_BASEFLOW", "OUT_SWE", "OUT_SOIL_MOIST", "OUT_EVAP", "OUT_GLAC_MBAL", "OUT_SOIL_TNODE"]
NSTEPS = 2
LIB = load_library()
LIB.hostemu_live_objects.restype = ctypes.c_longlong
LIB.hostemu_refuse_alloc.argtypes = [ctypes.c_longlong]
live = LIB.hostemu_live_objects
FAILED = []


def check(ok, what):
    if not ok:
        FAILED.append(what)
        print("  FAILED: " + what, flush=True)


def same(a, b):
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b, equal_nan=True)


def setup(kw, glacier, ncell, ntile):
    opt = abi.default_options(**kw)
    d = domain.make_domain(ncell, opt, ntile=ntile, glacier_top_band=glacier)
    f, sf, dmy = domain.make_forcing(d, 0, NSTEPS, start_doy=120)
    sd0, si0 = init_state.initial_state(d, f[0])
    return d, f, sf, dmy, sd0, si0


def run_steps(m, f, sf, dmy, sd0, si0):
    m.set_state(sd0, si0)
    m.put_data_config(NSTEPS)
    m.put_data_init()
    fp = m.pinned(f.shape); fp[:] = f
    m.push_forcing(fp, sf, dmy)
    m.dist_prec(0, NSTEPS)


def read_backs(m):
    r = dict(out=m.get_outputs(OUT, reset=False), flux=m.get_fluxes(), records=m.get_state_records(), balance=m.get_balance(),
             fit=m.glacier_mass_balance_fit(reset=False), errors=m.get_cell_errors())
    r["sd"], r["si"] = m.get_state()
    return r


def lifecycle():
    for name, (kw, glacier) in CASES.items():
        big, small = setup(kw, glacier, 5, 2), setup(kw, glacier, 3, 1)
        live0 = live()
        m = Model(big[0])
        run_steps(m, *big[1:])
        n = live()
        read_backs(m)
        check(live() == n, "%s: the read-backs changed the object count by %d" % (name, live() - n))
        m.set_domain(small[0])
        run_steps(m, *small[1:])
        second = read_backs(m)
        fresh_model = Model(small[0])
        run_steps(fresh_model, *small[1:])
        fresh = read_backs(fresh_model)
        bad = [k for k in fresh if not same(fresh[k], second[k])]
        check(not bad, "%s: second domain differs from a fresh context in %s" % (name, bad))
        fresh_model.close()
        m.close()
        check(live() == live0, "%s: %d objects left after close" % (name, live() - live0))
        print("lifecycle %s: %d objects with the domain, %d left after close, second domain differs in: %s"
              % (name, n - live0, live() - live0, bad or "nothing"), flush=True)


def sweep(what, call, expect=None, may_grow=False, allocates=True):
    """call() with the n-th allocation refused, n = 1, 2, ... until it gets through; returns what that call returned.
    expect: the object count a refused call must leave (default: the count before the call)."""
    for n in range(1, 201):
        before = live()
        LIB.hostemu_refuse_alloc(n)
        try:
            r = call()
        except VicGpuError as e:
            after = live()
            want = before if expect is None else expect
            check("(%d)" % C["VICGPU_ERR_HIP"] in str(e), "%s, allocation %d refused: %s" % (what, n, e))
            check(after == want or (may_grow and after >= want), "%s, allocation %d refused: object count %d -> %d (want %d)" % (what, n, before, after, want))
            continue
        finally:
            LIB.hostemu_refuse_alloc(0)
        print("refusals %s: %d refused, then through" % (what, n - 1), flush=True)
        check((n > 1) == allocates, "%s: %d allocations were refused" % (what, n - 1))
        return r
    check(False, "%s: still refused at allocation 200" % what)
    raise SystemExit(1)


def bare_model(d):
    """A context with the vegetation library and no domain."""
    m = Model.__new__(Model)
    m.lib, m.dom, m.opt, m.h = LIB, d, d.opt, ctypes.c_void_p()
    assert LIB.vicgpu_create(ctypes.byref(d.opt), 0, ctypes.byref(m.h)) == 0
    m._chk(LIB.vicgpu_set_veglib(m.h, d.veglib.shape[0], _d(np.ascontiguousarray(d.veglib))))
    return m


def refusals():
    d, f, sf, dmy, sd0, si0 = setup(FROZEN, True, 5, 2)
    raw = np.zeros((NSTEPS, C["VIC_NRAW"], d.opt.dt, d.ncell))
    for name, src, scale in (("VIC_RAW_AIR_TEMP", "VIC_F_AIR_TEMP", 1.0), ("VIC_RAW_PREC", "VIC_F_PREC", 1.0), ("VIC_RAW_PRESSURE_KPA", "VIC_F_PRESSURE", 1e-3),
                             ("VIC_RAW_VP_KPA", "VIC_F_VP", 1e-3), ("VIC_RAW_SHORTWAVE", "VIC_F_SHORTWAVE", 1.0), ("VIC_RAW_LONGWAVE", "VIC_F_LONGWAVE", 1.0),
                             ("VIC_RAW_WIND", "VIC_F_WIND", 1.0)):
        raw[:, C[name]] = f[:, C[src], :d.opt.NF] * scale
    nodes = nc.make_battery(n_plain=6, n_nose=2)[0]
    g = bc.load_fixture()
    bounds, fvals, off = bc.gather(g, [0, 1, 2])
    pure = np.array([[0.5], [2.0], [10.0]])
    live0 = live()

    def sequence(m, through):
        """The calls of the check in one order; `through(what, call, **kw)` runs one of them.  Returns every result."""
        r = {}
        nodomain = live()
        through("set_domain", lambda: m.set_domain(d), expect=nodomain)
        m.set_state(sd0, si0)

        def config():
            try:
                m.put_data_config(NSTEPS)
            except VicGpuError:             # a failed call leaves put_data off, not half-configured
                check(LIB.vicgpu_put_data_init(m.h) == C["VICGPU_ERR_STATE"], "put_data is on after a failed put_data_config")
                raise
        through("put_data_config", config)
        m.put_data_init()
        n0 = live()
        through("prefetch_forcing (pageable)", lambda: m.prefetch_forcing(f, sf, dmy), may_grow=True)
        r["slot_objects"] = live() - n0
        n1 = live()
        through("prefetch_forcing (pageable), again", lambda: m.prefetch_forcing(f, sf, dmy), allocates=False)
        check(live() == n1, "a repeated prefetch_forcing grew the object count by %d" % (live() - n1))
        m.swap_forcing()
        m.dist_prec(0, NSTEPS)
        r["state"], r["flux"], r["errors"] = m.get_state(), m.get_fluxes(), m.get_cell_errors()
        r["out"] = through("get_outputs", lambda: m.get_outputs(OUT, reset=False))
        n0 = live()
        through("prefetch_forcing_raw", lambda: m.prefetch_forcing_raw(raw, dmy, 0.1, True), may_grow=True)
        r["raw_slot_objects"] = live() - n0
        n1 = live()
        through("prefetch_forcing_raw, again", lambda: m.prefetch_forcing_raw(raw, dmy, 0.1, True), allocates=False)
        check(live() == n1, "a repeated prefetch_forcing_raw grew the object count by %d" % (live() - n1))
        m.swap_forcing()
        r["derived"] = m.get_forcing(NSTEPS - 1)
        r["records"] = through("get_state_records", m.get_state_records)
        through("set_state_records", lambda: m.set_state_records(r["records"]))
        r["state_after_records"] = m.get_state()
        r["fit"] = through("glacier_mass_balance_fit", lambda: m.glacier_mass_balance_fit(reset=True))
        r["state_after_fit"] = m.get_state()
        r["pure"] = through("debug_pure", lambda: m.debug_pure(C["VICGPU_PURE_LN_POS"], pure))
        r["node"] = through("debug_node_root", lambda: m.debug_node_root(0, nodes))
        r["brent"] = through("debug_root_brent", lambda: m.debug_root_brent(C["VICGPU_BRENT_FULL"], bounds, fvals, off))
        return r

    plain, swept = bare_model(d), bare_model(d)
    want = sequence(plain, lambda what, call, **kw: call())
    got = sequence(swept, sweep)
    bad = [k for k in want if not same(want[k], got[k])]
    check(not bad, "after the refusals the context differs from an undisturbed one in %s" % bad)
    plain.close()
    swept.close()
    check(live() == live0, "%d objects left after close" % (live() - live0))
    print("refusals: differing from the undisturbed context: %s; %d objects left after close" % (bad or "nothing", live() - live0), flush=True)


if __name__ == "__main__":
    {"lifecycle": lifecycle, "refusals": refusals}[sys.argv[1]]()
    print("check_lifecycle %s: %d problems" % (sys.argv[1], len(FAILED)), flush=True)
    sys.exit(1 if FAILED else 0)
