"""Output records (vicgpu_run_records, include/vicgpu_out.h) through the host build of the library, against the loop they
replace.  Run by tests/test_records.py with VICGPU_LIB pointing at the unsanitized host build (SAN=none tools/hostemu/build.sh):
    python tools/hostemu/check_records.py run <case> [<case> ...]
        one Model (or Group) runs vicgpu_run_records, a second one from the same state runs, record by record,
        vicgpu_step + vicgpu_get_outputs(reset) + vicgpu_get_cell_errors; every record, the error flags, the final state,
        fluxes, balance, accumulators and cell outputs must be bit-identical, and the aggregates zero afterwards
    python tools/hostemu/check_records.py errors
        every error return the header lists
    python tools/hostemu/check_records.py refusals
        vicgpu_records_config under a runtime that refuses its n-th allocation, for every n: VICGPU_ERR_HIP and nothing left
        behind; nothing is left behind by nvar = 0 and by closing a context whose records ran either"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from vic_amd import abi, domain, init_state
from vic_amd.abi import C
from vic_amd.api import Group, Model, load_library

# out of table order, every aggregation type (END, SUM, AVG, the resistances vic_put_finish aggregates) and element kind
OUT = ["OUT_SWE_BAND", "OUT_RUNOFF", "OUT_SURF_TEMP", "OUT_SOIL_MOIST", "OUT_AERO_RESIST", "OUT_SWE"]

CASES = {
    # name: options, cells, tiles, start day, R, records, depths, steps before the first record, VICGPU_CHUNKS, group devices
    "quickflux": (dict(FULL_ENERGY=1, Nband=3), 7, 2, 80, 3, 4, (1, 2), 1, None, None),
    "waterbalance_daily": (dict(FULL_ENERGY=0, dt=24, snow_step=3), 7, 2, 60, 1, 5, (2,), 0, None, None),
    "frozen_chunks": (dict(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=10, Nband=2, frozen_compat=0), 5, 2, 330, 2, 2, (2,), 0, "2", None),
    "group": (dict(FULL_ENERGY=1, Nband=3), 7, 2, 80, 3, 4, (2,), 1, None, [0, 0, 0]),
}


def _tables(m):
    r = {}
    r["sd"], r["si"] = m.get_state()
    r["flux"] = m.get_fluxes()
    r["balance"] = m.get_balance()
    r["accum"] = m.get_accum() if not isinstance(m, Group) else np.zeros(1)
    r["cell_out"] = m.get_cell_outputs() if not isinstance(m, Group) else np.zeros(1)
    r["agg_after"] = m.get_output_data(OUT, aggregated=True) if not isinstance(m, Group) else m.get_outputs(OUT, reset=False)
    r["nlaunch"] = np.asarray(m.last_kernel_ms()[1]) if not isinstance(m, Group) else np.zeros(1)
    return r


def _start(make, d, f, sf, dmy, sd0, si0, R, pre):
    m = make()
    m.set_state(sd0, si0)
    m.put_data_config(R)
    m.put_data_init()
    m.push_forcing(f, sf, dmy)
    if pre:
        m.dist_prec(0, pre)          # record 0 includes what the aggregates held
    return m


def run_case(name):
    kw, ncell, ntile, doy, R, nrec, depths, pre, chunks, devices = CASES[name]
    if chunks:
        os.environ["VICGPU_CHUNKS"] = chunks
    else:
        os.environ.pop("VICGPU_CHUNKS", None)
    opt = abi.default_options(**kw)
    d = domain.make_domain(ncell, opt, ntile=ntile)
    nsteps = pre + R * nrec
    f, sf, dmy = domain.make_forcing(d, 0, nsteps, start_doy=doy)
    sd0, si0 = init_state.initial_state(d, f[0])
    make = (lambda: Group(d, devices=devices)) if devices else (lambda: Model(d))
    # the loop
    a = _start(make, d, f, sf, dmy, sd0, si0, R, pre)
    want_out, want_err = [], []
    for k in range(nrec):
        a.dist_prec(pre + k * R, R, sync=False)
        want_out.append(a.get_outputs(OUT, reset=True))
        want_err.append(a.get_cell_errors())
    want = _tables(a)
    want["out"], want["errors"] = np.stack(want_out), np.stack(want_err)
    a.close()
    rc = 0
    for depth in depths:
        b = _start(make, d, f, sf, dmy, sd0, si0, R, pre)
        b.records_config(OUT, depth=depth)
        rec = b.run_records(pre, nrec, errors=True)
        rec.wait(0)
        rec.wait()
        got = _tables(b)
        got["out"], got["errors"] = rec.out.copy(), rec.errors.copy()
        bad = [k for k in want if not np.array_equal(want[k], got[k], equal_nan=True)]
        zero = not got["agg_after"].any()
        # a second call on the same configuration, without errors, reuses the slots: the next records of a fresh chunk
        b.push_forcing(f, sf, dmy)
        rec2 = b.run_records(pre, 1, errors=False)
        rec2.wait()
        again = rec2.errors is None and rec2.out.shape == (1,) + want["out"].shape[1:] and np.isfinite(rec2.out).all()
        del rec, rec2
        b.close()
        print("hostemu records %s depth %d: %d records of %d rows x %d cells, %d tables, aggregates zero: %s, second call: %s, differing: %s"
              % (name, depth, nrec, want["out"].shape[1], ncell, len(want), zero, again, bad or "none"), flush=True)
        if bad or not zero or not again or not np.isfinite(want["out"]).all() or not want["out"].any():
            rc = 1
    return rc


def errors():
    lib = load_library()
    ARG, STATE, OK = C["VICGPU_ERR_ARG"], C["VICGPU_ERR_STATE"], 0
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int)
    checks = []

    def want(what, got, code):
        checks.append((what, got, code))

    # null handles
    one = np.zeros(1, dtype=np.int32)
    for pre in ("vicgpu_", "vicgpu_group_"):
        want(pre + "records_config(NULL)", getattr(lib, pre + "records_config")(None, 1, one.ctypes.data_as(ip), 2), ARG)
        want(pre + "records_nrow(NULL)", getattr(lib, pre + "records_nrow")(None), ARG)
        want(pre + "run_records(NULL)", getattr(lib, pre + "run_records")(None, 0, 1, None, None), ARG)
        want(pre + "records_wait(NULL)", getattr(lib, pre + "records_wait")(None, -1), ARG)

    opt = abi.default_options(FULL_ENERGY=1, Nband=3)
    d = domain.make_domain(7, opt, ntile=2)
    R, nrec = 2, 3
    f, sf, dmy = domain.make_forcing(d, 0, R * nrec, start_doy=80)
    sd0, si0 = init_state.initial_state(d, f[0])
    m = Model(d)
    m.set_state(sd0, si0)
    ids = m.var_ids(OUT)
    nrow = m._out_rows(ids)
    out = m.pinned((nrec, nrow, d.ncell), np.float32)
    err = m.pinned((nrec, d.ncell), np.int32)
    pageable_out, pageable_err = np.zeros(out.shape, np.float32), np.zeros(err.shape, np.int32)
    cfg = lambda i, depth: lib.vicgpu_records_config(m.h, len(i), i.ctypes.data_as(ip), depth)
    run = lambda s0, n, o, e: lib.vicgpu_run_records(m.h, s0, n, o.ctypes.data_as(fp), e.ctypes.data_as(ip) if e is not None else None)

    want("records_config before put_data_config", cfg(ids, 2), STATE)
    want("records_nrow before records_config", lib.vicgpu_records_nrow(m.h), STATE)
    m.put_data_config(R)
    m.put_data_init()
    want("run_records before records_config", run(0, 1, out, err), STATE)
    want("records_wait before records_config", lib.vicgpu_records_wait(m.h, -1), STATE)
    want("depth 0", cfg(ids, 0), ARG)
    bad = ids.copy(); bad[1] = lib.vicgpu_out_nvar()
    want("id out of range", cfg(bad, 2), ARG)
    bad = ids.copy(); bad[1] = -1
    want("negative id", cfg(bad, 2), ARG)
    twice = np.concatenate([ids, ids[:1]])
    want("id listed twice", cfg(twice, 2), ARG)
    want("records_nrow after refused configurations", lib.vicgpu_records_nrow(m.h), STATE)
    want("records_config", cfg(ids, 2), OK)
    want("records_nrow", lib.vicgpu_records_nrow(m.h), nrow)
    want("run_records without a forcing chunk", run(0, 1, out, err), STATE)
    m.push_forcing(f, sf, dmy)
    want("records_wait before any run", lib.vicgpu_records_wait(m.h, -1), STATE)
    want("nrecords 0", run(0, 0, out, err), ARG)
    want("negative step0", run(-1, 1, out, err), ARG)
    want("past the chunk", run(R, nrec, out, err), ARG)
    want("out NULL", lib.vicgpu_run_records(m.h, 0, nrec, None, None), ARG)
    want("out not pinned", run(0, nrec, pageable_out, err), ARG)
    want("cell_err not pinned", run(0, nrec, out, pageable_err), ARG)
    want("records_wait after refused runs", lib.vicgpu_records_wait(m.h, -1), STATE)
    want("run_records", run(0, nrec, out, err), OK)
    want("records_wait(k = nrecords)", lib.vicgpu_records_wait(m.h, nrec), ARG)
    want("records_wait(-2)", lib.vicgpu_records_wait(m.h, -2), ARG)
    want("records_wait(last)", lib.vicgpu_records_wait(m.h, nrec - 1), OK)
    want("records_wait(-1)", lib.vicgpu_records_wait(m.h, -1), OK)
    want("run_records without cell_err", run(0, 1, out, None), OK)
    want("synchronize", lib.vicgpu_synchronize(m.h), OK)
    # what drops the configuration
    m.put_data_config(R)
    want("run_records after put_data_config", run(0, 1, out, err), STATE)
    want("records_nrow after put_data_config", lib.vicgpu_records_nrow(m.h), STATE)
    want("records_config again", cfg(ids, 1), OK)
    m.set_domain(d)
    want("records_nrow after set_domain", lib.vicgpu_records_nrow(m.h), STATE)
    m.set_state(sd0, si0); m.put_data_config(R)
    want("records_config on the new domain", cfg(ids, 3), OK)
    want("nvar 0 releases", lib.vicgpu_records_config(m.h, 0, None, 0), OK)
    want("records_nrow after release", lib.vicgpu_records_nrow(m.h), STATE)
    m.close()
    failed = [(w, g, c) for w, g, c in checks if g != c]
    for w, g, c in failed:
        print("records error return: %s gave %d, want %d" % (w, g, c), flush=True)
    print("hostemu records errors: %d checks, failed: %d" % (len(checks), len(failed)), flush=True)
    return 1 if failed else 0


def refusals():
    """vicgpu_records_config with the n-th allocation refused (hostemu_refuse_alloc), n = 1, 2, ...: VICGPU_ERR_HIP, the count of
    live runtime objects where it was and no configuration, until the call gets through; what it then owns goes with
    nvar = 0, and a configuration in use goes with the context."""
    lib = load_library()
    lib.hostemu_live_objects.restype = ctypes.c_longlong
    lib.hostemu_refuse_alloc.argtypes = [ctypes.c_longlong]
    live0 = lib.hostemu_live_objects()
    os.environ["VICGPU_CHUNKS"] = "2"
    opt = abi.default_options(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=10, Nband=2, frozen_compat=0)
    d = domain.make_domain(5, opt, ntile=2)
    f, sf, dmy = domain.make_forcing(d, 0, 2, start_doy=330)
    sd0, si0 = init_state.initial_state(d, f[0])
    m = _start(lambda: Model(d), d, f, sf, dmy, sd0, si0, 1, 0)
    ids = m.var_ids(OUT)
    bad = []
    before = lib.hostemu_live_objects()
    for n in range(1, 50):
        lib.hostemu_refuse_alloc(n)
        rc = lib.vicgpu_records_config(m.h, len(ids), ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 3)
        lib.hostemu_refuse_alloc(0)
        if rc == 0:
            break
        if rc != C["VICGPU_ERR_HIP"] or lib.hostemu_live_objects() != before or lib.vicgpu_records_nrow(m.h) != C["VICGPU_ERR_STATE"]:
            bad.append("allocation %d refused: code %d, %d objects more" % (n, rc, lib.hostemu_live_objects() - before))
    owned = lib.hostemu_live_objects() - before
    if n != 1 + 2 * 3 + 1:           # the row map and three slots of two buffers were refused once each
        bad.append("%d refusals" % (n - 1))
    lib.vicgpu_records_config(m.h, 0, None, 0)
    if lib.hostemu_live_objects() != before:
        bad.append("%d objects left by nvar = 0" % (lib.hostemu_live_objects() - before))
    m.records_config(OUT, depth=2)
    rec = m.run_records(0, 2, errors=True)
    rec.wait()
    del rec
    m.close()
    left = lib.hostemu_live_objects() - live0
    if left:
        bad.append("%d objects left after close" % left)
    print("hostemu records refusals: %d refused, then through owning %d objects; problems: %s" % (n - 1, owned, bad or "none"), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "run":
        sys.exit(max(run_case(n) for n in sys.argv[2:]))
    sys.exit({"errors": errors, "refusals": refusals}[sys.argv[1]]())
