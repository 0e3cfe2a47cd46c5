"""Output records without a host round trip per record (vicgpu_run_records, include/vicgpu_out.h) on the GPU.  Every case
runs the call on one Model (or Group) and, on a second one from the same state, the loop it replaces -- vicgpu_step +
vicgpu_get_outputs(reset) + vicgpu_get_cell_errors per record -- and compares bit for bit: the records, the error flags per
record, the final state, fluxes, balance and accumulators, and that the aggregates are zero afterwards.  Shapes are the
smallest that reach every path: a full wave plus a tail, a slot ring that wraps, two cell chunks, ragged shards."""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from vic_amd import abi, domain, init_state   # noqa: E402
from vic_amd.abi import C                     # noqa: E402

pytestmark = pytest.mark.gpu

# out of table order, every aggregation type (END, SUM, AVG, the resistances vic_put_finish aggregates) and element kind
OUT = ["OUT_SWE_BAND", "OUT_RUNOFF", "OUT_SURF_TEMP", "OUT_SOIL_MOIST", "OUT_AERO_RESIST", "OUT_SWE"]


def _start(m, f, sf, dmy, sd0, si0, R, pre=0):
    m.set_state(sd0, si0)
    m.put_data_config(R)
    m.put_data_init()
    m.push_forcing(f, sf, dmy)
    if pre:
        m.dist_prec(0, pre)
    return m


def _loop(m, step0, R, nrec, names):
    outs, errs = [], []
    for k in range(nrec):
        m.dist_prec(step0 + k * R, R, sync=False)
        outs.append(m.get_outputs(names, reset=True))
        errs.append(m.get_cell_errors())
    return np.stack(outs), np.stack(errs)


def _tables(m, names, single=True):
    r = {}
    r["sd"], r["si"] = m.get_state()
    r["flux"] = m.get_fluxes()
    r["balance"] = m.get_balance()
    r["aggregates"] = m.get_outputs(names, reset=False)
    if single:                       # entries without a group form
        r["accum"] = m.get_accum()
        r["cell_out"] = m.get_cell_outputs()
        r["nlaunch"] = np.asarray(m.last_kernel_ms()[1])
    return r


def _assert_same(want, got):
    assert sorted(want) == sorted(got)
    bad = [k for k in want if not np.array_equal(want[k], got[k], equal_nan=True)]
    assert not bad, "run_records differs from the loop in " + ", ".join(bad)
    assert not got["aggregates"].any(), "the aggregates are not zero after the call"
    assert np.isfinite(want["out"]).all() and want["out"].any()


def _compare(d, f, sf, dmy, sd0, si0, R, nrec, depth, names=OUT, pre=0, make_b=None):
    from vic_amd.api import Model
    a = _start(Model(d), f, sf, dmy, sd0, si0, R, pre)
    want_out, want_err = _loop(a, pre, R, nrec, names)
    want = _tables(a, names, single=make_b is None)
    want["out"], want["errors"] = want_out, want_err
    a.close()
    b = _start(make_b() if make_b else Model(d), f, sf, dmy, sd0, si0, R, pre)
    b.records_config(names, depth=depth)
    rec = b.run_records(pre, nrec, errors=True)
    rec.wait(0)
    first = rec.out[0].copy()        # record 0 is complete once wait(0) returns, whatever is still running
    rec.wait()
    got = _tables(b, names, single=make_b is None)
    got["out"], got["errors"] = rec.out.copy(), rec.errors.copy()
    del rec
    b.close()
    assert np.array_equal(first, want_out[0], equal_nan=True), "record 0 after wait(0)"
    _assert_same(want, got)
    return want


def _domain(kw, ncell, ntile, nsteps, doy):
    opt = abi.default_options(**kw)
    d = domain.make_domain(ncell, opt, ntile=ntile)
    f, sf, dmy = domain.make_forcing(d, 0, nsteps, start_doy=doy)
    sd0, si0 = init_state.initial_state(d, f[0])
    return d, f, sf, dmy, sd0, si0


def test_quick_flux_daily_records_ring_wraps():
    """QUICK_FLUX, 3 bands, 70 cells (a full wave and a tail of 6), R = 24, 3 records through 2 slots; one step aggregated before
    the first record, which must include it."""
    d, f, sf, dmy, sd0, si0 = _domain(dict(FULL_ENERGY=1, Nband=3), 70, 2, 1 + 72, 80)
    _compare(d, f, sf, dmy, sd0, si0, 24, 3, 2, pre=1)


def test_daily_water_balance_a_record_per_step():
    """FULL_ENERGY = 0, dt = 24, snow_step = 3, 65 cells, R = 1: 10 records through 3 slots, nothing between two records but one step."""
    d, f, sf, dmy, sd0, si0 = _domain(dict(FULL_ENERGY=0, dt=24, snow_step=3), 65, 2, 10, 60)
    _compare(d, f, sf, dmy, sd0, si0, 1, 10, 3)


@pytest.mark.parametrize("chunks", ["1", "2"])
def test_frozen_soil_chunks_deliver_their_own_columns(monkeypatch, chunks):
    """FROZEN_SOIL, 10 nodes, 2 bands, 24 cells x 2 tiles, R = 3, 4 records: the finite-difference pipeline as one chunk and as two,
    each packing and copying its own cell columns at its own record boundaries."""
    monkeypatch.setenv("VICGPU_CHUNKS", chunks)
    d, f, sf, dmy, sd0, si0 = _domain(dict(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=10, Nband=2, frozen_compat=0), 24, 2, 12, 330)
    _compare(d, f, sf, dmy, sd0, si0, 3, 4, 2)


def test_cfg4_shape_with_glacier_bands():
    """The cfg4 shape of bench.config (FROZEN_SOIL, 10 nodes, 5 bands x 5 tiles, glacier top band) at 48 cells, R = 2, 3 records."""
    import bench
    cfg = bench.config("cfg4")
    d = domain.make_domain(48, cfg["opt"], ntile=cfg["ntile"], glacier_top_band=True)
    f, sf, dmy = domain.make_forcing(d, 0, 6, start_doy=cfg["start_doy"])
    sd0, si0 = init_state.initial_state(d, f[0])
    sd0[C["SD_GLAC_CUM_MASS_BALANCE"], d.hru_iparams[C["HPI_IS_GLACIER"]] != 0] = 0.0
    names = ["OUT_GLAC_MBAL_BAND"] + OUT
    want = _compare(d, f, sf, dmy, sd0, si0, 2, 3, 2, names=names)
    assert want["out"][:, :cfg["opt"].Nband].any()       # the glacier band rows did something


def test_group_of_three_shards_against_one_context():
    """70 cells in 3 ragged shards on the visible devices: the group's records in the global tables against one context's loop."""
    import torch
    from vic_amd.api import Group
    n = max(torch.cuda.device_count(), 1)
    d, f, sf, dmy, sd0, si0 = _domain(dict(FULL_ENERGY=1, Nband=3), 70, 2, 12, 80)
    _compare(d, f, sf, dmy, sd0, si0, 3, 4, 2, make_b=lambda: Group(d, devices=[k % n for k in range(3)]))


def test_next_forcing_chunk_prefetched_while_records_are_in_flight():
    """Two forcing chunks of 12 steps, R = 3: the second is prefetched (from pinned memory) while run_records of the first is in
    flight and swapped in afterwards, without a wait in between; equal to the loop on the resident 24 steps."""
    from vic_amd.api import Model
    R, n = 3, 12
    d, f, sf, dmy, sd0, si0 = _domain(dict(FULL_ENERGY=1, Nband=3), 70, 2, 2 * n, 80)
    a = _start(Model(d), f, sf, dmy, sd0, si0, R)
    want_out, want_err = _loop(a, 0, R, 2 * n // R, OUT)
    want = _tables(a, OUT)
    a.close()
    b = _start(Model(d), f[:n], sf[:n], dmy[:n], sd0, si0, R)
    b.records_config(OUT, depth=2)
    pf, psf = b.pinned(f[n:].shape), b.pinned(sf[n:].shape, np.uint8)
    pf[...] = f[n:]; psf[...] = sf[n:]
    r0 = b.run_records(0, n // R, errors=True)
    b.prefetch_forcing(pf, psf, dmy[n:])
    b.swap_forcing()
    r1 = b.run_records(0, n // R, errors=True)
    r1.wait()                        # the download stream is in order: the first call's records landed before these
    got = _tables(b, OUT)
    got_out, got_err = np.concatenate([r0.out, r1.out]), np.concatenate([r0.errors, r1.errors])
    del r0, r1
    b.close()
    assert got["nlaunch"] == R       # vicgpu_last_kernel_ms: the steps of the last record
    assert np.array_equal(want_out, got_out, equal_nan=True) and np.array_equal(want_err, got_err)
    bad = [k for k in want if not np.array_equal(want[k], got[k], equal_nan=True)]
    assert not bad, bad


def test_cell_errors_per_record():
    """The stress_error scenario (TFALLBACK = 0, a shortwave flux no surface temperature balances every 7th step on a third of
    the cells): the flags of every record equal the loop's after that record, and they do change from record to record."""
    from tests import scenarios
    sp, d, f, sf, dmy = scenarios.build("stress_error", nsteps=20)
    sd0, si0 = init_state.initial_state(d, f[0])
    want = _compare(d, f, sf, dmy, sd0, si0, 4, 5, 2)
    per_record = (want["errors"] != 0).sum(axis=1)
    assert per_record[-1] > per_record[0], per_record    # the first failure comes at step 5, in the second record


def test_error_returns():
    """Every error return of the header on the real runtime (the pinned-memory test is the runtime's own there)."""
    spec = importlib.util.spec_from_file_location("check_records", os.path.join(ROOT, "tools", "hostemu", "check_records.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.errors() == 0
