"""The device group (include/vicgpu_group.h) on the GPU: one domain cut into shards, each shard a context of its own, stepped at
the same time from the group's host threads.  Shards are placed round-robin on the visible devices (all on device 0 when
there is one).  Cells never interact, so a group must compute exactly what one context computes on the whole domain: every
comparison here is bit for bit."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from vic_amd import domain, init_state   # noqa: E402
from vic_amd.abi import C                # noqa: E402

pytestmark = pytest.mark.gpu

OUT = ["OUT_RUNOFF", "OUT_BASEFLOW", "OUT_SWE", "OUT_SOIL_MOIST", "OUT_EVAP", "OUT_GLAC_MBAL", "OUT_SOIL_TNODE", "OUT_FDEPTH"]


def _devices(nshard):
    import torch
    n = max(torch.cuda.device_count(), 1)
    return [k % n for k in range(nshard)]


def _bench_setup(name, ncell, nsteps):
    """A bench.py workload shape at `ncell` cells."""
    import bench
    cfg = bench.config(name)
    d = domain.make_domain(ncell, cfg["opt"], ntile=cfg["ntile"], glacier_top_band=cfg.get("glacier", False))
    f, sf, dmy = domain.make_forcing(d, 0, nsteps, start_doy=cfg["start_doy"])
    sd0, si0 = init_state.initial_state(d, f[0])
    if cfg.get("glacier"):
        sd0[C["SD_GLAC_CUM_MASS_BALANCE"], d.hru_iparams[C["HPI_IS_GLACIER"]] != 0] = 0.0
    return d, f, sf, dmy, sd0, si0


def _run(m, f, sf, dmy, sd0, si0, ratio, glacier):
    nsteps = f.shape[0]
    m.set_state(sd0, si0)
    if ratio:
        m.put_data_config(ratio)
        m.put_data_init()
    m.push_forcing(f, sf, dmy)
    r = {}
    for k in range(0, nsteps, ratio or nsteps):
        m.dist_prec(k, ratio or nsteps)
        if ratio:
            r["out%d" % k] = m.get_outputs(OUT, reset=True)
    if ratio:
        r["balance"] = m.get_balance()
    r["sd"], r["si"] = m.get_state()
    r["flux"] = m.get_fluxes()
    r["records"] = m.get_state_records()
    r["errors"] = m.get_cell_errors()
    if glacier:
        r["fit"] = m.glacier_mass_balance_fit(reset=True)
        r["sd_after_fit"] = m.get_state()[0]
    m.close()
    return r


def _assert_same(one, grp):
    assert sorted(one) == sorted(grp)
    bad = [k for k in one if not np.array_equal(one[k], grp[k], equal_nan=True)]
    assert not bad, "group differs from one context in " + ", ".join(bad)


@pytest.mark.parametrize("solver", ["BRENT", "NEWTON"])
def test_cfg4_shape_three_shards(solver):
    """The cfg4 shape (FROZEN_SOIL, 10 nodes, 5 bands x 5 tiles, glacier top band) on 37 cells: 24 steps, put_data with a
    daily output record, 3 ragged shards."""
    from vic_amd.api import Group, Model
    d, f, sf, dmy, sd0, si0 = _bench_setup("cfg4", 37, 24)
    d.opt.NODE_SOLVER = C["VIC_NODE_SOLVER_" + solver]
    one = _run(Model(d), f, sf, dmy, sd0, si0, 24, True)
    g = Group(d, devices=_devices(3))
    b = g.shard_bounds()
    assert b[0] == 0 and b[-1] == d.ncell and len(set(np.diff(b))) > 1
    grp = _run(g, f, sf, dmy, sd0, si0, 24, True)
    _assert_same(one, grp)
    assert one["errors"].sum() == 0 and np.abs(one["out0"][2]).max() > 0       # SWE: the winter glacier domain did something


def test_cfg2_shape_quick_flux_two_shards():
    """The cfg2 shape (QUICK_FLUX, the single-kernel step, enqueued without blocking) on 301 cells, 2 shards, hourly output."""
    from vic_amd.api import Group, Model
    d, f, sf, dmy, sd0, si0 = _bench_setup("cfg2", 301, 12)
    one = _run(Model(d), f, sf, dmy, sd0, si0, 1, False)
    grp = _run(Group(d, devices=_devices(2)), f, sf, dmy, sd0, si0, 1, False)
    _assert_same(one, grp)


def test_cfg5_sequence_restored_into_a_different_shard_count():
    """The cfg5 sequence (bench.cfg5_sequence: hourly raw forcing prefetched and swapped in 6-step chunks from pinned buffers,
    put_data every step, the writer's table every 24 steps) on a 3-shard group, interrupted after day one: its state,
    fluxes and state records restored into a NEW group of 2 shards, which runs day two.  Every output record and the final
    state equal one context running both days without a break."""
    import bench
    from vic_amd.api import Group, Model
    opt = bench.config("cfg5")["opt"]
    nsteps, CH, OUT_EVERY = 48, 6, 24
    d, f, sf, dmy, sd0, si0 = _bench_setup("cfg5", 41, nsteps)

    def fresh(m, sd, si, fx=None, rec=None):
        m.set_state(sd, si)
        if fx is not None:
            m.set_fluxes(fx)
            m.set_state_records(rec)
        m.put_data_config(OUT_EVERY)
        m.put_data_init()
        return m
    a = fresh(Model(d), sd0, si0)
    rec_a = bench.cfg5_sequence(a, f, dmy, 0, nsteps, CH, OUT_EVERY, opt, lambda o: o)
    (sd_a, si_a), rec_state_a = a.get_state(), a.get_state_records()
    a.close()
    g3 = fresh(Group(d, devices=_devices(3)), sd0, si0)
    rec_g = bench.cfg5_sequence(g3, f, dmy, 0, OUT_EVERY, CH, OUT_EVERY, opt, lambda o: o)
    (sd1, si1), fx1, r1 = g3.get_state(), g3.get_fluxes(), g3.get_state_records()
    g3.close()
    g2 = fresh(Group(d, devices=_devices(2)), sd1, si1, fx1, r1)
    rec_g += bench.cfg5_sequence(g2, f, dmy, OUT_EVERY, nsteps - OUT_EVERY, CH, OUT_EVERY, opt, lambda o: o)
    assert len(rec_a) == len(rec_g) == 2
    for k in range(2):
        assert np.array_equal(rec_a[k], rec_g[k], equal_nan=True), "output record %d" % k
    sd_g, si_g = g2.get_state()
    assert np.array_equal(sd_a, sd_g, equal_nan=True) and np.array_equal(si_a, si_g)
    assert np.array_equal(rec_state_a, g2.get_state_records(), equal_nan=True)
    assert g2.get_cell_errors().sum() == 0
    g2.close()


def test_chunked_context_against_unchunked_shards():
    """A FROZEN_SOIL domain of 30k cells: one context splits it into two cell chunks (20k cells or more), the two 15k-cell
    shards of a group run one chunk each.  The chunking must not be visible in any result."""
    from vic_amd.api import Group, Model
    d, f, sf, dmy, sd0, si0 = _bench_setup("cfg3", 30000, 3)
    one = _run(Model(d), f, sf, dmy, sd0, si0, 3, False)
    g = Group(d, devices=_devices(2))
    assert (np.diff(g.shard_bounds()) < 20000).all()
    grp = _run(g, f, sf, dmy, sd0, si0, 3, False)
    _assert_same(one, grp)
