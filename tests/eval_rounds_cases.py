"""Domains for the evaluation-round tests (tests/test_eval_rounds_gpu.py, tools/hostemu/check_eval_rounds.py): the options of
the bench's cfg3 workload -- FULL_ENERGY + FROZEN_SOIL (fixed), 10 thermal nodes, 5 snow bands x 5 vegetation tiles, hourly
steps -- on a few cells, started from columns that are frozen to different depths, so that the work list has several keys
and the Tsurf iterations of a wave end in different rounds.

Sizes: 1 cell (25 HRUs, less than a wave), 67 cells (1675 HRUs: a ragged last wave), 200 cells (5000 HRUs: 79 waves, more
than the pending list has stripes, so stripes hold several chunks).

Variants: "plain"; "quick_solve" (QUICK_SOLVE: the shortened column and the restart of the iteration); "thin_snow" (a snowpack
below the energy-balance threshold on a third of the HRUs: the pack is solved together with the ground surface, INCLUDE_SNOW,
so the [incl] group and the [feed] words of the parked context are in use)."""
import functools

import numpy as np

from vic_amd import abi, domain, init_state
from vic_amd.abi import C

SIZES = (1, 67, 200)
NSTEPS = 6
NTILE = 5
START_DOY = 60


def options(variant="plain", **more):
    kw = dict(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=10, Nband=5, frozen_compat=0)
    if variant == "quick_solve":
        kw["QUICK_SOLVE"] = 1
    kw.update(more)
    return kw


def mixed_start(sd, Nn):
    """Frozen from the top down to a depth that differs from HRU to HRU (0 .. Nn - 2 nodes), with a temperature gradient (a
    column at one temperature makes the cold-nose test compare rounding noise, tests/deep_scenarios.py); every fifth HRU has
    the node below the front just above 0 C, inside the node solver's first bracket."""
    nh = sd.shape[1]
    g = np.arange(nh)
    k = (7 * g + g // 64) % (Nn - 1)
    for n in range(1, Nn - 1):                   # the bottom node is the boundary condition
        T = np.where(n <= k, -1.2 - 0.05 * n, 1.2 + 0.05 * n)
        T = np.where((g % 5 == 0) & (n == k + 1), 0.2, T)
        sd[abi.sd_node(C["SDN_T"], n, Nn)] = T
    return sd


def thin_snow(sd, si):
    """0.6 mm of snow water on every third HRU: below MIN_SWQ_EB_THRES the pack has no energy balance of its own."""
    nh = sd.shape[1]
    m = np.arange(nh) % 3 == 0
    swq, density = 0.0006, 250.0
    sd[C["SD_SNOW_SWQ"], m] = swq
    sd[C["SD_SNOW_DENSITY"], m] = density
    sd[C["SD_SNOW_DEPTH"], m] = swq * 1000.0 / density
    sd[C["SD_SNOW_COVERAGE"], m] = 1.0
    sd[C["SD_SNOW_SURF_TEMP"], m] = -3.0
    sd[C["SD_SNOW_PACK_TEMP"], m] = -3.0
    sd[C["SD_SNOW_SURF_WATER"], m] = 0.0
    sd[C["SD_SNOW_PACK_WATER"], m] = 0.0
    sd[C["SD_SNOW_COLDCONTENT"], m] = 2100.0 * swq * 1000.0 * -3.0      # CH_ICE * swq * Tsurf
    sd[C["SD_SNOW_ALBEDO"], m] = 0.85
    si[C["SI_SNOW_SNOW"], m] = 0
    si[C["SI_SNOW_LAST_SNOW"], m] = 1
    si[C["SI_SNOW_MELTING"], m] = 0
    return sd, si


def build(ncell, variant="plain", nsteps=NSTEPS, **more):
    """(d, f, sf, dmy, sd0, si0) of a case; `more` = further options (NODE_SOLVER)."""
    opt = abi.default_options(**options(variant, **more))
    d = domain.make_domain(ncell, opt, ntile=NTILE)
    f, sf, dmy = domain.make_forcing(d, 0, nsteps, start_doy=START_DOY)
    sd0, si0 = init_state.initial_state(d, f[0])
    mixed_start(sd0, opt.Nnode)
    if variant == "thin_snow":
        thin_snow(sd0, si0)
    return d, f, sf, dmy, sd0, si0


@functools.lru_cache(maxsize=None)
def oracle_run(pyref, ncell, variant, solver, nsteps=NSTEPS):
    """The oracle's free run of a case, computed once per process: per step (state in, state out, fluxes, cell outputs,
    cell errors).  Read-only for the callers."""
    d, f, sf, dmy, sd0, si0 = build(ncell, variant, nsteps, NODE_SOLVER=C["VIC_NODE_SOLVER_" + solver.upper()])
    orc = pyref.OracleModel(d, converged_nodes=(solver == "newton"))
    orc.set_state(sd0, si0)
    steps = []
    for s in range(nsteps):
        sd_in, si_in = orc.get_state()
        fo, co, eo = orc.step(f[s], sf[s], dmy[s])
        so, io = orc.get_state()
        steps.append(tuple(np.array(a) for a in (sd_in, si_in, so, io, fo, co, eo)))
    for st in steps:
        for a in st:
            a.setflags(write=False)
    return (d, f, sf, dmy), steps


def device_run(Model, case, steps):
    """Teacher-forced device steps from the oracle's states: per step (state, int state, fluxes, cell outputs, cell errors)."""
    d, f, sf, dmy = case
    m = Model(d)
    m.push_forcing(f, sf, dmy)
    out = []
    for s, st in enumerate(steps):
        m.set_state(np.array(st[0]), np.array(st[1]))
        m.dist_prec(s, 1)
        sg, ig = m.get_state()
        out.append((sg, ig, m.get_fluxes(), m.get_cell_outputs(), m.get_cell_errors()))
    m.close()
    return out
