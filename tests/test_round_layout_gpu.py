"""Every reader and writer of the two tables the rounds exchange -- item blocks and solution records, vic_layout.hpp --
against the oracle, on domains of 65 cells: one full wave plus one lane per (tile, band) slot, so every kernel runs a full
and a ragged wave and the tables' last entries are in use.

The cases are those whose kernels index the tables differently: the register-resident 10-node kernel without and with
NOFLUX (the bottom node's record, last in the block), the generic kernel at 5 and 24 nodes (start column in LDS), the deep
bound at 50 nodes (start column read from the block at every visit), QUICK_SOLVE (both records' keys invalidated when the
iteration moves to the whole column) and IMPLICIT (record written by the implicit kernel, counters copied from the last
explicit solve's record).  Scenario options, start days and tolerances are those of tests/scenarios.py, tests/test_deep_nodes_gpu.py
and tests/test_gpu_parity.py (IMPLICIT: its envelope measure); teacher-forced, integer state exact in every case.
"""
import numpy as np
import pytest

from vic_amd.abi import C
from tests import scenarios
from tests import test_deep_nodes_gpu as tdn
from tests import test_gpu_parity as gp
from tests.util import FLUX_ROWS_COMMON, worst

pytestmark = pytest.mark.gpu

NCELL = 65
NSTEPS = 12


def _spec(name):
    sp = scenarios.OPTION_BRANCHES.get(name) or scenarios.IMPLICIT_BRANCHES.get(name) or scenarios.QUICK_SOLVE_BRANCHES[name]
    return sp["kw"], sp["ntile"], sp["doy"]


# name -> (options, tiles, start day of year)
CASES = {
    "n10": gp.CASES["frozen_fixed"][0:1] + gp.CASES["frozen_fixed"][2:4],
    "n10_noflux": _spec("frozen_noflux"),
    "n5": _spec("frozen_n5"),
    "n24": _spec("frozen_n24"),
    "n50": tdn.DEEP_CASES["deep_n50"][0:1] + tdn.DEEP_CASES["deep_n50"][2:4],
    "quick_solve": _spec("quick_solve"),
    "implicit_n10": _spec("implicit"),
}


def _teacher_forced(name, solver, oracle_lib):
    from vic_amd.api import Model
    kw, ntile, doy = CASES[name]
    kw = dict(kw, NODE_SOLVER=gp.SOLVERS[solver])
    d, f, sf, dmy, sd0, si0 = gp._setup(kw, NCELL, ntile, NSTEPS, doy)
    implicit = bool(d.opt.IMPLICIT)
    tol, floor = (gp.IMPLICIT_TOL, gp.IMPLICIT_FLOOR) if implicit else (gp.TF_TOL, 1e-6)
    orc = gp._oracle_for(oracle_lib, d, solver)
    orc.set_state(sd0, si0)
    gpu = Model(d)
    gpu.push_forcing(f, sf, dmy)
    worst_all = 0.0
    probe = gp._oracle_for(oracle_lib, d, solver) if implicit else None
    for s in range(NSTEPS):
        sd_in, si_in = orc.get_state()
        fx_in = orc.get_fluxes() if probe else None
        fo, co, eo = orc.step(f[s], sf[s], dmy[s])
        so, io = orc.get_state()
        gpu.set_state(sd_in, si_in)
        gpu.dist_prec(s, 1)
        sg, ig = gpu.get_state()
        fg, cg = gpu.get_fluxes(), gpu.get_cell_outputs()
        assert gpu.get_cell_errors().sum() == 0 and eo.sum() == 0
        so[C["SD_ERROR"]] = 0; sg[C["SD_ERROR"]] = 0
        if probe:
            # IMPLICIT, as tests/test_gpu_parity.py::test_teacher_forced_option_branches measures it: the distance to the envelope of
            # the oracle's own answers when its inputs move by a few ulp (the reference's Newton iteration sits on convergence /
            # failure edges, where a flat bound on the distance to one answer fails: measured here 1.4e-3 at step 3, newton)
            T0, Nn = C["SD_NSCALAR"], d.opt.Nnode
            env, env_f, env_c = [so.copy()], [fo.copy()], [co.copy()]
            for eps in (1e-15, -1e-15, 3e-15):
                sdp = sd_in.copy()
                sdp[T0:T0 + Nn] *= (1 + eps); sdp[C["SD_MOIST0"]:C["SD_MOIST0"] + 3] *= (1 + eps)
                probe.set_state(sdp, si_in); probe.set_fluxes(fx_in)
                fp, cp, _ = probe.step(f[s], sf[s], dmy[s])
                sp_ = probe.get_state()[0]
                sp_[C["SD_ERROR"]] = 0
                env.append(sp_); env_f.append(fp); env_c.append(cp)

            def nearest(got, lo, hi):
                return np.where((got >= lo) & (got <= hi), got, np.where(got < lo, lo, hi))
            so = nearest(sg, np.minimum.reduce(env), np.maximum.reduce(env))
            fo = np.where(np.isnan(fo), fo, nearest(fg, np.fmin.reduce(env_f), np.fmax.reduce(env_f)))
            co = nearest(cg, np.fmin.reduce(env_c), np.fmax.reduce(env_c))
        w1, m1 = worst(so, sg, "SD_", floor=floor)
        w2, m2 = worst(fo[FLUX_ROWS_COMMON], fg[FLUX_ROWS_COMMON], "FX_", floor=floor)
        w3, m3 = worst(co, cg, "CO_", floor=floor)
        print(name, solver, "step %d worst rel diff state %.3e flux %.3e cell %.3e, int entries differing %d" % (
            s, w1, w2, w3, int((io != ig).sum())))
        assert w1 < tol, "step %d state %s" % (s, m1)
        assert w2 < tol, "step %d flux %s" % (s, m2)
        assert w3 < tol, "step %d cell %s" % (s, m3)
        gp.assert_int_state_equal(io, ig, d.opt.Nnode, "step %d" % s)
        worst_all = max(worst_all, w1, w2, w3)
    print(name, solver, "teacher-forced worst rel diff %.3e" % worst_all)


@pytest.mark.parametrize("solver", list(gp.SOLVERS))
@pytest.mark.parametrize("name", list(CASES))
def test_round_tables_against_oracle(name, solver, oracle_lib):
    _teacher_forced(name, solver, oracle_lib)


def test_round_tables_run_twice_bit_identical():
    """The 10-node case free-running, twice from the same state on the same context: the records and keys the first run
    left in the tables must not reach the second one."""
    from vic_amd.api import Model
    kw, ntile, doy = CASES["n10"]
    d, f, sf, dmy, sd0, si0 = gp._setup(kw, NCELL, ntile, NSTEPS, doy)
    gpu = Model(d)
    gpu.push_forcing(f, sf, dmy)
    runs = []
    for rep in range(2):
        gpu.set_state(sd0, si0)
        gpu.reset_accum()
        gpu.dist_prec(0, NSTEPS)
        runs.append((*gpu.get_state(), gpu.get_fluxes(), gpu.get_accum()))
    assert gpu.get_cell_errors().sum() == 0
    for a, b in zip(*runs):
        assert np.array_equal(a, b, equal_nan=True)
