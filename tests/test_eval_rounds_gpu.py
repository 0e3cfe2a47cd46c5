"""How the evaluation rounds of the Tsurf iteration are formed -- dense (lane = HRU of the chunk) or from the flat pending
list (lane = list entry: stripe counters, packed prefix, bisection), in one chunk or two -- must not change a bit, and the
parked context must give every path the words it parked whatever slab word they sit in (the parking map of region A).

The cases (tests/eval_rounds_cases.py) have the options of the bench's cfg3 workload and start from columns frozen to
different depths, so several work-list keys occur and the lanes of a wave leave the iteration in different rounds.  Every
run is teacher-forced from the oracle's free run (computed once per case and shared): with VICGPU_EVAL_LIST_PCT=0 the flat
list is never consumed, so bit-identity of the other thresholds with that run shows that every pending HRU was served exactly
once; the PCT=0 run itself is held to the oracle at the tolerances of tests/test_gpu_parity.py::test_teacher_forced."""
import numpy as np
import pytest

from vic_amd.abi import C
from tests import eval_rounds_cases as ec
from tests.test_gpu_parity import TF_TOL, assert_int_state_equal
from tests.util import worst, FLUX_ROWS_COMMON

pytestmark = pytest.mark.gpu

LAUNCHES = [(pct, chunks) for pct in ("0", "30", "100") for chunks in ("1", "2")]


def _check(monkeypatch, oracle_lib, ncell, variant, solver):
    from vic_amd.api import Model
    case, steps = ec.oracle_run(oracle_lib, ncell, variant, solver)
    Nn = case[0].opt.Nnode
    runs = {}
    for pct, chunks in LAUNCHES:
        monkeypatch.setenv("VICGPU_EVAL_LIST_PCT", pct)
        monkeypatch.setenv("VICGPU_CHUNKS", chunks)
        runs[pct, chunks] = ec.device_run(Model, case, steps)
    base = runs["0", "1"]
    worst_all = 0.0
    for s, (st, (sg, ig, fg, cg, eg)) in enumerate(zip(steps, base)):
        so, io, fo, co, eo = np.array(st[2]), st[3], st[4], st[5], st[6]
        sg = np.array(sg)
        assert eg.sum() == 0 and eo.sum() == 0
        assert np.nanmax(np.abs(so[C["SD_ERROR"]] - sg[C["SD_ERROR"]])) < 1e-3
        so[C["SD_ERROR"]] = 0; sg[C["SD_ERROR"]] = 0
        w1, m1 = worst(so, sg, "SD_", floor=1e-6)
        w2, m2 = worst(fo[FLUX_ROWS_COMMON], fg[FLUX_ROWS_COMMON], "FX_", floor=1e-6)
        w3, m3 = worst(co, cg, "CO_", floor=1e-6)
        print("%d cells %s %s step %d: worst rel diff state %.3e flux %.3e cell %.3e" % (ncell, variant, solver, s, w1, w2, w3))
        assert w1 < TF_TOL, "step %d state %s" % (s, m1)
        assert w2 < TF_TOL, "step %d flux %s" % (s, m2)
        assert w3 < TF_TOL, "step %d cell %s" % (s, m3)
        assert_int_state_equal(io, ig, Nn, "step %d" % s)
        worst_all = max(worst_all, w1, w2, w3)
    for key, run in runs.items():
        for s, (r0, r1) in enumerate(zip(base, run)):
            for name, a, b in zip(("state", "int state", "fluxes", "cell outputs", "cell errors"), r0, r1):
                assert np.array_equal(a, b, equal_nan=True), "PCT %s CHUNKS %s step %d: %s differ from the dense run" % (key + (s, name))
    return steps


@pytest.mark.parametrize("solver", ["brent", "newton"])
@pytest.mark.parametrize("ncell", ec.SIZES)
def test_rounds_are_invisible(monkeypatch, oracle_lib, ncell, solver):
    """1 cell (fewer HRUs than a wave), 67 cells (ragged last wave), 200 cells (79 waves on 64 stripes), 6 steps, both node
    solvers; thresholds 0 / 30 / 100 % x 1 / 2 chunks."""
    steps = _check(monkeypatch, oracle_lib, ncell, "plain", solver)
    # the start is what the case promises: several work-list keys (frozen-node counts) among the HRUs of the first step
    from vic_amd import abi
    Nn = 10
    T = np.array([steps[0][0][abi.sd_node(C["SDN_T"], n, Nn)] for n in range(1, Nn)])
    assert len(np.unique((T < 0).sum(axis=0))) >= 5


def test_quick_solve_rounds(monkeypatch, oracle_lib):
    """QUICK_SOLVE: the iteration on the shortened column and its restart on the whole one go through the same rounds."""
    _check(monkeypatch, oracle_lib, 67, "quick_solve", "brent")


def test_thin_snow_rounds(monkeypatch, oracle_lib):
    """A snowpack below the energy-balance threshold is solved together with the ground surface (INCLUDE_SNOW): the [incl]
    group and the [feed] words, carried from one evaluation to the next, go through the parking map."""
    steps = _check(monkeypatch, oracle_lib, 67, "thin_snow", "brent")
    swq = steps[0][0][C["SD_SNOW_SWQ"]]
    assert ((swq > 0) & (swq < 1e-3)).sum() > 100
