"""More than 24 thermal nodes on the device (the <50> instantiations: vic_fd_stage, vic_profile_solve_lockstep,
vic_hru_step<50, true>, vic_put_sum_deep) against the oracle, with the checks and tolerances of the existing suites run on
deep columns: teacher-forced and free-running (tests/test_gpu_parity.py), put_data (tests/test_putdata.py), state records
(tests/test_state_records.py), a two-shard group (tests/test_group_gpu.py); and IMPLICIT above 24 nodes refused."""
import numpy as np
import pytest

from vic_amd import abi, domain, init_state
from vic_amd.abi import C
from tests import deep_scenarios
from tests import test_gpu_parity as gp
from tests import test_group_gpu as gg
from tests import test_putdata as tpd
from tests import test_state_records as tsr
from tests.util import worst

pytestmark = pytest.mark.gpu

FROZEN = dict(FULL_ENERGY=1, FROZEN_SOIL=1, frozen_compat=0)
# name -> (options, ncell, ntile, start doy) in the format of tests/test_gpu_parity.py CASES
DEEP_CASES = {
    "deep_n25": (dict(FROZEN, Nnode=25), 32, 2, 330),
    "deep_n33": (dict(FROZEN, Nnode=33), 32, 2, 20),
    "deep_n50": (dict(FROZEN, Nnode=50), 32, 2, 330),
    "deep_n50_spring": (dict(FROZEN, Nnode=50), 32, 2, 95),
}
SOLVER_NAMES = ["brent", "newton"]


@pytest.mark.parametrize("solver", SOLVER_NAMES)
@pytest.mark.parametrize("name", list(DEEP_CASES))
def test_teacher_forced_deep(name, solver, oracle_lib, monkeypatch):
    monkeypatch.setitem(gp.CASES, name, DEEP_CASES[name])
    gp.test_teacher_forced(name, solver, oracle_lib)


class _ConvergedNodeOracle:
    """The oracle with its node root finds converged (tests/test_gpu_parity.py, "newton"): the judge of the Newton node
    solver over a free run.  Over 240 free-running steps of a deep column, the reference Brent's own stopping noise in
    the node temperatures (up to ~1e-7 K at every frozen node) moves near-zero accumulated evaporation of a few cells by
    more than 1e-5 relative against the Newton trajectory (measured 2.8e-4 at 25 nodes, 2.0e-5 at 33), which is a
    property of the reference's tolerance, not of the device; the Brent solver is held to the unmodified oracle."""
    def __init__(self, lib):
        self.lib = lib

    def OracleModel(self, d):
        return self.lib.OracleModel(d, converged_nodes=True)


@pytest.mark.parametrize("solver", SOLVER_NAMES)
@pytest.mark.parametrize("name", list(DEEP_CASES))
def test_free_running_deep(name, solver, oracle_lib, monkeypatch):
    monkeypatch.setitem(gp.CASES, name, DEEP_CASES[name])
    gp.test_free_running(name, solver, _ConvergedNodeOracle(oracle_lib) if solver == "newton" else oracle_lib)


@pytest.mark.parametrize("solver", SOLVER_NAMES)
@pytest.mark.parametrize("name", [n for n, sp in deep_scenarios.DEEP_BRANCHES.items() if not sp.get("start")])
def test_teacher_forced_deep_branches(name, solver, oracle_lib, monkeypatch):
    """The deep option branches of tests/deep_scenarios.py (each pinned oracle-vs-reference in tests/test_deep_nodes.py)
    through the option-branch check of tests/test_gpu_parity.py."""
    monkeypatch.setattr(gp.scenarios, "build", deep_scenarios.build)
    gp.test_teacher_forced_option_branches(name, solver, oracle_lib)


@pytest.mark.parametrize("solver", SOLVER_NAMES)
@pytest.mark.parametrize("name", ["deep_spikes_n50", "deep_spikes_n40"])
def test_deep_node_fallback_flags(name, solver, oracle_lib):
    """Fall-back flags at node index 32 and above, from the profile kernel's record through vic_fd_stage / surf_post into
    SI T_fbflag / T_fbcount: a frozen column with cold spikes deep in it (tests/deep_scenarios.py; the same start pinned
    against the reference in tests/test_deep_nodes.py), teacher-forced, integer state identical at every step."""
    from vic_amd.api import Model
    sp, d, f, sf, dmy = deep_scenarios.build(name)
    d.opt.NODE_SOLVER = gp.SOLVERS[solver]
    Nn = d.opt.Nnode
    sd0, si0 = init_state.initial_state(d, f[0])
    deep_scenarios.start_state(sp, sd0)
    orc = gp._oracle_for(oracle_lib, d, solver)
    orc.set_state(sd0, si0)
    gpu = Model(d)
    gpu.push_forcing(f, sf, dmy)
    flagged = set()
    for s in range(f.shape[0]):
        sd_in, si_in = orc.get_state()
        orc.step(f[s], sf[s], dmy[s])
        so, io = orc.get_state()
        gpu.set_state(sd_in, si_in)
        gpu.dist_prec(s, 1)
        sg, ig = gpu.get_state()
        assert gpu.get_cell_errors().sum() == 0
        so[C["SD_ERROR"]] = 0; sg[C["SD_ERROR"]] = 0
        w, msg = worst(so, sg, "SD_", floor=1e-6)
        assert w < gp.TF_TOL, "step %d state %s" % (s, msg)
        gp.assert_int_state_equal(io, ig, Nn, "step %d" % s)
        fb = np.array([ig[abi.si_node(C["SIN_T_FBFLAG"], n, Nn)] for n in range(Nn)])
        flagged |= set(int(n) for n in np.flatnonzero(fb.sum(axis=1)))
    assert {n for n in deep_scenarios.SPIKE_NODES if n < Nn - 1} <= flagged, sorted(flagged)
    if Nn == 50:
        assert set(range(32, Nn)) <= flagged, sorted(flagged)     # the non-convergence fall-back: the whole column


PUT_CASES = [
    # tests/test_putdata.py GPU_CASES format: OUT_SOIL_TNODE / OUT_SOILT_FBFLAG have Nnode = 50 elements
    ("deep_n50", dict(FROZEN, Nnode=50, Nband=2), 12, 3, False, 24, 330, 6, "brent"),
    ("deep_n50_newton_glacier", dict(FROZEN, Nnode=50, Nband=2), 12, 2, True, 24, 20, 4, "newton"),
]


@pytest.mark.parametrize("case", PUT_CASES, ids=[c[0] for c in PUT_CASES])
def test_device_put_data_deep(case, oracle_lib):
    tpd.test_device_put_data_against_oracle(case, oracle_lib)


@pytest.mark.parametrize("case", [("deep_n50", dict(FROZEN, Nnode=50, Nband=2), 12, 2, False, 12, 330),
                                  ("deep_n50_glacier", dict(FROZEN, Nnode=50, Nband=2), 12, 2, True, 12, 20)], ids=["plain", "glacier"])
def test_device_state_records_deep(case, oracle_lib):
    """Save, restore and continue at Nnode = 50; interrupted == uninterrupted bit for bit."""
    tsr.test_device_state_records(case, oracle_lib)


def test_group_two_shards_deep():
    """A two-shard vicgpu_group equals one context at 50 nodes: state, fluxes, records, put_data outputs, bit for bit."""
    from vic_amd.api import Group, Model
    opt = abi.default_options(**dict(FROZEN, Nnode=50, Nband=2))
    d = domain.make_domain(41, opt, ntile=2, glacier_top_band=True)
    f, sf, dmy = domain.make_forcing(d, 0, 12, start_doy=330)
    sd0, si0 = init_state.initial_state(d, f[0])
    sd0[C["SD_GLAC_CUM_MASS_BALANCE"], d.hru_iparams[C["HPI_IS_GLACIER"]] != 0] = 0.0
    one = gg._run(Model(d), f, sf, dmy, sd0, si0, 6, True)
    grp = gg._run(Group(d, devices=gg._devices(2)), f, sf, dmy, sd0, si0, 6, True)
    gg._assert_same(one, grp)
    assert one["errors"].sum() == 0


@pytest.mark.parametrize("nnode,accepted", [(24, True), (25, False), (50, False)])
def test_implicit_above_24_nodes_refused(nnode, accepted):
    from vic_amd.api import Model, VicGpuError
    opt = abi.default_options(**dict(FROZEN, Nnode=nnode, IMPLICIT=1))
    d = domain.make_domain(8, opt, ntile=2)
    if accepted:
        Model(d).close()
        return
    with pytest.raises(VicGpuError) as e:
        Model(d)
    assert "code %d " % C["VICGPU_ERR_UNSUPPORTED"] in str(e.value)
