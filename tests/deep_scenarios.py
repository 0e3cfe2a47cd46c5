"""Scenarios with more than 24 thermal nodes (the deep node bound, up to the reference's MAX_NODES = 50), shared by the
oracle-vs-reference tests (tests/test_deep_nodes.py), the sanitizer run of the device code (tools/hostemu/check_deep.py)
and the GPU parity tests (tests/test_deep_nodes_gpu.py).  Same format as tests/scenarios.py, built by its build(); one
addition: start = optional name of a start-state modifier (start_state below), applied to the state after initialisation."""
from unittest import mock

from vic_amd import abi
from vic_amd.abi import C
from tests import scenarios

FROZEN = dict(FULL_ENERGY=1, FROZEN_SOIL=1, frozen_compat=0)

DEEP_BRANCHES = {
    # node counts across the deep bound: 25 (first deep count), 32 / 33 (either side of a 32-bit mask), 50 (MAX_NODES)
    "deep_n25": dict(kw=dict(FROZEN, Nnode=25), variant="fixed", ncell=4, ntile=2, nsteps=60, doy=330),
    "deep_n32": dict(kw=dict(FROZEN, Nnode=32), variant="fixed", ncell=4, ntile=2, nsteps=60, doy=20),
    "deep_n33": dict(kw=dict(FROZEN, Nnode=33), variant="fixed", ncell=4, ntile=2, nsteps=60, doy=95),
    "deep_n50": dict(kw=dict(FROZEN, Nnode=50), variant="fixed", ncell=4, ntile=2, nsteps=60, doy=330),
    # the run-time branches of the profile solve at the deep bound
    "deep_exp_trans_n40": dict(kw=dict(FROZEN, Nnode=40, EXP_TRANS=1), variant="fixed", ncell=4, ntile=2, nsteps=60, doy=330),
    "deep_noflux_n33": dict(kw=dict(FROZEN, Nnode=33, NOFLUX=1), variant="fixed", ncell=4, ntile=2, nsteps=60, doy=10),
    "deep_quick_solve_n50": dict(kw=dict(FROZEN, Nnode=50, QUICK_SOLVE=1), variant="fixed", ncell=4, ntile=3, nsteps=60, doy=95),
    "deep_glacier_n36": dict(kw=dict(FROZEN, Nnode=36, Nband=2), variant="fixed", ncell=4, ntile=2, glacier=True, nsteps=60, doy=20),
    "deep_tfallback0_n50": dict(kw=dict(FROZEN, Nnode=50, TFALLBACK=0), variant="fixed", ncell=4, ntile=2, nsteps=50, doy=330),
    # stress forcing with TFALLBACK: the surface-temperature root find fails and falls back
    "deep_stress_n50": dict(kw=dict(FROZEN, Nnode=50, TFALLBACK=1), variant="fixed", ncell=6, ntile=2, nsteps=40, doy=330, tweak="stress"),
    "deep_wide_soils_n45": dict(kw=dict(FROZEN, Nnode=45), variant="fixed", ncell=6, ntile=2, nsteps=60, doy=330, soils="wide"),
    # node fall-backs deep in the column: a frozen column with cold spikes at nodes 34, 41 and 47 (start_state).  The
    # reference's node root finds fail there in the first step (no root within T0 +- 50.25 K: those nodes are flagged), and
    # from the second step the Gauss-Seidel iteration no longer converges, which flags every node of the column
    # (frozen_soil.c:486-493); every HRU starts with 48-49 frozen nodes (the top work-list segment of the deep bound)
    "deep_spikes_n50": dict(kw=dict(FROZEN, Nnode=50, TFALLBACK=1), variant="fixed", ncell=4, ntile=2, nsteps=12, doy=330,
                            start="cold_spikes"),
    "deep_spikes_n40": dict(kw=dict(FROZEN, Nnode=40, TFALLBACK=1), variant="fixed", ncell=4, ntile=2, nsteps=12, doy=20,
                            start="cold_spikes"),
}

SPIKE_NODES = (34, 41, 47)


_build = scenarios.build      # (taken at import: a test may substitute scenarios.build by this module's build)


def build(name, nsteps=None):
    """Domain + forcing of a scenario: returns (spec, d, f, sf, dmy) -- tests/scenarios.py's build with the spec lent to it."""
    sp = DEEP_BRANCHES[name]
    with mock.patch.dict(scenarios.RANDOM_COMBINATIONS, {name: sp}):
        return _build(name, nsteps)


def start_state(sp, sd):
    """Applies the scenario's start-state modifier to the double state table sd (in place).

    cold_spikes: the column cools with depth (-2 C - 0.037 K per node) and nodes 34 / 41 / 47 start at -120 C - n.  The
    gradient matters: a column at ONE temperature makes neighbouring start temperatures equal, and the cold-nose test
    (frozen_soil.c:470-484) then compares differences that are zero up to rounding -- its flags change when the state moves
    by 1e-12, so no two implementations (not even the oracle with converged node roots) would agree on them."""
    if sp.get("start") == "cold_spikes":
        Nn = sp["kw"]["Nnode"]
        for n in range(1, Nn - 1):                   # the bottom node is the boundary condition (dp, avg_temp)
            sd[abi.sd_node(C["SDN_T"], n, Nn)] = -2.0 - 0.037 * n
        for n in SPIKE_NODES:
            if n < Nn - 1:
                sd[abi.sd_node(C["SDN_T"], n, Nn)] = -120.0 - n
    return sd
