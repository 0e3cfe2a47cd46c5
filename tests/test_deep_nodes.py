"""More than 24 thermal nodes (up to the reference's MAX_NODES = 50), on the CPU: the oracle against the real reference
side by side, bit for bit, over the deep-column scenarios of tests/deep_scenarios.py (node counts 25 / 32 / 33 / 50 and the
option branches of the profile solve at the deep bound).  The device side is tests/test_deep_nodes_gpu.py."""
import numpy as np
import pytest

from vic_amd import abi
from vic_amd.abi import C
from tests import deep_scenarios
from tests.util import rel_diff, worst


def test_header_node_bound():
    """The C ABI admits the reference's MAX_NODES (user_def.h:96)."""
    assert abi.VIC_MAX_NODES == 50


@pytest.mark.parametrize("name", list(deep_scenarios.DEEP_BRANCHES))
def test_oracle_vs_reference_deep_columns(name, oracle_lib, ref_available):
    if not ref_available:
        pytest.skip("reference build (oracle/_ref) not available")
    sp, d, f, sf, dmy = deep_scenarios.build(name)
    Nn = sp["kw"]["Nnode"]
    ref = oracle_lib.RefModel(d, sp["variant"])
    ref.init_state(f[0], dmy[0], d.init_moist)
    sd0, si0 = ref.get_state()
    if sp.get("glacier"):
        isg = d.hru_iparams[C["HPI_IS_GLACIER"]] != 0
        sd0[C["SD_GLAC_CUM_MASS_BALANCE"], isg] = 0.0
    deep_scenarios.start_state(sp, sd0)
    ref.set_state(sd0, si0)
    d.cell_params[...] = ref.get_cell_params()
    orc = oracle_lib.OracleModel(d)
    orc.set_state(sd0, si0)
    orc.set_fluxes(ref.get_fluxes())
    rows = [r for r in range(C["FX_NROW"]) if r not in (C["FX_OUT_PREC"], C["FX_OUT_RAIN"], C["FX_OUT_SNOW"])]
    deep_frozen, deep_flagged = 0, set()
    for s in range(f.shape[0]):
        fr, cr, er = ref.step(f[s], sf[s], dmy[s])
        fo, co, eo = orc.step(f[s], sf[s], dmy[s])
        sr, ir = ref.get_state()
        so, io = orc.get_state()
        assert np.array_equal(er != 0, eo != 0), "step %d error cells %s vs %s" % (s, np.flatnonzero(er), np.flatnonzero(eo))
        assert er.sum() == 0, "step %d" % s
        assert rel_diff(sr, so, 1e-12).max() == 0.0, "step %d %s" % (s, worst(sr, so, "SD_", 1e-12)[1])
        assert rel_diff(fr[rows], fo[rows], 1e-12).max() == 0.0, "step %d %s" % (s, worst(fr[rows], fo[rows], "FX_", 1e-12)[1])
        assert rel_diff(cr, co, 1e-12).max() == 0.0
        assert np.array_equal(ir, io), "step %d int state %s" % (s, np.argwhere(ir != io)[:4])
        T = np.array([so[abi.sd_node(C["SDN_T"], n, Nn)] for n in range(Nn)])
        deep_frozen = max(deep_frozen, int((T[24:] < 0).sum(axis=0).max()))
        fb = np.array([io[abi.si_node(C["SIN_T_FBFLAG"], n, Nn)] for n in range(Nn)])
        deep_flagged |= set(np.flatnonzero(fb.sum(axis=1)).tolist())
    ref.close()
    if sp.get("start") == "cold_spikes":
        # the reference itself flags nodes at index 32 and above: the 64-bit fall-back mask carries them on the device
        assert {n for n in deep_scenarios.SPIKE_NODES if n < Nn - 1} <= deep_flagged, sorted(deep_flagged)
    if sp["doy"] in (330, 10, 20):
        assert deep_frozen > 0, "no node below the 24th froze: the deep part of the column was not exercised"
