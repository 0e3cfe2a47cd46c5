"""Teacher-forced steps of deep-column scenarios (tests/deep_scenarios.py, start state included) through the sanitizer
build of the device code, against the oracle -- check.py for more than 24 thermal nodes.  Besides the worst relative
difference it reports what the steps reached: the fewest frozen nodes any HRU started a step with (25 or more: the
clamped top work-list segment) and the nodes at index 32 or above the device flagged (the 64-bit fall-back mask).
Run by tests/test_deep_nodes_hostemu.py:
    python tools/hostemu/check_deep.py <nsteps> <case> [<case> ...]"""
import os, sys
import numpy as np
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from tests import deep_scenarios
from tests.util import worst
from vic_amd import abi, init_state
from vic_amd.abi import C
from vic_amd.api import Model
from oracle import pyref


def main():
    nsteps = int(sys.argv[1])
    rc = 0
    for name in sys.argv[2:]:
        sp, d, f, sf, dmy = deep_scenarios.build(name, nsteps=nsteps)
        Nn = d.opt.Nnode
        sd0, si0 = init_state.initial_state(d, f[0])
        deep_scenarios.start_state(sp, sd0)
        orc = pyref.OracleModel(d, converged_nodes=os.environ.get("VICGPU_NODE_SOLVER") == "newton"); orc.set_state(sd0, si0)
        dev = Model(d); dev.push_forcing(f, sf, dmy)
        w_all, min_frozen, flagged = 0.0, Nn, set()
        for s in range(nsteps):
            sd_in, si_in = orc.get_state()
            T = np.array([sd_in[abi.sd_node(C["SDN_T"], n, Nn)] for n in range(1, Nn)])
            min_frozen = min(min_frozen, int((T < 0).sum(axis=0).min()))
            orc.step(f[s], sf[s], dmy[s])
            so, io = orc.get_state()
            dev.set_state(sd_in, si_in); dev.dist_prec(s, 1)
            sg, ig = dev.get_state()
            so[C["SD_ERROR"]] = 0; sg[C["SD_ERROR"]] = 0
            w1, m1 = worst(so, sg, "SD_", floor=1e-6)
            w_all = max(w_all, w1)
            if not np.array_equal(io, ig): w_all = max(w_all, 1.0)
            fb = np.array([ig[abi.si_node(C["SIN_T_FBFLAG"], n, Nn)] for n in range(Nn)])
            flagged |= set(int(n) for n in np.flatnonzero(fb.sum(axis=1)) if n >= 32)
        print("hostemu %s: worst rel diff %.3e; min frozen nodes at a step start %d; flagged nodes >= 32: %s"
              % (name, w_all, min_frozen, sorted(flagged)), flush=True)
        if not w_all < 1e-6: rc = 1
    return rc


if __name__ == "__main__":
    sys.exit(main())
