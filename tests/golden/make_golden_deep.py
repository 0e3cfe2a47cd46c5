"""Generates the deep-column reference fixtures (more than 24 thermal nodes) with make_golden.py's trajectory writer:
same format, picked up by tests/test_oracle.py::test_oracle_reproduces_golden and
tests/test_gpu_parity.py::test_gpu_against_reference_goldens like the others.

    python tests/golden/make_golden_deep.py [name ...]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden  # noqa: E402

DEEP_SCENARIOS = {
    # name: (option kwargs, variant, ncell, ntile, glacier, nsteps, start_doy, stride) as in make_golden.SCENARIOS
    "frozen_deep_n50": (dict(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=50, frozen_compat=0), "fixed", 4, 2, False, 48, 330, 6),
    # EXP_TRANS: exponential node grid.  At 36 nodes numpy's exp() gives the reference's node depths bit for bit (the
    # generator asserts it); at some other counts (18) the last bit differs
    "frozen_deep_exp_trans_n36": (dict(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=36, EXP_TRANS=1, frozen_compat=0), "fixed", 4, 2, False, 48, 20, 6),
    "frozen_deep_n33_thaw": (dict(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=33, frozen_compat=0), "fixed", 4, 3, False, 48, 95, 6),
}


if __name__ == "__main__":
    make_golden.SCENARIOS = DEEP_SCENARIOS
    sys.argv = sys.argv[:1] + (sys.argv[1:] or list(DEEP_SCENARIOS))
    make_golden.main()
