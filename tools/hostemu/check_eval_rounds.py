"""Teacher-forced steps of the evaluation-round cases (tests/eval_rounds_cases.py) through the sanitizer build of the device
code, against the oracle, once per sparse-round threshold: with VICGPU_EVAL_LIST_PCT=0 every evaluation round is dense, with
100 every round after the first is formed from the flat pending list (stripe counters, packed prefix, bisection).  The two
runs must also agree bit for bit.  Run by tests/test_eval_rounds_hostemu.py:
    python tools/hostemu/check_eval_rounds.py <nsteps> <ncell>[:<variant>] [...]"""
import os, sys
import numpy as np
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from tests import eval_rounds_cases as ec
from tests.util import worst
from vic_amd.abi import C
from vic_amd.api import Model
from oracle import pyref


def main():
    nsteps = int(sys.argv[1])
    solver = os.environ.get("VICGPU_NODE_SOLVER", "brent")
    rc = 0
    for spec in sys.argv[2:]:
        ncell, _, variant = spec.partition(":")
        variant = variant or "plain"
        case, steps = ec.oracle_run(pyref, int(ncell), variant, solver, nsteps)
        runs = {}
        for pct in ("0", "100"):
            os.environ["VICGPU_EVAL_LIST_PCT"] = pct
            runs[pct] = ec.device_run(Model, case, steps)
            w_all = 0.0
            for st, (sg, ig, fg, cg, eg) in zip(steps, runs[pct]):
                so, io, co = np.array(st[2]), st[3], st[5]
                sg = np.array(sg)
                so[C["SD_ERROR"]] = 0; sg[C["SD_ERROR"]] = 0
                w1, m1 = worst(so, sg, "SD_", floor=1e-6)
                w3, m3 = worst(co, cg, "CO_", floor=1e-6)
                w_all = max(w_all, w1, w3)
                if not np.array_equal(io, ig) or eg.sum() != 0: w_all = max(w_all, 1.0)
            print("hostemu eval rounds %s pct %s: worst rel diff %.3e" % (spec, pct, w_all), flush=True)
            if not w_all < 1e-6: rc = 1
        same = all(np.array_equal(a, b, equal_nan=True) for r0, r1 in zip(runs["0"], runs["100"]) for a, b in zip(r0, r1))
        print("hostemu eval rounds %s: pct 0 and 100 %s" % (spec, "bit-identical" if same else "DIFFER"), flush=True)
        if not same: rc = 1
    return rc


if __name__ == "__main__":
    sys.exit(main())
