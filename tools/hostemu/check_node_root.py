"""The frozen-node root battery (tests/node_cases.py) through the sanitizer build of the device code, against the
arbitrary-precision reference, in both node-solver modes.  The host build replaces the predictor's v_log_f32 / v_exp_f32
by log2f / exp2f and rcp_refined by a division: it is held to the bounds, not to the GPU's bits.  Run by
tests/test_node_root.py with the ASan runtime preloaded and VICGPU_LIB pointing at the host build:
    python tools/hostemu/check_node_root.py"""
import os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from tests import node_cases as nc


def main():
    X, n1, ex, lb = nc.make_battery()
    refs = nc.references(X, n1, ex)
    m = nc.hook_model()
    Tb, Fb = nc.run_groups(nc.device_fn(m, newton=False), X, n1, ex)
    Tn, Fn = nc.run_groups(nc.device_fn(m, newton=True), X, n1, ex)
    rc = 0
    for name, (T, F, mode, other) in (("brent", (Tb, Fb, "brent", None)), ("newton", (Tn, Fn, "newton", (Tb, Fb)))):
        bad, worst = nc.check(X, n1, ex, lb, refs, T, F, mode, other)
        print("hostemu node %s: %d cases, %d violations; worst |T - r| per class: %s" % (
            name, len(X), len(bad), ", ".join("%s %.2e" % kv for kv in sorted(worst.items()))), flush=True)
        for b in bad[:20]:
            print("  " + b)
        if bad:
            rc = 1
    return rc


if __name__ == "__main__":
    sys.exit(main())
