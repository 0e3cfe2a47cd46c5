"""The Brent battery (tests/brent_cases.py, tests/golden/brent_traces.npz) through the sanitizer build of the device code:
vicgpu_debug_root_brent replays every case with Brent (bit for bit: only + - * / are involved) and the ERROR-free ones with
BrentLean (up to its documented difference).  Run by tests/test_brent.py with the ASan runtime preloaded and VICGPU_LIB
pointing at the host build:
    python tools/hostemu/check_brent.py"""
import os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from tests import brent_cases as bc
from tests import node_cases as nc
from vic_amd.abi import C


def main():
    g = bc.load_fixture()
    cases, runs = bc.fixture_battery(g)
    m = nc.hook_model()
    n = len(runs)
    b, f, off = bc.gather(g, list(range(n)))
    xreq, out = m.debug_root_brent(C["VICGPU_BRENT_FULL"], b, f, off)
    bad = bc.check_full(g, runs, xreq, out)
    print("hostemu brent: %d cases, %d problems" % (n, len(bad)), flush=True)
    for s in bad[:20]:
        print("  " + s)
    idx = bc.lean_cases(g)
    b, f, off = bc.gather(g, idx)
    xreq, out = m.debug_root_brent(C["VICGPU_BRENT_LEAN"], b, f, off)
    bad2, div = bc.check_lean(g, runs, xreq, out, idx)
    print("hostemu brent lean: %d cases, %d diverge, largest step difference %.3e (bound %.0e), %d problems" % (
        len(idx), len(div), max([d[3] for d in div] or [0.0]), bc.LEAN_STEP_REL, len(bad2)), flush=True)
    for s in bad2[:20]:
        print("  " + s)
    return 1 if (bad or bad2) else 0


if __name__ == "__main__":
    sys.exit(main())
