"""Generates tests/golden/brent_traces.npz: the reference's own run (RootBrent::root_brent, root_brent.c:97-337, through
oracle/_ref/libvicref.so) of every case of the Brent battery (tests/brent_cases.py): bounds, the values it was given, the
abscissae it asked for, its result and whether it failed.  The slow-to-make scripted cases (the oracle's traces, the
adversarial long main loops) are generated here and read back from the fixture by the tests.

    python tests/golden/make_golden_brent.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import pyref  # noqa: E402
from tests import brent_cases as bc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "brent_traces.npz")


def main():
    assert pyref.have_ref("plain"), "build the reference harness first (oracle/ref_build/build_ref.sh)"
    cases, runs = bc.run_battery(bc.make_battery(recorded=bc.recorded_scripts()))
    for c, R in zip(cases, runs):                 # the reference's run, which the transcription must reproduce
        r, xs, fs, err = pyref.ref_root_brent(c.lower, c.upper, c.make())
        assert (r, xs, fs, bool(err)) == (R.result, R.xs, R.fs, R.failed), (c.cls, c.lower, c.upper)
        R.result, R.xs, R.fs, R.failed = r, xs, fs, bool(err)
    np.savez_compressed(OUT, **bc.pack(cases, runs))
    print("%s: %d cases, %d evaluations, %d bytes" % (OUT, len(cases), sum(len(R.fs) for R in runs), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
