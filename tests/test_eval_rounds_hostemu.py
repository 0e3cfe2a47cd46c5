"""The evaluation rounds through the sanitizer build of the device code (tools/hostemu), with fresh device allocations
poisoned: dense rounds only (VICGPU_EVAL_LIST_PCT=0) and rounds formed from the flat pending list from the second round on
(100), teacher-forced against the oracle and compared with each other bit for bit (tools/hostemu/check_eval_rounds.py).
A clean run means that the stripe appends stay inside their stripes, that no wave reads a list entry, a prefix word or a
parked context word that nothing has written, and that the parking map sends no two words to one place -- before any GPU
time is spent.  1 cell has fewer HRUs than a wave; 67 cells (27 waves) end in a ragged wave.

The emulation pays for every wave it launches (64 fibers), so the 67-cell case is slow: about 11 minutes for its two runs of
3 steps, against 3.5 for the 1-cell case -- hence a time limit of its own."""
import os
import subprocess
import sys

import pytest

from tests.test_hostemu_sanitizers import ROOT, hostemu_lib  # noqa: F401  (fixture)


def _run(lib, rt, args):
    env = dict(os.environ, LD_PRELOAD=rt, VICGPU_LIB=lib, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", HOSTEMU_POISON="1")
    env.pop("VICGPU_EVAL_LIST_PCT", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hostemu", "check_eval_rounds.py")] + args, env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=3000)
    report = [l for l in p.stderr.splitlines() if "runtime error" in l or "ERROR: AddressSanitizer" in l]
    assert not report, "\n".join(report[:10])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


@pytest.mark.parametrize("ncell", ["1", "67"])
def test_eval_rounds_clean(hostemu_lib, ncell):  # noqa: F811
    out = _run(*hostemu_lib, ["3", ncell])
    assert out.count("worst rel diff") == 2, out
    assert "pct 0 and 100 bit-identical" in out, out
