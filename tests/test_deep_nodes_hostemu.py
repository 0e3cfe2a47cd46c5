"""Deep columns through the sanitizer build of the device code (tools/hostemu), teacher-forced against the oracle with
both node solvers.  The scenarios start from a frozen column with cold spikes deep in it (tests/deep_scenarios.py
"cold_spikes"): every HRU keys its work list with 25 or more frozen nodes (the clamped top segment of the deep bound),
and the node root finds fail at nodes 34 / 41 / 47 in the first step -- so the 64-bit fall-back masks shift at bit 32 and
above, under UBSan, before any GPU time is spent.  (One step: from the second one the Gauss-Seidel iteration runs its
1000 sweeps without converging, too slow for the emulation; that whole-column flagging is pinned on the GPU.)"""
import re

import pytest

from tests.test_hostemu_sanitizers import _run, hostemu_lib  # noqa: F401  (fixture)


@pytest.mark.parametrize("solver", ["brent", "newton"])
def test_deep_columns_clean(hostemu_lib, solver):  # noqa: F811
    out = _run(*hostemu_lib, ["1", "deep_spikes_n50"], True, script="check_deep.py", VICGPU_NODE_SOLVER=solver)
    lines = [l for l in out.splitlines() if "worst rel diff" in l]
    assert len(lines) == 1, out
    for line, nn in zip(lines, (50,)):
        m = re.search(r"min frozen nodes at a step start (\d+); flagged nodes >= 32: \[([0-9, ]*)\]", line)
        assert m, line
        assert int(m.group(1)) >= 26, line
        flagged = {int(x) for x in m.group(2).split(",") if x.strip()}
        assert {34, 41, 47} <= flagged, line
