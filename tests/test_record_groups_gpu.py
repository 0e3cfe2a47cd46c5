"""Output records reduced over cell groups (vicgpu_records_set_groups, include/vicgpu_out.h) on the GPU: the comparisons of
tests/test_record_groups.py (tools/hostemu/check_record_groups.py holds them and the numpy statement of the contract) at sizes
where a group takes several passes of a wave.  Each case runs a plain model and a grouped one from the same state; the
grouped records must equal the contract applied to the plain float records bit for bit."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = dict(FULL_ENERGY=1, Nband=3)
FROZEN = dict(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=10, Nband=2, frozen_compat=0)


@pytest.fixture(scope="module")
def chk():
    spec = importlib.util.spec_from_file_location("check_record_groups", os.path.join(ROOT, "tools", "hostemu", "check_record_groups.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    saved = os.environ.get("VICGPU_CHUNKS")
    yield mod
    if saved is None:
        os.environ.pop("VICGPU_CHUNKS", None)      # the cases set it; a domain reads it when it is set
    else:
        os.environ["VICGPU_CHUNKS"] = saved


def _run(chk, name, spec):
    lines = []
    bad = chk.run(name, spec, log=lambda s, flush=True: lines.append(s))
    print("\n".join(lines))
    assert not bad, (bad, lines)
    return lines


@pytest.mark.gpu
def test_wave_per_group_equals_the_contract(chk):
    """QUICK_FLUX, 3 bands, 200 cells x 2 tiles (three full waves and a tail of 8), R = 3, 3 records through 2 slots.  Groups:
    all 200 cells in scrambled order (four passes, ragged last), 65, 64 and 1 members, an empty group, two groups that share
    cells in permuted order, a cell repeated within a group (the cancelling pair that shows the order in the float result).
    Also: tables after the call, the follow-on call, removal."""
    spec = (QUICK, 200, 2, 80, 3, 3, (2,), 1, (None,), lambda n: chk.mixed_groups(n, (200, 65, 64, 1)), -9.0)
    lines = _run(chk, "gpu_quickflux", spec)
    assert any("differs from the contract's order in" in s and " in 0 of" not in s for s in lines), lines


@pytest.mark.gpu
def test_lane_per_group_grid_equals_the_contract(chk):
    """The same domain on a 260-node grid with fill 1e20 and no weights: the lane-per-group kernel (no group has more than one
    member), five blocks with a ragged last one."""
    spec = (QUICK, 200, 2, 80, 3, 3, (2,), 1, (None,), lambda n: chk.grid_groups(n, 260), 1e20)
    _run(chk, "gpu_grid", spec)


@pytest.mark.gpu
def test_groups_across_cell_chunks_equal_the_contract(chk):
    """FROZEN_SOIL, 10 nodes, 2 bands, 24 cells x 2 tiles, VICGPU_CHUNKS 1 and 2 (boundary at cell 12), R = 3, 4 records,
    depth 2: the reduction of a record is a join of the chunks.  Groups: all 24 cells, the cells 10..13 across the boundary,
    a cancelling pair in front of all cells.  Results are identical for both chunk counts."""
    spec = (FROZEN, 24, 2, 330, 3, 4, (2,), 0, ("1", "2"), lambda n: chk.span_groups(n, 10, 14), 0.5)
    lines = _run(chk, "gpu_frozen_chunks", spec)
    assert sum("differing: none" in s for s in lines) == 2, lines
