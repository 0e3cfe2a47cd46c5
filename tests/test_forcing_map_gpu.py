"""Cells that share forcing columns (vicgpu_set_forcing_map, include/vicgpu.h) on the GPU: the comparisons of
tests/test_forcing_map.py (tools/hostemu/check_forcing_map.py holds them) with 3 members on 40 columns, 120 cells.  The member
boundaries fall at lanes 40 and 16 of the two 64-lane waves of a slot, so a wave reads the columns of two members and the
column index restarts inside it."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCOL, M = 40, 3


@pytest.fixture(scope="module")
def chk():
    spec = importlib.util.spec_from_file_location("check_forcing_map", os.path.join(ROOT, "tools", "hostemu", "check_forcing_map.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    saved = os.environ.get("VICGPU_CHUNKS")
    yield mod
    if saved is None:
        os.environ.pop("VICGPU_CHUNKS", None)      # the cases set it; a domain reads it when it is set
    else:
        os.environ["VICGPU_CHUNKS"] = saved


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["member-major", "scrambled"])
@pytest.mark.parametrize("case", ["full_energy", "waterbalance_daily", "frozen", "frozen_chunks", "glacier"])
def test_mapped_run_equals_replicated_run_bit_for_bit(chk, case, kind):
    """Identity map on forcing replicated per cell against the map on the 40-wide forcing, from the same state: state, fluxes,
    accumulators, cell outputs, error flags, balance, plain and aggregated output data, the forcing read back and (glacier) the
    mass-balance fit.  frozen runs the finite-difference pipeline as one chunk, frozen_chunks as two."""
    bad, members_differ, ok, split = chk.run_case(case, NCOL, M, kind)
    assert not bad, bad
    assert members_differ and ok
    if case == "waterbalance_daily":
        assert split >= 1, "no flag differs within a column: a flag read through the column would pass"


@pytest.mark.gpu
def test_raw_forcing_rows_once_per_column_flags_once_per_cell(chk, oracle_lib):
    bad, split, nflag = chk.run_raw(NCOL, M, oracle_lib)
    assert not bad, bad
    assert split >= 1, "no (step, sub-step, column) whose members' flags differ: the per-cell flag is not tested"


@pytest.mark.gpu
def test_run_records_with_a_map_equals_the_loop_with_a_map(chk):
    bad, ok = chk.run_records(NCOL, M, depth=2)
    assert not bad, bad
    assert ok


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["member-major", "scrambled", "blocked"])
def test_group_of_two_shards_on_one_device_equals_one_context(chk, kind):
    bad, bounds = chk.run_group("full_energy", NCOL, M, [0, 0], kind)
    assert not bad, bad
    assert bounds.tolist() == [0, 60, 120]
