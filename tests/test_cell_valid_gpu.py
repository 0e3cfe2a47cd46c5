"""Cell validity (vicgpu_set_retire_on_error / vicgpu_set_cell_valid / vicgpu_get_cell_valid, include/vicgpu.h) on the GPU:
cells whose step returned ERROR are retired on the device as the reference driver retires them (cell.isValid,
CONTINUEONERROR: vicNl.c:429, 521, 545-559).  The checks are those of tools/hostemu/check_cell_valid.py (see its header for
the three runs X, Y, Z and the assertions), here at sizes that fill a wave and leave a tail, with one cell chunk and with two.
Every case first proves that its inputs fail where it needs them to: run X and the CPU oracle flag exactly the cells
c % 3 == 1 after step 5."""
import importlib.util
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def chk(oracle_lib):
    spec = importlib.util.spec_from_file_location("check_cell_valid", os.path.join(ROOT, "tools", "hostemu", "check_cell_valid.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _model(d):
    from vic_amd.api import Model
    return Model(d)


def test_monolithic_kernel(chk, monkeypatch):
    """FULL_ENERGY, TFALLBACK = 0, 3 bands, 70 cells x 2 tiles (a full wave and a tail of 6), 16 steps from day 80: 23 cells fail."""
    monkeypatch.delenv("VICGPU_CHUNKS", raising=False)
    assert chk.check_retirement(_model, chk.MONOLITH, 70, 80) == 23


@pytest.mark.parametrize("chunks", ["1", "2"])
def test_finite_difference_pipeline(chk, monkeypatch, chunks):
    """FROZEN_SOIL, 10 nodes, 2 bands, 24 cells x 2 tiles, 16 steps from day 330, as one cell chunk and as two: 8 cells fail; their
    HRUs enter no work list, no dense wave's live set and no sparse round from step 6 on."""
    monkeypatch.setenv("VICGPU_CHUNKS", chunks)
    assert chk.check_retirement(_model, chk.FROZEN, 24, 330) == 8


def test_glacier_cells_stop_accumulating(chk, monkeypatch):
    """The finite-difference case with a glacier top band: cum_mass_balance of a retired cell is frozen, the fit gives the cell the
    default equation (0, 0, 0, -1) and resets nothing of it; the other cells' fits and resets equal the run with mask 0."""
    monkeypatch.delenv("VICGPU_CHUNKS", raising=False)
    assert chk.check_retirement(_model, chk.FROZEN, 24, 330, glacier=True) == 8


def test_cells_the_host_marks_invalid(chk, monkeypatch):
    """70 cells, no stress, mask 0, every 5th cell invalid before put_data_init: frozen at the initial tables with records of
    0.0 for 8 steps, then valid again and stepping like a fresh model started from those tables."""
    monkeypatch.delenv("VICGPU_CHUNKS", raising=False)
    assert chk.check_host_validity(_model, 70) == 14


def test_group_of_three_shards_against_one_context(chk, monkeypatch):
    """The 70-cell stress case in 3 ragged shards on the visible devices against one context: validity table, records, tables."""
    import torch
    from vic_amd.api import Group
    monkeypatch.delenv("VICGPU_CHUNKS", raising=False)
    n = max(torch.cuda.device_count(), 1)
    assert chk.check_group(lambda d: Group(d, devices=[k % n for k in range(3)]), _model, 70) == 23


def test_error_returns(chk, monkeypatch):
    """Every error return of the header on the real runtime."""
    monkeypatch.delenv("VICGPU_CHUNKS", raising=False)
    assert chk.check_errors(_model) >= 30
