"""The per-column ensemble transform solved and applied on the device (vicgpu_member_transform_solve / _set / _get / _apply,
include/vicgpu.h) on the GPU: the comparisons of tests/test_member_transform.py (tools/hostemu/check_member_transform.py holds
them) on the real library, same shapes and the same expectations -- the apply against vicgpu_mix_cells bit for bit, the solve
against mpmath and numpy -- plus one analysis cycle end to end.  Error returns: only those the host refuses before any launch."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = ("VICGPU_CHUNKS", "VICGPU_COPY_STAGE_MB", "VICGPU_TRANSFORM_SWEEPS")


@pytest.fixture(scope="module")
def chk():
    spec = importlib.util.spec_from_file_location("check_member_transform", os.path.join(ROOT, "tools", "hostemu", "check_member_transform.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    saved = {k: os.environ.get(k) for k in ENV}
    yield mod
    for k, v in saved.items():           # the cases set them; a domain reads them when it is set
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def _run(fn, **kw):
    lines = []
    bad = fn(log=lambda s, flush=True: lines.append(s), **kw)
    print("\n".join(lines))
    assert not bad, (bad, lines)
    return lines


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(4, 35), (16, 9), (64, 2)])
def test_apply_equals_mix_cells_bit_for_bit(chk, shape):
    """924 HRUs at 4 x 35 (more than one wave, no multiple of 64), 11 rows (no multiple of the row tile); the default stage and
    one row per pass; all columns and a shuffled subset; a random T and the T a solve leaves."""
    _run(chk.check_apply, shapes=(shape,))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(4, 35), (16, 9), (64, 2)])
def test_solve_accuracy_against_mpmath_and_numpy(chk, shape):
    """The bound and the yardsticks of tests/test_member_transform.py::test_solve_accuracy_against_mpmath_and_numpy; the figures
    measured on the GPU are in DESIGN.md (d)."""
    _run(chk.check_accuracy, shapes=(shape,))


@pytest.mark.gpu
def test_guarantees_a_to_d(chk):
    _run(chk.check_guarantees)


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", ["1", "2"])
def test_mid_run_apply_in_the_finite_difference_pipeline(chk, chunks):
    _run(chk.check_midrun, chunks=chunks)


@pytest.mark.gpu
def test_error_returns_refused_on_the_host(chk):
    lines = []
    bad, n = chk.error_returns(log=lambda s, flush=True: lines.append(s))
    assert not bad and n >= 40, (bad, lines)


@pytest.mark.gpu
def test_analysis_cycle_end_to_end(chk):
    """4 members x 12 columns, FULL_ENERGY + FROZEN_SOIL: steps, hx from the snow water equivalent, solve, apply on the SWE and the
    moisture rows, derive_soil_state, more steps: no cell error flag, finite outputs, the state equal to the mix_cells twin."""
    _run(chk.check_endtoend)
