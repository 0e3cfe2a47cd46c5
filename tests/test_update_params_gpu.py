"""Cell and HRU parameters updated in place (vicgpu_update_cell_params / vicgpu_update_hru_params and their group forms,
include/vicgpu.h) on the GPU: the comparisons of tests/test_update_params.py (tools/hostemu/check_update_params.py holds
them) on the real library, same shapes and the same expectation -- a second model that takes the updated tables through
vicgpu_set_domain -- bit for bit, plus a larger update that takes several row passes.  Error returns: only those the host
refuses before any launch."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = ("VICGPU_CHUNKS", "VICGPU_COPY_STAGE_MB")


@pytest.fixture(scope="module")
def chk():
    spec = importlib.util.spec_from_file_location("check_update_params", os.path.join(ROOT, "tools", "hostemu", "check_update_params.py"))
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
def test_update_before_the_run_equals_set_domain_bit_for_bit(chk):
    """140 cells = 4 members x 35 base cells of 6 or 9 HRUs; 70 listed cells (a wave and a ragged one), 14 rows; the listed
    form, the dense form over all rows, one row per pass: the tables and the records of all variables."""
    lines = _run(chk.check_start)
    assert sum("differing: none" in s for s in lines) == 3, lines


@pytest.mark.gpu
def test_derived_conductivity_rows_follow_the_soil_rows(chk):
    _run(chk.check_derived)


@pytest.mark.gpu
def test_tree_line_rows_follow_cv_and_abovetreeline(chk):
    lines = _run(chk.check_treeline)
    assert sum("differing: none" in s for s in lines) == 2, lines


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", ["1", "2"])
def test_mid_run_update_in_the_finite_difference_pipeline(chk, chunks):
    _run(chk.check_midrun, chunks=chunks)


@pytest.mark.gpu
def test_untouched_tables_and_columns(chk):
    _run(chk.check_untouched)


@pytest.mark.gpu
def test_group_of_three_shards_on_one_device_equals_one_context(chk):
    _run(chk.check_group, devices=(0, 0, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("stage_mb", [None, "1"])
def test_large_update_equals_set_domain(chk, stage_mb):
    """4 members x 2 000 cells x 6 HRUs: every CP row of three members, 6 000 columns.  A row of the update is 48 kB, so the
    default budget takes all rows in one pass and 1 MB in passes of 21 rows."""
    _run(chk.check_large, stage_mb=stage_mb)


@pytest.mark.gpu
def test_error_returns_refused_on_the_host(chk):
    lines = []
    bad, n = chk.error_returns(log=lambda s, flush=True: lines.append(s))
    assert not bad and n >= 140, (bad, lines)
