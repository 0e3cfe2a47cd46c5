"""Model state combined linearly across cells (vicgpu_mix_cells, include/vicgpu.h) on the GPU: the comparisons of
tests/test_mix_cells.py (tools/hostemu/check_mix_cells.py holds them) on the real library, same shapes and the same
expectations -- numpy in the contract's order, bit for bit, NaNs by position -- plus a larger shape that takes several row
passes.  Error returns: only those the host refuses before any launch."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = ("VICGPU_CHUNKS", "VICGPU_COPY_STAGE_MB")


@pytest.fixture(scope="module")
def chk():
    spec = importlib.util.spec_from_file_location("check_mix_cells", os.path.join(ROOT, "tools", "hostemu", "check_mix_cells.py"))
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
def test_dense_member_transform_bit_for_bit(chk):
    """924 HRUs (more than one wave, no multiple of 64), 11 rows (no multiple of the row tile); the default stage and one row
    per pass give the same bits, numpy's."""
    _run(chk.check_dense)


@pytest.mark.gpu
def test_per_column_transform(chk):
    _run(chk.check_percolumn)


@pytest.mark.gpu
def test_irregular_terms_and_simultaneity(chk):
    _run(chk.check_irregular)


@pytest.mark.gpu
def test_special_values_and_weight_one_equals_copy_cells(chk):
    _run(chk.check_special)


@pytest.mark.gpu
def test_untouched_tables_rows_and_columns(chk):
    _run(chk.check_untouched)


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", ["1", "2"])
def test_mid_run_mix_in_the_finite_difference_pipeline(chk, chunks):
    _run(chk.check_midrun, chunks=chunks)


@pytest.mark.gpu
def test_error_returns_refused_on_the_host(chk):
    lines = []
    bad, n = chk.error_returns(log=lambda s, flush=True: lines.append(s))
    assert not bad and n >= 70, (bad, lines)


@pytest.mark.gpu
@pytest.mark.parametrize("stage_mb", [None, "1"])
def test_large_mix_and_derive(chk, stage_mb):
    """4 members x 2 000 cells x 6 HRUs: a dense 4 x 4 W on 12 rows of 48 000 HRUs.  A row of the stage is 384 kB, so the default
    budget takes all rows in one pass and 1 MB in passes of 2 rows; then a derive over all HRUs."""
    _run(chk.check_large, stage_mb=stage_mb)
