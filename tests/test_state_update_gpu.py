"""Model state read and changed in place, its dependent soil rows re-derived (vicgpu_get_state_rows / vicgpu_update_state /
vicgpu_derive_soil_state and their group forms, include/vicgpu.h) on the GPU: the comparisons of tests/test_state_update.py
(tools/hostemu/check_state_update.py holds them) on the real library, same shapes and the same expectations, plus a larger
shape that takes several row passes.  The derive is held to the reference's own tables (tests/golden/*.npz) and to the numpy
restatement; everything else is bit for bit.  Error returns: only those the host refuses before any launch."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = ("VICGPU_CHUNKS", "VICGPU_COPY_STAGE_MB")

# rel_diff(ref, got, 1e-12).max() of tests/util.py for the rows a derive produces.  The device's pow, exp and log differ from
# glibc's in the last ulps; 1e-12 is what test_pure_functions_on_device (tests/test_gpu_parity.py) holds
# VICGPU_PURE_SOIL_CONDUCTIVITY and VICGPU_PURE_MAX_UNFROZEN_WATER to, and far inside the 1e-6 tests/test_gpu_parity.py allows
# the same rows after a step.  Measured on one MI355X: the figures are in DESIGN.md (d).
GPU_TOL = 1e-12


@pytest.fixture(scope="module")
def chk():
    spec = importlib.util.spec_from_file_location("check_state_update", os.path.join(ROOT, "tools", "hostemu", "check_state_update.py"))
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
def test_derive_reproduces_the_reference_initial_state(chk):
    """Every fixture: sd0 / si0 with the produced rows overwritten, derive(all, NODES | LAYERS | FRONTS): back to the
    reference's state after initialize_model_state; integer rows exactly."""
    lines = _run(chk.check_initial, tol=GPU_TOL)
    assert sum(": Nnode" in s for s in lines) >= 14, lines


@pytest.mark.gpu
def test_derive_reproduces_the_reference_stepped_states(chk):
    """Every recorded step of every FULL_ENERGY / FROZEN_SOIL fixture (the 10-node and the 50-node instantiation), and a
    synthetic 14-node domain for the middle one."""
    lines = _run(chk.check_stepped, tol=GPU_TOL)
    assert sum(": Nnode" in s for s in lines) >= 13 and any("n14 (synthetic" in s for s in lines), lines


@pytest.mark.gpu
def test_derive_nodes_after_steps_changes_nothing(chk):
    _run(chk.check_selfcheck, tol=GPU_TOL)


@pytest.mark.gpu
def test_cap_moist_bit_for_bit_and_refused_with_glacier_dynamics(chk):
    _run(chk.check_cap)


@pytest.mark.gpu
def test_gather_and_scatter_bit_for_bit(chk):
    lines = _run(chk.check_rows)
    assert sum("differing: none" in s for s in lines) == 9, lines


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", ["1", "2"])
def test_mid_run_update_and_derive_in_the_finite_difference_pipeline(chk, chunks):
    _run(chk.check_midrun, chunks=chunks)


@pytest.mark.gpu
def test_nodes_above_the_bottom_layer_flag_their_cell(chk):
    _run(chk.check_errorpath, tol=GPU_TOL)


@pytest.mark.gpu
def test_hrus_without_area_get_empty_node_blocks(chk):
    _run(chk.check_zeroarea)


@pytest.mark.gpu
def test_untouched_tables_rows_and_columns(chk):
    _run(chk.check_untouched)


@pytest.mark.gpu
def test_group_of_three_shards_on_one_device_equals_one_context(chk):
    _run(chk.check_group, devices=(0, 0, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("stage_mb", [None, "1"])
def test_large_update_get_and_derive(chk, stage_mb):
    """4 members x 2 000 cells x 6 HRUs: 12 rows of three members, 36 000 columns.  A row of the update is 288 kB, so the default
    budget takes all rows in one pass and 1 MB in passes of 3 rows; then a derive over all 48 000 HRUs."""
    _run(chk.check_large, stage_mb=stage_mb, tol=GPU_TOL)


@pytest.mark.gpu
def test_error_returns_refused_on_the_host(chk):
    lines = []
    bad, n = chk.error_returns(log=lambda s, flush=True: lines.append(s))
    assert not bad and n >= 366, (bad, lines)
