"""Model state copied between cells on the device (vicgpu_copy_cells / vicgpu_group_copy_cells, include/vicgpu.h) on the GPU:
the comparisons of tests/test_copy_cells.py (tools/hostemu/check_copy_cells.py holds them) on the real library, same shapes
and the same expectation -- a second model that makes the assignment through the host -- bit for bit, plus a larger rotation
that takes several row passes.  Error returns: only those the host refuses before any launch."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = ("VICGPU_CHUNKS", "VICGPU_COPY_STAGE_MB")


@pytest.fixture(scope="module")
def chk():
    spec = importlib.util.spec_from_file_location("check_copy_cells", os.path.join(ROOT, "tools", "hostemu", "check_copy_cells.py"))
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


@pytest.fixture(scope="module")
def qf(chk):
    return chk.quickflux()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fanout", "rotation", "resample", "swap", "rotation_row_per_pass"])
def test_pattern_equals_the_host_path_bit_for_bit(chk, qf, name):
    """140 cells = 4 members x 35 base cells of 6 or 9 HRUs (231 HRUs a member: the pair lists cross wave boundaries raggedly).
    The copy is queued behind a step that is not waited for; the tables right after it, then two records on both models."""
    dst, src, stage_mb = chk.patterns(qf)[name]
    lines = []
    bad, _ = chk.run_pattern(qf, dst, src, stage_mb, log=lambda s, flush=True: lines.append(s), name=name)
    assert not bad, (bad, lines)


@pytest.mark.gpu
def test_one_row_per_pass_gives_the_bits_of_the_default_budget(chk, qf):
    dst, src, _ = chk.patterns(qf)["rotation"]
    got = {}
    for mb in (None, "0"):
        m = chk.model(qf, mb)
        m.dist_prec(0, 1, sync=False)
        m.copy_cells(dst, src)
        got[mb] = chk.tables(m)
        m.close()
    assert not chk.differing(got[None], got["0"])


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", ["1", "2"])
def test_frozen_soil_pairs_across_the_chunk_boundary(chk, chunks):
    _run(chk.check_frozen, chunks=chunks)


@pytest.mark.gpu
def test_continuation_is_indistinguishable(chk):
    _run(chk.check_continuation)


@pytest.mark.gpu
def test_untouched_tables_and_cells(chk):
    _run(chk.check_untouched)


@pytest.mark.gpu
def test_group_of_three_shards_on_one_device_equals_one_context(chk):
    lines = _run(chk.check_group, devices=(0, 0, 0))
    assert sum("differing: none" in s for s in lines) == 3, lines


@pytest.mark.gpu
@pytest.mark.parametrize("stage_mb", [None, "1"])
def test_large_rotation_equals_the_host_path(chk, stage_mb):
    """4 members x 2 000 cells x 6 HRUs: 48 000 HRU pairs, 750 blocks a row tile.  A row of the SD table is 384 kB, so the
    default budget takes it in one pass and 1 MB in passes of two rows."""
    _run(chk.check_large, stage_mb=stage_mb)


@pytest.mark.gpu
def test_error_returns_refused_on_the_host(chk):
    lines = []
    bad, n = chk.error_returns(log=lambda s, flush=True: lines.append(s))
    assert not bad and n >= 35, (bad, lines)
