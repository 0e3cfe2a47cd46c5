"""Shared raw forcing expanded and perturbed per column (vicgpu_prefetch_forcing_perturbed, include/vicgpu.h) on the GPU: the
comparisons of tests/test_forcing_perturb.py (tools/hostemu/check_forcing_perturb.py holds them) with 3 members on 40 source
columns, 120 forcing columns.  The member boundaries fall at lanes 40 and 16 of the two 64-lane waves of a step, so a wave
reads the sources and the factors of two members and the source index restarts inside it.  The reference side is
vicgpu_prefetch_forcing_raw on the 120-wide table numpy builds, and the oracle's derivation of it."""
import importlib.util
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSRC, M = 40, 3


@pytest.fixture(scope="module")
def chk():
    here = os.path.join(ROOT, "tools", "hostemu")
    if here not in sys.path:
        sys.path.insert(0, here)               # the check imports check_forcing_map, its neighbour
    spec = importlib.util.spec_from_file_location("check_forcing_perturb", os.path.join(here, "check_forcing_perturb.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    saved = os.environ.get("VICGPU_CHUNKS")
    yield mod
    if saved is None:
        os.environ.pop("VICGPU_CHUNKS", None)      # the cases clear it; a domain reads it when it is set
    else:
        os.environ["VICGPU_CHUNKS"] = saved


@pytest.mark.gpu
def test_table_bit_for_bit_and_against_the_oracle(chk, oracle_lib):
    """Member-major, scrambled and group-per-column lists; pert NULL with and without col_src; an explicit identity pert."""
    bad, facts = chk.run_table(NSRC, M, oracle_lib)
    print(facts)
    assert not bad, bad
    assert not chk.facts_missing(facts), chk.facts_missing(facts)
    assert facts["wind_floored"] > facts["wind_floored_unperturbed"] >= 1


@pytest.mark.gpu
def test_composes_with_a_forcing_map(chk, oracle_lib):
    bad, split = chk.run_mapped(oracle_lib)
    assert not bad, bad
    assert split >= 1, "no flag differs within a column: a flag read through the column would pass"


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["daily", "hourly"])
def test_runs_equal_the_replicated_call_bit_for_bit(chk, shape):
    """State (double and int), fluxes, accumulators, cell outputs, error flags, balance, plain and aggregated output data and
    the forcing read back, 3 daily / 4 hourly steps from the same state through the new entry and through the replicated call."""
    bad, members_differ, ok = chk.run_steps(shape, NSRC, M)
    assert not bad, bad
    assert members_differ and ok


@pytest.mark.gpu
def test_streamed_chunks_equal_one_chunk(chk):
    """prefetch(k + 1) issued before step(k); every chunk by the new entry, and alternating with vicgpu_prefetch_forcing_raw."""
    bad, ok = chk.run_stream(NSRC, M)
    assert not bad, bad
    assert ok


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["member-major", "scrambled", "blocked"])
def test_group_of_two_shards_on_one_device_equals_one_context(chk, kind):
    bad, bounds = chk.run_group(NSRC, M, [0, 0], kind)
    assert not bad, bad
    assert bounds.tolist() == [0, 60, 120]


@pytest.mark.gpu
def test_error_and_lifetime_returns(chk, capsys):
    assert chk.errors() == 0, capsys.readouterr().out
