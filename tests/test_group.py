"""The device group's partition (include/vicgpu_group.h) on the CPU, through the real libvicgpu.so (no device needed):
vicgpu_group_partition is the one definition of a shard, and it must be shard.partition_cells exactly."""
import numpy as np
import pytest

from vic_amd import abi, api, domain, shard
from vic_amd.abi import C


def _domains():
    yield "plain", domain.make_domain(37, abi.default_options(FULL_ENERGY=1), ntile=3)
    yield "wide", domain.make_domain(29, abi.default_options(FULL_ENERGY=1), ntile=4, soils="wide")
    yield "glacier", domain.make_domain(23, abi.default_options(FULL_ENERGY=1, Nband=3), ntile=2, glacier_top_band=True)
    # ragged HRU counts per cell: from 1 to 9 HRUs, and one cell with most of them
    rng = np.random.default_rng(3)
    for name, counts in (("ragged", rng.integers(1, 10, size=41)), ("lopsided", np.r_[np.ones(12, int), 200, np.ones(7, int)])):
        off = np.r_[0, np.cumsum(counts)].astype(np.int32)
        yield name, off


@pytest.mark.parametrize("name,dom", list(_domains()), ids=[n for n, _ in _domains()])
def test_partition_matches_shard_partition_cells(name, dom):
    off = dom if isinstance(dom, np.ndarray) else dom.cell_hru_offset
    ncell = len(off) - 1
    for nshard in range(1, 9):
        if nshard > ncell:
            continue
        want = shard.partition_cells(off, nshard)
        got = api.partition(off, nshard)
        assert np.array_equal(got, want), (name, nshard, got, want)
        assert got[0] == 0 and got[-1] == ncell and (np.diff(got) >= 0).all()


def test_partition_refuses_bad_shard_counts():
    lib = api.load_library()
    off = np.ascontiguousarray(domain.make_domain(5, abi.default_options(FULL_ENERGY=1), ntile=2).cell_hru_offset, dtype=np.int32)
    b = np.zeros(16, dtype=np.int32)
    ip = api._i
    assert lib.vicgpu_group_partition(5, ip(off), 0, ip(b)) == C["VICGPU_ERR_ARG"]
    assert lib.vicgpu_group_partition(5, ip(off), 6, ip(b)) == C["VICGPU_ERR_ARG"]
    assert lib.vicgpu_group_partition(5, ip(off), -1, ip(b)) == C["VICGPU_ERR_ARG"]
    assert lib.vicgpu_group_partition(5, ip(off), 5, ip(b)) == C["VICGPU_OK"]
    assert list(b[:6]) == list(shard.partition_cells(off, 5))


def test_group_mirrors_the_single_context_entries():
    """Every vicgpu_group_<name> mirror has its single-context vicgpu_<name>, and the Python Group exposes Model's methods
    through them; an entry without a group form is an error, not a silent per-shard call."""
    for n in api.GROUP_ENTRIES:
        assert "vicgpu_" + n in api.EXPORTED_SYMBOLS and "vicgpu_group_" + n in api.EXPORTED_SYMBOLS
    gl = api._GroupLib(api.load_library())
    assert gl.vicgpu_step is api.load_library().vicgpu_group_step
    assert gl.vicgpu_out_nvar is api.load_library().vicgpu_out_nvar
    with pytest.raises(AttributeError):
        gl.vicgpu_debug_pure
