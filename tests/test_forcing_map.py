"""Cells that share forcing columns (vicgpu_set_forcing_map / vicgpu_get_forcing_map and their group forms, include/vicgpu.h),
on the CPU: the unsanitized host build of the library (tools/hostemu) runs tools/hostemu/check_forcing_map.py in a child
process.  An ensemble of 3 members on 5 shared columns -- members perturbed in b_infilt, Ds, MAX_SNOW_TEMP (0.5 / 3.0 / 1.5)
and the bands' Tfactor, so that they differ in results and in snowflags -- runs once with the identity map on forcing
replicated per cell and once with the map on the 5-wide forcing; every table must come out bit-identical, with the
member-major map of domain.tile_members and with a scrambled one (a fixed-seed random assignment with repeats and an unused
column).  A stride of ncell where ncol is meant, a step or sub-step offset of the wrong width, a flag read through the
column and an echo read through the cell each change a result at these shapes.  The kernels, the derived HRU row, the
pitched copies of a shard's columns and the host pipeline are the library's own code; only the runtime underneath is the
emulation's (synchronous)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from vic_amd import abi, domain
from vic_amd.abi import C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tools", "hostemu", "build.sh")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
ENTRIES = ["set_forcing_map", "get_forcing_map"]
NCOL, M = 5, 3


@pytest.fixture(scope="module")
def plain_lib():
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++")
    subprocess.check_call(["bash", BUILD], env=dict(os.environ, SAN="none"), stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "tools", "hostemu", "libvicgpu_hostemu_plain.so")


def _check(lib, args):
    env = dict(os.environ, VICGPU_LIB=lib)
    env.pop("LD_PRELOAD", None)
    env.pop("VICGPU_CHUNKS", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hostemu", "check_forcing_map.py")] + [str(a) for a in args], env=env,
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout


def test_headers_declare_and_libraries_export_the_entries(plain_lib):
    ctx_h = open(os.path.join(ROOT, "include", "vicgpu.h")).read()
    group_h = open(os.path.join(ROOT, "include", "vicgpu_group.h")).read()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", plain_lib]).decode()
    for e in ENTRIES:
        assert re.search(r"\bint\s+vicgpu_%s\s*\(" % e, ctx_h), e
        assert re.search(r"\bint\s+vicgpu_group_%s\s*\(" % e, group_h), e
        for name in ("vicgpu_" + e, "vicgpu_group_" + e):
            assert re.search(r"\bT %s\b" % name, syms), "missing export " + name
    assert C["VICGPU_ABI_VERSION"] == 3


def test_null_handles_are_refused():
    """The gfx950 library itself (hipcc cross-compiles it, loading it needs no GPU) exports the four entries and tells a null
    handle from an argument without a context."""
    import ctypes
    from vic_amd import api, build as vb
    vb.build(force=False)
    lib = api.load_library()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", vb.OUT]).decode()
    for e in ENTRIES:
        assert re.search(r"\bT vicgpu_%s\b" % e, syms) and re.search(r"\bT vicgpu_group_%s\b" % e, syms), e
    n = ctypes.c_int(0)
    one = np.zeros(1, dtype=np.int32)
    for pre in ("vicgpu_", "vicgpu_group_"):
        assert getattr(lib, pre + "set_forcing_map")(None, 1, one.ctypes.data_as(ctypes.POINTER(ctypes.c_int))) == C["VICGPU_ERR_ARG"]
        assert getattr(lib, pre + "set_forcing_map")(None, 0, None) == C["VICGPU_ERR_ARG"]
        assert getattr(lib, pre + "get_forcing_map")(None, ctypes.byref(n), None) == C["VICGPU_ERR_ARG"]


@pytest.mark.parametrize("ntile,bare,drop", [(2, 0.0, False), (3, 0.2, False), (2, 0.0, True)], ids=["regular", "bare_slots", "ragged"])
def test_tile_members_builds_the_member_major_domain(ntile, bare, drop):
    """domain.tile_members: cell m * ncol + j is a copy of cell j, the HRUs are numbered slot-major as make_domain numbers them
    (exactly make_domain's numbering for a regular domain), the CSR lists name every HRU once, in the base cell's order, and
    cell_col is j."""
    opt = abi.default_options(FULL_ENERGY=1, Nband=2)
    d = domain.make_domain(7, opt, ntile=ntile, bare_fraction=bare)
    if drop:
        dropped = np.zeros(d.nhru, dtype=bool)
        dropped[[3, 8, 9, 17]] = True
        domain.drop_hrus(d, dropped)
    D, col = domain.tile_members(d, 3)
    assert D.ncell == 21 and D.nhru == 3 * d.nhru and np.array_equal(col, np.tile(np.arange(7), 3))
    assert np.array_equal(D.cell_params, np.tile(d.cell_params, (1, 3)))
    cell = D.hru_iparams[C["HPI_CELL"]]
    assert np.array_equal(np.diff(D.cell_hru_offset), np.tile(np.diff(d.cell_hru_offset), 3))
    assert sorted(D.cell_hru_list.tolist()) == list(range(D.nhru))
    for c in range(D.ncell):
        new = D.cell_hru_list[D.cell_hru_offset[c]:D.cell_hru_offset[c + 1]]
        old = d.cell_hru_list[d.cell_hru_offset[c % 7]:d.cell_hru_offset[c % 7 + 1]]
        assert (cell[new] == c).all()
        for row in ("HPI_BAND", "HPI_VEG_INDEX", "HPI_VEG_CLASS", "HPI_IS_GLACIER", "HPI_IS_ARTIFICIAL_BARE"):
            assert np.array_equal(D.hru_iparams[C[row], new], d.hru_iparams[C[row], old]), row
        assert np.array_equal(D.hru_dparams[:, new], d.hru_dparams[:, old])
        assert np.array_equal(np.argsort(new, kind="stable"), np.argsort(old, kind="stable"))      # the same slot order
    if not drop:
        slot = np.arange(D.nhru) // D.ncell
        assert np.array_equal(cell, np.arange(D.nhru) % D.ncell)                                   # hru = slot * ncell + cell
        assert np.array_equal(D.hru_iparams[C["HPI_BAND"]], d.hru_iparams[C["HPI_BAND"]][slot * 7])


def test_make_snowflag_is_the_flag_rule_of_make_forcing():
    opt = abi.default_options(FULL_ENERGY=0, dt=24, snow_step=3, Nband=2)
    d = domain.make_domain(40, opt, ntile=1)
    f, sf, _ = domain.make_forcing(d, 0, 3, start_doy=60)
    assert sf.any() and np.array_equal(domain.make_snowflag(d, f), sf)
    col = np.arange(40)[::-1].copy()
    assert np.array_equal(domain.make_snowflag(d, f[..., col], np.argsort(col)), sf)


@pytest.mark.parametrize("case", ["full_energy", "waterbalance_daily", "frozen_chunks", "glacier"])
def test_mapped_run_equals_replicated_run_bit_for_bit(plain_lib, case):
    """full_energy: FULL_ENERGY with 3 bands x 2 tiles, 4 hourly steps.  waterbalance_daily: FULL_ENERGY = 0, dt = 24,
    snow_step = 3 (NF = 8: the NR slot and the sub-step stride), 3 steps.  frozen_chunks: FROZEN_SOIL, 10 nodes, 2 bands, the 15
    cells as two chunks, so that a chunk boundary cuts through member 1.  glacier: a glacier HRU in the top band, the
    mass-balance fit compared too.  State (double and int), fluxes, accumulators, cell outputs, cell error flags, balance,
    plain and aggregated output data (forcing echoes, OUT_PREC, per-band, per-layer) and the forcing read back, for both maps."""
    out = _check(plain_lib, ["run", case, NCOL, M])
    assert out.count("differing: none") == 2 and out.count("members differ: True") == 2 and out.count("clean run: True") == 2, out
    assert "member-major map" in out and "scrambled map" in out, out


def test_flags_are_read_through_the_cell(plain_lib):
    """The daily case on 40 columns, where the table has flags that differ between the members of a column (at 5 columns it
    has next to none): a step kernel that read the flag through the column would change these results."""
    out = _check(plain_lib, ["run", "waterbalance_daily", 40, M])
    assert out.count("differing: none") == 2 and out.count("clean run: True") == 2, out
    assert all(int(n) >= 1 for n in re.findall(r"flags apart within a column: (\d+)", out)), out


def test_raw_forcing_rows_once_per_column_flags_once_per_cell(plain_lib, oracle_lib):
    """vicgpu_prefetch_forcing_raw with a map on 40 columns (dt = 24, snow_step = 3, from day 60, 3 steps) against the replicated
    run: the derived rows bit for bit, the flags per cell; both against the oracle's derivation on the tiled domain (flags
    and the rows without a transcendental exactly, vp / vpd to 1e-11).  MAX_SNOW_TEMP 0.5 against 3.0 splits the members' flags
    on 7 (step, sub-step, column) of this table, so the per-cell flag is really tested."""
    out = _check(plain_lib, ["raw", 40, M])
    m = re.search(r"raw: (\d+) of (\d+) .* oracle: True, problems: none", out)
    assert m and int(m.group(1)) >= 1, out


def test_run_records_with_a_map_equals_the_loop_with_a_map(plain_lib):
    out = _check(plain_lib, ["records", NCOL, M])
    assert "finite and non-zero: True, differing: none" in out, out


def test_group_of_three_shards_equals_one_context(plain_lib):
    """3 shards over the 15 cells against one context, for the member-major and the scrambled map, and for a blocked one
    (consecutive cells on one column), with which the shards' column ranges start at columns 0, 1 and 3."""
    out = _check(plain_lib, ["group", NCOL, M, 3])
    assert out.count("differing: none") == 3 and "shards at [0, 5, 10, 15]" in out, out


def test_error_and_lifetime_returns(plain_lib):
    """VICGPU_ERR_STATE before a domain; VICGPU_ERR_ARG for null handles, ncol < 1 with a map and entries out of range, which
    leave the old map and chunk usable (a step still succeeds); a step after a new map is VICGPU_ERR_STATE until a push;
    vicgpu_set_domain and NULL restore the identity (ncol == ncell, cell_col[c] == c)."""
    out = _check(plain_lib, ["errors"])
    m = re.search(r"forcing map errors: (\d+) checks, failed: 0", out)
    assert m and int(m.group(1)) >= 45, out


def test_refused_allocations_leave_nothing_behind(plain_lib):
    """Whichever allocation of vicgpu_set_forcing_map the runtime refuses, the call returns VICGPU_ERR_HIP with the count of live
    runtime objects where it was and the map in force unchanged; the identity releases what a successful call owns."""
    out = _check(plain_lib, ["refusals"])
    assert "2 refused, then through owning 2 objects" in out and "problems: none" in out, out
