"""Output records without a host round trip per record (vicgpu_records_config / vicgpu_run_records / vicgpu_records_wait and
their group forms, include/vicgpu_out.h), on the CPU: the unsanitized host build of the library (tools/hostemu) runs
tools/hostemu/check_records.py in a child process, which compares vicgpu_run_records with the loop it replaces --
vicgpu_step + vicgpu_get_outputs(reset) + vicgpu_get_cell_errors per record -- bit for bit on tiny domains, and walks
through every error return.  The packing kernel, the slot ring, the pitched copies of a chunk's and a shard's columns and
the host pipeline are the library's own code; only the runtime underneath is the emulation's (synchronous)."""
import os
import re
import subprocess
import sys

import pytest

from vic_amd.abi import C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tools", "hostemu", "build.sh")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
ENTRIES = ["records_config", "records_nrow", "run_records", "records_wait"]


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
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hostemu", "check_records.py")] + args, env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout


def test_headers_declare_and_library_exports_the_record_entries(plain_lib):
    out_h = open(os.path.join(ROOT, "include", "vicgpu_out.h")).read()
    group_h = open(os.path.join(ROOT, "include", "vicgpu_group.h")).read()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", plain_lib]).decode()
    for e in ENTRIES:
        assert re.search(r"\bint\s+vicgpu_%s\s*\(" % e, out_h), e
        assert re.search(r"\bint\s+vicgpu_group_%s\s*\(" % e, group_h), e
        for name in ("vicgpu_" + e, "vicgpu_group_" + e):
            assert re.search(r"\bT %s\b" % name, syms), "missing export " + name


def test_null_handles_are_refused():
    """The gfx950 library itself (hipcc cross-compiles it, loading it needs no GPU): no context is needed, and none is made, to
    be told that a null handle is an argument error."""
    from vic_amd import api, build as vb
    vb.build(force=False)
    lib = api.load_library()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", vb.OUT]).decode()
    for e in ENTRIES:
        assert re.search(r"\bT vicgpu_%s\b" % e, syms) and re.search(r"\bT vicgpu_group_%s\b" % e, syms), e
    for pre in ("vicgpu_", "vicgpu_group_"):
        assert getattr(lib, pre + "records_config")(None, 0, None, 1) == C["VICGPU_ERR_ARG"]
        assert getattr(lib, pre + "records_nrow")(None) == C["VICGPU_ERR_ARG"]
        assert getattr(lib, pre + "run_records")(None, 0, 1, None, None) == C["VICGPU_ERR_ARG"]
        assert getattr(lib, pre + "records_wait")(None, -1) == C["VICGPU_ERR_ARG"]


@pytest.mark.parametrize("case,lines", [("quickflux", 2), ("waterbalance_daily", 1), ("frozen_chunks", 1), ("group", 1)])
def test_run_records_equals_the_loop_bit_for_bit(plain_lib, case, lines):
    """quickflux: QUICK_FLUX, 3 bands, 7 cells x 2 tiles, R = 3, 4 records, depth 1 and 2, one step aggregated before the first
    record.  waterbalance_daily: FULL_ENERGY = 0, dt = 24, snow_step = 3, R = 1, 5 records, depth 2.  frozen_chunks: FROZEN_SOIL,
    10 nodes, 2 bands, 5 cells as two chunks, R = 2, 2 records.  group: 3 shards over 7 cells.  Records, error flags, state,
    fluxes, balance, accumulators, cell outputs and the step count of vicgpu_last_kernel_ms equal the loop's; the aggregates
    are zero afterwards; a second call reuses the slots."""
    out = _check(plain_lib, ["run", case])
    assert out.count("differing: none") == lines and out.count("aggregates zero: True") == lines, out


def test_refused_allocations_leave_nothing_behind(plain_lib):
    """vicgpu_records_config owns the row map, the slots and the events through the handles of vic_host.hpp: whichever of its
    allocations the runtime refuses, the call returns VICGPU_ERR_HIP with the count of live runtime objects where it was and
    no configuration; nvar = 0 releases what a successful call owns, vicgpu_destroy what a run used."""
    out = _check(plain_lib, ["refusals"])
    assert "7 refused, then through" in out and "problems: none" in out, out


def test_error_returns(plain_lib):
    """VICGPU_ERR_STATE: put_data or records not configured (dropped by vicgpu_put_data_config and vicgpu_set_domain, released
    by nvar = 0), no forcing chunk, wait before any run.  VICGPU_ERR_ARG: null handles, depth < 1, an id out of range or listed
    twice, nrecords < 1, a range past the chunk, out or cell_err not pinned, k outside the last call."""
    out = _check(plain_lib, ["errors"])
    m = re.search(r"records errors: (\d+) checks, failed: 0", out)
    assert m and int(m.group(1)) >= 40, out
