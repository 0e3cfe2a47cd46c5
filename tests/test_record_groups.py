"""Output records reduced over cell groups on the device (vicgpu_records_set_groups / vicgpu_records_get_groups /
vicgpu_records_ncol, include/vicgpu_out.h), on the CPU: the unsanitized host build of the library (tools/hostemu) runs
tools/hostemu/check_record_groups.py in a child process.  The expected values are the header's contract restated in numpy
(explicit loops, float64 products) over the float records of a second model that runs the plain vicgpu_run_records from the same
state; the grouped output must equal that bit for bit.  The reduce kernels, the join of the cell chunks and the host pipeline
are the library's own code; only the runtime underneath is the emulation's (synchronous)."""
import os
import re
import subprocess
import sys

import pytest

from vic_amd.abi import C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tools", "hostemu", "build.sh")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
ENTRIES = ["records_set_groups", "records_get_groups", "records_ncol"]


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
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hostemu", "check_record_groups.py")] + args, env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout


def test_headers_declare_and_libraries_export_the_entries(plain_lib):
    from vic_amd import build as vb
    vb.build(force=False)
    out_h = open(os.path.join(ROOT, "include", "vicgpu_out.h")).read()
    group_h = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "vicgpu_group.h")).read(), flags=re.S)
    for lib in (plain_lib, vb.OUT):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
        for e in ENTRIES:
            assert re.search(r"\bint\s+vicgpu_%s\s*\(" % e, out_h), e
            assert re.search(r"\bT vicgpu_%s\b" % e, syms), "missing export vicgpu_%s in %s" % (e, lib)
            assert "vicgpu_group_" + e not in group_h and "vicgpu_group_" + e not in syms, "the entries have no group form"
    assert "vicgpu_records_set_groups" in open(os.path.join(ROOT, "include", "vicgpu_group.h")).read(), "vicgpu_group.h says why"


def test_null_handles_are_refused():
    """The gfx950 library itself (hipcc cross-compiles it, loading it needs no GPU)."""
    import ctypes
    from vic_amd import api, build as vb
    vb.build(force=False)
    lib = api.load_library()
    n = ctypes.c_int(0)
    assert lib.vicgpu_records_set_groups(None, 0, None, None, None, 0.0) == C["VICGPU_ERR_ARG"]
    assert lib.vicgpu_records_get_groups(None, ctypes.byref(n), ctypes.byref(n)) == C["VICGPU_ERR_ARG"]
    assert lib.vicgpu_records_ncol(None) == C["VICGPU_ERR_ARG"]


def test_the_numpy_contract_is_the_stated_order():
    """The checker's restatement on values small enough to follow by hand: a single member of weight 1 reproduces the float with
    -0.0 as +0.0; 65 members put member 64 on lane 0 behind member 0; an empty group holds the fill value."""
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location("check_record_groups", os.path.join(ROOT, "tools", "hostemu", "check_record_groups.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    v = np.array([[-0.0, 1.5, 3.0e-8]], dtype=np.float32)
    one = chk.contract(v, [0, 1, 2, 2], [0, 1], None, 7.0)
    assert one.view(np.uint32).tolist() == [[0, np.float32(1.5).view(np.uint32), np.float32(7.0).view(np.uint32)]]
    # 65 members: lane 0 holds (t_0 + t_64), so with t_0 = 1, t_64 = 2^-53 and t_1 = 2^-53 the contract rounds t_64 away first
    # (1 + 2^-53 = 1, then + 2^-53 from lane 1 = 1 again); adding the two small terms to each other first gives 1 + 2^-52
    x = np.zeros((1, 65), dtype=np.float32)
    x[0, 0], x[0, 1], x[0, 64] = 1.0, 1.0, 1.0
    w = np.zeros(65)
    w[0], w[1], w[64] = 1.0, 2.0 ** -53, 2.0 ** -53
    t = chk._terms(x, list(range(65)), w)
    assert float(chk._contract_sum(t)[0]) == 1.0
    assert float(chk._left_to_right_sum([t[1], t[64], t[0]])[0]) == 1.0 + 2.0 ** -52


@pytest.mark.parametrize("case,lines", [("quickflux", 2), ("grid", 1), ("frozen_chunks", 2)])
def test_grouped_records_equal_the_contract_bit_for_bit(plain_lib, case, lines):
    """quickflux: QUICK_FLUX, 3 bands, 130 cells x 2 tiles, R = 3, 4 records, depth 1 and 2 (the ring wraps), one step aggregated
    before the first record; groups: all 130 cells in scrambled order, 65 cells, 64 cells, 1 cell, an empty group, two groups
    sharing cells, and a group in which a cell repeats (a cancelling pair of weights in front of 68 small terms).  grid: the
    same domain through the lane-per-group kernel, a 150-node grid with the 130 cells scattered over it, fill 1e20, no weights.
    frozen_chunks: FROZEN_SOIL, 10 nodes, 2 bands, 5 cells as two chunks (boundary at cell 2), R = 2, 3 records, depth 1 and 2;
    groups: all cells, the cells 1..3 across the boundary, a cancelling pair in front of all cells.
    Each case with a multi-member group first shows that a left-to-right sum of the same terms differs from the contract's
    order in the float result.  Then: grouped records of the first and of a second call equal the contract; cell_err records,
    state, fluxes, balance, accumulators and cell outputs equal the plain run's; the aggregates are zero; with the groups
    removed a third call delivers the plain [nrow][ncell] records; nothing depends on depth."""
    out = _check(plain_lib, ["run", case])
    assert out.count("differing: none") == lines and "problems: none" in out, out
    if case != "grid":
        m = re.search(r"differs from the contract's order in (\d+) of", out)
        assert m and int(m.group(1)) > 0, out


def test_error_and_lifetime_returns(plain_lib):
    """VICGPU_ERR_STATE without a records configuration (before vicgpu_put_data_config, before vicgpu_records_config, after
    nvar = 0, vicgpu_put_data_config and vicgpu_set_domain); another vicgpu_records_config drops the groups; VICGPU_ERR_ARG for
    null handles and result pointers, ngroup < 0, missing tables, bad offsets, cells out of range, weights that are not finite,
    each leaving the groups in force; ngroup = 0 removes; empty groups deliver the fill value; vicgpu_group_run_records refuses
    a shard whose context has groups set, and runs again once they are removed; Group.records_set_groups raises."""
    out = _check(plain_lib, ["errors"])
    m = re.search(r"record groups errors: (\d+) checks, failed: 0", out)
    assert m and int(m.group(1)) >= 45, out


def test_refused_allocations_leave_nothing_behind(plain_lib):
    """Offsets, cells, weights and one [nrow][ngroup] table per slot (depth 3): whichever allocation the runtime refuses, the
    call returns VICGPU_ERR_HIP with the count of live runtime objects where it was and the groups in force kept."""
    out = _check(plain_lib, ["refusals"])
    assert "6 refused" in out and "problems: none" in out, out
