"""Model state copied between cells on the device (vicgpu_copy_cells / vicgpu_group_copy_cells, include/vicgpu.h), on the CPU:
the unsanitized host build of the library (tools/hostemu) runs tools/hostemu/check_copy_cells.py in a child process.  The
expected values come from a second model of the same domain that performs the same assignment through the host (get_state /
get_fluxes, the columns permuted with numpy, set_state / set_fluxes); every comparison is bit for bit.  The planner, the copy
kernels and the host code are the library's own; only the runtime underneath is the emulation's (synchronous).  The planner
and the kernels also run as a stand-alone program under ASan + UBSan (tools/hostemu/copy_cells_check.cpp)."""
import os
import re
import subprocess
import sys

import pytest

from vic_amd.abi import C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tools", "hostemu", "build.sh")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"          # CXX of tools/hostemu/build.sh


@pytest.fixture(scope="module")
def plain_lib():
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++")
    subprocess.check_call(["bash", BUILD], env=dict(os.environ, SAN="none"), stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "tools", "hostemu", "libvicgpu_hostemu_plain.so")


def _check(lib, what):
    env = dict(os.environ, VICGPU_LIB=lib)
    for k in ("LD_PRELOAD", "VICGPU_CHUNKS", "VICGPU_COPY_STAGE_MB"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hostemu", "check_copy_cells.py"), what], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "copy cells %s: problems: none" % what in p.stdout, p.stdout
    return p.stdout


def test_headers_declare_and_libraries_export_the_entries(plain_lib):
    from vic_amd import build as vb
    vb.build(force=False)
    ctx_h = open(os.path.join(ROOT, "include", "vicgpu.h")).read()
    group_h = open(os.path.join(ROOT, "include", "vicgpu_group.h")).read()
    assert re.search(r"\bint\s+vicgpu_copy_cells\s*\(", ctx_h)
    assert re.search(r"\bint\s+vicgpu_group_copy_cells\s*\(", group_h)
    assert C["VICGPU_COPY_STATE"] == 1 and C["VICGPU_COPY_BALANCE"] == 2 and C["VICGPU_ABI_VERSION"] == 3
    for lib in (plain_lib, vb.OUT):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
        for e in ("vicgpu_copy_cells", "vicgpu_group_copy_cells"):
            assert re.search(r"\bT %s\b" % e, syms), "missing export %s in %s" % (e, lib)


def test_null_handles_are_refused():
    """The gfx950 library itself (hipcc cross-compiles it, loading it needs no GPU)."""
    import ctypes
    from vic_amd import api, build as vb
    vb.build(force=False)
    lib = api.load_library()
    one = (ctypes.c_int * 1)(0)
    for what in (C["VICGPU_COPY_STATE"], C["VICGPU_COPY_STATE"] | C["VICGPU_COPY_BALANCE"]):
        assert lib.vicgpu_copy_cells(None, 1, one, one, what) == C["VICGPU_ERR_ARG"]
        assert lib.vicgpu_group_copy_cells(None, 1, one, one, what) == C["VICGPU_ERR_ARG"]
    assert lib.vicgpu_copy_cells(None, 0, None, None, C["VICGPU_COPY_STATE"]) == C["VICGPU_ERR_ARG"]


def test_patterns_equal_the_host_path_bit_for_bit(plain_lib):
    """QUICK_FLUX, 3 bands, 35 base cells of 6 or 9 HRUs x 4 members (140 cells, 231 HRUs a member) on shared forcing columns,
    every member from its own state (asserted).  Fan-out 0 -> 1, 2, 3 (direct); rotation 0 -> 1 -> 2 -> 3 -> 0 (staged);
    resample [0, 0, 2, 2] (identity pairs next to repeated sources); a swap of two cells inside member 1; the rotation again
    with VICGPU_COPY_STAGE_MB=0 (one row per pass), which gives the bits of the rotation.  SD / SI / FX and every other table
    right after the copy, queued behind a step; then two records of three steps on both models: SD, SI, FX, the records, the
    flags, CA, CO, balance."""
    out = _check(plain_lib, "patterns")
    assert out.count("differing: none") == 5, out


def test_frozen_soil_chunks_pairs_across_the_boundary(plain_lib):
    """FROZEN_SOIL, 10 nodes, 2 bands, glacier HRUs, 5 base cells x 2 members as two chunks (VICGPU_CHUNKS=2); a direct and a
    staged call whose pairs cross the chunk boundary, issued right behind a two-step vicgpu_step that was not waited for."""
    _check(plain_lib, "frozen")


def test_continuation_is_indistinguishable(plain_lib):
    """copy_cells(member 1 <- member 0, STATE | BALANCE) at a record boundary: vicgpu_get_balance columns of member 1 equal
    member 0's and every later record of member 1 through vicgpu_run_records, all variables, equals member 0's bit for bit; the
    records before differed.  With STATE alone the PB columns of member 1 stay as they were."""
    _check(plain_lib, "continuation")


def test_untouched_tables_and_cells(plain_lib):
    _check(plain_lib, "untouched")


def test_error_returns_leave_every_table_as_it_was(plain_lib):
    out = _check(plain_lib, "errors")
    m = re.search(r"copy cells errors: (\d+) checks, failed: 0", out)
    assert m and int(m.group(1)) >= 35, out


def test_refused_allocations_leave_nothing_behind(plain_lib):
    out = _check(plain_lib, "refusals")
    assert "1 + 2 refused" in out, out


def test_group_of_three_shards_equals_one_context(plain_lib):
    """Three shards on device 0 over the 140 cells (bounds 47 and 94: every member pair crosses a shard boundary), fan-out,
    rotation and resample with STATE | BALANCE: every table equal to one context's, and a record after."""
    out = _check(plain_lib, "group")
    assert out.count("differing: none") == 3, out


def test_planner_and_kernels_clean_under_sanitizers(tmp_path):
    """tools/hostemu/copy_cells_check.cpp: its own main, ASan + UBSan, no preload."""
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ with sanitizer runtimes")
    exe = str(tmp_path / "copy_cells_check")
    cmd = [CLANG, "-x", "c++", "-std=c++17", "-O0", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-ffp-contract=off", "-ftrivial-auto-var-init=zero", "-Wno-unknown-attributes", "-Wno-ignored-attributes",
           "-I" + os.path.join(ROOT, "tools", "hostemu"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "vic_amd", "csrc"), os.path.join(ROOT, "tools", "hostemu", "copy_cells_check.cpp"),
           "-o", exe, "-lpthread"]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    p = subprocess.run([exe], env=env, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    report = [l for l in p.stderr.splitlines() if "runtime error" in l or "ERROR: " in l]
    assert not report, "\n".join(report[:10])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "copy_cells_check: all checks held" in p.stdout and p.stdout.count("direct") == 2 and p.stdout.count("staged") == 2, p.stdout
