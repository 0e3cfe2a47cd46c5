"""Cell and HRU parameters updated in place (vicgpu_update_cell_params / vicgpu_update_hru_params, the getters and their
group forms, include/vicgpu.h), on the CPU: the unsanitized host build of the library (tools/hostemu) runs
tools/hostemu/check_update_params.py in a child process.  The expected values come from a second model that takes the
updated tables through vicgpu_set_domain; every comparison is bit for bit.  The check of a call, the scatter and derive
kernels and the host code are the library's own; only the runtime underneath is the emulation's (synchronous).  The check and
the kernels also run as a stand-alone program under ASan + UBSan (tools/hostemu/update_params_check.cpp)."""
import os
import re
import subprocess
import sys

import pytest

from vic_amd.abi import C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tools", "hostemu", "build.sh")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"          # CXX of tools/hostemu/build.sh
ENTRIES = ("update_cell_params", "update_hru_params", "get_cell_params", "get_hru_params")


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
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hostemu", "check_update_params.py"), what], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "update params %s: problems: none" % what in p.stdout, p.stdout
    return p.stdout


def test_headers_declare_and_libraries_export_the_entries(plain_lib):
    from vic_amd import api, build as vb
    vb.build(force=False)
    ctx_h = open(os.path.join(ROOT, "include", "vicgpu.h")).read()
    group_h = open(os.path.join(ROOT, "include", "vicgpu_group.h")).read()
    for e in ENTRIES:
        assert re.search(r"\bint\s+vicgpu_%s\s*\(" % e, ctx_h), e
        assert re.search(r"\bint\s+vicgpu_group_%s\s*\(" % e, group_h), e
        assert "vicgpu_" + e in api.EXPORTED_SYMBOLS and "vicgpu_group_" + e in api.EXPORTED_SYMBOLS
    assert C["VICGPU_ABI_VERSION"] == 3
    for lib in (plain_lib, vb.OUT):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
        for e in ENTRIES:
            for name in ("vicgpu_" + e, "vicgpu_group_" + e):
                assert re.search(r"\bT %s\b" % name, syms), "missing export %s in %s" % (name, lib)


def test_null_handles_are_refused():
    """The gfx950 library itself (hipcc cross-compiles it, loading it needs no GPU)."""
    import ctypes
    from vic_amd import api, build as vb
    vb.build(force=False)
    lib = api.load_library()
    one = (ctypes.c_int * 1)(0)
    val = (ctypes.c_double * 1)(0.0)
    for fn in (lib.vicgpu_update_cell_params, lib.vicgpu_update_hru_params, lib.vicgpu_group_update_cell_params, lib.vicgpu_group_update_hru_params):
        assert fn(None, 1, one, 1, one, val) == C["VICGPU_ERR_ARG"]
        assert fn(None, 0, None, 0, None, None) == C["VICGPU_ERR_ARG"]
    for fn in (lib.vicgpu_get_cell_params, lib.vicgpu_get_hru_params, lib.vicgpu_group_get_cell_params, lib.vicgpu_group_get_hru_params):
        assert fn(None, val) == C["VICGPU_ERR_ARG"]


def test_update_before_the_run_equals_set_domain_bit_for_bit(plain_lib):
    """QUICK_FLUX, 3 bands, 35 base cells of 6 or 9 HRUs x 4 members on shared forcing columns.  Members 1 and 3 (70 cells)
    take new CP_B_INFILT, CP_DS, depths, CPL_MAX_MOIST, CPL_QUARTZ and CPL_BULK_DENSITY, member 1's HRUs new root fractions;
    then state, put_data and two records of three steps.  SD, SI, FX, CO, CA, flags, balance and the records of all variables
    equal those of a model that got the updated tables through vicgpu_set_domain; the records of members 1 and 3 differ from
    a run without the update, those of members 0 and 2 do not.  The listed form, the dense form over all rows, and the
    listed form with VICGPU_COPY_STAGE_MB=0 (one row per pass)."""
    out = _check(plain_lib, "start")
    assert out.count("differing: none") == 3, out


def test_derived_conductivity_rows_follow_the_soil_rows(plain_lib):
    """CPL_QUARTZ, the four density rows and CPL_ORGANIC of cell 0: VICGPU_PURE_SOIL_CONDUCTIVITY_DERIVED equals
    VICGPU_PURE_SOIL_CONDUCTIVITY fed with the new parameters and differs from its value before."""
    _check(plain_lib, "derived")


def test_tree_line_rows_follow_cv_and_abovetreeline(plain_lib):
    """CPB_ABOVETREELINE = 1 on the top band of a third of the cells, overstory HRUs in it.  HPD_CV of listed HRUs (the band's
    sum kept), then CPB_ABOVETREELINE of listed cells flipped; OUT_SWE, OUT_EVAP, OUT_SNOW_DEPTH_BAND against the set_domain
    path, the update before and after vicgpu_put_data_config."""
    out = _check(plain_lib, "treeline")
    assert out.count("differing: none") == 2, out


def test_mid_run_update_in_the_finite_difference_pipeline(plain_lib):
    """FROZEN_SOIL, 10 nodes, 2 bands, glacier HRUs, 5 base cells x 2 members as two chunks: cells on both sides of the chunk
    boundary updated right behind a two-step vicgpu_step that was not waited for."""
    _check(plain_lib, "midrun")


def test_untouched_tables_and_columns(plain_lib):
    _check(plain_lib, "untouched")


def test_error_returns_leave_every_table_as_it_was(plain_lib):
    out = _check(plain_lib, "errors")
    m = re.search(r"update params errors: (\d+) checks, failed: 0", out)
    assert m and int(m.group(1)) >= 140, out


def test_refused_allocations_leave_nothing_behind(plain_lib):
    out = _check(plain_lib, "refusals")
    assert "2 + 2 refused" in out, out


def test_group_of_three_shards_equals_one_context(plain_lib):
    _check(plain_lib, "group")


def test_check_and_kernels_clean_under_sanitizers(tmp_path):
    """tools/hostemu/update_params_check.cpp: its own main, ASan + UBSan, no preload."""
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ with sanitizer runtimes")
    exe = str(tmp_path / "update_params_check")
    cmd = [CLANG, "-x", "c++", "-std=c++17", "-O0", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-ffp-contract=off", "-ftrivial-auto-var-init=zero", "-Wno-unknown-attributes", "-Wno-ignored-attributes",
           "-I" + os.path.join(ROOT, "tools", "hostemu"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "vic_amd", "csrc"), os.path.join(ROOT, "tools", "hostemu", "update_params_check.cpp"),
           "-o", exe, "-lpthread"]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    p = subprocess.run([exe], env=env, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    report = [l for l in p.stderr.splitlines() if "runtime error" in l or "ERROR: " in l]
    assert not report, "\n".join(report[:10])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "update_params_check: all checks held" in p.stdout, p.stdout
