"""Model state read and changed in place, its dependent soil rows re-derived (vicgpu_get_state_rows / vicgpu_update_state /
vicgpu_derive_soil_state, the int forms and the group forms, include/vicgpu.h), on the CPU: the unsanitized host build of the
library (tools/hostemu) runs tools/hostemu/check_state_update.py in a child process.  The derive is held to the reference's
own tables (tests/golden/*.npz) and to the numpy restatement (vic_amd/init_state.py) at the 1e-12 that tests/test_domain.py
holds that restatement to; gather, scatter, the moisture cap, ordering, untouched tables and the group are compared bit for
bit.  The check of a call, the kernels and the host code are the library's own; only the runtime underneath is the
emulation's (synchronous).  The check and the kernels also run as a stand-alone program under ASan + UBSan
(tools/hostemu/state_update_check.cpp)."""
import os
import re
import subprocess
import sys

import pytest

from vic_amd.abi import C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tools", "hostemu", "build.sh")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"          # CXX of tools/hostemu/build.sh
ENTRIES = ("get_state_rows", "get_state_rows_i", "update_state", "update_state_i", "derive_soil_state")


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
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hostemu", "check_state_update.py"), what], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "state update %s: problems: none" % what in p.stdout, p.stdout
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
    assert (C["VICGPU_STATE_SET"], C["VICGPU_STATE_ADD"]) == (0, 1)
    assert [C["VICGPU_DERIVE_" + k] for k in ("CAP_MOIST", "NODES", "LAYERS", "FRONTS")] == [1, 2, 4, 8]
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
    ARG = C["VICGPU_ERR_ARG"]
    for p in ("vicgpu_", "vicgpu_group_"):
        f = lambda name: getattr(lib, p + name)
        assert f("get_state_rows")(None, 1, one, 1, one, val) == ARG and f("get_state_rows")(None, 0, None, 0, None, None) == ARG
        assert f("get_state_rows_i")(None, 1, one, 1, one, one) == ARG
        assert f("update_state")(None, 1, one, 1, one, val, C["VICGPU_STATE_ADD"]) == ARG and f("update_state")(None, 0, None, 0, None, None, 0) == ARG
        assert f("update_state_i")(None, 1, one, 1, one, one) == ARG
        assert f("derive_soil_state")(None, 1, one, C["VICGPU_DERIVE_NODES"]) == ARG and f("derive_soil_state")(None, 0, None, 15) == ARG


def test_derive_reproduces_the_reference_initial_state(plain_lib):
    """Every fixture: sd0 / si0 (the reference's state after initialize_model_state) with the produced rows overwritten,
    derive(all, NODES | LAYERS | FRONTS): back to sd0 / si0 within 1e-12, integer rows exactly; the front depths against the
    numpy restatement.  3, 8, 10, 33, 36 and 50 nodes: all three instantiations."""
    out = _check(plain_lib, "initial")
    assert len(re.findall(r"state update initial \w+: Nnode", out)) >= 14, out


def test_derive_reproduces_the_reference_stepped_states(plain_lib):
    """Every FULL_ENERGY / FROZEN_SOIL fixture, every recorded step: the node blocks and SD_LAYER_T0..2 from the reference's
    stepped node temperatures and layer moistures, within 1e-12.  A synthetic 14-node, 3-band domain for the middle bound."""
    out = _check(plain_lib, "stepped")
    assert len(re.findall(r"state update stepped \w+: Nnode", out)) >= 13 and "n14 (synthetic" in out, out


def test_derive_nodes_after_steps_changes_nothing(plain_lib):
    out = _check(plain_lib, "selfcheck")
    assert "bit for bit: yes" in out, out


def test_cap_moist_bit_for_bit_and_refused_with_glacier_dynamics(plain_lib):
    _check(plain_lib, "cap")


def test_gather_and_scatter_bit_for_bit(plain_lib):
    """924 HRUs; a wave-aligned, a ragged, a permuted list and the dense form; get, SET, ADD and the int entries (INT_MIN, NaN,
    -0.0); the default stage and one row per pass; then SET through the device against the same edit through set_state over
    two records of three steps."""
    out = _check(plain_lib, "rows")
    assert out.count("differing: none") == 9, out


def test_mid_run_update_and_derive_in_the_finite_difference_pipeline(plain_lib):
    _check(plain_lib, "midrun")


def test_nodes_above_the_bottom_layer_flag_their_cell(plain_lib):
    _check(plain_lib, "errorpath")


def test_hrus_without_area_get_empty_node_blocks(plain_lib):
    _check(plain_lib, "zeroarea")


def test_untouched_tables_rows_and_columns(plain_lib):
    _check(plain_lib, "untouched")


def test_error_returns_leave_every_table_as_it_was(plain_lib):
    out = _check(plain_lib, "errors")
    m = re.search(r"state update errors: (\d+) checks, failed: 0", out)
    assert m and int(m.group(1)) >= 366, out


def test_refused_allocations_leave_nothing_behind(plain_lib):
    out = _check(plain_lib, "refusals")
    assert "2 + 2 + 2 + 2 + 1 refused" in out, out


def test_group_of_three_shards_equals_one_context(plain_lib):
    _check(plain_lib, "group")


def test_check_and_kernels_clean_under_sanitizers(tmp_path):
    """tools/hostemu/state_update_check.cpp: its own main, ASan + UBSan, no preload."""
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ with sanitizer runtimes")
    exe = str(tmp_path / "state_update_check")
    cmd = [CLANG, "-x", "c++", "-std=c++17", "-O0", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-ffp-contract=off", "-ftrivial-auto-var-init=zero", "-Wno-unknown-attributes", "-Wno-ignored-attributes",
           "-I" + os.path.join(ROOT, "tools", "hostemu"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "vic_amd", "csrc"), os.path.join(ROOT, "tools", "hostemu", "state_update_check.cpp"),
           "-o", exe, "-lpthread"]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    p = subprocess.run([exe], env=env, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    report = [l for l in p.stderr.splitlines() if "runtime error" in l or "ERROR: " in l]
    assert not report, "\n".join(report[:10])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "state_update_check: all checks held" in p.stdout, p.stdout
