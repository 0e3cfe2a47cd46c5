"""The per-column ensemble transform solved and applied on the device (vicgpu_member_transform_solve / _set / _get / _apply,
include/vicgpu.h) on the CPU: the unsanitized host build of the library (tools/hostemu) runs
tools/hostemu/check_member_transform.py in a child process.  The apply is held to the library's own vicgpu_mix_cells with the
lists of domain.member_transform, bit for bit, NaNs by position; the solve to the header's formulas evaluated with mpmath at 50
digits and with numpy's eigh.  The checks, both kernels and the host code are the library's own; only the runtime underneath is
the emulation's (synchronous).  The checks and the kernels also run as a stand-alone program under ASan + UBSan
(tools/hostemu/member_transform_check.cpp)."""
import os
import re
import subprocess
import sys

import pytest

from vic_amd.abi import C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tools", "hostemu", "build.sh")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"          # CXX of tools/hostemu/build.sh
ENTRIES = ["vicgpu_member_transform_" + n for n in ("solve", "set", "get", "apply")]


@pytest.fixture(scope="module")
def plain_lib():
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++")
    subprocess.check_call(["bash", BUILD], env=dict(os.environ, SAN="none"), stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "tools", "hostemu", "libvicgpu_hostemu_plain.so")


def _check(lib, what):
    env = dict(os.environ, VICGPU_LIB=lib)
    for k in ("LD_PRELOAD", "VICGPU_CHUNKS", "VICGPU_COPY_STAGE_MB", "VICGPU_TRANSFORM_SWEEPS"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hostemu", "check_member_transform.py"), what], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "member transform %s: problems: none" % what in p.stdout, p.stdout
    return p.stdout


# ------------------------------------------------------------------------------------------------ the surface
def test_header_declares_and_libraries_export_the_entries(plain_lib):
    from vic_amd import api, build as vb
    vb.build(force=False)
    ctx_h = open(os.path.join(ROOT, "include", "vicgpu.h")).read()
    group_h = open(os.path.join(ROOT, "include", "vicgpu_group.h")).read()
    assert C["VICGPU_TRANSFORM_MAX_MEMBERS"] == 64 and C["VICGPU_ABI_VERSION"] == 3
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, ctx_h), name
        assert name in group_h and not re.search(r"\bint\s+%s\s*\(" % name.replace("vicgpu_", "vicgpu_group_"), group_h)      # named, no group form
        assert name in api.EXPORTED_SYMBOLS and name.replace("vicgpu_", "vicgpu_group_") not in api.EXPORTED_SYMBOLS
        assert callable(getattr(api.Model, name[len("vicgpu_"):], None))
        with pytest.raises(api.VicGpuError):
            getattr(api.Group, name[len("vicgpu_"):])(None)
        for lib in (plain_lib, vb.OUT):
            syms = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
            assert re.search(r"\bT %s\b" % name, syms), "missing export %s in %s" % (name, lib)
    res = [l.split() for l in open(os.path.splitext(vb.OUT)[0] + ".resources.txt").read().splitlines()]
    for prefix, count in (("vic::vic_member_transform_solve<", 4), ("vic::vic_member_transform_apply", 1), ("vic::vic_mix_cells", 1)):
        lines = [l for l in res if l and l[0].startswith(prefix)]
        assert len(lines) == count, (prefix, lines)
        limit = [v for k, v in vb.RESOURCE_LIMITS.items() if prefix.rstrip("<").startswith(k)]
        assert limit == [(128, 0)], (prefix, limit)
        for l in lines:
            assert int(l[-7]) <= 128 and int(l[-4]) == 0, l                  # VGPRs, scratch bytes


def test_null_handle_is_refused():
    """The gfx950 library itself (hipcc cross-compiles it, loading it needs no GPU)."""
    import importlib.util
    from vic_amd import build as vb
    vb.build(force=False)
    spec = importlib.util.spec_from_file_location("check_member_transform", os.path.join(ROOT, "tools", "hostemu", "check_member_transform.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    got = chk.null_handle_returns()
    assert len(got) == 6 and all(rc == want == C["VICGPU_ERR_ARG"] for _, rc, want in got), got


# ------------------------------------------------------------------------------------------------ the host build
def test_apply_equals_mix_cells_bit_for_bit(plain_lib):
    """4 members x 35 columns (924 HRUs: more than one wave, no multiple of 64), 16 x 9 and 64 x 2; 11 rows (two row tiles); the
    default stage and one row per pass; all columns and a shuffled subset; a random T and the T a solve leaves (get).  What a
    call must leave alone: unlisted rows and columns, the SI and FX tables, the flag words."""
    _check(plain_lib, "apply")


def test_solve_accuracy_against_mpmath_and_numpy(plain_lib):
    """Observation counts 0, 1, 3 and 40 per column, rinv from 1e-6 to 1e6 and exactly 0, infl 1 and 1.1.  Yardstick: the
    header's formulas with mpmath at 50 digits on columns of every observation count (8 of 35 at 4 members, 4 of 9 at 16, 1 of 2
    at 64); bound on max |T_dev - T_mp| = 16 x max(the deviation of numpy's eigh evaluation from the same mpmath values, 64 ulp of
    max |T|); the remaining columns against numpy with the same bound.  Every column of T sums to 1 within 4 M ulp of its
    largest entry.  Measured on the host build (the GPU's figures are in DESIGN.md (d)):
      members   numpy - mpmath   device - mpmath   device - numpy (rest)   bound      column sums
      4         7.9e-12          3.7e-12           2.9e-11                 1.3e-10    1.0 ulp of 16
      16        4.7e-11          3.9e-11           5.3e-11                 7.5e-10    4.0 ulp of 64
      64        1.2e-10          8.0e-11           -                       1.8e-09    2.0 ulp of 256
    The deviations are far above 1e-15 for both solvers because the columns with rinv = 1e6 next to 1e-6 are ill-conditioned in
    float64 whoever solves them: what is compared is the solver, not the conditioning."""
    out = _check(plain_lib, "accuracy")
    assert len(re.findall(r"member transform accuracy: \d+ members", out)) == 3, out


def test_guarantees_a_to_d(plain_lib):
    """(a) two runs, equal bits; (b) a column alone equals the column among others; (c) no observation or all rinv == 0: the
    exact closed form, with rho == 1 the exact identity, whose apply leaves the rows bit-identical; (d) with
    VICGPU_TRANSFORM_SWEEPS=1 the dense 16-member columns report -1 and hold exactly the identity while the diagonal columns of
    the same call converge."""
    _check(plain_lib, "guarantees")


def test_mid_run_apply_in_the_finite_difference_pipeline(plain_lib):
    out = _check(plain_lib, "midrun")
    assert "midrun (chunks 1)" in out and "midrun (chunks 2)" in out, out


def test_error_returns_leave_tables_and_transform_as_they_were(plain_lib):
    out = _check(plain_lib, "errors")
    m = re.search(r"member transform errors: (\d+) checks, failed: 0", out)
    assert m and int(m.group(1)) >= 40, out


def test_refused_allocations_leave_nothing_behind(plain_lib):
    out = _check(plain_lib, "refusals")
    assert "'apply': 2, 'set': 1, 'solve': 3" in out, out


def test_analysis_cycle_end_to_end_on_the_host_build(plain_lib):
    _check(plain_lib, "endtoend")


def test_checks_and_kernels_clean_under_sanitizers(tmp_path):
    """tools/hostemu/member_transform_check.cpp: its own main, ASan + UBSan, no preload."""
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ with sanitizer runtimes")
    exe = str(tmp_path / "member_transform_check")
    cmd = [CLANG, "-x", "c++", "-std=c++17", "-O0", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-ffp-contract=off", "-ftrivial-auto-var-init=zero", "-Wno-unknown-attributes", "-Wno-ignored-attributes",
           "-I" + os.path.join(ROOT, "tools", "hostemu"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "vic_amd", "csrc"), os.path.join(ROOT, "tools", "hostemu", "member_transform_check.cpp"),
           "-o", exe, "-lpthread"]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    p = subprocess.run([exe], env=env, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    report = [l for l in p.stderr.splitlines() if "runtime error" in l or "ERROR: " in l]
    assert not report, "\n".join(report[:10])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "member_transform_check: all checks held" in p.stdout, p.stdout
