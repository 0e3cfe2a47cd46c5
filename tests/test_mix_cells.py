"""Model state combined linearly across cells (vicgpu_mix_cells, include/vicgpu.h) on the CPU: the unsanitized host build of the
library (tools/hostemu) runs tools/hostemu/check_mix_cells.py in a child process.  The expected values are numpy's, written in
the contract's order (w0 * x0, then + w_t * x_t, every operation rounded once), and compared bit for bit, NaNs by position.
The planning of a call, the kernel and the host code are the library's own; only the runtime underneath is the emulation's
(synchronous).  The planning and the kernel also run as a stand-alone program under ASan + UBSan
(tools/hostemu/mix_cells_check.cpp).  domain.member_transform is held to a plain triple loop."""
import os
import re
import subprocess
import sys

import numpy as np
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
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hostemu", "check_mix_cells.py"), what], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "mix cells %s: problems: none" % what in p.stdout, p.stdout
    return p.stdout


# ------------------------------------------------------------------------------------------------ no library needed
def _triple_loop(M, ncol, W, cols):
    W = np.asarray(W)
    dst, off, tc, tw = [], [0], [], []
    for m in range(M):
        for j in (range(ncol) if cols is None else cols):
            dst.append(m * ncol + j)
            for mp in range(M):
                tc.append(mp * ncol + j)
                tw.append(W[mp, m] if W.ndim == 2 else W[j, mp, m])
            off.append(len(tc))
    return dst, off, tc, tw


@pytest.mark.parametrize("case", ["2-D", "3-D", "2-D cols", "3-D cols", "no column"])
def test_member_transform_against_a_triple_loop(case):
    from vic_amd import domain
    M, ncol = 3, 5
    rng = np.random.default_rng(1)
    W = rng.normal(size=(M, M) if case.startswith("2-D") else (ncol, M, M))
    cols = [4, 0, 2] if "cols" in case else [] if case == "no column" else None
    got = domain.member_transform(M, ncol, W, cols)
    want = _triple_loop(M, ncol, W, cols)
    assert [g.dtype for g in got] == [np.int32, np.int32, np.int32, np.float64]
    for g, w in zip(got, want):
        assert g.ndim == 1 and g.tolist() == list(w)
    with pytest.raises(AssertionError):
        domain.member_transform(M, ncol, np.zeros((M, M + 1)))
    with pytest.raises(AssertionError):
        domain.member_transform(M, ncol, W, [ncol])


def test_header_declares_and_libraries_export_the_entry(plain_lib):
    from vic_amd import api, build as vb
    vb.build(force=False)
    ctx_h = open(os.path.join(ROOT, "include", "vicgpu.h")).read()
    group_h = open(os.path.join(ROOT, "include", "vicgpu_group.h")).read()
    assert re.search(r"\bint\s+vicgpu_mix_cells\s*\(", ctx_h)
    assert "vicgpu_mix_cells" in group_h and not re.search(r"\bint\s+vicgpu_group_mix_cells\s*\(", group_h)      # named, no group form
    assert "vicgpu_mix_cells" in api.EXPORTED_SYMBOLS and "vicgpu_group_mix_cells" not in api.EXPORTED_SYMBOLS
    assert C["VICGPU_ABI_VERSION"] == 3
    assert callable(getattr(api.Model, "mix_cells", None))
    for lib in (plain_lib, vb.OUT):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
        assert re.search(r"\bT vicgpu_mix_cells\b", syms), "missing export vicgpu_mix_cells in %s" % lib
    res = open(os.path.splitext(vb.OUT)[0] + ".resources.txt").read()
    line = [l.split() for l in res.splitlines() if l.startswith("vic::vic_mix_cells")]
    assert len(line) == 1 and int(line[0][1]) <= 128 and int(line[0][4]) == 0, line           # VGPRs, scratch bytes
    assert any(k.endswith("vic_mix_cells") and v == (128, 0) for k, v in vb.RESOURCE_LIMITS.items())


def test_null_handle_is_refused():
    """The gfx950 library itself (hipcc cross-compiles it, loading it needs no GPU)."""
    import ctypes
    from vic_amd import api, build as vb
    vb.build(force=False)
    lib = api.load_library()
    one = (ctypes.c_int * 1)(0)
    off = (ctypes.c_int * 2)(0, 1)
    val = (ctypes.c_double * 1)(1.0)
    assert lib.vicgpu_mix_cells(None, 1, one, 1, one, off, one, val) == C["VICGPU_ERR_ARG"]
    assert lib.vicgpu_mix_cells(None, 0, None, 0, None, None, None, None) == C["VICGPU_ERR_ARG"]


# ------------------------------------------------------------------------------------------------ the host build
def test_dense_member_transform_bit_for_bit(plain_lib):
    """140 cells of 6 or 9 HRUs, 924 HRUs; a random 4 x 4 W on 11 rows (two row tiles); the default stage and one row per pass."""
    _check(plain_lib, "dense")


def test_per_column_transform(plain_lib):
    _check(plain_lib, "percolumn")


def test_irregular_terms_and_simultaneity(plain_lib):
    """Shuffled destinations with 1, 2, 3 and 65 terms; a destination that is a term of itself; two that are terms of each
    other; two nine-HRU cells of one member."""
    _check(plain_lib, "irregular")


def test_special_values_and_weight_one_equals_copy_cells(plain_lib):
    _check(plain_lib, "special")


def test_untouched_tables_rows_and_columns(plain_lib):
    _check(plain_lib, "untouched")


def test_mid_run_mix_in_the_finite_difference_pipeline(plain_lib):
    out = _check(plain_lib, "midrun")
    assert "midrun (chunks 1)" in out and "midrun (chunks 2)" in out, out


def test_error_returns_leave_every_table_as_it_was(plain_lib):
    out = _check(plain_lib, "errors")
    m = re.search(r"mix cells errors: (\d+) checks, failed: 0", out)
    assert m and int(m.group(1)) >= 70, out


def test_refused_allocations_leave_nothing_behind(plain_lib):
    out = _check(plain_lib, "refusals")
    assert "3 refused" in out, out


def test_plan_and_kernel_clean_under_sanitizers(tmp_path):
    """tools/hostemu/mix_cells_check.cpp: its own main, ASan + UBSan, no preload."""
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ with sanitizer runtimes")
    exe = str(tmp_path / "mix_cells_check")
    cmd = [CLANG, "-x", "c++", "-std=c++17", "-O0", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-ffp-contract=off", "-ftrivial-auto-var-init=zero", "-Wno-unknown-attributes", "-Wno-ignored-attributes",
           "-I" + os.path.join(ROOT, "tools", "hostemu"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "vic_amd", "csrc"), os.path.join(ROOT, "tools", "hostemu", "mix_cells_check.cpp"),
           "-o", exe, "-lpthread"]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    p = subprocess.run([exe], env=env, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    report = [l for l in p.stderr.splitlines() if "runtime error" in l or "ERROR: " in l]
    assert not report, "\n".join(report[:10])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "mix_cells_check: all checks held" in p.stdout, p.stdout
