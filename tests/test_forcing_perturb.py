"""Shared raw forcing expanded and perturbed per column on the device (vicgpu_prefetch_forcing_perturbed and its group form,
include/vicgpu.h), on the CPU: the unsanitized host build of the library (tools/hostemu) runs
tools/hostemu/check_forcing_perturb.py in a child process.  The reference side of every comparison is the same library's
vicgpu_prefetch_forcing_raw on the ncol-wide table numpy builds as raw[..., col_src] * mul[..., col_group] + add[..., col_group],
and the oracle's derivation of that table; the comparisons are bit for bit (vp / vpd against the oracle to 1e-11).  The
kernels, the group's source ranges and the host pipeline are the library's own code; only the runtime underneath is the
emulation's (synchronous).  The argument check, which is free of HIP, also runs as a stand-alone program under ASan + UBSan
(tools/hostemu/forcing_perturb_check.cpp).  domain.member_perturbations is held to its contract here, without a library."""
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
CLANG = "/opt/rocm/lib/llvm/bin/clang++"          # CXX of tools/hostemu/build.sh
ENTRY = "prefetch_forcing_perturbed"
NSRC, M = 5, 3


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
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hostemu", "check_forcing_perturb.py")] + [str(a) for a in args], env=env,
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout


# ------------------------------------------------------------------------------------------------ host layer and generator
def test_headers_declare_and_libraries_export_the_entries(plain_lib):
    from vic_amd import api, build as vb
    vb.build(force=False)
    ctx_h = open(os.path.join(ROOT, "include", "vicgpu.h")).read()
    group_h = open(os.path.join(ROOT, "include", "vicgpu_group.h")).read()
    assert re.search(r"\bint\s+vicgpu_%s\s*\(" % ENTRY, ctx_h)
    assert re.search(r"\bint\s+vicgpu_group_%s\s*\(" % ENTRY, group_h)
    for macro in ("VICGPU_PERT_MUL(v)", "VICGPU_PERT_ADD(v)", "VICGPU_NPERT"):
        assert "#define " + macro in ctx_h, macro
    assert "vicgpu_" + ENTRY in api.EXPORTED_SYMBOLS and "vicgpu_group_" + ENTRY in api.EXPORTED_SYMBOLS and ENTRY in api.GROUP_ENTRIES
    assert callable(getattr(api.Model, ENTRY, None))
    for lib in (plain_lib, vb.OUT):
        syms = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
        for name in ("vicgpu_" + ENTRY, "vicgpu_group_" + ENTRY):
            assert re.search(r"\bT %s\b" % name, syms), "missing export %s in %s" % (name, lib)
    assert C["VICGPU_ABI_VERSION"] == 3
    assert C["VICGPU_NPERT"] == 2 * C["VIC_NRAW"]
    assert [abi.pert_mul(v) for v in range(C["VIC_NRAW"])] == list(range(0, C["VICGPU_NPERT"], 2))
    assert [abi.pert_add(v) for v in range(C["VIC_NRAW"])] == list(range(1, C["VICGPU_NPERT"], 2))


def test_null_handles_are_refused():
    """The gfx950 library itself (hipcc cross-compiles it, loading it needs no GPU)."""
    import ctypes
    from vic_amd import api, build as vb
    vb.build(force=False)
    lib = api.load_library()
    raw = (ctypes.c_double * C["VIC_NRAW"])()
    dmy = (ctypes.c_int * C["VIC_NDMY"])(1, 1, 0, 1, 2001)
    for pre in ("vicgpu_", "vicgpu_group_"):
        assert getattr(lib, pre + ENTRY)(None, 1, 1, raw, None, 0, None, None, dmy, 0.0, 1) == C["VICGPU_ERR_ARG"]


def test_the_new_kernels_use_no_scratch_and_are_policed():
    """The four instantiations are in the build's resource table with 0 B of scratch, the table passes the build's limits, and
    the limits name the kernel."""
    from vic_amd import build as vb
    vb.build(force=False)
    res = open(os.path.splitext(vb.OUT)[0] + ".resources.txt").read()
    rows = [tuple(re.split(r"\s{2,}", l.strip())) for l in res.splitlines()[1:]]
    mine = [r for r in rows if r[0].startswith("vic_derive_forcing_pert<")]
    assert sorted(r[0] for r in mine) == ["vic_derive_forcing_pert<%s, %s>" % (a, b) for a in ("false", "true") for b in ("false", "true")], mine
    for r in mine:
        assert int(r[4]) == 0 and int(r[5]) == 0 and int(r[1]) <= 128, r          # scratch bytes, VGPR spills, VGPRs
    assert vb.RESOURCE_LIMITS["vic_derive_forcing_pert"] == (128, 0)
    assert vb.check_resources(rows) == []
    assert {r[0] for r in rows} >= {"vic_derive_forcing", "vic_derive_forcing_cols", "vic_derive_forcing_flags"}


PREC, SW, T, LW = (C[v] for v in ("VIC_RAW_PREC", "VIC_RAW_SHORTWAVE", "VIC_RAW_AIR_TEMP", "VIC_RAW_LONGWAVE"))


def test_member_perturbations_rows_not_asked_for_are_the_identity():
    pert, state = domain.member_perturbations(4, 50, 1.0, {"VIC_RAW_PREC": 0.5, T: 2.0}, 24.0, seed=7)
    assert pert.shape == (50, C["VICGPU_NPERT"], 4) and pert.dtype == np.float64 and pert.flags["C_CONTIGUOUS"]
    touched = {abi.pert_mul(PREC), abi.pert_add(T)}
    for r in range(C["VICGPU_NPERT"]):
        if r in touched:
            assert len(np.unique(pert[:, r])) == pert[:, r].size, r      # different for every member at every step
        else:
            want = 1.0 if r % 2 == 0 else 0.0
            assert (pert[:, r] == want).all() and not np.signbit(pert[:, r]).any(), r
    assert (pert[:, abi.pert_mul(PREC)] > 0).all() and np.isfinite(pert).all()
    assert state["r"].shape == (4, 4)
    with pytest.raises(AssertionError):
        domain.member_perturbations(4, 5, 1.0, {"VIC_RAW_WIND": 0.1}, 24.0)


def test_member_perturbations_std_zero_is_the_identity():
    pert, _ = domain.member_perturbations(3, 20, 3.0, {PREC: 0.0, SW: 0.0, T: 0.0, LW: 0.0}, 6.0, seed=1)
    ident = np.zeros_like(pert); ident[:, 0::2] = 1.0
    assert np.array_equal(pert, ident) and not np.signbit(pert).any()


def test_member_perturbations_two_chunks_equal_one():
    std, tau = {PREC: 0.5, SW: 0.2, T: 2.0, LW: 10.0}, {PREC: 24.0, SW: 6.0, T: 48.0, LW: 12.0}
    whole, sw = domain.member_perturbations(5, 37, 1.0, std, tau, seed=20261020)
    a, st = domain.member_perturbations(5, 13, 1.0, std, tau, seed=20261020)
    b, sb = domain.member_perturbations(5, 24, 1.0, std, tau, state=st)
    assert np.array_equal(np.concatenate([a, b]), whole)
    assert np.array_equal(sb["r"], sw["r"])
    other, _ = domain.member_perturbations(5, 37, 1.0, std, tau, seed=1)
    assert not np.array_equal(other, whole)


def test_member_perturbations_ar1_and_unit_mean():
    """16 members x 20 000 hourly steps, tau = 24 h: the mean of the precipitation multipliers exp(sigma r - sigma^2 / 2) is 1
    within 5 standard errors, the standard error taken from the sample itself -- the members are independent series, so it is
    the spread of the 16 member means; and r has the lag-one correlation phi = exp(-1 / 24)."""
    sigma, Mm, n = 0.5, 16, 20000
    pert, _ = domain.member_perturbations(Mm, n, 1.0, {PREC: sigma, T: 1.0}, 24.0, seed=20261020)
    mul = pert[:, abi.pert_mul(PREC)]
    means = mul.mean(axis=0)
    se = means.std(ddof=1) / np.sqrt(Mm)
    print("mean %.6f, standard error %.6f" % (means.mean(), se))
    assert abs(means.mean() - 1.0) < 5 * se
    r = pert[:, abi.pert_add(T)]             # sigma 1: r itself
    phi = np.exp(-1.0 / 24.0)
    lag1 = np.mean([np.corrcoef(r[:-1, m], r[1:, m])[0, 1] for m in range(Mm)])
    # the estimate's standard error is about sqrt((1 - phi^2) / (n M)) = 5e-4
    assert abs(lag1 - phi) < 5 * np.sqrt((1 - phi * phi) / (n * Mm)) + 1e-3, (lag1, phi)
    assert abs(r.var() - 1.0) < 0.1


# ------------------------------------------------------------------------------------------------ the host build
def test_table_bit_for_bit_and_against_the_oracle(plain_lib, oracle_lib):
    """Comparisons 1 and 2 on 40 source columns x 3 members of identical parameters (dt = 24, snow_step = 3, 3 steps from day 60):
    the member-major lists, scrambled ones (repeats, an unused source, an unused group) and a group per column with col_group
    NULL; pert NULL with and without col_src; an explicit identity pert.  What keeps the case from passing empty is counted by
    the check and asserted here."""
    out = _check(plain_lib, ["table", 40, M])
    assert "missing: none; problems: none" in out and "'oracle': True" in out, out
    f = {k: int(v) for k, v in re.findall(r"'(\w+)': (\d+)", out)}
    assert f["flags_split"] >= 1 and f["vpd_newly_clipped"] >= 1 and f["prec_mul_zero"] >= 1, out
    assert f["wind_floored"] > f["wind_floored_unperturbed"] >= 1, out


def test_composes_with_a_forcing_map(plain_lib, oracle_lib):
    """120 cells -> 60 forcing columns (a scrambled forcing map) -> 20 sources, 3 groups of which one is unused; the members'
    parameters differ, so the flags are per cell."""
    out = _check(plain_lib, ["mapped"])
    m = re.search(r"flags apart within a column: (\d+), oracle: True, problems: none", out)
    assert m and int(m.group(1)) >= 1, out


@pytest.mark.parametrize("shape", ["daily", "hourly"])
def test_runs_equal_the_replicated_call_bit_for_bit(plain_lib, shape):
    out = _check(plain_lib, ["run", shape, NSRC, M])
    assert "members differ: True, clean run: True, differing: none" in out, out


def test_streamed_chunks_equal_one_chunk(plain_lib):
    out = _check(plain_lib, ["stream", NSRC, M])
    assert "clean run: True, differing: none" in out, out


def test_group_of_three_shards_equals_one_context(plain_lib):
    out = _check(plain_lib, ["group", NSRC, M, 3])
    assert out.count("differing: none") == 3 and "shards at [0, 5, 10, 15]" in out, out
    assert "member-major lists" in out and "scrambled lists" in out and "blocked lists" in out, out


def test_error_and_lifetime_returns(plain_lib):
    out = _check(plain_lib, ["errors"])
    m = re.search(r"forcing perturb errors: (\d+) checks, failed: 0", out)
    assert m and int(m.group(1)) >= 55, out


def test_refused_allocations_leave_nothing_behind(plain_lib):
    """Seven allocations into an empty slot (rows, flags, raw, factors, two lists, staging), seven into the other, five when a
    slot grows with the chunk length: each refused once, the count of live objects where it was, the chunk in force usable."""
    out = _check(plain_lib, ["refusals"])
    assert "[(7, 7), (7, 7), (5, 0)] refused / owned; problems: none" in out, out


def test_argument_check_clean_under_sanitizers(tmp_path):
    """tools/hostemu/forcing_perturb_check.cpp: check_forcing_perturbed of vic_checks.hpp (no HIP), its own main, ASan + UBSan, no
    preload; the lists sit in exact-size heap blocks, so a read past ncol or past pert's end is a report."""
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ with sanitizer runtimes")
    exe = str(tmp_path / "forcing_perturb_check")
    cmd = [CLANG, "-x", "c++", "-std=c++17", "-O0", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "vic_amd", "csrc"),
           os.path.join(ROOT, "tools", "hostemu", "forcing_perturb_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    env.pop("LD_PRELOAD", None)
    p = subprocess.run([exe], env=env, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    report = [l for l in p.stderr.splitlines() if "runtime error" in l or "ERROR: " in l]
    assert not report, "\n".join(report[:10])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "forcing_perturb_check: all checks held" in p.stdout, p.stdout
