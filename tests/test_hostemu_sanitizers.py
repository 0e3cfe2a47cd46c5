"""The device code under AddressSanitizer + UBSan.

GPU sanitizers are not available on the MI355X pool, so tools/hostemu compiles vic_amd/csrc/vicgpu_api.hip as host C++
(kernels as functions, one fiber per work-item, wave operations as rendezvous) with -fsanitize=address,undefined and the
parity scenarios run through it against the oracle.  A clean run means: no out-of-bounds access to the state tables or
to a kernel-local array, no signed overflow / bad shift / misaligned access, and -- with fresh device allocations
poisoned -- no read of a word the kernels never wrote.  The build is a checker only; see tools/hostemu/hip/hip_runtime.h.
"""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tools", "hostemu", "build.sh")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def hostemu_lib(oracle_lib):
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ with sanitizer runtimes")
    subprocess.check_call(["bash", BUILD], stdout=subprocess.DEVNULL)
    rt = subprocess.check_output(["bash", BUILD, "--asan-runtime"], text=True).strip()
    return os.path.join(ROOT, "tools", "hostemu", "libvicgpu_hostemu.so"), rt


def _run(lib, rt, args, poison, script="check.py", **extra_env):
    env = dict(os.environ, **extra_env, LD_PRELOAD=rt, VICGPU_LIB=lib, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", HOSTEMU_POISON="1" if poison else "0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hostemu", script)] + args, env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    report = [l for l in p.stderr.splitlines() if "runtime error" in l or "ERROR: AddressSanitizer" in l]
    assert not report, "\n".join(report[:10])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


@pytest.mark.parametrize("poison", [False, True])
def test_monolithic_kernel_clean(hostemu_lib, poison):
    """vic_hru_step (QUICK_FLUX, water balance, glacier HRUs, gauge correction) + vic_cell_reduce."""
    out = _run(*hostemu_lib, ["6", "4", "quickflux_melt", "bands", "waterbalance_daily", "glacier_summer", "corrprec_glacier"], poison)
    assert out.count("worst rel diff") == 5


@pytest.mark.parametrize("poison", [True])          # (the poisoned run checks everything the plain one does; one of them keeps the CPU suite short)
def test_fd_pipeline_clean(hostemu_lib, poison):
    """vic_fd_stage -> { vic_profile_solve_reg ; vic_surf_eval } rounds -> vic_fd_stage, work lists included."""
    out = _run(*hostemu_lib, ["3", "2", "frozen_fixed", "frozen_compat", "glacier_frozen"], poison)
    assert out.count("worst rel diff") == 3


def test_fd_pipeline_newton_and_generic_kernel_clean(hostemu_lib):
    """The Newton node solver (VICGPU_NODE_SOLVER=newton) in the register-resident 10-node kernel and in the generic one
    (8 nodes), and the sub-stepped water-balance case."""
    out = _run(*hostemu_lib, ["3", "2", "frozen_fixed", "frozen_wb_daily", "frozen_fixed_n8"], False, VICGPU_NODE_SOLVER="newton")
    assert out.count("worst rel diff") == 3


@pytest.mark.parametrize("poison", [True])
def test_round2_entry_points_clean(hostemu_lib, poison):
    """put_data (three kernels), state-file records (gather and scatter), forcing prefetch / swap with the on-device
    derivation of atmos[rec], and the IMPLICIT profile kernel with its explicit fall-back."""
    out = _run(*hostemu_lib, ["3"], poison, script="check_round2.py")
    assert out.count("worst rel diff") == 5


def test_node_root_battery_clean(hostemu_lib):
    """The frozen-node root battery of tests/test_node_root.py (tests/node_cases.py) through vicgpu_debug_node_root, both
    node-solver modes, against the arbitrary-precision reference: tools/hostemu/check_node_root.py exits non-zero on any
    violated bound."""
    out = _run(*hostemu_lib, [], False, script="check_node_root.py")
    assert out.count(" 0 violations;") == 2, out


def test_brent_battery_clean(hostemu_lib):
    """The Brent battery of tests/test_brent.py (tests/golden/brent_traces.npz) through vicgpu_debug_root_brent: Brent's
    replay bit for bit, BrentLean's up to its documented difference (tools/hostemu/check_brent.py)."""
    out = _run(*hostemu_lib, [], False, script="check_brent.py")
    assert out.count(" 0 problems") == 2, out


def test_lifecycle_leaves_nothing_behind(hostemu_lib):
    """Every runtime object the host layer creates has one owner (vic_amd/csrc/vic_host.hpp): per option set, the read-backs
    leave the object count alone, a second vicgpu_set_domain on the same handle computes what a fresh context does, and
    after close the count is back where it was before create (tools/hostemu/check_lifecycle.py)."""
    out = _run(*hostemu_lib, ["lifecycle"], False, script="check_lifecycle.py")
    assert out.count(" 0 left after close, second domain differs in: nothing") == 3, out
    assert "check_lifecycle lifecycle: 0 problems" in out, out


def test_refused_allocations_leave_nothing_behind(hostemu_lib):
    """Every entry point that allocates, with the n-th allocation refused for every n it makes: VICGPU_ERR_HIP, the object
    count where it was, and the first call that gets through computes what an undisturbed context computes."""
    out = _run(*hostemu_lib, ["refusals"], False, script="check_lifecycle.py")
    assert out.count(" refused, then through") == 13, out
    assert "check_lifecycle refusals: 0 problems" in out, out
