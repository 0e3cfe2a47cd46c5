"""The device group (include/vicgpu_group.h) under AddressSanitizer + UBSan, on the CPU: tools/hostemu builds the library as
host C++ (see tests/test_hostemu_sanitizers.py) and tools/hostemu/check_group.py drives a 3-shard group on device 0 beside
one context on the same domain.  The group's host threads, its split / merge of the per-HRU tables and its pitched copies of
shard columns (from pinned memory as well as through the staging area) all run under the sanitizers."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tools", "hostemu", "build.sh")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def hostemu_lib():
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ with sanitizer runtimes")
    subprocess.check_call(["bash", BUILD], stdout=subprocess.DEVNULL)
    rt = subprocess.check_output(["bash", BUILD, "--asan-runtime"], text=True).strip()
    return os.path.join(ROOT, "tools", "hostemu", "libvicgpu_hostemu.so"), rt


def _run(lib, rt, args, poison):
    env = dict(os.environ, LD_PRELOAD=rt, VICGPU_LIB=lib, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", HOSTEMU_POISON="1" if poison else "0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hostemu", "check_group.py")] + args, env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1200)
    report = [l for l in p.stderr.splitlines() if "runtime error" in l or "ERROR: AddressSanitizer" in l]
    assert not report, "\n".join(report[:10])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


@pytest.mark.parametrize("poison", [True])     # the poisoned run checks everything the plain one does
def test_group_equals_one_context_bit_for_bit(hostemu_lib, poison):
    """QUICK_FLUX and FROZEN_SOIL + glacier, 7 cells in ragged shards of 3 / 2 / 2: outputs with reset, state tables, state
    records (read back, and a mismatching one refused with nothing scattered), cell error flags, balance, glacier fit."""
    out = _run(*hostemu_lib, ["run", "7", "3", "quickflux_melt", "glacier_frozen"], poison)
    assert out.count("differing: none") == 2, out


def test_refused_group_leaves_nothing_behind(hostemu_lib):
    """An option vicgpu_create refuses (IMPLICIT with QUICK_FLUX) and a device out of range return their codes with no runtime
    object and no host thread left; a group that is closed joins its shard threads and frees everything."""
    out = _run(*hostemu_lib, ["refuse"], False)
    assert out.count("left behind: 0 objects, 0 threads") == 4, out
