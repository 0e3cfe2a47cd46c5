"""The kernel-free parts of the host layer under AddressSanitizer + UBSan, as a stand-alone program.

tools/hostemu/host_layer_check.cpp exercises the counted transfers of the buffer owners (vic_amd/csrc/vic_host.hpp: whole and
partial moves, refusal past size(), allocate-and-fill, the pitched download), the domain-list and state-record checks
(vic_checks.hpp) and the reading of the tuning variables, against the runtime stand-in tools/hostemu/hip/hip_runtime.h, where
device memory is malloc'ed.  An executable with the sanitizers linked in; no GPU is touched.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"          # CXX of tools/hostemu/build.sh


def test_host_layer_clean(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ with sanitizer runtimes")
    exe = str(tmp_path / "host_layer_check")
    cmd = [CLANG, "-x", "c++", "-std=c++17", "-O0", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-ffp-contract=off", "-ftrivial-auto-var-init=zero", "-Wno-unknown-attributes", "-Wno-ignored-attributes",
           "-I" + os.path.join(ROOT, "tools", "hostemu"), "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "vic_amd", "csrc"), os.path.join(ROOT, "tools", "hostemu", "host_layer_check.cpp"),
           "-o", exe, "-lpthread"]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], env=env, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    report = [l for l in p.stderr.splitlines() if "runtime error" in l or "Sanitizer" in l]
    assert not report, "\n".join(report[:10])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "host_layer_check: 0 problems" in p.stdout, p.stdout
