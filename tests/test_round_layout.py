"""The layout of the two tables the rounds of the finite-difference pipeline exchange, under AddressSanitizer + UBSan.

vic_amd/csrc/vic_layout.hpp places the profile item blocks and the solution records on 64-byte sectors.
tools/hostemu/round_layout_check.cpp includes those accessors into a stand-alone host program and checks, for node counts
3, 5, 10, 11, 24, 25 and 50 with and without NOFLUX, on tables of exactly the allocated size: strides are multiples of 8
words; the accessors' ranges are disjoint and inside the stride; key, flag word, T1 and T2 of a record share its first
sector; the start column and the node records a solve reads form a contiguous prefix of the block.  An executable with
the sanitizers linked in; no GPU is touched.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"          # CXX of tools/hostemu/build.sh


def test_round_layout_clean(tmp_path):
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++ with sanitizer runtimes")
    exe = str(tmp_path / "round_layout_check")
    cmd = [CLANG, "-x", "c++", "-std=c++17", "-O0", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-Wno-unknown-attributes", "-Wno-ignored-attributes",
           "-I" + os.path.join(ROOT, "tools", "hostemu"), "-I" + os.path.join(ROOT, "vic_amd", "csrc"),
           os.path.join(ROOT, "tools", "hostemu", "round_layout_check.cpp"), "-o", exe, "-lpthread"]
    b = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    p = subprocess.run([exe], env=env, cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    report = [l for l in p.stderr.splitlines() if "runtime error" in l or "Sanitizer" in l]
    assert not report, "\n".join(report[:10])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "round_layout_check: 0 problems" in p.stdout, p.stdout
