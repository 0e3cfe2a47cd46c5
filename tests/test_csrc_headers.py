"""Every header under vic_amd/csrc/ compiles on its own.

vicgpu_api.hip is the library's one translation unit and the code lives in the headers it includes.  A header that
only compiles at one position of that list (because it uses what another file happens to define above it) cannot be read,
moved or tested alone, so each one is compiled here as a translation unit of its own -- `#include "<header>"` and nothing
else -- by the two compilers the project uses: hipcc for gfx950 (host and device pass, the include paths of
vic_amd/build.py) and the host-emulation compiler of tools/hostemu/build.sh (its flags, no sanitizer).  Syntax only: nothing
is executed and no GPU is touched.
"""
import glob
import os
import subprocess

import pytest

from vic_amd import build as vb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vic_amd", "csrc")
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hpp")))
HOST_CLANG = "/opt/rocm/lib/llvm/bin/clang++"          # CXX of tools/hostemu/build.sh


def _syntax_only(cmd, tmp_path, header, suffix):
    tu = tmp_path / ("tu_" + os.path.splitext(header)[0] + suffix)
    tu.write_text('#include "%s"\n' % header)
    p = subprocess.run(cmd + [str(tu)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=str(tmp_path))
    assert p.returncode == 0, "%s does not compile on its own:\n%s" % (header, p.stdout[-4000:])


def test_headers_are_found():
    assert "vic_types.hpp" in HEADERS, "the glob above no longer finds the headers"


@pytest.mark.parametrize("header", HEADERS)
def test_header_stands_alone_hipcc(header, tmp_path):
    if not os.path.exists(vb.HIPCC):
        pytest.skip("no hipcc")
    includes = [f for f in vb.FLAGS if f.startswith("-I")]
    _syntax_only([vb.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only"] + includes, tmp_path, header, ".hip")


@pytest.mark.parametrize("header", HEADERS)
def test_header_stands_alone_hostemu(header, tmp_path):
    if not os.path.exists(HOST_CLANG):
        pytest.skip("no host clang++")
    cmd = [HOST_CLANG, "-x", "c++", "-std=c++17", "-fsyntax-only", "-ffp-contract=off", "-ftrivial-auto-var-init=zero",
           "-Wno-unknown-attributes", "-Wno-ignored-attributes",
           "-I" + os.path.join(ROOT, "tools", "hostemu"), "-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    _syntax_only(cmd, tmp_path, header, ".cpp")
