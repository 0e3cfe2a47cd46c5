"""Cell validity (vicgpu_set_retire_on_error / vicgpu_set_cell_valid / vicgpu_get_cell_valid and their group forms,
include/vicgpu.h) on the CPU: what the reference driver does with cell.isValid and CONTINUEONERROR (vicNl.c:429, 521,
545-559).  The unsanitized host build of the library (tools/hostemu) runs tools/hostemu/check_cell_valid.py in a child
process on tiny domains: the kernels' validity tests, the three-state word between vic_cell_reduce and the put_data kernels,
the host pipeline and the group are the library's own code; only the runtime underneath is the emulation's."""
import os
import re
import subprocess
import sys

import pytest

from vic_amd.abi import C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tools", "hostemu", "build.sh")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
ENTRIES = ["set_retire_on_error", "set_cell_valid", "get_cell_valid"]


@pytest.fixture(scope="module")
def plain_lib(oracle_lib):
    if not os.path.exists(CLANG):
        pytest.skip("no host clang++")
    subprocess.check_call(["bash", BUILD], env=dict(os.environ, SAN="none"), stdout=subprocess.DEVNULL)
    return os.path.join(ROOT, "tools", "hostemu", "libvicgpu_hostemu_plain.so")


def _check(lib, case):
    env = dict(os.environ, VICGPU_LIB=lib)
    env.pop("LD_PRELOAD", None)
    env.pop("VICGPU_CHUNKS", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hostemu", "check_cell_valid.py"), case], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    m = re.search(r"cell validity %s: ok \((\d+)\)" % case, p.stdout)
    assert m, p.stdout
    return int(m.group(1))


def test_headers_declare_and_library_exports_the_entries(plain_lib):
    h = open(os.path.join(ROOT, "include", "vicgpu.h")).read()
    group_h = open(os.path.join(ROOT, "include", "vicgpu_group.h")).read()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", plain_lib]).decode()
    assert re.search(r"#define\s+VICGPU_CELLERR_REFERENCE\s+\(VICGPU_CELLERR_SOLVER \| VICGPU_CELLERR_AERO \| VICGPU_CELLERR_NODES\)", h)
    assert C["VICGPU_CELLERR_REFERENCE"] == 7 and C["VICGPU_ABI_VERSION"] == 3
    for e in ENTRIES:
        assert re.search(r"\bint\s+vicgpu_%s\s*\(" % e, h), e
        assert re.search(r"\bint\s+vicgpu_group_%s\s*\(" % e, group_h), e
        for name in ("vicgpu_" + e, "vicgpu_group_" + e):
            assert re.search(r"\bT %s\b" % name, syms), "missing export " + name


def test_null_handles_are_refused():
    """The gfx950 library itself (hipcc cross-compiles it, loading it needs no GPU): a null handle is an argument error."""
    from vic_amd import api, build as vb
    vb.build(force=False)
    lib = api.load_library()
    syms = subprocess.check_output(["nm", "-D", "--defined-only", vb.OUT]).decode()
    for e in ENTRIES:
        assert re.search(r"\bT vicgpu_%s\b" % e, syms) and re.search(r"\bT vicgpu_group_%s\b" % e, syms), e
    for pre in ("vicgpu_", "vicgpu_group_"):
        assert getattr(lib, pre + "set_retire_on_error")(None, 0) == C["VICGPU_ERR_ARG"]
        assert getattr(lib, pre + "set_cell_valid")(None, None) == C["VICGPU_ERR_ARG"]
        assert getattr(lib, pre + "get_cell_valid")(None, None) == C["VICGPU_ERR_ARG"]


@pytest.mark.parametrize("case", ["monolith", "frozen_chunks"])
def test_failed_cells_retire_on_the_device(plain_lib, case):
    """monolith: FULL_ENERGY, TFALLBACK = 0, 3 bands, 7 cells x 2 tiles.  frozen_chunks: FROZEN_SOIL, 10 nodes, 2 bands, 5 cells
    as two chunks.  Stress forcing at steps 5 and 12 on the cells c % 3 == 1 (the oracle flags exactly them at step 5), R = 4,
    4 records.  With the mask VICGPU_CELLERR_REFERENCE: bit-identical to mask 0 through step 5; from step 6 on the failed cells
    are invalid and every table column of theirs stays what it was after step 5 (CA_NSTEPS = 6), the other cells equal the run
    with mask 0; record 1 holds the aggregates of steps 4 and 5, records 2 and 3 are 0.0; one run_records call over all four
    records delivers the same records and flag words and leaves the same tables."""
    assert _check(plain_lib, case) == 2


def test_cells_the_host_marks_invalid(plain_lib):
    """7 cells, no stress, mask 0: the cells c % 5 == 0 are invalid before put_data_init.  After 8 steps their tables are the
    initial ones and their records 0.0, the others equal an all-valid run; valid again, they take the next step exactly as a
    fresh model started from their tables does."""
    assert _check(plain_lib, "host_validity") == 2


def test_group_of_three_shards(plain_lib):
    """3 shards over 7 cells against one context: validity table in the caller's cell order, records, final tables."""
    assert _check(plain_lib, "group") == 2


def test_error_returns(plain_lib):
    """VICGPU_ERR_ARG: null handle, null table, a mask with bits outside the four VICGPU_CELLERR_*.  VICGPU_ERR_STATE: the
    validity entries before a domain is set.  The mask survives vicgpu_set_domain, which makes every cell valid;
    vicgpu_set_state and vicgpu_reset_accum keep the table, vicgpu_reset_accum clears the flags."""
    assert _check(plain_lib, "errors") >= 30
