"""The device group (include/vicgpu_group.h) through the sanitizer build of the library, against one context on the same domain.
Run by tests/test_group_hostemu.py with the ASan runtime preloaded and VICGPU_LIB pointing at the host build:
    python tools/hostemu/check_group.py run <ncell> <nsteps> <case> [<case> ...]
        a 3-shard group on device 0 and one context step the same domain; outputs (with reset), state tables, state
        records, cell error flags, balance and glacier-fit equations must be bit-identical
    python tools/hostemu/check_group.py refuse
        group creations that must fail (an option vicgpu_create refuses, a device out of range) return their codes and leave
        no runtime object and no thread behind; so does a group that is created, given a domain and destroyed"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
from vic_amd import abi, domain, init_state
from vic_amd.abi import C
from vic_amd.api import Group, Model, VicGpuError, load_library

CASES = {
    # name: option overrides, tiles, start day, glacier top band
    "quickflux_melt": (dict(FULL_ENERGY=1), 3, 80, False),
    "glacier_frozen": (dict(FULL_ENERGY=1, FROZEN_SOIL=1, Nnode=10, Nband=2, frozen_compat=0), 2, 120, True),
}
OUT = ["OUT_RUNOFF", "OUT_BASEFLOW", "OUT_SWE", "OUT_SOIL_MOIST", "OUT_EVAP", "OUT_GLAC_MBAL", "OUT_SOIL_TNODE"]


def _setup(name, ncell, nsteps):
    kw, ntile, doy, glacier = CASES[name]
    opt = abi.default_options(**kw)
    # with artificial bare-soil HRUs (read_vegparam.c:312-340): they take the last slots of the HRU numbering
    d = domain.make_domain(ncell, opt, ntile=ntile, glacier_top_band=glacier, bare_fraction=0.2)
    f, sf, dmy = domain.make_forcing(d, 0, nsteps, start_doy=doy)
    sd0, si0 = init_state.initial_state(d, f[0])
    if glacier:
        sd0[C["SD_GLAC_CUM_MASS_BALANCE"], d.hru_iparams[C["HPI_IS_GLACIER"]] != 0] = 0.0
    return d, f, sf, dmy, sd0, si0


def _run(m, d, f, sf, dmy, sd0, si0):
    """One sequence on a Model or a Group: forcing from pinned memory, two step calls, put_data, every read-back."""
    nsteps = f.shape[0]
    m.set_state(sd0, si0)
    m.put_data_config(nsteps)
    m.put_data_init()
    fp = m.pinned(f.shape); fp[:] = f
    m.push_forcing(fp, sf, dmy)
    m.dist_prec(0, 1)
    m.dist_prec(1, nsteps - 1)
    r = dict(out=m.get_outputs(OUT, reset=True), out_after_reset=m.get_outputs(OUT, reset=False))
    r["sd"], r["si"] = m.get_state()
    r["flux"] = m.get_fluxes()
    r["records"] = m.get_state_records()
    r["errors"] = m.get_cell_errors()
    r["balance"] = m.get_balance()
    r["fit"] = m.glacier_mass_balance_fit(reset=True)
    r["sd_after_fit"] = m.get_state()[0]
    # the records read back in change nothing; a record with the wrong band is refused and scatters nothing
    m.set_state_records(r["records"])
    r["sd_after_records"] = m.get_state()[0]
    bad = r["records"].copy()
    bad[-1, C["SR_BAND_INDEX"]] += 1
    try:
        m.set_state_records(bad)
        r["refused"] = False
    except VicGpuError as e:
        r["refused"] = "state record %d" % (d.nhru - 1) in str(e)
    r["sd_after_refused"] = m.get_state()[0]
    return r


def run(ncell, nsteps, names):
    rc = 0
    for name in names:
        d, f, sf, dmy, sd0, si0 = _setup(name, ncell, nsteps)
        one = _run(Model(d), d, f, sf, dmy, sd0, si0)
        g = Group(d, devices=[0, 0, 0])
        b = g.shard_bounds()
        hru_per_shard = np.diff(d.cell_hru_offset[b])
        grp = _run(g, d, f, sf, dmy, sd0, si0)
        g.close()
        bad = [k for k in one if not np.array_equal(one[k], grp[k], equal_nan=True)]
        ragged = len(set(np.diff(b))) > 1 or len(set(hru_per_shard)) > 1
        if not one["refused"]:
            bad.append("refused")
        print("hostemu group %s: shards of %s cells (%s HRUs), %d tables, differing: %s"
              % (name, np.diff(b).tolist(), hru_per_shard.tolist(), len(one), bad or "none"), flush=True)
        if bad or not ragged or one["errors"].any():
            rc = 1
    return rc


def _threads():
    return len(os.listdir("/proc/self/task"))


def refuse():
    lib = load_library()
    lib.hostemu_live_objects.restype = ctypes.c_longlong
    live0, threads0 = lib.hostemu_live_objects(), _threads()
    rc = 0

    def create(opt, devices):
        h = ctypes.c_void_p()
        dev = np.asarray(devices, dtype=np.int32)
        r = lib.vicgpu_group_create(ctypes.byref(opt), len(dev), dev.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), ctypes.byref(h))
        return r, h.value
    cases = [
        ("IMPLICIT with QUICK_FLUX", abi.default_options(FULL_ENERGY=1, IMPLICIT=1), [0, 0, 0], C["VICGPU_ERR_UNSUPPORTED"]),
        ("device out of range", abi.default_options(FULL_ENERGY=1), [0, 0, 1], C["VICGPU_ERR_ARG"]),
        ("negative device", abi.default_options(FULL_ENERGY=1), [-1], C["VICGPU_ERR_ARG"]),
    ]
    for what, opt, devices, want in cases:
        single = ctypes.c_void_p()
        r1 = lib.vicgpu_create(ctypes.byref(opt), 0, ctypes.byref(single))
        if single.value:
            lib.vicgpu_destroy(single)
        r, h = create(opt, devices)
        same = (r == r1) if want == C["VICGPU_ERR_UNSUPPORTED"] else True
        left = lib.hostemu_live_objects() - live0, _threads() - threads0
        print("refused %s: code %d (want %d, vicgpu_create %d), left behind: %d objects, %d threads" % (what, r, want, r1, *left), flush=True)
        if r != want or h or not same or left != (0, 0):
            rc = 1
    # created, given a domain, destroyed: every object and every shard thread is gone
    d = domain.make_domain(5, abi.default_options(FULL_ENERGY=1), ntile=2)
    g = Group(d, devices=[0, 0])
    during = _threads() - threads0
    g.close()
    left = lib.hostemu_live_objects() - live0, _threads() - threads0
    print("group of 2 closed: %d shard threads while open, left behind: %d objects, %d threads" % (during, *left), flush=True)
    if during != 2 or left != (0, 0):
        rc = 1
    return rc


if __name__ == "__main__":
    if sys.argv[1] == "run":
        sys.exit(run(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4:]))
    sys.exit(refuse())
