"""vicgpu_set_domain on the GPU: what it leaves in the tables it does not upload, and what it refuses.

The tables of the model state, the fluxes, the per-cell outputs, the accumulators and the error flags start as zero: the
fills are queued on the context's stream and waited for once, so the read-backs right after the call must see every one of
them.  A malformed domain (the variants of tools/hostemu/host_layer_check.cpp, on the lists of a real domain) is refused with
VICGPU_ERR_ARG by the single context and by a group, and the handle computes afterwards what a fresh one computes.
Shapes: 70 cells x 2 tiles x 2 bands in two chunks of 35 cells (less than a wave per slot: ragged last waves), and 6 cells.
"""
import copy

import numpy as np
import pytest

from vic_amd.abi import C
from tests.test_gpu_parity import CASES, _setup

pytestmark = pytest.mark.gpu

ERR_ARG = "(%d)" % C["VICGPU_ERR_ARG"]


def _read_all(m):
    """Every table vicgpu_set_domain fills, read into host arrays that hold no zero before the call."""
    from vic_amd import abi
    from vic_amd.api import _d, _i
    nn, nhru, ncell = m.opt.Nnode, m.dom.nhru, m.dom.ncell
    sd, si = np.full((abi.sd_nrow(nn), nhru), np.nan), np.full((abi.si_nrow(nn), nhru), -7, dtype=np.int32)
    fx, co, ac = np.full((C["FX_NROW"], nhru), np.nan), np.full((C["CO_NROW"], ncell), np.nan), np.full((C["CA_NROW"], ncell), np.nan)
    ce = np.full(ncell, -7, dtype=np.int32)
    m._chk(m.lib.vicgpu_get_state(m.h, _d(sd), _i(si)))
    m._chk(m.lib.vicgpu_get_fluxes(m.h, _d(fx)))
    m._chk(m.lib.vicgpu_get_cell_outputs(m.h, _d(co)))
    m._chk(m.lib.vicgpu_get_accum(m.h, _d(ac)))
    m._chk(m.lib.vicgpu_get_cell_errors(m.h, _i(ce)))
    return dict(sd=sd, si=si, flux=fx, cell_out=co, accum=ac, cell_err=ce)


@pytest.mark.parametrize("case,ncell", [("glacier_frozen", 70), ("quickflux_winter", 6)])
def test_fresh_domain_reads_back_zero(monkeypatch, case, ncell):
    from vic_amd.api import Model
    monkeypatch.setenv("VICGPU_CHUNKS", "2")
    kw, _, ntile, doy = CASES[case]
    d = _setup(kw, ncell, ntile, 1, doy)[0]
    m = Model(d)
    for name, a in _read_all(m).items():
        assert a.size > 0 and not a.any(), "%s: %d of %d words are not zero right after set_domain" % (name, np.count_nonzero(a), a.size)
    m.close()


def _malformed(d):
    """{name: domain}: d with one flaw in its lists or per-HRU indices."""
    nhru, nslot = d.nhru, d.nhru // d.ncell
    assert d.cell_hru_offset[1] == nslot >= 2

    def variant(off=None, lst=None, hpi=None):
        v = copy.copy(d)
        v.cell_hru_offset, v.cell_hru_list, v.hru_iparams = d.cell_hru_offset.copy(), d.cell_hru_list.copy(), d.hru_iparams.copy()
        for arr, edits in ((v.cell_hru_offset, off), (v.cell_hru_list, lst), (v.hru_iparams, hpi)):
            for k, val in (edits or {}).items():
                arr[k] = val
        return v
    lst = d.cell_hru_list
    return {
        "first offset non-zero": variant(off={0: 1}),
        "offset decreases": variant(off={2: d.cell_hru_offset[1] - 1}),
        "last offset is not nhru": variant(off={d.ncell: nhru - 1}),
        "list entry -1": variant(lst={nslot + 1: -1}),
        "list entry nhru": variant(lst={nslot + 1: nhru}),
        "entry listed twice": variant(lst={nslot + 1: lst[nslot]}),                       # twice under its own cell
        "HRU under another cell": variant(lst={0: lst[nslot], nslot: lst[0]}),            # cells 0 and 1 swap an HRU
        "HRU never listed": variant(lst={nhru - 1: lst[0]}),                              # its place names one of cell 0
        "band = Nband": variant(hpi={(C["HPI_BAND"], 3): d.opt.Nband}),
        "vegetation index = nveg_types + 4": variant(hpi={(C["HPI_VEG_INDEX"], 3): d.opt.nveg_types + 4}),
    }


def test_malformed_domains_are_refused_and_the_handle_survives(monkeypatch):
    from vic_amd.api import Group, Model, VicGpuError
    monkeypatch.setenv("VICGPU_CHUNKS", "2")
    kw, _, ntile, doy = CASES["glacier_frozen"]
    d, f, sf, dmy, sd0, si0 = _setup(kw, 6, ntile, 2, doy)

    def run(m):
        m.set_state(sd0, si0)
        m.push_forcing(f, sf, dmy)
        m.dist_prec(0, 2)
        return [*m.get_state(), m.get_fluxes(), m.get_cell_errors()]
    m = Model(d)
    want = run(m)                                  # the handle holds a stepped domain
    g = Group(d, devices=(0, 0))
    bad = _malformed(d)
    assert len(bad) == 10
    for name, v in bad.items():
        for handle in (m, g):
            with pytest.raises(VicGpuError) as e:
                handle.set_domain(v)
            assert ERR_ARG in str(e.value), "%s, %s: %s" % (name, type(handle).__name__, e.value)
    g.close()
    m.set_domain(d)
    got = run(m)
    fresh = run(Model(d))
    assert len(got) == len(want) == len(fresh) == 4
    for a, b, c in zip(fresh, got, want):
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(a, c, equal_nan=True)
