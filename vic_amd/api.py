"""Host-side binding of the C-ABI in include/vicgpu.h (libvicgpu.so, HIP/gfx950).

The method names mirror the reference driver's vocabulary for this path
(vicNl.c:390-654 runModel / dist_prec.c:8 dist_prec): a `Model` owns the domain
tables on one GPU, `push_forcing` replaces cell.atmos[rec], `dist_prec(rec0, n)`
advances every cell n records.  A `Group` (include/vicgpu_group.h) is the same
on several contexts at once: one domain cut into contiguous cell blocks, one
block per device, tables in the domain's global layout.  There is NO CPU
fallback: if the HIP library is missing or no GPU is visible, construction raises.
"""
import ctypes
import os

import numpy as np

from . import abi
from .abi import C

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvicgpu.so")

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int)
_up = ctypes.POINTER(ctypes.c_ubyte)

_lib = None


class VicGpuError(RuntimeError):
    pass


def load_library():
    """Loads libvicgpu.so and declares every entry point of include/vicgpu.h.  Raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("VICGPU_LIB", LIB_PATH)      # tuning: an alternative build of the same library (tools/ab.sh)
    if not os.path.exists(path):
        raise VicGpuError("HIP extension %s not built: run `python -c 'import __graft_entry__ as g; g.build()'`" % path)
    lib = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    sig = {
        "vicgpu_abi_version": (ctypes.c_int, []),
        "vicgpu_create": (ctypes.c_int, [ctypes.POINTER(abi.Options), ctypes.c_int, ctypes.POINTER(vp)]),
        "vicgpu_destroy": (None, [vp]),
        "vicgpu_last_error": (ctypes.c_char_p, [vp]),
        "vicgpu_set_veglib": (ctypes.c_int, [vp, ctypes.c_int, _dp]),
        "vicgpu_set_domain": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, _dp, _ip, _dp, _ip, _ip]),
        "vicgpu_set_state": (ctypes.c_int, [vp, _dp, _ip]),
        "vicgpu_get_state": (ctypes.c_int, [vp, _dp, _ip]),
        "vicgpu_push_forcing": (ctypes.c_int, [vp, ctypes.c_int, _dp, _up, _ip]),
        "vicgpu_step": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int]),
        "vicgpu_synchronize": (ctypes.c_int, [vp]),
        "vicgpu_get_fluxes": (ctypes.c_int, [vp, _dp]),
        "vicgpu_get_cell_outputs": (ctypes.c_int, [vp, _dp]),
        "vicgpu_get_accum": (ctypes.c_int, [vp, _dp]),
        "vicgpu_reset_accum": (ctypes.c_int, [vp]),
        "vicgpu_get_cell_errors": (ctypes.c_int, [vp, _ip]),
        "vicgpu_set_retire_on_error": (ctypes.c_int, [vp, ctypes.c_int]),
        "vicgpu_set_cell_valid": (ctypes.c_int, [vp, _ip]),
        "vicgpu_get_cell_valid": (ctypes.c_int, [vp, _ip]),
        "vicgpu_set_stream": (ctypes.c_int, [vp, vp]),
        "vicgpu_set_write_fluxes": (ctypes.c_int, [vp, ctypes.c_int]),
        "vicgpu_device_ptr": (vp, [vp, ctypes.c_int]),
        "vicgpu_last_kernel_ms": (ctypes.c_int, [vp, _dp, _ip]),
        "vicgpu_debug_pure": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, _dp, _dp]),
        "vicgpu_debug_node_root": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, _dp, _dp]),
        "vicgpu_debug_root_brent": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, _dp, _ip, _dp, _dp, _dp]),
        "vicgpu_glacier_mass_balance_fit": (ctypes.c_int, [vp, _dp, ctypes.c_int]),
        "vicgpu_prefetch_forcing": (ctypes.c_int, [vp, ctypes.c_int, _dp, _up, _ip]),
        "vicgpu_prefetch_forcing_raw": (ctypes.c_int, [vp, ctypes.c_int, _dp, _ip, ctypes.c_double, ctypes.c_int]),
        "vicgpu_prefetch_forcing_perturbed": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, _dp, _ip, ctypes.c_int, _ip, _dp, _ip,
                                                             ctypes.c_double, ctypes.c_int]),
        "vicgpu_swap_forcing": (ctypes.c_int, [vp]),
        "vicgpu_get_forcing": (ctypes.c_int, [vp, ctypes.c_int, _dp, _up]),
        "vicgpu_set_forcing_map": (ctypes.c_int, [vp, ctypes.c_int, _ip]),
        "vicgpu_get_forcing_map": (ctypes.c_int, [vp, _ip, _ip]),
        "vicgpu_copy_cells": (ctypes.c_int, [vp, ctypes.c_int, _ip, _ip, ctypes.c_int]),
        "vicgpu_update_cell_params": (ctypes.c_int, [vp, ctypes.c_int, _ip, ctypes.c_int, _ip, _dp]),
        "vicgpu_update_hru_params": (ctypes.c_int, [vp, ctypes.c_int, _ip, ctypes.c_int, _ip, _dp]),
        "vicgpu_get_cell_params": (ctypes.c_int, [vp, _dp]),
        "vicgpu_get_hru_params": (ctypes.c_int, [vp, _dp]),
        "vicgpu_get_state_rows": (ctypes.c_int, [vp, ctypes.c_int, _ip, ctypes.c_int, _ip, _dp]),
        "vicgpu_get_state_rows_i": (ctypes.c_int, [vp, ctypes.c_int, _ip, ctypes.c_int, _ip, _ip]),
        "vicgpu_update_state": (ctypes.c_int, [vp, ctypes.c_int, _ip, ctypes.c_int, _ip, _dp, ctypes.c_int]),
        "vicgpu_update_state_i": (ctypes.c_int, [vp, ctypes.c_int, _ip, ctypes.c_int, _ip, _ip]),
        "vicgpu_derive_soil_state": (ctypes.c_int, [vp, ctypes.c_int, _ip, ctypes.c_int]),
        "vicgpu_mix_cells": (ctypes.c_int, [vp, ctypes.c_int, _ip, ctypes.c_int, _ip, _ip, _ip, _dp]),
        "vicgpu_member_transform_solve": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, _ip, _dp, _dp, _dp, _dp, _ip]),
        "vicgpu_member_transform_set": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, _dp]),
        "vicgpu_member_transform_get": (ctypes.c_int, [vp, _ip, _ip, _dp]),
        "vicgpu_member_transform_apply": (ctypes.c_int, [vp, ctypes.c_int, _ip, ctypes.c_int, _ip]),
        "vicgpu_host_alloc": (vp, [ctypes.c_size_t]),
        "vicgpu_host_free": (None, [vp]),
        "vicgpu_get_state_records": (ctypes.c_int, [vp, _dp]),
        "vicgpu_set_state_records": (ctypes.c_int, [vp, _dp]),
        # include/vicgpu_out.h
        "vicgpu_out_nvar": (ctypes.c_int, []),
        "vicgpu_out_var_id": (ctypes.c_int, [ctypes.c_char_p]),
        "vicgpu_out_var_name": (ctypes.c_char_p, [ctypes.c_int]),
        "vicgpu_out_var_kind": (ctypes.c_int, [ctypes.c_int]),
        "vicgpu_out_var_agg": (ctypes.c_int, [ctypes.c_int]),
        "vicgpu_out_var_nelem": (ctypes.c_int, [ctypes.POINTER(abi.Options), ctypes.c_int]),
        "vicgpu_put_data_config": (ctypes.c_int, [vp, ctypes.c_int]),
        "vicgpu_put_data_init": (ctypes.c_int, [vp]),
        "vicgpu_get_outputs": (ctypes.c_int, [vp, ctypes.c_int, _ip, ctypes.POINTER(ctypes.c_float), ctypes.c_int]),
        "vicgpu_get_output_data": (ctypes.c_int, [vp, ctypes.c_int, _ip, ctypes.c_int, _dp]),
        "vicgpu_get_balance": (ctypes.c_int, [vp, _dp]),
        "vicgpu_set_fluxes": (ctypes.c_int, [vp, _dp]),
        "vicgpu_records_config": (ctypes.c_int, [vp, ctypes.c_int, _ip, ctypes.c_int]),
        "vicgpu_records_nrow": (ctypes.c_int, [vp]),
        "vicgpu_run_records": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float), _ip]),
        "vicgpu_records_wait": (ctypes.c_int, [vp, ctypes.c_int]),
        "vicgpu_records_set_groups": (ctypes.c_int, [vp, ctypes.c_int, _ip, _ip, _dp, ctypes.c_float]),
        "vicgpu_records_get_groups": (ctypes.c_int, [vp, _ip, _ip]),
        "vicgpu_records_ncol": (ctypes.c_int, [vp]),
        # include/vicgpu_group.h
        "vicgpu_group_partition": (ctypes.c_int, [ctypes.c_int, _ip, ctypes.c_int, _ip]),
        "vicgpu_group_create": (ctypes.c_int, [ctypes.POINTER(abi.Options), ctypes.c_int, _ip, ctypes.POINTER(vp)]),
        "vicgpu_group_destroy": (None, [vp]),
        "vicgpu_group_last_error": (ctypes.c_char_p, [vp]),
        "vicgpu_group_shard_bounds": (ctypes.c_int, [vp, _ip]),
        "vicgpu_group_shard_ctx": (vp, [vp, ctypes.c_int]),
        "vicgpu_group_set_veglib": (ctypes.c_int, [vp, ctypes.c_int, _dp]),
        "vicgpu_group_set_domain": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, _dp, _ip, _dp, _ip, _ip]),
        "vicgpu_group_set_state": (ctypes.c_int, [vp, _dp, _ip]),
        "vicgpu_group_get_state": (ctypes.c_int, [vp, _dp, _ip]),
        "vicgpu_group_set_fluxes": (ctypes.c_int, [vp, _dp]),
        "vicgpu_group_get_fluxes": (ctypes.c_int, [vp, _dp]),
        "vicgpu_group_push_forcing": (ctypes.c_int, [vp, ctypes.c_int, _dp, _up, _ip]),
        "vicgpu_group_prefetch_forcing": (ctypes.c_int, [vp, ctypes.c_int, _dp, _up, _ip]),
        "vicgpu_group_prefetch_forcing_raw": (ctypes.c_int, [vp, ctypes.c_int, _dp, _ip, ctypes.c_double, ctypes.c_int]),
        "vicgpu_group_prefetch_forcing_perturbed": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, _dp, _ip, ctypes.c_int, _ip, _dp, _ip,
                                                                   ctypes.c_double, ctypes.c_int]),
        "vicgpu_group_swap_forcing": (ctypes.c_int, [vp]),
        "vicgpu_group_set_forcing_map": (ctypes.c_int, [vp, ctypes.c_int, _ip]),
        "vicgpu_group_get_forcing_map": (ctypes.c_int, [vp, _ip, _ip]),
        "vicgpu_group_copy_cells": (ctypes.c_int, [vp, ctypes.c_int, _ip, _ip, ctypes.c_int]),
        "vicgpu_group_update_cell_params": (ctypes.c_int, [vp, ctypes.c_int, _ip, ctypes.c_int, _ip, _dp]),
        "vicgpu_group_update_hru_params": (ctypes.c_int, [vp, ctypes.c_int, _ip, ctypes.c_int, _ip, _dp]),
        "vicgpu_group_get_cell_params": (ctypes.c_int, [vp, _dp]),
        "vicgpu_group_get_hru_params": (ctypes.c_int, [vp, _dp]),
        "vicgpu_group_get_state_rows": (ctypes.c_int, [vp, ctypes.c_int, _ip, ctypes.c_int, _ip, _dp]),
        "vicgpu_group_get_state_rows_i": (ctypes.c_int, [vp, ctypes.c_int, _ip, ctypes.c_int, _ip, _ip]),
        "vicgpu_group_update_state": (ctypes.c_int, [vp, ctypes.c_int, _ip, ctypes.c_int, _ip, _dp, ctypes.c_int]),
        "vicgpu_group_update_state_i": (ctypes.c_int, [vp, ctypes.c_int, _ip, ctypes.c_int, _ip, _ip]),
        "vicgpu_group_derive_soil_state": (ctypes.c_int, [vp, ctypes.c_int, _ip, ctypes.c_int]),
        "vicgpu_group_step": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int]),
        "vicgpu_group_synchronize": (ctypes.c_int, [vp]),
        "vicgpu_group_put_data_config": (ctypes.c_int, [vp, ctypes.c_int]),
        "vicgpu_group_put_data_init": (ctypes.c_int, [vp]),
        "vicgpu_group_get_outputs": (ctypes.c_int, [vp, ctypes.c_int, _ip, ctypes.POINTER(ctypes.c_float), ctypes.c_int]),
        "vicgpu_group_get_balance": (ctypes.c_int, [vp, _dp]),
        "vicgpu_group_get_cell_errors": (ctypes.c_int, [vp, _ip]),
        "vicgpu_group_set_retire_on_error": (ctypes.c_int, [vp, ctypes.c_int]),
        "vicgpu_group_set_cell_valid": (ctypes.c_int, [vp, _ip]),
        "vicgpu_group_get_cell_valid": (ctypes.c_int, [vp, _ip]),
        "vicgpu_group_get_state_records": (ctypes.c_int, [vp, _dp]),
        "vicgpu_group_set_state_records": (ctypes.c_int, [vp, _dp]),
        "vicgpu_group_glacier_mass_balance_fit": (ctypes.c_int, [vp, _dp, ctypes.c_int]),
        "vicgpu_group_records_config": (ctypes.c_int, [vp, ctypes.c_int, _ip, ctypes.c_int]),
        "vicgpu_group_records_nrow": (ctypes.c_int, [vp]),
        "vicgpu_group_run_records": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_float), _ip]),
        "vicgpu_group_records_wait": (ctypes.c_int, [vp, ctypes.c_int]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name)   # AttributeError here = the library does not export a declared symbol
        f.restype = res
        f.argtypes = args
    if lib.vicgpu_abi_version() != C["VICGPU_ABI_VERSION"]:
        raise VicGpuError("ABI version mismatch between include/vicgpu.h and libvicgpu.so")
    _lib = lib
    return lib


# the entries of include/vicgpu_group.h that mirror a single-context entry: vicgpu_group_<name> for vicgpu_<name>
GROUP_ENTRIES = [
    "destroy", "last_error", "set_veglib", "set_domain", "set_state", "get_state", "set_fluxes", "get_fluxes", "push_forcing",
    "prefetch_forcing", "prefetch_forcing_raw", "prefetch_forcing_perturbed", "swap_forcing", "step", "synchronize", "put_data_config", "put_data_init",
    "get_outputs", "get_balance", "get_cell_errors", "get_state_records", "set_state_records", "glacier_mass_balance_fit",
    "records_config", "records_nrow", "run_records", "records_wait", "set_retire_on_error", "set_cell_valid", "get_cell_valid",
    "set_forcing_map", "get_forcing_map", "copy_cells", "update_cell_params", "update_hru_params", "get_cell_params", "get_hru_params",
    "get_state_rows", "get_state_rows_i", "update_state", "update_state_i", "derive_soil_state",
]

EXPORTED_SYMBOLS = [
    "vicgpu_abi_version", "vicgpu_create", "vicgpu_destroy", "vicgpu_last_error", "vicgpu_set_veglib", "vicgpu_set_domain",
    "vicgpu_set_state", "vicgpu_get_state", "vicgpu_push_forcing", "vicgpu_step", "vicgpu_synchronize", "vicgpu_get_fluxes",
    "vicgpu_get_cell_outputs", "vicgpu_get_accum", "vicgpu_reset_accum", "vicgpu_get_cell_errors", "vicgpu_set_stream",
    "vicgpu_set_write_fluxes", "vicgpu_device_ptr", "vicgpu_last_kernel_ms", "vicgpu_debug_pure",
    "vicgpu_debug_node_root", "vicgpu_debug_root_brent", "vicgpu_glacier_mass_balance_fit",
    "vicgpu_out_nvar", "vicgpu_out_var_id", "vicgpu_out_var_name", "vicgpu_out_var_kind", "vicgpu_out_var_agg", "vicgpu_out_var_nelem",
    "vicgpu_put_data_config", "vicgpu_put_data_init", "vicgpu_get_outputs", "vicgpu_get_output_data", "vicgpu_get_balance",
    "vicgpu_set_fluxes", "vicgpu_get_state_records", "vicgpu_set_state_records",
    "vicgpu_records_config", "vicgpu_records_nrow", "vicgpu_run_records", "vicgpu_records_wait",
    "vicgpu_records_set_groups", "vicgpu_records_get_groups", "vicgpu_records_ncol",
    "vicgpu_prefetch_forcing", "vicgpu_prefetch_forcing_raw", "vicgpu_prefetch_forcing_perturbed", "vicgpu_swap_forcing", "vicgpu_get_forcing", "vicgpu_host_alloc",
    "vicgpu_host_free", "vicgpu_set_retire_on_error", "vicgpu_set_cell_valid", "vicgpu_get_cell_valid",
    "vicgpu_set_forcing_map", "vicgpu_get_forcing_map", "vicgpu_copy_cells",
    "vicgpu_update_cell_params", "vicgpu_update_hru_params", "vicgpu_get_cell_params", "vicgpu_get_hru_params",
    "vicgpu_get_state_rows", "vicgpu_get_state_rows_i", "vicgpu_update_state", "vicgpu_update_state_i", "vicgpu_derive_soil_state",
    "vicgpu_mix_cells",
    "vicgpu_member_transform_solve", "vicgpu_member_transform_set", "vicgpu_member_transform_get", "vicgpu_member_transform_apply",
] +["vicgpu_group_" + n for n in GROUP_ENTRIES + ["partition", "create", "shard_bounds", "shard_ctx"]]


def _d(a):
    return a.ctypes.data_as(_dp)


def _i(a):
    return a.ctypes.data_as(_ip)


class Records:
    """The records of one Model.run_records call: `.out` float32 [nrecords][nrow][ncol] (ncol = Model.records_ncol(): the
    cells, or the cell groups of Model.records_set_groups) and `.errors` int32 [nrecords][ncell]
    (None unless asked for) over pinned memory that the copies land in while later records are still being computed.
    Record k may be read after `wait(k)`, everything after `wait()`.  The memory lives as long as this object."""

    def __init__(self, model, nrecords, nrow, errors, ncol=None):
        self._model = model          # keeps the library and the context alive while copies may be in flight
        self._lib = model.lib
        self._ptrs = []
        self.nrecords = nrecords
        self.out = self._pinned((nrecords, nrow, model.dom.ncell if ncol is None else ncol), np.float32)
        self.errors = self._pinned((nrecords, model.dom.ncell), np.int32) if errors else None

    def _pinned(self, shape, dtype):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = self._lib.vicgpu_host_alloc(n)
        if not p:
            raise VicGpuError("vicgpu_host_alloc(%d) failed" % n)
        self._ptrs.append(p)
        return np.frombuffer((ctypes.c_char * n).from_address(p), dtype=dtype).reshape(shape)

    def wait(self, k=None):
        """Blocks until record k (None: every record) is in `.out` / `.errors`."""
        m = self._model
        m._chk(m.lib.vicgpu_records_wait(m.h, -1 if k is None else int(k)))

    def __del__(self):
        try:
            m = self._model
            if self._ptrs and getattr(m, "h", None):
                m.lib.vicgpu_synchronize(m.h)       # no copy may still be writing into the memory
            for p in self._ptrs:
                self._lib.vicgpu_host_free(p)
            self._ptrs = []
        except Exception:
            pass


class Model:
    """One domain (or one rank's shard of it) resident on one GPU."""

    def __init__(self, dom, device=0):
        self.lib = load_library()
        self.dom = dom
        self.opt = dom.opt
        h = ctypes.c_void_p()
        rc = self.lib.vicgpu_create(ctypes.byref(dom.opt), device, ctypes.byref(h))
        if rc != 0:
            raise VicGpuError("vicgpu_create failed with code %d (no GPU, or unsupported options)" % rc)
        self.h = h
        self._chk(self.lib.vicgpu_set_veglib(h, dom.veglib.shape[0], _d(np.ascontiguousarray(dom.veglib))))
        self.set_domain(dom)

    def set_domain(self, dom):
        """vicgpu_set_domain: `dom` replaces the domain of this handle (its tables, state, outputs and forcing go with it;
        the vegetation library stays).  Same options as the domain the handle was created for."""
        self._chk(self.lib.vicgpu_set_domain(self.h, dom.ncell, dom.nhru, _d(dom.cell_params), _i(dom.hru_iparams),
                                             _d(dom.hru_dparams), _i(dom.cell_hru_offset), _i(dom.cell_hru_list)))
        self.dom = dom
        self.ncol = dom.ncell        # the forcing map of a fresh domain is the identity

    def _chk(self, rc):
        if rc != 0:
            msg = self.lib.vicgpu_last_error(self.h)
            raise VicGpuError("vicgpu call failed (%d): %s" % (rc, msg.decode() if msg else ""))

    def close(self):
        if getattr(self, "h", None):
            self.lib.vicgpu_destroy(self.h)
            self.h = None
            for p in getattr(self, "_pinned", []):
                self.lib.vicgpu_host_free(p)
            self._pinned = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- state (initialize_model_state result in / write_model_state content out)
    def set_state(self, sd, si):
        sd = np.ascontiguousarray(sd, dtype=np.float64)
        si = np.ascontiguousarray(si, dtype=np.int32)
        assert sd.shape == (abi.sd_nrow(self.opt.Nnode), self.dom.nhru), sd.shape
        assert si.shape == (abi.si_nrow(self.opt.Nnode), self.dom.nhru), si.shape
        self._chk(self.lib.vicgpu_set_state(self.h, _d(sd), _i(si)))

    def get_state(self):
        sd = np.zeros((abi.sd_nrow(self.opt.Nnode), self.dom.nhru))
        si = np.zeros((abi.si_nrow(self.opt.Nnode), self.dom.nhru), dtype=np.int32)
        self._chk(self.lib.vicgpu_get_state(self.h, _d(sd), _i(si)))
        return sd, si

    # ---- forcing chunk
    def push_forcing(self, forcing, snowflag, dmy):
        forcing = np.ascontiguousarray(forcing, dtype=np.float64)
        snowflag = np.ascontiguousarray(snowflag, dtype=np.uint8)
        dmy = np.ascontiguousarray(dmy, dtype=np.int32)
        n = forcing.shape[0]
        assert forcing.shape == (n, C["VIC_NFORCE"], self.opt.NR + 1, self.ncol), forcing.shape
        assert snowflag.shape == (n, self.opt.NR + 1, self.dom.ncell)
        assert dmy.shape == (n, C["VIC_NDMY"])
        self._hold = (forcing, snowflag, dmy)   # the H2D copy is asynchronous
        self._chk(self.lib.vicgpu_push_forcing(self.h, n, _d(forcing), snowflag.ctypes.data_as(_up), _i(dmy)))

    # ---- forcing streaming: the next chunk uploads while the steps of the current one run
    def prefetch_forcing(self, forcing, snowflag, dmy):
        forcing = np.ascontiguousarray(forcing, dtype=np.float64)
        snowflag = np.ascontiguousarray(snowflag, dtype=np.uint8)
        dmy = np.ascontiguousarray(dmy, dtype=np.int32)
        n = forcing.shape[0]
        assert forcing.shape == (n, C["VIC_NFORCE"], self.opt.NR + 1, self.ncol), forcing.shape
        assert snowflag.shape == (n, self.opt.NR + 1, self.dom.ncell)
        self._hold_next = (forcing, snowflag, dmy)   # pinned sources are read until swap_forcing returns
        self._chk(self.lib.vicgpu_prefetch_forcing(self.h, n, _d(forcing), snowflag.ctypes.data_as(_up), _i(dmy)))

    def prefetch_forcing_raw(self, raw, dmy, min_wind_speed=0.0, plapse=True):
        """Hourly raw forcing [nsteps][VIC_NRAW][dt][ncell] (kPa pressures): initialize_atmos.c's derivation runs on the device."""
        raw = np.ascontiguousarray(raw, dtype=np.float64)
        dmy = np.ascontiguousarray(dmy, dtype=np.int32)
        n = raw.shape[0]
        assert raw.shape == (n, C["VIC_NRAW"], self.opt.dt, self.ncol), raw.shape
        self._hold_next = (raw, dmy)
        self._chk(self.lib.vicgpu_prefetch_forcing_raw(self.h, n, _d(raw), _i(dmy), float(min_wind_speed), int(bool(plapse))))

    def prefetch_forcing_perturbed(self, raw, dmy, col_src=None, col_group=None, pert=None, min_wind_speed=0.0, plapse=True):
        """vicgpu_prefetch_forcing_perturbed: raw [nsteps][VIC_NRAW][dt][nsrc] shared source columns; forcing column i (of the
        ncol the forcing tables are wide) reads source col_src[i] (None: nsrc == ncol, its own) as x * mul + add with the
        factors pert [nsteps][VICGPU_NPERT][ngroup] (abi.pert_mul / abi.pert_add, domain.member_perturbations) of group
        col_group[i] (None: a group per column when pert is given); pert None: the values verbatim.  The derivation of
        prefetch_forcing_raw follows on the device.  The lists and pert are free on return, a pinned raw after swap_forcing."""
        raw = np.ascontiguousarray(raw, dtype=np.float64)
        dmy = np.ascontiguousarray(dmy, dtype=np.int32)
        n = raw.shape[0]
        assert raw.ndim == 4 and raw.shape[:3] == (n, C["VIC_NRAW"], self.opt.dt), raw.shape
        nsrc = raw.shape[3]
        src = None if col_src is None else np.ascontiguousarray(col_src, dtype=np.int32)
        grp = None if col_group is None else np.ascontiguousarray(col_group, dtype=np.int32)
        assert src is None or src.shape == (self.ncol,), src.shape
        assert grp is None or grp.shape == (self.ncol,), grp.shape
        ngroup = 0
        if pert is not None:
            pert = np.ascontiguousarray(pert, dtype=np.float64)
            assert pert.ndim == 3 and pert.shape[:2] == (n, C["VICGPU_NPERT"]), pert.shape
            ngroup = pert.shape[2]
        self._hold_next = (raw, dmy)
        self._chk(self.lib.vicgpu_prefetch_forcing_perturbed(self.h, n, nsrc, _d(raw), None if src is None else _i(src), ngroup,
                                                             None if grp is None else _i(grp), None if pert is None else _d(pert),
                                                             _i(dmy), float(min_wind_speed), int(bool(plapse))))

    def swap_forcing(self):
        self._chk(self.lib.vicgpu_swap_forcing(self.h))
        self._hold = getattr(self, "_hold_next", None)

    # ---- forcing map: cells that share forcing columns (ensembles, a model grid finer than its forcing grid)
    def set_forcing_map(self, cell_col, ncol=None):
        """vicgpu_set_forcing_map: cell c reads forcing column cell_col[c] of the ncol-wide forcing and raw tables (ncol None:
        max(cell_col) + 1); the snowflag stays [..][ncell].  cell_col None: every cell its own column again.  Drops the forcing
        chunks: push one before the next step."""
        if cell_col is None:
            self._chk(self.lib.vicgpu_set_forcing_map(self.h, 0, None))
            self.ncol = self.dom.ncell
            return
        m = np.ascontiguousarray(cell_col, dtype=np.int32)
        assert m.shape == (self.dom.ncell,), m.shape
        ncol = int(m.max()) + 1 if ncol is None else int(ncol)
        self._chk(self.lib.vicgpu_set_forcing_map(self.h, ncol, _i(m)))
        self.ncol = ncol

    def get_forcing_map(self):
        """(ncol, cell_col [ncell]) as the library holds it."""
        n = ctypes.c_int(0)
        m = np.zeros(self.dom.ncell, dtype=np.int32)
        self._chk(self.lib.vicgpu_get_forcing_map(self.h, ctypes.byref(n), _i(m)))
        return n.value, m

    # ---- model state copied between cells on the device (ensemble seeding, resampling, rollback)
    STATE, BALANCE = C["VICGPU_COPY_STATE"], C["VICGPU_COPY_BALANCE"]

    def copy_cells(self, dst, src, what=STATE):
        """vicgpu_copy_cells: cell dst[i] takes the state (STATE: every SD / SI / FX row of its HRUs, paired by position) and /
        or the balance bookkeeping (BALANCE: every PB row) of cell src[i]; simultaneous, so a permutation is legal; a source
        may repeat, a destination must not.  Queued behind the steps queued so far; synchronize() waits for it."""
        d = np.ascontiguousarray(dst, dtype=np.int32)
        s = np.ascontiguousarray(src, dtype=np.int32)
        assert d.ndim == 1 and d.shape == s.shape, (d.shape, s.shape)
        self._chk(self.lib.vicgpu_copy_cells(self.h, len(d), _i(d), _i(s), int(what)))

    # ---- cell and HRU parameters updated in place (calibration generations, sensitivity sweeps, glacier coupling)
    def _update_params(self, fn, table, rows, values, cols):
        r = np.ascontiguousarray(rows, dtype=np.int32)
        c = None if cols is None else np.ascontiguousarray(cols, dtype=np.int32)
        n = table.shape[1] if c is None else len(c)
        v = np.ascontiguousarray(values, dtype=np.float64)
        assert r.ndim == 1 and (c is None or c.ndim == 1) and v.shape == (len(r), n), (r.shape, v.shape, n)
        self._chk(fn(self.h, len(r), _i(r), n, None if c is None else _i(c), _d(v)))
        if r.size and n:             # the host tables follow only a call that got through
            if c is None:
                table[r] = v
            else:
                table[np.ix_(r, c)] = v

    def update_cell_params(self, rows, values, cells=None):
        """vicgpu_update_cell_params: values[k][i] -> row rows[k] of cell cells[i] (cells None: every cell, in order) of the
        cell parameter table, in place; the library re-derives its own rows for the listed cells.  State, forcing, put_data,
        records and groups stay.  Queued behind the steps queued so far.  `dom.cell_params` of this model follows."""
        self._update_params(self.lib.vicgpu_update_cell_params, self.dom.cell_params, rows, values, cells)

    def update_hru_params(self, rows, values, hrus=None):
        """vicgpu_update_hru_params: the same on the HPD_* rows of the HRU columns `hrus`.  `dom.hru_dparams` follows."""
        self._update_params(self.lib.vicgpu_update_hru_params, self.dom.hru_dparams, rows, values, hrus)

    def get_cell_params(self):
        """[cp_nrow][ncell]: the caller's rows of the cell parameter table as the library holds them."""
        cp = np.zeros((abi.cp_nrow(self.opt.Nnode, self.opt.Nband), self.dom.ncell))
        self._chk(self.lib.vicgpu_get_cell_params(self.h, _d(cp)))
        return cp

    def get_hru_params(self):
        hpd = np.zeros((C["HPD_NROW"], self.dom.nhru))
        self._chk(self.lib.vicgpu_get_hru_params(self.h, _d(hpd)))
        return hpd

    # ---- model state read and changed in place, its dependent soil rows re-derived (the analysis update of an ensemble loop)
    SET, ADD = C["VICGPU_STATE_SET"], C["VICGPU_STATE_ADD"]
    CAP_MOIST, NODES, LAYERS, FRONTS = (C["VICGPU_DERIVE_CAP_MOIST"], C["VICGPU_DERIVE_NODES"], C["VICGPU_DERIVE_LAYERS"],
                                        C["VICGPU_DERIVE_FRONTS"])

    def _state_lists(self, rows, hrus):
        r = np.ascontiguousarray(rows, dtype=np.int32)
        h = None if hrus is None else np.ascontiguousarray(hrus, dtype=np.int32)
        assert r.ndim == 1 and (h is None or h.ndim == 1), (r.shape, None if h is None else h.shape)
        return r, h, self.dom.nhru if h is None else len(h)

    def get_state_rows(self, rows, hrus=None, ints=False):
        """vicgpu_get_state_rows(_i): [len(rows)][n] -- row rows[k] of HRU hrus[i] (hrus None: every HRU, in order) of the SD
        table (ints: of the SI table).  Waits for everything queued before it."""
        r, h, n = self._state_lists(rows, hrus)
        v = np.zeros((len(r), n), dtype=np.int32 if ints else np.float64)
        fn = self.lib.vicgpu_get_state_rows_i if ints else self.lib.vicgpu_get_state_rows
        self._chk(fn(self.h, len(r), _i(r), n, None if h is None else _i(h), _i(v) if ints else _d(v)))
        return v

    def update_state(self, rows, values, hrus=None, mode=SET, ints=False):
        """vicgpu_update_state (ints: vicgpu_update_state_i): values[k][i] -> row rows[k] of HRU hrus[i] of the SD (SI) table,
        verbatim (SET) or added to what is there (ADD, SD only).  No other row follows: derive_soil_state."""
        r, h, n = self._state_lists(rows, hrus)
        v = np.ascontiguousarray(values, dtype=np.int32 if ints else np.float64)
        assert v.shape == (len(r), n), (v.shape, len(r), n)
        if ints:
            assert mode == self.SET, "the integer table takes SET only"
            self._chk(self.lib.vicgpu_update_state_i(self.h, len(r), _i(r), n, None if h is None else _i(h), _i(v)))
        else:
            self._chk(self.lib.vicgpu_update_state(self.h, len(r), _i(r), n, None if h is None else _i(h), _d(v), int(mode)))

    def derive_soil_state(self, what, hrus=None):
        """vicgpu_derive_soil_state: the stages `what` (CAP_MOIST | NODES | LAYERS | FRONTS) of the tail of
        initialize_model_state for the HRUs `hrus` (None: all), from the state and the parameters on the device."""
        h = None if hrus is None else np.ascontiguousarray(hrus, dtype=np.int32)
        assert h is None or h.ndim == 1
        self._chk(self.lib.vicgpu_derive_soil_state(self.h, self.dom.nhru if h is None else len(h), None if h is None else _i(h), int(what)))

    # ---- model state combined linearly across cells (the ensemble transform of a filter, inflation, recentring)
    def mix_cells(self, rows, dst_cells, term_off, term_cell, term_weight):
        """vicgpu_mix_cells: on the SD rows `rows`, cell dst_cells[i] becomes the sum over t in [term_off[i], term_off[i + 1]) of
        term_weight[t] * cell term_cell[t], HRUs paired by position, in list order (w0 * x0, then + w_t * x_t, each rounded once);
        simultaneous, so a destination may be a term of itself and of others.  domain.member_transform builds the lists of a
        member transform.  No other row follows: derive_soil_state.  Queued behind the steps queued so far."""
        r = np.ascontiguousarray(rows, dtype=np.int32)
        d = np.ascontiguousarray(dst_cells, dtype=np.int32)
        o = np.ascontiguousarray(term_off, dtype=np.int32)
        c = np.ascontiguousarray(term_cell, dtype=np.int32)
        w = np.ascontiguousarray(term_weight, dtype=np.float64)
        assert r.ndim == 1 and d.ndim == 1 and o.shape == (len(d) + 1,) and c.ndim == 1 and w.shape == c.shape, (r.shape, d.shape, o.shape, c.shape, w.shape)
        assert len(c) == o[-1], (len(c), int(o[-1]))
        self._chk(self.lib.vicgpu_mix_cells(self.h, len(r), _i(r), len(d), _i(d), _i(o), _i(c), _d(w)))

    # ---- the per-column ensemble transform of a localised filter, solved and applied on the device
    def member_transform_solve(self, nmember, obs_off, hx, yobs, rinv, infl=None):
        """vicgpu_member_transform_solve: the LETKF transform of every base column of the member-major ensemble (cell
        m * ncol + j is member m of column j) from hx [nobs][nmember], yobs [nobs] and rinv [nobs], column j owning the
        observations obs_off[j] .. obs_off[j + 1] - 1; infl [ncol] is the covariance inflation (default 1).  The transform stays
        on the device (member_transform_get reads it).  Returns info [ncol]: the sweeps a column took, or -1 where it did not
        converge and got the identity."""
        M = int(nmember)
        o = np.ascontiguousarray(obs_off, dtype=np.int32)
        assert o.ndim == 1 and len(o) >= 2, o.shape
        ncol, nobs = len(o) - 1, int(o[-1])
        h = np.ascontiguousarray(hx, dtype=np.float64)
        y = np.ascontiguousarray(yobs, dtype=np.float64)
        r = np.ascontiguousarray(rinv, dtype=np.float64)
        assert h.shape == (nobs, M) and y.shape == (nobs,) and r.shape == (nobs,), (h.shape, y.shape, r.shape, nobs, M)
        f = None if infl is None else np.ascontiguousarray(infl, dtype=np.float64)
        assert f is None or f.shape == (ncol,), f.shape
        info = np.zeros(ncol, dtype=np.int32)
        self._chk(self.lib.vicgpu_member_transform_solve(self.h, M, ncol, _i(o), _d(h), _d(y), _d(r), None if f is None else _d(f), _i(info)))
        return info

    def member_transform_set(self, T):
        """vicgpu_member_transform_set: stores T [ncol][nmember][nmember], T[j, m', m] as domain.member_transform's 3-D W."""
        T = np.ascontiguousarray(T, dtype=np.float64)
        assert T.ndim == 3 and T.shape[1] == T.shape[2], T.shape
        self._chk(self.lib.vicgpu_member_transform_set(self.h, T.shape[1], T.shape[0], _d(T)))

    def member_transform_get(self):
        """vicgpu_member_transform_get: the stored transform, [ncol][nmember][nmember]."""
        M, n = ctypes.c_int(0), ctypes.c_int(0)
        self._chk(self.lib.vicgpu_member_transform_get(self.h, ctypes.byref(M), ctypes.byref(n), None))
        T = np.zeros((n.value, M.value, M.value))
        self._chk(self.lib.vicgpu_member_transform_get(self.h, ctypes.byref(M), ctypes.byref(n), _d(T)))
        return T

    def member_transform_apply(self, rows, cols=None):
        """vicgpu_member_transform_apply: the stored transform on the SD rows `rows` of the base columns `cols` (default: all);
        bit for bit mix_cells(rows, *domain.member_transform(M, ncol, T, cols)).  No other row follows: derive_soil_state."""
        r = np.ascontiguousarray(rows, dtype=np.int32)
        assert r.ndim == 1, r.shape
        if cols is None:
            M, n = ctypes.c_int(0), ctypes.c_int(0)
            self._chk(self.lib.vicgpu_member_transform_get(self.h, ctypes.byref(M), ctypes.byref(n), None))
            self._chk(self.lib.vicgpu_member_transform_apply(self.h, len(r), _i(r), n.value, None))
        else:
            c = np.ascontiguousarray(cols, dtype=np.int32)
            assert c.ndim == 1, c.shape
            self._chk(self.lib.vicgpu_member_transform_apply(self.h, len(r), _i(r), len(c), _i(c)))

    def get_forcing(self, step):
        f = np.zeros((C["VIC_NFORCE"], self.opt.NR + 1, self.ncol)); sf = np.zeros((self.opt.NR + 1, self.dom.ncell), dtype=np.uint8)
        self._chk(self.lib.vicgpu_get_forcing(self.h, int(step), _d(f), sf.ctypes.data_as(_up)))
        return f, sf

    def pinned(self, shape, dtype=np.float64):
        """A numpy array over pinned host memory (vicgpu_host_alloc): forcing chunks in it are uploaded by DMA without a
        staging copy.  Freed when the Model is closed."""
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = self.lib.vicgpu_host_alloc(n)
        if not p:
            raise VicGpuError("vicgpu_host_alloc(%d) failed" % n)
        self._pinned = getattr(self, "_pinned", []) + [p]
        buf = (ctypes.c_char * n).from_address(p)
        return np.frombuffer(buf, dtype=dtype).reshape(shape)

    # ---- the hot path
    def dist_prec(self, rec0, nrec=1, sync=True):
        """dist_prec (dist_prec.c:8) for every cell, records [rec0, rec0+nrec) of the pushed chunk."""
        self._chk(self.lib.vicgpu_step(self.h, rec0, nrec))
        if sync:
            self._chk(self.lib.vicgpu_synchronize(self.h))

    def synchronize(self):
        self._chk(self.lib.vicgpu_synchronize(self.h))

    # ---- outputs
    def get_fluxes(self):
        fx = np.zeros((C["FX_NROW"], self.dom.nhru))
        self._chk(self.lib.vicgpu_get_fluxes(self.h, _d(fx)))
        return fx

    def get_cell_outputs(self):
        co = np.zeros((C["CO_NROW"], self.dom.ncell))
        self._chk(self.lib.vicgpu_get_cell_outputs(self.h, _d(co)))
        return co

    def get_accum(self):
        ac = np.zeros((C["CA_NROW"], self.dom.ncell))
        self._chk(self.lib.vicgpu_get_accum(self.h, _d(ac)))
        return ac

    def reset_accum(self):
        self._chk(self.lib.vicgpu_reset_accum(self.h))

    def get_cell_errors(self):
        ce = np.zeros(self.dom.ncell, dtype=np.int32)
        self._chk(self.lib.vicgpu_get_cell_errors(self.h, _i(ce)))
        return ce

    # ---- cell validity: cell.isValid and CONTINUEONERROR (vicNl.c:429, 521, 545-559)
    def set_retire_on_error(self, mask):
        """An OR of VICGPU_CELLERR_*: a cell whose flag word has one of these bits set after a step is skipped from the next
        step on, decided on the device.  0 (the default): no cell is ever retired."""
        self._chk(self.lib.vicgpu_set_retire_on_error(self.h, int(mask)))

    def set_cell_valid(self, valid):
        """[ncell]: 0 = skip the cell from the next step on (put_data_init included), non-zero = step it."""
        v = np.ascontiguousarray(valid, dtype=np.int32)
        assert v.shape == (self.dom.ncell,), v.shape
        self._chk(self.lib.vicgpu_set_cell_valid(self.h, _i(v)))

    def get_cell_valid(self):
        v = np.zeros(self.dom.ncell, dtype=np.int32)
        self._chk(self.lib.vicgpu_get_cell_valid(self.h, _i(v)))
        return v

    def set_write_fluxes(self, on):
        self._chk(self.lib.vicgpu_set_write_fluxes(self.h, int(bool(on))))

    # ---- the state as the reference's state file holds it (write_model_state.c:95-337)
    def get_state_records(self):
        rec = np.zeros((self.dom.nhru, abi.sr_len(self.opt.Nnode)))
        self._chk(self.lib.vicgpu_get_state_records(self.h, _d(rec)))
        return rec

    def set_state_records(self, rec):
        rec = np.ascontiguousarray(rec, dtype=np.float64)
        assert rec.shape == (self.dom.nhru, abi.sr_len(self.opt.Nnode))
        self._chk(self.lib.vicgpu_set_state_records(self.h, _d(rec)))

    # ---- put_data: the aggregated output variables (include/vicgpu_out.h)
    def output_list(self):
        """[(name, nelem, aggregation)] of every variable the library provides, index = variable id."""
        lib = self.lib
        return [(lib.vicgpu_out_var_name(v).decode(), lib.vicgpu_out_var_nelem(ctypes.byref(self.opt), v), lib.vicgpu_out_var_agg(v))
                for v in range(lib.vicgpu_out_nvar())]

    def var_ids(self, names):
        ids = [self.lib.vicgpu_out_var_id(n.encode()) for n in names]
        if min(ids) < 0:
            raise VicGpuError("output variable not provided: %s" % [n for n, i in zip(names, ids) if i < 0])
        return np.asarray(ids, dtype=np.int32)

    def put_data_config(self, out_step_ratio=1):
        self._chk(self.lib.vicgpu_put_data_config(self.h, int(out_step_ratio)))

    def put_data_init(self):
        self._chk(self.lib.vicgpu_put_data_init(self.h))

    def _out_rows(self, ids):
        return int(sum(self.lib.vicgpu_out_var_nelem(ctypes.byref(self.opt), int(v)) for v in ids))

    def get_outputs(self, names, reset=True):
        """The aggregates (OutputData.aggdata) of the named variables as the writer wants them: float32 [sum nelem][ncell]."""
        ids = self.var_ids(names)
        out = np.zeros((self._out_rows(ids), self.dom.ncell), dtype=np.float32)
        self._chk(self.lib.vicgpu_get_outputs(self.h, len(ids), _i(ids), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), int(bool(reset))))
        return out

    def get_output_data(self, names, aggregated=False):
        ids = self.var_ids(names)
        out = np.zeros((self._out_rows(ids), self.dom.ncell))
        self._chk(self.lib.vicgpu_get_output_data(self.h, len(ids), _i(ids), int(bool(aggregated)), _d(out)))
        return out

    # ---- output records without a host round trip per record (vicgpu_run_records)
    def records_config(self, names, depth=2):
        """Selects the variables of the records and allocates `depth` device slots; an empty list releases them."""
        ids = self.var_ids(names) if len(names) else np.zeros(0, dtype=np.int32)
        self._chk(self.lib.vicgpu_records_config(self.h, len(ids), _i(ids), int(depth)))

    def run_records(self, step0, nrecords, errors=False):
        """nrecords output records from step step0 of the chunk, out_step_ratio steps each: what dist_prec + get_outputs(reset=True)
        + get_cell_errors give record by record, delivered while the following records run.  Returns a Records."""
        nrow = self.lib.vicgpu_records_nrow(self.h)
        self._chk(min(nrow, 0))
        rec = Records(self, int(nrecords), nrow, errors, self.records_ncol())
        self._chk(self.lib.vicgpu_run_records(self.h, int(step0), int(nrecords), rec.out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                              _i(rec.errors) if errors else None))
        return rec

    def records_set_groups(self, offsets, cells, weights=None, fill=0.0):
        """vicgpu_records_set_groups: the records of run_records become [nrow][ngroup], group g the weighted sum (in the
        order include/vicgpu_out.h states) of the cells cells[offsets[g]:offsets[g + 1]]; weights None: all 1.0; `fill`: the
        value of a group without members.  offsets None (or empty): the groups are removed."""
        if offsets is None or len(offsets) == 0:
            self._chk(self.lib.vicgpu_records_set_groups(self.h, 0, None, None, None, float(fill)))
            return
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        cell = np.ascontiguousarray(cells, dtype=np.int32)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        assert off.ndim == 1 and cell.shape == (int(off[-1]),) and (w is None or w.shape == cell.shape), (off.shape, cell.shape)
        self._chk(self.lib.vicgpu_records_set_groups(self.h, len(off) - 1, _i(off), _i(cell), None if w is None else _d(w), float(fill)))

    def records_get_groups(self):
        """(ngroup, nnz) of the groups in force; (0, 0) when none is set."""
        ng, nnz = ctypes.c_int(0), ctypes.c_int(0)
        self._chk(self.lib.vicgpu_records_get_groups(self.h, ctypes.byref(ng), ctypes.byref(nnz)))
        return ng.value, nnz.value

    def records_ncol(self):
        """Columns of a record: the groups when groups are set, else the cells."""
        n = self.lib.vicgpu_records_ncol(self.h)
        self._chk(min(n, 0))
        return n

    def get_balance(self):
        pb = np.zeros((C["PB_NROW"], self.dom.ncell))
        self._chk(self.lib.vicgpu_get_balance(self.h, _d(pb)))
        return pb

    def set_fluxes(self, fx):
        fx = np.ascontiguousarray(fx, dtype=np.float64)
        assert fx.shape == (C["FX_NROW"], self.dom.nhru)
        self._chk(self.lib.vicgpu_set_fluxes(self.h, _d(fx)))

    def glacier_mass_balance_fit(self, reset=True):
        """End of a glacier accumulation interval (accumulateGlacierMassBalance.c:53-66): [GMB_NROW][ncell] fit per cell."""
        eq = np.zeros((C["GMB_NROW"], self.dom.ncell))
        self._chk(self.lib.vicgpu_glacier_mass_balance_fit(self.h, _d(eq), int(bool(reset))))
        return eq

    def debug_pure(self, fn, inputs):
        """Test hook (vicgpu_debug_pure): one pure function of the path for every row of inputs [n][VICGPU_PURE_NIN]."""
        inp = np.zeros((len(inputs), C["VICGPU_PURE_NIN"]) if "VICGPU_PURE_NIN" in C else (len(inputs), 10))
        inputs = np.asarray(inputs, dtype=np.float64)
        inp[:, :inputs.shape[1]] = inputs
        out = np.zeros(inp.shape[0])
        self._chk(self.lib.vicgpu_debug_pure(self.h, int(fn), inp.shape[0], _d(inp), _d(out)))
        return out

    def debug_node_root(self, mode, cases):
        """Test hook (vicgpu_debug_node_root): one frozen-node visit for every row of cases [n][VICGPU_NODE_NIN];
        mode: an OR of VICGPU_NODE_NODE1 / _NEWTON / _EXP_TRANS.  Returns (T [n], failed [n] bool)."""
        inp = np.ascontiguousarray(cases, dtype=np.float64)
        assert inp.ndim == 2 and inp.shape[1] == C["VICGPU_NODE_NIN"] and inp.shape[0] > 0
        out = np.zeros((inp.shape[0], C["VICGPU_NODE_NOUT"]))
        self._chk(self.lib.vicgpu_debug_node_root(self.h, int(mode), inp.shape[0], _d(inp), _d(out)))
        return out[:, 0].copy(), out[:, 1] != 0

    def debug_root_brent(self, mode, bounds, fvals, off):
        """Test hook (vicgpu_debug_root_brent): replays root finds with recorded residual values.  bounds [n][2]; case i is
        given fvals[off[i]:off[i + 1]] in turn; mode VICGPU_BRENT_FULL (Brent) or VICGPU_BRENT_LEAN (BrentLean).
        Returns (xreq [off[n]]: the abscissae requested, out [n][VICGPU_BRENT_NOUT])."""
        b = np.ascontiguousarray(bounds, dtype=np.float64)
        f = np.ascontiguousarray(fvals, dtype=np.float64)
        o = np.ascontiguousarray(off, dtype=np.int32)
        assert b.ndim == 2 and b.shape[1] == 2 and b.shape[0] > 0 and o.shape == (b.shape[0] + 1,) and f.shape == (o[-1],)
        x = np.full(max(int(o[-1]), 1), np.nan)
        out = np.zeros((b.shape[0], C["VICGPU_BRENT_NOUT"]))
        self._chk(self.lib.vicgpu_debug_root_brent(self.h, int(mode), b.shape[0], _d(b), _i(o), _d(f) if f.size else None,
                                                   _d(x), _d(out)))
        return x[:o[-1]].copy(), out

    def last_kernel_ms(self):
        ms = ctypes.c_double(0)
        n = ctypes.c_int(0)
        self._chk(self.lib.vicgpu_last_kernel_ms(self.h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value


def partition(cell_hru_offset, nshard):
    """vicgpu_group_partition: the shard boundaries [nshard+1] the group cuts a domain at (the rule of shard.partition_cells)."""
    lib = load_library()
    off = np.ascontiguousarray(cell_hru_offset, dtype=np.int32)
    b = np.zeros(int(nshard) + 1, dtype=np.int32)
    rc = lib.vicgpu_group_partition(len(off) - 1, _i(off), int(nshard), _i(b))
    if rc != 0:
        raise VicGpuError("vicgpu_group_partition failed with code %d" % rc)
    return b


class _GroupLib:
    """The library as a Group's methods see it: vicgpu_<name> is vicgpu_group_<name> for every entry the group mirrors, the
    functions that take no context (vicgpu_out_*, vicgpu_host_*) are the library's own, anything else has no group form."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        base = name[len("vicgpu_"):]
        if base in GROUP_ENTRIES:
            return getattr(self._lib, "vicgpu_group_" + base)
        if base.startswith(("out_", "host_", "group_")):
            return getattr(self._lib, name)
        raise AttributeError("%s has no device-group form (use Group.shard_ctx)" % name)


class Group(Model):
    """One domain on several contexts (include/vicgpu_group.h): contiguous cell blocks, one per entry of `devices` (devices
    may repeat), stepped at the same time from one host thread per shard.  Model's methods, on the whole domain: every
    table goes in and comes out in the domain's global layout."""

    def __init__(self, dom, devices=(0,)):
        lib = load_library()
        self.lib = _GroupLib(lib)
        self.dom = dom
        self.opt = dom.opt
        self.devices = np.ascontiguousarray(devices, dtype=np.int32)
        h = ctypes.c_void_p()
        rc = lib.vicgpu_group_create(ctypes.byref(dom.opt), len(self.devices), _i(self.devices), ctypes.byref(h))
        if rc != 0:
            raise VicGpuError("vicgpu_group_create failed with code %d (no GPU, a device out of range, or unsupported options)" % rc)
        self.h = h
        self._chk(self.lib.vicgpu_set_veglib(h, dom.veglib.shape[0], _d(np.ascontiguousarray(dom.veglib))))
        self.set_domain(dom)

    def shard_bounds(self):
        """[nshard+1]: shard k holds the cells [b[k], b[k+1])."""
        b = np.zeros(len(self.devices) + 1, dtype=np.int32)
        self._chk(self.lib.vicgpu_group_shard_bounds(self.h, _i(b)))
        return b

    # ---- cell groups of the records have no device-group form (include/vicgpu_group.h)
    def records_set_groups(self, offsets, cells, weights=None, fill=0.0):
        raise VicGpuError("records_set_groups has no device-group form: a cell group that spans shards has no summation order")

    def records_get_groups(self):
        return 0, 0

    def records_ncol(self):
        return self.dom.ncell

    # ---- a mix across shards would be an all-to-all with a summation order of its own (include/vicgpu_group.h)
    def mix_cells(self, rows, dst_cells, term_off, term_cell, term_weight):
        raise VicGpuError("mix_cells has no device-group form: give a shard's context (shard_ctx) the call in its local numbering")

    def _no_member_transform(self, *args, **kw):
        raise VicGpuError("the member transform has no device-group form: a column's members would lie on different devices")

    member_transform_solve = member_transform_set = member_transform_get = member_transform_apply = _no_member_transform

    def shard_ctx(self, k):
        """Shard k's vicgpu_ctx handle, for the per-context entries (stream, tuning, debug)."""
        p = self.lib.vicgpu_group_shard_ctx(self.h, int(k))
        if not p:
            raise VicGpuError("no shard %d" % k)
        return ctypes.c_void_p(p)
