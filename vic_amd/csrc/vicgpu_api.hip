// vicgpu_api.hip — the C ABI of the MI355X VIC hot path (include/vicgpu.h): the extern "C" entry points and their static
// helpers, nothing else.  gfx950 only.  This is the one translation unit of the library; the code lives in the headers:
//   vic_types / _math / _soil / _snow / _surface / _blowing / _step / _glacier .hpp   the physics of an HRU step, lane-private
//   vic_profile.hpp, vic_implicit.hpp   the soil-profile solves as kernels of their own, and the work lists they run on
//   vic_putdata.hpp      vic_put_sum/_finish/_aggregate: put_data (put_data.c:7-760), the aggregated output variables
//   vic_ctx.hpp          the parked context of the finite-difference pipeline: layout, parking map, accessors
//   vic_hru_io.hpp       KArgs, LaunchMap and the HRU table I/O
//   vic_kernels.hpp      vic_hru_step, vic_fd_stage, vic_surf_eval
//   vic_aux_kernels.hpp  glacier fit, derived cell rows, test hooks, vic_cell_reduce, state records, forcing derivation
//   vic_records.hpp      vic_out_pack_reset: the end of an output record (vicgpu_run_records); vic_out_group_reduce: its
//                        reduction over cell groups (vicgpu_records_set_groups)
//   vic_rows.hpp         listed rows and columns of a table through a budgeted stage: the host check of the lists,
//                        vic_rows_gather / _scatter, the pass loop; shared by the four headers below
//   vic_copy_cells.hpp   vicgpu_copy_cells: the host planning of a copy between cells, vic_copy_direct, the staged path
//   vic_params.hpp       vicgpu_update_cell_params / _hru_params: the owner cells of listed HRUs and the listed-cell forms
//                        of the derive kernels
//   vic_state_update.hpp vicgpu_get_state_rows / _update_state / _derive_soil_state: vic_derive_soil_state, the tail of
//                        initialize_model_state for listed HRUs
//   vic_mix_cells.hpp    vicgpu_mix_cells: the host planning of a linear combination across cells and vic_mix_cells
//   vic_member_transform.hpp  vicgpu_member_transform_solve / _set / _get / _apply: the checks of a call, the batched Jacobi
//                        eigen-solver vic_member_transform_solve and vic_member_transform_apply, vic_mix_cells with implied terms
//   vic_host.hpp         owners of every device buffer, pinned block, stream and event; the buffers' counted transfers; the
//                        VICGPU_STATS timer of an entry
//   vic_checks.hpp       the domain-list and state-record checks (no HIP), shared with the group
//   vic_pipeline.hpp     vicgpu_ctx, Tuning, Domain, FdChunk and the steps that build them, the launchers, fd_step, the read-backs
//   vic_group.hpp        the device group (include/vicgpu_group.h): host code on top of the entries below
// An entry moves a table that a DevBuf owns through that buffer (upload / download / fill, counted in elements and checked
// against its size); sizeof is left for what no DevBuf owns.
// The order of the device headers below is the order of the device code in the code object (calls to the out-of-line
// calc_blowing_snow are pc-relative): keep it.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <thread>
#include <vector>
#include "vicgpu.h"
#include "vic_glacier.hpp"
#include "vic_profile.hpp"
#include "vic_putdata.hpp"
#include "vic_host.hpp"
#include "vic_checks.hpp"
#include "vic_implicit.hpp"
#include "vic_ctx.hpp"
#include "vic_hru_io.hpp"
#include "vic_kernels.hpp"
#include "vic_aux_kernels.hpp"
#include "vic_records.hpp"
#include "vic_rows.hpp"
#include "vic_copy_cells.hpp"
#include "vic_params.hpp"
#include "vic_state_update.hpp"
#include "vic_mix_cells.hpp"
#include "vic_member_transform.hpp"
#include "vic_pipeline.hpp"
#include "vic_group.hpp"

using namespace vic;

extern "C" {

#ifdef VIC_PROF
// tuning build only (not part of include/vicgpu.h): read and clear the section counters
int vicgpu_prof_read(unsigned long long* cyc, unsigned long long* cnt) {
  if (hipMemcpyFromSymbol(cyc, HIP_SYMBOL(vic_prof_cyc), sizeof(unsigned long long) * 32) != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(cnt, HIP_SYMBOL(vic_prof_cnt), sizeof(unsigned long long) * 32) != hipSuccess) return -1;
  unsigned long long z[32] = {0};
  if (hipMemcpyToSymbol(HIP_SYMBOL(vic_prof_cyc), z, sizeof(z)) != hipSuccess) return -1;
  if (hipMemcpyToSymbol(HIP_SYMBOL(vic_prof_cnt), z, sizeof(z)) != hipSuccess) return -1;
  return 0;
}
#endif

int vicgpu_abi_version(void) { return VICGPU_ABI_VERSION; }

const char* vicgpu_last_error(const vicgpu_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int vicgpu_create(const vicgpu_options* opt, int device, vicgpu_ctx** out) {
  if (!opt || !out) return VICGPU_ERR_ARG;
  *out = nullptr;
  if (opt->abi_version != VICGPU_ABI_VERSION) return VICGPU_ERR_ARG;
  if (opt->Nlayer != VIC_NLAYER || opt->Nnode < 3 || opt->Nnode > VIC_MAX_NODES || opt->Nband < 1 || opt->Nband > VIC_MAX_BANDS)
    return VICGPU_ERR_UNSUPPORTED;
  if (opt->dt <= 0 || opt->snow_step <= 0 || opt->dt % opt->snow_step != 0) return VICGPU_ERR_ARG;
  if (opt->QUICK_FLUX && opt->Nnode != 3) return VICGPU_ERR_ARG;             // get_global_param.c:1151-1155
  if (opt->FROZEN_SOIL && opt->QUICK_FLUX) return VICGPU_ERR_ARG;            // get_global_param.c:376-381
  // options of the reference this library does not implement are refused, never silently replaced
  // QUICK_SOLVE (calc_surf_energy_bal.c:289-309, 400-480; ignored with QUICK_FLUX like in the reference): the reference forces
  // NOFLUX and EXP_TRANS off for the iteration and keeps whatever it last set for the final evaluation (NOFLUX returns with a
  // second iteration, EXP_TRANS never does): reproduced; not combined with IMPLICIT
  if (opt->QUICK_SOLVE && !opt->QUICK_FLUX && opt->IMPLICIT) return VICGPU_ERR_UNSUPPORTED;
  // IMPLICIT up to VIC_MID_NODES nodes (the reference's own Newton-Raphson solver stops at 21: MAXSIZE, newt_raph_func_fast.c:7)
  if (opt->IMPLICIT && !opt->QUICK_FLUX && opt->Nnode > VIC_MID_NODES) return VICGPU_ERR_UNSUPPORTED;
  // IMPLICIT (newt_raph_func_fast.c): the finite-difference soil profile with the node freezing parameters of the node
  // arrays; the reference as shipped reads the 3-element layer arrays out of bounds there (frozen_soil.c:283-284)
  if (opt->IMPLICIT && (opt->QUICK_FLUX || opt->frozen_compat)) return VICGPU_ERR_UNSUPPORTED;
  if (opt->NODE_SOLVER != VIC_NODE_SOLVER_BRENT && opt->NODE_SOLVER != VIC_NODE_SOLVER_NEWTON) return VICGPU_ERR_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return VICGPU_ERR_HIP;   // no CPU fallback: fail loudly
  if (device < 0 || device >= ndev) return VICGPU_ERR_ARG;
  std::unique_ptr<vicgpu_ctx> c(new vicgpu_ctx());       // a failure below deletes it, and with it whatever it holds by then
  c->opt = *opt;
  c->device = device;
  Opt& o = c->o;
  o.Nnode = opt->Nnode; o.Nband = opt->Nband; o.dt = opt->dt; o.snow_step = opt->snow_step;
  o.NF = VICGPU_NF(opt); o.NR = VICGPU_NR(opt);
  o.FULL_ENERGY = opt->FULL_ENERGY; o.FROZEN_SOIL = opt->FROZEN_SOIL; o.QUICK_FLUX = opt->QUICK_FLUX; o.NOFLUX = opt->NOFLUX;
  o.EXP_TRANS = opt->EXP_TRANS; o.GRND_FLUX_TYPE = opt->GRND_FLUX_TYPE; o.TFALLBACK = opt->TFALLBACK;
  o.AERO_RESIST_CANSNOW = opt->AERO_RESIST_CANSNOW; o.SNOW_ALBEDO = opt->SNOW_ALBEDO; o.SNOW_DENSITY = opt->SNOW_DENSITY;
  o.TEMP_TH_TYPE = opt->TEMP_TH_TYPE; o.GLACIER_ID = opt->GLACIER_ID; o.GLACIER_DYNAMICS = opt->GLACIER_DYNAMICS;
  o.frozen_compat = opt->frozen_compat; o.nveg_types = opt->nveg_types; o.wind_h = opt->wind_h; o.CORRPREC = opt->CORRPREC;
  o.BLOWING = opt->BLOWING ? 1 : 0; o.IMPLICIT = opt->IMPLICIT; o.QUICK_SOLVE = (opt->QUICK_SOLVE && !opt->QUICK_FLUX) ? 1 : 0;
  // calc_surf_energy_bal.c:300-308: with QUICK_SOLVE and a surface energy balance the solver's EXP_TRANS is FALSE from the first
  // iteration to the final evaluation (the linear-spacing coefficients on the run's node geometry, whatever it is)
  if (o.QUICK_SOLVE && o.FULL_ENERGY) o.EXP_TRANS = 0;
  HIPCHK(c, hipSetDevice(device));
  HIPCHK(c, c->stream.create());
  HIPCHK(c, c->copy_stream.create());
  for (auto& sl : c->slot) { HIPCHK(c, sl.uploaded.create(hipEventDisableTiming)); HIPCHK(c, sl.released.create(hipEventDisableTiming)); }
  *out = c.release();
  return VICGPU_OK;
}

void vicgpu_destroy(vicgpu_ctx* c) {
  if (!c) return;
  HIPIGN(hipSetDevice(c->device));
  if (c->stream) HIPIGN(hipStreamSynchronize(c->stream));
  if (c->copy_stream) HIPIGN(hipStreamSynchronize(c->copy_stream));
  if (c->rec.dl) HIPIGN(hipStreamSynchronize(c->rec.dl));
  records_report_reduce(c);
  if (c->tune.stats)
    for (size_t k = 0; k < c->dom.chunks.size(); k++)
      if (c->dom.chunks[k].steps)
        fprintf(stderr, "[vicgpu] chunk %zu: %d cells, %d HRUs, %lld steps, %.1f Brent rounds per step\n", k, c->dom.chunks[k].ccount,
                c->dom.chunks[k].gcount, c->dom.chunks[k].steps, (double)c->dom.chunks[k].rounds / c->dom.chunks[k].steps);
  delete c;                        // the members release what they own (vic_host.hpp)
}

int vicgpu_set_veglib(vicgpu_ctx* c, int nrow, const double* veglib) {
  if (!c || !veglib || nrow != c->opt.nveg_types + 4) return VICGPU_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, c->d_veglib.alloc((size_t)nrow * VL_NFIELD));
  HIPCHK(c, c->d_veglib.upload(c->stream, veglib));
  c->nveg_rows = nrow;
  return VICGPU_OK;
}

static int set_domain_impl(vicgpu_ctx* c, int ncell, int nhru, const double* cell_params, const int* hpi, const double* hpd,
                           const int* cell_hru_offset, const int* cell_hru_list) {
  if (!c || ncell <= 0 || nhru <= 0 || !cell_params || !hpi || !hpd || !cell_hru_offset || !cell_hru_list) return VICGPU_ERR_ARG;
  if (check_domain_lists(ncell, nhru, cell_hru_offset, cell_hru_list, hpi, c->opt.Nband, c->opt.nveg_types + 4).rule != DOMAIN_OK)
    return VICGPU_ERR_ARG;         // the domain the context holds stays as it is
  HIPCHK(c, hipSetDevice(c->device));
  free_domain(c);
  c->tune = read_tuning(c->opt.NODE_SOLVER, ncell);
  c->dom.ncell = ncell; c->dom.nhru = nhru;
  c->dom.ncol = ncell;             // the forcing map of a fresh domain is the identity
  c->dom.fd = !c->o.QUICK_FLUX;
  int r = domain_tables(c, cell_params, hpi, hpd, cell_hru_offset, cell_hru_list);
  if (r == VICGPU_OK && c->dom.fd) r = domain_fd_workspace(c);
  if (r == VICGPU_OK && c->dom.fd) r = domain_chunks(c, hpi, cell_hru_offset, cell_hru_list);
  if (r != VICGPU_OK) return r;
  HIPCHK(c, hipStreamSynchronize(c->stream));      // the one wait for every fill queued above
  return VICGPU_OK;
}

int vicgpu_set_domain(vicgpu_ctx* c, int ncell, int nhru, const double* cell_params, const int* hpi, const double* hpd,
                      const int* cell_hru_offset, const int* cell_hru_list) {
  if (!c) return VICGPU_ERR_ARG;
  const int r = set_domain_impl(c, ncell, nhru, cell_params, hpi, hpd, cell_hru_offset, cell_hru_list);
  if (r == VICGPU_OK) c->dom.domain_ready = true;
  else if (r == VICGPU_ERR_HIP || r == VICGPU_ERR_NOMEM) {     // failed half-way: leave no partially built domain behind
    HIPIGN(hipSetDevice(c->device));
    HIPIGN(hipStreamSynchronize(c->stream));                   // fills may still be queued on its tables
    free_domain(c);
  }
  return r;
}

int vicgpu_set_state(vicgpu_ctx* c, const double* sd, const int* si) {
  if (!c || !sd || !si) return VICGPU_ERR_ARG;
  if (!c->dom.domain_ready) return VICGPU_ERR_STATE;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, c->dom.d_sd.upload(c->stream, sd));
  HIPCHK(c, c->dom.d_si.upload(c->stream, si));
  return VICGPU_OK;
}

int vicgpu_get_state(vicgpu_ctx* c, double* sd, int* si) {
  if (!c || !sd || !si) return VICGPU_ERR_ARG;
  if (!c->dom.domain_ready) return VICGPU_ERR_STATE;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, c->dom.d_sd.download(c->stream, sd));
  HIPCHK(c, c->dom.d_si.download(c->stream, si));
  return VICGPU_OK;
}

static bool is_pinned(const void* p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { HIPIGN(hipGetLastError()); return false; }
  return at.type == hipMemoryTypeHost;
}

// source -> device on the copy stream: `rows` rows of `width` bytes, `pitch` bytes apart in the source (pitch > width: a
// column block of a wider table, vicgpu_group.h) and packed on the device; straight from pinned memory, through the slot's
// staging area otherwise
static hipError_t upload(vicgpu_ctx* c, vicgpu_ctx::ForcingSlot& sl, void* dst, const void* src, size_t width, size_t rows,
                         size_t pitch, size_t stage_off) {
  if (!is_pinned(src)) {
    char* st = sl.h_stage + stage_off;
    if (pitch == width) memcpy(st, src, width * rows);
    else for (size_t r = 0; r < rows; r++) memcpy(st + r * width, (const char*)src + r * pitch, width);
    return hipMemcpyAsync(dst, st, width * rows, hipMemcpyHostToDevice, c->copy_stream);
  }
  if (pitch == width) return hipMemcpyAsync(dst, src, width * rows, hipMemcpyHostToDevice, c->copy_stream);
  return hipMemcpy2DAsync(dst, width, src, pitch, width, rows, hipMemcpyHostToDevice, c->copy_stream);
}

// ld: columns per row of the source forcing / raw tables (c->dom.ncol, or the global column count when a group uploads one
// shard's columns); ld_flag: cells per row of the source flags (c->dom.ncell, or the global cell count).  P: the raw table is
// P->nsrc wide and every forcing column is expanded and perturbed from it (checked by the caller, check_forcing_perturbed).
// Whatever has to grow is allocated before anything is released or uploaded: a refused allocation leaves the slot as it was.
static int prefetch_impl(vicgpu_ctx* c, int nsteps, const double* forcing, const unsigned char* snowflag, const double* raw,
                         const int* dmy, double min_wind, int plapse, int ld, int ld_flag, const PertLists* P) {
  if (!c || nsteps <= 0 || !dmy || (!raw && (!forcing || !snowflag))) return VICGPU_ERR_ARG;
  if (!c->dom.domain_ready) return VICGPU_ERR_STATE;
  HIPCHK(c, hipSetDevice(c->device));
  for (int s = 0; s < nsteps; s++) {
    int m = dmy[(size_t)s * VIC_NDMY + VIC_DMY_MONTH];
    if (m < 1 || m > 12) return VICGPU_ERR_ARG;          // month indexes the veg library tables
  }
  const size_t nsub = c->o.NR + 1;
  const size_t ncol = c->dom.ncol;                                                            // values per column, flags per cell
  const size_t sbytes = (size_t)nsteps * nsub * c->dom.ncell, nf = (size_t)VIC_NFORCE * nsteps * nsub * ncol;      // flags (a byte each) and forcing values
  const size_t rawcols = P ? (size_t)P->nsrc : ncol;
  const size_t nraw = raw ? (size_t)nsteps * VIC_NRAW * c->o.dt * rawcols : 0;
  const size_t fbytes = sizeof(double) * nf, rbytes = sizeof(double) * nraw;                   // in the staging area
  const size_t npert = (P && P->pert) ? (size_t)nsteps * VICGPU_NPERT * P->ngroup : 0;         // the factors and the two lists
  const size_t nlsrc = (P && P->col_src) ? ncol : 0, nlgrp = (P && P->col_group) ? ncol : 0;
  const int t = (c->cur == 0) ? 1 : 0;
  vicgpu_ctx::ForcingSlot& sl = c->slot[t];
  // the slot's previous upload may still be reading its staging area; the steps that read the slot's device buffers were
  // queued before `released` was recorded (vicgpu_swap_forcing): the copy stream waits for that, not the host
  if (sl.upload_pending) { HIPCHK(c, hipEventSynchronize(sl.uploaded)); sl.upload_pending = false; }
  if (sl.was_current) HIPCHK(c, hipStreamWaitEvent(c->copy_stream, sl.released, 0));
  const size_t raw_stage = raw ? (is_pinned(raw) ? 0 : rbytes) : 0;
  const size_t need_stage = raw ? raw_stage + sizeof(double) * npert + sizeof(int) * (nlsrc + nlgrp)      // the lists always go through it
                                : ((is_pinned(forcing) ? 0 : fbytes) + (is_pinned(snowflag) ? 0 : sbytes));
  DevBuf<double> g_f, g_raw, g_pert;
  DevBuf<unsigned char> g_s;
  DevBuf<int> g_src, g_grp;
  PinnedBuf<char> g_stage;
  if (nf > sl.d_f.size()) HIPCHK(c, g_f.alloc(nf));
  if (sbytes > sl.d_s.size()) HIPCHK(c, g_s.alloc(sbytes));
  if (nraw > sl.d_raw.size()) HIPCHK(c, g_raw.alloc(nraw));
  if (npert > sl.d_pert.size()) HIPCHK(c, g_pert.alloc(npert));
  if (nlsrc > sl.d_col_src.size()) HIPCHK(c, g_src.alloc(nlsrc));
  if (nlgrp > sl.d_col_group.size()) HIPCHK(c, g_grp.alloc(nlgrp));
  if (need_stage > sl.h_stage.size()) HIPCHK(c, g_stage.alloc(need_stage));
  if (g_f || g_s || g_raw || g_pert || g_src || g_grp) {      // re-allocation: nothing may still use the old buffers
    HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    if (sl.was_current) HIPCHK(c, hipEventSynchronize(sl.released));
  }
  // every allocation got through: the slot takes the new buffers and the old ones go
  if (g_f) { sl.d_f = std::move(g_f); g_f.reset(); }
  if (g_s) { sl.d_s = std::move(g_s); g_s.reset(); }
  if (g_raw) { sl.d_raw = std::move(g_raw); g_raw.reset(); }
  if (g_pert) { sl.d_pert = std::move(g_pert); g_pert.reset(); }
  if (g_src) { sl.d_col_src = std::move(g_src); g_src.reset(); }
  if (g_grp) { sl.d_col_group = std::move(g_grp); g_grp.reset(); }
  if (g_stage) { sl.h_stage = std::move(g_stage); g_stage.reset(); }
  if (raw) {
    HIPCHK(c, upload(c, sl, sl.d_raw, raw, sizeof(double) * rawcols, (size_t)nsteps * VIC_NRAW * c->o.dt, sizeof(double) * ld, 0));
    FArgs a;
    a.nsteps = nsteps; a.ncell = c->dom.ncell; a.dt = c->o.dt; a.snow_step = c->o.snow_step; a.NF = c->o.NF; a.NR = c->o.NR;
    a.temp_th_type = c->o.TEMP_TH_TYPE; a.Nband = c->o.Nband; a.Nnode = c->o.Nnode; a.plapse = plapse;
    a.ncol = c->dom.ncol; a.cell_col = c->dom.d_cell_col;
    a.min_wind = (double)(float)min_wind;        // options.MIN_WIND_SPEED is a float (vicNl_def.h:713)
    a.raw = sl.d_raw; a.cell_params = c->dom.d_cp; a.forcing = sl.d_f; a.snowflag = sl.d_s;
    const size_t n = (size_t)nsteps * c->dom.ncell, nc = (size_t)nsteps * ncol;
    const dim3 gcell((unsigned)((n + 255) / 256)), gcol((unsigned)((nc + 255) / 256)), block(256);
    FPArgs pa;
    if (P) {                                     // the factors and the lists: staged behind the raw table, free when the call returns
      char* st = sl.h_stage + raw_stage;
      if (npert) {
        memcpy(st, P->pert, sizeof(double) * npert);
        HIPCHK(c, hipMemcpyAsync(sl.d_pert.get(), st, sizeof(double) * npert, hipMemcpyHostToDevice, c->copy_stream));
        st += sizeof(double) * npert;
      }
      if (nlsrc) {
        int* l = (int*)st;
        for (size_t i = 0; i < ncol; i++) l[i] = P->col_src[i] - P->src_base;
        HIPCHK(c, hipMemcpyAsync(sl.d_col_src.get(), st, sizeof(int) * ncol, hipMemcpyHostToDevice, c->copy_stream));
        st += sizeof(int) * ncol;
      }
      if (nlgrp) {
        memcpy(st, P->col_group, sizeof(int) * ncol);
        HIPCHK(c, hipMemcpyAsync(sl.d_col_group.get(), st, sizeof(int) * ncol, hipMemcpyHostToDevice, c->copy_stream));
      }
      pa.f = a; pa.nsrc = P->nsrc; pa.ngroup = P->ngroup; pa.group_base = P->group_base;
      pa.col_src = nlsrc ? sl.d_col_src.get() : nullptr; pa.col_group = nlgrp ? sl.d_col_group.get() : nullptr;
      pa.pert = npert ? sl.d_pert.get() : nullptr;
    }
    if (c->tune.stats && !sl.derive_t0) { HIPCHK(c, sl.derive_t0.create()); HIPCHK(c, sl.derive_t1.create()); }
    const bool timed = c->tune.stats;
    if (timed) HIPCHK(c, hipEventRecord(sl.derive_t0, c->copy_stream));
    const bool mapped = c->dom.d_cell_col;
    if (P) {                                     // rows (and, without a map, flags) per forcing column
      if (mapped) {
        if (npert) hipLaunchKernelGGL((vic_derive_forcing_pert<false, true>), gcol, block, 0, c->copy_stream, pa);
        else hipLaunchKernelGGL((vic_derive_forcing_pert<false, false>), gcol, block, 0, c->copy_stream, pa);
      } else {
        if (npert) hipLaunchKernelGGL((vic_derive_forcing_pert<true, true>), gcol, block, 0, c->copy_stream, pa);
        else hipLaunchKernelGGL((vic_derive_forcing_pert<true, false>), gcol, block, 0, c->copy_stream, pa);
      }
    } else if (!mapped) hipLaunchKernelGGL(vic_derive_forcing, gcell, block, 0, c->copy_stream, a);
    else hipLaunchKernelGGL(vic_derive_forcing_cols, gcol, block, 0, c->copy_stream, a);      // the rows once per column
    if (mapped) hipLaunchKernelGGL(vic_derive_forcing_flags, gcell, block, 0, c->copy_stream, a);      // every cell's flag from its column's rows
    HIPCHK(c, hipGetLastError());
    if (timed) HIPCHK(c, hipEventRecord(sl.derive_t1, c->copy_stream));
    sl.derive_timed = timed;
  } else {
    HIPCHK(c, upload(c, sl, sl.d_f, forcing, sizeof(double) * ncol, (size_t)nsteps * VIC_NFORCE * nsub, sizeof(double) * ld, 0));
    HIPCHK(c, upload(c, sl, sl.d_s, snowflag, c->dom.ncell, (size_t)nsteps * nsub, ld_flag, is_pinned(forcing) ? 0 : fbytes));
    sl.derive_timed = false;
  }
  HIPCHK(c, hipEventRecord(sl.uploaded, c->copy_stream));
  sl.upload_pending = true;
  sl.was_current = false;
  sl.dmy.assign(dmy, dmy + (size_t)nsteps * VIC_NDMY);
  sl.nsteps = nsteps;
  c->staged = t;
  return VICGPU_OK;
}

int vicgpu_prefetch_forcing(vicgpu_ctx* c, int nsteps, const double* forcing, const unsigned char* snowflag, const int* dmy) {
  return c ? prefetch_impl(c, nsteps, forcing, snowflag, nullptr, dmy, 0.0, 1, c->dom.ncol, c->dom.ncell) : VICGPU_ERR_ARG;
}
int vicgpu_prefetch_forcing_raw(vicgpu_ctx* c, int nsteps, const double* raw, const int* dmy, double min_wind_speed, int plapse) {
  if (!raw) return VICGPU_ERR_ARG;
  return c ? prefetch_impl(c, nsteps, nullptr, nullptr, raw, dmy, min_wind_speed, plapse, c->dom.ncol, c->dom.ncell) : VICGPU_ERR_ARG;
}
int vicgpu_prefetch_forcing_perturbed(vicgpu_ctx* c, int nsteps, int nsrc, const double* raw, const int* col_src, int ngroup,
                                      const int* col_group, const double* pert, const int* dmy, double min_wind_speed, int plapse) {
  if (!c || !raw || !dmy || nsteps <= 0 || nsrc < 1) return VICGPU_ERR_ARG;
  if (!c->dom.domain_ready) return VICGPU_ERR_STATE;
  c->err = check_forcing_perturbed(c->dom.ncol, nsteps, nsrc, col_src, ngroup, col_group, pert, dmy);
  if (!c->err.empty()) return VICGPU_ERR_ARG;
  if (!col_src && ngroup == 0) return prefetch_impl(c, nsteps, nullptr, nullptr, raw, dmy, min_wind_speed, plapse, c->dom.ncol, c->dom.ncell);
  const PertLists P{nsrc, col_src, 0, ngroup, col_group, 0, pert};
  return prefetch_impl(c, nsteps, nullptr, nullptr, raw, dmy, min_wind_speed, plapse, nsrc, c->dom.ncell, &P);
}

int vicgpu_swap_forcing(vicgpu_ctx* c) {
  if (!c) return VICGPU_ERR_ARG;
  if (c->staged < 0) return VICGPU_ERR_STATE;
  HIPCHK(c, hipSetDevice(c->device));
  if (c->cur >= 0) {                                      // every step queued so far read the old chunk: fence it
    HIPCHK(c, hipEventRecord(c->slot[c->cur].released, c->stream));
    c->slot[c->cur].was_current = true;
  }
  vicgpu_ctx::ForcingSlot& sl = c->slot[c->staged];
  // the source buffer (pinned user memory or the staging area) is free again once the upload has finished
  HIPCHK(c, hipEventSynchronize(sl.uploaded));
  sl.upload_pending = false;
  if (sl.derive_timed) {                                  // tuning (VICGPU_STATS): what the derivation of this chunk took on the device
    float ms = 0;
    if (hipEventElapsedTime(&ms, sl.derive_t0, sl.derive_t1) == hipSuccess)
      fprintf(stderr, "[vicgpu] forcing derive: %d steps, %d columns, %d cells: %.4f ms\n", sl.nsteps, c->dom.ncol, c->dom.ncell, ms);
    sl.derive_timed = false;
  }
  c->cur = c->staged; c->staged = -1;
  c->d_forcing = sl.d_f; c->d_snowflag = sl.d_s; c->dmy = sl.dmy; c->chunk_steps = sl.nsteps;
  return VICGPU_OK;
}

int vicgpu_push_forcing(vicgpu_ctx* c, int nsteps, const double* forcing, const unsigned char* snowflag, const int* dmy) {
  const int r = vicgpu_prefetch_forcing(c, nsteps, forcing, snowflag, dmy);
  return r == VICGPU_OK ? vicgpu_swap_forcing(c) : r;
}

int vicgpu_get_forcing(vicgpu_ctx* c, int step, double* forcing, unsigned char* snowflag) {
  if (!c || !forcing || !snowflag) return VICGPU_ERR_ARG;
  if (c->cur < 0 || step < 0 || step >= c->chunk_steps) return VICGPU_ERR_STATE;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t nflag = (size_t)(c->o.NR + 1) * c->dom.ncell, nforce = (size_t)VIC_NFORCE * (c->o.NR + 1) * c->dom.ncol;      // of one step
  const vicgpu_ctx::ForcingSlot& sl = c->slot[c->cur];      // d_forcing / d_snowflag are views of its buffers
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, sl.d_f.download(c->stream, forcing, step * nforce, nforce));
  HIPCHK(c, sl.d_s.download(c->stream, snowflag, step * nflag, nflag));
  return VICGPU_OK;
}

// ---- forcing map: cell -> forcing column (ensembles, a model grid finer than its forcing grid)
int vicgpu_set_forcing_map(vicgpu_ctx* c, int ncol, const int* cell_col) {
  if (!c) return VICGPU_ERR_ARG;
  if (!c->dom.domain_ready) return VICGPU_ERR_STATE;
  Domain& d = c->dom;
  if (cell_col) {
    if (ncol < 1) return VICGPU_ERR_ARG;
    for (int i = 0; i < d.ncell; i++)
      if (cell_col[i] < 0 || cell_col[i] >= ncol) return VICGPU_ERR_ARG;      // the map and the chunk in force stay
  } else if (ncol != 0 && ncol != d.ncell) return VICGPU_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));      // the steps queued so far ran on the map as it was
  HIPCHK(c, hipStreamSynchronize(c->copy_stream)); // and a prefetch in flight fills a slot of the old width
  DevBuf<int> cols, fcol;          // become the domain's only when complete
  if (cell_col) {
    HIPCHK(c, cols.alloc(d.ncell));
    HIPCHK(c, fcol.alloc(d.nhru));
    HIPCHK(c, cols.upload(c->stream, cell_col));
    const int* hpi_cell = d.d_hpi + (size_t)HPI_CELL * d.nhru;
    const int* cols_arg = cols;
    int* fcol_arg = fcol;
    const int nhru = d.nhru;
    hipLaunchKernelGGL(vic_fill_hru_fcol, dim3((unsigned)((nhru + 255) / 256)), dim3(256), 0, c->stream, hpi_cell, cols_arg, nhru, fcol_arg);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  d.d_cell_col = std::move(cols); d.d_hru_fcol = std::move(fcol);      // identity: both empty, the old ones released
  if (cell_col) d.cell_col.assign(cell_col, cell_col + d.ncell); else d.cell_col.clear();
  d.ncol = cell_col ? ncol : d.ncell;
  drop_forcing(c);                 // a chunk's rows are as wide as the map it was pushed for
  return VICGPU_OK;
}

int vicgpu_get_forcing_map(vicgpu_ctx* c, int* ncol, int* cell_col) {
  if (!c || !ncol) return VICGPU_ERR_ARG;
  if (!c->dom.domain_ready) return VICGPU_ERR_STATE;
  *ncol = c->dom.ncol;
  if (cell_col)
    for (int i = 0; i < c->dom.ncell; i++) cell_col[i] = c->dom.cell_col.empty() ? i : c->dom.cell_col[i];
  return VICGPU_OK;
}

void* vicgpu_host_alloc(size_t bytes) {
  PinnedBuf<char> b;               // the caller owns the block from here to vicgpu_host_free
  return b.alloc(bytes ? bytes : 1) == hipSuccess ? b.release() : nullptr;
}
void vicgpu_host_free(void* p) { PinnedBuf<char> b((char*)p); }

// vicgpu_step (ratio = 0), or the steps of vicgpu_run_records: nsteps = nrecords * ratio, an output record ends after every
// `ratio` steps (c->rec describes the call).  The event pairs of vicgpu_last_kernel_ms cover the steps of the last record.
static int step_impl(vicgpu_ctx* c, int step0, int nsteps, int ratio) {
  const bool records = ratio > 0;
  const int per = records ? ratio : nsteps;          // steps the event pairs cover
  while ((int)c->ev.size() < 2 * per) {
    Event e;
    HIPCHK(c, e.create());
    c->ev.push_back(std::move(e));
  }
  c->ev_used = 0;
  c->ev_steps = 0;
  StepPlan plan;
  plan.c = c; plan.step0 = step0; plan.nsteps = nsteps; plan.records = records; plan.ratio = ratio;
  if (c->retire_mask) c->dom.valid_live = true;      // these steps may retire cells: the kernels take the validity table from here on
  plan.ka = make_kargs(c); plan.ca = make_cargs(c);
  KArgs& ka = plan.ka;
  const CArgs& ca = plan.ca;
  if (!c->dom.fd) {
    // QUICK_FLUX (implies Nnode == 3, vicgpu_create): one kernel per step, enqueued without blocking
    for (int s = step0; s < step0 + nsteps; s++) {
      const int i = (s - step0) % per;
      set_step_inputs(c, ka, s);
      HIPCHK(c, hipEventRecord(c->ev[2 * i], c->stream));
      HIPCHK(c, launch_hru<3>(ka, c->stream, true, c->dom.any_glacier));
      HIPCHK(c, hipEventRecord(c->ev[2 * i + 1], c->stream));
      hipLaunchKernelGGL(vic_cell_reduce, dim3((c->dom.ncell + 255) / 256), dim3(256), 0, c->stream, ca);
      HIPCHK(c, hipGetLastError());
      if (c->dom.put_on) HIPCHK(c, launch_put_data(c, c->stream, 0, c->dom.ncell, s));
      c->steps_done++;
      if (records && i == per - 1) {
        const int re = records_emit(c, &c->err, 0, c->stream, 0, c->dom.ncell, (s - step0) / per);
        if (re != VICGPU_OK) return re;
      }
    }
    c->ev_used = per;
    c->ev_steps = per;
    return VICGPU_OK;
  }
  // finite-difference pipeline: every chunk runs all nsteps on its own stream (ordered after what is queued on the
  // context's stream, which in turn waits for every chunk before anything queued later)
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  for (FdChunk& ch : c->dom.chunks) {
    HIPCHK(c, hipStreamWaitEvent(ch.stream, c->ev[0], 0));
    ch.status = VICGPU_OK;
    ch.err.clear();
  }
  if (c->dom.chunks.size() == 1) c->dom.chunks[0].status = fd_chunk_run(plan, &c->dom.chunks[0]);
  else {
    std::vector<std::thread> th;
    for (FdChunk& ch : c->dom.chunks) th.emplace_back([&plan, &ch]() { ch.status = fd_chunk_run(plan, &ch); });
    for (std::thread& t : th) t.join();
  }
  int status = VICGPU_OK;
  for (FdChunk& ch : c->dom.chunks) {
    if (ch.status != VICGPU_OK && status == VICGPU_OK) { status = ch.status; c->err = ch.err; }
  }
  if (status != VICGPU_OK) {
    for (FdChunk& ch : c->dom.chunks) HIPIGN(hipStreamSynchronize(ch.stream));
    return status;
  }
  for (FdChunk& ch : c->dom.chunks) HIPCHK(c, hipStreamWaitEvent(c->stream, ch.done, 0));
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  c->ev_used = 1;
  c->ev_steps = per;
  c->steps_done += nsteps;
  return VICGPU_OK;
}

int vicgpu_step(vicgpu_ctx* c, int step0, int nsteps) {
  if (!c) return VICGPU_ERR_ARG;
  if (!c->dom.domain_ready || !c->d_veglib || !c->d_forcing || c->chunk_steps <= 0) return VICGPU_ERR_STATE;
  if (step0 < 0 || nsteps <= 0 || step0 + nsteps > c->chunk_steps) return VICGPU_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  return step_impl(c, step0, nsteps, 0);
}

int vicgpu_synchronize(vicgpu_ctx* c) {
  if (!c) return VICGPU_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->rec.dl) HIPCHK(c, hipStreamSynchronize(c->rec.dl));      // the output records queued behind the steps (vicgpu_run_records)
  return VICGPU_OK;
}

int vicgpu_last_kernel_ms(vicgpu_ctx* c, double* ms_per_launch, int* nlaunch) {
  if (!c || !ms_per_launch) return VICGPU_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  double tot = 0;
  for (int i = 0; i < c->ev_used; i++) {
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev[2 * i], c->ev[2 * i + 1]));
    tot += ms;
  }
  *ms_per_launch = c->ev_steps ? tot / c->ev_steps : 0.0;
  if (nlaunch) *nlaunch = c->ev_steps;
  return VICGPU_OK;
}

int vicgpu_get_fluxes(vicgpu_ctx* c, double* flux) { return c ? d2h(c, flux, c->dom.d_flux) : VICGPU_ERR_ARG; }
int vicgpu_get_cell_outputs(vicgpu_ctx* c, double* o) { return c ? d2h(c, o, c->dom.d_cell_out) : VICGPU_ERR_ARG; }
int vicgpu_get_accum(vicgpu_ctx* c, double* a) { return c ? d2h(c, a, c->dom.d_accum) : VICGPU_ERR_ARG; }
int vicgpu_get_cell_errors(vicgpu_ctx* c, int* f) { return c ? d2h(c, f, c->dom.d_cell_err) : VICGPU_ERR_ARG; }

int vicgpu_reset_accum(vicgpu_ctx* c) {
  if (!c || !c->dom.d_accum) return VICGPU_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, c->dom.d_accum.fill(c->stream, 0));
  HIPCHK(c, c->dom.d_cell_err.fill(c->stream, 0));
  return VICGPU_OK;
}

// ---- cell validity: cell.isValid and CONTINUEONERROR (vicNl.c:429, 521, 545-559)
int vicgpu_set_retire_on_error(vicgpu_ctx* c, int mask) {
  const int all = VICGPU_CELLERR_SOLVER | VICGPU_CELLERR_AERO | VICGPU_CELLERR_NODES | VICGPU_CELLERR_NAN;
  if (!c || (mask & ~all)) return VICGPU_ERR_ARG;
  c->retire_mask = mask;           // read when the next steps are queued; the table keeps what earlier steps left in it
  return VICGPU_OK;
}

int vicgpu_set_cell_valid(vicgpu_ctx* c, const int* valid) {
  if (!c || !valid) return VICGPU_ERR_ARG;
  if (!c->dom.domain_ready) return VICGPU_ERR_STATE;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));      // the steps queued so far ran on the table as it was
  std::vector<int> w(c->dom.ncell);
  bool any_invalid = false;
  for (size_t i = 0; i < w.size(); i++) {
    w[i] = valid[i] ? CELL_VALID : CELL_SKIP;
    any_invalid = any_invalid || !valid[i];
  }
  HIPCHK(c, c->dom.d_valid.upload(c->stream, w.data()));
  c->dom.valid_live = any_invalid;
  return VICGPU_OK;
}

int vicgpu_get_cell_valid(vicgpu_ctx* c, int* valid) {
  if (!c || !valid) return VICGPU_ERR_ARG;
  if (!c->dom.domain_ready) return VICGPU_ERR_STATE;
  const int r = d2h(c, valid, c->dom.d_valid);
  if (r != VICGPU_OK) return r;
  for (int i = 0; i < c->dom.ncell; i++) valid[i] = valid[i] == CELL_VALID ? 1 : 0;
  return VICGPU_OK;
}

static int glacier_fit_impl(vicgpu_ctx* c, double* eq, int reset, int ld) {
  if (!c || !c->dom.d_cp || !eq || ld < c->dom.ncell) return VICGPU_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  DevBuf<double> d_eq;
  HIPCHK(c, d_eq.alloc((size_t)GMB_NROW * c->dom.ncell));
  GArgs g;
  g.o = c->o; g.ncell = c->dom.ncell; g.nhru = c->dom.nhru; g.reset = reset ? 1 : 0; g.cell_params = c->dom.d_cp; g.cell_off = c->dom.d_cell_off;
  g.cell_list = c->dom.d_cell_list; g.hpi = c->dom.d_hpi; g.sd = c->dom.d_sd; g.eq = d_eq;
  g.valid = valid_table(c);
  hipLaunchKernelGGL(vic_glacier_fit, dim3((c->dom.ncell + 63) / 64), dim3(64), 0, c->stream, g);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, d_eq.download_cols(c->stream, eq, ld, GMB_NROW, c->dom.ncell));
  return VICGPU_OK;
}
int vicgpu_glacier_mass_balance_fit(vicgpu_ctx* c, double* eq, int reset) { return c ? glacier_fit_impl(c, eq, reset, c->dom.ncell) : VICGPU_ERR_ARG; }

int vicgpu_debug_pure(vicgpu_ctx* c, int fn, int n, const double* in, double* out) {
  if (!c || !c->dom.d_cp || fn < 0 || fn >= VICGPU_PURE_NFN_DEVICE || n <= 0 || !in || !out) return VICGPU_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  DevBuf<double> d_in, d_out;
  HIPCHK(c, d_in.alloc((size_t)n * VICGPU_PURE_NIN));
  HIPCHK(c, d_out.alloc(n));
  HIPCHK(c, d_in.upload(c->stream, in));
  DArgs d;
  d.o = c->o; d.cell_params = c->dom.d_cp; d.ncell = c->dom.ncell; d.fn = fn; d.n = n; d.in = d_in; d.out = d_out;
  hipLaunchKernelGGL(vic_debug_pure, dim3((n + 63) / 64), dim3(64), 0, c->stream, d);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, d_out.download(c->stream, out));
  return VICGPU_OK;
}

int vicgpu_debug_root_brent(vicgpu_ctx* c, int mode, int n, const double* bounds, const int* off, const double* fvals,
                            double* xreq, double* out) {
  if (!c || (mode != VICGPU_BRENT_FULL && mode != VICGPU_BRENT_LEAN) || n <= 0 || !bounds || !off || !out) return VICGPU_ERR_ARG;
  if (off[0] != 0) return VICGPU_ERR_ARG;
  for (int i = 0; i < n; i++) if (off[i + 1] < off[i]) return VICGPU_ERR_ARG;
  const int nv = off[n];
  if (nv > 0 && (!fvals || !xreq)) return VICGPU_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  DevBuf<double> d_bounds, d_f, d_x, d_out;
  DevBuf<int> d_off;
  const size_t nvs = nv > 0 ? (size_t)nv : 1;
  HIPCHK(c, d_bounds.alloc(2 * (size_t)n));
  HIPCHK(c, d_off.alloc((size_t)n + 1));
  HIPCHK(c, d_f.alloc(nvs));
  HIPCHK(c, d_x.alloc(nvs));
  HIPCHK(c, d_out.alloc((size_t)n * VICGPU_BRENT_NOUT));
  HIPCHK(c, d_bounds.upload(c->stream, bounds));
  HIPCHK(c, d_off.upload(c->stream, off));
  if (nv > 0) HIPCHK(c, d_f.upload(c->stream, fvals));
  RBArgs d;
  d.n = n; d.bounds = d_bounds; d.off = d_off; d.fvals = d_f; d.xreq = d_x; d.out = d_out;
  const dim3 grid((n + 63) / 64), block(64);
  if (mode == VICGPU_BRENT_FULL) hipLaunchKernelGGL((vic_debug_root_brent<Brent>), grid, block, 0, c->stream, d);
  else hipLaunchKernelGGL((vic_debug_root_brent<BrentLean>), grid, block, 0, c->stream, d);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (nv > 0) HIPCHK(c, d_x.download(c->stream, xreq));
  HIPCHK(c, d_out.download(c->stream, out));
  return VICGPU_OK;
}

int vicgpu_debug_node_root(vicgpu_ctx* c, int mode, int n, const double* in, double* out) {
  if (!c || mode < 0 || mode > (VICGPU_NODE_NODE1 | VICGPU_NODE_NEWTON | VICGPU_NODE_EXP_TRANS) || n <= 0 || !in || !out) return VICGPU_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  DevBuf<double> d_in, d_out;
  HIPCHK(c, d_in.alloc((size_t)n * VICGPU_NODE_NIN));
  HIPCHK(c, d_out.alloc((size_t)n * VICGPU_NODE_NOUT));
  HIPCHK(c, d_in.upload(c->stream, in));
  NRArgs d;
  d.n = n; d.EXP_TRANS = (mode & VICGPU_NODE_EXP_TRANS) != 0; d.in = d_in; d.out = d_out;
  const dim3 grid((n + 63) / 64), block(64);
  switch (mode & (VICGPU_NODE_NODE1 | VICGPU_NODE_NEWTON)) {
    case 0: hipLaunchKernelGGL((vic_debug_node_root<false, false>), grid, block, 0, c->stream, d); break;
    case VICGPU_NODE_NODE1: hipLaunchKernelGGL((vic_debug_node_root<true, false>), grid, block, 0, c->stream, d); break;
    case VICGPU_NODE_NEWTON: hipLaunchKernelGGL((vic_debug_node_root<false, true>), grid, block, 0, c->stream, d); break;
    default: hipLaunchKernelGGL((vic_debug_node_root<true, true>), grid, block, 0, c->stream, d); break;
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, d_out.download(c->stream, out));
  return VICGPU_OK;
}

int vicgpu_set_stream(vicgpu_ctx* c, void* hip_stream) {
  if (!c) return VICGPU_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (hip_stream) c->stream.borrow((hipStream_t)hip_stream);
  else if (c->stream.borrowed()) HIPCHK(c, c->stream.create());
  return VICGPU_OK;
}

int vicgpu_set_write_fluxes(vicgpu_ctx* c, int on) {
  if (!c) return VICGPU_ERR_ARG;
  c->write_fluxes = on ? 1 : 0;
  return VICGPU_OK;
}

void* vicgpu_device_ptr(vicgpu_ctx* c, int which) {
  if (!c) return nullptr;
  switch (which) {
    case VICGPU_PTR_STATE_D: return c->dom.d_sd;
    case VICGPU_PTR_STATE_I: return c->dom.d_si;
    case VICGPU_PTR_FLUX: return c->dom.d_flux;
    case VICGPU_PTR_FORCING: return c->d_forcing;
    case VICGPU_PTR_ACCUM: return c->dom.d_accum;
    case VICGPU_PTR_CELL_OUT: return c->dom.d_cell_out;
    default: return nullptr;
  }
}

static int state_records(vicgpu_ctx* c, double* host, bool gather) {
  if (!c || !host) return VICGPU_ERR_ARG;
  if (!c->dom.domain_ready) return VICGPU_ERR_STATE;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t L = VICGPU_SR_LEN(c->opt.Nnode), nhru = c->dom.nhru;
  DevBuf<double> d_rec;
  DevBuf<int> d_mis;
  HIPCHK(c, d_rec.alloc(L * nhru));
  HIPCHK(c, d_mis.alloc_fill(1, 0, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!gather) HIPCHK(c, d_rec.upload(c->stream, host));
  RArgs a;
  a.nhru = c->dom.nhru; a.Nn = c->opt.Nnode; a.cell_list = c->dom.d_cell_list; a.hpi = c->dom.d_hpi; a.sd = c->dom.d_sd; a.si = c->dom.d_si;
  a.flux = c->dom.d_flux; a.rec = d_rec; a.mismatch = d_mis;
  if (!gather) {
    // read side, pass 1: validate every record before anything is scattered (a reader that throws changes nothing)
    std::vector<int> hpi_band(nhru), hpi_veg(nhru), list(nhru);
    HIPCHK(c, c->dom.d_hpi.download(c->stream, hpi_band.data(), HPI_BAND * nhru, nhru));
    HIPCHK(c, c->dom.d_hpi.download(c->stream, hpi_veg.data(), HPI_VEG_CLASS * nhru, nhru));
    HIPCHK(c, c->dom.d_cell_list.download(c->stream, list.data()));
    for (size_t k = 0; k < nhru; k++) {
      c->err = check_state_record(host + k * L, k, hpi_band[list[k]], hpi_veg[list[k]]);
      if (!c->err.empty()) return VICGPU_ERR_ARG;
    }
  }
  const unsigned nblk = (unsigned)((c->dom.nhru + 255) / 256);
  if (gather) hipLaunchKernelGGL(vic_state_records<true>, dim3(nblk), dim3(256), 0, c->stream, a);
  else hipLaunchKernelGGL(vic_state_records<false>, dim3(nblk), dim3(256), 0, c->stream, a);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (gather) HIPCHK(c, d_rec.download(c->stream, host));
  return VICGPU_OK;
}
int vicgpu_get_state_records(vicgpu_ctx* c, double* rec) { return state_records(c, rec, true); }
int vicgpu_set_state_records(vicgpu_ctx* c, const double* rec) { return state_records(c, const_cast<double*>(rec), false); }

// ------------------------------------------------------------------------------------------------ put_data (vicgpu_out.h)
int vicgpu_out_nvar(void) { return VOUT_NVAR; }
const char* vicgpu_out_var_name(int id) { return (id >= 0 && id < VOUT_NVAR) ? vout_name_host[id] : nullptr; }
int vicgpu_out_var_id(const char* name) {
  if (!name) return -1;
  for (int v = 0; v < VOUT_NVAR; v++)
    if (strcmp(name, vout_name_host[v]) == 0) return v;
  return -1;
}
int vicgpu_out_var_kind(int id) { return (id >= 0 && id < VOUT_NVAR) ? vout_kind_host[id] : -1; }
int vicgpu_out_var_agg(int id) { return (id >= 0 && id < VOUT_NVAR) ? vout_agg_host[id] : -1; }
int vicgpu_out_var_nelem(const vicgpu_options* opt, int id) {
  if (!opt || id < 0 || id >= VOUT_NVAR) return -1;
  return vout_kind_nelem(vout_kind_host[id], opt->Nnode, opt->Nband, opt->FROZEN_SOIL);
}

int vicgpu_put_data_config(vicgpu_ctx* c, int out_step_ratio) {
  if (!c || out_step_ratio < 1) return VICGPU_ERR_ARG;
  if (!c->dom.domain_ready || !c->d_veglib) return VICGPU_ERR_STATE;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  free_records(c);                 // a records configuration belongs to the output layout it was made for
  // the tree-line adjustment factor of every band (a function of the domain and the vegetation library's overstory flags)
  hipLaunchKernelGGL(vic_derive_tree_adjust, dim3((c->dom.ncell + 63) / 64), dim3(64), 0, c->stream, c->dom.d_cp, c->dom.ncell, c->dom.nhru, c->opt.Nnode,
                     c->opt.Nband, c->dom.d_cell_off, c->dom.d_cell_list, c->dom.d_hpi, c->dom.d_hpd, c->d_veglib);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  int r = 0;
  for (int v = 0; v < VOUT_NVAR; v++) {
    c->dom.out_lay.off[v] = r; c->dom.out_lay.agg[v] = vout_agg_host[v];
    r += vout_kind_nelem(vout_kind_host[v], c->opt.Nnode, c->opt.Nband, c->opt.FROZEN_SOIL);
  }
  c->dom.out_lay.off[VOUT_NVAR] = r;
  c->dom.out_nrow = r;
  c->out_step_ratio = out_step_ratio;
  std::vector<unsigned char> rowagg(r);
  for (int v = 0; v < VOUT_NVAR; v++) {
    const bool by_finish = (v == VOUT_AERO_RESIST || v == VOUT_AERO_RESIST1 || v == VOUT_AERO_RESIST2);   // vic_put_finish
    for (int k = c->dom.out_lay.off[v]; k < c->dom.out_lay.off[v + 1]; k++) rowagg[k] = (unsigned char)(by_finish ? VOUT_AGG_SKIP : vout_agg_host[v]);
  }
  c->dom.put_on = false;
  if (!c->dom.d_out_data) {        // all four tables or none: a failed call leaves nothing half-present for the next one
    DevBuf<double> out_data, out_agg, pb;
    DevBuf<unsigned char> d_rowagg;
    HIPCHK(c, out_data.alloc((size_t)r * c->dom.ncell));
    HIPCHK(c, out_agg.alloc((size_t)r * c->dom.ncell));
    HIPCHK(c, pb.alloc((size_t)PBX_NROW * c->dom.ncell));                  // the public PB_NROW rows + put_data's own
    HIPCHK(c, d_rowagg.alloc(r));
    c->dom.d_out_data = std::move(out_data); c->dom.d_out_agg = std::move(out_agg); c->dom.d_pb = std::move(pb); c->dom.d_rowagg = std::move(d_rowagg);
  }
  HIPCHK(c, c->dom.d_rowagg.upload(c->stream, rowagg.data()));
  HIPCHK(c, c->dom.d_out_data.fill(c->stream, 0));
  HIPCHK(c, c->dom.d_out_agg.fill(c->stream, 0));
  HIPCHK(c, c->dom.d_pb.fill(c->stream, 0));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->dom.put_on = true;
  return VICGPU_OK;
}

int vicgpu_put_data_init(vicgpu_ctx* c) {
  if (!c) return VICGPU_ERR_ARG;
  if (!c->dom.domain_ready || !c->dom.put_on || !c->d_veglib) return VICGPU_ERR_STATE;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, launch_put_data(c, c->stream, 0, c->dom.ncell, -1));
  return VICGPU_OK;
}

// the rows of the listed variables, in the order asked for; -1 when an id is out of range
static int out_rows(const vicgpu_ctx* c, int nvar, const int* ids, std::vector<int>& rows) {
  rows.clear();
  for (int k = 0; k < nvar; k++) {
    if (ids[k] < 0 || ids[k] >= VOUT_NVAR) return -1;
    for (int r = c->dom.out_lay.off[ids[k]]; r < c->dom.out_lay.off[ids[k] + 1]; r++) rows.push_back(r);
  }
  return (int)rows.size();
}

// ld: cells per row of `out` (c->dom.ncell, or the global cell count when a group writes one shard's columns)
static int get_outputs_impl(vicgpu_ctx* c, int nvar, const int* var_ids, float* out, int reset, int ld) {
  if (!c || nvar < 0 || (nvar > 0 && (!var_ids || !out)) || ld < c->dom.ncell) return VICGPU_ERR_ARG;
  if (!c->dom.put_on) return VICGPU_ERR_STATE;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<int> rows;
  const int nr = out_rows(c, nvar, var_ids, rows);
  if (nr < 0) return VICGPU_ERR_ARG;
  if (nr > 0) {
    DevBuf<int> d_rows;
    DevBuf<float> d_f;
    const size_t n = (size_t)nr * c->dom.ncell;
    HIPCHK(c, d_rows.alloc(nr));
    HIPCHK(c, d_f.alloc(n));
    HIPCHK(c, d_rows.upload(c->stream, rows.data()));
    const int* rows_arg = d_rows;
    float* f_arg = d_f;
    hipLaunchKernelGGL(vic_out_rows_f32, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->dom.d_out_agg, rows_arg, nr,
                       c->dom.ncell, f_arg);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, d_f.download_cols(c->stream, out, ld, nr, c->dom.ncell));
  }
  if (reset) {                     // vicNl.c:599-606
    HIPCHK(c, c->dom.d_out_agg.fill(c->stream, 0));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return VICGPU_OK;
}
int vicgpu_get_outputs(vicgpu_ctx* c, int nvar, const int* var_ids, float* out, int reset) {
  return c ? get_outputs_impl(c, nvar, var_ids, out, reset, c->dom.ncell) : VICGPU_ERR_ARG;
}

int vicgpu_get_output_data(vicgpu_ctx* c, int nvar, const int* var_ids, int which, double* out) {
  if (!c || nvar <= 0 || !var_ids || !out || which < 0 || which > 1) return VICGPU_ERR_ARG;
  if (!c->dom.put_on) return VICGPU_ERR_STATE;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const DevBuf<double>& table = which ? c->dom.d_out_agg : c->dom.d_out_data;
  size_t at = 0;
  for (int k = 0; k < nvar; k++) {
    if (var_ids[k] < 0 || var_ids[k] >= VOUT_NVAR) return VICGPU_ERR_ARG;
    const int r0 = c->dom.out_lay.off[var_ids[k]], ne = c->dom.out_lay.off[var_ids[k] + 1] - r0;
    HIPCHK(c, table.download(c->stream, out + at, (size_t)r0 * c->dom.ncell, (size_t)ne * c->dom.ncell));
    at += (size_t)ne * c->dom.ncell;
  }
  return VICGPU_OK;
}

int vicgpu_get_balance(vicgpu_ctx* c, double* pb) {
  if (!c || !pb) return VICGPU_ERR_ARG;
  if (!c->dom.put_on) return VICGPU_ERR_STATE;
  return d2h(c, pb, c->dom.d_pb, (size_t)PB_NROW * c->dom.ncell);      // the public rows of PBX_NROW
}

int vicgpu_set_fluxes(vicgpu_ctx* c, const double* flux) {
  if (!c || !flux) return VICGPU_ERR_ARG;
  if (!c->dom.domain_ready) return VICGPU_ERR_STATE;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, c->dom.d_flux.upload(c->stream, flux));
  return VICGPU_OK;
}

// ---- model state copied between cells on the device (vic_copy_cells.hpp): ensemble seeding, resampling, rollback
int vicgpu_copy_cells(vicgpu_ctx* c, int n, const int* dst_cell, const int* src_cell, int what) {
  if (!c || n < 0 || (n > 0 && (!dst_cell || !src_cell))) return VICGPU_ERR_ARG;
  if (what == 0 || (what & ~(VICGPU_COPY_STATE | VICGPU_COPY_BALANCE))) return VICGPU_ERR_ARG;
  if (!c->dom.domain_ready) return VICGPU_ERR_STATE;
  if ((what & VICGPU_COPY_BALANCE) && !c->dom.put_on) return VICGPU_ERR_STATE;
  const Domain& d = c->dom;
  // every pair is checked here, before the first write
  const CopyPlan p = plan_cell_copy(d.ncell, d.nhru, d.cell_off.data(), d.cell_list.data(), d.copy_key.data(), COPY_NKEY, n, dst_cell, src_cell);
  if (p.fault != COPY_OK) { c->err = copy_fault_text(p); return VICGPU_ERR_ARG; }
  if (p.cell.size() == 0) return VICGPU_OK;        // n == 0, or identity pairs only
  HIPCHK(c, hipSetDevice(c->device));
  const int nh = (int)p.hru.size(), nc = (int)p.cell.size();
  // what the call allocates, before anything is queued: the pairs [HRU dst][HRU src][cell dst][cell src], and the stage
  DevBuf<int> idx;
  DevBuf<double> stage;
  HIPCHK(c, idx.alloc(2 * ((size_t)nh + nc)));
  const size_t budget = (size_t)c->tune.copy_stage_mb << 20;
  if (!p.direct) {
    size_t bytes = 0;
    for (int t = 0; t < COPY_NTABLE; t++)
      HIPIGN(copy_table(c, t, what, [&](auto* table, int nrow, size_t, bool per_cell) {
        const size_t np = per_cell ? nc : nh, eb = sizeof(*table);
        bytes = std::max(bytes, (size_t)rows_per_pass(budget, np, eb, nrow) * np * eb);
        return hipSuccess;
      }));
    HIPCHK(c, stage.alloc((bytes + 7) / 8));
  }
  std::vector<int> h;
  h.reserve(idx.size());
  h.insert(h.end(), p.hru.dst.begin(), p.hru.dst.end()); h.insert(h.end(), p.hru.src.begin(), p.hru.src.end());
  h.insert(h.end(), p.cell.dst.begin(), p.cell.dst.end()); h.insert(h.end(), p.cell.src.begin(), p.cell.src.end());
  // the context's stream follows every step queued so far (with the finite-difference pipeline it waits for every chunk's
  // `done` event, step_impl) and precedes every step queued later: the copy is queued there
  StreamTimer timer;               // tuning (VICGPU_STATS): the kernels' own time
  HIPCHK(c, timer.create(c->tune.stats));
  HIPCHK(c, idx.upload(c->stream, h.data()));
  HIPCHK(c, timer.begin(c->stream));
  size_t moved = 0;                // bytes the tables take
  for (int t = 0; t < COPY_NTABLE; t++) {
    const hipError_t queued = copy_table(c, t, what, [&](auto* table, int nrow, size_t ld, bool per_cell) {
      using T = typename std::remove_pointer<decltype(table)>::type;
      const int np = per_cell ? nc : nh;
      const int* dst = idx.get() + (per_cell ? 2 * (size_t)nh : 0);
      const int* src = dst + np;
      moved += sizeof(T) * nrow * np;
      if (p.direct) return copy_direct<T>(c->stream, table, ld, nrow, dst, src, np);
      return copy_staged<T>(c->stream, table, ld, nrow, dst, src, np, reinterpret_cast<T*>(stage.get()), rows_per_pass(budget, np, sizeof(T), nrow));
    });
    HIPCHK(c, queued);
  }
  HIPCHK(c, timer.end(c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));      // the pairs and the stage are released when the call returns
  float ms = 0;
  if (timer.elapsed(&ms))
    fprintf(stderr, "[vicgpu] copy_cells: %d cell pairs, %d HRU pairs, %s, %zu bytes written: %.4f ms on the device\n", nc, nh,
            p.direct ? "direct" : "staged", moved, ms);
  return VICGPU_OK;
}

// ---- cell and HRU parameters updated in place (vic_params.hpp): calibration generations, sensitivity sweeps, glacier coupling
// One call on the caller's rows of d_cp (per_cell) or on d_hpd.  Everything the call allocates is allocated before the first
// write: one list block [rows][columns, when listed][cells whose tree-line rows are re-derived, when listed] and the stage.
static int update_params_impl(vicgpu_ctx* c, bool per_cell, int nrow, const int* rows, int n, const int* cols, const double* values) {
  if (!c || nrow < 0 || n < 0) return VICGPU_ERR_ARG;
  if (!c->dom.domain_ready) return VICGPU_ERR_STATE;
  if (nrow == 0 || n == 0) return VICGPU_OK;
  if (!rows || !values) return VICGPU_ERR_ARG;
  Domain& d = c->dom;
  const int Nn = c->opt.Nnode, Nb = c->opt.Nband;
  const char* name = per_cell ? "update_cell_params" : "update_hru_params";
  const int table_rows = per_cell ? (int)VICGPU_CP_NROW(Nn, Nb) : (int)HPD_NROW;
  const int ncol = per_cell ? d.ncell : d.nhru;
  // every row and column is checked here, before the first write
  const ParamFault f = check_param_update(table_rows, ncol, nrow, rows, n, cols);
  if (f.rule != PARAM_OK) {
    c->err = param_fault_message(name, f);
    return VICGPU_ERR_ARG;
  }
  // the cells whose tree-line rows follow: the listed cells, or the owners of the listed HRUs; with a dense call, all
  const bool tree = d.put_on && c->d_veglib;
  std::vector<int> owners;
  if (!per_cell && cols && tree) owners = param_owner_cells(d.ncell, d.nhru, d.cell_off.data(), d.cell_list.data(), n, cols);
  HIPCHK(c, hipSetDevice(c->device));
  const size_t nlist = cols ? (size_t)n : 0;
  DevBuf<int> lists;
  DevBuf<double> stage;
  HIPCHK(c, lists.alloc((size_t)nrow + nlist + owners.size()));
  const int rpp = rows_per_pass((size_t)c->tune.copy_stage_mb << 20, (size_t)n, sizeof(double), nrow);
  HIPCHK(c, stage.alloc((size_t)rpp * n));
  std::vector<int> h(rows, rows + nrow);
  if (cols) h.insert(h.end(), cols, cols + n);
  h.insert(h.end(), owners.begin(), owners.end());
  const int* d_rows = lists.get();
  const int* d_cols = cols ? lists.get() + nrow : nullptr;
  const int* d_owners = lists.get() + nrow + nlist;
  // the context's stream follows every step queued so far (with the finite-difference pipeline it waits for every chunk's
  // `done` event, step_impl) and precedes every step queued later: the update is queued there
  StreamTimer timer;               // tuning (VICGPU_STATS): the call's time on the stream, uploads of the passes included
  HIPCHK(c, timer.create(c->tune.stats));
  HIPCHK(c, lists.upload(c->stream, h.data()));
  HIPCHK(c, timer.begin(c->stream));
  int nderived = 0;
  if (per_cell) {
    HIPCHK(c, rows_put_staged<double>(c->stream, d.d_cp, (size_t)d.ncell, d_rows, nrow, d_cols, n, values, stage, rpp));
    HIPCHK(c, derive_cell_params_listed(c->stream, d.d_cp, d.ncell, Nn, Nb, d_cols, n));
    if (tree)
      HIPCHK(c, derive_tree_adjust_listed(c->stream, d.d_cp, d.ncell, d.nhru, Nn, Nb, d.d_cell_off, d.d_cell_list, d.d_hpi, d.d_hpd, c->d_veglib, d_cols, n));
    nderived = n;
  } else {
    HIPCHK(c, rows_put_staged<double>(c->stream, d.d_hpd, (size_t)d.nhru, d_rows, nrow, d_cols, n, values, stage, rpp));
    if (tree) {
      nderived = cols ? (int)owners.size() : d.ncell;
      HIPCHK(c, derive_tree_adjust_listed(c->stream, d.d_cp, d.ncell, d.nhru, Nn, Nb, d.d_cell_off, d.d_cell_list, d.d_hpi, d.d_hpd, c->d_veglib,
                                          cols ? d_owners : nullptr, nderived));
    }
  }
  HIPCHK(c, timer.end(c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));      // the lists and the stage are released when the call returns
  float ms = 0;
  if (timer.elapsed(&ms))
    fprintf(stderr, "[vicgpu] %s: %d rows x %d %s, %s, %d passes, %zu bytes written, rows re-derived for %d cells: %.4f ms on the stream\n", name,
            nrow, n, per_cell ? "cells" : "HRUs", cols ? "listed" : "dense", (nrow + rpp - 1) / rpp, sizeof(double) * nrow * n, nderived, ms);
  return VICGPU_OK;
}

int vicgpu_update_cell_params(vicgpu_ctx* c, int nrow, const int* rows, int n, const int* cells, const double* values) {
  return update_params_impl(c, true, nrow, rows, n, cells, values);
}

int vicgpu_update_hru_params(vicgpu_ctx* c, int nrow, const int* rows, int n, const int* hrus, const double* values) {
  return update_params_impl(c, false, nrow, rows, n, hrus, values);
}

// the caller's rows of the cell parameter table (the library's appended rows stay inside) into a table whose rows are ld cells wide
static int get_cell_params_impl(vicgpu_ctx* c, double* cell_params, int ld) {
  if (!c || !cell_params) return VICGPU_ERR_ARG;
  if (!c->dom.domain_ready) return VICGPU_ERR_STATE;
  return d2h_cols(c, cell_params, ld, c->dom.d_cp, (int)VICGPU_CP_NROW(c->opt.Nnode, c->opt.Nband));
}

int vicgpu_get_cell_params(vicgpu_ctx* c, double* cell_params) { return get_cell_params_impl(c, cell_params, c ? c->dom.ncell : 0); }

int vicgpu_get_hru_params(vicgpu_ctx* c, double* hru_dparams) {
  if (!c || !hru_dparams) return VICGPU_ERR_ARG;
  if (!c->dom.domain_ready) return VICGPU_ERR_STATE;
  return d2h(c, hru_dparams, c->dom.d_hpd);
}

// ---- model state read and changed in place, its dependent soil rows re-derived (vic_state_update.hpp): the analysis update
// One call on listed rows of d_sd or d_si.  Everything it allocates is allocated before anything is queued: one list block
// [rows][HRUs, when listed] and the stage.  GET: values is written; otherwise read.
}  // extern "C": a template

template <typename T>
static int state_rows_impl(vicgpu_ctx* c, const char* name, DevBuf<T> Domain::*table, int table_rows, int op, int nrow, const int* rows, int n,
                           const int* hrus, T* values) {
  if (!c->dom.domain_ready) return VICGPU_ERR_STATE;
  if (nrow == 0 || n == 0) return VICGPU_OK;
  if (!rows || !values) return VICGPU_ERR_ARG;
  Domain& d = c->dom;
  // every row and column is checked here, before the first write
  const ParamFault f = check_param_update(table_rows, d.nhru, nrow, rows, n, hrus);
  if (f.rule != PARAM_OK) {
    c->err = param_fault_message(name, f);
    return VICGPU_ERR_ARG;
  }
  HIPCHK(c, hipSetDevice(c->device));
  DevBuf<int> lists;
  DevBuf<T> stage;
  HIPCHK(c, lists.alloc((size_t)nrow + (hrus ? (size_t)n : 0)));
  const int rpp = rows_per_pass((size_t)c->tune.copy_stage_mb << 20, (size_t)n, sizeof(T), nrow);
  HIPCHK(c, stage.alloc((size_t)rpp * n));
  std::vector<int> h(rows, rows + nrow);
  if (hrus) h.insert(h.end(), hrus, hrus + n);
  const int* d_rows = lists.get();
  const int* d_hrus = hrus ? lists.get() + nrow : nullptr;
  // the context's stream follows every step queued so far (with the finite-difference pipeline it waits for every chunk's
  // `done` event, step_impl) and precedes every step queued later
  StreamTimer timer;               // tuning (VICGPU_STATS): the call's time on the stream, the copies of the passes included
  HIPCHK(c, timer.create(c->tune.stats));
  HIPCHK(c, lists.upload(c->stream, h.data()));
  HIPCHK(c, timer.begin(c->stream));
  T* tab = (d.*table).get();
  if (op == ROWS_GET) HIPCHK(c, rows_get_staged<T>(c->stream, tab, (size_t)d.nhru, d_rows, nrow, d_hrus, n, values, stage, rpp));
  else HIPCHK(c, rows_put_staged<T>(c->stream, tab, (size_t)d.nhru, d_rows, nrow, d_hrus, n, values, stage, rpp, op == ROWS_ADD));
  HIPCHK(c, timer.end(c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));      // the lists and the stage are released when the call returns
  float ms = 0;
  if (timer.elapsed(&ms))
    fprintf(stderr, "[vicgpu] %s: %s, %d rows x %d HRUs, %s, %d passes, %zu bytes: %.4f ms on the stream\n", name,
            op == ROWS_GET ? "get" : op == ROWS_SET ? "set" : "add", nrow, n, hrus ? "listed" : "dense", (nrow + rpp - 1) / rpp, sizeof(T) * nrow * n, ms);
  return VICGPU_OK;
}

extern "C" {

int vicgpu_get_state_rows(vicgpu_ctx* c, int nrow, const int* rows, int n, const int* hrus, double* values) {
  if (!c || nrow < 0 || n < 0) return VICGPU_ERR_ARG;
  return state_rows_impl<double>(c, "get_state_rows", &Domain::d_sd, (int)VICGPU_SD_NROW(c->o.Nnode), ROWS_GET, nrow, rows, n, hrus, values);
}

int vicgpu_get_state_rows_i(vicgpu_ctx* c, int nrow, const int* rows, int n, const int* hrus, int* values) {
  if (!c || nrow < 0 || n < 0) return VICGPU_ERR_ARG;
  return state_rows_impl<int>(c, "get_state_rows_i", &Domain::d_si, (int)VICGPU_SI_NROW(c->o.Nnode), ROWS_GET, nrow, rows, n, hrus, values);
}

int vicgpu_update_state(vicgpu_ctx* c, int nrow, const int* rows, int n, const int* hrus, const double* values, int mode) {
  if (!c || nrow < 0 || n < 0 || (mode != VICGPU_STATE_SET && mode != VICGPU_STATE_ADD)) return VICGPU_ERR_ARG;
  return state_rows_impl<double>(c, "update_state", &Domain::d_sd, (int)VICGPU_SD_NROW(c->o.Nnode), mode == VICGPU_STATE_ADD ? ROWS_ADD : ROWS_SET, nrow,
                                 rows, n, hrus, const_cast<double*>(values));
}

int vicgpu_update_state_i(vicgpu_ctx* c, int nrow, const int* rows, int n, const int* hrus, const int* values) {
  if (!c || nrow < 0 || n < 0) return VICGPU_ERR_ARG;
  return state_rows_impl<int>(c, "update_state_i", &Domain::d_si, (int)VICGPU_SI_NROW(c->o.Nnode), ROWS_SET, nrow, rows, n, hrus, const_cast<int*>(values));
}

int vicgpu_derive_soil_state(vicgpu_ctx* c, int n, const int* hrus, int what) {
  if (!c || n < 0) return VICGPU_ERR_ARG;
  const int rule = check_derive_what(what, c->o.GLACIER_DYNAMICS);
  if (rule == DERIVE_WHAT) return VICGPU_ERR_ARG;
  if (!c->dom.domain_ready) return VICGPU_ERR_STATE;
  if (rule == DERIVE_UNSUPPORTED) {
    c->err = "derive_soil_state: VICGPU_DERIVE_CAP_MOIST with GLACIER_DYNAMICS: the excess moisture (cell.excess_moist) has no table";
    return VICGPU_ERR_UNSUPPORTED;
  }
  if (n == 0) return VICGPU_OK;
  Domain& d = c->dom;
  const ParamFault f = check_param_update(0, d.nhru, 0, nullptr, n, hrus);
  if (f.rule != PARAM_OK) {
    c->err = param_fault_message("derive_soil_state", f);
    return VICGPU_ERR_ARG;
  }
  HIPCHK(c, hipSetDevice(c->device));
  DevBuf<int> list;
  if (hrus) HIPCHK(c, list.alloc(n));
  StreamTimer timer;               // tuning (VICGPU_STATS): the kernel's own time
  HIPCHK(c, timer.create(c->tune.stats));
  if (hrus) HIPCHK(c, list.upload(c->stream, hrus));
  DSArgs a{};
  a.o = c->o; a.ncell = d.ncell; a.nhru = d.nhru; a.n = n; a.what = what; a.hrus = hrus ? list.get() : nullptr;
  a.cp = d.d_cp; a.hpi = d.d_hpi; a.hpd = d.d_hpd; a.sd = d.d_sd; a.si = d.d_si; a.flux = d.d_flux; a.cell_err = d.d_cell_err;
  HIPCHK(c, timer.begin(c->stream));
  HIPCHK(c, derive_soil_state(c->stream, a));
  HIPCHK(c, timer.end(c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));      // the list is released when the call returns
  float ms = 0;
  if (timer.elapsed(&ms))
    fprintf(stderr, "[vicgpu] derive_soil_state: %d HRUs, %s, stages %d: %.4f ms on the device\n", n, hrus ? "listed" : "dense", what, ms);
  return VICGPU_OK;
}

// ---- model state combined linearly across cells (vic_mix_cells.hpp): the ensemble transform of a filter, inflation, recentring
// Everything the call allocates is allocated before anything is queued: one list block [rows][destination HRUs][their
// destinations][their positions][term_off][term_cell], the weights and the stage.
int vicgpu_mix_cells(vicgpu_ctx* c, int nrow, const int* rows, int ndst, const int* dst_cell, const int* term_off, const int* term_cell,
                     const double* term_weight) {
  if (!c || nrow < 0 || ndst < 0) return VICGPU_ERR_ARG;
  if (!c->dom.domain_ready) return VICGPU_ERR_STATE;
  if (nrow == 0 || ndst == 0) return VICGPU_OK;
  if (!rows || !dst_cell || !term_off || !term_cell || !term_weight) return VICGPU_ERR_ARG;
  Domain& d = c->dom;
  // the structure of a domain does not change: the cells' classes under the pair rule are built once
  if (d.cell_class.empty()) d.cell_class = copy_cell_classes(d.ncell, d.nhru, d.cell_off.data(), d.cell_list.data(), d.copy_key.data(), COPY_NKEY);
  // every list is checked here, before the first write
  MixPlan& p = d.mix_plan;                         // kept with the domain: the next call reuses its memory
  plan_cell_mix(p, d.ncell, d.nhru, d.cell_off.data(), d.cell_list.data(), d.copy_key.data(), COPY_NKEY, d.cell_class.data(),
                                  (int)VICGPU_SD_NROW(c->o.Nnode), nrow, rows, ndst, dst_cell, term_off, term_cell, term_weight);
  if (p.fault != MIX_OK) { c->err = mix_fault_text(p); return VICGPU_ERR_ARG; }
  const int n = (int)p.size(), nnz = term_off[ndst];
  if (n == 0) return VICGPU_OK;                    // destinations without HRUs
  HIPCHK(c, hipSetDevice(c->device));
  DevBuf<int> lists;
  DevBuf<double> weights, stage;
  HIPCHK(c, lists.alloc((size_t)nrow + 3 * (size_t)n + (size_t)ndst + 1 + (size_t)nnz));
  HIPCHK(c, weights.alloc((size_t)nnz));
  const int rpp = rows_per_pass((size_t)c->tune.copy_stage_mb << 20, (size_t)n, sizeof(double), nrow);
  HIPCHK(c, stage.alloc((size_t)rpp * n));
  MixLists l;
  l.rows = lists.get(); l.hru = l.rows + nrow; l.dst_index = l.hru + n; l.pos = l.dst_index + n; l.term_off = l.pos + n;
  l.term_cell = l.term_off + ndst + 1; l.term_weight = weights.get(); l.cell_off = d.d_cell_off; l.cell_list = d.d_cell_list;
  // the context's stream follows every step queued so far (with the finite-difference pipeline it waits for every chunk's
  // `done` event, step_impl) and precedes every step queued later: the mix is queued there
  StreamTimer timer;               // tuning (VICGPU_STATS): the kernels' own time
  HIPCHK(c, timer.create(c->tune.stats));
  const size_t un = (size_t)n, at_hru = (size_t)nrow, at_off = at_hru + 3 * un, at_cell = at_off + (size_t)ndst + 1;
  HIPCHK(c, lists.upload(c->stream, rows, 0, (size_t)nrow));
  HIPCHK(c, lists.upload(c->stream, p.hru.data(), at_hru, un));
  HIPCHK(c, lists.upload(c->stream, p.dst_index.data(), at_hru + un, un));
  HIPCHK(c, lists.upload(c->stream, p.pos.data(), at_hru + 2 * un, un));
  HIPCHK(c, lists.upload(c->stream, term_off, at_off, (size_t)ndst + 1));
  HIPCHK(c, lists.upload(c->stream, term_cell, at_cell, (size_t)nnz));
  HIPCHK(c, weights.upload(c->stream, term_weight));
  HIPCHK(c, timer.begin(c->stream));
  HIPCHK(c, mix_cells_staged(c->stream, d.d_sd, (size_t)d.nhru, l, nrow, n, stage, rpp));
  HIPCHK(c, timer.end(c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));      // the lists and the stage are released when the call returns
  float ms = 0;
  if (timer.elapsed(&ms))
    fprintf(stderr, "[vicgpu] mix_cells: %d destinations, %d HRUs, %d terms, %d rows, %d passes, %zu bytes written: %.4f ms on the device\n", ndst, n,
            nnz, nrow, (nrow + rpp - 1) / rpp, sizeof(double) * nrow * n, ms);
  return VICGPU_OK;
}

// ---- the per-column ensemble transform solved and applied on the device (vic_member_transform.hpp): the analysis of a localised
// filter.  The domain holds the stored transform; a call that fails leaves it as it was: solve and set fill a fresh buffer and
// the domain takes it at the end.
static int transform_sizes_check(vicgpu_ctx* c, int nmember, int ncol) {
  if (!c || nmember < 2 || nmember > VICGPU_TRANSFORM_MAX_MEMBERS || ncol < 1) return VICGPU_ERR_ARG;
  if (!c->dom.domain_ready) return VICGPU_ERR_STATE;
  if ((long long)nmember * ncol != (long long)c->dom.ncell) return VICGPU_ERR_ARG;
  return VICGPU_OK;
}

int vicgpu_member_transform_solve(vicgpu_ctx* c, int nmember, int ncol, const int* obs_off, const double* hx, const double* yobs,
                                  const double* rinv, const double* infl, int* info) {
  const int r = transform_sizes_check(c, nmember, ncol);
  if (r != VICGPU_OK) return r;
  if (!obs_off) return VICGPU_ERR_ARG;
  if (obs_off[0] != 0) { c->err = "member_transform_solve: obs_off does not start at 0"; return VICGPU_ERR_ARG; }
  for (int j = 0; j < ncol; j++)
    if (obs_off[j + 1] < obs_off[j]) { c->err = "member_transform_solve: column " + std::to_string(j) + ": obs_off decreases"; return VICGPU_ERR_ARG; }
  const int nobs = obs_off[ncol];
  if (nobs > 0 && (!hx || !yobs || !rinv)) return VICGPU_ERR_ARG;
  // every list is checked here, before anything is queued
  const SolveFault f = check_transform_solve(nmember, ncol, obs_off, hx, yobs, rinv, infl);
  if (f.rule != MT_OK) { c->err = solve_fault_text(f); return VICGPU_ERR_ARG; }
  Domain& d = c->dom;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t M = (size_t)nmember, un = (size_t)ncol, uo = (size_t)nobs, no1 = uo ? uo : 1;
  // what the call allocates, before anything is queued: [obs_off][info], [hx][yobs][rinv][infl][sqrt(infl)], the new transform
  DevBuf<int> ints;
  DevBuf<double> obs, fresh;
  HIPCHK(c, ints.alloc(2 * un + 1));
  HIPCHK(c, obs.alloc(no1 * (M + 2) + 2 * un));
  HIPCHK(c, fresh.alloc(un * M * M));
  const size_t at_y = no1 * M, at_r = at_y + no1, at_infl = at_r + no1, at_sq = at_infl + un;
  StreamTimer timer;               // tuning (VICGPU_STATS): the kernel's own time
  HIPCHK(c, timer.create(c->tune.stats));
  HIPCHK(c, ints.upload(c->stream, obs_off, 0, un + 1));
  if (nobs > 0) {
    HIPCHK(c, obs.upload(c->stream, hx, 0, uo * M));
    HIPCHK(c, obs.upload(c->stream, yobs, at_y, uo));
    HIPCHK(c, obs.upload(c->stream, rinv, at_r, uo));
  }
  if (infl) {
    std::vector<double> sq(un);
    for (size_t j = 0; j < un; j++) sq[j] = std::sqrt(infl[j]);
    HIPCHK(c, obs.upload(c->stream, infl, at_infl, un));
    HIPCHK(c, obs.upload(c->stream, sq.data(), at_sq, un));
  }
  MTSolveArgs a;
  a.nmember = nmember; a.ncol = ncol; a.max_sweeps = c->tune.transform_sweeps; a.obs_off = ints.get(); a.hx = obs.get(); a.yobs = obs.get() + at_y;
  a.rinv = obs.get() + at_r; a.infl = infl ? obs.get() + at_infl : nullptr; a.sqrt_infl = infl ? obs.get() + at_sq : nullptr;
  a.T = fresh.get(); a.info = ints.get() + un + 1;
  // the solve touches no model table, but the transform it replaces may still be read by an apply queued on the stream: it is
  // queued there too, and the call waits for it
  HIPCHK(c, timer.begin(c->stream));
  HIPCHK(c, transform_solve(c->stream, a));
  HIPCHK(c, timer.end(c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (info) HIPCHK(c, ints.download(c->stream, info, un + 1, un));
  d.d_transform = std::move(fresh);                // the old one goes with `fresh`
  d.tf_nmember = nmember; d.tf_ncol = ncol;
  float ms = 0;
  if (timer.elapsed(&ms))
    fprintf(stderr, "[vicgpu] member_transform_solve: %d members, %d columns, %d observations: %.4f ms on the device\n", nmember, ncol, nobs, ms);
  return VICGPU_OK;
}

int vicgpu_member_transform_set(vicgpu_ctx* c, int nmember, int ncol, const double* T) {
  const int r = transform_sizes_check(c, nmember, ncol);
  if (r != VICGPU_OK) return r;
  if (!T) return VICGPU_ERR_ARG;
  const size_t count = (size_t)ncol * nmember * nmember;
  for (size_t i = 0; i < count; i++)
    if (!std::isfinite(T[i])) {
      c->err = "member_transform_set: column " + std::to_string(i / ((size_t)nmember * nmember)) + ": a weight is not finite";
      return VICGPU_ERR_ARG;
    }
  Domain& d = c->dom;
  HIPCHK(c, hipSetDevice(c->device));
  DevBuf<double> fresh;
  HIPCHK(c, fresh.alloc(count));
  HIPCHK(c, hipStreamSynchronize(c->stream));      // an apply queued earlier may still read the transform this one replaces
  HIPCHK(c, fresh.upload(c->stream, T));
  d.d_transform = std::move(fresh);
  d.tf_nmember = nmember; d.tf_ncol = ncol;
  return VICGPU_OK;
}

int vicgpu_member_transform_get(vicgpu_ctx* c, int* nmember, int* ncol, double* T) {
  if (!c) return VICGPU_ERR_ARG;
  if (!c->dom.domain_ready || !c->dom.d_transform) return VICGPU_ERR_STATE;
  const Domain& d = c->dom;
  if (nmember) *nmember = d.tf_nmember;
  if (ncol) *ncol = d.tf_ncol;
  if (!T) return VICGPU_OK;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, d.d_transform.download(c->stream, T));
  return VICGPU_OK;
}

// Everything the call allocates is allocated before anything is queued: one list block [rows][destination HRUs][their cells]
// [their positions] and the stage.
int vicgpu_member_transform_apply(vicgpu_ctx* c, int nrow, const int* rows, int n, const int* cols) {
  if (!c || nrow < 0 || n < 0) return VICGPU_ERR_ARG;
  if (!c->dom.domain_ready || !c->dom.d_transform) return VICGPU_ERR_STATE;
  if (nrow == 0 || n == 0) return VICGPU_OK;
  if (!rows) return VICGPU_ERR_ARG;
  Domain& d = c->dom;
  const int M = d.tf_nmember, ncol = d.tf_ncol;
  if (d.cell_class.empty()) d.cell_class = copy_cell_classes(d.ncell, d.nhru, d.cell_off.data(), d.cell_list.data(), d.copy_key.data(), COPY_NKEY);
  // every list is checked here, before the first write
  TransformPlan& p = d.transform_plan;             // kept with the domain: the next call reuses its memory
  plan_transform_apply(p, M, ncol, d.nhru, d.cell_off.data(), d.cell_list.data(), d.copy_key.data(), COPY_NKEY, d.cell_class.data(),
                       (int)VICGPU_SD_NROW(c->o.Nnode), nrow, rows, n, cols);
  if (p.fault != MT_OK) { c->err = transform_fault_text(p); return VICGPU_ERR_ARG; }
  const int nh = (int)p.size();
  if (nh == 0) return VICGPU_OK;                   // columns without HRUs
  HIPCHK(c, hipSetDevice(c->device));
  DevBuf<int> lists;
  DevBuf<double> stage;
  const size_t un = (size_t)nh;
  HIPCHK(c, lists.alloc((size_t)nrow + 3 * un));
  const int rpp = rows_per_pass((size_t)c->tune.copy_stage_mb << 20, un, sizeof(double), nrow);
  HIPCHK(c, stage.alloc((size_t)rpp * un));
  TransformLists l;
  l.rows = lists.get(); l.hru = l.rows + nrow; l.cell = l.hru + nh; l.pos = l.cell + nh; l.cell_off = d.d_cell_off; l.cell_list = d.d_cell_list;
  // the context's stream follows every step queued so far (with the finite-difference pipeline it waits for every chunk's
  // `done` event, step_impl) and precedes every step queued later: the transform is queued there
  StreamTimer timer;               // tuning (VICGPU_STATS): the kernels' own time
  HIPCHK(c, timer.create(c->tune.stats));
  HIPCHK(c, lists.upload(c->stream, rows, 0, (size_t)nrow));
  HIPCHK(c, lists.upload(c->stream, p.hru.data(), (size_t)nrow, un));
  HIPCHK(c, lists.upload(c->stream, p.cell.data(), (size_t)nrow + un, un));
  HIPCHK(c, lists.upload(c->stream, p.pos.data(), (size_t)nrow + 2 * un, un));
  HIPCHK(c, timer.begin(c->stream));
  HIPCHK(c, transform_apply_staged(c->stream, d.d_sd, (size_t)d.nhru, l, M, ncol, d.d_transform, nrow, nh, stage, rpp));
  HIPCHK(c, timer.end(c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));      // the lists and the stage are released when the call returns
  float ms = 0;
  if (timer.elapsed(&ms))
    fprintf(stderr, "[vicgpu] member_transform_apply: %d members, %d columns, %d HRUs, %d rows, %d passes, %zu bytes written: %.4f ms on the device\n", M,
            n, nh, nrow, (nrow + rpp - 1) / rpp, sizeof(double) * nrow * un, ms);
  return VICGPU_OK;
}

// ------------------------------------------------------------------------------------------------ output records (vicgpu_out.h)
int vicgpu_records_config(vicgpu_ctx* c, int nvar, const int* var_ids, int depth) {
  if (!c) return VICGPU_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  if (nvar == 0) {                 // releases the slots
    HIPCHK(c, hipStreamSynchronize(c->stream));
    free_records(c);
    return VICGPU_OK;
  }
  if (!c->dom.put_on) return VICGPU_ERR_STATE;
  if (nvar < 0 || !var_ids || depth < 1) return VICGPU_ERR_ARG;
  std::vector<int> sel(c->dom.out_nrow, -1);
  int nrow = 0;
  for (int k = 0; k < nvar; k++) {
    if (var_ids[k] < 0 || var_ids[k] >= VOUT_NVAR) return VICGPU_ERR_ARG;
    for (int r = c->dom.out_lay.off[var_ids[k]]; r < c->dom.out_lay.off[var_ids[k] + 1]; r++) {
      if (sel[r] >= 0) return VICGPU_ERR_ARG;        // listed twice
      sel[r] = nrow++;
    }
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));        // a record of the last call may still be on its way into a slot
  free_records(c);
  Records r;                       // becomes the context's only when complete
  r.nrow = nrow; r.depth = depth;
  HIPCHK(c, r.d_sel_pos.alloc(sel.size()));
  HIPCHK(c, r.d_sel_pos.upload(c->stream, sel.data()));
  r.slot.resize(depth);
  for (Records::Slot& s : r.slot) {
    HIPCHK(c, s.d_out.alloc((size_t)nrow * c->dom.ncell));
    HIPCHK(c, s.d_err.alloc(c->dom.ncell));
  }
  r.nlane = c->dom.fd ? (int)c->dom.chunks.size() : 1;
  r.packed.resize((size_t)r.nlane * depth);
  for (Event& e : r.packed) HIPCHK(c, e.create(hipEventDisableTiming));
  HIPCHK(c, r.drained.create(hipEventDisableTiming));
  if (!c->dom.fd) HIPCHK(c, r.dl.create());
  c->rec = std::move(r);
  return VICGPU_OK;
}

int vicgpu_records_nrow(vicgpu_ctx* c) {
  if (!c) return VICGPU_ERR_ARG;
  return c->rec.depth > 0 ? c->rec.nrow : VICGPU_ERR_STATE;
}

// Cell groups of the records (vicgpu_out.h).  Checks first; then what the groups need is allocated aside, filled once the records
// still on their way have landed, and handed to the configuration only when complete: a refused call leaves the groups in force.
int vicgpu_records_set_groups(vicgpu_ctx* c, int ngroup, const int* group_off, const int* group_cell, const double* group_weight, float fill) {
  if (!c) return VICGPU_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  if (c->rec.depth < 1) return VICGPU_ERR_STATE;
  if (ngroup < 0 || (ngroup > 0 && (!group_off || !group_cell))) return VICGPU_ERR_ARG;
  int nnz = 0, most = 0;
  if (ngroup > 0) {
    if (group_off[0] != 0) return VICGPU_ERR_ARG;
    for (int g = 0; g < ngroup; g++) {
      if (group_off[g + 1] < group_off[g]) return VICGPU_ERR_ARG;
      most = std::max(most, group_off[g + 1] - group_off[g]);
    }
    nnz = group_off[ngroup];
    for (int i = 0; i < nnz; i++)
      if (group_cell[i] < 0 || group_cell[i] >= c->dom.ncell || (group_weight && !std::isfinite(group_weight[i]))) return VICGPU_ERR_ARG;
  }
  Records& R = c->rec;
  DevBuf<int> d_off, d_cell;
  DevBuf<double> d_weight;
  std::vector<DevBuf<float>> d_group(ngroup > 0 ? R.depth : 0);
  if (ngroup > 0) {
    const std::vector<double> ones(group_weight ? 0 : nnz, 1.0);
    HIPCHK(c, d_off.alloc((size_t)ngroup + 1));
    HIPCHK(c, d_cell.alloc(std::max(nnz, 1)));
    HIPCHK(c, d_weight.alloc(std::max(nnz, 1)));
    for (DevBuf<float>& b : d_group) HIPCHK(c, b.alloc((size_t)R.nrow * ngroup));
    HIPCHK(c, hipStreamSynchronize(c->stream));      // a record of the last call may still be on its way
    HIPCHK(c, hipStreamSynchronize(records_stream(c)));
    HIPCHK(c, d_off.upload(c->stream, group_off));
    if (nnz > 0) {
      HIPCHK(c, d_cell.upload(c->stream, group_cell, 0, nnz));
      HIPCHK(c, d_weight.upload(c->stream, group_weight ? group_weight : ones.data(), 0, nnz));
    }
  } else {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(records_stream(c)));
  }
  records_report_reduce(c);
  R.d_group_off = std::move(d_off); R.d_group_cell = std::move(d_cell); R.d_group_weight = std::move(d_weight);
  for (int s = 0; s < R.depth; s++) R.slot[s].d_group = ngroup > 0 ? std::move(d_group[s]) : DevBuf<float>();
  R.ngroup = ngroup; R.nnz = nnz; R.fill = fill; R.lane_per_group = most <= 1;
  if (ngroup > 0 && !R.join) R.join.reset(new RecordsJoin);
  R.last_nrecords = 0;             // nothing of an earlier call is in flight, and its events describe records of another shape
  return VICGPU_OK;
}

int vicgpu_records_get_groups(vicgpu_ctx* c, int* ngroup, int* nnz) {
  if (!c || !ngroup || !nnz) return VICGPU_ERR_ARG;
  if (c->rec.depth < 1) return VICGPU_ERR_STATE;
  *ngroup = c->rec.ngroup; *nnz = c->rec.nnz;
  return VICGPU_OK;
}

int vicgpu_records_ncol(vicgpu_ctx* c) {
  if (!c) return VICGPU_ERR_ARG;
  if (c->rec.depth < 1) return VICGPU_ERR_STATE;
  return c->rec.ngroup > 0 ? c->rec.ngroup : c->dom.ncell;
}

// ld: cells per row of `out` and `cell_err` (c->dom.ncell, or the global cell count when a group delivers one shard's columns)
static int run_records_impl(vicgpu_ctx* c, int step0, int nrecords, float* out, int* cell_err, int ld) {
  if (!c) return VICGPU_ERR_ARG;
  if (!c->dom.domain_ready || !c->d_veglib || !c->dom.put_on || c->rec.depth < 1 || !c->d_forcing || c->chunk_steps <= 0) return VICGPU_ERR_STATE;
  const int ratio = c->out_step_ratio;
  if (step0 < 0 || nrecords < 1 || (long long)step0 + (long long)nrecords * ratio > c->chunk_steps || ld < c->dom.ncell) return VICGPU_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  if (!out || !is_pinned(out) || (cell_err && !is_pinned(cell_err))) return VICGPU_ERR_ARG;
  Records& R = c->rec;
  if (R.ngroup > 0 && ld != c->dom.ncell) return VICGPU_ERR_STATE;      // grouped records have no pitched form (vicgpu_group.h)
  // record k's landed event of every lane
  const size_t nev = (size_t)R.nlane * nrecords;
  if (R.landed.size() < nev) {
    const size_t had = R.landed.size();
    R.landed.resize(nev);
    for (size_t i = had; i < nev; i++) HIPCHK(c, R.landed[i].create(hipEventDisableTiming));
  }
  if (R.ngroup > 0) {              // record k's reduction over the groups, joined from the lanes (Records)
    if (R.reduced.size() < (size_t)nrecords) {
      const size_t had = R.reduced.size();
      R.reduced.resize(nrecords);
      for (size_t i = had; i < (size_t)nrecords; i++) HIPCHK(c, R.reduced[i].create(hipEventDisableTiming));
    }
    if (c->tune.stats && !R.reduce_t0) {
      HIPCHK(c, R.reduce_t0.create());
      HIPCHK(c, R.reduce_t1.create());
    }
    R.join->start(nrecords);
  }
  // the first packing kernels of this call reuse slots the last call's copies may still read: they wait for `drained`, which
  // is recorded anew only after them (the steps themselves wait for nothing)
  R.follows = R.last_nrecords > 0;
  R.out = out; R.err = cell_err; R.ld = ld;
  R.last_nrecords = nrecords;
  int r = step_impl(c, step0, nrecords * ratio, ratio);
  if (r == VICGPU_OK) {
    const hipError_t e = hipEventRecord(R.drained, records_stream(c));
    if (e != hipSuccess) { c->err = std::string("hipEventRecord: ") + hipGetErrorString(e); r = VICGPU_ERR_HIP; }
  }
  if (r != VICGPU_OK) {            // no copy stays in flight after an error return
    HIPIGN(hipStreamSynchronize(c->stream));
    for (FdChunk& ch : c->dom.chunks) HIPIGN(hipStreamSynchronize(ch.stream));
    HIPIGN(hipStreamSynchronize(records_stream(c)));
    R.last_nrecords = 0;
  }
  return r;
}
int vicgpu_run_records(vicgpu_ctx* c, int step0, int nrecords, float* out, int* cell_err) {
  return c ? run_records_impl(c, step0, nrecords, out, cell_err, c->dom.ncell) : VICGPU_ERR_ARG;
}

int vicgpu_records_wait(vicgpu_ctx* c, int k) {
  if (!c) return VICGPU_ERR_ARG;
  const Records& R = c->rec;
  if (R.depth < 1 || R.last_nrecords < 1) return VICGPU_ERR_STATE;
  if (k < -1 || k >= R.last_nrecords) return VICGPU_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  if (k < 0) { HIPCHK(c, hipEventSynchronize(R.drained)); return VICGPU_OK; }
  // with groups the reduction of record k is queued behind every lane's part of it, on the same stream
  if (R.ngroup > 0) { HIPCHK(c, hipEventSynchronize(R.reduced[k])); return VICGPU_OK; }
  for (int lane = 0; lane < R.nlane; lane++) HIPCHK(c, hipEventSynchronize(R.landed[(size_t)lane * R.last_nrecords + k]));
  return VICGPU_OK;
}

}  // extern "C"
