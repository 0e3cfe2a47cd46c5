// vic_aux_kernels.hpp — the small kernels around the step, each with its argument struct (device only, gfx950): the glacier
// mass-balance fit, the derived cell-parameter rows, the test hooks (vicgpu_debug_*), vic_cell_reduce (one lane per cell:
// atmos->out_prec/out_rain/out_snow, full_energy.c:429-431, summed in hruList order -- deterministic, no atomics -- and the
// Cv-weighted per-cell accumulators), the state-file records, the forcing derivation and the float rows of the output read-back.
#pragma once
#include <cstddef>
#include "vic_profile.hpp"

using namespace vic;

// ------------------------------------------------------------------------------------------------ glacier mass-balance fit
// GlacierMassBalanceResult.c:34-73 + GraphingEquation.c:8-125 for every cell at once (lane = cell): the accumulated
// mass balance of the cell's glacier HRUs against band elevation, points merged per elevation in hruList order, closed-form
// normal equations in the reference's order of operations; then resetAccumulationValues
// (accumulateGlacierMassBalance.c:5-11) when asked.
struct GArgs {
  Opt o;
  int ncell, nhru, reset;
  const double* cell_params;
  const int* cell_off;
  const int* cell_list;
  const int* hpi;
  double* sd;
  double* eq;          // [GMB_NROW][ncell]
  const int* valid;    // [ncell] cell validity words (CELL_*, vic_types.hpp), or null: every cell is valid
};

__global__ __launch_bounds__(64) void vic_glacier_fit(const GArgs a) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= a.ncell) return;
  const size_t nh = a.nhru, nc = a.ncell;
  if (a.valid && a.valid[c] != CELL_VALID) {
    // vicNl.c:562 skips accumulateGlacierMassBalance for an invalid cell: the default equation, and no reset of its HRUs
    a.eq[(size_t)GMB_B0 * nc + c] = 0; a.eq[(size_t)GMB_B1 * nc + c] = 0; a.eq[(size_t)GMB_B2 * nc + c] = 0;
    a.eq[(size_t)GMB_FIT_ERROR * nc + c] = -1;
    return;
  }
  CellView cv{a.cell_params, a.ncell, c, a.o.Nnode, a.o.Nband};
  double X[VIC_MAX_BANDS], Y[VIC_MAX_BANDS];      // at most one point per band elevation
  int np = 0;
  for (int k = a.cell_off[c]; k < a.cell_off[c + 1]; k++) {
    const int g = a.cell_list[k];
    if (a.hpi[(size_t)HPI_IS_GLACIER * nh + g] == 0) continue;
    const double cum = a.sd[(size_t)SD_GLAC_CUM_MASS_BALANCE * nh + g];
    if (!isnan(cum)) {
      const double x = cv.band(CPB_BANDELEV, a.hpi[(size_t)HPI_BAND * nh + g]);
      bool found = false;
      for (int j = 0; j < np; j++)
        if (X[j] == x) { Y[j] += cum; found = true; }
      if (!found && np < VIC_MAX_BANDS) { X[np] = x; Y[np] = cum; np++; }
    }
    if (a.reset) a.sd[(size_t)SD_GLAC_CUM_MASS_BALANCE * nh + g] = 0.0;
  }
  int k2 = 0;
  for (int i = 0; i < np; i++)
    if (!(X[i] == 0)) { X[k2] = X[i]; Y[k2] = Y[i]; k2++; }       // "meaningless" points (GlacierMassBalanceResult.c:58-66)
  np = k2;
  double b0 = 0, b1 = 0, b2 = 0, fit = -1;
  if (np == 1) b0 = Y[0];
  else if (np == 2) {
    const double slope = (Y[1] - Y[0]) / (X[1] - X[0]);
    b0 = Y[0] - slope * X[0]; b1 = slope;
  } else if (np >= 3) {
    double sumx4 = 0, sumx3 = 0, sumx2 = 0, sumx1 = 0;
    const int size = np;
    for (int i = 0; i < np; i++) {
      sumx4 += X[i] * X[i] * X[i] * X[i];
      sumx3 += X[i] * X[i] * X[i];
      sumx2 += X[i] * X[i];
      sumx1 += X[i];
    }
    const double det = (sumx4 * sumx2 * size) + (sumx3 * sumx1 * sumx2) + (sumx2 * sumx3 * sumx1) - (sumx2 * sumx2 * sumx2)
                       - (sumx1 * sumx1 * sumx4) - (size * sumx3 * sumx3);
    const double inv[3][3] = {{size * sumx2 - sumx1 * sumx1, -(size * sumx3 - sumx1 * sumx2), sumx1 * sumx3 - sumx2 * sumx2},
                              {-(size * sumx3 - sumx2 * sumx1), size * sumx4 - sumx2 * sumx2, -(sumx1 * sumx4 - sumx3 * sumx2)},
                              {sumx1 * sumx3 - sumx2 * sumx2, -(sumx1 * sumx4 - sumx2 * sumx3), sumx2 * sumx4 - sumx3 * sumx3}};
    double acoef[3] = {0, 0, 0};
#pragma unroll
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < np; j++) {
        const double stuff = inv[i][0] * (X[j] * X[j]) + inv[i][1] * X[j] + inv[i][2] * 1;
        acoef[i] += stuff * Y[j];
      }
      acoef[i] /= det;
    }
    b0 = acoef[2]; b1 = acoef[1]; b2 = acoef[0];
  }
  if (np > 0) {
    fit = 0;
    for (int i = 0; i < np; i++) fit += fabs((b0 + b1 * X[i] + b2 * (X[i] * X[i])) - Y[i]);
  }
  a.eq[(size_t)GMB_B0 * nc + c] = b0; a.eq[(size_t)GMB_B1 * nc + c] = b1; a.eq[(size_t)GMB_B2 * nc + c] = b2;
  a.eq[(size_t)GMB_FIT_ERROR * nc + c] = fit;
}

// ------------------------------------------------------------------------------------------------ derived cell rows
// The rows the library appends to its copy of the cell parameter table (vic_types.hpp), for one cell.  Device functions: the
// full-domain kernels below (vicgpu_set_domain, vicgpu_put_data_config) and the listed-cell kernels of vic_params.hpp
// (vicgpu_update_cell_params / vicgpu_update_hru_params) both call them, so a re-derived row holds the bits a fresh domain gets.
VIC_DEV void derive_cell_params_of(double* cp, int ncell, int c, int Nn, int Nb) {
  CellView cv{cp, ncell, c, Nn, Nb};
#pragma unroll
  for (int l = 0; l < VIC_NLAYER; l++) {
    const SoilKLayer k = soil_conductivity_layer_constants(cv.lay(CPL_SOIL_DENS_MIN, l), cv.lay(CPL_BULK_DENS_MIN, l), cv.lay(CPL_QUARTZ, l),
                                                           cv.lay(CPL_SOIL_DENSITY, l), cv.lay(CPL_BULK_DENSITY, l), cv.lay(CPL_ORGANIC, l));
    cp[(size_t)VIC_CPX_ROW(CPX_KDRY, l, Nn, Nb) * ncell + c] = k.Kdry;
    cp[(size_t)VIC_CPX_ROW(CPX_KSP, l, Nn, Nb) * ncell + c] = k.KsP;
    cp[(size_t)VIC_CPX_ROW(CPX_KWP, l, Nn, Nb) * ncell + c] = k.KwP;
    cp[(size_t)VIC_CPX_ROW(CPX_POROSITY, l, Nn, Nb) * ncell + c] = k.porosity;
  }
}

// TreeAdjustFactor of put_data.c:185-208 for every band of one cell
VIC_DEV void derive_tree_adjust_of(double* cp, int ncell, int nhru, int c, int Nn, int Nb, const int* cell_off, const int* cell_list, const int* hpi,
                                   const double* hpd, const double* veglib) {
  for (int b = 0; b < Nb; b++) {
    double bandCv = 0;
    for (int k = cell_off[c]; k < cell_off[c + 1]; k++) {          // hruList order, like the reference's sum
      const int g = cell_list[k];
      if (hpi[(size_t)HPI_BAND * nhru + g] != b) continue;
      if (veglib[(size_t)hpi[(size_t)HPI_VEG_INDEX * nhru + g] * VL_NFIELD + VL_OVERSTORY] != 0.0) bandCv += hpd[(size_t)HPD_CV * nhru + g];
    }
    const bool atl = cp[(size_t)VICGPU_CP_BAND(CPB_ABOVETREELINE, b, Nn, Nb) * ncell + c] != 0.0;
    cp[(size_t)VIC_CPX_TREE_ROW(b, Nn, Nb) * ncell + c] = atl ? 1. / (1. - bandCv) : 1.;
  }
}

__global__ __launch_bounds__(256) void vic_derive_cell_params(double* cp, int ncell, int Nn, int Nb) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= ncell) return;
  derive_cell_params_of(cp, ncell, c, Nn, Nb);
}

// ... for every cell (lane = cell; once per vicgpu_put_data_config)
__global__ __launch_bounds__(64) void vic_derive_tree_adjust(double* cp, int ncell, int nhru, int Nn, int Nb, const int* cell_off, const int* cell_list,
                                                             const int* hpi, const double* hpd, const double* veglib) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= ncell) return;
  derive_tree_adjust_of(cp, ncell, nhru, c, Nn, Nb, cell_off, cell_list, hpi, hpd, veglib);
}

// ------------------------------------------------------------------------------------------------ test hook
struct DArgs { Opt o; const double* cell_params; int ncell, fn, n; const double* in; double* out; };

__global__ __launch_bounds__(64) void vic_debug_pure(const DArgs d) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= d.n) return;
  const double* a = d.in + (size_t)i * VICGPU_PURE_NIN;
  CellView cv{d.cell_params, d.ncell, 0, d.o.Nnode, d.o.Nband};
  double r = NAN;
  switch (d.fn) {
    case VICGPU_PURE_SVP: r = svp(a[0]); break;
    case VICGPU_PURE_SVP_SLOPE: r = svp_slope(a[0]); break;
    case VICGPU_PURE_CALC_RAINONLY: r = calc_rainonly(d.o, a[0], a[1], a[2], a[3]); break;
    case VICGPU_PURE_SNOW_ALBEDO: r = snow_albedo(d.o, cv, a[0], a[1], a[2], a[3], a[4], a[5], (int)a[6], a[7] != 0.0 ? 1 : 0); break;
    case VICGPU_PURE_NEW_SNOW_DENSITY: r = new_snow_density(d.o, a[0]); break;
    case VICGPU_PURE_STABILITY: r = stability_correction(a[0], a[1], a[2], a[3], a[4], a[5]); break;
    case VICGPU_PURE_PENMAN: r = penman(a[0], a[1], a[2], a[3], a[4], a[5], a[6]); break;
    case VICGPU_PURE_CALC_RC: r = calc_rc(a[0], a[1], (float)a[2], a[3], a[4], a[5], a[6], a[7] != 0.0); break;
    case VICGPU_PURE_ESTIMATE_T1: r = estimate_T1(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9]); break;
    case VICGPU_PURE_SOIL_CONDUCTIVITY: r = soil_conductivity(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]); break;
    case VICGPU_PURE_VOL_HEAT_CAPACITY: r = volumetric_heat_capacity(a[0], a[1], a[2], a[3]); break;
    case VICGPU_PURE_MAX_UNFROZEN_WATER: r = maximum_unfrozen_water(a[0], a[1], a[2], a[3]); break;
    case VICGPU_PURE_LINEAR_INTERP: r = linear_interp(a[0], a[1], a[2], a[3], a[4]); break;
    case VICGPU_PURE_VEG_HEIGHT: r = calc_veg_height(a[0], a[1]); break;
    case VICGPU_PURE_SOIL_CONDUCTIVITY_DERIVED: {
      const int l = (int)a[2];
      const SoilKLayer kc{cv.x(CPX_KDRY, l), cv.x(CPX_KSP, l), cv.x(CPX_KWP, l), cv.x(CPX_POROSITY, l)};
      r = soil_conductivity_pre(a[0], a[1], kc);
      break;
    }
    case VICGPU_PURE_LN_POS: r = ln_pos(a[0]); break;
    case VICGPU_PURE_POW_POS: r = pow_pos(a[0], a[1]); break;
    case VICGPU_PURE_POW_POS_APPROX: r = pow_pos_approx(a[0], (float)a[1]); break;
    case VICGPU_PURE_RCP_REFINED: r = rcp_refined(a[0]); break;
    default: break;
  }
  d.out[i] = r;
}

// One node visit per lane (vicgpu_debug_node_root).  Every lane of every wave calls node_visit, which votes across the
// wave: lanes past the last case take part with sweeping = false.
struct NRArgs { int n; bool EXP_TRANS; const double* in; double* out; };

template <bool NODE1, bool NEWTON>
__global__ __launch_bounds__(64) void vic_debug_node_root(const NRArgs d) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  const bool live = i < d.n;
  const double* a = d.in + (size_t)(live ? i : 0) * VICGPU_NODE_NIN;
  double rec[PREC];
  profile_node_fold(rec, d.EXP_TRANS, true, a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10]);
  NodeK K;
  K.load(rec);
  bool failed;
  const double T = node_visit<NODE1, NEWTON>(live, true, d.EXP_TRANS, K, a[13], a[11], a[12], a[5], failed);
  if (live) {
    d.out[(size_t)i * VICGPU_NODE_NOUT] = T;
    d.out[(size_t)i * VICGPU_NODE_NOUT + 1] = failed ? 1.0 : 0.0;
  }
}

// One root find per lane (vicgpu_debug_root_brent): the production state machines, fed with recorded residual values.
// The lanes of a wave loop until the last one is done, as in the solves of the model.
struct RBArgs { int n; const double* bounds; const int* off; const double* fvals; double* xreq; double* out; };

__device__ __forceinline__ bool rb_finished(const Brent& st) { return st.phase == Brent::DONE; }
__device__ __forceinline__ bool rb_finished(const BrentLean& st) { return st.finished(); }
// out[2..7]: failed, result, i, j, k, which_err.  Brent's only failure mark is its ERROR result (root_brent.c's return value).
__device__ __forceinline__ void rb_report(const Brent& st, double* r) {
  r[2] = (st.phase == Brent::DONE && st.result == ERROR_VAL) ? 1.0 : 0.0;
  r[3] = st.result; r[4] = st.i; r[5] = st.j; r[6] = st.k; r[7] = st.which_err;
}
__device__ __forceinline__ void rb_report(const BrentLean& st, double* r) {
  r[2] = (st.phase == BrentLean::FAILED) ? 1.0 : 0.0;
  r[3] = (st.phase == BrentLean::DONE) ? st.b : ERROR_VAL; r[4] = st.i; r[5] = st.j; r[6] = 0; r[7] = 0;
}

template <class S>
__global__ __launch_bounds__(64) void vic_debug_root_brent(const RBArgs d) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= d.n) return;
  const int o0 = d.off[i], o1 = d.off[i + 1];
  S st;
  st.start(d.bounds[2 * (size_t)i], d.bounds[2 * (size_t)i + 1]);
  int k = 0;
  bool overrun = false;
  while (!rb_finished(st)) {
    if (o0 + k >= o1) { overrun = true; break; }
    d.xreq[o0 + k] = st.x;
    st.advance(d.fvals[o0 + k]);
    k++;
  }
  double* r = d.out + (size_t)i * VICGPU_BRENT_NOUT;
  r[0] = k;
  r[1] = rb_finished(st) ? 1.0 : 0.0;
  rb_report(st, r);
  r[8] = overrun ? 1.0 : 0.0;
}

// ------------------------------------------------------------------------------------------------ cell kernel
struct CArgs {
  int ncell, nhru;
  int c0, ccount;        // cells of this launch
  const int* cell_off;
  const int* cell_list;
  const double* hpd;
  const int* hpi_glac;   // row HPI_IS_GLACIER of the int parameter table
  const double* flux;
  const double* sd;
  const int* hru_err;
  double* cell_out;   // [CO_NROW][ncell]
  double* accum;      // [CA_NROW][ncell]
  int* cell_err;      // [ncell], OR-accumulated
  int* valid;         // [ncell] cell validity words (CELL_*, vic_types.hpp), or null: every cell is valid
  int retire_mask;    // VICGPU_CELLERR_* bits that retire a cell (vicgpu_set_retire_on_error)
};

__global__ __launch_bounds__(256) void vic_cell_reduce(const CArgs a) {
  const int ci = blockIdx.x * 256 + threadIdx.x;
  if (ci >= a.ccount) return;
  const int c = a.c0 + ci;
  // an invalid cell keeps its sums, its step count and its flag word; the cell that took its last step in the step before
  // (put_data has seen it since) is skipped from here on
  if (a.valid) {
    const int v = a.valid[c];
    if (v != CELL_VALID) {
      if (v == CELL_LAST) a.valid[c] = CELL_SKIP;
      return;
    }
  }
  const size_t nh = a.nhru, nc = a.ncell;
  double op = 0, orn = 0, os = 0, ro = 0, bf = 0, ev = 0, swe = 0, sm0 = 0, sm1 = 0, sm2 = 0, gmb = 0;
  int err = 0;
  for (int k = a.cell_off[c]; k < a.cell_off[c + 1]; k++) {
    const int g = a.cell_list[k];
    const double Cv = a.hpd[(size_t)HPD_CV * nh + g];
    op += a.flux[(size_t)FX_OUT_PREC * nh + g] * Cv;            // full_energy.c:429-431
    orn += a.flux[(size_t)FX_OUT_RAIN * nh + g] * Cv;
    os += a.flux[(size_t)FX_OUT_SNOW * nh + g] * Cv;
    ro += a.flux[(size_t)FX_RUNOFF * nh + g] * Cv;              // put_data.c:789-800 AreaFactor = Cv (mu = TreeAdjust = 1)
    bf += a.flux[(size_t)FX_BASEFLOW * nh + g] * Cv;
    double e = a.flux[(size_t)FX_EVAP0 * nh + g] + a.flux[(size_t)FX_EVAP1 * nh + g] + a.flux[(size_t)FX_EVAP2 * nh + g]
               + a.flux[(size_t)FX_CANOPYEVAP * nh + g]
               + (a.flux[(size_t)FX_SNOW_VAPOR_FLUX * nh + g] + a.flux[(size_t)FX_SNOW_CANOPY_VAPOR_FLUX * nh + g]) * 1000.;
    ev += e * Cv;
    swe += a.sd[(size_t)SD_SNOW_SWQ * nh + g] * 1000. * Cv;
    sm0 += a.sd[(size_t)SD_MOIST0 * nh + g] * Cv;
    sm1 += a.sd[(size_t)SD_MOIST1 * nh + g] * Cv;
    sm2 += a.sd[(size_t)SD_MOIST2 * nh + g] * Cv;
    { double mb = a.flux[(size_t)FX_GLAC_MASS_BALANCE * nh + g]; if (a.hpi_glac[g] && !isnan(mb)) gmb += mb * Cv; }
    err |= a.hru_err[g];
  }
  a.cell_out[(size_t)CO_OUT_PREC * nc + c] = op;
  a.cell_out[(size_t)CO_OUT_RAIN * nc + c] = orn;
  a.cell_out[(size_t)CO_OUT_SNOW * nc + c] = os;
  a.accum[(size_t)CA_RUNOFF * nc + c] += ro;
  a.accum[(size_t)CA_BASEFLOW * nc + c] += bf;
  a.accum[(size_t)CA_EVAP * nc + c] += ev;
  a.accum[(size_t)CA_PREC * nc + c] += op;
  a.accum[(size_t)CA_SWE_END * nc + c] = swe;
  a.accum[(size_t)CA_SOIL_MOIST_END0 * nc + c] = sm0;
  a.accum[(size_t)CA_SOIL_MOIST_END1 * nc + c] = sm1;
  a.accum[(size_t)CA_SOIL_MOIST_END2 * nc + c] = sm2;
  a.accum[(size_t)CA_GLAC_MASS_BALANCE * nc + c] += gmb;
  a.accum[(size_t)CA_NSTEPS * nc + c] += 1.0;
  err |= a.cell_err[c];
  a.cell_err[c] = err;
  // vicNl.c:545-559: isValid = FALSE after a step that returned ERROR; this step's put_data still runs (dist_prec.c:167)
  if (a.valid && (err & a.retire_mask)) a.valid[c] = CELL_LAST;
}

// ------------------------------------------------------------------------------------------------ state-file records
// One lane per HRU in hruList order: the HRU's values in the order processCellForStateFile streams them
// (write_model_state.c:166-285).  GATHER = false is the read side; lanes whose band / vegetation class do not match the
// record count themselves in *mismatch and scatter nothing.
struct RArgs {
  int nhru, Nn;
  const int* cell_list;
  const int* hpi;
  double* sd;
  int* si;
  double* flux;
  double* rec;
  int* mismatch;
};

template <bool GATHER>
__global__ __launch_bounds__(256) void vic_state_records(const RArgs a) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= a.nhru) return;
  const int g = a.cell_list[k], Nn = a.Nn;
  const size_t nh = a.nhru;
  double* r = a.rec + (size_t)k * VICGPU_SR_LEN(Nn);
  const int band = a.hpi[(size_t)HPI_BAND * nh + g], vegc = a.hpi[(size_t)HPI_VEG_CLASS * nh + g];
  if (GATHER) { r[SR_BAND_INDEX] = band; r[SR_VEG_CLASS] = vegc; }
  else if ((int)r[SR_BAND_INDEX] != band || (int)r[SR_VEG_CLASS] != vegc) { atomicAdd(a.mismatch, 1); return; }
#define D(slot, row) do { if (GATHER) r[slot] = a.sd[(size_t)(row) * nh + g]; else a.sd[(size_t)(row) * nh + g] = r[slot]; } while (0)
#define I(slot, row) do { if (GATHER) r[slot] = a.si[(size_t)(row) * nh + g]; else a.si[(size_t)(row) * nh + g] = (int)r[slot]; } while (0)
#define F(slot, row) do { if (GATHER) r[slot] = a.flux[(size_t)(row) * nh + g]; else a.flux[(size_t)(row) * nh + g] = r[slot]; } while (0)
  for (int l = 0; l < 3; l++) { D(SR_MOIST0 + l, SD_MOIST0 + l); D(SR_ICE0 + l, SD_ICE0 + l); }
  D(SR_WDEW, SD_WDEW);
  D(SR_SNOW_CANOPY, SD_SNOW_CANOPY); D(SR_SNOW_DENSITY, SD_SNOW_DENSITY); D(SR_SNOW_DEPTH, SD_SNOW_DEPTH);
  D(SR_SNOW_PACK_WATER, SD_SNOW_PACK_WATER); D(SR_SNOW_SURF_WATER, SD_SNOW_SURF_WATER); D(SR_SNOW_SWQ, SD_SNOW_SWQ);
  D(SR_GLAC_WATER_STORAGE, SD_GLAC_WATER_STORAGE); D(SR_GLAC_CUM_MASS_BALANCE, SD_GLAC_CUM_MASS_BALANCE);
  for (int n = 0; n < Nn; n++) { D(SR_ENERGY_T + n, VICGPU_SD_NODE(SDN_T, n, Nn)); I(VICGPU_SR_T(SRT_T_FBCOUNT, Nn) + n, VICGPU_SI_NODE(SIN_T_FBCOUNT, n, Nn)); }
  D(VICGPU_SR_T(SRT_TFOLIAGE, Nn), SD_TFOLIAGE); D(VICGPU_SR_T(SRT_GLAC_SURF_TEMP, Nn), SD_GLAC_SURF_TEMP);
  D(VICGPU_SR_T(SRT_SNOW_COLD_CONTENT, Nn), SD_SNOW_COLDCONTENT); D(VICGPU_SR_T(SRT_SNOW_PACK_TEMP, Nn), SD_SNOW_PACK_TEMP);
  D(VICGPU_SR_T(SRT_SNOW_SURF_TEMP, Nn), SD_SNOW_SURF_TEMP); D(VICGPU_SR_T(SRT_SNOW_ALBEDO, Nn), SD_SNOW_ALBEDO);
  I(VICGPU_SR_T(SRT_SNOW_LAST_SNOW, Nn), SI_SNOW_LAST_SNOW); I(VICGPU_SR_T(SRT_SNOW_MELTING, Nn), SI_SNOW_MELTING);
  I(VICGPU_SR_T(SRT_TCANOPY_FBCOUNT, Nn), SI_TCANOPY_FBCOUNT);
  I(VICGPU_SR_U(SRU_TFOLIAGE_FBCOUNT, Nn), SI_TFOLIAGE_FBCOUNT); I(VICGPU_SR_U(SRU_TSURF_FBCOUNT, Nn), SI_TSURF_FBCOUNT);
  I(VICGPU_SR_U(SRU_GLAC_SURF_TEMP_FBCOUNT, Nn), SI_GLAC_SURF_TEMP_FBCOUNT); I(VICGPU_SR_U(SRU_SNOW_SURF_TEMP_FBCOUNT, Nn), SI_SNOW_SURF_TEMP_FBCOUNT);
  I(VICGPU_SR_U(SRU_GLAC_SURF_TEMP_FBFLAG, Nn), SI_GLAC_SURF_TEMP_FBFLAG);
  F(VICGPU_SR_U(SRU_GLAC_VAPOR_FLUX, Nn), FX_GLAC_VAPOR_FLUX);
  if (GATHER) r[VICGPU_SR_U(SRU_SNOW_CANOPY_ALBEDO, Nn)] = 0.0;            // snow.canopy_albedo: initialize_snow.c:62, never assigned again
  F(VICGPU_SR_U(SRU_SNOW_SURFACE_FLUX, Nn), FX_SNOW_SURFACE_FLUX);
  I(VICGPU_SR_U(SRU_SNOW_SURF_TEMP_FBFLAG, Nn), SI_SNOW_SURF_TEMP_FBFLAG);
  D(VICGPU_SR_U(SRU_SNOW_TMP_INT_STORAGE, Nn), SD_SNOW_TMP_INT_STORAGE);
  F(VICGPU_SR_U(SRU_SNOW_VAPOR_FLUX, Nn), FX_SNOW_VAPOR_FLUX);
#undef D
#undef I
#undef F
}

// ------------------------------------------------------------------------------------------------ forcing derivation
// initialize_atmos.c, the derivation of atmos[rec] from the hourly forcing of one record (see include/vicgpu.h).  The nine
// numeric rows depend on the raw values and the options only, the snowflag on the cell's parameters too (:1275-1303: the
// coldest band's Tfactor, MAX_SNOW_TEMP, MIN_RAIN_TEMP).  Without a forcing map a lane is one (step, cell) and does both.
// With one (vicgpu_set_forcing_map) the rows are derived once per (step, column) and the flags once per (step, cell), by the
// same expression from the column's T and prec, re-read from the derived table.
struct FArgs {
  int nsteps, ncell, dt, snow_step, NF, NR, temp_th_type, Nband, Nnode, plapse;
  int ncol;                    // columns of raw and forcing; ncell without a map
  double min_wind;
  const double* raw;
  const double* cell_params;
  double* forcing;
  unsigned char* snowflag;
  const int* cell_col;         // [ncell], read by vic_derive_forcing_flags only
};

// Where a lane's raw values come from: raw(v, h) is variable v (VIC_RAW_*) of hour h of the lane's step and column.
// RawDirect: column col of the ncol-wide table (vicgpu_prefetch_forcing_raw).
struct RawDirect {
  const double* p;
  size_t dt, nw;
  VIC_DEV RawDirect(const FArgs& a, int s, int col) : p(a.raw + (size_t)s * VIC_NRAW * a.dt * a.ncol + col), dt(a.dt), nw(a.ncol) {}
  VIC_DEV double operator()(int v, int h) const { return p[((size_t)v * dt + h) * nw]; }
};

// the flags of a mapped run read the derived table, no raw value
struct RawNone {
  VIC_DEV double operator()(int, int) const { return 0.0; }
};

// vicgpu_prefetch_forcing_perturbed: forcing column col reads source column col_src[col] of the nsrc-wide table in a.f.raw and,
// with PERT, the factors of group col_group[col]: x' = (x * mul) + add, the product and the sum rounded once each (the
// library is built without contraction).  Without PERT the value is the table's, verbatim.
struct FPArgs {
  FArgs f;                     // f.raw: [nsteps][VIC_NRAW][dt][nsrc]
  int nsrc, ngroup;
  int group_base;              // the group of column 0 when col_group is null (a group per column; a shard's columns start past 0)
  const int* col_src;          // [ncol], or null: column i reads source i
  const int* col_group;        // [ncol], or null: column i is group group_base + i
  const double* pert;          // [nsteps][VICGPU_NPERT][ngroup]; unread without PERT
};

// The 2 * VIC_NRAW factors of the lane's (step, group) are loaded once, here, into registers (v is a constant at every call of
// the derivation, so mul[v] / add[v] are plain registers); nearly every lane of a wave names the same group, so the loads of a
// wave hit one line.  The raw reads of consecutive lanes are consecutive source columns with the member-major lists.
template <bool PERT>
struct RawPerturbed {
  const double* p;
  size_t dt, nw;
  double mul[VIC_NRAW], add[VIC_NRAW];
  VIC_DEV RawPerturbed(const FPArgs& a, int s, int col) : dt(a.f.dt), nw(a.nsrc) {
    p = a.f.raw + (size_t)s * VIC_NRAW * a.f.dt * a.nsrc + (a.col_src ? a.col_src[col] : col);
    if constexpr (PERT) {
      const double* q = a.pert + (size_t)s * VICGPU_NPERT * a.ngroup + (a.col_group ? a.col_group[col] : a.group_base + col);
#pragma unroll
      for (int v = 0; v < VIC_NRAW; v++) { mul[v] = q[(size_t)VICGPU_PERT_MUL(v) * a.ngroup]; add[v] = q[(size_t)VICGPU_PERT_ADD(v) * a.ngroup]; }
    }
  }
  VIC_DEV double operator()(int v, int h) const {
    const double x = p[((size_t)v * dt + h) * nw];
    if constexpr (!PERT) return x;
    else {
      const double m = x * mul[v];
      return m + add[v];
    }
  }
};

// step s: the rows of column col (VALUES) and / or the flags of cell c, whose column is col (FLAGS); RAW: the raw values (unread
// without VALUES)
template <bool VALUES, bool FLAGS, class Raw>
VIC_DEV void derive_forcing_lane(const FArgs& a, const Raw& RAW, int s, int col, int c) {
  const size_t nc = a.ncell, nw = a.ncol;
  const int ns = a.NR + 1, NF = a.NF;
  double* f = a.forcing + (size_t)s * VIC_NFORCE * ns * nw + col;
  unsigned char* sf = a.snowflag + (size_t)s * ns * nc + c;
#define F(v, j) f[((size_t)(v) * ns + (j)) * nw]
  double min_Tfactor = 0, thr = 0;
  if constexpr (FLAGS) {
    CellView cv{a.cell_params, a.ncell, c, a.Nnode, a.Nband};
    min_Tfactor = cv.band(CPB_TFACTOR, 0);                                            // initialize_atmos.c:1275-1280
    for (int b = 1; b < a.Nband; b++) { const double t = cv.band(CPB_TFACTOR, b); if (t < min_Tfactor) min_Tfactor = t; }
    const double max_snow = cv.s(CP_MAX_SNOW_TEMP), min_rain = cv.s(CP_MIN_RAIN_TEMP);
    thr = (a.temp_th_type == VIC_TEMP_TH_KIENZLE) ? (max_snow + min_rain / 2) : max_snow;
  }
  double sT = 0, sP = 0, sPr = 0, sVp = 0, sVpd = 0, sD = 0, sSw = 0, sLw = 0, sW = 0;
  bool any_snow = false;
  for (int j = 0; j < NF; j++) {
    if constexpr (!VALUES) {                                                          // the flags of a mapped run: T and prec as derived
      const bool snow = ((F(VIC_F_AIR_TEMP, j) + min_Tfactor) < thr) && (F(VIC_F_PREC, j) > 0);
      sf[(size_t)j * nc] = snow ? 1 : 0;
      any_snow = any_snow || snow;
      continue;
    }
    double T = 0, prec = 0, pr = 0, vp = 0, sw = 0, lw = 0, wind = 0;
    for (int h = j * a.snow_step; h < (j + 1) * a.snow_step; h++) {                   // the snow_step-hour aggregation (:886-893 et al.)
      T += RAW(VIC_RAW_AIR_TEMP, h); prec += RAW(VIC_RAW_PREC, h);
      pr += RAW(VIC_RAW_PRESSURE_KPA, h) * 1000.0; vp += RAW(VIC_RAW_VP_KPA, h) * 1000.0;      // kPa2Pa, :290-295
      sw += RAW(VIC_RAW_SHORTWAVE, h); lw += RAW(VIC_RAW_LONGWAVE, h);
      const double w = RAW(VIC_RAW_WIND, h);
      wind += (w < a.min_wind) ? a.min_wind : w;                                      // :527-530
    }
    T /= a.snow_step; pr /= a.snow_step; vp /= a.snow_step; sw /= a.snow_step; lw /= a.snow_step; wind /= a.snow_step;
    const double dens = a.plapse ? pr / (287.0 * (KELVIN + T)) : 0.003486 * pr / (275.0 + T);   // :988-998 (Rd = 287)
    double vpd = svp(T) - vp;                                                         // :1179-1183
    if (vpd < 0) { vpd = 0; vp = svp(T); }
    F(VIC_F_AIR_TEMP, j) = T; F(VIC_F_PREC, j) = prec; F(VIC_F_PRESSURE, j) = pr; F(VIC_F_VP, j) = vp; F(VIC_F_VPD, j) = vpd;
    F(VIC_F_DENSITY, j) = dens; F(VIC_F_SHORTWAVE, j) = sw; F(VIC_F_LONGWAVE, j) = lw; F(VIC_F_WIND, j) = wind;
    if constexpr (FLAGS) {
      const bool snow = ((T + min_Tfactor) < thr) && (prec > 0);                      // :1283-1300
      sf[(size_t)j * nc] = snow ? 1 : 0;
      any_snow = any_snow || snow;
    }
    sT += T; sP += prec; sPr += pr; sVp += vp; sVpd += vpd; sD += dens; sSw += sw; sLw += lw; sW += wind;
  }
  if (NF > 1 && FLAGS) sf[(size_t)a.NR * nc] = any_snow ? 1 : 0;
  if (NF > 1 && VALUES) {                                                             // x[NR] = sum / (float)NF; prec[NR] = sum
    const double n = (double)(float)NF;
    F(VIC_F_AIR_TEMP, a.NR) = sT / n; F(VIC_F_PREC, a.NR) = sP; F(VIC_F_PRESSURE, a.NR) = sPr / n; F(VIC_F_VP, a.NR) = sVp / n;
    F(VIC_F_VPD, a.NR) = sVpd / n; F(VIC_F_SHORTWAVE, a.NR) = sSw / n; F(VIC_F_LONGWAVE, a.NR) = sLw / n;
    F(VIC_F_WIND, a.NR) = sW / n;
    // density[NR] is derived from pressure[NR] and air_temp[NR] like every other slot (initialize_atmos.c:984-998), not averaged
    F(VIC_F_DENSITY, a.NR) = a.plapse ? (sPr / n) / (287.0 * (KELVIN + sT / n)) : 0.003486 * (sPr / n) / (275.0 + sT / n);
  }
#undef F
}

// no map: one lane per (step, cell), rows and flag
extern "C" __global__ __launch_bounds__(256) void vic_derive_forcing(const FArgs a) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)a.nsteps * a.ncell) return;
  const int s = (int)(i / a.ncell), c = (int)(i % a.ncell);
  derive_forcing_lane<true, true>(a, RawDirect(a, s, c), s, c, c);
}
// with a map: one lane per (step, column) for the rows, then one lane per (step, cell) for the flags
extern "C" __global__ __launch_bounds__(256) void vic_derive_forcing_cols(const FArgs a) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)a.nsteps * a.ncol) return;
  const int s = (int)(i / a.ncol), col = (int)(i % a.ncol);
  derive_forcing_lane<true, false>(a, RawDirect(a, s, col), s, col, 0);
}
extern "C" __global__ __launch_bounds__(256) void vic_derive_forcing_flags(const FArgs a) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)a.nsteps * a.ncell) return;
  const int c = (int)(i % a.ncell);
  derive_forcing_lane<false, true>(a, RawNone(), (int)(i / a.ncell), a.cell_col[c], c);
}
// vicgpu_prefetch_forcing_perturbed: one lane per (step, forcing column), consecutive lanes consecutive columns; the flags in
// the same lane when there is no forcing map (FLAGS: column = cell), by vic_derive_forcing_flags after it when there is one
template <bool FLAGS, bool PERT>
__global__ __launch_bounds__(256) void vic_derive_forcing_pert(const FPArgs a) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)a.f.nsteps * a.f.ncol) return;
  const int s = (int)(i / a.f.ncol), col = (int)(i % a.f.ncol);
  derive_forcing_lane<true, FLAGS>(a.f, RawPerturbed<PERT>(a, s, col), s, col, col);
}

// the derived row of vicgpu_set_forcing_map: every HRU's forcing column, read by the step kernels next to the HPI rows
extern "C" __global__ __launch_bounds__(256) void vic_fill_hru_fcol(const int* __restrict__ hpi_cell, const int* __restrict__ cell_col, int nhru,
                                                          int* __restrict__ fcol) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g < nhru) fcol[g] = cell_col[hpi_cell[g]];
}

// ------------------------------------------------------------------------------------------------ output read-back
extern "C" __global__ __launch_bounds__(256) void vic_out_rows_f32(const double* __restrict__ src, const int* __restrict__ rows, int nrows, int ncell,
                                                         float* __restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)nrows * ncell) return;
  const int r = (int)(i / ncell), cc = (int)(i % ncell);
  dst[i] = (float)src[(size_t)rows[r] * ncell + cc];                       // WriteOutputNetCDF.c:387-455 writes floats
}
