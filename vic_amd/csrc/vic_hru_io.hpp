// vic_hru_io.hpp — the HRU kernels' arguments and their traffic with the SoA tables (device only, gfx950): LaunchMap (the
// XCD-aware launch order), KArgs, the identity of an HRU (HruId / hru_id), and the loads and stores between the state, flux
// and parameter tables and a lane's working set (load_* / store_* / load_soil3).  No kernel lives here.
#pragma once
#include <cstddef>
#include "vic_step.hpp"

using namespace vic;

// XCD-aware launch order.  HRUs are numbered slot-major (hru = slot * ncell + cell), so the 64 HRUs of a block are 64
// consecutive cells of one (tile, band) slot, and the ~300 cell-parameter rows and the forcing rows of those cells are read
// again by the block of every other slot.  Workgroups go round-robin over the 8 XCDs and every XCD has its own L2: in launch
// order "all cells of slot 0, then slot 1 ..." those re-reads are a whole domain apart and come from HBM every time.  With
// map_nslot > 0 a launch covers a REGULAR list (nslot slots x ccount cells, entry = slot * ccount + cell) and block b takes
// cell block (b >> 3) / nslot * 8 + (b & 7) of slot (b >> 3) % nslot: the blocks of one cell block's slots are consecutive on
// ONE XCD, so its table rows are fetched from HBM once and hit in that XCD's L2 for the other slots.
struct LaunchMap {
  int nslot = 0, ccount = 0;         // nslot == 0: identity (irregular lists)
  __host__ __device__ int nblocks(int gcount) const {
    if (nslot == 0) return (gcount + 63) / 64;
    const int ncb = (ccount + 63) / 64;
    return (ncb + 7) / 8 * 8 * nslot;
  }
  // list index of (block, lane), or -1
  VIC_DEV int index(int block, int lane, int gcount) const {
    if (nslot == 0) { const int gi = block * 64 + lane; return gi < gcount ? gi : -1; }
    const int q = block >> 3, cb = q / nslot * 8 + (block & 7), cell = cb * 64 + lane;
    return cell < ccount ? (q % nslot) * ccount + cell : -1;
  }
};

struct KArgs {
  Opt o;
  LaunchMap map;
  int ncell, nhru, nveg_rows, write_fluxes;
  const double* veglib;
  const double* cell_params;
  const int* hpi;
  const double* hpd;
  const double* forcing;            // this step: [VIC_NFORCE][NF+1][ncol]
  const unsigned char* snowflag;    // this step: [NF+1][ncell]
  const int* fcol;                  // [nhru] forcing column of each HRU's cell; without a map the HPI_CELL row itself
  int ncol;                         // forcing columns (vicgpu_set_forcing_map); ncell without a map
  Dmy dmy;
  double* sd;
  int* si;
  double* flux;
  int* hru_err;                     // [nhru]
  const int* glist;                 // HRUs of this launch (a cell chunk), or null: all HRUs in order
  int gcount;
  // finite-difference pipeline only (null otherwise)
  unsigned long long* ctx;          // parked per-HRU context, [hru / 64][word][hru % 64]
  double* pin;                      // profile item blocks [nhru][item_stride(Nn)] (vic_layout.hpp)
  double* ts;                       // trial surface temperature [nhru]
  double* pout;                     // profile solutions [nhru][pout_hru_stride(Nn)] (two keyed records)
  int* pslot;                       // [nhru] record the next profile solve writes
  int* hstate;                      // [nhru] 0 idle, 1 residual evaluation pending, 2 root found: stage kernel's turn
  int* list;                        // work list the stage kernel appends to (NBUCKET segments of list_cap entries)
  int* count;                       // [NBUCKET]
  int list_cap;
  int* hkey;                        // [nhru] work-list segment of each HRU (number of frozen nodes)
  double* pimp;                     // IMPLICIT: the implicit solver's item blocks [nhru][Nn][PIMP]
  int* lastexp;                     // IMPLICIT: [nhru] record slot holding the flags of the root find's last explicit solve
  int* jl;                          // QUICK_SOLVE: [nhru] end of the column the profile kernel solves
  int phase;                        // 0: start of the step; p >= 1: after the root finder of sub-step p - 1
  const int* valid;                 // [ncell] cell validity words (CELL_*), or null: every cell is valid
};

// ------------------------------------------------------------------------------------------------ state table I/O
// node_props = false leaves the node moisture / ice / conductivity / heat-capacity rows for load_node_props
template <int NN>
VIC_DEV void load_state(const KArgs& a, int g, HruWork<NN>& w, bool node_props = true) {
  const int Nn = a.o.Nnode;
  const size_t nh = a.nhru;
  const double* __restrict__ sd = a.sd;
  const int* __restrict__ si = a.si;
#define SD(row) sd[(size_t)(row) * nh + g]
#define SI(row) si[(size_t)(row) * nh + g]
#pragma unroll
  for (int l = 0; l < 3; l++) { w.moist[l] = SD(SD_MOIST0 + l); w.ice[l] = SD(SD_ICE0 + l); w.layer_T[l] = SD(SD_LAYER_T0 + l); w.evap[l] = 0; }
  SoilEnergy& so = w.so; SnowEnergy& se = w.se; Snow& s = w.snow;
  so.snow_flux = SD(SD_SNOW_FLUX); so.grnd_flux = SD(SD_GRND_FLUX); so.deltaH = SD(SD_DELTAH); so.fusion = SD(SD_FUSION);
  so.LongUnderOut = SD(SD_LONGUNDEROUT); se.Tfoliage = SD(SD_TFOLIAGE);
  s.albedo = SD(SD_SNOW_ALBEDO); s.coldcontent = SD(SD_SNOW_COLDCONTENT); s.coverage = SD(SD_SNOW_COVERAGE);
  s.density = SD(SD_SNOW_DENSITY); s.depth = SD(SD_SNOW_DEPTH); s.pack_temp = SD(SD_SNOW_PACK_TEMP);
  s.pack_water = SD(SD_SNOW_PACK_WATER); s.snow_canopy = SD(SD_SNOW_CANOPY); s.surf_temp = SD(SD_SNOW_SURF_TEMP);
  s.surf_water = SD(SD_SNOW_SURF_WATER); s.swq = SD(SD_SNOW_SWQ); s.tmp_int_storage = SD(SD_SNOW_TMP_INT_STORAGE);
  s.store_swq = SD(SD_SNOW_STORE_SWQ); s.store_coverage = SD(SD_SNOW_STORE_COVERAGE); s.swq_slope = SD(SD_SNOW_SWQ_SLOPE);
  s.max_swq = SD(SD_SNOW_MAX_SWQ);
  s.blowing_flux = 0; s.canopy_vapor_flux = 0; s.mass_error = 0; s.melt = 0; s.Qnet = 0; s.surface_flux = 0; s.vapor_flux = 0;
  w.vv.Wdew = SD(SD_WDEW); w.vv.canopyevap = 0; w.vv.throughfall = 0;
  w.Tcanopy = SD(SD_TCANOPY); so.Tsurf = SD(SD_TSURF); se.AlbedoOver = SD(SD_ALBEDO_OVER); so.AlbedoUnder = SD(SD_ALBEDO_UNDER);
  se.canopy_advection = SD(SD_CANOPY_ADVECTION); se.canopy_latent = SD(SD_CANOPY_LATENT);
  se.canopy_latent_sub = SD(SD_CANOPY_LATENT_SUB); se.canopy_sensible = SD(SD_CANOPY_SENSIBLE);
  se.canopy_refreeze = SD(SD_CANOPY_REFREEZE);
  se.advected_sensible = so.advected_sensible = SD(SD_ADVECTED_SENSIBLE);
  se.advection = so.advection = SD(SD_ADVECTION);
  se.deltaCC = so.deltaCC = SD(SD_DELTACC);
  se.refreeze_energy = so.refreeze_energy = SD(SD_REFREEZE_ENERGY);
  so.melt_energy = SD(SD_MELT_ENERGY);
  se.error = so.error = SD(SD_ERROR);
  se.latent = so.latent = SD(SD_LATENT); se.latent_sub = so.latent_sub = SD(SD_LATENT_SUB);
  se.sensible = so.sensible = SD(SD_SENSIBLE);
  se.snow_flux = so.snow_flux;
  se.LongOverIn = SD(SD_LONGOVERIN); se.NetLongOver = SD(SD_NETLONGOVER); se.NetShortOver = SD(SD_NETSHORTOVER);
  se.ShortOverIn = SD(SD_SHORTOVERIN);
  so.NetShortGrnd = 0; so.NetLongUnder = SD(SD_NETLONGUNDER); so.NetShortUnder = 0;
  w.gl.surf_temp = SD(SD_GLAC_SURF_TEMP); w.gl.water_storage = SD(SD_GLAC_WATER_STORAGE);
  w.gl.cum_mass_balance = SD(SD_GLAC_CUM_MASS_BALANCE);
  w.gl.cold_content = NAN; w.gl.Qnet = NAN; w.gl.mass_balance = NAN; w.gl.ice_mass_balance = 0; w.gl.accumulation = NAN;
  w.gl.melt = NAN; w.gl.vapor_flux = NAN; w.gl.outflow = NAN; w.gl.outflow_coef = NAN; w.gl.inflow = NAN;
  w.deltaCC_glac = 0; w.glacier_flux = 0; w.glacier_melt_energy = 0;
  so.kappa[0] = so.kappa[1] = so.Cs[0] = so.Cs[1] = 0;
#pragma unroll
  for (int f = 0; f < 3; f++) { so.fdepth[f] = 0; so.tdepth[f] = 0; }
#pragma unroll
  for (int n = 0; n < NN; n++) {
    if (n < Nn) {
      w.nd.T[n] = SD(VICGPU_SD_NODE(SDN_T, n, Nn));
      if (node_props) {
        w.nd.moist[n] = SD(VICGPU_SD_NODE(SDN_MOIST, n, Nn)); w.nd.ice[n] = SD(VICGPU_SD_NODE(SDN_ICE, n, Nn));
        w.nd.kappa[n] = SD(VICGPU_SD_NODE(SDN_KAPPA, n, Nn)); w.nd.Cs[n] = SD(VICGPU_SD_NODE(SDN_CS, n, Nn));
      } else { w.nd.moist[n] = 0; w.nd.ice[n] = 0; w.nd.kappa[n] = 0; w.nd.Cs[n] = 0; }
      w.nd.fbflag[n] = SI(VICGPU_SI_NODE(SIN_T_FBFLAG, n, Nn)); w.nd.fbcount[n] = SI(VICGPU_SI_NODE(SIN_T_FBCOUNT, n, Nn));
    } else {
      w.nd.T[n] = 0; w.nd.moist[n] = 0; w.nd.ice[n] = 0; w.nd.kappa[n] = 0; w.nd.Cs[n] = 0; w.nd.fbflag[n] = 0; w.nd.fbcount[n] = 0;
    }
  }
  s.last_snow = SI(SI_SNOW_LAST_SNOW); s.MELTING = SI(SI_SNOW_MELTING); s.snow = SI(SI_SNOW_SNOW); s.store_snow = SI(SI_SNOW_STORE_SNOW);
  s.surf_temp_fbcount = SI(SI_SNOW_SURF_TEMP_FBCOUNT); s.surf_temp_fbflag = SI(SI_SNOW_SURF_TEMP_FBFLAG);
  so.Tsurf_fbcount = SI(SI_TSURF_FBCOUNT); so.Tsurf_fbflag = SI(SI_TSURF_FBFLAG);
  se.Tfoliage_fbcount = SI(SI_TFOLIAGE_FBCOUNT); se.Tfoliage_fbflag = SI(SI_TFOLIAGE_FBFLAG);
  so.frozen = SI(SI_FROZEN); so.Nfrost = SI(SI_NFROST); so.Nthaw = SI(SI_NTHAW);
  w.gl.surf_temp_fbcount = SI(SI_GLAC_SURF_TEMP_FBCOUNT); w.gl.surf_temp_fbflag = SI(SI_GLAC_SURF_TEMP_FBFLAG);
#undef SD
#undef SI
}

// the node rows that do not change during a step (distribute_node_moisture_properties rewrites them at its end)
template <int NN>
VIC_DEV void load_node_props(const KArgs& a, int g, Nodes<NN>& nd) {
  const int Nn = a.o.Nnode;
  const size_t nh = a.nhru;
  const double* __restrict__ sd = a.sd;
#pragma unroll
  for (int n = 0; n < NN; n++) {
    if (n < Nn) {
      nd.moist[n] = sd[(size_t)VICGPU_SD_NODE(SDN_MOIST, n, Nn) * nh + g]; nd.ice[n] = sd[(size_t)VICGPU_SD_NODE(SDN_ICE, n, Nn) * nh + g];
      nd.kappa[n] = sd[(size_t)VICGPU_SD_NODE(SDN_KAPPA, n, Nn) * nh + g]; nd.Cs[n] = sd[(size_t)VICGPU_SD_NODE(SDN_CS, n, Nn) * nh + g];
    }
  }
}

// Phase p >= 1 of the stage kernel: the part of the HRU's working set that neither crosses the root finder in the parked
// context nor is assigned by the bookkeeping before it is read -- state the step has not touched yet, from the state table
// (see WCarry, vic_step.hpp); what the bookkeeping assigns starts as zero.
template <int NN>
VIC_DEV void load_untouched_state(const KArgs& a, int g, HruWork<NN>& w) {
  const int Nn = a.o.Nnode;
  const size_t nh = a.nhru;
  const double* __restrict__ sd = a.sd;
  const int* __restrict__ si = a.si;
#pragma unroll
  for (int l = 0; l < 3; l++) {
    w.moist[l] = sd[(size_t)(SD_MOIST0 + l) * nh + g]; w.ice[l] = sd[(size_t)(SD_ICE0 + l) * nh + g];
    w.layer_T[l] = sd[(size_t)(SD_LAYER_T0 + l) * nh + g]; w.evap[l] = 0;
  }
  w.vv.Wdew = sd[(size_t)SD_WDEW * nh + g]; w.vv.canopyevap = 0; w.vv.throughfall = 0;
  SoilEnergy& so = w.so;
  so.deltaCC = 0; so.refreeze_energy = 0; so.deltaH = 0; so.fusion = 0; so.grnd_flux = 0; so.latent = 0; so.latent_sub = 0; so.sensible = 0;
  so.snow_flux = 0; so.error = 0; so.NetShortGrnd = 0; so.NetLongUnder = 0; so.NetShortUnder = 0; so.LongUnderOut = 0; so.AlbedoUnder = 0;
  so.melt_energy = 0; so.Tsurf = 0; so.kappa[0] = so.kappa[1] = so.Cs[0] = so.Cs[1] = 0;
#pragma unroll
  for (int f = 0; f < 3; f++) { so.fdepth[f] = 0; so.tdepth[f] = 0; }
  so.advected_sensible = sd[(size_t)SD_ADVECTED_SENSIBLE * nh + g];
  so.Tsurf_fbflag = 0; so.Tsurf_fbcount = si[(size_t)SI_TSURF_FBCOUNT * nh + g];
  so.frozen = 0; so.Nfrost = 0; so.Nthaw = si[(size_t)SI_NTHAW * nh + g];
  w.Tcanopy = 0;
  w.gl.surf_temp = sd[(size_t)SD_GLAC_SURF_TEMP * nh + g]; w.gl.water_storage = sd[(size_t)SD_GLAC_WATER_STORAGE * nh + g];
  w.gl.cum_mass_balance = sd[(size_t)SD_GLAC_CUM_MASS_BALANCE * nh + g];
  w.gl.cold_content = NAN; w.gl.Qnet = NAN; w.gl.mass_balance = NAN; w.gl.ice_mass_balance = 0; w.gl.accumulation = NAN;
  w.gl.melt = NAN; w.gl.vapor_flux = NAN; w.gl.outflow = NAN; w.gl.outflow_coef = NAN; w.gl.inflow = NAN;
  w.gl.surf_temp_fbcount = si[(size_t)SI_GLAC_SURF_TEMP_FBCOUNT * nh + g]; w.gl.surf_temp_fbflag = si[(size_t)SI_GLAC_SURF_TEMP_FBFLAG * nh + g];
  w.deltaCC_glac = 0; w.glacier_flux = 0; w.glacier_melt_energy = 0;
#pragma unroll
  for (int n = 0; n < NN; n++) {
    w.nd.T[n] = 0; w.nd.moist[n] = 0; w.nd.ice[n] = 0; w.nd.kappa[n] = 0; w.nd.Cs[n] = 0; w.nd.fbflag[n] = 0;
    w.nd.fbcount[n] = (n < Nn) ? si[(size_t)VICGPU_SI_NODE(SIN_T_FBCOUNT, n, Nn) * nh + g] : 0;
  }
#pragma unroll
  for (int p = 0; p < NPET; p++) w.pot_evap[p] = 0;
}

template <int NN>
VIC_DEV void store_state(const KArgs& a, int g, const HruWork<NN>& w) {
  const int Nn = a.o.Nnode;
  const size_t nh = a.nhru;
  double* __restrict__ sd = a.sd;
  int* __restrict__ si = a.si;
#define SD(row) sd[(size_t)(row) * nh + g]
#define SI(row) si[(size_t)(row) * nh + g]
#pragma unroll
  for (int l = 0; l < 3; l++) { SD(SD_MOIST0 + l) = w.moist[l]; SD(SD_ICE0 + l) = w.ice[l]; SD(SD_LAYER_T0 + l) = w.layer_T[l]; }
  const SoilEnergy& so = w.so; const SnowEnergy& se = w.se; const Snow& s = w.snow;
  SD(SD_SNOW_FLUX) = so.snow_flux; SD(SD_GRND_FLUX) = so.grnd_flux; SD(SD_DELTAH) = so.deltaH; SD(SD_FUSION) = so.fusion;
  SD(SD_LONGUNDEROUT) = so.LongUnderOut; SD(SD_TFOLIAGE) = se.Tfoliage;
  SD(SD_SNOW_ALBEDO) = s.albedo; SD(SD_SNOW_COLDCONTENT) = s.coldcontent; SD(SD_SNOW_COVERAGE) = s.coverage;
  SD(SD_SNOW_DENSITY) = s.density; SD(SD_SNOW_DEPTH) = s.depth; SD(SD_SNOW_PACK_TEMP) = s.pack_temp;
  SD(SD_SNOW_PACK_WATER) = s.pack_water; SD(SD_SNOW_CANOPY) = s.snow_canopy; SD(SD_SNOW_SURF_TEMP) = s.surf_temp;
  SD(SD_SNOW_SURF_WATER) = s.surf_water; SD(SD_SNOW_SWQ) = s.swq; SD(SD_SNOW_TMP_INT_STORAGE) = s.tmp_int_storage;
  SD(SD_SNOW_STORE_SWQ) = s.store_swq; SD(SD_SNOW_STORE_COVERAGE) = s.store_coverage; SD(SD_SNOW_SWQ_SLOPE) = s.swq_slope;
  SD(SD_SNOW_MAX_SWQ) = s.max_swq; SD(SD_WDEW) = w.vv.Wdew;
  SD(SD_TCANOPY) = w.Tcanopy; SD(SD_TSURF) = so.Tsurf; SD(SD_ALBEDO_OVER) = w.AlbedoOver_avg; SD(SD_ALBEDO_UNDER) = so.AlbedoUnder;
  SD(SD_CANOPY_ADVECTION) = se.canopy_advection; SD(SD_CANOPY_LATENT) = se.canopy_latent;
  SD(SD_CANOPY_LATENT_SUB) = se.canopy_latent_sub; SD(SD_CANOPY_SENSIBLE) = se.canopy_sensible;
  SD(SD_CANOPY_REFREEZE) = se.canopy_refreeze; SD(SD_ADVECTED_SENSIBLE) = so.advected_sensible;
  SD(SD_ADVECTION) = so.advection; SD(SD_DELTACC) = so.deltaCC; SD(SD_REFREEZE_ENERGY) = so.refreeze_energy;
  SD(SD_MELT_ENERGY) = so.melt_energy; SD(SD_ERROR) = so.error; SD(SD_LATENT) = so.latent; SD(SD_LATENT_SUB) = so.latent_sub;
  SD(SD_SENSIBLE) = so.sensible; SD(SD_LONGOVERIN) = w.LongOverIn_avg; SD(SD_NETLONGOVER) = w.NetLongOver_avg;
  SD(SD_NETSHORTOVER) = w.NetShortOver_avg; SD(SD_SHORTOVERIN) = w.ShortOverIn_avg; SD(SD_NETLONGUNDER) = so.NetLongUnder;
  SD(SD_GLAC_SURF_TEMP) = w.gl.surf_temp; SD(SD_GLAC_WATER_STORAGE) = w.gl.water_storage;
  SD(SD_GLAC_CUM_MASS_BALANCE) = w.gl.cum_mass_balance;
#pragma unroll
  for (int n = 0; n < NN; n++) {
    if (n < Nn) {
      SD(VICGPU_SD_NODE(SDN_T, n, Nn)) = w.nd.T[n]; SD(VICGPU_SD_NODE(SDN_MOIST, n, Nn)) = w.nd.moist[n];
      SD(VICGPU_SD_NODE(SDN_ICE, n, Nn)) = w.nd.ice[n]; SD(VICGPU_SD_NODE(SDN_KAPPA, n, Nn)) = w.nd.kappa[n];
      SD(VICGPU_SD_NODE(SDN_CS, n, Nn)) = w.nd.Cs[n];
      SI(VICGPU_SI_NODE(SIN_T_FBFLAG, n, Nn)) = w.nd.fbflag[n]; SI(VICGPU_SI_NODE(SIN_T_FBCOUNT, n, Nn)) = w.nd.fbcount[n];
    }
  }
  SI(SI_SNOW_LAST_SNOW) = s.last_snow; SI(SI_SNOW_MELTING) = s.MELTING; SI(SI_SNOW_SNOW) = s.snow; SI(SI_SNOW_STORE_SNOW) = s.store_snow;
  SI(SI_SNOW_SURF_TEMP_FBCOUNT) = s.surf_temp_fbcount; SI(SI_SNOW_SURF_TEMP_FBFLAG) = s.surf_temp_fbflag;
  SI(SI_TSURF_FBCOUNT) = so.Tsurf_fbcount; SI(SI_TSURF_FBFLAG) = so.Tsurf_fbflag;
  SI(SI_TFOLIAGE_FBCOUNT) = se.Tfoliage_fbcount; SI(SI_TFOLIAGE_FBFLAG) = se.Tfoliage_fbflag;
  SI(SI_FROZEN) = so.frozen; SI(SI_NFROST) = so.Nfrost; SI(SI_NTHAW) = so.Nthaw;
  SI(SI_GLAC_SURF_TEMP_FBCOUNT) = w.gl.surf_temp_fbcount; SI(SI_GLAC_SURF_TEMP_FBFLAG) = w.gl.surf_temp_fbflag;
#undef SD
#undef SI
}

template <int NN>
VIC_DEV void store_flux(const KArgs& a, int g, const HruWork<NN>& w, bool glac) {
  const size_t nh = a.nhru;
  double* __restrict__ fx = a.flux;
#define FX(row) fx[(size_t)(row) * nh + g]
  // the three per-HRU precipitation terms are always written: vic_cell_reduce consumes them
  FX(FX_OUT_PREC) = w.out_prec; FX(FX_OUT_RAIN) = w.out_rain; FX(FX_OUT_SNOW) = w.out_snow;
  FX(FX_RUNOFF) = w.runoff; FX(FX_BASEFLOW) = w.baseflow;
  FX(FX_EVAP0) = w.evap[0]; FX(FX_EVAP1) = w.evap[1]; FX(FX_EVAP2) = w.evap[2];
  FX(FX_CANOPYEVAP) = w.vv.canopyevap; FX(FX_SNOW_VAPOR_FLUX) = w.snow.vapor_flux;
  FX(FX_SNOW_CANOPY_VAPOR_FLUX) = w.snow.canopy_vapor_flux; FX(FX_GLAC_MASS_BALANCE) = w.gl.mass_balance;
  if (!a.write_fluxes) return;
  FX(FX_ASAT) = w.asat; FX(FX_INFLOW) = w.inflow; FX(FX_THROUGHFALL) = w.vv.throughfall;
  FX(FX_SNOW_BLOWING_FLUX) = w.snow.blowing_flux; FX(FX_SNOW_SURFACE_FLUX) = w.snow.surface_flux; FX(FX_SNOW_MELT) = w.snow.melt;
  FX(FX_SNOW_MASS_ERROR) = w.snow.mass_error; FX(FX_SNOW_QNET) = w.snow.Qnet;
#pragma unroll
  for (int p = 0; p < NPET; p++) FX(FX_POT_EVAP0 + p) = w.pot_evap[p];
  FX(FX_AERO_RESIST_SURFACE) = w.aero_resist_surface; FX(FX_AERO_RESIST_OVERSTORY) = w.aero_resist_overstory;
  FX(FX_ROOTMOIST) = w.rootmoist; FX(FX_WETNESS) = w.wetness;
  FX(FX_ZWT) = w.zwt.zwt; FX(FX_ZWT2) = w.zwt.zwt2; FX(FX_ZWT3) = w.zwt.zwt3;
#pragma unroll
  for (int l = 0; l < 3; l++) FX(FX_ZWTL0 + l) = w.zwt.lz[l];
  // the frost / thaw fronts exist where find_0_degree_fronts ran (surface_fluxes.c, FROZEN_SOIL); glacier HRUs keep the
  // values initialize_model_state gave them (vicgpu_set_fluxes), as they do in the reference
  if (a.o.FROZEN_SOIL && !glac) {
#pragma unroll
    for (int l = 0; l < 3; l++) { FX(FX_FDEPTH0 + l) = w.so.fdepth[l]; FX(FX_TDEPTH0 + l) = w.so.tdepth[l]; }
  }
  FX(FX_ATMOS_LATENT) = w.AtmosLatent; FX(FX_ATMOS_LATENT_SUB) = w.AtmosLatentSub; FX(FX_ATMOS_SENSIBLE) = w.AtmosSensible;
  FX(FX_LONG_UNDER_IN) = w.LongUnderIn; FX(FX_NET_LONG_ATMOS) = w.NetLongAtmos; FX(FX_NET_LONG_UNDER) = w.so.NetLongUnder;
  FX(FX_NET_SHORT_ATMOS) = w.NetShortAtmos; FX(FX_NET_SHORT_GRND) = w.so.NetShortGrnd; FX(FX_NET_SHORT_UNDER) = w.so.NetShortUnder;
  FX(FX_SHORT_UNDER_IN) = w.ShortUnderIn_avg;
  FX(FX_GLAC_ICE_MASS_BALANCE) = w.gl.ice_mass_balance; FX(FX_GLAC_ACCUMULATION) = w.gl.accumulation;
  FX(FX_GLAC_MELT) = w.gl.melt; FX(FX_GLAC_VAPOR_FLUX) = w.gl.vapor_flux; FX(FX_GLAC_INFLOW) = w.gl.inflow;
  FX(FX_GLAC_OUTFLOW) = w.gl.outflow; FX(FX_GLAC_OUTFLOW_COEF) = w.gl.outflow_coef; FX(FX_GLAC_QNET) = w.gl.Qnet;
  FX(FX_GLAC_COLD_CONTENT) = w.gl.cold_content; FX(FX_GLACIER_FLUX) = w.glacier_flux; FX(FX_DELTACC_GLAC) = w.deltaCC_glac;
  FX(FX_GLACIER_MELT_ENERGY) = w.glacier_melt_energy;
#undef FX
}

// ------------------------------------------------------------------------------------------------ HRU identity
struct HruId { int c, band, veg_idx; bool is_glacier, is_art_bare, run; };

VIC_DEV HruId hru_id(const KArgs& a, int g) {
  const size_t nh = a.nhru;
  HruId id;
  id.c = a.hpi[(size_t)HPI_CELL * nh + g];
  id.band = a.hpi[(size_t)HPI_BAND * nh + g];
  id.veg_idx = a.hpi[(size_t)HPI_VEG_INDEX * nh + g];
  id.is_glacier = a.hpi[(size_t)HPI_IS_GLACIER * nh + g] != 0;
  id.is_art_bare = a.hpi[(size_t)HPI_IS_ARTIFICIAL_BARE * nh + g] != 0;
  const double Cv = a.hpd[(size_t)HPD_CV * nh + g];
  // full_energy.c:220
  const bool active = (Cv > 0.0) || (id.is_glacier && a.o.GLACIER_DYNAMICS && Cv >= 0.0);
  const double area = a.cell_params[(size_t)VICGPU_CP_BAND(CPB_AREAFRACT, id.band, a.o.Nnode, a.o.Nband) * a.ncell + id.c];
  id.run = active && ((area > 0) || (id.is_glacier && a.o.GLACIER_DYNAMICS && area >= 0.0));
  return id;
}

VIC_DEV void store_zero_record(const KArgs& a, int g) {
  const size_t nh = a.nhru;
  double* fx = a.flux;
  fx[(size_t)FX_OUT_PREC * nh + g] = 0; fx[(size_t)FX_OUT_RAIN * nh + g] = 0; fx[(size_t)FX_OUT_SNOW * nh + g] = 0;
  fx[(size_t)FX_RUNOFF * nh + g] = 0; fx[(size_t)FX_BASEFLOW * nh + g] = 0;
  fx[(size_t)FX_EVAP0 * nh + g] = 0; fx[(size_t)FX_EVAP1 * nh + g] = 0; fx[(size_t)FX_EVAP2 * nh + g] = 0;
  fx[(size_t)FX_CANOPYEVAP * nh + g] = 0; fx[(size_t)FX_SNOW_VAPOR_FLUX * nh + g] = 0;
  fx[(size_t)FX_SNOW_CANOPY_VAPOR_FLUX * nh + g] = 0; fx[(size_t)FX_GLAC_MASS_BALANCE * nh + g] = 0;
  a.hru_err[g] = 0;
}

VIC_DEV Soil3 load_soil3(const CellView& cv) {
  Soil3 s3;
#pragma unroll
  for (int l = 0; l < 3; l++) {
    s3.depth[l] = cv.lay(CPL_DEPTH, l); s3.max_moist[l] = cv.lay(CPL_MAX_MOIST, l); s3.Wcr[l] = cv.lay(CPL_WCR, l);
    s3.Wpwp[l] = cv.lay(CPL_WPWP, l); s3.resid_moist[l] = cv.lay(CPL_RESID_MOIST, l);
  }
  return s3;
}
