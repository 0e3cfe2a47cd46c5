// vic_state_update.hpp — model state read and changed in place, row by row, and its dependent soil rows re-derived on the
// device (vicgpu_get_state_rows / vicgpu_update_state / vicgpu_derive_soil_state, include/vicgpu.h): the analysis update of an
// ensemble loop, and the tail of a restart.  The check of a derive on the host, the derive kernel for gfx950 and its launcher.
// Reading and writing the rows is vic_rows.hpp as it stands: check_param_update, then rows_get_staged (vic_rows_gather) or
// rows_put_staged (vic_rows_scatter, SET or ADD) on the SD or the SI table.  Nothing here knows a context: a table is a
// [..][ld] array, the lists are row and column indices, the parameter tables are passed in (as in vic_params.hpp).
//
//   check_derive_what    the stage bits of a derive.
//   vic_derive_soil_state<NN>
//                        lane = listed HRU.  The tail of initialize_model_state.c for one HRU, stage by stage, through the
//                        device functions the step itself calls (vic_soil.hpp): the moisture cap (:397-434),
//                        distribute_node_moisture_properties (:712), estimate_layer_ice_content(_quick_flux) (:728-732),
//                        find_0_degree_fronts (:736-737).  A stage's rows are stored before the next stage starts, and a
//                        later stage reads what the earlier ones left.  Plain vector loads and stores, no LDS.
// The kernel trusts its indices: the check has seen them.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "vic_hru_io.hpp"
#include "vic_rows.hpp"

namespace vic {

// ------------------------------------------------------------------------------------------------ check (host)
constexpr int DERIVE_ALL = VICGPU_DERIVE_CAP_MOIST | VICGPU_DERIVE_NODES | VICGPU_DERIVE_LAYERS | VICGPU_DERIVE_FRONTS;
enum { DERIVE_OK = 0, DERIVE_WHAT, DERIVE_UNSUPPORTED };
enum { ROWS_GET = 0, ROWS_SET, ROWS_ADD };      // what a call does with its listed rows

// the stage bits of a vicgpu_derive_soil_state call under the options of the context
static inline int check_derive_what(int what, int glacier_dynamics) {
  if (what == 0 || (what & ~DERIVE_ALL)) return DERIVE_WHAT;
  // the reference keeps the moisture above max_moist in cell.excess_moist (initialize_model_state.c:410), which no table carries
  if ((what & VICGPU_DERIVE_CAP_MOIST) && glacier_dynamics) return DERIVE_UNSUPPORTED;
  return DERIVE_OK;
}

// ------------------------------------------------------------------------------------------------ derive kernel
struct DSArgs {
  Opt o;
  int ncell, nhru;
  int n;                           // listed HRUs
  int what;                        // VICGPU_DERIVE_* bits, checked
  const int* hrus;                 // [n] HRU columns, or null: HRU i
  const double* cp;                // [VIC_CPX_NROW][ncell]: the caller's rows and the library's appended ones
  const int* hpi;                  // [HPI_NROW][nhru]
  const double* hpd;               // [HPD_NROW][nhru]
  double* sd;                      // [VICGPU_SD_NROW][nhru]
  int* si;                         // [VICGPU_SI_NROW][nhru]
  double* flux;                    // [FX_NROW][nhru]
  int* cell_err;                   // [ncell] flag words
};

template <int NN>
__global__ __launch_bounds__(64) void vic_derive_soil_state(const DSArgs a) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.n) return;
  const int g = a.hrus ? a.hrus[i] : i;
  const Opt& o = a.o;
  const int Nn = o.Nnode;
  const size_t nh = a.nhru;
  double* __restrict__ sd = a.sd;
#define SD(row) sd[(size_t)(row) * nh + g]
  const int c = a.hpi[(size_t)HPI_CELL * nh + g], band = a.hpi[(size_t)HPI_BAND * nh + g];
  const CellView cv{a.cp, a.ncell, c, Nn, o.Nband};
  const Soil3 s3 = load_soil3(cv);
  double moist[3], ice[3];
#pragma unroll
  for (int l = 0; l < 3; l++) { moist[l] = SD(SD_MOIST0 + l); ice[l] = SD(SD_ICE0 + l); }

  // initialize_model_state.c:405-432, every HRU of the list whatever its area
  if (a.what & VICGPU_DERIVE_CAP_MOIST) {
#pragma unroll
    for (int l = 0; l < 3; l++) {
      if (moist[l] > s3.max_moist[l]) {
        ice[l] *= s3.max_moist[l] / moist[l];
        moist[l] = s3.max_moist[l];
      }
      if (ice[l] > moist[l]) ice[l] = moist[l];
      SD(SD_MOIST0 + l) = moist[l]; SD(SD_ICE0 + l) = ice[l];
    }
  }

  // :692-694, :740-747: an HRU without area gets empty node blocks and nothing else
  const bool live = a.hpd[(size_t)HPD_CV * nh + g] > 0 && cv.band(CPB_AREAFRACT, band) > 0.;
  if (!live) {
    if (a.what & VICGPU_DERIVE_NODES) {
#pragma unroll
      for (int n = 0; n < NN; n++)
        if (n < Nn) {
          SD(VICGPU_SD_NODE(SDN_MOIST, n, Nn)) = 0; SD(VICGPU_SD_NODE(SDN_ICE, n, Nn)) = 0;
          SD(VICGPU_SD_NODE(SDN_KAPPA, n, Nn)) = 0; SD(VICGPU_SD_NODE(SDN_CS, n, Nn)) = 0;
        }
    }
    return;
  }

  Nodes<NN> nd;
#pragma unroll
  for (int n = 0; n < NN; n++) {
    nd.T[n] = (n < Nn) ? SD(VICGPU_SD_NODE(SDN_T, n, Nn)) : 0.0;
    nd.moist[n] = 0; nd.ice[n] = 0; nd.kappa[n] = 0; nd.Cs[n] = 0;
  }

  if (a.what & VICGPU_DERIVE_NODES) {                                       // :712
    distribute_node_moisture_properties<NN>(o, cv, s3, nd, moist);
#pragma unroll
    for (int n = 0; n < NN; n++)
      if (n < Nn) {
        SD(VICGPU_SD_NODE(SDN_MOIST, n, Nn)) = nd.moist[n]; SD(VICGPU_SD_NODE(SDN_ICE, n, Nn)) = nd.ice[n];
        SD(VICGPU_SD_NODE(SDN_KAPPA, n, Nn)) = nd.kappa[n]; SD(VICGPU_SD_NODE(SDN_CS, n, Nn)) = nd.Cs[n];
      }
  }

  if (a.what & VICGPU_DERIVE_LAYERS) {                                      // :728-732
    double lT[3];
#pragma unroll
    for (int l = 0; l < 3; l++) lT[l] = SD(SD_LAYER_T0 + l);
    if (o.QUICK_FLUX) estimate_layer_ice_content_quick_flux(o, cv, s3, nd.T[0], nd.T[1], moist, ice, lT);
    else if (!estimate_layer_ice_content<NN>(o, cv, s3, nd.T, moist, ice, lT)) atomicOr(a.cell_err + c, (int)VICGPU_CELLERR_NODES);
    // the layers behind a failing one come back as they were loaded
#pragma unroll
    for (int l = 0; l < 3; l++) { SD(SD_ICE0 + l) = ice[l]; SD(SD_LAYER_T0 + l) = lT[l]; }
  }

  if ((a.what & VICGPU_DERIVE_FRONTS) && !o.QUICK_FLUX && cv.s(CP_FS_ACTIVE) != 0.0) {      // :736-737
    SoilEnergy e;
    find_0_degree_fronts<NN>(o, cv, e, nd.T);
    a.si[(size_t)SI_NFROST * nh + g] = e.Nfrost; a.si[(size_t)SI_NTHAW * nh + g] = e.Nthaw;
#pragma unroll
    for (int f = 0; f < 3; f++) {
      a.flux[(size_t)(FX_FDEPTH0 + f) * nh + g] = e.fdepth[f]; a.flux[(size_t)(FX_TDEPTH0 + f) * nh + g] = e.tdepth[f];
    }
  }
#undef SD
}

// ------------------------------------------------------------------------------------------------ launchers (host)
template <int NN>
static inline hipError_t derive_soil_state_nn(hipStream_t st, const DSArgs& a) {
  hipLaunchKernelGGL(vic_derive_soil_state<NN>, dim3((unsigned)((a.n + 63) / 64)), dim3(64), 0, st, a);
  return hipGetLastError();
}

// the instantiation the node count runs on (node_bound), as the step kernels
static inline hipError_t derive_soil_state(hipStream_t st, const DSArgs& a) {
  if (a.n <= 0) return hipSuccess;
  const int b = node_bound(a.o.Nnode);
  return b == 10 ? derive_soil_state_nn<10>(st, a) : b == VIC_MID_NODES ? derive_soil_state_nn<VIC_MID_NODES>(st, a) : derive_soil_state_nn<VIC_MAX_NODES>(st, a);
}

}  // namespace vic
