// vic_params.hpp — cell and HRU parameters updated in place (vicgpu_update_cell_params / vicgpu_update_hru_params,
// include/vicgpu.h): the owner cells of listed HRUs on the host, the listed-cell forms of the two derive kernels of
// vic_aux_kernels.hpp, and their launchers.  The check of a call (check_param_update) and the scatter of its values
// (rows_put_staged: vic_rows_scatter in row passes through a budgeted stage) are those of vic_rows.hpp.  Nothing here knows a
// context: a table is a [..][ld] array of double, the lists are row and column indices.
//
//   param_owner_cells    (host, no HIP) the cells that own the listed HRUs, ascending, each once, from the domain's CSR lists:
//                        the cells whose tree-line rows depend on an updated HPD_CV.
//   vic_derive_cell_params_listed / vic_derive_tree_adjust_listed
//                        lane = listed cell (cells == NULL: cell i), calling derive_cell_params_of / derive_tree_adjust_of,
//                        the bodies of the full-domain kernels.
// The kernels trust their indices: check_param_update has checked them.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <vector>
#include "vic_aux_kernels.hpp"
#include "vic_rows.hpp"

namespace vic {

// ------------------------------------------------------------------------------------------------ plan (host)
// cell_off[ncell + 1] / cell_list[nhru]: the domain's CSR; hrus[n]: checked HRU ids
static inline std::vector<int> param_owner_cells(int ncell, int nhru, const int* cell_off, const int* cell_list, int n, const int* hrus) {
  std::vector<int> owner(nhru > 0 ? nhru : 0, -1);
  for (int c = 0; c < ncell; c++)
    for (int k = cell_off[c]; k < cell_off[c + 1]; k++) owner[cell_list[k]] = c;
  std::vector<char> hit(ncell > 0 ? ncell : 0, 0);
  for (int i = 0; i < n; i++)
    if (owner[hrus[i]] >= 0) hit[owner[hrus[i]]] = 1;
  std::vector<int> cells;
  for (int c = 0; c < ncell; c++)
    if (hit[c]) cells.push_back(c);
  return cells;
}

// ------------------------------------------------------------------------------------------------ kernels
__global__ __launch_bounds__(64) void vic_derive_cell_params_listed(double* cp, int ncell, int Nn, int Nb, const int* cells, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  derive_cell_params_of(cp, ncell, cells ? cells[i] : i, Nn, Nb);
}

__global__ __launch_bounds__(64) void vic_derive_tree_adjust_listed(double* cp, int ncell, int nhru, int Nn, int Nb, const int* cell_off,
                                                                    const int* cell_list, const int* hpi, const double* hpd, const double* veglib,
                                                                    const int* cells, int n) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  derive_tree_adjust_of(cp, ncell, nhru, cells ? cells[i] : i, Nn, Nb, cell_off, cell_list, hpi, hpd, veglib);
}

// ------------------------------------------------------------------------------------------------ launchers (host)
static inline hipError_t derive_cell_params_listed(hipStream_t st, double* cp, int ncell, int Nn, int Nb, const int* d_cells, int n) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(vic_derive_cell_params_listed, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, cp, ncell, Nn, Nb, d_cells, n);
  return hipGetLastError();
}

static inline hipError_t derive_tree_adjust_listed(hipStream_t st, double* cp, int ncell, int nhru, int Nn, int Nb, const int* cell_off,
                                                   const int* cell_list, const int* hpi, const double* hpd, const double* veglib,
                                                   const int* d_cells, int n) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(vic_derive_tree_adjust_listed, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, cp, ncell, nhru, Nn, Nb, cell_off, cell_list,
                     hpi, hpd, veglib, d_cells, n);
  return hipGetLastError();
}

}  // namespace vic
