// vic_params.hpp — cell and HRU parameters updated in place (vicgpu_update_cell_params / vicgpu_update_hru_params,
// include/vicgpu.h): the check of a call on the host, the scatter kernel for gfx950, the listed-cell forms of the two derive
// kernels of vic_aux_kernels.hpp, and their launchers.  Nothing here knows a context: a table is a [..][ld] array of double,
// the lists are row and column indices.
//
//   check_param_update   (host, no HIP) rows and columns of a call: range, a row or a column listed twice, the column count of
//                        the dense form.  Everything is checked before anything is written.
//   param_owner_cells    (host, no HIP) the cells that own the listed HRUs, ascending, each once, from the domain's CSR lists:
//                        the cells whose tree-line rows depend on an updated HPD_CV.
//   vic_param_scatter    table[rows[k]][idx[i]] = values[k][i].  A lane is one listed column i and a tile of PU_ROWS rows
//                        (blockIdx.y): its index is loaded once, the tile's values are all loaded (consecutive lanes read
//                        consecutive words of a row of `values`) before they are stored.  idx == NULL is the dense form,
//                        column i itself: the stores coalesce like the loads.  Plain vector loads and stores, no LDS.
//   vic_derive_cell_params_listed / vic_derive_tree_adjust_listed
//                        lane = listed cell (cells == NULL: cell i), calling derive_cell_params_of / derive_tree_adjust_of,
//                        the bodies of the full-domain kernels.
//   param_scatter_staged the values of a call go through a device stage in row passes of at most rows_per_pass rows
//                        (copy_rows_per_pass, vic_copy_cells.hpp), so the stage stays within a budget whatever the table's size;
//                        a row is written within its own pass, so the result does not depend on the budget.
// The kernels trust their indices: check_param_update has checked them.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <vector>
#include "vic_aux_kernels.hpp"
#include "vic_copy_cells.hpp"
#include "vic_host.hpp"

namespace vic {

// ------------------------------------------------------------------------------------------------ check and plan (host)
enum { PARAM_OK = 0, PARAM_ROW_RANGE, PARAM_ROW_REPEATS, PARAM_COL_RANGE, PARAM_COL_REPEATS, PARAM_DENSE_COUNT };

struct ParamFault {
  int rule = PARAM_OK;             // PARAM_*: the first rule the call breaks
  int index = -1;                  // ... and the entry of `rows` / `cols` that breaks it
};

// rows[nrow] of a table of table_rows rows, cols[n] of its ncol columns (cols == nullptr: the dense form, n must be ncol)
static inline ParamFault check_param_update(int table_rows, int ncol, int nrow, const int* rows, int n, const int* cols) {
  ParamFault f;
  const auto fail = [&](int rule, int i) { f.rule = rule; f.index = i; return f; };
  std::vector<char> seen_row(table_rows > 0 ? table_rows : 0, 0);
  for (int k = 0; k < nrow; k++) {
    if (rows[k] < 0 || rows[k] >= table_rows) return fail(PARAM_ROW_RANGE, k);
    if (seen_row[rows[k]]) return fail(PARAM_ROW_REPEATS, k);
    seen_row[rows[k]] = 1;
  }
  if (!cols) return n == ncol ? f : fail(PARAM_DENSE_COUNT, -1);
  std::vector<char> seen_col(ncol > 0 ? ncol : 0, 0);
  for (int i = 0; i < n; i++) {
    if (cols[i] < 0 || cols[i] >= ncol) return fail(PARAM_COL_RANGE, i);
    if (seen_col[cols[i]]) return fail(PARAM_COL_REPEATS, i);
    seen_col[cols[i]] = 1;
  }
  return f;
}

static inline const char* param_fault_text(int rule) {
  return rule == PARAM_ROW_RANGE ? "a row is outside the table"
         : rule == PARAM_ROW_REPEATS ? "a row is listed twice"
         : rule == PARAM_COL_RANGE ? "a column is outside the domain"
         : rule == PARAM_COL_REPEATS ? "a column is listed twice"
                                     : "no list, but n is not the number of columns";
}

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
constexpr int PU_ROWS = 8;         // rows per launch row (blockIdx.y): values a lane holds between its loads and its stores

struct PUArgs {
  int n, nrow;                     // listed columns; rows of this pass, counted from the entry `rows` and the row `values` point to
  size_t ld;                       // columns per row of the table
  const int* rows;                 // [nrow] table rows
  const int* idx;                  // [n] table columns, or null: column i
  const double* values;            // [nrow][n]
  double* table;                   // [..][ld]
};

__global__ __launch_bounds__(64) void vic_param_scatter(const PUArgs a) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.n) return;
  const int r0 = blockIdx.y * PU_ROWS;
  const size_t col = a.idx ? (size_t)a.idx[i] : (size_t)i;
  const double* __restrict__ in = a.values + (size_t)r0 * a.n + i;
  double v[PU_ROWS];
#pragma unroll
  for (int k = 0; k < PU_ROWS; k++)
    if (r0 + k < a.nrow) v[k] = in[(size_t)k * a.n];
#pragma unroll
  for (int k = 0; k < PU_ROWS; k++)
    if (r0 + k < a.nrow) a.table[(size_t)a.rows[r0 + k] * a.ld + col] = v[k];
}

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
// rows d_rows[0 .. nr) of table[..][ld], columns d_idx[0 .. n) (null: 0 .. n), from d_values[nr][n] in device memory
static inline hipError_t param_scatter(hipStream_t st, double* table, size_t ld, const int* d_rows, int nr, const int* d_idx, int n,
                                       const double* d_values) {
  if (n <= 0 || nr <= 0) return hipSuccess;
  PUArgs a;
  a.n = n; a.nrow = nr; a.ld = ld; a.rows = d_rows; a.idx = d_idx; a.values = d_values; a.table = table;
  hipLaunchKernelGGL(vic_param_scatter, dim3((unsigned)((n + 63) / 64), (unsigned)((nr + PU_ROWS - 1) / PU_ROWS)), dim3(64), 0, st, a);
  return hipGetLastError();
}

// values[nrow][n] of the host through stage[rows_per_pass][n], rows_per_pass rows at a time.  Every upload waits for the
// stream, and so for the pass before it: `values` may be reused when this returns, the last kernel may still be running.
static inline hipError_t param_scatter_staged(hipStream_t st, double* table, size_t ld, const int* d_rows, int nrow, const int* d_idx, int n,
                                              const double* values, double* stage, int rows_per_pass) {
  hipError_t e = hipSuccess;
  for (int r0 = 0; r0 < nrow && e == hipSuccess; r0 += rows_per_pass) {
    const int nr = nrow - r0 < rows_per_pass ? nrow - r0 : rows_per_pass;
    e = copy_on(st, stage, values + (size_t)r0 * n, sizeof(double) * nr * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = param_scatter(st, table, ld, d_rows + r0, nr, d_idx, n, stage);
  }
  return e;
}

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
