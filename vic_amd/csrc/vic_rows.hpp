// vic_rows.hpp — listed rows and columns of a [row][column] device table moved through a budgeted stage: what
// vicgpu_copy_cells, vicgpu_update_cell_params / _hru_params, vicgpu_get_state_rows / _update_state, vicgpu_mix_cells and
// vicgpu_member_transform_apply (include/vicgpu.h) and their device-group forms have in common.  The check of a call's lists on the host, the gather and the
// scatter kernel for gfx950, their launchers and the pass loop.  Nothing here knows a context: a table is a [..][ld] array of
// double or int, the lists are row and column indices.
//
//   check_param_update   (host, no HIP) rows and columns of a call: range, a row or a column listed twice, the column count of
//                        the dense form.  Everything is checked before anything is written.  param_fault_message is the text
//                        an entry reports for what the check found.
//   vic_rows_gather<T>   values[k][i] = table[rows[k]][idx[i]].
//   vic_rows_scatter<T, ADD>
//                        table[rows[k]][idx[i]] = values[k][i] (ADD: old + value, one rounded add).
//                        A lane is one listed column i and a tile of ROW_TILE rows (blockIdx.y): its index is loaded once, the
//                        tile's words are all loaded before they are stored, and consecutive lanes touch consecutive words of
//                        a row of `values`.  idx == NULL is the dense form, column i itself: the table side then coalesces like
//                        the values side.  rows == NULL means consecutive rows, row k of the table pointer passed in: the
//                        pack and unpack of a copy between cells.  Plain vector loads and stores, no LDS, no scratch.
//   rows_per_pass / for_row_passes
//                        the rows go through a device stage in passes of at most rows_per_pass rows, so the stage stays within
//                        a budget whatever the table's size; a row is moved within its own pass, so the result does not depend
//                        on the budget.
//   rows_get_staged / rows_put_staged
//                        the passes of a call whose values are the host's.
// The kernels trust their indices: the check has seen them.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <string>
#include <type_traits>
#include <vector>
#include "vic_host.hpp"

namespace vic {

// ------------------------------------------------------------------------------------------------ check (host)
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

// "<entry point>: entry <i>: <rule>"; a rule that no single entry breaks names none
static inline std::string param_fault_message(const char* name, const ParamFault& f) {
  return std::string(name) + ": " + (f.index >= 0 ? "entry " + std::to_string(f.index) + ": " : "") + param_fault_text(f.rule);
}

// ------------------------------------------------------------------------------------------------ passes (host)
// Rows a pass may hold: as many as fit into budget_bytes, at least one, at most all
static inline int rows_per_pass(size_t budget_bytes, size_t ncol, size_t elem_bytes, int nrow) {
  const size_t row = ncol * elem_bytes;
  const size_t fit = row ? budget_bytes / row : (size_t)nrow;
  return fit < 1 ? 1 : (fit > (size_t)nrow ? nrow : (int)fit);
}

// f(r0, nr) for the passes [r0, r0 + nr) of nrow rows, in order, until one does not return zero (hipSuccess, VICGPU_OK): that
// result, or zero
template <typename F>
static inline auto for_row_passes(int nrow, int per_pass, F&& f) -> decltype(f(0, 0)) {
  decltype(f(0, 0)) e{};
  for (int r0 = 0; r0 < nrow && e == decltype(e){}; r0 += per_pass) e = f(r0, nrow - r0 < per_pass ? nrow - r0 : per_pass);
  return e;
}

// ------------------------------------------------------------------------------------------------ kernels
constexpr int ROW_TILE = 8;        // rows per launch row (blockIdx.y): values a lane holds between its loads and its stores

template <typename T>
struct RowsArgs {
  int n, nrow;                     // listed columns; rows of this pass, counted from the entry `rows` and the row `values` point to
  size_t ld;                       // columns per row of the table
  const int* rows;                 // [nrow] table rows, or null: row k
  const int* idx;                  // [n] table columns, or null: column i
  T* values;                       // [nrow][n]: written by the gather, read by the scatter
  T* table;                        // [..][ld]
};

template <typename T>
__global__ __launch_bounds__(64) void vic_rows_gather(const RowsArgs<T> a) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.n) return;
  const int r0 = blockIdx.y * ROW_TILE;
  const size_t col = a.idx ? (size_t)a.idx[i] : (size_t)i;
  T* __restrict__ out = a.values + (size_t)r0 * a.n + i;
  T v[ROW_TILE];
#pragma unroll
  for (int k = 0; k < ROW_TILE; k++)
    if (r0 + k < a.nrow) v[k] = a.table[(size_t)(a.rows ? a.rows[r0 + k] : r0 + k) * a.ld + col];
#pragma unroll
  for (int k = 0; k < ROW_TILE; k++)
    if (r0 + k < a.nrow) out[(size_t)k * a.n] = v[k];
}

template <typename T, bool ADD>
__global__ __launch_bounds__(64) void vic_rows_scatter(const RowsArgs<T> a) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.n) return;
  const int r0 = blockIdx.y * ROW_TILE;
  const size_t col = a.idx ? (size_t)a.idx[i] : (size_t)i;
  const T* __restrict__ in = a.values + (size_t)r0 * a.n + i;
  T v[ROW_TILE];
#pragma unroll
  for (int k = 0; k < ROW_TILE; k++)
    if (r0 + k < a.nrow) {
      v[k] = in[(size_t)k * a.n];
      if (ADD) v[k] = a.table[(size_t)(a.rows ? a.rows[r0 + k] : r0 + k) * a.ld + col] + v[k];
    }
#pragma unroll
  for (int k = 0; k < ROW_TILE; k++)
    if (r0 + k < a.nrow) a.table[(size_t)(a.rows ? a.rows[r0 + k] : r0 + k) * a.ld + col] = v[k];
}

// ------------------------------------------------------------------------------------------------ launchers (host)
static inline dim3 rows_grid(int n, int nr) { return dim3((unsigned)((n + 63) / 64), (unsigned)((nr + ROW_TILE - 1) / ROW_TILE)); }

// d_values[nr][n] = rows d_rows[0 .. nr) (null: 0 .. nr) of table[..][ld], columns d_idx[0 .. n) (null: 0 .. n)
template <typename T>
static inline hipError_t rows_gather(hipStream_t st, const T* table, size_t ld, const int* d_rows, int nr, const int* d_idx, int n, T* d_values) {
  if (n <= 0 || nr <= 0) return hipSuccess;
  const RowsArgs<T> a{n, nr, ld, d_rows, d_idx, d_values, const_cast<T*>(table)};
  hipLaunchKernelGGL(vic_rows_gather<T>, rows_grid(n, nr), dim3(64), 0, st, a);
  return hipGetLastError();
}

// ... and d_values[nr][n] into them; add (double only: no entry adds to an int table): old + value
template <typename T>
static inline hipError_t rows_scatter(hipStream_t st, T* table, size_t ld, const int* d_rows, int nr, const int* d_idx, int n, const T* d_values,
                                      bool add = false) {
  if (n <= 0 || nr <= 0) return hipSuccess;
  const RowsArgs<T> a{n, nr, ld, d_rows, d_idx, const_cast<T*>(d_values), table};
  if constexpr (std::is_same<T, double>::value)
    if (add) {
      hipLaunchKernelGGL((vic_rows_scatter<double, true>), rows_grid(n, nr), dim3(64), 0, st, a);
      return hipGetLastError();
    }
  hipLaunchKernelGGL((vic_rows_scatter<T, false>), rows_grid(n, nr), dim3(64), 0, st, a);
  return hipGetLastError();
}

// The listed rows into values[nrow][n] of the host through stage[per_pass][n].  Every download waits for the stream: the
// values are in place when this returns.
template <typename T>
static inline hipError_t rows_get_staged(hipStream_t st, const T* table, size_t ld, const int* d_rows, int nrow, const int* d_idx, int n, T* values,
                                         T* stage, int per_pass) {
  return for_row_passes(nrow, per_pass, [&](int r0, int nr) {
    const hipError_t e = rows_gather<T>(st, table, ld, d_rows + r0, nr, d_idx, n, stage);
    return e == hipSuccess ? copy_on(st, values + (size_t)r0 * n, stage, sizeof(T) * nr * n, hipMemcpyDeviceToHost) : e;
  });
}

// values[nrow][n] of the host into the listed rows.  Every upload waits for the stream, and so for the pass before it:
// `values` may be reused when this returns, the last kernel may still be running.
template <typename T>
static inline hipError_t rows_put_staged(hipStream_t st, T* table, size_t ld, const int* d_rows, int nrow, const int* d_idx, int n, const T* values,
                                         T* stage, int per_pass, bool add = false) {
  return for_row_passes(nrow, per_pass, [&](int r0, int nr) {
    const hipError_t e = copy_on(st, stage, values + (size_t)r0 * n, sizeof(T) * nr * n, hipMemcpyHostToDevice);
    return e == hipSuccess ? rows_scatter<T>(st, table, ld, d_rows + r0, nr, d_idx, n, stage, add) : e;
  });
}

}  // namespace vic
