// vic_mix_cells.hpp — model state combined linearly across cells on the device (vicgpu_mix_cells, include/vicgpu.h): the
// ensemble transform of a filter, x_a[m] = sum over m' of W[m'][m] * x_f[m'], inflation, recentring.  The planning of a call on
// the host, the gather-multiply-add kernel for gfx950 and its launchers.  Nothing here knows a context: the table is a
// [..][ld] array of double, the lists are row, cell and HRU indices, the CSR is passed in.
//
//   plan_cell_mix      (host, no HIP) checks a call -- rows, destinations, offsets, term cells, weights, and every destination /
//                      term pair under the pair rule of plan_cell_copy (copy_cell_classes) -- before anything is written, and
//                      lists the destination HRUs in ascending HRU id (consecutive lanes then write consecutive stage columns
//                      and, where destination cells are contiguous, read consecutive table columns), each with the index i of
//                      its destination in the caller's list and its position j in the cell.  The term lists stay per cell.
//   vic_mix_cells      stage[k][lane] = w_0 * x_0, then + (w_t * x_t) for t = 1, 2, ... in list order, every product and every
//                      sum rounded once (the build has -ffp-contract=off), x_t = table[rows[k]][the j-th HRU of term cell t].
//                      A lane is one destination HRU and a tile of MX_ROWS rows (blockIdx.y).  It walks its destination's
//                      terms in order, resolves a term's source column once from the device's CSR and reuses it for the
//                      tile's rows; a term's loads are all issued, and the next term's column resolved, before the dependent
//                      adds: the row tile gives MX_ROWS independent chains.  Accumulators in registers, no LDS, no scratch,
//                      plain vector loads and stores.  A zero weight still reads its operand.
//   mix_cells_staged   the rows go in passes of at most per_pass rows (rows_per_pass, vic_rows.hpp) through stage[..][n], and each
//                      pass is scattered into table[rows[k]][hru] by rows_scatter (SET).  The result always goes through the
//                      stage: every source is read before any destination is written.  A row is read and written within its
//                      own pass, so the result does not depend on the budget.
// The kernel trusts its indices: plan_cell_mix has checked them.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include <string>
#include <vector>
#include "vic_copy_cells.hpp"      // the pair rule: copy_pair_fault, copy_pair_fault_text
#include "vic_rows.hpp"

namespace vic {

// ------------------------------------------------------------------------------------------------ planning (host)
enum { MIX_OK = 0, MIX_ROW_RANGE, MIX_ROW_REPEATS, MIX_DST_RANGE, MIX_DST_REPEATS, MIX_OFFSETS, MIX_NO_TERM, MIX_TERM_RANGE, MIX_WEIGHT,
       MIX_HRU_COUNT, MIX_HRU_STRUCTURE };

struct MixPlan {
  int fault = MIX_OK;              // MIX_*: the first rule the call breaks
  int row = -1;                    // the entry of `rows` that breaks it, or
  int dst = -1, term = -1;         // the destination (index into dst_cell) and the term (index into term_cell), where there is one
  std::vector<int> hru;            // destination HRUs, ascending
  std::vector<int> dst_index;      // [hru.size()] the HRU's destination: index i into dst_cell / term_off
  std::vector<int> pos;            // [hru.size()] its position j in the cell, in cell_list order
  size_t size() const { return hru.size(); }
  // Workspace, by HRU: (i, j) of a destination HRU while a plan is made, (-1, -1) everywhere between two plans.  A plan that is
  // reused for the next call (the analysis of every cycle of an ensemble loop) keeps its pages instead of faulting them in again.
  struct Where { int i, j; };
  std::vector<Where> where;
};

// cell_off[ncell + 1] / cell_list[nhru] / key[nkey][nhru] as for plan_cell_copy, cell_class[ncell] = copy_cell_classes of them
// (a destination / term pair is legal when the classes agree); rows[nrow] of a table of table_rows rows;
// destination dst_cell[i] has the terms term_off[i] .. term_off[i + 1] - 1 of term_cell / term_weight.  Every list is checked
// before the plan holds anything.  `p` may be the plan of an earlier call on the same domain: its memory is reused.
static inline void plan_cell_mix(MixPlan& p, int ncell, int nhru, const int* cell_off, const int* cell_list, const int* key, int nkey,
                                 const int* cell_class, int table_rows, int nrow, const int* rows, int ndst, const int* dst_cell,
                                 const int* term_off, const int* term_cell, const double* term_weight) {
  p.fault = MIX_OK; p.row = p.dst = p.term = -1;
  p.hru.clear(); p.dst_index.clear(); p.pos.clear();
  const auto fail = [&](int rule, int i, int t) { p.fault = rule; p.dst = i; p.term = t; };
  const ParamFault rf = check_param_update(table_rows, 0, nrow, rows, 0, nullptr);
  if (rf.rule != PARAM_OK) {
    p.fault = rf.rule == PARAM_ROW_RANGE ? MIX_ROW_RANGE : MIX_ROW_REPEATS; p.row = rf.index;
    return;
  }
  std::vector<int> index_of(ncell > 0 ? ncell : 0, -1);      // by destination cell: its index in the caller's list
  if (ndst > 0 && term_off[0] != 0) return fail(MIX_OFFSETS, 0, -1);
  for (int i = 0; i < ndst; i++) {
    const int d = dst_cell[i];
    if (d < 0 || d >= ncell) return fail(MIX_DST_RANGE, i, -1);
    if (index_of[d] >= 0) return fail(MIX_DST_REPEATS, i, -1);
    index_of[d] = i;
    if (term_off[i + 1] < term_off[i]) return fail(MIX_OFFSETS, i, -1);
    if (term_off[i + 1] == term_off[i]) return fail(MIX_NO_TERM, i, -1);
  }
  size_t nh = 0;
  for (int i = 0; i < ndst; i++) {
    const int d = dst_cell[i];
    for (int t = term_off[i]; t < term_off[i + 1]; t++) {
      const int s = term_cell[t];
      if (s < 0 || s >= ncell) return fail(MIX_TERM_RANGE, i, t);
      if (!std::isfinite(term_weight[t])) return fail(MIX_WEIGHT, i, t);
      if (cell_class[s] != cell_class[d])
        return fail(copy_pair_fault(nhru, cell_off, cell_list, key, nkey, d, s) == COPY_HRU_COUNT ? MIX_HRU_COUNT : MIX_HRU_STRUCTURE, i, t);
    }
    nh += (size_t)(cell_off[d + 1] - cell_off[d]);
  }
  // the destination HRUs ascending: a scan instead of a sort
  std::vector<MixPlan::Where>& where = p.where;
  if (where.size() != (size_t)(nhru > 0 ? nhru : 0)) where.assign(nhru > 0 ? nhru : 0, MixPlan::Where{-1, -1});
  for (int i = 0; i < ndst; i++) {
    const int d = dst_cell[i];
    for (int j = 0, n = cell_off[d + 1] - cell_off[d]; j < n; j++) where[cell_list[cell_off[d] + j]] = MixPlan::Where{i, j};
  }
  p.hru.resize(nh); p.dst_index.resize(nh); p.pos.resize(nh);
  size_t k = 0;
  for (int h = 0; h < nhru; h++)
    if (where[h].i >= 0) {
      p.hru[k] = h; p.dst_index[k] = where[h].i; p.pos[k] = where[h].j; k++;
      where[h] = MixPlan::Where{-1, -1};
    }
}

static inline std::string mix_fault_text(const MixPlan& p) {
  const char* rule = p.fault == MIX_ROW_RANGE ? "a row is outside the table"
                     : p.fault == MIX_ROW_REPEATS ? "a row is listed twice"
                     : p.fault == MIX_DST_RANGE ? "the destination cell is outside the domain"
                     : p.fault == MIX_DST_REPEATS ? "the destination repeats"
                     : p.fault == MIX_OFFSETS ? "term_off does not start at 0 or decreases"
                     : p.fault == MIX_NO_TERM ? "the destination has no term"
                     : p.fault == MIX_TERM_RANGE ? "the term cell is outside the domain"
                     : p.fault == MIX_WEIGHT ? "the weight is not finite"
                                             : copy_pair_fault_text(p.fault == MIX_HRU_COUNT ? COPY_HRU_COUNT : COPY_HRU_STRUCTURE);
  std::string where = p.row >= 0 ? "row entry " + std::to_string(p.row) : "destination " + std::to_string(p.dst);
  if (p.term >= 0) where += ", term " + std::to_string(p.term);
  return "mix_cells: " + where + ": " + rule;
}

// ------------------------------------------------------------------------------------------------ kernel
constexpr int MX_ROWS = ROW_TILE;  // rows per launch row (blockIdx.y): the independent accumulator chains of a lane

struct MXArgs {
  int n, nrow;                     // destination HRUs; rows of this pass, counted from the entry `rows` and the row `stage` point to
  size_t ld;                       // columns per row of the table
  const int* rows;                 // [nrow] table rows
  const int* dst_index;            // [n] destination i of the lane's HRU
  const int* pos;                  // [n] its position j in the cell
  const int* term_off;             // [ndst + 1]
  const int* term_cell;            // [nnz]
  const double* term_weight;       // [nnz]
  const int* cell_off;             // [ncell + 1] the domain's CSR
  const int* cell_list;            // [nhru]
  const double* table;             // [..][ld]
  double* stage;                   // [nrow][n]
};

__global__ __launch_bounds__(64) void vic_mix_cells(const MXArgs a) {
  const int lane = blockIdx.x * 64 + threadIdx.x;
  if (lane >= a.n) return;
  const int r0 = blockIdx.y * MX_ROWS;
  const int i = a.dst_index[lane], j = a.pos[lane];
  const int t1 = a.term_off[i + 1];
  int t = a.term_off[i];
  const double* __restrict__ row[MX_ROWS];
#pragma unroll
  for (int k = 0; k < MX_ROWS; k++) row[k] = a.table + (size_t)a.rows[r0 + k < a.nrow ? r0 + k : r0] * a.ld;
  size_t col = (size_t)a.cell_list[a.cell_off[a.term_cell[t]] + j];
  double w = a.term_weight[t];
  double acc[MX_ROWS], x[MX_ROWS];
#pragma unroll
  for (int k = 0; k < MX_ROWS; k++)
    if (r0 + k < a.nrow) x[k] = row[k][col];
  for (bool first = true;; first = false) {
    // the next term's column, weight and loads are issued before the adds of this one
    const bool more = ++t < t1;
    double wn = 0.0, xn[MX_ROWS];
    if (more) {
      col = (size_t)a.cell_list[a.cell_off[a.term_cell[t]] + j];
      wn = a.term_weight[t];
#pragma unroll
      for (int k = 0; k < MX_ROWS; k++)
        if (r0 + k < a.nrow) xn[k] = row[k][col];
    }
#pragma unroll
    for (int k = 0; k < MX_ROWS; k++) acc[k] = first ? w * x[k] : acc[k] + w * x[k];       // the first term is assigned, not added to zero
    if (!more) break;
    w = wn;
#pragma unroll
    for (int k = 0; k < MX_ROWS; k++) x[k] = xn[k];
  }
  double* __restrict__ out = a.stage + (size_t)r0 * a.n + lane;
#pragma unroll
  for (int k = 0; k < MX_ROWS; k++)
    if (r0 + k < a.nrow) out[(size_t)k * a.n] = acc[k];
}

// ------------------------------------------------------------------------------------------------ launchers (host)
// The lists of a call in device memory: d_rows[nrow], and per destination HRU d_hru / d_dst_index / d_pos [n]
struct MixLists {
  const int *rows, *hru, *dst_index, *pos, *term_off, *term_cell;
  const double* term_weight;
  const int *cell_off, *cell_list;
};

// stage[nr][n] = the mix of rows d_rows[r0 .. r0 + nr) of table[..][ld]
static inline hipError_t mix_cells_pass(hipStream_t st, const double* table, size_t ld, const MixLists& l, int r0, int nr, int n, double* stage) {
  if (n <= 0 || nr <= 0) return hipSuccess;
  MXArgs a;
  a.n = n; a.nrow = nr; a.ld = ld; a.rows = l.rows + r0; a.dst_index = l.dst_index; a.pos = l.pos; a.term_off = l.term_off;
  a.term_cell = l.term_cell; a.term_weight = l.term_weight; a.cell_off = l.cell_off; a.cell_list = l.cell_list; a.table = table; a.stage = stage;
  hipLaunchKernelGGL(vic_mix_cells, dim3((unsigned)((n + 63) / 64), (unsigned)((nr + MX_ROWS - 1) / MX_ROWS)), dim3(64), 0, st, a);
  return hipGetLastError();
}

// every listed row, per_pass rows at a time through stage[per_pass][n]: the mix of a pass, then its scatter into
// table[rows[k]][hru].  The scatter of a pass follows its mix on the stream, and the next pass reads other rows.
static inline hipError_t mix_cells_staged(hipStream_t st, double* table, size_t ld, const MixLists& l, int nrow, int n, double* stage, int per_pass) {
  return for_row_passes(nrow, per_pass, [&](int r0, int nr) {
    const hipError_t e = mix_cells_pass(st, table, ld, l, r0, nr, n, stage);
    return e == hipSuccess ? rows_scatter<double>(st, table, ld, l.rows + r0, nr, l.hru, n, stage) : e;
  });
}

}  // namespace vic
