// vic_copy_cells.hpp — model state copied between cells on the device (vicgpu_copy_cells, include/vicgpu.h): the planning of
// a call on the host, the direct kernel for gfx950 and the launchers of both paths.  Nothing here knows a context: the tables
// are [nrow][ld] arrays of double or int, the pairs are column indices.
//
//   plan_cell_copy     (host, no HIP) checks a call's cell pairs -- range, repeated destination, equal HRU structure position
//                      by position -- before anything is written, drops the identity pairs and turns the rest into cell
//                      pairs (for the per-cell tables) and HRU pairs (the j-th HRU of the destination cell, in CSR order,
//                      takes the j-th of the source cell), both sorted by destination: consecutive lanes then write
//                      consecutive columns where destination cells are contiguous (member-major ensembles).  It also says
//                      whether the direct path is legal: no destination is the source of another remaining pair.
//   vic_copy_direct    T[r][dst_j] = T[r][src_j]: one kernel per table.  Legal on the direct path only -- a lane then reads
//                      columns no lane writes.  Geometry of vic_rows.hpp: a lane is one pair and a tile of ROW_TILE rows
//                      (blockIdx.y); the two indices are loaded once and reused for the tile's rows; a tile's loads are all
//                      issued before its stores.  No LDS, no scratch, plain vector loads and stores.
//   copy_pack          stage[r][j] = T[r][src_j]: vic_rows_gather on consecutive rows
//   copy_unpack        T[r][dst_j] = stage[r][j]: vic_rows_scatter on them.  The staged path, for permutations (every source is
//                      read as it was before the call).  The rows go in passes of at most `rows_per_pass` rows, so the stage
//                      never exceeds a budget; the passes are independent, because a row is read and written within its own pass.
// The kernels trust their indices: plan_cell_copy has checked them.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <string>
#include <unordered_map>
#include <vector>
#include "vic_rows.hpp"

namespace vic {

// ------------------------------------------------------------------------------------------------ planning (host)
enum { COPY_OK = 0, COPY_CELL_RANGE, COPY_DST_REPEATS, COPY_HRU_COUNT, COPY_HRU_STRUCTURE };

struct CopyPairs {
  std::vector<int> dst, src;       // column j of dst takes column j of src; dst ascending, no identity pair
  size_t size() const { return dst.size(); }
};
struct CopyPlan {
  int fault = COPY_OK;             // COPY_*: the first rule a pair breaks
  int index = -1;                  // ... and the pair that breaks it
  bool direct = true;              // no destination is also the source of a remaining pair
  CopyPairs cell, hru;
};

// pairs (dst[i] <- src_of[dst[i]]) for every column with src_of >= 0, ascending: a scan instead of a sort
static inline void copy_pairs_from(const std::vector<int>& src_of, size_t count, CopyPairs& out) {
  out.dst.clear(); out.src.clear();
  out.dst.reserve(count); out.src.reserve(count);
  for (size_t d = 0; d < src_of.size(); d++)
    if (src_of[d] >= 0) { out.dst.push_back((int)d); out.src.push_back(src_of[d]); }
}

// The pair rule for cells d and s (both in range): COPY_OK, or the rule the pair breaks.  cell_off / cell_list / key as below.
static inline int copy_pair_fault(int nhru, const int* cell_off, const int* cell_list, const int* key, int nkey, int d, int s) {
  const int nh = cell_off[d + 1] - cell_off[d];
  if (cell_off[s + 1] - cell_off[s] != nh) return COPY_HRU_COUNT;
  for (int j = 0; j < nh; j++) {
    const int hd = cell_list[cell_off[d] + j], hs = cell_list[cell_off[s] + j];
    for (int k = 0; k < nkey; k++)
      if (key[(size_t)k * nhru + hd] != key[(size_t)k * nhru + hs]) return COPY_HRU_STRUCTURE;
  }
  return COPY_OK;
}

// A class per cell: two cells have the same class exactly when copy_pair_fault gives COPY_OK for them.  A call that compares
// many pairs (vicgpu_mix_cells: every destination with every term) pays for the structure once per domain, not once per pair.
static inline std::vector<int> copy_cell_classes(int ncell, int nhru, const int* cell_off, const int* cell_list, const int* key, int nkey) {
  std::vector<int> cls(ncell > 0 ? ncell : 0, 0);
  std::unordered_map<std::string, int> seen;
  std::string sig;
  for (int c = 0; c < ncell; c++) {
    const int nh = cell_off[c + 1] - cell_off[c];
    sig.resize(sizeof(int) * (size_t)nh * nkey);
    int* w = reinterpret_cast<int*>(&sig[0]);           // nh follows from the length
    for (int j = 0; j < nh; j++)
      for (int k = 0; k < nkey; k++) *w++ = key[(size_t)k * nhru + cell_list[cell_off[c] + j]];
    cls[c] = seen.emplace(sig, (int)seen.size()).first->second;
  }
  return cls;
}

static inline const char* copy_pair_fault_text(int fault) {
  return fault == COPY_HRU_COUNT ? "the cells differ in their number of HRUs"
                                 : "the cells' HRUs differ in band, vegetation class, glacier or bare-soil flag";
}

// cell_off[ncell + 1] / cell_list[nhru]: the domain's CSR; key[nkey][nhru]: the HRU rows a pair must agree in, position by
// position.  Every pair is checked before the plan holds anything.
static inline CopyPlan plan_cell_copy(int ncell, int nhru, const int* cell_off, const int* cell_list, const int* key, int nkey, int n,
                                      const int* dst_cell, const int* src_cell) {
  CopyPlan p;
  const auto fail = [&](int rule, int i) { p.fault = rule; p.index = i; return p; };
  for (int i = 0; i < n; i++)
    if (dst_cell[i] < 0 || dst_cell[i] >= ncell || src_cell[i] < 0 || src_cell[i] >= ncell) return fail(COPY_CELL_RANGE, i);
  std::vector<int> src_of(ncell, -1);          // by destination cell; identity pairs count as destinations too
  for (int i = 0; i < n; i++) {
    if (src_of[dst_cell[i]] >= 0) return fail(COPY_DST_REPEATS, i);
    src_of[dst_cell[i]] = src_cell[i];
  }
  size_t ncp = 0, nhp = 0;
  for (int i = 0; i < n; i++) {
    const int d = dst_cell[i], s = src_cell[i];
    if (d == s) { src_of[d] = -1; continue; }
    const int rule = copy_pair_fault(nhru, cell_off, cell_list, key, nkey, d, s);
    if (rule != COPY_OK) return fail(rule, i);
    ncp++; nhp += cell_off[d + 1] - cell_off[d];
  }
  copy_pairs_from(src_of, ncp, p.cell);
  std::vector<char> is_dst(ncell, 0);
  for (int d : p.cell.dst) is_dst[d] = 1;
  for (int s : p.cell.src) if (is_dst[s]) p.direct = false;
  std::vector<int> hsrc_of(nhru, -1);
  for (size_t i = 0; i < p.cell.size(); i++) {
    const int d = p.cell.dst[i], s = p.cell.src[i];
    for (int j = 0, nh = cell_off[d + 1] - cell_off[d]; j < nh; j++) hsrc_of[cell_list[cell_off[d] + j]] = cell_list[cell_off[s] + j];
  }
  copy_pairs_from(hsrc_of, nhp, p.hru);
  return p;
}

// ------------------------------------------------------------------------------------------------ kernels
template <typename T>
struct CCArgs {
  int npair, nrow;                 // pairs; rows of the table
  size_t ld;                       // columns per row of the table
  const int* dst;                  // [npair]
  const int* src;                  // [npair]
  T* table;                        // [nrow][ld]
};

template <typename T>
__global__ __launch_bounds__(64) void vic_copy_direct(const CCArgs<T> a) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= a.npair) return;
  const int r0 = blockIdx.y * ROW_TILE;
  const T* in = a.table + (size_t)r0 * a.ld + a.src[j];
  T* out = a.table + (size_t)r0 * a.ld + a.dst[j];
  T v[ROW_TILE];
#pragma unroll
  for (int i = 0; i < ROW_TILE; i++)
    if (r0 + i < a.nrow) v[i] = in[(size_t)i * a.ld];
#pragma unroll
  for (int i = 0; i < ROW_TILE; i++)
    if (r0 + i < a.nrow) out[(size_t)i * a.ld] = v[i];
}

// ------------------------------------------------------------------------------------------------ launchers (host)
// every row of table[nrow][ld] on the direct path; d_dst / d_src: the pairs in device memory
template <typename T>
static inline hipError_t copy_direct(hipStream_t st, T* table, size_t ld, int nrow, const int* d_dst, const int* d_src, int npair) {
  if (npair <= 0 || nrow <= 0) return hipSuccess;
  const CCArgs<T> a{npair, nrow, ld, d_dst, d_src, table};
  hipLaunchKernelGGL((vic_copy_direct<T>), rows_grid(npair, nrow), dim3(64), 0, st, a);
  return hipGetLastError();
}

// rows [r0, r0 + nr) of table[..][ld]: the columns d_src[0 .. npair) into stage[nr][npair]
template <typename T>
static inline hipError_t copy_pack(hipStream_t st, const T* table, size_t ld, int r0, int nr, const int* d_src, int npair, T* stage) {
  return rows_gather<T>(st, table + (size_t)r0 * ld, ld, nullptr, nr, d_src, npair, stage);
}

// ... and stage[nr][npair] into the columns d_dst[0 .. npair) of those rows
template <typename T>
static inline hipError_t copy_unpack(hipStream_t st, T* table, size_t ld, int r0, int nr, const int* d_dst, int npair, const T* stage) {
  return rows_scatter<T>(st, table + (size_t)r0 * ld, ld, nullptr, nr, d_dst, npair, stage);
}

// every row of table[nrow][ld] on the staged path, per_pass rows at a time through stage[per_pass][npair]
template <typename T>
static inline hipError_t copy_staged(hipStream_t st, T* table, size_t ld, int nrow, const int* d_dst, const int* d_src, int npair, T* stage,
                                     int per_pass) {
  return for_row_passes(nrow, per_pass, [&](int r0, int nr) {
    const hipError_t e = copy_pack<T>(st, table, ld, r0, nr, d_src, npair, stage);
    return e == hipSuccess ? copy_unpack<T>(st, table, ld, r0, nr, d_dst, npair, stage) : e;
  });
}

}  // namespace vic
