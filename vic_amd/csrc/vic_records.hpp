// vic_records.hpp — the device side of the output records (vicgpu_run_records, include/vicgpu_out.h): the kernel that ends
// an output record for the cells of a launch, and the kernels that reduce a packed record over cell groups
// (vicgpu_records_set_groups).  Device only, gfx950.
//
//   vic_out_pack_reset   the geometry of vic_put_aggregate: one lane = one cell x PUT_AGG_ROWS rows, blockIdx.y over the row
//                        groups.  A row the record selects (sel_pos[r] >= 0) is stored as a float into that row of the
//                        record slot -- the plain cast of vic_out_rows_f32, what WriteOutputNetCDF.c:387-455 writes -- and
//                        every row of the aggregates is set to zero (vicNl.c:599-606).  The row groups' first blocks also
//                        copy the cells' error flags into the slot.
// Consecutive lanes are consecutive cells, so every access is a contiguous row segment; sel_pos[r] is the same for the whole
// wave.  No LDS, a handful of registers.
//
//   vic_out_group_reduce       a wave per group and tile of RG_ROWS rows: reads a slot's [nrow][ncell] floats and the groups'
//                              CSR, writes the slot's [nrow][ngroup] floats.  Member index and weight are loaded once per 64
//                              members and reused for the tile's rows; a contiguous member list reads contiguous row segments.
//   vic_out_group_reduce_lane  a lane per group, for groups of at most one member (a full output grid with a fill value,
//                              where a wave per group would be almost empty).
// Both produce the bits of the summation order include/vicgpu_out.h states: lane l of 64 takes the products w_i * (double)v of
// the members l, l + 64, ... in that order (the first one assigned, not added to zero; +0.0 without a member), then
// p_l = p_l + p_{l+s} for s = 32 .. 1, and the value is (float)p_0.  No LDS, no scratch.
#pragma once
#include <cstddef>
#include "vic_putdata.hpp"

namespace vic {

struct RPArgs {
  int ncell, nrow, c0, ccount;     // cells per row of every table, rows of the aggregates, the cells [c0, c0 + ccount) of the launch
  double* out_agg;                 // [nrow][ncell]
  const int* sel_pos;              // [nrow]: the row of the record an aggregate row goes to, or -1
  const int* cell_err;             // [ncell]
  float* slot_out;                 // [rows of a record][ncell]
  int* slot_err;                   // [ncell]
};

__global__ __launch_bounds__(64) void vic_out_pack_reset(const RPArgs a) {
  const int ci = blockIdx.x * 64 + threadIdx.x;
  if (ci >= a.ccount) return;
  const int c = a.c0 + ci;
  const size_t nc = a.ncell;
  const int r0 = blockIdx.y * PUT_AGG_ROWS;
  double* __restrict__ ag = a.out_agg + c;
  float* __restrict__ so = a.slot_out + c;
#pragma unroll
  for (int i = 0; i < PUT_AGG_ROWS; i++) {
    const int r = r0 + i;
    if (r < a.nrow) {
      const int pos = a.sel_pos[r];
      if (pos >= 0) so[(size_t)pos * nc] = (float)ag[(size_t)r * nc];
      ag[(size_t)r * nc] = 0.0;
    }
  }
  if (blockIdx.y == 0) a.slot_err[c] = a.cell_err[c];
}

constexpr int RG_ROWS = 8;         // rows of a record per launch row (blockIdx.y): accumulators a lane keeps in registers

struct RGArgs {
  int ncell, nrow, ngroup;         // cells per row of the packed record, its rows, columns of the reduced record
  const int* off;                  // [ngroup + 1]
  const int* cell;                 // [off[ngroup]]
  const double* weight;            // [off[ngroup]]
  const float* slot_out;           // [nrow][ncell]
  float* group_out;                // [nrow][ngroup]
  float fill;                      // value of a group without members
};

__global__ __launch_bounds__(64) void vic_out_group_reduce(const RGArgs a) {
  const int g = blockIdx.x, lane = threadIdx.x;      // g < ngroup by the grid; every lane stays to the end (cross-lane sums)
  const int r0 = blockIdx.y * RG_ROWS;
  const int nr = a.nrow - r0 < RG_ROWS ? a.nrow - r0 : RG_ROWS;
  const int i0 = a.off[g], i1 = a.off[g + 1];
  const size_t nc = a.ncell;
  const float* __restrict__ v = a.slot_out + (size_t)r0 * nc;
  double p[RG_ROWS];
#pragma unroll
  for (int r = 0; r < RG_ROWS; r++) p[r] = 0.0;
  for (int base = i0; base < i1; base += 64) {
    const int i = base + lane;
    if (i < i1) {
      const int c = a.cell[i];
      const double w = a.weight[i];
#pragma unroll
      for (int r = 0; r < RG_ROWS; r++)
        if (r < nr) {
          const double t = w * (double)v[(size_t)r * nc + c];
          p[r] = base == i0 ? t : p[r] + t;
        }
    }
  }
  for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
    for (int r = 0; r < RG_ROWS; r++) p[r] = p[r] + __shfl(p[r], lane + s);      // lanes >= s hold values nobody reads
  }
  if (lane == 0) {
    float* __restrict__ o = a.group_out + (size_t)r0 * a.ngroup + g;
#pragma unroll
    for (int r = 0; r < RG_ROWS; r++)
      if (r < nr) o[(size_t)r * a.ngroup] = i1 > i0 ? (float)p[r] : a.fill;
  }
}

__global__ __launch_bounds__(64) void vic_out_group_reduce_lane(const RGArgs a) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= a.ngroup) return;
  const int r0 = blockIdx.y * RG_ROWS;
  const int i0 = a.off[g];
  const bool member = a.off[g + 1] > i0;
  const size_t nc = a.ncell;
  const float* __restrict__ v = a.slot_out + (size_t)r0 * nc + (member ? a.cell[i0] : 0);
  const double w = member ? a.weight[i0] : 0.0;
  float* __restrict__ o = a.group_out + (size_t)r0 * a.ngroup + g;
#pragma unroll
  for (int r = 0; r < RG_ROWS; r++)
    if (r0 + r < a.nrow) {
      // lane 0's only term, then the sums with the +0.0 of the 63 empty lanes: they change -0.0 into +0.0 and nothing else
      o[(size_t)r * a.ngroup] = member ? (float)(w * (double)v[(size_t)r * nc] + 0.0) : a.fill;
    }
}

}  // namespace vic
