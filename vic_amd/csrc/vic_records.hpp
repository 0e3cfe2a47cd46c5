// vic_records.hpp — the device side of the output records (vicgpu_run_records, include/vicgpu_out.h): one kernel (device
// only, gfx950) that ends an output record for the cells of a launch.
//
//   vic_out_pack_reset   the geometry of vic_put_aggregate: one lane = one cell x PUT_AGG_ROWS rows, blockIdx.y over the row
//                        groups.  A row the record selects (sel_pos[r] >= 0) is stored as a float into that row of the
//                        record slot -- the plain cast of vic_out_rows_f32, what WriteOutputNetCDF.c:387-455 writes -- and
//                        every row of the aggregates is set to zero (vicNl.c:599-606).  The row groups' first blocks also
//                        copy the cells' error flags into the slot.
// Consecutive lanes are consecutive cells, so every access is a contiguous row segment; sel_pos[r] is the same for the whole
// wave.  No LDS, a handful of registers.
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

}  // namespace vic
