// vic_member_transform.hpp — the per-column ensemble transform of a localised filter solved and applied on the device
// (vicgpu_member_transform_solve / _set / _get / _apply, include/vicgpu.h).  The checks of a call on the host, the batched
// Jacobi eigen-solver and the apply kernel for gfx950, and their launchers.  Nothing here knows a context: the transform is a
// [ncol][M][M] array of double, the table a [..][ld] array, the lists are row, column, cell and HRU indices, the CSR is
// passed in.  The ensemble is member-major (domain.tile_members): cell m * ncol + j is member m of base column j.
//
//   check_transform_solve  (host, no HIP) the observation lists of a solve: offsets, finite values, rinv >= 0, infl > 0.
//   vic_member_transform_solve<MB>
//                      one wave per base column, M <= MB members, the matrix A and the accumulated eigenvectors U in LDS
//                      ([MB][MB + 1]: the odd row pitch keeps a column walk off one bank).  Hunt et al. (2007): per observation
//                      p, in order, ybar = (hx[p][0] + hx[p][1] + ...) / M, Y[a] = hx[p][a] - ybar, C[a][b] += (rinv * Y[a]) * Y[b]
//                      for a <= b (mirrored afterwards, so A is symmetric to the bit), g[a] += (rinv * Y[a]) * (yobs - ybar);
//                      A = C + ((M - 1) / rho) I.  Parallel cyclic Jacobi: round-robin pairing, M / 2 disjoint rotations per
//                      step (lane k owns pair k and computes its c and s; then all lanes rotate the columns of A and U, then
//                      the rows of A), M - 1 steps per sweep; a pair with |a_pq| <= eps * sqrt(a_pp * a_qq) is skipped, and a
//                      sweep that rotates nothing ends the iteration.  Then wbar = U diag(1 / lam) U^T g,
//                      Wa = (U diag(s^1/2)) (U diag(s^1/2))^T with s = sqrt((M - 1) / lam) -- symmetric to the bit, and one
//                      matrix of LDS less than U diag(s) U^T --, W = Wa + wbar, and T = W + (1 - column sum of W) / M with
//                      the column sum compensated (two-sum), so that a column of T sums to 1 within the rounding of its own
//                      entries.  T_j is written in consecutive words by consecutive lanes.  A column without information
//                      (no observation, or every rinv == 0) rotates nothing and gets the closed form
//                      sqrt(rho) I + (1 - sqrt(rho)) / M (sqrt(rho) is the host's); a column that is still rotating at the
//                      sweep cap gets the identity and info -1.  Every order above is fixed and a column sees no other column:
//                      the bits repeat from run to run and do not depend on the rest of the call.  No scratch, plain vector
//                      loads and stores; every lane stays to the end (the barriers are the wave's).
//   plan_transform_apply   (host, no HIP) checks the rows, the columns and, for every listed column, its members under the pair
//                      rule of plan_cell_copy (copy_cell_classes) before anything is written, and lists the destination HRUs
//                      ascending, each with its cell and its position in the cell.
//   vic_member_transform_apply
//                      vic_mix_cells with an implied term walk: a lane is one destination HRU (member m of column j, position
//                      k) and a tile of ROW_TILE rows; term m' = 0 .. M - 1 is the k-th HRU of cell m' * ncol + j with the
//                      weight T[j][m'][m].  The arithmetic is vic_mix_cells' own: p = w_0 * x_0, then p = p + w_m' * x_m', every
//                      product and sum rounded once, a zero weight still reads its operand.
//   transform_apply_staged  the passes of vic_mix_cells.hpp: rows through stage[..][n], then rows_scatter.
// The kernels trust their indices: the checks have seen them.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <string>
#include <vector>
#include "vic_copy_cells.hpp"      // the pair rule: copy_pair_fault, copy_pair_fault_text
#include "vic_rows.hpp"

namespace vic {

constexpr int MT_MAX_MEMBERS = 64;   // VICGPU_TRANSFORM_MAX_MEMBERS: a column's members are the lanes of one wave

// ------------------------------------------------------------------------------------------------ checks (host)
enum { MT_OK = 0, MT_OFFSETS, MT_HX, MT_YOBS, MT_RINV, MT_INFL, MT_ROW_RANGE, MT_ROW_REPEATS, MT_COL_RANGE, MT_COL_REPEATS,
       MT_DENSE_COUNT, MT_HRU_COUNT, MT_HRU_STRUCTURE };

struct SolveFault {
  int rule = MT_OK;                // MT_*: the first rule the call breaks
  long long index = -1;            // ... and the column or the observation that breaks it
};

// obs_off[ncol + 1]; hx[nobs][M], yobs[nobs], rinv[nobs] with nobs = obs_off[ncol]; infl[ncol] or null
static inline SolveFault check_transform_solve(int M, int ncol, const int* obs_off, const double* hx, const double* yobs, const double* rinv,
                                               const double* infl) {
  SolveFault f;
  const auto fail = [&](int rule, long long i) { f.rule = rule; f.index = i; return f; };
  if (obs_off[0] != 0) return fail(MT_OFFSETS, 0);
  for (int j = 0; j < ncol; j++)
    if (obs_off[j + 1] < obs_off[j]) return fail(MT_OFFSETS, j);
  const int nobs = obs_off[ncol];
  for (int p = 0; p < nobs; p++) {
    for (int m = 0; m < M; m++)
      if (!std::isfinite(hx[(size_t)p * M + m])) return fail(MT_HX, p);
    if (!std::isfinite(yobs[p])) return fail(MT_YOBS, p);
    if (!std::isfinite(rinv[p]) || rinv[p] < 0) return fail(MT_RINV, p);
  }
  if (infl)
    for (int j = 0; j < ncol; j++)
      if (!std::isfinite(infl[j]) || !(infl[j] > 0)) return fail(MT_INFL, j);
  return f;
}

static inline std::string solve_fault_text(const SolveFault& f) {
  const char* rule = f.rule == MT_OFFSETS ? "obs_off does not start at 0 or decreases"
                     : f.rule == MT_HX ? "hx is not finite"
                     : f.rule == MT_YOBS ? "yobs is not finite"
                     : f.rule == MT_RINV ? "rinv is not finite or negative"
                                         : "infl is not finite or not positive";
  const char* what = (f.rule == MT_OFFSETS || f.rule == MT_INFL) ? "column " : "observation ";
  return "member_transform_solve: " + (what + std::to_string(f.index)) + ": " + rule;
}

struct TransformPlan {
  int fault = MT_OK;               // MT_*: the first rule the call breaks
  int index = -1;                  // the entry of `rows` / `cols` that breaks it, or
  int col = -1, member = -1;       // the base column and the member whose cell breaks the pair rule
  std::vector<int> hru;            // destination HRUs, ascending
  std::vector<int> cell;           // [hru.size()] the HRU's cell, m * ncol + j
  std::vector<int> pos;            // [hru.size()] its position in the cell, in cell_list order
  size_t size() const { return hru.size(); }
  // Workspace, by HRU, as in MixPlan: (cell, position) while a plan is made, (-1, -1) between two plans
  struct Where { int cell, pos; };
  std::vector<Where> where;
};

// cell_off / cell_list / key / cell_class as for plan_cell_mix, ncell == M * ncol; rows[nrow] of a table of table_rows rows;
// cols[n] of the ncol base columns (null: all, n must be ncol).  `p` may be the plan of an earlier call on the same domain.
static inline void plan_transform_apply(TransformPlan& p, int M, int ncol, int nhru, const int* cell_off, const int* cell_list, const int* key,
                                        int nkey, const int* cell_class, int table_rows, int nrow, const int* rows, int n, const int* cols) {
  p.fault = MT_OK; p.index = p.col = p.member = -1;
  p.hru.clear(); p.cell.clear(); p.pos.clear();
  const ParamFault rf = check_param_update(table_rows, ncol, nrow, rows, n, cols);
  if (rf.rule != PARAM_OK) {
    p.fault = rf.rule == PARAM_ROW_RANGE ? MT_ROW_RANGE : rf.rule == PARAM_ROW_REPEATS ? MT_ROW_REPEATS
              : rf.rule == PARAM_COL_RANGE ? MT_COL_RANGE : rf.rule == PARAM_COL_REPEATS ? MT_COL_REPEATS : MT_DENSE_COUNT;
    p.index = rf.index;
    return;
  }
  size_t nh = 0;
  for (int i = 0; i < n; i++) {
    const int j = cols ? cols[i] : i;
    for (int m = 1; m < M; m++) {
      const int d = m * ncol + j;
      if (cell_class[d] != cell_class[j]) {
        p.fault = copy_pair_fault(nhru, cell_off, cell_list, key, nkey, d, j) == COPY_HRU_COUNT ? MT_HRU_COUNT : MT_HRU_STRUCTURE;
        p.col = j; p.member = m;
        return;
      }
    }
    nh += (size_t)M * (size_t)(cell_off[j + 1] - cell_off[j]);
  }
  std::vector<TransformPlan::Where>& where = p.where;
  if (where.size() != (size_t)(nhru > 0 ? nhru : 0)) where.assign(nhru > 0 ? nhru : 0, TransformPlan::Where{-1, -1});
  for (int i = 0; i < n; i++) {
    const int j = cols ? cols[i] : i;
    for (int m = 0; m < M; m++) {
      const int d = m * ncol + j;
      for (int k = 0, nk = cell_off[d + 1] - cell_off[d]; k < nk; k++) where[cell_list[cell_off[d] + k]] = TransformPlan::Where{d, k};
    }
  }
  p.hru.resize(nh); p.cell.resize(nh); p.pos.resize(nh);
  size_t k = 0;
  for (int h = 0; h < nhru; h++)
    if (where[h].cell >= 0) {
      p.hru[k] = h; p.cell[k] = where[h].cell; p.pos[k] = where[h].pos; k++;
      where[h] = TransformPlan::Where{-1, -1};
    }
}

static inline std::string transform_fault_text(const TransformPlan& p) {
  const std::string name = "member_transform_apply: ";
  if (p.col >= 0)
    return name + "column " + std::to_string(p.col) + ", member " + std::to_string(p.member) + ": " +
           copy_pair_fault_text(p.fault == MT_HRU_COUNT ? COPY_HRU_COUNT : COPY_HRU_STRUCTURE);
  const int rule = p.fault == MT_ROW_RANGE ? PARAM_ROW_RANGE : p.fault == MT_ROW_REPEATS ? PARAM_ROW_REPEATS
                   : p.fault == MT_COL_RANGE ? PARAM_COL_RANGE : p.fault == MT_COL_REPEATS ? PARAM_COL_REPEATS : PARAM_DENSE_COUNT;
  return name + (p.index >= 0 ? "entry " + std::to_string(p.index) + ": " : "") + param_fault_text(rule);
}

// ------------------------------------------------------------------------------------------------ the solve kernel
struct MTSolveArgs {
  int nmember, ncol;
  int max_sweeps;                  // the sweep cap (VICGPU_TRANSFORM_SWEEPS)
  const int* obs_off;              // [ncol + 1]
  const double* hx;                // [nobs][nmember]
  const double* yobs;              // [nobs]
  const double* rinv;              // [nobs]
  const double* infl;              // [ncol] rho, or null: 1
  const double* sqrt_infl;         // [ncol] sqrt(rho) as the host rounds it, or null: 1
  double* T;                       // [ncol][nmember][nmember]
  int* info;                       // [ncol]
};

template <int MB>
__global__ __launch_bounds__(64) void vic_member_transform_solve(const MTSolveArgs a) {
  constexpr int LD = MB + 1;
  __shared__ double A[MB * LD], U[MB * LD];
  __shared__ double vg[MB], vlam[MB], vz[MB], vrs[MB], vw[MB], vcorr[MB], vh[MB], vy[MB], vry[MB];
  __shared__ double rc[MB / 2], rs[MB / 2];
  __shared__ int rp[MB / 2], rq[MB / 2];
  const int lane = threadIdx.x, j = blockIdx.x, M = a.nmember, MM = M * M;
  const int o0 = a.obs_off[j], o1 = a.obs_off[j + 1];
  const double rho = a.infl ? a.infl[j] : 1.0;
  double* __restrict__ Tj = a.T + (size_t)j * MM;

  // ---- no information: no observation, or every rinv == 0 (the same words for every lane)
  bool informed = false;
  for (int p = o0; p < o1; p++) informed = informed || a.rinv[p] != 0.0;
  if (!informed) {
    const double s = a.sqrt_infl ? a.sqrt_infl[j] : 1.0;
    const double c = (1.0 - s) / (double)M;
    for (int e = lane; e < MM; e += 64) Tj[e] = (e / M == e % M) ? s + c : c;
    if (lane == 0) a.info[j] = 0;
    return;
  }

  // ---- A = C + ((M - 1) / rho) I and g, observation by observation
  for (int e = lane; e < MM; e += 64) {
    const int r = e / M, c = e - r * M;
    A[r * LD + c] = 0.0;
    U[r * LD + c] = r == c ? 1.0 : 0.0;
  }
  double g = 0.0;
  for (int p = o0; p < o1; p++) {
    if (lane < M) vh[lane] = a.hx[(size_t)p * M + lane];
    __syncthreads();
    double sum = vh[0];
    for (int m = 1; m < M; m++) sum = sum + vh[m];
    const double ybar = sum / (double)M, r = a.rinv[p], d = a.yobs[p] - ybar;
    if (lane < M) {
      const double y = vh[lane] - ybar, ry = r * y;
      vy[lane] = y; vry[lane] = ry;
      g = g + ry * d;
    }
    __syncthreads();
    for (int e = lane; e < MM; e += 64) {
      const int r_ = e / M, c_ = e - r_ * M;
      if (r_ <= c_) A[r_ * LD + c_] = A[r_ * LD + c_] + vry[r_] * vy[c_];
    }
  }
  if (lane < M) vg[lane] = g;
  __syncthreads();
  const double shift = (double)(M - 1) / rho;
  for (int e = lane; e < MM; e += 64) {
    const int r = e / M, c = e - r * M;
    if (r > c) A[r * LD + c] = A[c * LD + r];
    else if (r == c) A[r * LD + c] = A[r * LD + c] + shift;
  }
  __syncthreads();

  // ---- parallel cyclic Jacobi: ne players (M, or M + 1 with an idle one), ne / 2 pairs a step, ne - 1 steps a sweep
  const int ne = (M + 1) & ~1, npair = ne / 2;
  int sweeps = 0;
  bool converged = false;
  for (int sw = 0; sw < a.max_sweeps && !converged; sw++) {
    bool rotated = false;
    for (int st = 0; st < ne - 1; st++) {
      bool rot = false;
      if (lane < npair) {
        int p = lane == 0 ? ne - 1 : (st + lane) % (ne - 1);
        int q = lane == 0 ? st : (st - lane + ne - 1) % (ne - 1);
        if (p > q) { const int t = p; p = q; q = t; }
        double c = 1.0, s = 0.0;
        if (q < M) {
          const double app = A[p * LD + p], aqq = A[q * LD + q], apq = A[p * LD + q];
          if (fabs(apq) > DBL_EPSILON * sqrt(app * aqq)) {
            rot = true;
            const double tau = (aqq - app) / (2.0 * apq);
            const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
            c = 1.0 / sqrt(1.0 + t * t);
            s = t * c;
          }
        }
        rp[lane] = p; rq[lane] = q; rc[lane] = c; rs[lane] = s;
      }
      const bool any = __ballot(rot) != 0;
      __syncthreads();
      if (!any) continue;            // the same for every lane
      rotated = true;
      // the columns p and q of A and U: consecutive lanes take the pairs of one row
      for (int it = lane; it < M * npair; it += 64) {
        const int i = it / npair, k = it - i * npair;
        const double s = rs[k];
        if (s != 0.0) {
          const double c = rc[k];
          const int p = rp[k], q = rq[k];
          const double x = A[i * LD + p], y = A[i * LD + q];
          A[i * LD + p] = c * x - s * y;
          A[i * LD + q] = s * x + c * y;
          const double u = U[i * LD + p], v = U[i * LD + q];
          U[i * LD + p] = c * u - s * v;
          U[i * LD + q] = s * u + c * v;
        }
      }
      __syncthreads();
      // the rows p and q of A: consecutive lanes take consecutive columns of one pair
      for (int it = lane; it < M * npair; it += 64) {
        const int k = it / M, i = it - k * M;
        const double s = rs[k];
        if (s != 0.0) {
          const double c = rc[k];
          const int p = rp[k], q = rq[k];
          const double x = A[p * LD + i], y = A[q * LD + i];
          A[p * LD + i] = c * x - s * y;
          A[q * LD + i] = s * x + c * y;
        }
      }
      __syncthreads();
      if (rot) { A[rp[lane] * LD + rq[lane]] = 0.0; A[rq[lane] * LD + rp[lane]] = 0.0; }      // what the rotation annihilates
      __syncthreads();
    }
    if (rotated) sweeps++; else converged = true;
  }
  if (!converged) {                  // the same for every lane: the identity, and the caller is told
    for (int e = lane; e < MM; e += 64) Tj[e] = (e / M == e % M) ? 1.0 : 0.0;
    if (lane == 0) a.info[j] = -1;
    return;
  }

  // ---- wbar = U diag(1 / lam) U^T g; V = U diag(sqrt(s)), s = sqrt((M - 1) / lam)
  if (lane < M) {
    const double lam = A[lane * LD + lane];
    vlam[lane] = lam;
    vrs[lane] = sqrt(sqrt((double)(M - 1) / lam));
    double z = U[lane] * vg[0];
    for (int r = 1; r < M; r++) z = z + U[r * LD + lane] * vg[r];
    vz[lane] = z / lam;
  }
  __syncthreads();
  if (lane < M) {
    double w = U[lane * LD] * vz[0];
    for (int i = 1; i < M; i++) w = w + U[lane * LD + i] * vz[i];
    vw[lane] = w;
  }
  for (int e = lane; e < MM; e += 64) {
    const int r = e / M, i = e - r * M;
    A[r * LD + i] = U[r * LD + i] * vrs[i];
  }
  __syncthreads();
  // ---- W = V V^T + wbar, into U
  for (int e = lane; e < MM; e += 64) {
    const int r = e / M, c = e - r * M;
    double w = A[r * LD] * A[c * LD];
    for (int i = 1; i < M; i++) w = w + A[r * LD + i] * A[c * LD + i];
    U[r * LD + c] = w + vw[r];
  }
  __syncthreads();
  // ---- T = W + (1 - column sum) / M, the sum with its rounding errors carried along (two-sum)
  if (lane < M) {
    double s = U[lane], comp = 0.0;
    for (int r = 1; r < M; r++) {
      const double x = U[r * LD + lane], t = s + x, bp = t - s;
      comp = comp + ((s - (t - bp)) + (x - bp));
      s = t;
    }
    vcorr[lane] = ((1.0 - s) - comp) / (double)M;
  }
  __syncthreads();
  for (int e = lane; e < MM; e += 64) {
    const int r = e / M, c = e - r * M;
    Tj[e] = U[r * LD + c] + vcorr[c];
  }
  if (lane == 0) a.info[j] = sweeps;
}

// T[ncol][M][M] and info[ncol] from the observation lists, all in device memory; M in [2, MT_MAX_MEMBERS]
static inline hipError_t transform_solve(hipStream_t st, const MTSolveArgs& a) {
  if (a.ncol <= 0) return hipSuccess;
  const dim3 grid((unsigned)a.ncol), block(64);
  if (a.nmember <= 8) hipLaunchKernelGGL(vic_member_transform_solve<8>, grid, block, 0, st, a);
  else if (a.nmember <= 16) hipLaunchKernelGGL(vic_member_transform_solve<16>, grid, block, 0, st, a);
  else if (a.nmember <= 32) hipLaunchKernelGGL(vic_member_transform_solve<32>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(vic_member_transform_solve<64>, grid, block, 0, st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ the apply kernel
struct MTApplyArgs {
  int n, nrow;                     // destination HRUs; rows of this pass, counted from the entry `rows` and the row `stage` point to
  int nmember, ncol;
  size_t ld;                       // columns per row of the table
  const int* rows;                 // [nrow] table rows
  const int* cell;                 // [n] the cell m * ncol + j of the lane's HRU
  const int* pos;                  // [n] its position in the cell
  const double* T;                 // [ncol][nmember][nmember]
  const int* cell_off;             // [ncell + 1] the domain's CSR
  const int* cell_list;            // [nhru]
  const double* table;             // [..][ld]
  double* stage;                   // [nrow][n]
};

__global__ __launch_bounds__(64) void vic_member_transform_apply(const MTApplyArgs a) {
  const int lane = blockIdx.x * 64 + threadIdx.x;
  if (lane >= a.n) return;
  const int r0 = blockIdx.y * ROW_TILE;
  const int M = a.nmember, d = a.cell[lane], k = a.pos[lane];
  const int m = d / a.ncol, j = d - m * a.ncol;
  const double* __restrict__ wt = a.T + ((size_t)j * M) * M + m;     // T[j][m'][m] = wt[m' * M]
  const int* __restrict__ off = a.cell_off + j;                      // cell m' * ncol + j
  const double* __restrict__ row[ROW_TILE];
#pragma unroll
  for (int r = 0; r < ROW_TILE; r++) row[r] = a.table + (size_t)a.rows[r0 + r < a.nrow ? r0 + r : r0] * a.ld;
  int t = 0;
  size_t col = (size_t)a.cell_list[off[0] + k];
  double w = wt[0];
  double acc[ROW_TILE], x[ROW_TILE];
#pragma unroll
  for (int r = 0; r < ROW_TILE; r++)
    if (r0 + r < a.nrow) x[r] = row[r][col];
  for (bool first = true;; first = false) {
    // the next member's column, weight and loads are issued before the adds of this one
    const bool more = ++t < M;
    double wn = 0.0, xn[ROW_TILE];
    if (more) {
      col = (size_t)a.cell_list[off[(size_t)t * a.ncol] + k];
      wn = wt[(size_t)t * M];
#pragma unroll
      for (int r = 0; r < ROW_TILE; r++)
        if (r0 + r < a.nrow) xn[r] = row[r][col];
    }
#pragma unroll
    for (int r = 0; r < ROW_TILE; r++) acc[r] = first ? w * x[r] : acc[r] + w * x[r];       // the first term is assigned, not added to zero
    if (!more) break;
    w = wn;
#pragma unroll
    for (int r = 0; r < ROW_TILE; r++) x[r] = xn[r];
  }
  double* __restrict__ out = a.stage + (size_t)r0 * a.n + lane;
#pragma unroll
  for (int r = 0; r < ROW_TILE; r++)
    if (r0 + r < a.nrow) out[(size_t)r * a.n] = acc[r];
}

// ------------------------------------------------------------------------------------------------ launchers (host)
// The lists of an apply in device memory: rows[nrow], and per destination HRU hru / cell / pos [n]
struct TransformLists {
  const int *rows, *hru, *cell, *pos;
  const int *cell_off, *cell_list;
};

// every listed row, per_pass rows at a time through stage[per_pass][n], as mix_cells_staged: the transform of a pass, then its
// scatter into table[rows[k]][hru]
static inline hipError_t transform_apply_staged(hipStream_t st, double* table, size_t ld, const TransformLists& l, int M, int ncol, const double* T,
                                                int nrow, int n, double* stage, int per_pass) {
  return for_row_passes(nrow, per_pass, [&](int r0, int nr) -> hipError_t {
    if (n <= 0 || nr <= 0) return hipSuccess;
    MTApplyArgs a;
    a.n = n; a.nrow = nr; a.nmember = M; a.ncol = ncol; a.ld = ld; a.rows = l.rows + r0; a.cell = l.cell; a.pos = l.pos; a.T = T;
    a.cell_off = l.cell_off; a.cell_list = l.cell_list; a.table = table; a.stage = stage;
    hipLaunchKernelGGL(vic_member_transform_apply, rows_grid(n, nr), dim3(64), 0, st, a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? rows_scatter<double>(st, table, ld, l.rows + r0, nr, l.hru, n, stage) : e;
  });
}

}  // namespace vic
