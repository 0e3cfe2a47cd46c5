// update_params_check.cpp — vic_amd/csrc/vic_params.hpp as a stand-alone program under ASan + UBSan: the check of a call and
// the scatter kernel through its staged launcher (both of vic_rows.hpp), the owner cells of listed HRUs and the listed-cell
// derive kernels, on tables built here with exact-size allocations (the stand-in hip/hip_runtime.h mallocs "device" memory), so a
// stray column or row is a sanitizer report.  Ragged lists (no multiple of a wave), the dense form, one-row passes and ragged
// last passes against a plain loop, plus what the check must refuse.  Built and run by tests/test_update_params.py; exit
// status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "vic_params.hpp"

using namespace vic;

static int failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      failed++;                                                            \
      fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond);            \
    }                                                                      \
  } while (0)

static hipStream_t stream = nullptr;     // the stand-in's streams are tokens

template <typename T>
static T* to_device(const std::vector<T>& h) {
  T* p = nullptr;
  CHECK(hipMalloc(&p, sizeof(T) * (h.empty() ? 1 : h.size())) == hipSuccess);
  if (!h.empty()) CHECK(hipMemcpy(p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice) == hipSuccess);
  return p;
}

// table[table_rows][ld]: the listed rows and columns (cols empty: dense, all ld columns) take values, through a stage of
// `budget` bytes; against a plain loop.  Returns the number of passes.
static int run_scatter(int table_rows, int ld, const std::vector<int>& rows, const std::vector<int>& cols, size_t budget) {
  const int nrow = (int)rows.size(), n = cols.empty() ? ld : (int)cols.size();
  std::vector<double> t((size_t)table_rows * ld), v((size_t)nrow * n);
  for (size_t i = 0; i < t.size(); i++) t[i] = 1000.0 * (double)(i / ld) + (double)(i % ld) + 0.5;
  for (size_t i = 0; i < v.size(); i++) v[i] = -1.0 - (double)i;
  std::vector<double> want = t;
  for (int k = 0; k < nrow; k++)
    for (int i = 0; i < n; i++) want[(size_t)rows[k] * ld + (cols.empty() ? i : cols[i])] = v[(size_t)k * n + i];
  CHECK(check_param_update(table_rows, ld, nrow, rows.data(), n, cols.empty() ? nullptr : cols.data()).rule == PARAM_OK);
  double* table = to_device(t);
  int* d_rows = to_device(rows);
  int* d_cols = cols.empty() ? nullptr : to_device(cols);
  const int rpp = rows_per_pass(budget, (size_t)n, sizeof(double), nrow);
  CHECK(rpp >= 1 && rpp <= nrow && (rpp == 1 || (size_t)rpp * n * sizeof(double) <= budget));
  double* stage = nullptr;
  CHECK(hipMalloc(&stage, sizeof(double) * rpp * n) == hipSuccess);              // exactly what a pass may use
  CHECK(rows_put_staged<double>(stream, table, ld, d_rows, nrow, d_cols, n, v.data(), stage, rpp) == hipSuccess);
  std::vector<double> got(t.size());
  CHECK(hipMemcpy(got.data(), table, sizeof(double) * got.size(), hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(memcmp(got.data(), want.data(), sizeof(double) * got.size()) == 0);
  CHECK(memcmp(got.data(), t.data(), sizeof(double) * got.size()) != 0);
  CHECK(hipFree(stage) == hipSuccess && hipFree(table) == hipSuccess && hipFree(d_rows) == hipSuccess);
  if (d_cols) CHECK(hipFree(d_cols) == hipSuccess);
  return (nrow + rpp - 1) / rpp;
}

static ParamFault chk(int table_rows, int ncol, const std::vector<int>& rows, const std::vector<int>& cols) {
  return check_param_update(table_rows, ncol, (int)rows.size(), rows.data(), (int)cols.size(), cols.data());
}

int main() {
  // ---- the scatter: 19 rows of a 23-row table (no multiple of ROW_TILE, out of order), 209 of 280 columns (ends inside a wave)
  const int TR = 23, LD = 280;
  std::vector<int> rows, cols;
  for (int k = 0; k < 19; k++) rows.push_back((k * 7 + 3) % TR);
  for (int i = 0; i < 209; i++) cols.push_back((i * 3 + 1) % LD);
  CHECK(run_scatter(TR, LD, rows, cols, 1 << 20) == 1);
  CHECK(run_scatter(TR, LD, rows, cols, 0) == 19);                                        // one row per pass
  CHECK(run_scatter(TR, LD, rows, cols, 5 * cols.size() * sizeof(double) + 3) == 4);      // 5 rows fit: 4 passes, the last ragged
  CHECK(run_scatter(TR, LD, rows, {}, 1 << 20) == 1);                                     // dense
  CHECK(run_scatter(TR, LD, rows, {}, 0) == 19);
  CHECK(run_scatter(TR, LD, {22}, {279}, 0) == 1);                                        // the table's last word
  CHECK(run_scatter(TR, LD, {0}, {0}, 1 << 20) == 1);
  printf("scatter: listed, dense, one-row passes, ragged passes\n");
  // ---- what the check refuses, and what it reports
  CHECK(chk(TR, LD, {0, TR}, {1}).rule == PARAM_ROW_RANGE && chk(TR, LD, {0, TR}, {1}).index == 1);
  CHECK(chk(TR, LD, {-1}, {1}).rule == PARAM_ROW_RANGE);
  CHECK(chk(TR, LD, {2, 1, 2}, {1}).rule == PARAM_ROW_REPEATS && chk(TR, LD, {2, 1, 2}, {1}).index == 2);
  CHECK(chk(TR, LD, {1}, {0, LD}).rule == PARAM_COL_RANGE && chk(TR, LD, {1}, {0, LD}).index == 1);
  CHECK(chk(TR, LD, {1}, {-1}).rule == PARAM_COL_RANGE);
  CHECK(chk(TR, LD, {1}, {5, 70, 5}).rule == PARAM_COL_REPEATS && chk(TR, LD, {1}, {5, 70, 5}).index == 2);
  CHECK(chk(TR, LD, {1, 1}, {5, 5}).rule == PARAM_ROW_REPEATS);                           // rows first
  { const int r[1] = {1}; CHECK(check_param_update(TR, LD, 1, r, LD - 1, nullptr).rule == PARAM_DENSE_COUNT); }
  { const int r[1] = {1}; CHECK(check_param_update(TR, LD, 1, r, LD + 1, nullptr).rule == PARAM_DENSE_COUNT); }
  { const int r[1] = {1}; CHECK(check_param_update(TR, LD, 1, r, LD, nullptr).rule == PARAM_OK); }
  { const int none = 0; CHECK(check_param_update(TR, LD, 0, &none, 0, &none).rule == PARAM_OK); }     // empty lists
  printf("check: range, repeats, dense count\n");
  // ---- owner cells: 70 cells, cell c has 2 + c % 3 HRUs, ids slot-major (a cell's HRUs are far apart)
  const int NC = 70;
  std::vector<std::vector<int>> of_cell(NC);
  int nhru = 0;
  for (int slot = 0; slot < 4; slot++)
    for (int c = 0; c < NC; c++)
      if (slot < 2 + c % 3) of_cell[c].push_back(nhru++);
  std::vector<int> off(1, 0), list;
  for (int c = 0; c < NC; c++) { list.insert(list.end(), of_cell[c].begin(), of_cell[c].end()); off.push_back((int)list.size()); }
  {
    const std::vector<int> hrus = {of_cell[69][1], of_cell[3][0], of_cell[3][1], of_cell[0][0], of_cell[41][2]};
    const std::vector<int> own = param_owner_cells(NC, nhru, off.data(), list.data(), (int)hrus.size(), hrus.data());
    CHECK((own == std::vector<int>{0, 3, 41, 69}));
    CHECK(param_owner_cells(NC, nhru, off.data(), list.data(), 0, nullptr).empty());
    CHECK((int)param_owner_cells(NC, nhru, off.data(), list.data(), nhru, list.data()).size() == NC);
  }
  printf("owner cells: ascending, each once\n");
  // ---- the listed-cell derive kernels on a 70-cell table [VIC_CPX_NROW][70]: the listed cells get the rows the full-domain
  // kernels give every cell, the others keep theirs
  {
    const int Nn = 3, Nb = 2, ncp = VIC_CPX_NROW(Nn, Nb);
    std::vector<double> cp((size_t)ncp * NC, 0.0);
    for (int c = 0; c < NC; c++)
      for (int l = 0; l < VIC_NLAYER; l++) {
        cp[(size_t)VICGPU_CP_LAYER(CPL_SOIL_DENS_MIN, l) * NC + c] = 2650.0; cp[(size_t)VICGPU_CP_LAYER(CPL_SOIL_DENSITY, l) * NC + c] = 2650.0 - c;
        cp[(size_t)VICGPU_CP_LAYER(CPL_BULK_DENS_MIN, l) * NC + c] = 1500.0 + l; cp[(size_t)VICGPU_CP_LAYER(CPL_BULK_DENSITY, l) * NC + c] = 1450.0 + c;
        cp[(size_t)VICGPU_CP_LAYER(CPL_QUARTZ, l) * NC + c] = 0.1 + 0.01 * c; cp[(size_t)VICGPU_CP_LAYER(CPL_ORGANIC, l) * NC + c] = (c % 2) * 0.05;
      }
    for (int c = 0; c < NC; c += 3) cp[(size_t)VICGPU_CP_BAND(CPB_ABOVETREELINE, 1, Nn, Nb) * NC + c] = 1.0;
    std::vector<int> hpi((size_t)HPI_NROW * nhru, 0);
    std::vector<double> hpd((size_t)HPD_NROW * nhru, 0.0), veglib(2 * (size_t)VL_NFIELD, 0.0);
    veglib[(size_t)VL_NFIELD + VL_OVERSTORY] = 1.0;
    for (int c = 0; c < NC; c++)
      for (size_t j = 0; j < of_cell[c].size(); j++) {
        const int g = of_cell[c][j];
        hpi[(size_t)HPI_CELL * nhru + g] = c; hpi[(size_t)HPI_BAND * nhru + g] = (int)j % Nb; hpi[(size_t)HPI_VEG_INDEX * nhru + g] = (int)(j / Nb) % 2 ? 0 : 1;
        hpd[(size_t)HPD_CV * nhru + g] = 0.1 + 0.01 * (double)j;
      }
    double* d_full = to_device(cp);
    double* d_part = to_device(cp);
    int *d_off = to_device(off), *d_list = to_device(list), *d_hpi = to_device(hpi);
    double *d_hpd = to_device(hpd), *d_veg = to_device(veglib);
    hipLaunchKernelGGL(vic_derive_cell_params, dim3(1), dim3(256), 0, stream, d_full, NC, Nn, Nb);
    hipLaunchKernelGGL(vic_derive_tree_adjust, dim3(2), dim3(64), 0, stream, d_full, NC, nhru, Nn, Nb, d_off, d_list, d_hpi, d_hpd, d_veg);
    std::vector<int> some;
    for (int c = 0; c < NC; c++) if (c % 4 != 1) some.push_back(NC - 1 - c);     // 52 cells, descending
    int* d_some = to_device(some);
    CHECK(derive_cell_params_listed(stream, d_part, NC, Nn, Nb, d_some, (int)some.size()) == hipSuccess);
    CHECK(derive_tree_adjust_listed(stream, d_part, NC, nhru, Nn, Nb, d_off, d_list, d_hpi, d_hpd, d_veg, d_some, (int)some.size()) == hipSuccess);
    std::vector<double> full(cp.size()), part(cp.size());
    CHECK(hipMemcpy(full.data(), d_full, sizeof(double) * full.size(), hipMemcpyDeviceToHost) == hipSuccess);
    CHECK(hipMemcpy(part.data(), d_part, sizeof(double) * part.size(), hipMemcpyDeviceToHost) == hipSuccess);
    std::vector<char> listed(NC, 0);
    for (int c : some) listed[c] = 1;
    int changed = 0;
    for (int r = 0; r < ncp; r++)
      for (int c = 0; c < NC; c++) {
        const double want = listed[c] ? full[(size_t)r * NC + c] : cp[(size_t)r * NC + c];
        CHECK(memcmp(&want, &part[(size_t)r * NC + c], sizeof(double)) == 0);
        if (full[(size_t)r * NC + c] != cp[(size_t)r * NC + c]) changed++;
      }
    CHECK(changed >= NC * (CPX_NFIELD * VIC_NLAYER + Nb) / 2);
    bool adjusted = false;
    for (int c = 0; c < NC; c += 3) if (full[(size_t)VIC_CPX_TREE_ROW(1, Nn, Nb) * NC + c] > 1.0) adjusted = true;
    CHECK(adjusted);
    // the dense form: every cell, equal to the full-domain kernels
    CHECK(derive_cell_params_listed(stream, d_part, NC, Nn, Nb, nullptr, NC) == hipSuccess);
    CHECK(derive_tree_adjust_listed(stream, d_part, NC, nhru, Nn, Nb, d_off, d_list, d_hpi, d_hpd, d_veg, nullptr, NC) == hipSuccess);
    CHECK(hipMemcpy(part.data(), d_part, sizeof(double) * part.size(), hipMemcpyDeviceToHost) == hipSuccess);
    CHECK(memcmp(part.data(), full.data(), sizeof(double) * part.size()) == 0);
    CHECK(hipFree(d_full) == hipSuccess && hipFree(d_part) == hipSuccess && hipFree(d_off) == hipSuccess && hipFree(d_list) == hipSuccess);
    CHECK(hipFree(d_hpi) == hipSuccess && hipFree(d_hpd) == hipSuccess && hipFree(d_veg) == hipSuccess && hipFree(d_some) == hipSuccess);
  }
  printf("derive: listed cells, dense\n");
  if (failed) { fprintf(stderr, "%d checks failed\n", failed); return 1; }
  printf("update_params_check: all checks held\n");
  return 0;
}
