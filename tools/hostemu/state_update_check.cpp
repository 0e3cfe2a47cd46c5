// state_update_check.cpp — vic_amd/csrc/vic_state_update.hpp as a stand-alone program under ASan + UBSan: the check of a call,
// the gather and scatter kernels of vic_rows.hpp (SET and ADD, double and int) through their staged launchers, and
// vic_derive_soil_state for the three node bounds, on tables built here with exact-size allocations (the stand-in hip/hip_runtime.h of this directory
// mallocs "device" memory), so a stray column, row or node is a sanitizer report.  Ragged lists (no multiple of a wave), the
// dense form, one-row passes and ragged last passes against a plain loop; the derive against what its stages must leave.
// Built and run by tests/test_state_update.py; exit status 0 = every check held.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "vic_aux_kernels.hpp"     // vic_derive_cell_params: the appended rows of the parameter table the derive reads
#include "vic_state_update.hpp"

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

template <typename T>
static std::vector<T> to_host(const T* p, size_t n) {
  std::vector<T> h(n);
  CHECK(hipMemcpy(h.data(), p, sizeof(T) * n, hipMemcpyDeviceToHost) == hipSuccess);
  return h;
}

// table[table_rows][ld]: the listed rows and columns (cols empty: dense) are read, set, added to and read again through a
// stage of `budget` bytes; against plain loops.  Returns the number of passes.
template <typename T>
static int run_rows(int table_rows, int ld, const std::vector<int>& rows, const std::vector<int>& cols, size_t budget, bool add) {
  const int nrow = (int)rows.size(), n = cols.empty() ? ld : (int)cols.size();
  std::vector<T> t((size_t)table_rows * ld), v((size_t)nrow * n);
  for (size_t i = 0; i < t.size(); i++) t[i] = (T)(1000 * (i / ld) + (i % ld)) + (T)0.5;
  for (size_t i = 0; i < v.size(); i++) v[i] = (T)(-1) - (T)i;
  const auto at = [&](int k, int i) { return (size_t)rows[k] * ld + (cols.empty() ? i : cols[i]); };
  std::vector<T> want = t, slice(v.size());
  for (int k = 0; k < nrow; k++)
    for (int i = 0; i < n; i++) {
      slice[(size_t)k * n + i] = t[at(k, i)];
      want[at(k, i)] = add ? (T)(t[at(k, i)] + v[(size_t)k * n + i]) : v[(size_t)k * n + i];
    }
  CHECK(check_param_update(table_rows, ld, nrow, rows.data(), n, cols.empty() ? nullptr : cols.data()).rule == PARAM_OK);
  T* table = to_device(t);
  int* d_rows = to_device(rows);
  int* d_cols = cols.empty() ? nullptr : to_device(cols);
  const int rpp = rows_per_pass(budget, (size_t)n, sizeof(T), nrow);
  CHECK(rpp >= 1 && rpp <= nrow && (rpp == 1 || (size_t)rpp * n * sizeof(T) <= budget));
  T* stage = nullptr;
  CHECK(hipMalloc(&stage, sizeof(T) * rpp * n) == hipSuccess);                   // exactly what a pass may use
  std::vector<T> got(v.size());                                                  // exactly what a get may write
  CHECK(rows_get_staged<T>(stream, table, ld, d_rows, nrow, d_cols, n, got.data(), stage, rpp) == hipSuccess);
  CHECK(memcmp(got.data(), slice.data(), sizeof(T) * got.size()) == 0);
  CHECK(rows_put_staged<T>(stream, table, ld, d_rows, nrow, d_cols, n, v.data(), stage, rpp, add) == hipSuccess);
  const std::vector<T> after = to_host(table, t.size());
  CHECK(memcmp(after.data(), want.data(), sizeof(T) * after.size()) == 0);
  CHECK(memcmp(after.data(), t.data(), sizeof(T) * after.size()) != 0);
  CHECK(rows_get_staged<T>(stream, table, ld, d_rows, nrow, d_cols, n, got.data(), stage, rpp) == hipSuccess);
  for (int k = 0; k < nrow; k++)
    for (int i = 0; i < n; i++) CHECK(memcmp(&got[(size_t)k * n + i], &want[at(k, i)], sizeof(T)) == 0);
  CHECK(hipFree(stage) == hipSuccess && hipFree(table) == hipSuccess && hipFree(d_rows) == hipSuccess);
  if (d_cols) CHECK(hipFree(d_cols) == hipSuccess);
  return (nrow + rpp - 1) / rpp;
}

// The derive kernel of node count Nn on NC cells of 3 HRUs (slot-major ids), cell `short_cell` with thermal nodes that end
// above the bottom layer, HRU `dead` without area.  The listed HRUs get what the stages must leave, the others keep their bits.
static void run_derive(int Nn, int quick_flux) {
  const int Nb = 2, NC = 70, nhru = 3 * NC, ncp = VIC_CPX_NROW(Nn, Nb), nsd = VICGPU_SD_NROW(Nn), nsi = VICGPU_SI_NROW(Nn);
  const int short_cell = 41, dead = NC + 5;
  const double depth[3] = {0.1, 0.3, 1.5};
  std::vector<double> cp((size_t)ncp * NC, 0.0);
  const auto CP = [&](int row, int c) -> double& { return cp[(size_t)row * NC + c]; };
  for (int c = 0; c < NC; c++) {
    CP(CP_FS_ACTIVE, c) = (c % 7 == 3) ? 0.0 : 1.0; CP(CP_AVG_TEMP, c) = 2.0 + 0.05 * c; CP(CP_DP, c) = 4.0;
    for (int l = 0; l < VIC_NLAYER; l++) {
      CP(VICGPU_CP_LAYER(CPL_DEPTH, l), c) = depth[l]; CP(VICGPU_CP_LAYER(CPL_MAX_MOIST, l), c) = depth[l] * 1000.0 * 0.45;
      CP(VICGPU_CP_LAYER(CPL_BUBBLE, l), c) = 20.0 + l; CP(VICGPU_CP_LAYER(CPL_EXPT, l), c) = 10.0 + 0.1 * c;
      CP(VICGPU_CP_LAYER(CPL_SOIL_DENS_MIN, l), c) = 2650.0; CP(VICGPU_CP_LAYER(CPL_SOIL_DENSITY, l), c) = 2650.0 - c;
      CP(VICGPU_CP_LAYER(CPL_BULK_DENS_MIN, l), c) = 1500.0 + l; CP(VICGPU_CP_LAYER(CPL_BULK_DENSITY, l), c) = 1450.0 + c;
      CP(VICGPU_CP_LAYER(CPL_QUARTZ, l), c) = 0.1 + 0.01 * c; CP(VICGPU_CP_LAYER(CPL_ORGANIC, l), c) = (c % 2) * 0.05;
    }
    // nodes 0, 0.1, 0.2 and then evenly down to 4 m; in the short cell down to 1.2 m only (the layers end at 1.9 m)
    const double deepest = c == short_cell ? 1.2 : 4.0;
    for (int n = 0; n < Nn; n++) {
      CP(VICGPU_CP_NODE(CPN_ZSUM, n, Nn), c) = n < 3 ? 0.1 * n : 0.2 + (deepest - 0.2) * (n - 2) / (Nn - 3);
      CP(VICGPU_CP_NODE(CPN_MAX_MOIST, n, Nn), c) = 0.45; CP(VICGPU_CP_NODE(CPN_BUBBLE, n, Nn), c) = 21.0; CP(VICGPU_CP_NODE(CPN_EXPT, n, Nn), c) = 10.5;
    }
    for (int b = 0; b < Nb; b++) CP(VICGPU_CP_BAND(CPB_AREAFRACT, b, Nn, Nb), c) = 0.5;
  }
  double* d_cp = to_device(cp);
  hipLaunchKernelGGL(vic_derive_cell_params, dim3(1), dim3(256), 0, stream, d_cp, NC, Nn, Nb);
  std::vector<int> hpi((size_t)HPI_NROW * nhru, 0), si((size_t)nsi * nhru, 7), flags(NC, 0);
  std::vector<double> hpd((size_t)HPD_NROW * nhru, 0.0), sd((size_t)nsd * nhru, 1e30), fx((size_t)FX_NROW * nhru, 1e30);
  for (int g = 0; g < nhru; g++) {
    hpi[(size_t)HPI_CELL * nhru + g] = g % NC; hpi[(size_t)HPI_BAND * nhru + g] = (g / NC) % Nb;
    hpd[(size_t)HPD_CV * nhru + g] = g == dead ? 0.0 : 0.3;
    for (int l = 0; l < 3; l++) {
      sd[(size_t)(SD_MOIST0 + l) * nhru + g] = depth[l] * 1000.0 * (0.2 + 0.3 * ((g + l) % 4) / 3.0);        // up to 0.5: above the maximum
      sd[(size_t)(SD_ICE0 + l) * nhru + g] = depth[l] * 1000.0 * 0.1;
    }
    for (int n = 0; n < Nn; n++) sd[(size_t)VICGPU_SD_NODE(SDN_T, n, Nn) * nhru + g] = -4.0 + 7.0 * ((n * 5 + g) % 9) / 8.0;       // fronts
  }
  std::vector<int> list;
  for (int g = 0; g < nhru; g++) if (g % 4 != 1) list.push_back(nhru - 1 - g);           // 157 HRUs, descending, ends inside a wave
  std::vector<char> listed(nhru, 0);
  for (int g : list) listed[g] = 1;
  CHECK(listed[dead] && listed[short_cell]);
  int *d_hpi = to_device(hpi), *d_si = to_device(si), *d_flags = to_device(flags), *d_list = to_device(list);
  double *d_hpd = to_device(hpd), *d_sd = to_device(sd), *d_fx = to_device(fx);
  DSArgs a{};
  a.o.Nnode = Nn; a.o.Nband = Nb; a.o.FROZEN_SOIL = 1; a.o.FULL_ENERGY = 1; a.o.QUICK_FLUX = quick_flux;
  a.ncell = NC; a.nhru = nhru; a.n = (int)list.size(); a.what = DERIVE_ALL; a.hrus = d_list;
  a.cp = d_cp; a.hpi = d_hpi; a.hpd = d_hpd; a.sd = d_sd; a.si = d_si; a.flux = d_fx; a.cell_err = d_flags;
  CHECK(check_derive_what(a.what, 0) == DERIVE_OK);
  CHECK(check_param_update(0, nhru, 0, nullptr, a.n, list.data()).rule == PARAM_OK);
  CHECK(derive_soil_state(stream, a) == hipSuccess);
  const std::vector<double> sd1 = to_host(d_sd, sd.size()), fx1 = to_host(d_fx, fx.size());
  const std::vector<int> si1 = to_host(d_si, si.size()), fl1 = to_host(d_flags, flags.size());
  int capped = 0, frozen = 0, fronts = 0;
  for (int g = 0; g < nhru; g++) {
    const int c = g % NC;
    const auto SD1 = [&](int row) { return sd1[(size_t)row * nhru + g]; };
    if (!listed[g]) {                                          // every word of the column as it was
      for (int r = 0; r < nsd; r++) CHECK(memcmp(&sd1[(size_t)r * nhru + g], &sd[(size_t)r * nhru + g], sizeof(double)) == 0);
      for (int r = 0; r < nsi; r++) CHECK(si1[(size_t)r * nhru + g] == 7);
      for (int r = 0; r < FX_NROW; r++) CHECK(fx1[(size_t)r * nhru + g] == 1e30);
      continue;
    }
    for (int l = 0; l < 3; l++) {                              // the cap
      const double m0 = sd[(size_t)(SD_MOIST0 + l) * nhru + g], mm = depth[l] * 1000.0 * 0.45;
      CHECK(SD1(SD_MOIST0 + l) == (m0 > mm ? mm : m0));
      if (m0 > mm) capped++;
    }
    for (int n = 0; n < Nn; n++) CHECK(SD1(VICGPU_SD_NODE(SDN_T, n, Nn)) == sd[(size_t)VICGPU_SD_NODE(SDN_T, n, Nn) * nhru + g]);
    if (g == dead) {                                           // empty node blocks, nothing else
      for (int n = 0; n < Nn; n++)
        CHECK(SD1(VICGPU_SD_NODE(SDN_MOIST, n, Nn)) == 0 && SD1(VICGPU_SD_NODE(SDN_ICE, n, Nn)) == 0 && SD1(VICGPU_SD_NODE(SDN_KAPPA, n, Nn)) == 0 &&
              SD1(VICGPU_SD_NODE(SDN_CS, n, Nn)) == 0);
      CHECK(SD1(SD_LAYER_T0) == 1e30 && si1[(size_t)SI_NFROST * nhru + g] == 7 && fx1[(size_t)FX_FDEPTH0 * nhru + g] == 1e30);
      continue;
    }
    const bool fs = c % 7 != 3;
    for (int n = 0; n < Nn; n++) {
      const double mo = SD1(VICGPU_SD_NODE(SDN_MOIST, n, Nn)), ic = SD1(VICGPU_SD_NODE(SDN_ICE, n, Nn));
      CHECK(mo > 0 && mo <= 0.45 && ic >= 0 && ic <= mo && SD1(VICGPU_SD_NODE(SDN_KAPPA, n, Nn)) > 0 && SD1(VICGPU_SD_NODE(SDN_KAPPA, n, Nn)) < 10 &&
            SD1(VICGPU_SD_NODE(SDN_CS, n, Nn)) > 1e5 && SD1(VICGPU_SD_NODE(SDN_CS, n, Nn)) < 1e7);
      if (!fs) CHECK(ic == 0);
      if (ic > 0) frozen++;
    }
    { const double m0 = SD1(SD_MOIST0) / depth[0] / 1000; CHECK(SD1(VICGPU_SD_NODE(SDN_MOIST, 0, Nn)) == (m0 - 0.45 > 0 ? 0.45 : m0)); }
    const bool fails = c == short_cell && !quick_flux;
    for (int l = 0; l < 3; l++) {
      const double lt = SD1(SD_LAYER_T0 + l), li = SD1(SD_ICE0 + l);
      if (fails && l == 2) CHECK(lt == 0 && li == 0);
      else CHECK(lt > -10 && lt < 10 && li >= 0 && li <= SD1(SD_MOIST0 + l));
    }
    if (quick_flux || !fs) {
      CHECK(si1[(size_t)SI_NFROST * nhru + g] == 7 && si1[(size_t)SI_NTHAW * nhru + g] == 7 && fx1[(size_t)FX_TDEPTH2 * nhru + g] == 1e30);
    } else {
      const int nf = si1[(size_t)SI_NFROST * nhru + g], nt = si1[(size_t)SI_NTHAW * nhru + g];
      CHECK(nf >= 0 && nf <= 3 && nt >= 0 && nt <= 3);
      for (int f = 0; f < 3; f++) {
        const double fd = fx1[(size_t)(FX_FDEPTH0 + f) * nhru + g], td = fx1[(size_t)(FX_TDEPTH0 + f) * nhru + g];
        CHECK(f < nf ? (fd >= 0 && fd <= 4.0) : std::isnan(fd));
        CHECK(f < nt ? (td >= 0 && td <= 4.0) : std::isnan(td));
      }
      fronts += nf + nt;
    }
    for (int r = 0; r < FX_NROW; r++)
      if (r < FX_FDEPTH0 || r > FX_TDEPTH2) CHECK(fx1[(size_t)r * nhru + g] == 1e30);
  }
  CHECK(capped > 50 && frozen > 100 && (quick_flux || fronts > 100));
  for (int c = 0; c < NC; c++) CHECK(fl1[c] == (c == short_cell && !quick_flux ? VICGPU_CELLERR_NODES : 0));
  // the dense form: every HRU
  a.hrus = nullptr; a.n = nhru; a.what = VICGPU_DERIVE_NODES | VICGPU_DERIVE_LAYERS;
  CHECK(derive_soil_state(stream, a) == hipSuccess);
  const std::vector<double> sd2 = to_host(d_sd, sd.size());
  for (int g = 0; g < nhru; g++)
    if (g != dead) CHECK(sd2[(size_t)VICGPU_SD_NODE(SDN_CS, Nn - 1, Nn) * nhru + g] > 1e5 && sd2[(size_t)VICGPU_SD_NODE(SDN_CS, Nn - 1, Nn) * nhru + g] < 1e7);
  CHECK(hipFree(d_cp) == hipSuccess && hipFree(d_hpi) == hipSuccess && hipFree(d_si) == hipSuccess && hipFree(d_flags) == hipSuccess);
  CHECK(hipFree(d_list) == hipSuccess && hipFree(d_hpd) == hipSuccess && hipFree(d_sd) == hipSuccess && hipFree(d_fx) == hipSuccess);
}

int main() {
  // ---- gather and scatter: 19 rows of a 23-row table (no multiple of ROW_TILE, out of order), 209 of 280 columns (ends inside a wave)
  const int TR = 23, LD = 280;
  std::vector<int> rows, cols;
  for (int k = 0; k < 19; k++) rows.push_back((k * 7 + 3) % TR);
  for (int i = 0; i < 209; i++) cols.push_back((i * 3 + 1) % LD);
  for (int add = 0; add < 2; add++) {
    CHECK(run_rows<double>(TR, LD, rows, cols, 1 << 20, add) == 1);
    CHECK(run_rows<double>(TR, LD, rows, cols, 0, add) == 19);                                        // one row per pass
    CHECK(run_rows<double>(TR, LD, rows, cols, 5 * cols.size() * sizeof(double) + 3, add) == 4);      // 5 rows fit: 4 passes, the last ragged
    CHECK(run_rows<double>(TR, LD, rows, {}, 1 << 20, add) == 1);                                     // dense
    CHECK(run_rows<double>(TR, LD, rows, {}, 0, add) == 19);
    CHECK(run_rows<double>(TR, LD, {22}, {279}, 0, add) == 1);                                        // the table's last word
    CHECK(run_rows<double>(TR, LD, {0}, {0}, 1 << 20, add) == 1);
  }
  CHECK(run_rows<int>(TR, LD, rows, cols, 1 << 20, false) == 1);
  CHECK(run_rows<int>(TR, LD, rows, cols, 0, false) == 19);
  CHECK(run_rows<int>(TR, LD, rows, cols, 5 * cols.size() * sizeof(int) + 3, false) == 4);
  CHECK(run_rows<int>(TR, LD, rows, {}, 0, false) == 19);
  CHECK(run_rows<int>(TR, LD, {22}, {279}, 0, false) == 1);
  printf("gather and scatter: SET and ADD, double and int, listed, dense, one-row passes, ragged passes\n");
  // ---- what the checks refuse
  CHECK(check_derive_what(0, 0) == DERIVE_WHAT && check_derive_what(16, 0) == DERIVE_WHAT && check_derive_what(-1, 0) == DERIVE_WHAT);
  CHECK(check_derive_what(VICGPU_DERIVE_NODES | 32, 0) == DERIVE_WHAT && check_derive_what(DERIVE_ALL, 0) == DERIVE_OK);
  CHECK(check_derive_what(VICGPU_DERIVE_CAP_MOIST, 1) == DERIVE_UNSUPPORTED && check_derive_what(DERIVE_ALL & ~VICGPU_DERIVE_CAP_MOIST, 1) == DERIVE_OK);
  CHECK(check_derive_what(0, 1) == DERIVE_WHAT);
  { const int h[3] = {5, 70, 5}; CHECK(check_param_update(0, LD, 0, nullptr, 3, h).rule == PARAM_COL_REPEATS); }
  { const int h[2] = {0, LD}; CHECK(check_param_update(0, LD, 0, nullptr, 2, h).rule == PARAM_COL_RANGE); }
  CHECK(check_param_update(0, LD, 0, nullptr, LD - 1, nullptr).rule == PARAM_DENSE_COUNT && check_param_update(0, LD, 0, nullptr, LD, nullptr).rule == PARAM_OK);
  printf("check: stage bits, GLACIER_DYNAMICS, HRU lists\n");
  // ---- the derive kernel: the three node bounds, and the quick-flux form
  run_derive(10, 0);
  run_derive(14, 0);
  run_derive(30, 0);
  run_derive(10, 1);
  run_derive(3, 1);
  printf("derive: 10, 14 and 30 nodes, quick flux with 10 and 3\n");
  if (failed) { fprintf(stderr, "%d checks failed\n", failed); return 1; }
  printf("state_update_check: all checks held\n");
  return 0;
}
