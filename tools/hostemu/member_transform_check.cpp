// member_transform_check.cpp — vic_amd/csrc/vic_member_transform.hpp as a stand-alone program under ASan + UBSan:
// check_transform_solve, plan_transform_apply and both kernels on small member-major ensembles built here with exact-size
// allocations (the stand-in hip/hip_runtime.h of this directory mallocs "device" memory), so a stray observation, member,
// column, row or stage word is a sanitizer report.  The apply against the contract's sequential formula, bit for bit, with
// one-row and ragged passes; the solve for 4, 7, 16 and 33 members (every bucket, odd counts with an idle player) against a
// serial cyclic Jacobi iteration written here, its guarantees, and what the checks refuse.
// Built and run by tests/test_member_transform.py; exit status 0 = every check held.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "vic_member_transform.hpp"

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

static double noise(unsigned& s) {       // a fixed sequence in (-1, 1)
  s = s * 1664525u + 1013904223u;
  return (double)(s >> 8) / (double)(1u << 23) - 1.0;
}

// M members of NC base columns, member-major: cell m * NC + j has 3 HRUs when j % 3 == 0 and 2 otherwise, HRU ids slot-major;
// key row 0 = the slot, key row 1 = 1 for the second HRU of the cells in `odd`
struct Dom {
  int M = 0, ncol = 0, ncell = 0, nhru = 0;
  std::vector<int> off, list, key, cls;
};

static Dom make_dom(int M, int NC, const std::vector<int>& odd) {
  Dom d;
  d.M = M; d.ncol = NC; d.ncell = M * NC;
  std::vector<std::vector<int>> of(d.ncell);
  for (int slot = 0; slot < 3; slot++)
    for (int c = 0; c < d.ncell; c++)
      if (slot < ((c % NC) % 3 == 0 ? 3 : 2)) of[c].push_back(d.nhru++);
  d.off.push_back(0);
  for (int c = 0; c < d.ncell; c++) { d.list.insert(d.list.end(), of[c].begin(), of[c].end()); d.off.push_back((int)d.list.size()); }
  d.key.assign((size_t)2 * d.nhru, 0);
  for (int c = 0; c < d.ncell; c++)
    for (size_t k = 0; k < of[c].size(); k++) d.key[of[c][k]] = (int)k;
  for (int c : odd) d.key[(size_t)d.nhru + of[c][1]] = 1;
  d.cls = copy_cell_classes(d.ncell, d.nhru, d.off.data(), d.list.data(), d.key.data(), 2);
  return d;
}

static TransformPlan plan(const Dom& d, int table_rows, const std::vector<int>& rows, int n, const int* cols) {
  static TransformPlan p;                              // reused from call to call, as a context reuses its own
  plan_transform_apply(p, d.M, d.ncol, d.nhru, d.off.data(), d.list.data(), d.key.data(), 2, d.cls.data(), table_rows, (int)rows.size(), rows.data(), n, cols);
  for (const TransformPlan::Where& w : p.where) CHECK(w.cell == -1 && w.pos == -1);
  return p;
}

// ---- the apply on a table of table_rows rows through a stage of `budget` bytes, against the sequential formula.  Returns the passes.
static int run_apply(const Dom& d, int table_rows, const std::vector<int>& rows, const std::vector<int>* cols, size_t budget) {
  const int M = d.M, NC = d.ncol, nrow = (int)rows.size(), n = cols ? (int)cols->size() : NC;
  unsigned seed = 7u + (unsigned)M;
  std::vector<double> T((size_t)NC * M * M), t((size_t)table_rows * d.nhru);
  for (double& w : T) w = noise(seed);
  T[1] = 0.0;
  for (size_t i = 0; i < t.size(); i++) t[i] = 0.37 * (double)(i % 97) - 11.0 + 1e-3 * (double)(i / d.nhru);
  std::vector<double> want = t;
  for (int i = 0; i < n; i++) {
    const int j = cols ? (*cols)[i] : i;
    for (int m = 0; m < M; m++)
      for (int k = 0; k < d.off[j + 1] - d.off[j]; k++)
        for (int r = 0; r < nrow; r++) {
          double p = 0;
          for (int q = 0; q < M; q++) {
            const double x = t[(size_t)rows[r] * d.nhru + d.list[d.off[q * NC + j] + k]], w = T[((size_t)j * M + q) * M + m];
            p = q == 0 ? w * x : p + w * x;
          }
          want[(size_t)rows[r] * d.nhru + d.list[d.off[m * NC + j] + k]] = p;
        }
  }
  const TransformPlan p = plan(d, table_rows, rows, n, cols ? cols->data() : nullptr);
  CHECK(p.fault == MT_OK);
  const int nh = (int)p.size();
  size_t count = 0;
  for (int i = 0; i < n; i++) { const int j = cols ? (*cols)[i] : i; count += (size_t)M * (d.off[j + 1] - d.off[j]); }
  CHECK((size_t)nh == count && p.cell.size() == count && p.pos.size() == count);
  for (int i = 0; i < nh; i++) {
    CHECK(i == 0 || p.hru[i] > p.hru[i - 1]);
    CHECK(d.list[d.off[p.cell[i]] + p.pos[i]] == p.hru[i]);
  }
  double *table = to_device(t), *d_T = to_device(T);
  int *d_rows = to_device(rows), *d_hru = to_device(p.hru), *d_cell = to_device(p.cell), *d_pos = to_device(p.pos);
  int *d_coff = to_device(d.off), *d_clist = to_device(d.list);
  const int rpp = rows_per_pass(budget, (size_t)nh, sizeof(double), nrow);
  double* stage = nullptr;
  CHECK(hipMalloc(&stage, sizeof(double) * rpp * nh) == hipSuccess);               // exactly what a pass may use
  TransformLists l;
  l.rows = d_rows; l.hru = d_hru; l.cell = d_cell; l.pos = d_pos; l.cell_off = d_coff; l.cell_list = d_clist;
  CHECK(transform_apply_staged(stream, table, (size_t)d.nhru, l, M, NC, d_T, nrow, nh, stage, rpp) == hipSuccess);
  std::vector<double> got(t.size());
  CHECK(hipMemcpy(got.data(), table, sizeof(double) * got.size(), hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(memcmp(got.data(), want.data(), sizeof(double) * got.size()) == 0);
  CHECK(memcmp(got.data(), t.data(), sizeof(double) * got.size()) != 0);
  for (void* q : {(void*)table, (void*)d_T, (void*)d_rows, (void*)d_hru, (void*)d_cell, (void*)d_pos, (void*)d_coff, (void*)d_clist, (void*)stage})
    CHECK(hipFree(q) == hipSuccess);
  return (nrow + rpp - 1) / rpp;
}

// ---- the solve
struct Obs {
  std::vector<int> off;
  std::vector<double> hx, yobs, rinv, infl;
};

// NC columns with 0, 1, 3, 40, 0, ... observations; column 2 (3 observations) has every rinv == 0 when `quiet`
static Obs make_obs(int M, int NC, bool quiet) {
  Obs o;
  unsigned seed = 99u + (unsigned)M;
  const int counts[4] = {0, 1, 3, 40};
  o.off.push_back(0);
  for (int j = 0; j < NC; j++) {
    for (int p = 0; p < counts[j % 4]; p++) {
      const double truth = 3.0 * noise(seed), spread = 0.1 + fabs(noise(seed));
      for (int m = 0; m < M; m++) o.hx.push_back(truth + spread * noise(seed));
      o.yobs.push_back(truth + 0.3 * noise(seed));
      o.rinv.push_back((quiet && j == 2) || p % 7 == 6 ? 0.0 : pow(10.0, 6.0 * noise(seed)));
    }
    o.off.push_back((int)o.yobs.size());
    o.infl.push_back(j % 2 ? 1.1 : 1.0);
  }
  return o;
}

// the header's formulas with a serial cyclic Jacobi iteration
static std::vector<double> serial_transform(int M, const Obs& o, int j) {
  std::vector<double> A((size_t)M * M, 0.0), U((size_t)M * M, 0.0), g(M, 0.0), Y(M);
  for (int p = o.off[j]; p < o.off[j + 1]; p++) {
    double s = 0;
    for (int m = 0; m < M; m++) s += o.hx[(size_t)p * M + m];
    const double ybar = s / M, d = o.yobs[p] - ybar;
    for (int m = 0; m < M; m++) Y[m] = o.hx[(size_t)p * M + m] - ybar;
    for (int a = 0; a < M; a++) {
      g[a] += o.rinv[p] * Y[a] * d;
      for (int b = 0; b < M; b++) A[(size_t)a * M + b] += o.rinv[p] * Y[a] * Y[b];
    }
  }
  for (int a = 0; a < M; a++) { A[(size_t)a * M + a] += (M - 1) / o.infl[j]; U[(size_t)a * M + a] = 1.0; }
  for (int sweep = 0; sweep < 60; sweep++) {
    bool any = false;
    for (int p = 0; p < M; p++)
      for (int q = p + 1; q < M; q++) {
        const double apq = 0.5 * (A[(size_t)p * M + q] + A[(size_t)q * M + p]), app = A[(size_t)p * M + p], aqq = A[(size_t)q * M + q];
        if (fabs(apq) <= 1e-17 * sqrt(app * aqq)) continue;
        any = true;
        const double tau = (aqq - app) / (2 * apq), t = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1 + tau * tau)), c = 1 / sqrt(1 + t * t), s = t * c;
        for (int i = 0; i < M; i++) {
          const double x = A[(size_t)i * M + p], y = A[(size_t)i * M + q], u = U[(size_t)i * M + p], v = U[(size_t)i * M + q];
          A[(size_t)i * M + p] = c * x - s * y; A[(size_t)i * M + q] = s * x + c * y;
          U[(size_t)i * M + p] = c * u - s * v; U[(size_t)i * M + q] = s * u + c * v;
        }
        for (int i = 0; i < M; i++) {
          const double x = A[(size_t)p * M + i], y = A[(size_t)q * M + i];
          A[(size_t)p * M + i] = c * x - s * y; A[(size_t)q * M + i] = s * x + c * y;
        }
      }
    if (!any) break;
  }
  std::vector<double> W((size_t)M * M, 0.0), z(M, 0.0), T((size_t)M * M);
  for (int i = 0; i < M; i++) {
    for (int a = 0; a < M; a++) z[i] += U[(size_t)a * M + i] * g[a];
    z[i] /= A[(size_t)i * M + i];
  }
  for (int a = 0; a < M; a++) {
    double wbar = 0;
    for (int i = 0; i < M; i++) wbar += U[(size_t)a * M + i] * z[i];
    for (int b = 0; b < M; b++) {
      double w = 0;
      for (int i = 0; i < M; i++) w += U[(size_t)a * M + i] * sqrt((M - 1) / A[(size_t)i * M + i]) * U[(size_t)b * M + i];
      W[(size_t)a * M + b] = w + wbar;
    }
  }
  for (int b = 0; b < M; b++) {
    double s = 0;
    for (int a = 0; a < M; a++) s += W[(size_t)a * M + b];
    for (int a = 0; a < M; a++) T[(size_t)a * M + b] = W[(size_t)a * M + b] + (1 - s) / M;
  }
  return T;
}

static void run_solve(const Obs& o, int M, int NC, int max_sweeps, std::vector<double>& T, std::vector<int>& info) {
  std::vector<double> sq;
  for (double r : o.infl) sq.push_back(sqrt(r));
  int* d_off = to_device(o.off);
  double *d_hx = to_device(o.hx), *d_y = to_device(o.yobs), *d_r = to_device(o.rinv), *d_infl = to_device(o.infl), *d_sq = to_device(sq);
  double* d_T = nullptr;
  int* d_info = nullptr;
  CHECK(hipMalloc(&d_T, sizeof(double) * NC * M * M) == hipSuccess);               // exactly the transform
  CHECK(hipMalloc(&d_info, sizeof(int) * NC) == hipSuccess);
  MTSolveArgs a;
  a.nmember = M; a.ncol = NC; a.max_sweeps = max_sweeps; a.obs_off = d_off; a.hx = d_hx; a.yobs = d_y; a.rinv = d_r; a.infl = d_infl; a.sqrt_infl = d_sq;
  a.T = d_T; a.info = d_info;
  CHECK(transform_solve(stream, a) == hipSuccess);
  T.resize((size_t)NC * M * M); info.resize(NC);
  CHECK(hipMemcpy(T.data(), d_T, sizeof(double) * T.size(), hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(hipMemcpy(info.data(), d_info, sizeof(int) * NC, hipMemcpyDeviceToHost) == hipSuccess);
  for (void* q : {(void*)d_off, (void*)d_hx, (void*)d_y, (void*)d_r, (void*)d_infl, (void*)d_sq, (void*)d_T, (void*)d_info}) CHECK(hipFree(q) == hipSuccess);
}

static void check_solve(int M) {
  const int NC = 6;                                    // 0, 1, 3, 40, 0, 1 observations
  const Obs o = make_obs(M, NC, true);
  CHECK(check_transform_solve(M, NC, o.off.data(), o.hx.data(), o.yobs.data(), o.rinv.data(), o.infl.data()).rule == MT_OK);
  std::vector<double> T, T2;
  std::vector<int> info, info2;
  run_solve(o, M, NC, 30, T, info);
  run_solve(o, M, NC, 30, T2, info2);
  CHECK(memcmp(T.data(), T2.data(), sizeof(double) * T.size()) == 0 && info == info2);
  for (int j = 0; j < NC; j++) {
    const double* Tj = T.data() + (size_t)j * M * M;
    if (j % 4 == 0 || j == 2) {                          // no information: the closed form, no sweep
      const double s = sqrt(o.infl[j]), c = (1.0 - s) / M;
      CHECK(info[j] == 0);
      for (int e = 0; e < M * M; e++) CHECK(Tj[e] == (e / M == e % M ? s + c : c));
      continue;
    }
    CHECK(info[j] > 0 && info[j] < 30);
    const std::vector<double> want = serial_transform(M, o, j);
    double dev = 0, top = 0;
    for (int e = 0; e < M * M; e++) { dev = fmax(dev, fabs(Tj[e] - want[e])); top = fmax(top, fabs(want[e])); }
    CHECK(dev <= 1e-8 * top);                          // two float64 iterations on a matrix whose entries span twelve decades
    for (int b = 0; b < M; b++) {
      double s = 0;
      for (int a = 0; a < M; a++) s += Tj[(size_t)a * M + b];
      CHECK(fabs(s - 1.0) <= 1e-13);
    }
  }
  // a cap of one sweep: the dense column gets the identity and -1, the columns without information are as before
  run_solve(o, M, NC, 1, T2, info2);
  CHECK(info2[3] == -1);
  for (int e = 0; e < M * M; e++) CHECK(T2[(size_t)3 * M * M + e] == (e / M == e % M ? 1.0 : 0.0));
  CHECK(info2[0] == 0 && memcmp(T2.data(), T.data(), sizeof(double) * M * M) == 0);
}

int main() {
  const int TR = 23;
  // ---- the apply: 4 x 25 (250 HRUs, ends inside a wave), 16 x 5 and 64 x 2
  {
    const Dom d = make_dom(4, 25, {});
    CHECK(d.nhru == 4 * (25 * 2 + 9));
    std::vector<int> rows;
    for (int k = 0; k < 19; k++) rows.push_back((k * 7 + 3) % TR);                     // 19 of 23 rows, out of order, no multiple of ROW_TILE
    const std::vector<int> some = {24, 0, 7, 13, 3, 21};
    size_t nh = 0;
    for (int j : some) nh += 4 * (size_t)(d.off[j + 1] - d.off[j]);
    CHECK(run_apply(d, TR, rows, nullptr, 1 << 20) == 1);
    CHECK(run_apply(d, TR, rows, nullptr, 0) == 19);                                   // one row per pass
    CHECK(run_apply(d, TR, rows, &some, 5 * nh * sizeof(double) + 3) == 4);            // 5 rows fit: 4 passes, the last ragged
    CHECK(run_apply(d, TR, {TR - 1}, &some, 0) == 1);                                  // the table's last row
    const Dom d16 = make_dom(16, 5, {}), d64 = make_dom(64, 2, {});
    CHECK(run_apply(d16, TR, rows, nullptr, 1 << 20) == 1);
    CHECK(run_apply(d64, TR, {0, TR - 1, 5}, nullptr, 0) == 3);
    printf("apply: 4 x 25, 16 x 5 and 64 x 2; all columns and a shuffled subset; one pass, one-row passes, ragged passes\n");
  }
  // ---- the solve: every bucket, odd member counts
  for (int M : {2, 4, 7, 16, 33, 64}) check_solve(M);
  printf("solve: 2, 4, 7, 16, 33 and 64 members; two runs; the closed form; the sweep cap\n");
  // ---- what the checks refuse, and whom they name
  {
    const Dom d = make_dom(4, 25, {2 * 25 + 3});         // member 2 of column 3 is odd
    const std::vector<int> rows = {1, 2};
    const auto fault = [&](const std::vector<int>& r, int n, const int* cols) { return plan(d, TR, r, n, cols); };
    const int ok[3] = {0, 24, 7}, range[2] = {0, 25}, neg[1] = {-1}, twice[3] = {4, 1, 4}, odd[2] = {1, 3};
    CHECK(fault(rows, 3, ok).fault == MT_OK);
    { const TransformPlan p = fault({1, TR}, 3, ok); CHECK(p.fault == MT_ROW_RANGE && p.index == 1); }
    CHECK(fault({-1}, 3, ok).fault == MT_ROW_RANGE);
    { const TransformPlan p = fault({2, 1, 2}, 3, ok); CHECK(p.fault == MT_ROW_REPEATS && p.index == 2); }
    { const TransformPlan p = fault(rows, 2, range); CHECK(p.fault == MT_COL_RANGE && p.index == 1); }
    CHECK(fault(rows, 1, neg).fault == MT_COL_RANGE);
    { const TransformPlan p = fault(rows, 3, twice); CHECK(p.fault == MT_COL_REPEATS && p.index == 2); }
    CHECK(fault(rows, 24, nullptr).fault == MT_DENSE_COUNT);
    { const TransformPlan p = fault(rows, 2, odd); CHECK(p.fault == MT_HRU_STRUCTURE && p.col == 3 && p.member == 2); }
    { const TransformPlan p = fault(rows, 25, nullptr); CHECK(p.fault == MT_HRU_STRUCTURE && p.col == 3 && p.member == 2); }
    { const std::string s = transform_fault_text(fault(rows, 2, odd)); CHECK(s.find("column 3") != std::string::npos && s.find("member 2") != std::string::npos); }
    CHECK(transform_fault_text(fault({2, 1, 2}, 3, ok)).find("listed twice") != std::string::npos);
    CHECK(fault({}, 0, ok).fault == MT_OK && fault({}, 0, ok).size() == 0);
    const double inf = std::numeric_limits<double>::infinity();
    Obs o = make_obs(4, 6, false);
    const auto rule = [&](const Obs& x) { return check_transform_solve(4, 6, x.off.data(), x.hx.data(), x.yobs.data(), x.rinv.data(), x.infl.data()); };
    CHECK(rule(o).rule == MT_OK);
    CHECK(check_transform_solve(4, 6, o.off.data(), o.hx.data(), o.yobs.data(), o.rinv.data(), nullptr).rule == MT_OK);
    { Obs x = o; x.off[0] = 1; CHECK(rule(x).rule == MT_OFFSETS); }
    { Obs x = o; x.off[3] = x.off[2] - 1; const SolveFault f = rule(x); CHECK(f.rule == MT_OFFSETS && f.index == 2); }
    { Obs x = o; x.hx[4 * 2 + 1] = std::nan(""); const SolveFault f = rule(x); CHECK(f.rule == MT_HX && f.index == 2); }
    { Obs x = o; x.hx.back() = inf; CHECK(rule(x).rule == MT_HX); }
    { Obs x = o; x.yobs[1] = -inf; const SolveFault f = rule(x); CHECK(f.rule == MT_YOBS && f.index == 1); }
    { Obs x = o; x.rinv[0] = -1e-300; CHECK(rule(x).rule == MT_RINV); }
    { Obs x = o; x.rinv.back() = inf; CHECK(rule(x).rule == MT_RINV); }
    { Obs x = o; x.infl[5] = 0.0; const SolveFault f = rule(x); CHECK(f.rule == MT_INFL && f.index == 5); }
    { Obs x = o; x.infl[0] = std::nan(""); CHECK(rule(x).rule == MT_INFL); }
    { Obs x = o; x.hx[1] = std::nan(""); CHECK(solve_fault_text(rule(x)).find("observation 0") != std::string::npos); }
    printf("checks: rows, columns, the pair rule; offsets, hx, yobs, rinv, infl\n");
  }
  if (failed) { fprintf(stderr, "%d checks failed\n", failed); return 1; }
  printf("member_transform_check: all checks held\n");
  return 0;
}
