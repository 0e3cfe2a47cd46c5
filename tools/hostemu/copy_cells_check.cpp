// copy_cells_check.cpp — vic_amd/csrc/vic_copy_cells.hpp as a stand-alone program under ASan + UBSan: the planner and the
// direct and staged kernels on tables [nrow][nhru] of double and int built here, with exact-size allocations (the stand-in
// hip/hip_runtime.h of this directory mallocs "device" memory), so a stray column or row is a sanitizer report.  Five patterns
// over a ragged member-major domain -- fan-out, rotation, resample, swap, rotation with one row per pass -- against a plain
// loop, plus what the planner must refuse.  Built and run by tests/test_copy_cells.py; exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "vic_copy_cells.hpp"

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

// M members of NB base cells; base cell c has 2 + c % 3 HRUs whose key rows depend on the base cell and the position only.
// HRU ids are slot-major over all cells, as vic_amd/domain.py numbers them, so a cell's HRUs are far apart.
struct Dom {
  int ncell = 0, nhru = 0;
  std::vector<int> off, list, key;       // key [2][nhru]
};
static Dom make_dom(int M, int NB) {
  Dom d;
  d.ncell = M * NB;
  std::vector<std::vector<int>> of_cell(d.ncell);
  int id = 0;
  for (int slot = 0; slot < 4; slot++)
    for (int c = 0; c < d.ncell; c++)
      if (slot < 2 + (c % NB) % 3) of_cell[c].push_back(id++);
  d.nhru = id;
  d.off.push_back(0);
  d.key.assign(2 * (size_t)d.nhru, 0);
  for (int c = 0; c < d.ncell; c++) {
    for (size_t j = 0; j < of_cell[c].size(); j++) {
      d.list.push_back(of_cell[c][j]);
      d.key[of_cell[c][j]] = (int)j;
      d.key[d.nhru + of_cell[c][j]] = ((c % NB) / 3 + (int)j) % 3;
    }
    d.off.push_back((int)d.list.size());
  }
  return d;
}

template <typename T>
static T* to_device(const std::vector<T>& h) {
  T* p = nullptr;
  CHECK(hipMalloc(&p, sizeof(T) * h.size()) == hipSuccess);
  if (!h.empty()) CHECK(hipMemcpy(p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice) == hipSuccess);
  return p;
}

// the table after the copy, by a plain loop over the cell pairs (every source read from the table as it was)
template <typename T>
static std::vector<T> expected(const Dom& d, const std::vector<T>& t, int nrow, const std::vector<int>& dst, const std::vector<int>& src) {
  std::vector<T> out = t;
  for (size_t i = 0; i < dst.size(); i++)
    for (int j = 0; j < d.off[dst[i] + 1] - d.off[dst[i]]; j++)
      for (int r = 0; r < nrow; r++) out[(size_t)r * d.nhru + d.list[d.off[dst[i]] + j]] = t[(size_t)r * d.nhru + d.list[d.off[src[i]] + j]];
  return out;
}

// budget < 0: the direct path (the plan must allow it); else the staged path with that many bytes of stage
template <typename T>
static void run_table(const Dom& d, const CopyPlan& p, int nrow, const std::vector<int>& dst, const std::vector<int>& src, long budget, int* passes) {
  std::vector<T> t((size_t)nrow * d.nhru);
  for (size_t i = 0; i < t.size(); i++) t[i] = (T)(1000 * (i / d.nhru) + i % d.nhru) + (T)0.5;
  const std::vector<T> want = expected(d, t, nrow, dst, src);
  T* table = to_device(t);
  int* d_dst = to_device(p.hru.dst);
  int* d_src = to_device(p.hru.src);
  const int np = (int)p.hru.size();
  if (budget < 0) {
    CHECK(p.direct);
    CHECK(copy_direct<T>(stream, table, d.nhru, nrow, d_dst, d_src, np) == hipSuccess);
  } else {
    const int rpp = rows_per_pass((size_t)budget, np, sizeof(T), nrow);
    CHECK(rpp >= 1 && rpp <= nrow && (rpp == 1 || (size_t)rpp * np * sizeof(T) <= (size_t)budget));
    if (passes) *passes = (nrow + rpp - 1) / rpp;
    T* stage = nullptr;
    CHECK(hipMalloc(&stage, sizeof(T) * rpp * (np ? np : 1)) == hipSuccess);     // exactly what a pass may use
    CHECK(copy_staged<T>(stream, table, d.nhru, nrow, d_dst, d_src, np, stage, rpp) == hipSuccess);
    CHECK(hipFree(stage) == hipSuccess);
  }
  std::vector<T> got(t.size());
  CHECK(hipMemcpy(got.data(), table, sizeof(T) * got.size(), hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(memcmp(got.data(), want.data(), sizeof(T) * got.size()) == 0);
  if (np) CHECK(memcmp(got.data(), t.data(), sizeof(T) * got.size()) != 0);
  CHECK(hipFree(table) == hipSuccess && hipFree(d_dst) == hipSuccess && hipFree(d_src) == hipSuccess);
}

static CopyPlan plan(const Dom& d, const std::vector<int>& dst, const std::vector<int>& src) {
  return plan_cell_copy(d.ncell, d.nhru, d.off.data(), d.list.data(), d.key.data(), 2, (int)dst.size(), dst.data(), src.data());
}

static void members(int NB, int to, int from, std::vector<int>& dst, std::vector<int>& src) {
  for (int j = 0; j < NB; j++) { dst.push_back(to * NB + j); src.push_back(from * NB + j); }
}

int main() {
  const int M = 4, NB = 70;                // 4 members of 70 cells and 209 HRUs: pair lists end inside a wave
  const Dom d = make_dom(M, NB);
  CHECK(d.nhru == M * 209 && d.nhru % 64 != 0);
  const int NROW_D = 19, NROW_I = 11;      // no multiple of ROW_TILE: the last row tile is ragged
  struct Pattern { const char* name; std::vector<int> dst, src; bool direct; size_t ncell_pairs; };
  std::vector<Pattern> pats(4);
  pats[0].name = "fan-out"; pats[0].direct = true;
  for (int m = 1; m < M; m++) members(NB, m, 0, pats[0].dst, pats[0].src);
  pats[0].ncell_pairs = 3 * NB;
  pats[1].name = "rotation"; pats[1].direct = false;
  for (int m = 0; m < M; m++) members(NB, (m + 1) % M, m, pats[1].dst, pats[1].src);
  pats[1].ncell_pairs = 4 * NB;
  pats[2].name = "resample"; pats[2].direct = true;       // [0, 0, 2, 2]: the two identity members drop out
  { const int a[4] = {0, 0, 2, 2}; for (int m = 0; m < M; m++) members(NB, m, a[m], pats[2].dst, pats[2].src); }
  pats[2].ncell_pairs = 2 * NB;
  pats[3].name = "swap"; pats[3].direct = false;          // base cells 2 and 11 of member 1: 4 HRUs each, equal keys
  pats[3].dst = {NB + 2, NB + 11}; pats[3].src = {NB + 11, NB + 2}; pats[3].ncell_pairs = 2;
  for (const Pattern& pt : pats) {
    const CopyPlan p = plan(d, pt.dst, pt.src);
    CHECK(p.fault == COPY_OK);
    if (p.fault != COPY_OK) { fprintf(stderr, "%s: fault %d at pair %d\n", pt.name, p.fault, p.index); continue; }
    CHECK(p.direct == pt.direct);
    CHECK(p.cell.size() == pt.ncell_pairs && p.cell.dst.size() == p.cell.src.size() && p.hru.dst.size() == p.hru.src.size());
    for (size_t i = 1; i < p.hru.size(); i++) CHECK(p.hru.dst[i - 1] < p.hru.dst[i]);          // sorted, and so no destination twice
    for (size_t i = 1; i < p.cell.size(); i++) CHECK(p.cell.dst[i - 1] < p.cell.dst[i]);
    for (size_t i = 0; i < p.hru.size(); i++) CHECK(p.hru.dst[i] != p.hru.src[i] && p.hru.dst[i] >= 0 && p.hru.dst[i] < d.nhru && p.hru.src[i] >= 0 && p.hru.src[i] < d.nhru);
    if (pt.direct) {
      run_table<double>(d, p, NROW_D, pt.dst, pt.src, -1, nullptr);
      run_table<int>(d, p, NROW_I, pt.dst, pt.src, -1, nullptr);
    }
    // the staged path is legal for every plan and gives the same table
    int passes = 0;
    run_table<double>(d, p, NROW_D, pt.dst, pt.src, 1 << 20, &passes);
    CHECK(passes == 1);
    run_table<int>(d, p, NROW_I, pt.dst, pt.src, 1 << 20, nullptr);
    run_table<double>(d, p, NROW_D, pt.dst, pt.src, 0, &passes);                               // one row per pass
    CHECK(passes == NROW_D);
    run_table<int>(d, p, NROW_I, pt.dst, pt.src, 0, &passes);
    CHECK(passes == NROW_I);
    run_table<double>(d, p, NROW_D, pt.dst, pt.src, (long)(5 * p.hru.size() * sizeof(double) + 3), &passes);      // 5 rows fit: 4 passes, the last ragged
    CHECK(passes == 4);
    printf("%s: %zu cell pairs, %zu HRU pairs, %s\n", pt.name, p.cell.size(), p.hru.size(), p.direct ? "direct" : "staged");
  }
  // what the planner refuses, and what it reports
  CHECK(plan(d, {0, d.ncell}, {1, 0}).fault == COPY_CELL_RANGE && plan(d, {0, d.ncell}, {1, 0}).index == 1);
  CHECK(plan(d, {0}, {-1}).fault == COPY_CELL_RANGE);
  CHECK(plan(d, {5, 9, 5}, {NB + 5, NB + 9, 2 * NB + 5}).fault == COPY_DST_REPEATS && plan(d, {5, 9, 5}, {NB + 5, NB + 9, 2 * NB + 5}).index == 2);
  CHECK(plan(d, {5, 5}, {5, NB + 5}).fault == COPY_DST_REPEATS);                               // an identity pair is a destination too
  CHECK(plan(d, {0}, {1}).fault == COPY_HRU_COUNT);                                            // 2 and 3 HRUs
  CHECK(plan(d, {0}, {3}).fault == COPY_HRU_STRUCTURE);                                        // 2 HRUs each, other keys
  { const CopyPlan p = plan(d, {}, {}); CHECK(p.fault == COPY_OK && p.cell.size() == 0 && p.hru.size() == 0 && p.direct); }
  { const CopyPlan p = plan(d, {3, 4}, {3, 4}); CHECK(p.fault == COPY_OK && p.cell.size() == 0 && p.hru.size() == 0); }
  { const CopyPlan p = plan(d, {NB, 2 * NB}, {0, 0}); CHECK(p.fault == COPY_OK && p.direct && p.cell.size() == 2 && p.hru.size() == 4); }      // a source repeats
  if (failed) { fprintf(stderr, "%d checks failed\n", failed); return 1; }
  printf("copy_cells_check: all checks held\n");
  return 0;
}
