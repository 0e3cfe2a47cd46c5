// mix_cells_check.cpp — vic_amd/csrc/vic_mix_cells.hpp as a stand-alone program under ASan + UBSan: plan_cell_mix and
// vic_mix_cells through mix_cells_staged on a small ragged domain built here with exact-size allocations (the stand-in
// hip/hip_runtime.h of this directory mallocs "device" memory), so a stray column, row, term or stage word is a sanitizer
// report.  Cells of 2 or 3 HRUs numbered slot-major, destinations out of order with 1, 2, 3 and 65 terms, self and mutual terms,
// one-row passes and ragged last passes, against the contract's sequential formula; then what the plan refuses.
// Built and run by tests/test_mix_cells.py; exit status 0 = every check held.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "vic_mix_cells.hpp"

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

// NC cells, cell c with 3 HRUs when c % 3 == 0 and 2 otherwise, HRU ids slot-major (slot 0 of every cell, then slot 1, ...);
// key row 0 = the slot, key row 1 = 1 for the cells in `odd`
struct Dom {
  int ncell = 0, nhru = 0;
  std::vector<int> off, list, key;
};

static Dom make_dom(int NC, const std::vector<int>& odd) {
  Dom d;
  d.ncell = NC;
  std::vector<std::vector<int>> of(NC);
  for (int slot = 0; slot < 3; slot++)
    for (int c = 0; c < NC; c++)
      if (slot < (c % 3 == 0 ? 3 : 2)) of[c].push_back(d.nhru++);
  d.off.push_back(0);
  for (int c = 0; c < NC; c++) { d.list.insert(d.list.end(), of[c].begin(), of[c].end()); d.off.push_back((int)d.list.size()); }
  d.key.assign((size_t)2 * d.nhru, 0);
  for (int c = 0; c < NC; c++)
    for (size_t j = 0; j < of[c].size(); j++) d.key[of[c][j]] = (int)j;
  for (int c : odd) d.key[(size_t)d.nhru + of[c][1]] = 1;
  return d;
}

struct Call {
  std::vector<int> rows, dst, off, cell;
  std::vector<double> weight;
  void add(int d, const std::vector<int>& cells, const std::vector<double>& w) {
    if (off.empty()) off.push_back(0);
    dst.push_back(d); cell.insert(cell.end(), cells.begin(), cells.end()); weight.insert(weight.end(), w.begin(), w.end());
    off.push_back((int)cell.size());
  }
};

static MixPlan plan(const Dom& d, int table_rows, const Call& c) {
  const std::vector<int> cls = copy_cell_classes(d.ncell, d.nhru, d.off.data(), d.list.data(), d.key.data(), 2);
  for (int a = 0; a < d.ncell; a += 7)                 // a class per structure: the same verdict as the pair rule
    for (int b = 0; b < d.ncell; b++) CHECK((cls[a] == cls[b]) == (copy_pair_fault(d.nhru, d.off.data(), d.list.data(), d.key.data(), 2, a, b) == COPY_OK));
  static MixPlan p;                                    // reused from call to call, as a context reuses its own
  plan_cell_mix(p, d.ncell, d.nhru, d.off.data(), d.list.data(), d.key.data(), 2, cls.data(), table_rows, (int)c.rows.size(), c.rows.data(), (int)c.dst.size(),
                c.dst.data(), c.off.data(), c.cell.data(), c.weight.data());
  for (const MixPlan::Where& w : p.where) CHECK(w.i == -1 && w.j == -1);
  return p;
}

// the call on a table of table_rows rows through a stage of `budget` bytes, against the sequential formula.  Returns the passes.
static int run_mix(const Dom& d, int table_rows, const Call& c, size_t budget) {
  const int nrow = (int)c.rows.size(), ndst = (int)c.dst.size();
  std::vector<double> t((size_t)table_rows * d.nhru);
  for (size_t i = 0; i < t.size(); i++) t[i] = 0.37 * (double)(i % 97) - 11.0 + 1e-3 * (double)(i / d.nhru);
  t[(size_t)c.rows[0] * d.nhru + d.list[d.off[c.cell[0]]]] = -0.0;
  std::vector<double> want = t;
  for (int i = 0; i < ndst; i++)
    for (int j = 0; j < d.off[c.dst[i] + 1] - d.off[c.dst[i]]; j++)
      for (int k = 0; k < nrow; k++) {
        double p = 0;
        for (int q = c.off[i]; q < c.off[i + 1]; q++) {
          const double x = t[(size_t)c.rows[k] * d.nhru + d.list[d.off[c.cell[q]] + j]];
          p = q == c.off[i] ? c.weight[q] * x : p + c.weight[q] * x;
        }
        want[(size_t)c.rows[k] * d.nhru + d.list[d.off[c.dst[i]] + j]] = p;
      }
  const MixPlan p = plan(d, table_rows, c);
  CHECK(p.fault == MIX_OK);
  const int n = (int)p.size();
  size_t nh = 0;
  for (int i = 0; i < ndst; i++) nh += d.off[c.dst[i] + 1] - d.off[c.dst[i]];
  CHECK((size_t)n == nh && p.dst_index.size() == nh && p.pos.size() == nh);
  for (int i = 0; i < n; i++) {
    CHECK(i == 0 || p.hru[i] > p.hru[i - 1]);
    CHECK(d.list[d.off[c.dst[p.dst_index[i]]] + p.pos[i]] == p.hru[i]);
  }
  double* table = to_device(t);
  int *d_rows = to_device(c.rows), *d_hru = to_device(p.hru), *d_index = to_device(p.dst_index), *d_pos = to_device(p.pos);
  int *d_off = to_device(c.off), *d_cell = to_device(c.cell), *d_coff = to_device(d.off), *d_clist = to_device(d.list);
  double* d_weight = to_device(c.weight);
  const int rpp = rows_per_pass(budget, (size_t)n, sizeof(double), nrow);
  double* stage = nullptr;
  CHECK(hipMalloc(&stage, sizeof(double) * rpp * n) == hipSuccess);                // exactly what a pass may use
  MixLists l;
  l.rows = d_rows; l.hru = d_hru; l.dst_index = d_index; l.pos = d_pos; l.term_off = d_off; l.term_cell = d_cell; l.term_weight = d_weight;
  l.cell_off = d_coff; l.cell_list = d_clist;
  CHECK(mix_cells_staged(stream, table, (size_t)d.nhru, l, nrow, n, stage, rpp) == hipSuccess);
  std::vector<double> got(t.size());
  CHECK(hipMemcpy(got.data(), table, sizeof(double) * got.size(), hipMemcpyDeviceToHost) == hipSuccess);
  CHECK(memcmp(got.data(), want.data(), sizeof(double) * got.size()) == 0);
  CHECK(memcmp(got.data(), t.data(), sizeof(double) * got.size()) != 0);
  for (void* q : {(void*)table, (void*)d_rows, (void*)d_hru, (void*)d_index, (void*)d_pos, (void*)d_off, (void*)d_cell, (void*)d_coff, (void*)d_clist,
                  (void*)d_weight, (void*)stage})
    CHECK(hipFree(q) == hipSuccess);
  return (nrow + rpp - 1) / rpp;
}

int main() {
  const int NC = 100, TR = 23;                       // 100 cells, 234 HRUs, ends inside a wave
  const Dom d = make_dom(NC, {88});
  CHECK(d.nhru == 234);
  // ---- dense 4 x 4 transforms: the four "members" of a column are the cells c, c + 3, c + 6, c + 9 of one residue mod 3, so
  // they agree in structure; 21 columns, a third of them with 3 HRUs
  Call dense;
  for (int k = 0; k < 19; k++) dense.rows.push_back((k * 7 + 3) % TR);               // 19 of 23 rows, out of order, no multiple of MX_ROWS
  for (int c = 0; c < 12 * 7; c += 12)
    for (int m = 0; m < 4; m++) {
      std::vector<int> cells; std::vector<double> w;
      for (int q = 0; q < 4; q++) { cells.push_back(c + 3 * q); w.push_back(0.3 * (m + 1) - 0.45 * q + 0.01 * c); }
      for (int r = 1; r < 3; r++)
        for (int q = 0; q < 4; q++) { cells.push_back(c + r + 3 * q); w.push_back(0.1 * r); }
      // three destinations a round: residue 0 (3 HRUs), 1 and 2 (2 HRUs)
      dense.add(c + 3 * m, std::vector<int>(cells.begin(), cells.begin() + 4), std::vector<double>(w.begin(), w.begin() + 4));
      dense.add(c + 1 + 3 * m, std::vector<int>(cells.begin() + 4, cells.begin() + 8), std::vector<double>(w.begin() + 4, w.begin() + 8));
      dense.add(c + 2 + 3 * m, std::vector<int>(cells.begin() + 8, cells.end()), std::vector<double>(w.begin() + 8, w.end()));
    }
  CHECK(dense.dst.size() == 84);
  const size_t nh = 7 * 4 * (3 + 2 + 2);
  CHECK(run_mix(d, TR, dense, 1 << 20) == 1);
  CHECK(run_mix(d, TR, dense, 0) == 19);                                               // one row per pass
  CHECK(run_mix(d, TR, dense, 5 * nh * sizeof(double) + 3) == 4);                      // 5 rows fit: 4 passes, the last ragged
  printf("dense: 84 destinations x 4 terms, 19 rows, one pass, one-row passes, ragged passes\n");
  // ---- irregular: out of order, 1 / 2 / 3 / 65 terms, a term of itself, terms of each other, the table's last row and column
  Call irr;
  irr.rows = {TR - 1, 0, 7};
  irr.add(99, {96}, {1.0});                                                            // 99 % 3 == 0: 3 HRUs, the last HRU id
  irr.add(30, {30, 33}, {0.5, 0.5});                                                   // 3 HRUs, a term of itself
  irr.add(4, {7, 10, 7}, {0.25, 1.5, -0.75});
  { std::vector<int> cells; std::vector<double> w;
    for (int q = 0; q < 65; q++) { cells.push_back(2 + 3 * (q % 5)); w.push_back(0.01 * q - 0.3); }
    irr.add(2, cells, w); }
  irr.add(13, {16, 13}, {0.25, 0.75});
  irr.add(16, {13, 16}, {2.0, -1.0});
  irr.add(88, {88, 88}, {0.5, 0.5});                                                   // the odd cell with itself
  CHECK(run_mix(d, TR, irr, 1 << 20) == 1);
  CHECK(run_mix(d, TR, irr, 0) == 3);
  { Call one; one.rows = {22}; one.add(99, {99}, {-2.0}); CHECK(run_mix(d, TR, one, 0) == 1); }
  printf("irregular: 1, 2, 3 and 65 terms, self and mutual terms, the last row and column\n");
  // ---- what the plan refuses, and whom it names
  const auto fault = [&](const Call& c) { return plan(d, TR, c); };
  Call good; good.rows = {1, 2}; good.add(13, {16, 13}, {0.5, 0.5}); good.add(16, {13}, {1.0});
  CHECK(fault(good).fault == MIX_OK);
  { Call c = good; c.rows = {1, TR}; const MixPlan p = fault(c); CHECK(p.fault == MIX_ROW_RANGE && p.row == 1); }
  { Call c = good; c.rows = {-1}; CHECK(fault(c).fault == MIX_ROW_RANGE); }
  { Call c = good; c.rows = {2, 1, 2}; const MixPlan p = fault(c); CHECK(p.fault == MIX_ROW_REPEATS && p.row == 2); }
  { Call c = good; c.dst[1] = NC; const MixPlan p = fault(c); CHECK(p.fault == MIX_DST_RANGE && p.dst == 1); }
  { Call c = good; c.dst[0] = -1; CHECK(fault(c).fault == MIX_DST_RANGE); }
  { Call c = good; c.dst[1] = 13; const MixPlan p = fault(c); CHECK(p.fault == MIX_DST_REPEATS && p.dst == 1); }
  { Call c = good; c.off[0] = 1; CHECK(fault(c).fault == MIX_OFFSETS); }
  { Call c = good; c.off = {0, 2, 1}; const MixPlan p = fault(c); CHECK(p.fault == MIX_OFFSETS && p.dst == 1); }
  { Call c = good; c.off = {0, 0, 3}; const MixPlan p = fault(c); CHECK(p.fault == MIX_NO_TERM && p.dst == 0); }
  { Call c = good; c.off = {0, 3, 3}; const MixPlan p = fault(c); CHECK(p.fault == MIX_NO_TERM && p.dst == 1); }
  { Call c = good; c.cell[2] = NC; const MixPlan p = fault(c); CHECK(p.fault == MIX_TERM_RANGE && p.dst == 1 && p.term == 2); }
  { Call c = good; c.cell[0] = -1; CHECK(fault(c).fault == MIX_TERM_RANGE); }
  { Call c = good; c.weight[1] = std::nan(""); const MixPlan p = fault(c); CHECK(p.fault == MIX_WEIGHT && p.dst == 0 && p.term == 1); }
  { Call c = good; c.weight[2] = std::numeric_limits<double>::infinity(); CHECK(fault(c).fault == MIX_WEIGHT); }
  { Call c = good; c.weight[0] = -std::numeric_limits<double>::infinity(); CHECK(fault(c).fault == MIX_WEIGHT); }
  { Call c = good; c.cell[2] = 15; const MixPlan p = fault(c); CHECK(p.fault == MIX_HRU_COUNT && p.dst == 1 && p.term == 2); }       // 15: 3 HRUs
  { Call c = good; c.cell[0] = 88; const MixPlan p = fault(c); CHECK(p.fault == MIX_HRU_STRUCTURE && p.dst == 0 && p.term == 0); }  // the odd cell
  { Call c; c.rows = {1}; c.add(13, {16, 19}, {1.0, 1.0}); c.add(88, {16}, {1.0});                                                 // ... in a later destination
    const MixPlan p = fault(c); CHECK(p.fault == MIX_HRU_STRUCTURE && p.dst == 1 && p.term == 2); }
  { Call c; c.rows = {1}; c.add(13, {16}, {1.0}); c.add(19, {22}, {1.0}); c.add(16, {22, 88}, {1.0, 1.0});                         // ... behind legal terms
    const MixPlan p = fault(c); CHECK(p.fault == MIX_HRU_STRUCTURE && p.dst == 2 && p.term == 3); }
  CHECK(mix_fault_text(fault(good)).find("mix_cells") == 0);
  { Call c = good; c.cell[0] = 88; const std::string s = mix_fault_text(fault(c)); CHECK(s.find("destination 0") != std::string::npos && s.find("term 0") != std::string::npos); }
  { MixPlan p; plan_cell_mix(p, d.ncell, d.nhru, d.off.data(), d.list.data(), d.key.data(), 2, nullptr, TR, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
    CHECK(p.fault == MIX_OK && p.size() == 0); }
  printf("plan: rows, destinations, offsets, term cells, weights, pairs\n");
  if (failed) { fprintf(stderr, "%d checks failed\n", failed); return 1; }
  printf("mix_cells_check: all checks held\n");
  return 0;
}
