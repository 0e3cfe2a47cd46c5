// host_layer_check.cpp — the parts of the host layer that need no kernel, as a stand-alone program under ASan + UBSan:
// the counted transfers of Buf (vic_amd/csrc/vic_host.hpp), the domain-list and state-record checks (vic_checks.hpp) and the
// tuning variables (Tuning / read_tuning of vic_pipeline.hpp, of which nothing else is used).  Built against the stand-in
// hip/hip_runtime.h of this directory, where "device" memory is malloc'ed, so a copy past the end of a table is a
// sanitizer report.  Built and run by tests/test_host_layer.py; exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "vic_host.hpp"
#include "vic_checks.hpp"
#include "vic_pipeline.hpp"

static int failed = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      failed++;                                                            \
      fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond);            \
    }                                                                      \
  } while (0)

static hipStream_t stream = nullptr;     // the stand-in's streams are tokens

static void transfers() {
  const int GUARD = -77;
  std::vector<int> src(10), dst(10, GUARD);
  for (int i = 0; i < 10; i++) src[i] = 100 + i;
  DevBuf<int> b;
  CHECK(b.alloc(10) == hipSuccess && b.size() == 10);
  // whole buffer, both ways
  CHECK(b.upload(stream, src.data()) == hipSuccess);
  CHECK(b.download(stream, dst.data()) == hipSuccess);
  CHECK(dst == src);
  // (first, count): exactly those elements, on both sides
  const int part[3] = {7, 8, 9};
  CHECK(b.upload(stream, part, 4, 3) == hipSuccess);
  CHECK(b.download(stream, dst.data()) == hipSuccess);
  for (int i = 0; i < 10; i++) CHECK(dst[i] == (i >= 4 && i < 7 ? part[i - 4] : 100 + i));
  std::vector<int> win(5, GUARD);
  CHECK(b.download(stream, win.data() + 1, 5, 3) == hipSuccess);
  CHECK(win[0] == GUARD && win[1] == 8 && win[2] == 9 && win[3] == 107 && win[4] == GUARD);
  CHECK(b.fill(stream, 0, 8, 2) == hipSuccess);
  CHECK(b.download(stream, dst.data()) == hipSuccess);
  CHECK(dst[7] == 107 && dst[8] == 0 && dst[9] == 0);
  // one element past size(): refused, and nothing moved
  std::vector<int> guard(12, GUARD);
  CHECK(b.download(stream, guard.data(), 8, 3) == hipErrorInvalidValue);
  CHECK(b.download(stream, guard.data(), 11, 0) == hipErrorInvalidValue);
  CHECK(b.download(stream, guard.data(), 0, 11) == hipErrorInvalidValue);
  CHECK(b.download(stream, guard.data(), 1, (size_t)-1) == hipErrorInvalidValue);      // first + count wraps
  for (int v : guard) CHECK(v == GUARD);
  std::vector<int> before(10), after(10);
  CHECK(b.download(stream, before.data()) == hipSuccess);
  CHECK(b.upload(stream, guard.data(), 8, 3) == hipErrorInvalidValue);
  CHECK(b.fill(stream, 0x55, 8, 3) == hipErrorInvalidValue);
  CHECK(b.download(stream, after.data()) == hipSuccess);
  CHECK(before == after);
  CHECK(b.upload(stream, guard.data(), 10, 0) == hipSuccess);                          // the empty range at the end is in range

  // allocate-and-fill
  DevBuf<double> z;
  CHECK(z.alloc_fill(33, 0, stream) == hipSuccess && z.size() == 33);
  std::vector<unsigned char> bytes(33 * sizeof(double), 1);
  CHECK(hipMemcpy(bytes.data(), z.get(), bytes.size(), hipMemcpyDeviceToHost) == hipSuccess);
  for (unsigned char v : bytes) CHECK(v == 0);
  DevBuf<int> ff;
  CHECK(ff.alloc_fill(9, 0xFF, stream) == hipSuccess);
  std::vector<int> ones(9, 0);
  CHECK(ff.download(stream, ones.data()) == hipSuccess);
  for (int v : ones) CHECK(v == -1);
  // a refused allocation: the error, no object more, an empty buffer -- also for one that held something
  const long long live = hostemu_live_objects();
  DevBuf<int> r;
  hostemu_refuse_alloc(1);
  CHECK(r.alloc_fill(16, 0, stream) != hipSuccess);
  hostemu_refuse_alloc(0);
  CHECK(hostemu_live_objects() == live && r.get() == nullptr && r.size() == 0);
  hostemu_refuse_alloc(1);
  CHECK(ff.alloc_fill(16, 0, stream) != hipSuccess);
  hostemu_refuse_alloc(0);
  CHECK(hostemu_live_objects() == live - 1 && ff.get() == nullptr && ff.size() == 0);
}

static void pitched_download() {
  const size_t nrow = 3, ncell = 4, ld = 7, col = 2;
  const float GUARD = -5.f;
  std::vector<float> src(nrow * ncell);
  for (size_t i = 0; i < src.size(); i++) src[i] = 1.f + (float)i;
  DevBuf<float> b;
  CHECK(b.alloc(nrow * ncell) == hipSuccess && b.upload(stream, src.data()) == hipSuccess);
  std::vector<float> wide(nrow * ld, GUARD);      // exactly its size: the last row ends ld - col - ncell cells before the end
  CHECK(b.download_cols(stream, wide.data() + col, ld, nrow, ncell) == hipSuccess);
  int landed = 0, kept = 0;
  for (size_t r = 0; r < nrow; r++)
    for (size_t i = 0; i < ld; i++) {
      const float v = wide[r * ld + i];
      if (i >= col && i < col + ncell) landed += v == src[r * ncell + (i - col)];
      else kept += v == GUARD;
    }
  CHECK(landed == 12 && kept == 9);
  std::vector<float> packed(nrow * ncell, GUARD);
  CHECK(b.download_cols(stream, packed.data(), ncell, nrow, ncell) == hipSuccess);
  CHECK(packed == src);
  // fewer rows than the table holds (the public rows of a longer table)
  std::fill(wide.begin(), wide.end(), GUARD);
  CHECK(b.download_cols(stream, wide.data(), ld, 2, ncell) == hipSuccess);
  CHECK(wide[ld + ncell - 1] == src[2 * ncell - 1] && wide[2 * ld] == GUARD);
  // refused, nothing moved: rows narrower than the table's, more rows than the buffer holds
  std::fill(wide.begin(), wide.end(), GUARD);
  CHECK(b.download_cols(stream, wide.data(), ncell - 1, nrow, ncell) == hipErrorInvalidValue);
  CHECK(b.download_cols(stream, wide.data(), ld, nrow + 1, ncell) == hipErrorInvalidValue);
  for (float v : wide) CHECK(v == GUARD);
}

// A valid domain of 3 cells and 5 HRUs: cell 0 holds HRUs 3 and 0, cell 1 none, cell 2 holds 4, 1 and 2 (a ragged list, not in
// HRU order); two bands, nveg_types + 4 = 6 rows of the vegetation library.  hpi is allocated at exactly its size.
struct TestDomain {
  int ncell = 3, nhru = 5, Nband = 2, nveg_rows = 6;
  std::vector<int> off{0, 2, 2, 5}, list{3, 0, 4, 1, 2};
  std::vector<int> hpi;
  TestDomain() : hpi((size_t)HPI_NROW * 5, 0) {
    const int cell[5] = {0, 2, 2, 0, 2}, band[5] = {0, 1, 0, 1, 1}, veg[5] = {5, 0, 3, 2, 1};
    for (int g = 0; g < 5; g++) { row(HPI_CELL)[g] = cell[g]; row(HPI_BAND)[g] = band[g]; row(HPI_VEG_INDEX)[g] = veg[g]; }
  }
  int* row(int r) { return hpi.data() + (size_t)r * nhru; }
  DomainFault check(bool hru_ranges = true) const {
    // copies at exactly their sizes, so that a read past any of them is seen
    std::vector<int> o(off), l(list), h(hpi);
    o.shrink_to_fit(); l.shrink_to_fit(); h.shrink_to_fit();
    return check_domain_lists(ncell, nhru, o.data(), l.data(), h.data(), hru_ranges ? Nband : 0, hru_ranges ? nveg_rows : 0);
  }
};

static void list_check() {
  { TestDomain d; CHECK(d.check().rule == DOMAIN_OK); CHECK(d.check(false).rule == DOMAIN_OK); }
  DomainFault f;
  { TestDomain d; d.off[0] = 1; f = d.check(); CHECK(f.rule == DOMAIN_OFFSET_SPAN && f.index == 0); }
  { TestDomain d; d.off[1] = 3; f = d.check(); CHECK(f.rule == DOMAIN_OFFSET_DECREASES && f.index == 2); }      // 0 3 2 5
  { TestDomain d; d.off[3] = 4; f = d.check(); CHECK(f.rule == DOMAIN_OFFSET_SPAN && f.index == 3); }
  { TestDomain d; d.off[3] = 6; f = d.check(); CHECK(f.rule == DOMAIN_OFFSET_SPAN && f.index == 3); }
  // an offset far past the list, hidden by a later decrease: refused before any list entry is read
  { TestDomain d; d.off[1] = 1000; f = d.check(); CHECK(f.rule == DOMAIN_OFFSET_DECREASES && f.index == 2); }
  { TestDomain d; d.list[3] = -1; f = d.check(); CHECK(f.rule == DOMAIN_LIST_ENTRY && f.index == 3); }
  { TestDomain d; d.list[3] = d.nhru; f = d.check(); CHECK(f.rule == DOMAIN_LIST_ENTRY && f.index == 3); }
  { TestDomain d; d.list[2] = 1 << 30; f = d.check(); CHECK(f.rule == DOMAIN_LIST_ENTRY && f.index == 2); }
  // listed twice, within its own cell: the second mention is the fault
  { TestDomain d; d.list[4] = 1; f = d.check(); CHECK(f.rule == DOMAIN_LIST_ENTRY && f.index == 4); }
  // under a cell other than its own: HRU 3 (cell 0) and HRU 4 (cell 2) change places
  { TestDomain d; std::swap(d.list[0], d.list[2]); f = d.check(); CHECK(f.rule == DOMAIN_LIST_ENTRY && f.index == 0); }
  { TestDomain d; d.row(HPI_CELL)[1] = 1; f = d.check(); CHECK(f.rule == DOMAIN_LIST_ENTRY && f.index == 3); }
  // never listed: the list has nhru places, so the place of HRU 2 holds one that is listed elsewhere (HRU 0, of another cell)
  { TestDomain d; d.list[4] = 0; f = d.check(); CHECK(f.rule == DOMAIN_LIST_ENTRY && f.index == 4); }
  { TestDomain d; d.row(HPI_BAND)[3] = d.Nband; f = d.check(); CHECK(f.rule == DOMAIN_BAND && f.index == 3); CHECK(d.check(false).rule == DOMAIN_OK); }
  { TestDomain d; d.row(HPI_BAND)[0] = -1; f = d.check(); CHECK(f.rule == DOMAIN_BAND && f.index == 0); }
  { TestDomain d; d.row(HPI_VEG_INDEX)[4] = d.nveg_rows; f = d.check(); CHECK(f.rule == DOMAIN_VEG_INDEX && f.index == 4); CHECK(d.check(false).rule == DOMAIN_OK); }
  { TestDomain d; d.row(HPI_VEG_INDEX)[2] = -1; f = d.check(); CHECK(f.rule == DOMAIN_VEG_INDEX && f.index == 2); }
}

static void state_record_check() {
  const size_t L = VICGPU_SR_LEN(3);
  std::vector<double> rec(3 * L, 0.0);
  rec.shrink_to_fit();
  for (int k = 0; k < 3; k++) { rec[k * L + SR_BAND_INDEX] = k % 2; rec[k * L + SR_VEG_CLASS] = 10 + k; }
  for (int k = 0; k < 3; k++) CHECK(check_state_record(rec.data() + k * L, k, k % 2, 10 + k).empty());
  const std::string band = check_state_record(rec.data() + 2 * L, 2, 1, 12), veg = check_state_record(rec.data() + 1 * L, 1, 1, 12);
  CHECK(band == "state record 2: band / vegetation class do not match the domain (write_model_state.c:179-188)");
  CHECK(veg == "state record 1: band / vegetation class do not match the domain (write_model_state.c:179-188)");
}

static const char* const TUNING_VARS[] = {"VICGPU_NODE_SOLVER", "VICGPU_EVAL_LIST_PCT", "VICGPU_CHUNKS", "VICGPU_PROFILE_WAVES_PCT",
                                          "VICGPU_NO_XCD_MAP", "VICGPU_TRACE_ROUNDS", "VICGPU_TRACE", "VICGPU_STATS"};
static Tuning tuning_with(const char* name, const char* value, int node_solver = VIC_NODE_SOLVER_BRENT, int ncell = 100) {
  for (const char* v : TUNING_VARS) unsetenv(v);
  if (name) setenv(name, value, 1);
  const Tuning t = read_tuning(node_solver, ncell);
  for (const char* v : TUNING_VARS) unsetenv(v);
  return t;
}

static void tuning() {
  Tuning t = tuning_with(nullptr, nullptr);
  CHECK(!t.node_newton && t.eval_list_pct == 75 && t.nchunk == 1 && t.profile_waves_pct == 100 && t.xcd_map && !t.trace_rounds && !t.trace && !t.stats);
  CHECK(tuning_with(nullptr, nullptr, VIC_NODE_SOLVER_NEWTON).node_newton);
  // the 20 000-cell rule, and the half share of the wave slots that goes with two chunks
  CHECK(tuning_with(nullptr, nullptr, VIC_NODE_SOLVER_BRENT, 19999).nchunk == 1);
  t = tuning_with(nullptr, nullptr, VIC_NODE_SOLVER_BRENT, 20000);
  CHECK(t.nchunk == 2 && t.profile_waves_pct == 50);
  // each variable
  CHECK(tuning_with("VICGPU_NODE_SOLVER", "newton").node_newton);
  CHECK(!tuning_with("VICGPU_NODE_SOLVER", "brent", VIC_NODE_SOLVER_NEWTON).node_newton);
  CHECK(!tuning_with("VICGPU_NODE_SOLVER", "Newton").node_newton);                  // compared exactly
  CHECK(!tuning_with("VICGPU_NODE_SOLVER", "", VIC_NODE_SOLVER_NEWTON).node_newton);
  CHECK(tuning_with("VICGPU_EVAL_LIST_PCT", "0").eval_list_pct == 0);
  CHECK(tuning_with("VICGPU_EVAL_LIST_PCT", "100").eval_list_pct == 100);
  CHECK(tuning_with("VICGPU_EVAL_LIST_PCT", "101").eval_list_pct == 75);
  CHECK(tuning_with("VICGPU_EVAL_LIST_PCT", "-1").eval_list_pct == 75);
  CHECK(tuning_with("VICGPU_EVAL_LIST_PCT", "x").eval_list_pct == 0);               // atoi
  t = tuning_with("VICGPU_CHUNKS", "3");
  CHECK(t.nchunk == 3 && t.profile_waves_pct == 50);
  CHECK(tuning_with("VICGPU_CHUNKS", "abc").nchunk == 1);
  CHECK(tuning_with("VICGPU_CHUNKS", "0").nchunk == 1);
  CHECK(tuning_with("VICGPU_CHUNKS", "-4").nchunk == 1);
  CHECK(tuning_with("VICGPU_CHUNKS", "99").nchunk == 16);
  CHECK(tuning_with("VICGPU_CHUNKS", "99", VIC_NODE_SOLVER_BRENT, 5).nchunk == 5);   // at most a chunk per cell
  t = tuning_with("VICGPU_CHUNKS", "1", VIC_NODE_SOLVER_BRENT, 50000);
  CHECK(t.nchunk == 1 && t.profile_waves_pct == 100);
  CHECK(tuning_with("VICGPU_PROFILE_WAVES_PCT", "30").profile_waves_pct == 30);
  CHECK(tuning_with("VICGPU_PROFILE_WAVES_PCT", "5").profile_waves_pct == 5);
  CHECK(tuning_with("VICGPU_PROFILE_WAVES_PCT", "3").profile_waves_pct == 100);     // ignored
  CHECK(tuning_with("VICGPU_PROFILE_WAVES_PCT", "3", VIC_NODE_SOLVER_BRENT, 20000).profile_waves_pct == 50);
  CHECK(tuning_with("VICGPU_PROFILE_WAVES_PCT", "101").profile_waves_pct == 100);
  CHECK(tuning_with("VICGPU_PROFILE_WAVES_PCT", "junk").profile_waves_pct == 100);
  CHECK(!tuning_with("VICGPU_NO_XCD_MAP", "").xcd_map);                             // set is enough
  CHECK(tuning_with("VICGPU_TRACE_ROUNDS", "1").trace_rounds);
  CHECK(tuning_with("VICGPU_TRACE", "1").trace && !tuning_with("VICGPU_TRACE", "1").trace_rounds);
  CHECK(tuning_with("VICGPU_STATS", "0").stats);
  // nothing is kept from one reading to the next
  t = tuning_with(nullptr, nullptr);
  CHECK(!t.node_newton && t.eval_list_pct == 75 && t.nchunk == 1 && t.profile_waves_pct == 100 && t.xcd_map && !t.trace_rounds && !t.trace && !t.stats);
}

int main() {
  const long long live = hostemu_live_objects();
  transfers();
  pitched_download();
  list_check();
  state_record_check();
  tuning();
  CHECK(hostemu_live_objects() == live);
  printf("host_layer_check: %d problems\n", failed);
  return failed ? 1 : 0;
}
