// round_layout_check.cpp — the layout accessors of vic_amd/csrc/vic_layout.hpp (item blocks and solution records of the
// finite-difference pipeline's rounds) as a stand-alone host program, built with ASan + UBSan (tests/test_round_layout.py).
// For each node count, with and without NOFLUX, every word an accessor names is written into tables of exactly the size
// domain_fd_workspace allocates (the sanitizer sees any word past the end) and owned by one accessor only.
#include <cstdio>
#include <cstdint>
#include <vector>
#include "vic_layout.hpp"

using namespace vic;

static int problems = 0;
#define CHECK(cond, ...)                                            \
  do {                                                              \
    if (!(cond)) { problems++; printf("FAIL " __VA_ARGS__); printf("  [%s]\n", #cond); } \
  } while (0)

// claims words [at, at + n) of an entry of `stride` words for owner `id`
static void claim(std::vector<int>& owner, int stride, int at, int n, int id, const char* what, int Nn) {
  for (int w = at; w < at + n; w++) {
    CHECK(w >= 0 && w < stride, "Nn=%d %s: word %d outside the stride %d\n", Nn, what, w, stride);
    if (w < 0 || w >= stride) continue;
    CHECK(owner[w] == 0, "Nn=%d %s: word %d already belongs to accessor %d\n", Nn, what, w, owner[w]);
    owner[w] = id;
  }
}

static void check_items(int Nn, bool noflux) {
  const int stride = item_stride(Nn);
  CHECK(stride % SECTOR_WORDS == 0, "Nn=%d item stride %d\n", Nn, stride);
  CHECK(stride >= item_words(Nn), "Nn=%d item stride %d < %d words\n", Nn, stride, item_words(Nn));
  std::vector<int> owner(stride, 0);
  int id = 0;
  claim(owner, stride, item_header(), 1, ++id, "header", Nn);
  for (int j = 0; j < Nn; j++) claim(owner, stride, item_t0(j), 1, ++id, "t0", Nn);
  const int jlast = noflux ? Nn : Nn - 1;                      // node records a solve reads: 1 .. jlast - 1
  for (int j = 1; j < jlast; j++) claim(owner, stride, item_rec(Nn, j), PREC, ++id, "rec", Nn);
  // the start column and the records a solve reads form a contiguous prefix
  int used = 0;
  while (used < stride && owner[used] != 0) used++;
  for (int w = used; w < stride; w++) CHECK(owner[w] == 0, "Nn=%d noflux=%d: word %d in use behind a hole at %d\n", Nn, (int)noflux, w, used);
  CHECK(used == (noflux ? item_words(Nn) : item_prefix_words(Nn)), "Nn=%d noflux=%d: prefix of %d words\n", Nn, (int)noflux, used);
  if (!noflux) {
    // the bottom record: last, disjoint from everything a solve reads, inside the stride
    CHECK(item_rec(Nn, Nn - 1) == used, "Nn=%d bottom record at %d, prefix ends at %d\n", Nn, item_rec(Nn, Nn - 1), used);
    claim(owner, stride, item_rec(Nn, Nn - 1), PREC, ++id, "bottom rec", Nn);
  }
  // the table as allocated, three HRUs: every block 16-byte aligned relative to the base, last word of the last block in bounds
  const size_t nhru = 3;
  std::vector<double> pin((size_t)stride * nhru, 0.0);
  for (size_t h = 0; h < nhru; h++) {
    double* blk = item_block(pin.data(), h, Nn);
    CHECK(((blk - pin.data()) * sizeof(double)) % 64 == 0, "Nn=%d block %zu not on a sector boundary\n", Nn, h);
    blk[item_header()] = 1.0;
    for (int j = 0; j < Nn; j++) blk[item_t0(j)] = 100.0 + j;
    for (int j = 1; j < Nn; j++)
      for (int f = 0; f < PREC; f++) blk[item_rec(Nn, j) + f] = 1000.0 * j + f;
  }
  for (size_t h = 0; h < nhru; h++) {
    const double* blk = item_block((const double*)pin.data(), h, Nn);
    bool same = blk[item_header()] == 1.0;
    for (int j = 0; j < Nn; j++) same = same && blk[item_t0(j)] == 100.0 + j;
    for (int j = 1; j < Nn; j++)
      for (int f = 0; f < PREC; f++) same = same && blk[item_rec(Nn, j) + f] == 1000.0 * j + f;
    CHECK(same, "Nn=%d block %zu: a word was overwritten by another accessor's\n", Nn, h);
  }
}

static void check_records(int Nn) {
  const int stride = pout_stride(Nn);
  CHECK(stride % SECTOR_WORDS == 0, "Nn=%d record stride %d\n", Nn, stride);
  CHECK(pout_hru_stride(Nn) == 2 * stride, "Nn=%d HRU stride %d\n", Nn, pout_hru_stride(Nn));
  CHECK(stride >= rec_words(Nn), "Nn=%d record stride %d < %d words\n", Nn, stride, rec_words(Nn));
  std::vector<int> owner(stride, 0);
  int id = 0;
  CHECK(rec_key() == rec_t(0), "the key is T of node 0\n");
  for (int j = 0; j < Nn; j++) claim(owner, stride, rec_t(j), 1, ++id, "T", Nn);
  claim(owner, stride, rec_flag(), 1, ++id, "flag", Nn);
  claim(owner, stride, rec_cnt(Nn), (Nn + 1) / 2, ++id, "counters", Nn);
  // what an evaluation of the iteration reads sits in the record's first sector
  CHECK(rec_key() < SECTOR_WORDS && rec_flag() < SECTOR_WORDS && rec_t(1) < SECTOR_WORDS && rec_t(2) < SECTOR_WORDS,
        "Nn=%d header words %d %d %d %d\n", Nn, rec_key(), rec_flag(), rec_t(1), rec_t(2));
  const size_t nhru = 3;
  std::vector<double> pout((size_t)pout_hru_stride(Nn) * nhru, 0.0);
  for (size_t h = 0; h < nhru; h++)
    for (int slot = 0; slot < 2; slot++) {
      double* rec = pout_rec(pout.data(), h, Nn, slot);
      CHECK(((rec - pout.data()) * sizeof(double)) % 64 == 0, "Nn=%d record %zu/%d not on a sector boundary\n", Nn, h, slot);
      for (int j = 0; j < Nn; j++) rec[rec_t(j)] = 10.0 * slot + j;
      rec[rec_flag()] = -1.0 - slot;
      int* cnt = reinterpret_cast<int*>(rec + rec_cnt(Nn));
      for (int j = 0; j < Nn; j++) cnt[j] = 7 * j + slot;
    }
  for (size_t h = 0; h < nhru; h++)
    for (int slot = 0; slot < 2; slot++) {
      const double* rec = pout_rec((const double*)pout.data(), h, Nn, slot);
      bool same = rec[rec_flag()] == -1.0 - slot;
      for (int j = 0; j < Nn; j++) same = same && rec[rec_t(j)] == 10.0 * slot + j;
      const int* cnt = reinterpret_cast<const int*>(rec + rec_cnt(Nn));
      for (int j = 0; j < Nn; j++) same = same && cnt[j] == 7 * j + slot;
      CHECK(same, "Nn=%d record %zu/%d: a word was overwritten by another accessor's\n", Nn, h, slot);
    }
}

int main() {
  const int counts[] = {3, 5, 10, 11, 24, 25, 50};
  for (int Nn : counts) {
    check_items(Nn, false);
    check_items(Nn, true);
    check_records(Nn);
  }
  // the figures the 10-node kernels are designed around
  CHECK(pout_hru_stride(10) * sizeof(double) == 256, "10 nodes: %zu bytes of records per HRU\n", pout_hru_stride(10) * sizeof(double));
  CHECK(item_prefix_words(10) == 91 && (item_prefix_words(10) + SECTOR_WORDS - 1) / SECTOR_WORDS == 12, "10 nodes: %d words per fetch\n", item_prefix_words(10));
  printf("round_layout_check: %d problems\n", problems);
  return problems ? 1 : 0;
}
