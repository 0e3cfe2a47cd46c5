// The argument check of vicgpu_prefetch_forcing_perturbed (check_forcing_perturbed, vic_amd/csrc/vic_checks.hpp) as a program of
// its own for ASan + UBSan (tests/test_forcing_perturb.py builds and runs it).  The check needs no runtime, so nothing is
// emulated here.  Every list lives in a heap block of exactly its size: a read past ncol, past nsteps or past pert's end is a
// sanitizer report.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>
#include "vic_checks.hpp"

static int failures = 0;
static void expect(const char* what, const std::string& got, const char* part) {
  const bool ok = part ? got.find(part) != std::string::npos : got.empty();
  if (!ok) { printf("FAILED %s: \"%s\"\n", what, got.c_str()); failures++; }
}

int main() {
  const int ncol = 15, nsrc = 5, M = 3, nsteps = 4;
  std::vector<int> src(ncol), grp(ncol), dmy((size_t)nsteps * VIC_NDMY, 1);
  for (int i = 0; i < ncol; i++) { src[i] = i % nsrc; grp[i] = i / nsrc; }
  std::vector<double> pert((size_t)nsteps * VICGPU_NPERT * M, 1.0), percol((size_t)nsteps * VICGPU_NPERT * ncol, 0.5);
  auto chk = [&](int ns, const int* s, int ng, const int* g, const double* p, const int* d) {
    return check_forcing_perturbed(ncol, nsteps, ns, s, ng, g, p, d);
  };
  expect("legal call", chk(nsrc, src.data(), M, grp.data(), pert.data(), dmy.data()), nullptr);
  expect("no perturbation", chk(nsrc, src.data(), 0, nullptr, nullptr, dmy.data()), nullptr);
  expect("both lists null", chk(ncol, nullptr, 0, nullptr, nullptr, dmy.data()), nullptr);
  expect("a group per column", chk(nsrc, src.data(), ncol, nullptr, percol.data(), dmy.data()), nullptr);
  expect("one source, one group", check_forcing_perturbed(1, 1, 1, nullptr, 1, nullptr, pert.data(), dmy.data()), nullptr);
  { std::vector<int> d = dmy; d[(size_t)(nsteps - 1) * VIC_NDMY + VIC_DMY_MONTH] = 13; expect("month 13", chk(nsrc, src.data(), M, grp.data(), pert.data(), d.data()), "month"); }
  { std::vector<int> d = dmy; d[VIC_DMY_MONTH] = 0; expect("month 0", chk(nsrc, src.data(), M, grp.data(), pert.data(), d.data()), "month"); }
  expect("no col_src, nsrc != ncol", chk(nsrc, nullptr, M, grp.data(), pert.data(), dmy.data()), "no col_src");
  { std::vector<int> s = src; s[ncol - 1] = nsrc; expect("col_src == nsrc", chk(nsrc, s.data(), M, grp.data(), pert.data(), dmy.data()), "col_src entry 14"); }
  { std::vector<int> s = src; s[0] = -1; expect("col_src < 0", chk(nsrc, s.data(), M, grp.data(), pert.data(), dmy.data()), "col_src entry 0"); }
  expect("ngroup < 0", chk(nsrc, src.data(), -1, grp.data(), pert.data(), dmy.data()), "ngroup < 0");
  expect("groups without pert", chk(nsrc, src.data(), M, grp.data(), nullptr, dmy.data()), "without pert");
  expect("pert without groups", chk(nsrc, src.data(), 0, nullptr, pert.data(), dmy.data()), "without groups");
  expect("col_group without groups", chk(nsrc, src.data(), 0, grp.data(), nullptr, dmy.data()), "without groups");
  expect("no col_group, ngroup != ncol", chk(nsrc, src.data(), M, nullptr, pert.data(), dmy.data()), "no col_group");
  { std::vector<int> g = grp; g[ncol - 1] = M; expect("col_group == ngroup", chk(nsrc, src.data(), M, g.data(), pert.data(), dmy.data()), "col_group entry 14"); }
  { std::vector<int> g = grp; g[3] = -1; expect("col_group < 0", chk(nsrc, src.data(), M, g.data(), pert.data(), dmy.data()), "col_group entry 3"); }
  { std::vector<double> p = pert; p.back() = std::nan("");
    expect("NaN in the last value", chk(nsrc, src.data(), M, grp.data(), p.data(), dmy.data()), "step 3, row 13, group 2"); }
  { std::vector<double> p = pert; p[((size_t)2 * VICGPU_NPERT + 5) * M + 1] = -std::numeric_limits<double>::infinity();
    expect("-inf", chk(nsrc, src.data(), M, grp.data(), p.data(), dmy.data()), "step 2, row 5, group 1"); }
  { std::vector<double> p = pert; p[0] = std::numeric_limits<double>::max(); p[1] = -0.0; p[2] = std::numeric_limits<double>::denorm_min();
    expect("huge, negative zero and denormal values are finite", chk(nsrc, src.data(), M, grp.data(), p.data(), dmy.data()), nullptr); }
  if (failures) { printf("forcing_perturb_check: %d checks failed\n", failures); return 1; }
  printf("forcing_perturb_check: all checks held\n");
  return 0;
}
