// vic_checks.hpp — the checks of what a caller hands in that need no runtime: the lists of a domain (vicgpu_set_domain and
// vicgpu_group_set_domain) and the header of a state record (vicgpu_set_state_records and the group's).  Written once, used
// by the single context and by the group.  Host code only: include/vicgpu.h and the standard library, no HIP.
#pragma once
#include <cstddef>
#include <string>
#include <vector>
#include "vicgpu.h"

// The rule of check_domain_lists that failed, and where: `index` is the cell of an offset, the position of a
// cell_hru_list entry, or the HRU of a band / vegetation index
enum DomainRule { DOMAIN_OK = 0, DOMAIN_OFFSET_SPAN, DOMAIN_OFFSET_DECREASES, DOMAIN_LIST_ENTRY, DOMAIN_BAND, DOMAIN_VEG_INDEX };
struct DomainFault {
  DomainRule rule = DOMAIN_OK;
  int index = 0;
};

// cell_hru_offset [ncell + 1] starts at 0, never decreases and ends at nhru; every cell_hru_list entry is an HRU in range,
// listed once, under the cell its HPI_CELL row names.  The list has nhru entries then, all different, so no HRU is left
// out.  With Nband > 0 also: every HRU's band is below Nband and its vegetation index below nveg_rows.  Every index the
// kernels (and the group, to slice the domain) dereference is validated here, once; the offsets are checked as a whole
// before the first list entry is read, and no hpi element is read before the index into it is known to be in range.
static inline DomainFault check_domain_lists(int ncell, int nhru, const int* off, const int* list, const int* hpi, int Nband = 0,
                                             int nveg_rows = 0) {
  if (off[0] != 0) return {DOMAIN_OFFSET_SPAN, 0};
  if (off[ncell] != nhru) return {DOMAIN_OFFSET_SPAN, ncell};
  for (int i = 0; i < ncell; i++)
    if (off[i + 1] < off[i]) return {DOMAIN_OFFSET_DECREASES, i + 1};
  std::vector<char> seen(nhru, 0);
  for (int i = 0; i < ncell; i++)
    for (int j = off[i]; j < off[i + 1]; j++) {
      const int g = list[j];
      if (g < 0 || g >= nhru || seen[g] || hpi[(size_t)HPI_CELL * nhru + g] != i) return {DOMAIN_LIST_ENTRY, j};
      seen[g] = 1;
    }
  if (Nband > 0)
    for (int g = 0; g < nhru; g++) {
      const int b = hpi[(size_t)HPI_BAND * nhru + g], v = hpi[(size_t)HPI_VEG_INDEX * nhru + g];
      if (b < 0 || b >= Nband) return {DOMAIN_BAND, g};
      if (v < 0 || v >= nveg_rows) return {DOMAIN_VEG_INDEX, g};
    }
  return {};
}

// State record k (`rec`: its VICGPU_SR_LEN doubles) against the band and vegetation class of the HRU it is for: the empty
// string when they match, else the message of the refusal (a reader that throws changes nothing, write_model_state.c:179-188)
static inline std::string check_state_record(const double* rec, size_t k, int band, int veg_class) {
  if ((int)rec[SR_BAND_INDEX] == band && (int)rec[SR_VEG_CLASS] == veg_class) return std::string();
  return "state record " + std::to_string(k) + ": band / vegetation class do not match the domain (write_model_state.c:179-188)";
}
