// vic_checks.hpp — the checks of what a caller hands in that need no runtime: the lists of a domain (vicgpu_set_domain and
// vicgpu_group_set_domain), the header of a state record (vicgpu_set_state_records and the group's) and the lists of
// vicgpu_prefetch_forcing_perturbed (and the group's).  Written once, used
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

// The lists of vicgpu_prefetch_forcing_perturbed (and the group's, on the whole domain) against the width ncol of the forcing
// tables: the empty string when the call is legal, else the message of the refusal.  nsteps > 0, nsrc >= 1 and the non-null
// raw and dmy are the caller's to check first.
static inline std::string check_forcing_perturbed(int ncol, int nsteps, int nsrc, const int* col_src, int ngroup, const int* col_group,
                                                  const double* pert, const int* dmy) {
  const std::string name = "prefetch_forcing_perturbed: ";
  for (int s = 0; s < nsteps; s++) {
    const int m = dmy[(size_t)s * VIC_NDMY + VIC_DMY_MONTH];
    if (m < 1 || m > 12) return name + "step " + std::to_string(s) + ": month " + std::to_string(m) + " is not in 1..12";
  }
  if (!col_src && nsrc != ncol) return name + "no col_src, but nsrc is not the " + std::to_string(ncol) + " forcing columns";
  if (col_src)
    for (int i = 0; i < ncol; i++)
      if (col_src[i] < 0 || col_src[i] >= nsrc) return name + "col_src entry " + std::to_string(i) + " is not a source column";
  if (ngroup < 0) return name + "ngroup < 0";
  if (ngroup > 0 && !pert) return name + "groups without pert";
  if (ngroup == 0 && pert) return name + "pert without groups";
  if (ngroup == 0 && col_group) return name + "col_group without groups";
  if (!col_group && ngroup != 0 && ngroup != ncol) return name + "no col_group, but ngroup is neither 0 nor the " + std::to_string(ncol) + " forcing columns";
  if (col_group)
    for (int i = 0; i < ncol; i++)
      if (col_group[i] < 0 || col_group[i] >= ngroup) return name + "col_group entry " + std::to_string(i) + " is not a group";
  if (pert)
    for (int s = 0; s < nsteps; s++)
      for (int r = 0; r < VICGPU_NPERT; r++)
        for (int g = 0; g < ngroup; g++) {
          const double v = pert[((size_t)s * VICGPU_NPERT + r) * ngroup + g];
          if (!(v - v == 0.0))       // NaN or an infinity
            return name + "pert is not finite at step " + std::to_string(s) + ", row " + std::to_string(r) + ", group " + std::to_string(g);
        }
  return std::string();
}
