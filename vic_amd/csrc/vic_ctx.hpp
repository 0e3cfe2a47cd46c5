// vic_ctx.hpp — the parked context of the finite-difference pipeline (device only, gfx950): what an HRU carries in HBM
// across the ground-surface root finder, from the stage kernel that sets a sub-step up, through the evaluation kernel's rounds,
// to the stage kernel that books it (vic_kernels.hpp).
//
// Everything that decides WHERE a word of the context lives is here and nowhere else: the hstate bits, the word ranges of
// the structs (EBC_W_* / EBM_W_* / CW_* / CO_*), the lane groups, the parking map CTX_MAP with its static_asserts, and the
// only accessors allowed to use them (CtxRef, ctx_put / ctx_get and their _words variants, ebc_put / ebc_get, surf_eb_class).
// The host needs ctx_words and ctx_padded_words to size the table.
#pragma once
#include <cstddef>
#include <type_traits>
#include "vic_step.hpp"

using namespace vic;      // the kernels and what they are built from live in the global namespace (their names are matched by prefix)

// hstate[hru]: bits 0-1 state (0 idle, 1 evaluation pending, 2 root found: the stage kernel's turn), from bit 2 the EBG_* class
// of the root find.  (Stage, profile record and forcing sub-step packed into the same word, so that every load of the
// evaluation kernel can issue behind this one, were measured: 26.9 / 27.2 vs 27.0 / 27.2 ms per step -- nothing; removed.)
constexpr int HS_STATE = 3, HS_CLS_SHIFT = 2;

// ------------------------------------------------------------------------------------------------ parked context
// Plain structs are parked word by word.  The table is tiled by wave: one wave's whole context is a single contiguous slab
// (a handful of pages) instead of one row per word spread over the whole table, and inside the slab every lane owns runs of
// G consecutive words: [hru / 64][word / G][hru % 64][G].  G = 1 is the plain [word][lane] tiling (8-byte-per-lane rows run
// the load path at half its rate); G = 2 makes every access 16 bytes; G = 8 gives a lane whole 64-byte sectors, so a wave
// formed from the pending list (sparse rounds: lane = pending HRU, several slabs) wastes nothing of what it fetches,
// while a dense wave still reads its slab front to back (its 16-byte accesses, 64 bytes apart, fill the same lines over four
// instructions).  Measured, same box: evaluation kernel 6.8 vs 7.7-8.0 ms per step with the sparse rounds starting at 30 %
// pending instead of 4 %; the opening stage, which WRITES the context, 4.7-4.9 vs 4.3-4.5 ms.  So the slab has two regions:
// what the evaluation kernel reads (SurfSolve, SurfEBMut, SurfEBConst: words below CTX_NA) in groups of CTX_GROUP = 8, what
// only the two stage kernels exchange (everything after) in pairs.  (G = 16 and 32 measure like 8, G = 4 worse than 2.)
// (Not kept: one contiguous block per HRU, [hru][word], measured in round 2 against the slabs: sparse rounds -35 %, dense
// rounds +23 %.)
// SurfEBConst / SurfEBMut are parked group by group (vic_surface.hpp): word ranges of the groups
constexpr int EBC_W_POST = offsetof(SurfEBConst, delta_t) / 8, EBC_W_ALWAYS = offsetof(SurfEBConst, ice0) / 8,
              EBC_W_FROZEN = offsetof(SurfEBConst, kappa_snow) / 8, EBC_W_SNOWCOV = offsetof(SurfEBConst, LongSnowIn) / 8,
              EBC_W_INCL = offsetof(SurfEBConst, lmoist) / 8, EBC_W_EVAP = offsetof(SurfEBConst, Wdew) / 8,
              EBC_W_CANOPY = offsetof(SurfEBConst, Cs2) / 8;
constexpr int EBM_W_FEED = offsetof(SurfEBMut, deltaCC) / 8, EBM_W_IN3 = offsetof(SurfEBMut, Tsnow_surf) / 8,
              EBM_W_TSNOW = offsetof(SurfEBMut, ra_used) / 8, EBM_W_RA1 = EBM_W_TSNOW + 1, EBM_W_VV = offsetof(SurfEBMut, vv) / 8,
              EBM_W_KEEP = offsetof(SurfEBMut, Tnew2) / 8;
static_assert(offsetof(SurfEBMut, fusion) / 8 == EBM_W_IN3 - 1 && offsetof(SurfEBMut, layerevap) / 8 == EBM_W_VV + 3, "SurfEBMut layout");
constexpr size_t CW_SV = sizeof(SurfSolve) / 8, CW_EBM = sizeof(SurfEBMut) / 8, CW_EBC = EBC_W_CANOPY,      // Cs2 is never parked
                 CW_P = sizeof(SubStep) / 8, CW_L = sizeof(SubLoop) / 8, CW_C = sizeof(StepConst) / 8;
constexpr size_t CO_SV = 0, CO_EBM = CO_SV + CW_SV, CO_EBC = CO_EBM + CW_EBM, CO_P = CO_EBC + CW_EBC, CO_L = CO_P + CW_P,
                 CO_C = CO_L + CW_L, CO_W = CO_C + CW_C;
constexpr size_t CW_W = sizeof(WCarry) / 8, CO_WM = CO_W + CW_W;
template <int NN> constexpr size_t ctx_words() { return CO_WM + sizeof(WCarryMulti<NN>) / 8; }
static_assert(sizeof(StepConstPost) <= sizeof(StepConst), "StepConstPost is parked in StepConst's words");
// SubLoop in two parts: the head always, the sub-step sums only once a sub-step has been booked (they are zero before)
constexpr size_t CW_L_HEAD = offsetof(SubLoop, st_AlbedoOver) / 8;
// SurfSolve: the Brent state and the abscissa (rewritten by every evaluation), then the rest
constexpr size_t CW_SV_ITER = offsetof(SurfSolve, Tsurf) / 8;

constexpr int CTX_GROUP = 8, CTX_GROUP_B = 2;
constexpr size_t CTX_NA = sizeof(SurfSolve) / 8 + sizeof(SurfEBMut) / 8 + offsetof(SurfEBConst, Cs2) / 8;
static_assert(CTX_NA == CO_P, "region A of the context slab = what the evaluation kernel reads");
// Parking map of region A: struct word (CO_SV .. CO_P) -> slab word.  The structs keep their layout; where a word is parked
// follows who touches it, so that an evaluation of the iteration fetches whole 64-byte sectors it uses and no others.  Every
// range starts on a sector boundary:
//   CTXR_ITER    what an evaluation of the iteration rewrites: the Brent state and the abscissa (SurfSolve up to Tsurf)
//   CTXR_COMMON  what every evaluation reads: the SurfEBMut inputs of the iteration (deltaCC, NetLongSnow, fusion, Tsnow_surf,
//                ra_used[1]), then SurfEBConst [post] and [always]
//   CTXR_CLASS   [frozen], [evap], [canopy]: the groups of the common class of a frozen-soil run
//   CTXR_SNOW    [snowcov], [incl]
//   CTXR_COLD    what is read and written when the iteration ends or at the final evaluation: the tail of SurfSolve (result,
//                flags, stage, record bookkeeping) in the first sector, then ra_used[0], [feed] (thin snowpack only) and the
//                rest of SurfEBMut
// (The tail of SurfSolve stays among the words an evaluation fetches: surf_solve_consume needs it in the evaluation that ends
// the iteration, which is not known before the residual is.)
constexpr int CTXR_ITER = 0, CTXR_COMMON = 16, CTXR_CLASS = 48, CTXR_SNOW = 64, CTXR_COLD = 72, CTXR_END = 104;
struct CtxMap { unsigned char slab[CTX_NA]; int end[6]; };
constexpr int ctx_map_run(CtxMap& m, int at, size_t first, size_t last) {      // struct words [first, last) -> slab words from `at`
  for (size_t w = first; w < last; w++) m.slab[w] = (unsigned char)at++;
  return at;
}
constexpr CtxMap ctx_make_map() {
  CtxMap m{};
  int at = ctx_map_run(m, CTXR_ITER, CO_SV, CO_SV + CW_SV_ITER);
  m.end[0] = at;
  at = ctx_map_run(m, CTXR_COMMON, CO_EBM + EBM_W_FEED, CO_EBM + EBM_W_TSNOW);
  at = ctx_map_run(m, at, CO_EBM + EBM_W_RA1, CO_EBM + EBM_W_RA1 + 1);
  at = ctx_map_run(m, at, CO_EBC, CO_EBC + EBC_W_ALWAYS);
  m.end[1] = at;
  at = ctx_map_run(m, CTXR_CLASS, CO_EBC + EBC_W_ALWAYS, CO_EBC + EBC_W_FROZEN);
  at = ctx_map_run(m, at, CO_EBC + EBC_W_INCL, CO_EBC + EBC_W_CANOPY);
  m.end[2] = at;
  at = ctx_map_run(m, CTXR_SNOW, CO_EBC + EBC_W_FROZEN, CO_EBC + EBC_W_INCL);
  m.end[3] = at;
  at = ctx_map_run(m, CTXR_COLD, CO_SV + CW_SV_ITER, CO_SV + CW_SV);
  m.end[4] = at;
  at = ctx_map_run(m, at, CO_EBM + EBM_W_TSNOW, CO_EBM + EBM_W_TSNOW + 1);
  at = ctx_map_run(m, at, CO_EBM, CO_EBM + EBM_W_FEED);
  at = ctx_map_run(m, at, CO_EBM + EBM_W_VV, CO_EBM + CW_EBM);
  m.end[5] = at;
  return m;
}
constexpr CtxMap CTX_MAP = ctx_make_map();
constexpr bool ctx_map_is_permutation() {      // every struct word of region A has a slab word of its own
  bool used[CTXR_END] = {};
  for (size_t w = 0; w < CTX_NA; w++) {
    if (CTX_MAP.slab[w] >= CTXR_END || used[CTX_MAP.slab[w]]) return false;
    used[CTX_MAP.slab[w]] = true;
  }
  int n = 0;
  for (int i = 0; i < CTXR_END; i++) n += used[i] ? 1 : 0;
  return n == (int)CTX_NA;
}
static_assert(ctx_map_is_permutation(), "parking map of region A");
static_assert(CTXR_ITER % CTX_GROUP == 0 && CTXR_COMMON % CTX_GROUP == 0 && CTXR_CLASS % CTX_GROUP == 0 && CTXR_SNOW % CTX_GROUP == 0
              && CTXR_COLD % CTX_GROUP == 0 && CTXR_END % CTX_GROUP == 0, "every range of the parking map starts on a sector boundary");
static_assert(CTX_MAP.end[0] == CTXR_COMMON && CTX_MAP.end[1] <= CTXR_CLASS && CTX_MAP.end[2] <= CTXR_SNOW && CTX_MAP.end[3] <= CTXR_COLD
              && CTX_MAP.end[4] <= CTXR_COLD + CTX_GROUP && CTX_MAP.end[5] <= CTXR_END && CTXR_END - CTX_MAP.end[5] < CTX_GROUP,
              "ranges of the parking map; the tail of SurfSolve, which every evaluation fetches, in one sector");
static_assert(CTX_MAP.end[1] - CTXR_COMMON == 31 && CTX_MAP.end[2] - CTXR_CLASS == 13,
              "the iteration's inputs: 4 sectors for every class, 2 more for frozen soil / evaporation / canopy");
// Slab word S of HRU g: region A [hru / 64][S / G][hru % 64][G], then region B the same with G_B and W - CTX_NA
constexpr size_t CTX_NA_PAD = CTXR_END;
constexpr size_t ctx_padded_words(size_t words) {      // slab words per lane
  return CTX_NA_PAD + ((words > CTX_NA ? words - CTX_NA : 0) + CTX_GROUP_B - 1) / CTX_GROUP_B * CTX_GROUP_B;
}
struct CtxRef {
  unsigned long long* p;    // word 0 of this HRU's wave slab
  int lane;
  VIC_DEV static CtxRef at(unsigned long long* base, size_t words_per_hru, size_t g) {
    return CtxRef{base + (g >> 6) * (ctx_padded_words(words_per_hru) * 64), (int)(g & 63)};
  }
  VIC_DEV unsigned long long* word(size_t W) const {
    if (W < CTX_NA) {
      const size_t S = CTX_MAP.slab[W];
      return p + (S / CTX_GROUP) * (64 * CTX_GROUP) + lane * CTX_GROUP + (S % CTX_GROUP);
    }
    const size_t V = W - CTX_NA;
    return p + CTX_NA_PAD * 64 + (V / CTX_GROUP_B) * (64 * CTX_GROUP_B) + lane * CTX_GROUP_B + (V % CTX_GROUP_B);
  }
};
template <class T>
VIC_DEV void ctx_put(const CtxRef& r, size_t word0, const T& v) {
  static_assert(sizeof(T) % 8 == 0 && std::is_trivially_copyable<T>::value, "context structs are arrays of 8-byte words");
  constexpr int NW = sizeof(T) / 8;
  unsigned long long tmp[NW];
  __builtin_memcpy(tmp, &v, sizeof(T));
#pragma unroll
  for (int i = 0; i < NW; i++) *r.word(word0 + i) = tmp[i];
}
template <class T>
VIC_DEV void ctx_get(const CtxRef& r, size_t word0, T& v) {
  static_assert(sizeof(T) % 8 == 0 && std::is_trivially_copyable<T>::value, "context structs are arrays of 8-byte words");
  constexpr int NW = sizeof(T) / 8;
  unsigned long long tmp[NW];
#pragma unroll
  for (int i = 0; i < NW; i++) tmp[i] = *r.word(word0 + i);
  __builtin_memcpy(&v, tmp, sizeof(T));
}

template <class T>
VIC_DEV void ctx_put_words(const CtxRef& r, size_t word0, const T& v, int first, int last) {
  constexpr int NW = sizeof(T) / 8;
#pragma unroll
  for (int i = 0; i < NW; i++)
    if (i >= first && i < last) {
      unsigned long long w;
      __builtin_memcpy(&w, reinterpret_cast<const char*>(&v) + 8 * i, 8);
      *r.word(word0 + i) = w;
    }
}
// word by word into the object (no whole-struct copy: the conditional group loads of the evaluation kernel must not make the
// struct an aggregate the optimiser keeps in memory)
template <class T>
VIC_DEV void ctx_get_words(const CtxRef& r, size_t word0, T& v, int first, int last) {
  constexpr int NW = sizeof(T) / 8;
#pragma unroll
  for (int i = 0; i < NW; i++)
    if (i >= first && i < last) {
      const unsigned long long w = *r.word(word0 + i);
      __builtin_memcpy(reinterpret_cast<char*>(&v) + 8 * i, &w, 8);
    }
}

// The residual's inputs, group by group: `cls` = EBG_* bits of the HRU's root find (which groups its evaluations use)
VIC_DEV int surf_eb_class(const SurfEBConst& c) {
  return (c.frozen_on ? EBG_FROZEN : 0) | ((c.snow_coverage > 0 && !c.INCLUDE_SNOW) ? EBG_SNOWCOV : 0) | (c.INCLUDE_SNOW ? EBG_INCL : 0)
         | (!c.SNOWING ? EBG_EVAP : 0) | ((c.VEG && !c.SNOWING) ? EBG_CANOPY : 0);
}
VIC_DEV void ebc_put(const CtxRef& cx, const SurfEBConst& c, int cls) {
  ctx_put_words(cx, CO_EBC, c, 0, EBC_W_ALWAYS);
  if (cls & EBG_FROZEN) ctx_put_words(cx, CO_EBC, c, EBC_W_ALWAYS, EBC_W_FROZEN);
  if (cls & EBG_SNOWCOV) ctx_put_words(cx, CO_EBC, c, EBC_W_FROZEN, EBC_W_SNOWCOV);
  if (cls & EBG_INCL) ctx_put_words(cx, CO_EBC, c, EBC_W_SNOWCOV, EBC_W_INCL);
  if (cls & EBG_EVAP) ctx_put_words(cx, CO_EBC, c, EBC_W_INCL, EBC_W_EVAP);
  if (cls & EBG_CANOPY) ctx_put_words(cx, CO_EBC, c, EBC_W_EVAP, EBC_W_CANOPY);
}
VIC_DEV void ebc_get(const CtxRef& cx, SurfEBConst& c, int cls) {
  ctx_get_words(cx, CO_EBC, c, 0, EBC_W_ALWAYS);
  if (cls & EBG_FROZEN) ctx_get_words(cx, CO_EBC, c, EBC_W_ALWAYS, EBC_W_FROZEN);
  if (cls & EBG_SNOWCOV) ctx_get_words(cx, CO_EBC, c, EBC_W_FROZEN, EBC_W_SNOWCOV);
  if (cls & EBG_INCL) ctx_get_words(cx, CO_EBC, c, EBC_W_SNOWCOV, EBC_W_INCL);
  if (cls & EBG_EVAP) ctx_get_words(cx, CO_EBC, c, EBC_W_INCL, EBC_W_EVAP);
  if (cls & EBG_CANOPY) ctx_get_words(cx, CO_EBC, c, EBC_W_EVAP, EBC_W_CANOPY);
}
