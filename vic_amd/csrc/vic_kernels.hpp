// vic_kernels.hpp — the step kernels (device only, gfx950).
//
//   vic_hru_step<NN>   one lane per HRU: the per-HRU body of full_energy (full_energy.c:216-456) = aerodynamics,
//                      prepare_full_energy, surface_fluxes (snow, ground energy balance, pot. evap), runoff.
//                      HBM-side it is a streaming read-modify-write of the SoA state table; all physics is fp64 VALU.
//   vic_fd_stage<NN>   the same step for the finite-difference soil profile (FROZEN_SOIL / QUICK_FLUX off), cut at the
//                      ground-surface root finder into a pipeline: stage kernel (everything around the root finder, context
//                      parked in HBM, vic_ctx.hpp) -> rounds of { profile solves on a compacted work list (vic_profile.hpp,
//   vic_surf_eval      vic_implicit.hpp) ; residual + Brent step on Tsurf } -> stage kernel.  See vic_profile.hpp for why.
// hru_prologue / hru_epilogue are the parts the monolithic kernel and the stage kernel share.
#pragma once
#include <cstddef>
#include "vic_glacier.hpp"
#include "vic_profile.hpp"
#include "vic_implicit.hpp"
#include "vic_ctx.hpp"
#include "vic_hru_io.hpp"

using namespace vic;

// full_energy.c:216-354: state in, prepare_full_energy, aerodynamic resistances.  Returns the error bits.
template <int NN, bool GLAC>
VIC_DEV int hru_prologue(const KArgs& a, int g, const HruId& id, const CellView& cv, const VegLib& vl, const Forcing& fc, const Soil3& s3,
                         HruWork<NN>& w, StepConst& C, bool node_props = true) {
  const Opt& o = a.o;
  const size_t nh = a.nhru;
  const int month = a.dmy.month;
  const int veg_idx = id.veg_idx;
  int err = 0;
  C.veg_idx = veg_idx; C.band = id.band; C.is_art_bare = id.is_art_bare ? 1 : 0;
#pragma unroll
  for (int l = 0; l < 3; l++) C.root[l] = (double)(float)a.hpd[(size_t)(HPD_ROOT0 + l) * nh + g];
  if (o.BLOWING) {
    C.sigma_slope = (double)(float)a.hpd[(size_t)HPD_SIGMA_SLOPE * nh + g]; C.lag_one = (double)(float)a.hpd[(size_t)HPD_LAG_ONE * nh + g];
    C.fetch = (double)(float)a.hpd[(size_t)HPD_FETCH * nh + g];
  } else { C.sigma_slope = 0; C.lag_one = 0; C.fetch = 0; }
  load_state<NN>(a, g, w, node_props);
  w.snow.vapor_flux = 0.; w.snow.canopy_vapor_flux = 0.;                  // full_energy.c:261-262

  const double wind_h = vl.f(veg_idx, VL_WIND_H);
  const double lai_cur = vl.f(veg_idx, VL_LAI + month - 1);
  C.surf_atten = exp(-vl.f(veg_idx, VL_RAD_ATTEN) * lai_cur);   // full_energy.c:282

  // prepare_full_energy.c:8-94
  C.moist0 = w.moist[0] / (s3.depth[0] * 1000.); C.ice0 = 0.;
  if (o.FROZEN_SOIL && cv.s(CP_FS_ACTIVE) != 0.0) {
    const double tm = (w.nd.T[0] + w.nd.T[1]) / 2.;
    if (tm < 0.) {
      C.ice0 = C.moist0 - maximum_unfrozen_water(tm, s3.max_moist[0] / (s3.depth[0] * 1000.), cv.lay(CPL_BUBBLE, 0), cv.lay(CPL_EXPT, 0));
      if (C.ice0 < 0.) C.ice0 = 0.;
    }
  }
  top_layer_thermal_properties(cv, s3, w.moist, w.ice, w.so.kappa, w.so.Cs);
  C.bare_albedo = GLAC ? cv.s(CP_GLAC_ALBEDO) : vl.f(veg_idx, VL_ALBEDO + month - 1);

  // aerodynamic resistances for the 6 PET surfaces and the current vegetation (full_energy.c:302-354).  The loop is
  // kept rolled (7 x CalcAerodynamic); what it indexes by p lives in locals, not in C (see vsel()).
  Vc Ra, U, disp, zref, z0, ap[NPET];
#pragma unroll
  for (int k = 0; k < NCASE; k++) { disp.v[k] = NAN; zref.v[k] = NAN; z0.v[k] = NAN; U.v[k] = NAN; Ra.v[k] = NAN; }
#pragma unroll
  for (int q = 0; q < NPET; q++) {
#pragma unroll
    for (int k = 0; k < NCASE; k++) ap[q].v[k] = NAN;
  }
  bool overstory = false;
  const double rough = cv.s(CP_ROUGH), snow_rough = cv.s(CP_SNOW_ROUGH), wind = fc.v(VIC_F_WIND, o.NR);
#pragma unroll 1
  for (int p = 0; p < NPET + 1; p++) {
    const int pet_idx = (p < NPET_NON_NAT) ? o.nveg_types + p : veg_idx;
    if (pet_idx == o.GLACIER_ID) z0.v[SNOW_FREE] = cv.s(CP_GLAC_ROUGH);      // sic: library index compared with a class id
    else z0.v[SNOW_FREE] = vl.f(pet_idx, VL_ROUGHNESS + month - 1);
    disp.v[SNOW_FREE] = vl.f(pet_idx, VL_DISPLACEMENT + month - 1);
    overstory = vl.f(pet_idx, VL_OVERSTORY) != 0.0;
    if (p >= NPET_NON_NAT && z0.v[SNOW_FREE] == 0) z0.v[SNOW_FREE] = rough;
    const double height = calc_veg_height(disp.v[SNOW_FREE], lai_cur);
    if (disp.v[SNOW_FREE] < wind_h) zref.v[SNOW_FREE] = wind_h;
    else zref.v[SNOW_FREE] = disp.v[SNOW_FREE] + wind_h + z0.v[SNOW_FREE];
    const double wind_corr = log((zref.v[SNOW_FREE] - 0.) / rough) / log((o.wind_h - 0.) / rough);
    U.v[SNOW_FREE] = wind * wind_corr;
    U.v[CANOPY] = NAN; U.v[SNOW_COVERED] = NAN; U.v[GLACIER_SURF] = NAN;
#pragma unroll
    for (int k = 0; k < NCASE; k++) Ra.v[k] = NAN;
    if (!calc_aerodynamic(overstory, height, vl.f(pet_idx, VL_TRUNK_RATIO), snow_rough, rough, vl.f(pet_idx, VL_WIND_ATTEN), Ra, U,
                          disp, zref, z0))
      err |= VICGPU_CELLERR_AERO;
    // ap[p] = Ra without a run-time index: hipcc 7.2's alloca-to-vector promotion mis-generated the dynamically indexed
    // store of this 24-double array in several builds of vic_hru_step; a select per slot also keeps ap in
    // registers by construction
#pragma unroll
    for (int q = 0; q < NPET; q++) {
#pragma unroll
      for (int k = 0; k < NCASE; k++) ap[q].v[k] = (p == q) ? Ra.v[k] : ap[q].v[k];
    }
  }
#pragma unroll
  for (int p = 0; p < NPET; p++) C.aero_pet[p] = ap[p];
  C.Ra = Ra; C.U = U; C.disp = disp; C.zref = zref; C.z0 = z0;
  C.overstory = overstory ? 1 : 0;
  w.aero_resist_surface = Ra.v[SNOW_FREE];
  w.aero_resist_overstory = Ra.v[CANOPY];
#pragma unroll
  for (int p = 0; p < NPET; p++) w.pot_evap[p] = 0;
  return err;
}

// full_energy.c:437-455 and state / flux out
template <int NN>
VIC_DEV void hru_epilogue(const KArgs& a, int g, const CellView& cv, const Soil3& s3, const StepConst& C, HruWork<NN>& w, int err, bool glac) {
  // root zone moisture and wetness (full_energy.c:437-455)
  w.rootmoist = 0; w.wetness = 0;
#pragma unroll
  for (int l = 0; l < 3; l++) {
    if (C.root[l] > 0) w.rootmoist += w.moist[l];
    w.wetness += (w.moist[l] - s3.Wpwp[l]) / (cv.lay(CPL_POROSITY, l) * s3.depth[l] * 1000 - s3.Wpwp[l]);
  }
  w.wetness /= 3;

  bool finite = true;
#pragma unroll
  for (int l = 0; l < 3; l++) finite = finite && isfinite(w.moist[l]);
  finite = finite && isfinite(w.nd.T[0]) && isfinite(w.snow.swq);
  if (!finite) err |= VICGPU_CELLERR_NAN;

  PROF_T0(t_store);
  store_state<NN>(a, g, w);
  store_flux<NN>(a, g, w, glac);
  a.hru_err[g] = err;
  PROF_ADD(8, t_store);
}

// The whole HRU step in one lane: glacier HRUs (GLAC) and QUICK_FLUX (no soil-profile solve)
template <int NN, bool GLAC>
__global__ __launch_bounds__(64) void vic_hru_step(const KArgs a) {
  const int gi = a.map.index(blockIdx.x, threadIdx.x, a.gcount);
  if (gi < 0) return;
  const int g = a.glist ? a.glist[gi] : gi;
  const Opt& o = a.o;
  const HruId id = hru_id(a, g);
  // an invalid cell (vicNl.c:521): nothing of its HRUs is read or written, not even the zero record.  The lanes of a wave are
  // consecutive cells of one slot: one coalesced int row; without a table the branch is wave-uniform
  if (a.valid && a.valid[id.c] != CELL_VALID) return;
  // two instantiations share this body: GLAC = false handles ordinary HRUs (and writes the zero record of inactive
  // ones), GLAC = true handles glacier HRUs; the domain numbering keeps either kind wave-uniform
  if (id.is_glacier != GLAC && id.run) return;
  if (!id.run) {
    if (!GLAC) store_zero_record(a, g);
    return;
  }
  PROF_T0(t_kernel);
  CellView cv{a.cell_params, a.ncell, id.c, o.Nnode, o.Nband};
  VegLib vl{a.veglib};
  Forcing fc{a.forcing, a.snowflag, a.ncell, id.c, o.NR + 1, a.fcol[g], a.ncol};
  const Soil3 s3 = load_soil3(cv);
  HruWork<NN> w;
  StepConst C;
  int err = hru_prologue<NN, GLAC>(a, g, id, cv, vl, fc, s3, w, C);
  PROF_ADD(1, t_kernel);

  if (!(err & VICGPU_CELLERR_AERO)) {
    bool ok;
    if constexpr (GLAC) {
      GlacEnergy ge;
      double nlu, nsu, sui;
      const double blow[4] = {C.sigma_slope, C.lag_one, C.fetch, (double)C.is_art_bare};
      ok = surface_fluxes_glac<NN>(o, cv, vl, s3, fc, a.dmy, C.veg_idx, C.band, C.bare_albedo, C.aero_pet, C.Ra, C.U, C.zref, C.z0, C.disp, blow, w, w.gl,
                                   w.so.NetLongUnder, ge, nlu, nsu, sui);
      // hru.energy = step_energy + step averages (surface_fluxes_glac.c:485-526)
      SoilEnergy& so = w.so; SnowEnergy& se = w.se;
      so.snow_flux = ge.snow_flux; so.grnd_flux = ge.grnd_flux; so.deltaH = 0; so.fusion = 0; so.LongUnderOut = ge.LongUnderOut;
      so.AlbedoUnder = ge.AlbedoUnder; so.advected_sensible = ge.advected_sensible; so.advection = ge.advection;
      so.deltaCC = ge.deltaCC; so.refreeze_energy = ge.refreeze_energy; so.error = ge.error; so.latent = ge.latent;
      so.latent_sub = ge.latent_sub; so.sensible = ge.sensible; so.NetLongUnder = nlu; so.NetShortUnder = nsu; so.NetShortGrnd = 0;
      se.canopy_advection = 0; se.canopy_latent = 0; se.canopy_latent_sub = 0; se.canopy_sensible = 0; se.canopy_refreeze = 0;
      w.AlbedoOver_avg = 0; w.LongOverIn_avg = 0; w.NetLongOver_avg = 0; w.NetShortOver_avg = 0; w.ShortOverIn_avg = 0;
      w.ShortUnderIn_avg = sui;
      w.deltaCC_glac = ge.deltaCC_glac; w.glacier_flux = ge.glacier_flux; w.glacier_melt_energy = ge.glacier_melt_energy;
      // accumulateGlacierMassBalance.c:13-67: the per-step += (the accumulation-window decision is driver state: the
      // host makes cum_mass_balance valid when the window opens)
      if (!isnan(w.gl.cum_mass_balance) && !isnan(w.gl.mass_balance)) w.gl.cum_mass_balance += w.gl.mass_balance;
    } else {
      ok = surface_fluxes<NN>(o, cv, vl, s3, fc, a.dmy, C, w);
    }
    if (!ok) err |= VICGPU_CELLERR_SOLVER;
  }
  hru_epilogue<NN>(a, g, cv, s3, C, w, err, GLAC);
  PROF_ADD(0, t_kernel);
  PROF_WAVE(0);
  PROF_LANE(1);
}

// Finite-difference pipeline, stage kernel: phase 0 starts the step of every ordinary HRU; phase p >= 1 resumes the
// HRUs whose ground-surface root of sub-step p - 1 has been found.  Either way an HRU leaves with its next sub-step
// set up and parked (appended to the work list) or with its step finished and stored.
// FIRST: the phase-0 instantiation; MULTI: the run has more than one snow sub-step per step (otherwise phase 1 never sets up
// another sub-step and that code is not instantiated).
template <int NN, bool FIRST, bool MULTI>
__global__ __launch_bounds__(64) VIC_WAVES_PER_EU(1, 1) void vic_fd_stage(const KArgs a) {
  const int gi = a.map.index(blockIdx.x, threadIdx.x, a.gcount);
  if (gi < 0) return;
  const int g = a.glist ? a.glist[gi] : gi;
  const Opt& o = a.o;
  const HruId id = hru_id(a, g);
  if (id.run && id.is_glacier) return;              // vic_hru_step<NN, true> owns glacier HRUs
  // an invalid cell (vicNl.c:521): its HRUs stay idle for the whole step -- no zero record, no work list, no round; the later
  // phases and the evaluation kernel pass them by on hstate
  if (FIRST && a.valid && a.valid[id.c] != CELL_VALID) { a.hstate[g] = 0; return; }
  if (FIRST && !id.run) { store_zero_record(a, g); a.hstate[g] = 0; return; }
  if (!FIRST && (a.hstate[g] & HS_STATE) != 2) return;
  CellView cv{a.cell_params, a.ncell, id.c, o.Nnode, o.Nband};
  VegLib vl{a.veglib};
  Forcing fc{a.forcing, a.snowflag, a.ncell, id.c, o.NR + 1, a.fcol[g], a.ncol};
  const Soil3 s3 = load_soil3(cv);
  const int Nn = node_count<NN>(o.Nnode);
  const CtxRef cx = CtxRef::at(a.ctx, ctx_words<NN>(), g);
  HruWork<NN> w;
  StepConst C;
  SubLoop L;
  int err = 0;
  bool more;
  PROF_T0(t_stage);
  if constexpr (FIRST) {
    err = hru_prologue<NN, false>(a, g, id, cv, vl, fc, s3, w, C, /*node_props=*/false);
    PROF_ADD(1, t_stage);
    more = !(err & VICGPU_CELLERR_AERO);
    if (more) sf_begin<NN>(o, fc, C, w, L);
  } else {
    SubStep P;
    SurfEB eb;
    SurfSolve sv;
    ctx_get_words(cx, CO_SV, sv, (int)CW_SV_ITER, (int)CW_SV);                     // the result of the root find, not the Brent state
    ctx_get(cx, CO_EBM, static_cast<SurfEBMut&>(eb));
    ctx_get_words(cx, CO_EBC, static_cast<SurfEBConst&>(eb), 0, EBC_W_POST);      // the bookkeeping reads the flags and T2 only
    surf_cell_fill(eb, cv, vl, s3, fc, eb.hidx, id.veg_idx, a.dmy.month);
    ctx_get(cx, CO_P, P);
    ctx_get_words(cx, CO_L, L, 0, (int)CW_L_HEAD);
    if (MULTI && L.N_steps > 0) ctx_get_words(cx, CO_L, L, (int)CW_L_HEAD, (int)CW_L);
    else zero_substep_sums(L);
    load_untouched_state<NN>(a, g, w);
    if constexpr (MULTI) {
      ctx_get(cx, CO_C, C);
      WCarryMulti<NN> km;
      ctx_get(cx, CO_WM, km);
      carry_in_multi<NN>(km, w);
    } else {
      // one sub-step per step: of StepConst the bookkeeping needs the PET resistances of this sub-step's surface cases (parked),
      // the rest is in the HRU tables
      StepConstPost q;
      ctx_get(cx, CO_C, q);
      step_const_post_in(q, P.UnderStory, C);
      C.veg_idx = id.veg_idx; C.band = id.band; C.is_art_bare = id.is_art_bare ? 1 : 0;
      C.overstory = (vl.f(id.veg_idx, VL_OVERSTORY) != 0.0) ? 1 : 0;
#pragma unroll
      for (int l = 0; l < 3; l++) C.root[l] = (double)(float)a.hpd[(size_t)(HPD_ROOT0 + l) * a.nhru + g];
    }
    {
      WCarry k;
      ctx_get(cx, CO_W, k);
      carry_in<NN>(k, w);
    }
    PROF_ADD(11, t_stage);
    PROF_T0(t_post);
    // the soil profile of the final evaluation
    const double* __restrict__ po = pout_rec(static_cast<const double*>(a.pout), (size_t)g, Nn, sv.final_slot);
    const int* __restrict__ poc = reinterpret_cast<const int*>(po + rec_cnt(Nn));
    double Tprof[NN];
    int cntprof[NN];
    const unsigned long long flags = (unsigned long long)__double_as_longlong(po[rec_flag()]);
#pragma unroll
    for (int n = 0; n < NN; n++) {
      Tprof[n] = (n < Nn) ? po[rec_t(n)] : 0.0;
      cntprof[n] = (n < Nn) ? poc[n] : 0;
    }
    using mask_t = typename NodeBound<NN>::mask_t;      // the flag bits below the record's ok bit
    sf_sub_post<NN>(o, cv, vl, s3, fc, a.dmy, C, w, L, P, eb, sv, Tprof, cntprof,
                    (mask_t)(flags & ((1ull << NodeBound<NN>::ok_bit) - 1ull)));
    PROF_ADD(12, t_post);
    more = true;
  }
  bool pend = false;
  int key = 0;
  if ((FIRST || MULTI) && more && L.hidx < L.endhidx) {
    if constexpr (FIRST || MULTI) {
      SubStep P;
      SurfEB eb;
      SurfSolve sv;
      PROF_T0(t_pre);
      sf_sub_pre<NN>(o, cv, vl, s3, fc, a.dmy, C, w, L, P, eb, sv);
      PROF_ADD(13, t_pre);
      PROF_T0(t_put);
      ctx_put(cx, CO_SV, sv);
      ctx_put_words(cx, CO_EBM, static_cast<const SurfEBMut&>(eb), 0, EBM_W_KEEP);   // the outputs are the final evaluation's to write
      const int cls = surf_eb_class(eb);
      ebc_put(cx, eb, cls);
      ctx_put(cx, CO_P, P);
      ctx_put_words(cx, CO_L, L, 0, (int)CW_L_HEAD);
      if (MULTI && L.N_steps > 0) ctx_put_words(cx, CO_L, L, (int)CW_L_HEAD, (int)CW_L);
      if constexpr (MULTI) {
        if (FIRST) ctx_put(cx, CO_C, C);
        WCarryMulti<NN> km;
        carry_out_multi<NN>(w, km);
        ctx_put(cx, CO_WM, km);
      } else {
        StepConstPost q;
        step_const_post_out(C, P.UnderStory, q);
        ctx_put(cx, CO_C, q);
      }
      {
        WCarry k;
        carry_out<NN>(w, k);
        ctx_put(cx, CO_W, k);
      }
      // the item block needs the node rows that nothing before it reads: loaded last, so that they are not live (and
      // spilled) across solve_snow
      load_node_props<NN>(a, g, w.nd);
      {
        // Key = number of frozen nodes, plus a second set of segments for HRUs with a node whose Brent bracket
        // T0 +- SOIL_DT contains 0 C: the residual has a kink there (ice vanishes), Brent degrades to bisection and needs
        // 17-28 evaluations instead of 6-11 -- 1.5 % of the node solves, but one such lane holds up its whole wave.
        // (Finer keys -- frozen range, thawed top -- and the measured trip count were tried: no better.)
        int nfrozen = 0;
        bool kink = false;
#pragma unroll
        for (int n = 1; n < NN; n++)
          if (n < Nn && eb.frozen_on) {
            if (w.nd.T[n] < 0) nfrozen++;
            if (fabs(w.nd.T[n]) < SOIL_DT) kink = true;
          }
        if constexpr (NN >= NBUCKET / 2) nfrozen = (nfrozen < NBUCKET / 2 - 1) ? nfrozen : NBUCKET / 2 - 1;    // deep bound: 25+ share the top segment
        key = nfrozen + (kink ? NBUCKET / 2 : 0);
        a.hkey[g] = key;
      }
      profile_item_store<NN>(o, cv, s3, w.nd, eb.delta_t, eb.frozen_on != 0, item_block(a.pin, (size_t)g, Nn));
      if (o.IMPLICIT) {
        double* __restrict__ im = a.pimp + (size_t)g * Nn * PIMP;
#pragma unroll
        for (int n = 0; n < NN; n++)
          if (n < Nn) {
            im[n * PIMP + PI_MOIST] = w.nd.moist[n]; im[n * PIMP + PI_ICE] = (n == 0) ? eb.delta_t : w.nd.ice[n];
            im[n * PIMP + PI_KAPPA] = w.nd.kappa[n]; im[n * PIMP + PI_CS] = w.nd.Cs[n];
          }
        a.lastexp[g] = -1;
      }
      a.ts[g] = sv.x;
      a.pslot[g] = 0;
      if (o.QUICK_SOLVE) {
        // calc_surf_energy_bal.c:289-299: the iteration solves the nodes down to the thaw depth + 4 only
        int tmpNnodes = 0;
#pragma unroll
        for (int n = NN - 1; n >= 0; n--)
          if (n <= Nn - 5 && w.nd.T[n] >= 0 && w.nd.T[(n + 1 < NN) ? n + 1 : n] < 0) tmpNnodes = n + 1;
        if (tmpNnodes == 0) tmpNnodes = (w.nd.T[0] <= 0 && w.nd.T[1] >= 0) ? Nn : 3;
        else tmpNnodes += 4;
        // (the iteration runs with NOFLUX forced off, calc_surf_energy_bal.c:298; without an iteration -- no FULL_ENERGY -- the
        // run's own NOFLUX decides whether the bottom node is solved)
        a.jl[g] = (sv.stage == SurfSolve::ROOT_QUICK) ? tmpNnodes - 1 : (o.NOFLUX ? Nn : Nn - 1);
      }
      pout_rec(a.pout, (size_t)g, Nn, 0)[rec_key()] = NAN;      // no solve on record yet
      pout_rec(a.pout, (size_t)g, Nn, 1)[rec_key()] = NAN;
      a.hstate[g] = 1 | (cls << HS_CLS_SHIFT);
      pend = true;
      PROF_ADD(14, t_put);
    }
  } else {
    PROF_T0(t_end);
    if (more && !sf_end<NN>(o, cv, s3, C, w, L)) err |= VICGPU_CELLERR_SOLVER;
    PROF_ADD(15, t_end);
    hru_epilogue<NN>(a, g, cv, s3, C, w, err, false);
    a.hstate[g] = 0;
  }
  list_append(a.list, a.count, a.list_cap, pend, key, g);
  PROF_ADD(0, t_stage);
  PROF_WAVE(0);
  PROF_LANE(1);
}

// Finite-difference pipeline, evaluation kernel: the residual of the ground-surface energy balance at the trial
// temperature whose soil profile has just been solved, then one step of the Brent iteration on Tsurf.
struct EArgs {
  Opt o;
  LaunchMap map;
  int ncell, nhru, Nn;
  const int* glist;
  int gcount;
  const double* cell_params;
  const int* hpi;
  unsigned long long* ctx;
  size_t ctx_words;
  double* pout;
  int* pslot;
  double* ts;
  int* jl;               // QUICK_SOLVE: [nhru] end of the column the profile kernel solves (null otherwise)
  int* hstate;
  int* list_next;        // NBUCKET segments of list_cap entries
  int* count_next;       // [NBUCKET]
  int list_cap;
  const int* hkey;
  int* profile_next;     // work-list cursor of the profile kernel, cleared for its next launch
  // every HRU the round leaves pending -- for a solve, or for an evaluation without one (final evaluation on record) -- also
  // goes on a flat list: PEND_STRIPES stripes of pend_cap entries, one chunk per wave in lane order (vic_profile.hpp)
  int* pend_list_next;
  int* pend_count_next;  // the stripes' fill counters, PEND_CNT_STRIDE apart
  int pend_cap;
  // sparse rounds (at most list_thr HRUs pending; the others go through glist / map and test hstate): lane = entry of the flat
  // list the round before has left.  -1 in the round after a stage kernel, which leaves no flat list.
  int list_thr;
  const int* pend_list_cur;
  const int* pend_prefix; // [PEND_STRIPES + 1] entries before each stripe of pend_list_cur, packed by the round's profile kernel
  const int* npend_cur;   // the number of evaluations pending, written by the round's profile kernel
  int implicit;          // IMPLICIT: the final evaluation is always solved again (its fallback flags depend on the solves before it)
  const double* veglib;  // for the table-derived part of the residual's inputs (surf_cell_fill)
  const double* forcing; // this step: [VIC_NFORCE][NF+1][ncol]
  const int* fcol;        // [nhru] forcing column of each HRU's cell (KArgs)
  int ncol;
  int month;
};

constexpr int EVAL_WAVES = 2;
__global__ __launch_bounds__(64) VIC_WAVES_PER_EU(EVAL_WAVES, EVAL_WAVES) void vic_surf_eval(const EArgs a) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *a.profile_next = 0;
  // Sparse rounds.  A dense launch pays a whole wave -- its chain of dependent loads -- for every 64 HRUs of which one is
  // pending.  The number pending is on the device before the host knows it (the flat list the round before has left), so
  // every wave looks at it: from the round in which at most list_thr HRUs are pending, lane = entry of that list and the
  // waves beyond its end leave at once.  The entry's stripe is found by bisection of the packed prefix array; 64 consecutive
  // entries of a stripe come from about 1 / (fraction pending) producing waves, so a list-formed wave reads a few context slabs.
  const int npend = *a.npend_cur;
  int g;
  if (npend <= a.list_thr) {
    if ((int)blockIdx.x * 64 >= npend) return;
    __shared__ int prefix[PEND_STRIPES + 1];
    for (int b = threadIdx.x; b < PEND_STRIPES + 1; b += 64) prefix[b] = a.pend_prefix[b];
    __syncthreads();
    const int gi = blockIdx.x * 64 + threadIdx.x;
    if (gi >= npend) return;
    int lo = 0, hi = PEND_STRIPES;             // prefix[lo] <= gi < prefix[hi]
#pragma unroll
    for (int it = 0; it < 6; it++) {
      const int mid = (lo + hi) >> 1;
      const bool up = prefix[mid] <= gi;
      lo = up ? mid : lo; hi = up ? hi : mid;
    }
    g = a.pend_list_cur[(size_t)lo * a.pend_cap + (gi - prefix[lo])];
  } else {
    const int gi = a.map.index(blockIdx.x, threadIdx.x, a.gcount);
    if (gi < 0) return;
    g = a.glist ? a.glist[gi] : gi;
  }
  const int hs = a.hstate[g];
  if ((hs & HS_STATE) != 1) return;
  const int cls = hs >> HS_CLS_SHIFT;
  const size_t nh = a.nhru;
  const int c = a.hpi[(size_t)HPI_CELL * nh + g];
  const int veg_idx = a.hpi[(size_t)HPI_VEG_INDEX * nh + g];
  const int ps = a.pslot[g];
  CellView cv{a.cell_params, a.ncell, c, a.o.Nnode, a.o.Nband};
  const Soil3 s3 = load_soil3(cv);
  SurfSolve sv;
  SurfEB eb;
  const CtxRef cx = CtxRef::at(a.ctx, a.ctx_words, g);
  ctx_get(cx, CO_SV, sv);
  ebc_get(cx, eb, cls);
  const bool is_final = sv.stage == SurfSolve::FINAL;
  // the record the profile kernel has just written, or the one found on record for the final evaluation
  const int slot = sv.on_record ? sv.final_slot : ps;
  {
    // of SurfEBMut an evaluation of the iteration reads what it cannot know otherwise; the final one reads every input, since
    // what it does not assign passes through to the bookkeeping (vic_surface.hpp)
    SurfEBMut& m = eb;
    if (is_final) ctx_get_words(cx, CO_EBM, m, 0, EBM_W_KEEP);
    else {
      if (cls & EBG_INCL) ctx_get_words(cx, CO_EBM, m, 0, EBM_W_FEED);
      ctx_get_words(cx, CO_EBM, m, EBM_W_FEED, EBM_W_IN3);
      if (cls & EBG_SNOWCOV) ctx_get_words(cx, CO_EBM, m, EBM_W_IN3, EBM_W_TSNOW);
      if (cls & EBG_CANOPY) ctx_get_words(cx, CO_EBM, m, EBM_W_RA1, EBM_W_RA1 + 1);
    }
  }
  {
    const VegLib vl{a.veglib};
    const Forcing fc{a.forcing, nullptr, a.ncell, c, a.o.NR + 1, a.fcol[g], a.ncol};
    surf_cell_fill(eb, cv, vl, s3, fc, eb.hidx, veg_idx, a.month);
  }
  // key, flags, T1 and T2 are the record's first sector (vic_layout.hpp)
  const double* __restrict__ po = pout_rec(static_cast<const double*>(a.pout), (size_t)g, a.Nn, slot);
  const bool ok = (((unsigned long long)__double_as_longlong(po[rec_flag()])) >> record_ok_bit(node_bound(a.Nn))) & 1ull;
  if (sv.stage == SurfSolve::FINAL) sv.final_slot = slot;
  const double fx = ok ? eb.eval(a.o, s3, sv.x, po[rec_t(1)], po[rec_t(2)]) : ERROR_VAL;
  const bool was_quick = sv.stage == SurfSolve::ROOT_QUICK;
  const int stage_before = sv.stage;
  const double x_eval = sv.x;
  surf_solve_consume(a.o, sv, eb, eb, fx);
  // The iteration has just ended on the point it has just evaluated (the usual end of a Brent iteration: the newest point is
  // the best one): the evaluation "at the root" the reference makes next (calc_surf_energy_bal.c:489-506) would repeat this
  // one -- same trial temperature, same profile record, and for an HRU without a thin snowpack nothing an evaluation leaves
  // behind feeds the next -- so it is booked as done here instead of in another round.  Not taken: thin snowpack (the vapour
  // fluxes are carried from call to call), fallback / error results, QUICK_SOLVE and IMPLICIT (their final evaluation solves
  // another column / is always solved again).
  bool at_root = false;
  if (stage_before == SurfSolve::ROOT && sv.stage == SurfSolve::FINAL && !a.implicit && !a.o.QUICK_SOLVE && !(cls & EBG_INCL) && sv.ok
      && sv.fbflag == 0 && sv.Tsurf == x_eval && fabs(fx) < 1.e30) {
    sv.final_slot = slot;
    surf_solve_consume(a.o, sv, eb, eb, fx);       // FINAL -> DONE with this evaluation's residual
    at_root = true;
  }
  if (was_quick && sv.stage != SurfSolve::ROOT_QUICK) {
    // QUICK_SOLVE: from here on the whole column is solved; the records of the shortened column are not its solutions.  NOFLUX
    // comes back with a second iteration only (calc_surf_energy_bal.c:403); the final evaluation keeps what was last set
    a.jl[g] = (sv.stage == SurfSolve::ROOT && a.o.NOFLUX) ? a.Nn : a.Nn - 1;
    pout_rec(a.pout, (size_t)g, a.Nn, 0)[rec_key()] = NAN;
    pout_rec(a.pout, (size_t)g, a.Nn, 1)[rec_key()] = NAN;
  }
  bool need_solve = sv.stage != SurfSolve::DONE;
  if (sv.stage == SurfSolve::FINAL && !a.implicit) {
    // the root has been found: the final evaluation needs the profile at sv.x, which is on record if sv.x is one of the
    // last two trial points; the evaluation itself happens in the next round, together with everybody else's (making it
    // here, in a second pass over eval(), costs the kernel 548 B of scratch per lane and 5 ms per step: measured, dropped)
    // (the keys are read through a.pout, as the invalidation above writes them)
    if (pout_rec(a.pout, (size_t)g, a.Nn, slot)[rec_key()] == sv.x) { sv.final_slot = slot; sv.on_record = 1; need_solve = false; }
    else if (pout_rec(a.pout, (size_t)g, a.Nn, slot ^ 1)[rec_key()] == sv.x) { sv.final_slot = slot ^ 1; sv.on_record = 1; need_solve = false; }
  }
  // while the Brent iteration goes on only its own state and the next abscissa change: the tail of SurfSolve (result,
  // flags, stage, record bookkeeping) is written when it does
  if (sv.stage == stage_before && (sv.stage == SurfSolve::ROOT || sv.stage == SurfSolve::ROOT_QUICK)) ctx_put_words(cx, CO_SV, sv, 0, (int)CW_SV_ITER);
  else ctx_put(cx, CO_SV, sv);
  if (sv.stage == SurfSolve::DONE) {
    const SurfEBMut& m = eb;
    if (at_root) {
      // an evaluation of the iteration has not fetched the inputs it only passes through: written back are the outputs and
      // what this HRU's branch of the evaluation assigns (vic_surface.hpp); the rest keeps the values the set-up parked
      ctx_put_words(cx, CO_EBM, m, EBM_W_KEEP, (int)CW_EBM);
      ctx_put_words(cx, CO_EBM, m, EBM_W_TSNOW, EBM_W_TSNOW + 1);                                   // ra_used[0]
      if (cls & EBG_FROZEN) ctx_put_words(cx, CO_EBM, m, EBM_W_IN3 - 1, EBM_W_IN3);                 // fusion
      if (cls & EBG_CANOPY) ctx_put_words(cx, CO_EBM, m, EBM_W_VV, EBM_W_VV + 6);                   // vv, layerevap[3]
      else if (cls & EBG_EVAP) ctx_put_words(cx, CO_EBM, m, EBM_W_VV + 3, EBM_W_VV + 4);            // layerevap[0] (arno_evap)
    } else ctx_put(cx, CO_EBM, m);
  } else if (cls & EBG_INCL) ctx_put_words(cx, CO_EBM, static_cast<const SurfEBMut&>(eb), 0, EBM_W_FEED);
  if (sv.stage == SurfSolve::DONE) a.hstate[g] = 2;
  else if (need_solve) { a.ts[g] = sv.x; a.pslot[g] = slot ^ 1; }     // keep the record just used, overwrite the older one
  list_append(a.list_next, a.count_next, a.list_cap, need_solve, a.hkey[g], g);
  {
    // the flat list: one chunk per wave, one atomic on the stripe's own line
    const bool pend = sv.stage != SurfSolve::DONE;
    const unsigned long long m = __ballot(pend);
    if (m != 0) {
      const int lane = (int)__lane_id(), lead = __ffsll((long long)m) - 1, stripe = blockIdx.x % PEND_STRIPES;
      int base = 0;
      if (lane == lead) base = atomicAdd(a.pend_count_next + stripe * PEND_CNT_STRIDE, __popcll(m));
      base = __shfl(base, lead);
      if (pend) a.pend_list_next[(size_t)stripe * a.pend_cap + base + __popcll(m & ((1ull << lane) - 1ull))] = g;
    }
  }
}
