/*
 * vicgpu.h — C-ABI boundary of the MI355X-native VIC hot path.
 *
 * What this replaces.  The reference (pacificclimate/VIC) has no plugin/FFI
 * interface; its seam is the body of the OpenMP loop over cells in
 * vicNl.c:514-593, i.e. per cell and per record
 *
 *     dist_prec(&cell, dmy, &filep, outputFormat, outputData, rec, FALSE, state)   vicNl.c:543
 *       -> full_energy(NEWCELL, rec, atmos, prcp, dmy, lake_con, soil_con, ...)     dist_prec.c:159, full_energy.c:8
 *            -> surface_fluxes / surface_fluxes_glac per HRU                        full_energy.c:399-424
 *
 * The entry points below are what a reference-side binding
 * calls instead of that loop body, once for ALL cells of a domain: plain
 * pointers and sizes, caller-owned host buffers, int return codes
 * (0 = ok, negative = error; VICGPU_ERR_*), never throws, never exits.  What that loop does with a cell whose step returned
 * ERROR -- cell.isValid = FALSE, the cell skipped from the next record on (vicNl.c:521, 545-559; CONTINUEONERROR) -- is
 * behind the boundary too: vicgpu_set_retire_on_error / vicgpu_set_cell_valid / vicgpu_get_cell_valid, decided on the device.
 *
 * Data contract.  Everything is struct-of-arrays ("tables"): a table is a
 * dense row-major double (or int) array [nrow][ncol] where the column is the
 * cell (or the HRU) and the row is a field listed in the enums below.  One
 * HRU = one vegetation tile in one snow band of one cell (struct HRU,
 * vicNl_def.h:1374-1388).  All arithmetic is fp64 like the reference.
 *
 * Option coverage: Nlayer = 3, DIST_PRCP = FALSE
 * (Ndist = 1, mu = 1), no lakes, no EXCESS_ICE / SPATIAL_FROST / SPATIAL_SNOW /
 * QUICK_FS / LOW_RES_MOIST / CLOSE_ENERGY (all compiled out in the reference,
 * user_def.h:36-92).  CORRPREC, BLOWING, IMPLICIT (finite-difference soil profile, node-array
 * freezing parameters: frozen_compat = 0) and QUICK_SOLVE (with NOFLUX / EXP_TRANS as the reference handles them)
 * are implemented.  Nnode runs up to the reference's MAX_NODES = 50 (kernels instantiated for 10, up to 24 and up
 * to 50 nodes); IMPLICIT up to 24.  What the device code does not implement (see vicgpu_create) is
 * REJECTED with VICGPU_ERR_UNSUPPORTED, never silently replaced.
 */
#ifndef VICGPU_H_
#define VICGPU_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VICGPU_ABI_VERSION 3

#define VIC_NLAYER        3    /* MAX_LAYERS, user_def.h:95 */
#define VIC_MAX_NODES    50    /* MAX_NODES, user_def.h:96: the largest options.Nnode (IMPLICIT: 24, see vicgpu_options) */
#define VIC_MAX_BANDS    30    /* MAX_BANDS, user_def.h:97 */
#define VIC_N_PET_TYPES   6    /* vicNl_def.h:213 */
#define VIC_MAX_ZWTVMOIST 11   /* user_def.h:100 */

/* error codes */
#define VICGPU_OK               0
#define VICGPU_ERR_ARG         -1
#define VICGPU_ERR_UNSUPPORTED -2
#define VICGPU_ERR_HIP         -3
#define VICGPU_ERR_STATE       -4
#define VICGPU_ERR_NOMEM       -5

/* option enumerations (values follow vicNl_def.h:166-210) */
#define VIC_SNOW_ALBEDO_USACE   0
#define VIC_SNOW_ALBEDO_SUN1999 1
#define VIC_DENS_BRAS   0
#define VIC_DENS_SNTHRM 1
#define VIC_AR_406      0
#define VIC_AR_406_LS   1
#define VIC_AR_406_FULL 2
#define VIC_AR_410      3
#define VIC_AR_COMBO    4
#define VIC_GF_406  0
#define VIC_GF_410  1
#define VIC_GF_FULL 2
#define VIC_NODE_SOLVER_BRENT  0
#define VIC_NODE_SOLVER_NEWTON 1
#define VIC_TEMP_TH_VIC_412 0
#define VIC_TEMP_TH_KIENZLE 1

/* Snapshot of the option_struct / global_param_struct fields the hot path reads
 * (vicNl_def.h:655-790, 854-895). */
typedef struct vicgpu_options {
  int abi_version;          /* must be VICGPU_ABI_VERSION */
  int Nlayer;               /* must be 3 */
  int Nnode;                /* 3 with QUICK_FLUX; 3 .. VIC_MAX_NODES (get_global_param.c:1193) */
  int Nband;                /* options.SNOW_BAND */
  int dt;                   /* global_param.dt, hours */
  int snow_step;            /* options.SNOW_STEP, hours (== dt when dt < 24, get_global_param.c:965) */
  int FULL_ENERGY;
  int FROZEN_SOIL;
  int QUICK_FLUX;
  int NOFLUX;
  int EXP_TRANS;
  int GRND_FLUX_TYPE;       /* VIC_GF_* */
  int TFALLBACK;
  int AERO_RESIST_CANSNOW;  /* VIC_AR_* */
  int SNOW_ALBEDO;
  int SNOW_DENSITY;
  int TEMP_TH_TYPE;
  int GLACIER_ID;           /* veg_class number of the glacier class, -1 = none */
  int GLACIER_DYNAMICS;
  int frozen_compat;        /* 1 = reproduce frozen_soil.c:218-221 (layer arrays indexed by node,
                               SURVEY.md Finding 1.2); 0 = node arrays ("fixed") */
  int nveg_types;           /* veg_lib[0].NVegLibTypes; the table holds nveg_types + 4 rows */
  int CORRPREC;             /* gauge-undercatch correction of precipitation (correct_precip.c, full_energy.c:188-194) */
  int IMPLICIT;             /* options.IMPLICIT: Newton-Raphson soil heat solver (frozen_soil.c:229-301, newt_raph_func_fast.c),
                               the explicit solver as its fallback; rejected with QUICK_FLUX, frozen_compat or Nnode > 24
                               (the reference's own limit is 21 nodes: MAXSIZE 20, newt_raph_func_fast.c:7) */
  int BLOWING;              /* options.BLOWING: sublimation from blowing snow (CalcBlowingSnow.c), once per snow sub-step */
  int QUICK_SOLVE;          /* options.QUICK_SOLVE (calc_surf_energy_bal.c:289-314, 400-475): ignored with QUICK_FLUX (as in the
                               reference); the iteration runs with NOFLUX and EXP_TRANS forced off, NOFLUX comes back with a second
                               iteration only, EXP_TRANS never (calc_surf_energy_bal.c:298-308, 403); rejected together with IMPLICIT */
  int NODE_SOLVER;          /* VIC_NODE_SOLVER_*: how the frozen-node heat balance (soil_thermal_eqn.c) is solved -- not a
                               reference option; BRENT replays root_brent.c's iteration, NEWTON converges to the same root */
  double wind_h;            /* global_param.wind_h (m) */
  double reserved_d[3];
} vicgpu_options;

/* NF / NR as get_global_param.c:964-973 derives them */
#define VICGPU_NF(opt) ((opt)->dt / (opt)->snow_step == 1 ? 1 : (opt)->dt / (opt)->snow_step)
#define VICGPU_NR(opt) ((opt)->dt / (opt)->snow_step == 1 ? 0 : (opt)->dt / (opt)->snow_step)

/* ---------------------------------------------------------------- veg library
 * veg_lib_struct (vicNl_def.h:1034-1051): AoS table double[nveg_types+4][VL_NFIELD];
 * the last 4 rows are the reference PET surfaces read_veglib.c:118-136 appends. */
enum {
  VL_OVERSTORY = 0, VL_RARC, VL_RMIN, VL_RAD_ATTEN, VL_TRUNK_RATIO, VL_WIND_ATTEN,
  VL_WIND_H, VL_RGL, VL_VEG_CLASS,
  VL_LAI = 9,            /* 12 monthly values each from here on */
  VL_WDMAX = 21,
  VL_ALBEDO = 33,
  VL_DISPLACEMENT = 45,
  VL_EMISSIVITY = 57,
  VL_ROUGHNESS = 69,
  VL_NFIELD = 81
};

/* ---------------------------------------------------------------- forcing
 * atmos_data_struct (vicNl_def.h:1060-1076).  Units as inside the reference's
 * time loop: T in C, prec mm/step, pressure/vp/vpd in Pa, W/m2, kg/m3, m/s.
 * Layout double[nsteps][VIC_NFORCE][NF+1][ncell]; sub-index NR holds the
 * step average, 0..NF-1 the snow sub-steps.  snowflag uint8[nsteps][NF+1][ncell].  With a forcing map
 * (vicgpu_set_forcing_map) the forcing and raw tables are ncol wide, the flags stay ncell wide. */
enum {
  VIC_F_AIR_TEMP = 0, VIC_F_PREC, VIC_F_PRESSURE, VIC_F_VP, VIC_F_VPD,
  VIC_F_DENSITY, VIC_F_SHORTWAVE, VIC_F_LONGWAVE, VIC_F_WIND, VIC_NFORCE
};

/* The same forcing as the forcing files hold it, hour by hour, before initialize_atmos.c derives atmos[rec] from it:
 * double[nsteps][VIC_NRAW][dt][ncell] (dt = hours per model step), pressure and vapour pressure in kPa
 * (initialize_atmos.c:290-295).  vicgpu_prefetch_forcing_raw derives the table above from it on the device. */
enum {
  VIC_RAW_AIR_TEMP = 0, VIC_RAW_PREC, VIC_RAW_PRESSURE_KPA, VIC_RAW_VP_KPA, VIC_RAW_SHORTWAVE, VIC_RAW_LONGWAVE, VIC_RAW_WIND,
  VIC_NRAW
};

/* dmy_struct (vicNl_def.h:1082-1088): int[nsteps][VIC_NDMY] */
enum { VIC_DMY_MONTH = 0, VIC_DMY_DAY_IN_YEAR, VIC_DMY_HOUR, VIC_DMY_DAY, VIC_DMY_YEAR, VIC_NDMY };

/* ---------------------------------------------------------------- cell parameters
 * soil_con_struct (vicNl_def.h:900-999) fields read by the path.
 * Table double[VICGPU_CP_NROW(Nnode,Nband)][ncell]. */
enum {
  CP_DS = 0, CP_DSMAX, CP_WS, CP_C, CP_B_INFILT, CP_DP, CP_AVG_TEMP, CP_ROUGH, CP_SNOW_ROUGH,
  CP_ELEVATION, CP_LAT, CP_FS_ACTIVE,
  CP_NEW_SNOW_ALB, CP_SNOW_ALB_ACCUM_A, CP_SNOW_ALB_ACCUM_B, CP_SNOW_ALB_THAW_A, CP_SNOW_ALB_THAW_B,
  CP_MIN_RAIN_TEMP, CP_MAX_SNOW_TEMP, CP_PADJ_R, CP_PADJ_S,
  CP_GLAC_SURF_THICK, CP_GLAC_SURF_WE, CP_GLAC_KMIN, CP_GLAC_DK, CP_GLAC_A, CP_GLAC_ALBEDO, CP_GLAC_ROUGH,
  CP_NSCALAR
};
/* per-layer fields (x VIC_NLAYER) */
enum {
  CPL_KSAT = 0, CPL_WCR, CPL_WPWP, CPL_EXPT, CPL_BUBBLE, CPL_DEPTH, CPL_MAX_MOIST, CPL_RESID_MOIST,
  CPL_POROSITY, CPL_QUARTZ, CPL_ORGANIC, CPL_BULK_DENSITY, CPL_SOIL_DENSITY, CPL_BULK_DENS_MIN,
  CPL_SOIL_DENS_MIN, CPL_NFIELD
};
/* per-node fields (x Nnode) */
enum {
  CPN_ZSUM = 0, CPN_DZ, CPN_ALPHA, CPN_BETA, CPN_GAMMA, CPN_MAX_MOIST, CPN_EXPT, CPN_BUBBLE, CPN_NFIELD
};
/* per-band fields (x Nband) */
enum { CPB_AREAFRACT = 0, CPB_TFACTOR, CPB_PFACTOR, CPB_BANDELEV, CPB_ABOVETREELINE, CPB_NFIELD };
/* water-table curves zwtvmoist_zwt / zwtvmoist_moist [Nlayer+2][MAX_ZWTVMOIST] (vicNl_def.h:965-966) */
#define VIC_NZWT_ROWS ((VIC_NLAYER + 2) * VIC_MAX_ZWTVMOIST)

#define VICGPU_CP_LAYER(f, l)            (CP_NSCALAR + (f) * VIC_NLAYER + (l))
#define VICGPU_CP_NODE0                  (CP_NSCALAR + CPL_NFIELD * VIC_NLAYER)
#define VICGPU_CP_NODE(f, n, Nn)         (VICGPU_CP_NODE0 + (f) * (Nn) + (n))
#define VICGPU_CP_BAND0(Nn)              (VICGPU_CP_NODE0 + CPN_NFIELD * (Nn))
#define VICGPU_CP_BAND(f, b, Nn, Nb)     (VICGPU_CP_BAND0(Nn) + (f) * (Nb) + (b))
#define VICGPU_CP_ZWT0(Nn, Nb)           (VICGPU_CP_BAND0(Nn) + CPB_NFIELD * (Nb))
#define VICGPU_CP_ZWT_ZWT(l, i, Nn, Nb)  (VICGPU_CP_ZWT0(Nn, Nb) + (l) * VIC_MAX_ZWTVMOIST + (i))
#define VICGPU_CP_ZWT_MOIST(l, i, Nn, Nb) (VICGPU_CP_ZWT0(Nn, Nb) + VIC_NZWT_ROWS + (l) * VIC_MAX_ZWTVMOIST + (i))
#define VICGPU_CP_NROW(Nn, Nb)           (VICGPU_CP_ZWT0(Nn, Nb) + 2 * VIC_NZWT_ROWS)

/* ---------------------------------------------------------------- HRU parameters
 * veg_con_struct + HRU meta (vicNl_def.h:1017-1029, 1374-1388).
 * int table int[HPI_NROW][nhru], double table double[HPD_NROW][nhru]. */
enum { HPI_CELL = 0, HPI_BAND, HPI_VEG_INDEX, HPI_VEG_CLASS, HPI_IS_GLACIER, HPI_IS_ARTIFICIAL_BARE, HPI_NROW };
/* HPD_SIGMA_SLOPE, HPD_LAG_ONE, HPD_FETCH: veg_con.sigma_slope / lag_one / fetch (float in the reference, read_vegparam.c),
 * read by the blowing-snow model only (options.BLOWING) */
enum { HPD_CV = 0, HPD_ROOT0, HPD_ROOT1, HPD_ROOT2, HPD_SIGMA_SLOPE, HPD_LAG_ONE, HPD_FETCH, HPD_NROW };

/* ---------------------------------------------------------------- HRU state
 * SURVEY.md Appendix A.  double[VICGPU_SD_NROW(Nnode)][nhru], int[SI_NROW][nhru].
 * Rows up to SD_NPROG-1 plus the node block are prognostic (they steer the next
 * step); rows SD_NPROG.. are "sticky" diagnostics of energy_bal_struct that the
 * reference carries from step to step because surface_fluxes.c:301-302 seeds its
 * scratch copies from last step's struct (they only influence outputs). */
enum {
  /* soil layers (layer_data_struct, vicNl_def.h:1094-1107) */
  SD_MOIST0 = 0, SD_MOIST1, SD_MOIST2,
  SD_ICE0, SD_ICE1, SD_ICE2,
  SD_LAYER_T0, SD_LAYER_T1, SD_LAYER_T2,
  /* energy_bal_struct scalars that feed the next step */
  SD_SNOW_FLUX, SD_GRND_FLUX, SD_DELTAH, SD_FUSION, SD_LONGUNDEROUT, SD_TFOLIAGE,
  /* snow_data_struct (vicNl_def.h:1223-1257) */
  SD_SNOW_ALBEDO, SD_SNOW_COLDCONTENT, SD_SNOW_COVERAGE, SD_SNOW_DENSITY, SD_SNOW_DEPTH,
  SD_SNOW_PACK_TEMP, SD_SNOW_PACK_WATER, SD_SNOW_CANOPY, SD_SNOW_SURF_TEMP, SD_SNOW_SURF_WATER,
  SD_SNOW_SWQ, SD_SNOW_TMP_INT_STORAGE, SD_SNOW_STORE_SWQ, SD_SNOW_STORE_COVERAGE, SD_SNOW_SWQ_SLOPE,
  SD_SNOW_MAX_SWQ,
  /* veg_var_struct */
  SD_WDEW,
  /* glac_data_struct (vicNl_def.h:1341-1365) */
  SD_GLAC_SURF_TEMP, SD_GLAC_WATER_STORAGE, SD_GLAC_CUM_MASS_BALANCE,
  SD_NPROG,
  /* sticky diagnostics */
  SD_TCANOPY = SD_NPROG, SD_TSURF, SD_ALBEDO_OVER, SD_ALBEDO_UNDER,
  SD_CANOPY_ADVECTION, SD_CANOPY_LATENT, SD_CANOPY_LATENT_SUB, SD_CANOPY_SENSIBLE, SD_CANOPY_REFREEZE,
  SD_ADVECTED_SENSIBLE, SD_ADVECTION, SD_DELTACC, SD_REFREEZE_ENERGY, SD_MELT_ENERGY, SD_ERROR,
  SD_LATENT, SD_LATENT_SUB, SD_SENSIBLE,
  SD_LONGOVERIN, SD_NETLONGOVER, SD_NETSHORTOVER, SD_SHORTOVERIN,
  SD_NETLONGUNDER,   /* glacier HRUs feed last step's NetLongUnder into compute_pot_evap (surface_fluxes_glac.c:343,380) */
  SD_NSCALAR
};
/* per-node fields (x Nnode): T is prognostic; the other four are what
 * distribute_node_moisture_properties (runoff.c:763) leaves for the next step */
enum { SDN_T = 0, SDN_MOIST, SDN_ICE, SDN_KAPPA, SDN_CS, SDN_NFIELD };
#define VICGPU_SD_NODE(f, n, Nn) (SD_NSCALAR + (f) * (Nn) + (n))
#define VICGPU_SD_NROW(Nn)       (SD_NSCALAR + SDN_NFIELD * (Nn))

enum {
  SI_SNOW_LAST_SNOW = 0,   /* may be INT_MIN = INVALID_INT (vicNl_def.h:151) */
  SI_SNOW_MELTING, SI_SNOW_SNOW, SI_SNOW_STORE_SNOW,
  SI_SNOW_SURF_TEMP_FBCOUNT, SI_SNOW_SURF_TEMP_FBFLAG,
  SI_TSURF_FBCOUNT, SI_TSURF_FBFLAG, SI_TFOLIAGE_FBCOUNT, SI_TFOLIAGE_FBFLAG,
  SI_TCANOPY_FBCOUNT, SI_TCANOPY_FBFLAG,
  SI_GLAC_SURF_TEMP_FBCOUNT, SI_GLAC_SURF_TEMP_FBFLAG,
  SI_FROZEN, SI_NFROST, SI_NTHAW,
  SI_NSCALAR
};
/* per-node ints (x Nnode): T_fbflag, T_fbcount (vicNl_def.h:1152-1153) */
enum { SIN_T_FBFLAG = 0, SIN_T_FBCOUNT, SIN_NFIELD };
#define VICGPU_SI_NODE(f, n, Nn) (SI_NSCALAR + (f) * (Nn) + (n))
#define VICGPU_SI_NROW(Nn)       (SI_NSCALAR + SIN_NFIELD * (Nn))

/* ---------------------------------------------------------------- per-step HRU fluxes
 * What put_data (put_data.c:762-1232) reads from an HRU after dist_prec.
 * double[FX_NROW][nhru], overwritten every step. */
enum {
  FX_RUNOFF = 0, FX_BASEFLOW, FX_ASAT, FX_INFLOW,
  FX_EVAP0, FX_EVAP1, FX_EVAP2,            /* layer[l].evap, mm */
  FX_CANOPYEVAP, FX_THROUGHFALL,
  FX_SNOW_VAPOR_FLUX, FX_SNOW_CANOPY_VAPOR_FLUX, FX_SNOW_BLOWING_FLUX, FX_SNOW_SURFACE_FLUX,
  FX_SNOW_MELT, FX_SNOW_MASS_ERROR, FX_SNOW_QNET,
  FX_POT_EVAP0, FX_POT_EVAP1, FX_POT_EVAP2, FX_POT_EVAP3, FX_POT_EVAP4, FX_POT_EVAP5,
  FX_AERO_RESIST_SURFACE, FX_AERO_RESIST_OVERSTORY,
  FX_ROOTMOIST, FX_WETNESS,
  FX_ZWT, FX_ZWT2, FX_ZWT3,
  /* energy_bal_struct step averages (surface_fluxes.c:842-881) */
  FX_ATMOS_LATENT, FX_ATMOS_LATENT_SUB, FX_ATMOS_SENSIBLE,
  FX_LONG_UNDER_IN, FX_NET_LONG_ATMOS, FX_NET_LONG_UNDER, FX_NET_SHORT_ATMOS, FX_NET_SHORT_GRND,
  FX_NET_SHORT_UNDER, FX_SHORT_UNDER_IN,
  FX_OUT_PREC, FX_OUT_RAIN, FX_OUT_SNOW,   /* this HRU's contribution before the Cv weighting (full_energy.c:429-431) */
  /* glacier */
  FX_GLAC_MASS_BALANCE, FX_GLAC_ICE_MASS_BALANCE, FX_GLAC_ACCUMULATION, FX_GLAC_MELT, FX_GLAC_VAPOR_FLUX,
  FX_GLAC_INFLOW, FX_GLAC_OUTFLOW, FX_GLAC_OUTFLOW_COEF, FX_GLAC_QNET, FX_GLAC_COLD_CONTENT,
  FX_GLACIER_FLUX, FX_DELTACC_GLAC, FX_GLACIER_MELT_ENERGY,
  /* read by put_data only: frost / thaw front depths (energy.fdepth/tdepth, m; NaN = no such front) and the per-layer
   * water table (layer[l].zwt, cm).  Like every row here they are rewritten by the step for the HRUs it computes; for
   * HRUs whose step does not produce them (glacier HRUs have no soil column step) they keep what vicgpu_set_fluxes gave */
  FX_FDEPTH0, FX_FDEPTH1, FX_FDEPTH2, FX_TDEPTH0, FX_TDEPTH1, FX_TDEPTH2, FX_ZWTL0, FX_ZWTL1, FX_ZWTL2,
  FX_NROW
};

/* per-step cell outputs: atmos->out_prec/out_rain/out_snow (full_energy.c:429-431), double[CO_NROW][ncell] */
enum { CO_OUT_PREC = 0, CO_OUT_RAIN, CO_OUT_SNOW, CO_NROW };

/* per-cell running sums over the steps of one vicgpu_step call (Cv-weighted like
 * put_data.c:789 "AreaFactor = Cv * mu * TreeAdjust", TreeAdjust = 1):
 * double[CA_NROW][ncell]; zeroed by vicgpu_reset_accum. */
enum {
  CA_RUNOFF = 0, CA_BASEFLOW, CA_EVAP, CA_SWE_END, CA_SOIL_MOIST_END0, CA_SOIL_MOIST_END1, CA_SOIL_MOIST_END2,
  CA_GLAC_MASS_BALANCE, CA_PREC, CA_NSTEPS, CA_NROW
};

/* per-cell error bits (the reference's ERROR returns, vicNl.c:545-559) */
#define VICGPU_CELLERR_SOLVER   1   /* a solver returned ERROR with TFALLBACK off */
#define VICGPU_CELLERR_AERO     2   /* CalcAerodynamic trunk-space error (CalcAerodynamic.c:214-217) */
#define VICGPU_CELLERR_NODES    4   /* thermal nodes do not reach below the bottom layer (soil_conduction.c:526-529) */
#define VICGPU_CELLERR_NAN      8   /* non-finite prognostic state after the step */
#define VICGPU_CELLERR_REFERENCE (VICGPU_CELLERR_SOLVER | VICGPU_CELLERR_AERO | VICGPU_CELLERR_NODES)  /* the reference's ERROR returns */

typedef struct vicgpu_ctx vicgpu_ctx;

/* ---- lifetime ------------------------------------------------------------ */
/* replaces ProgramState construction for the path (initialize_global.c:8, get_global_param.c:131) */
int  vicgpu_create(const vicgpu_options *opt, int device, vicgpu_ctx **out);
void vicgpu_destroy(vicgpu_ctx *ctx);
const char *vicgpu_last_error(const vicgpu_ctx *ctx);
int  vicgpu_abi_version(void);

/* ---- static domain --------------------------------------------------------
 * veg_lib: read_veglib.c:44-137 result.  Domain: readSoilData + read_vegparam +
 * read_snowband results (vicNl.c:237-293,170-175).  cell_hru_offset[ncell+1] /
 * cell_hru_list[nhru] is the CSR listing of each cell's HRUs in hruList order
 * (the order full_energy.c:216 iterates and sums out_prec in). */
int vicgpu_set_veglib(vicgpu_ctx *ctx, int nrow, const double *veglib);
int vicgpu_set_domain(vicgpu_ctx *ctx, int ncell, int nhru,
                      const double *cell_params,      /* [CP_NROW][ncell] */
                      const int    *hru_iparams,      /* [HPI_NROW][nhru] */
                      const double *hru_dparams,      /* [HPD_NROW][nhru] */
                      const int    *cell_hru_offset,  /* [ncell+1] */
                      const int    *cell_hru_list);   /* [nhru] */

/* ---- state: initialize_model_state result in / write_model_state content out -- */
int vicgpu_set_state(vicgpu_ctx *ctx, const double *state_d, const int *state_i);
int vicgpu_get_state(vicgpu_ctx *ctx, double *state_d, int *state_i);

/* The same state as the reference's state file holds it (write_model_state.c:95-337, processCellForStateFile): one record
 * per HRU, HRUs in cell-major hruList order (cell_hru_list order), every value as a double, fields in the order the
 * StateIO stream sees them (SR_*; node arrays Nnode long).  vicgpu_get_state_records gathers the records on the device
 * (the write side: the host streams them through its StateIO back-end unchanged); vicgpu_set_state_records is the read
 * side (read_initial_model_state.c): it scatters the persisted fields into the state and flux tables and leaves every
 * other row as it is -- like the reference, whose reader fills the HRUs initialize_model_state has just initialised.
 * Band and vegetation class of every record must match the domain (the reference throws, write_model_state.c:179-188):
 * VICGPU_ERR_ARG otherwise, with nothing scattered. */
enum {
  SR_BAND_INDEX = 0, SR_VEG_CLASS,
  SR_MOIST0, SR_MOIST1, SR_MOIST2, SR_ICE0, SR_ICE1, SR_ICE2,
  SR_WDEW,                       /* not in the stream of an artificial bare-soil HRU (write_model_state.c:240-242) */
  SR_SNOW_CANOPY, SR_SNOW_DENSITY, SR_SNOW_DEPTH, SR_SNOW_PACK_WATER, SR_SNOW_SURF_WATER, SR_SNOW_SWQ,
  SR_GLAC_WATER_STORAGE, SR_GLAC_CUM_MASS_BALANCE,
  SR_ENERGY_T                    /* Nnode values; the fields after it are addressed with VICGPU_SR() */
};
/* position of the fields that follow the first node array */
enum {
  SRT_TFOLIAGE = 0, SRT_GLAC_SURF_TEMP, SRT_SNOW_COLD_CONTENT, SRT_SNOW_PACK_TEMP, SRT_SNOW_SURF_TEMP, SRT_SNOW_ALBEDO,
  SRT_SNOW_LAST_SNOW, SRT_SNOW_MELTING, SRT_TCANOPY_FBCOUNT,
  SRT_T_FBCOUNT                  /* Nnode values */
};
enum {
  SRU_TFOLIAGE_FBCOUNT = 0, SRU_TSURF_FBCOUNT, SRU_GLAC_SURF_TEMP_FBCOUNT, SRU_SNOW_SURF_TEMP_FBCOUNT,
  SRU_GLAC_SURF_TEMP_FBFLAG, SRU_GLAC_VAPOR_FLUX, SRU_SNOW_CANOPY_ALBEDO, SRU_SNOW_SURFACE_FLUX, SRU_SNOW_SURF_TEMP_FBFLAG,
  SRU_SNOW_TMP_INT_STORAGE, SRU_SNOW_VAPOR_FLUX, SRU_NFIELD
};
#define VICGPU_SR_T(f, Nn)   (SR_ENERGY_T + (Nn) + (f))                  /* SRT_* field */
#define VICGPU_SR_U(f, Nn)   (SR_ENERGY_T + (Nn) + SRT_T_FBCOUNT + (Nn) + (f))   /* SRU_* field */
#define VICGPU_SR_LEN(Nn)    VICGPU_SR_U(SRU_NFIELD, Nn)
int vicgpu_get_state_records(vicgpu_ctx *ctx, double *records);         /* [nhru][VICGPU_SR_LEN(Nnode)] */
int vicgpu_set_state_records(vicgpu_ctx *ctx, const double *records);

/* ---- forcing chunk: replaces cell.atmos[rec] (initialize_atmos.c) for steps
 * [0, nsteps) of the chunk; copied to the device asynchronously on the copy stream. */
int vicgpu_push_forcing(vicgpu_ctx *ctx, int nsteps,
                        const double *forcing,          /* [nsteps][VIC_NFORCE][NF+1][ncell] */
                        const unsigned char *snowflag,  /* [nsteps][NF+1][ncell] */
                        const int *dmy);                /* [nsteps][VIC_NDMY] */

/* ---- forcing streaming.  The context holds two forcing chunks: the current one (vicgpu_step indexes it) and a spare.
 *   vicgpu_prefetch_forcing      starts the upload of the NEXT chunk into the spare (copy stream; returns at once)
 *   vicgpu_prefetch_forcing_raw  the same from hourly raw forcing (VIC_RAW_*): the device derives what initialize_atmos.c
 *                                derives per record -- kPa -> Pa (:290-295), the MIN_WIND_SPEED floor (:518-536), air
 *                                density from pressure (:980-1000, plapse != 0: the PLAPSE form), vpd = svp(T) - vp clipped
 *                                at 0 (:1175-1193), the snow_step aggregation with the step mean / sum in sub-index NR, and
 *                                the snowflag (:1275-1303)
 *   vicgpu_prefetch_forcing_perturbed  the same from shared raw columns, expanded and perturbed per forcing column (below)
 *   vicgpu_swap_forcing          makes the prefetched chunk the current one (steps already queued keep the old one)
 * so a driver overlaps the transfer of chunk k+1 with the steps of chunk k:
 *     push(0);  for k: { prefetch(k+1); step(0, n_k); swap(); }
 * vicgpu_push_forcing == prefetch + swap.  Host buffers: memory from vicgpu_host_alloc (pinned) is read by DMA while the
 * steps run and must stay unchanged until vicgpu_swap_forcing returns; any other memory is first copied into the
 * library's own pinned staging area, so it can be reused as soon as the call returns. */
int vicgpu_prefetch_forcing(vicgpu_ctx *ctx, int nsteps, const double *forcing, const unsigned char *snowflag, const int *dmy);
int vicgpu_prefetch_forcing_raw(vicgpu_ctx *ctx, int nsteps,
                                const double *raw,      /* [nsteps][VIC_NRAW][dt][ncell] */
                                const int *dmy, double min_wind_speed, int plapse);
/* ---- perturbed and expanded raw forcing: the front of a data-assimilation cycle.  An ensemble filter gets its spread from
 * perturbed meteorology -- multiplicative noise on precipitation and shortwave, additive noise on air temperature and longwave,
 * different for every member at every step.  The derived rows cannot be perturbed after the fact (air temperature changes vpd,
 * the density and the snowflag), so the perturbation enters in front of the derivation: the caller uploads the shared raw
 * columns once, nsrc wide, and the few factors; the device expands, perturbs and derives every forcing column.
 *   ncol       the width of the context's forcing tables: ncell without a forcing map, the map's ncol with one.  The lists here
 *              go from forcing columns to source columns and groups; the context's map still goes from cells to forcing
 *              columns, so the two compose.
 *   col_src    forcing column i reads source column col_src[i] of raw.  NULL: nsrc == ncol, column i reads source i.
 *   col_group  forcing column i takes the factors of group col_group[i].  NULL: a group per column (ngroup == ncol, spatial
 *              noise), or no perturbation (ngroup == 0).
 *   pert       rows VICGPU_PERT_MUL(v) and VICGPU_PERT_ADD(v) of one (step, group) for raw variable v (VIC_RAW_*).
 * The member ensemble: the identity forcing map, col_src = tile(arange(nsrc), M), col_group = repeat(arange(M), nsrc).  A
 * calibration ensemble whose members share columns keeps its map.
 * What a column reads: for forcing column i, step s, raw variable v and hour h the derivation reads x' = (x * mul) + add with
 *   x = raw[s][v][h][col_src[i]], mul = pert[s][VICGPU_PERT_MUL(v)][col_group[i]], add = pert[s][VICGPU_PERT_ADD(v)][col_group[i]];
 * the product and the sum are each rounded once (the library is built without contraction; this is part of the contract).
 * With pert == NULL x' = x verbatim: no multiply by one, no add of zero.  Everything after that is
 * vicgpu_prefetch_forcing_raw's derivation, unchanged and in the same order: kPa -> Pa, the MIN_WIND_SPEED floor (on the
 * perturbed wind), the snow_step aggregation, density, vpd = svp(T) - vp with its clip, the NR slot, and the flag per cell, from
 * that cell's parameters and its column's derived T and prec.  So the chunk it stages is bit for bit the chunk
 * vicgpu_prefetch_forcing_raw stages from the ncol-wide table of the x'; with col_src == NULL and ngroup == 0 the call is
 * vicgpu_prefetch_forcing_raw.  Nothing is clamped: a multiplier that makes precipitation negative is the caller's, and vapour
 * pressure does not follow a temperature perturbation unless the caller perturbs it.
 * Order and buffers are those of vicgpu_prefetch_forcing_raw: the copy stream, the spare slot, vicgpu_swap_forcing after it; a
 * pinned raw is read until vicgpu_swap_forcing returns, other memory goes through the slot's staging area.  col_src, col_group
 * and pert are free when the call returns.  The slot owns its device copies of the three lists and of the nsrc-wide raw table;
 * they are re-used by the next call and released with the slot.
 * Everything is checked before the first upload; a failing call leaves the current and the staged chunk as they were.
 * VICGPU_ERR_ARG: a null handle, raw or dmy; nsteps <= 0 or nsrc < 1; a month outside 1..12; col_src == NULL with nsrc != ncol;
 * an entry of col_src outside [0, nsrc); ngroup < 0; ngroup > 0 with pert == NULL, or pert with ngroup == 0; col_group == NULL
 * with ngroup other than 0 or ncol; an entry of col_group outside [0, ngroup); a pert value that is not finite
 * (vicgpu_last_error names step, row and group).  VICGPU_ERR_STATE: no domain.  VICGPU_ERR_HIP: the runtime refused an
 * allocation -- nothing is left behind, and the slot stays usable. */
#define VICGPU_PERT_MUL(v) (2 * (v))
#define VICGPU_PERT_ADD(v) (2 * (v) + 1)
#define VICGPU_NPERT       (2 * VIC_NRAW)
int vicgpu_prefetch_forcing_perturbed(vicgpu_ctx *ctx, int nsteps,
        int nsrc, const double *raw,        /* [nsteps][VIC_NRAW][dt][nsrc] */
        const int *col_src,                 /* [ncol], each in [0, nsrc); NULL: nsrc must be ncol, column i reads source i */
        int ngroup, const int *col_group,   /* [ncol], each in [0, ngroup); NULL: ngroup must be ncol (column i is group i) or 0 */
        const double *pert,                 /* [nsteps][VICGPU_NPERT][ngroup]; NULL with ngroup == 0: no perturbation */
        const int *dmy, double min_wind_speed, int plapse);
int vicgpu_swap_forcing(vicgpu_ctx *ctx);
int vicgpu_get_forcing(vicgpu_ctx *ctx, int step, double *forcing /* [VIC_NFORCE][NF+1][ncell] */,
                       unsigned char *snowflag /* [NF+1][ncell] */);       /* read-back of the current chunk (tests) */
void *vicgpu_host_alloc(size_t bytes);                  /* pinned host memory for forcing chunks */
void vicgpu_host_free(void *p);

/* ---- forcing map: cells that share forcing columns (ensembles over the same meteorology -- calibration, sensitivity and
 * perturbed-state runs, whose members are just more cells -- and a model grid finer than its forcing grid).
 *   vicgpu_set_forcing_map   cell_col[ncell], 0 <= cell_col[c] < ncol, ncol >= 1: cell c reads forcing column cell_col[c].  A
 *                            column may be used by any number of cells or by none; any map is legal (it need not be monotone
 *                            or blocked).  cell_col == NULL (with ncol 0 or ncell): the identity, every cell its own column.
 *   vicgpu_get_forcing_map   *ncol, and the map into cell_col[ncell] unless cell_col is NULL.
 * Once a map is set every forcing table is ncol wide instead of ncell wide: forcing of vicgpu_push_forcing /
 * vicgpu_prefetch_forcing and of vicgpu_get_forcing is [nsteps][VIC_NFORCE][NF+1][ncol], raw of vicgpu_prefetch_forcing_raw is
 * [nsteps][VIC_NRAW][dt][ncol], and VICGPU_PTR_FORCING points to the current chunk in that layout.  put_data's forcing echoes
 * (OUT_AIR_TEMP .. OUT_WIND, OUT_QAIR, OUT_REL_HUMID; OUT_PREC / OUT_RAINF / OUT_SNOWF come from the cell's own step) are those
 * of the cell's column.
 * snowflag stays per cell, [nsteps][NF+1][ncell]: the flag is a function of the cell's own parameters (the smallest Tfactor
 * of its bands, MAX_SNOW_TEMP, MIN_RAIN_TEMP: initialize_atmos.c:1275-1303) -- calibration parameters, so two members on one
 * column may differ in it.  vicgpu_prefetch_forcing_raw derives the nine numeric rows once per column (they depend on the raw
 * values and the options only) and the flag once per cell, from that cell's parameters and its column's air temperature and
 * precipitation.
 * The map belongs to the domain: vicgpu_set_domain resets it to the identity.  Setting a map (the identity included) waits
 * for the steps queued so far and drops both forcing chunks, because a chunk's rows are as wide as the map it was pushed for:
 * vicgpu_step and vicgpu_run_records return VICGPU_ERR_STATE until a chunk is pushed, as after vicgpu_set_domain.  The state,
 * the validity table, the put_data and records configuration and the aggregates are untouched.
 * VICGPU_ERR_ARG: a null handle (or ncol pointer), ncol < 1 with a map, an entry outside [0, ncol), NULL with an ncol other
 * than 0 or ncell -- the map and the chunk in force stay; VICGPU_ERR_STATE: no domain; VICGPU_ERR_HIP: the runtime refused an
 * allocation -- nothing is left behind and the map in force stays. */
int vicgpu_set_forcing_map(vicgpu_ctx *ctx, int ncol, const int *cell_col);
int vicgpu_get_forcing_map(vicgpu_ctx *ctx, int *ncol, int *cell_col);   /* cell_col may be NULL: ncol only */

/* ---- the hot path: for rec in [step0, step0+nsteps): dist_prec for every cell
 * (vicNl.c:506-543).  With QUICK_FLUX the call only enqueues work.  With the
 * finite-difference soil profile (QUICK_FLUX off / FROZEN_SOIL) a step is a
 * data-dependent number of kernel rounds, so the call returns when the last
 * step's kernels have been issued, i.e. it blocks for most of the run time.
 * vicgpu_synchronize waits for completion in both cases.
 * Environment: VICGPU_CHUNKS=n runs n cell chunks as independent pipelines
 * (own streams and host threads; results are identical for any n),
 * VICGPU_TRACE / VICGPU_STATS print per-step round counts and timings. */
int vicgpu_step(vicgpu_ctx *ctx, int step0, int nsteps);
int vicgpu_synchronize(vicgpu_ctx *ctx);

/* ---- outputs of the last executed step / accumulated over calls ---------- */
int vicgpu_get_fluxes(vicgpu_ctx *ctx, double *flux);             /* [FX_NROW][nhru] */
int vicgpu_get_cell_outputs(vicgpu_ctx *ctx, double *cell_out);   /* [CO_NROW][ncell] */
int vicgpu_get_accum(vicgpu_ctx *ctx, double *accum);             /* [CA_NROW][ncell] */
int vicgpu_reset_accum(vicgpu_ctx *ctx);
int vicgpu_get_cell_errors(vicgpu_ctx *ctx, int *flags);          /* [ncell] */

/* ---- cell validity: cell.isValid and CONTINUEONERROR (vicNl.c:429, 521, 545-559) ----------
 * The reference stops stepping a cell once its step has returned ERROR: isValid = FALSE (vicNl.c:545-559), and from the next
 * record on vicNl.c:521 skips the cell entirely -- no dist_prec, no put_data, no accumulateGlacierMassBalance.  The cell
 * keeps the state it failed in, and its aggregates, never refilled after the reset of vicNl.c:599-606, stay 0.
 *   vicgpu_set_retire_on_error  mask = OR of VICGPU_CELLERR_*: a cell whose flag word has a bit of the mask set at the end of
 *                               step s is invalid from step s + 1 on, decided on the device -- inside a multi-step vicgpu_step
 *                               and inside vicgpu_run_records as well.  Step s itself is complete (every HRU, the cell sums,
 *                               put_data: dist_prec.c:167 calls it after a failed full_energy too).  0 (the default): no cell is
 *                               ever retired.  A setting of the context: it survives vicgpu_set_domain.
 *   vicgpu_set_cell_valid       the host's own isValid, [ncell]: 0 = skip the cell from the next step on (a cell that failed
 *                               initialisation, vicNl.c:429), vicgpu_put_data_init included; non-zero = step it again from the
 *                               tables as they stand (a cell whose flag word still has a bit of the mask retires again after
 *                               that step: vicgpu_reset_accum clears the flags).
 *   vicgpu_get_cell_valid       [ncell], 1 = the next step computes the cell, 0 = it does not.
 * Nothing of an invalid cell changes: the SD_* / SI_* / FX_* columns and hru_err of its HRUs (no zero record is written),
 * its CO_* / CA_* columns (CA_NSTEPS included), its flag word, its PB_* bookkeeping and its un-aggregated output values.  Its
 * aggregates receive nothing: after the next reset they are 0.0 in every row and stay so, as in the reference's files; an
 * output record of such a cell holds those zeros and the frozen flag word.  Its glacier HRUs stop accumulating
 * cum_mass_balance, and vicgpu_glacier_mass_balance_fit gives it the default equation without resetting them (vicNl.c:562).
 * The validity table belongs to the domain: vicgpu_set_domain sets it to all 1; vicgpu_set_state and vicgpu_reset_accum
 * leave it alone.  vicgpu_get_state_records / vicgpu_set_state_records keep their fixed [nhru] layout and include invalid
 * cells; the reference leaves them out of the state file (vicNl.c:521 precedes write_model_state), so a driver filters the
 * records with vicgpu_get_cell_valid.
 * VICGPU_ERR_ARG: null handle or pointer, a mask with bits outside the four VICGPU_CELLERR_*; VICGPU_ERR_STATE: the validity
 * entries before a domain is set. */
int vicgpu_set_retire_on_error(vicgpu_ctx *ctx, int mask);        /* OR of VICGPU_CELLERR_*; 0 (default) = no cell is retired */
int vicgpu_set_cell_valid(vicgpu_ctx *ctx, const int *valid);     /* [ncell], 0 = skip the cell from the next step on (cell.isValid) */
int vicgpu_get_cell_valid(vicgpu_ctx *ctx, int *valid);           /* [ncell], 1 / 0 */

/* ---- model state copied between cells on the device: the ensemble workflows that move state from one member (= a block of
 * cells) to another without a host round trip -- seeding (spin up one member, hand its state to all), resampling (a particle
 * filter replaces members by copies of other members, every assimilation cycle) and rollback (a spare block of cells kept as
 * a snapshot of a member, restored from later).
 *   vicgpu_copy_cells   for every i < n, cell dst_cell[i] takes the listed rows of cell src_cell[i].  what = an OR of
 *                       VICGPU_COPY_STATE    every SD_* / SDN_* row, every SI_* / SIN_* row and every FX_* row of the cell's HRUs
 *                       VICGPU_COPY_BALANCE  every PB_* row of the cell (vicgpu_out.h: put_data's bookkeeping, which has no
 *                                            setter), so that the destination's next OUT_DELSOILMOIST / OUT_WATER_ERROR continue
 *                                            the source's instead of showing the jump; needs vicgpu_put_data_config.
 * The assignment is simultaneous: every source is read as it was before the call, so a permutation (a rotation, a swap) is
 * legal.  A source may repeat; a destination must not.  dst == src is a legal pair and a no-op, and so is n == 0.
 * HRUs pair by position: the j-th HRU of the destination cell, in cell_hru_list order, takes the j-th HRU of the source cell.
 * Values are copied verbatim, nothing is rescaled: a member with other soil depths gets the source's millimetres, exactly as
 * vicgpu_set_state would give it.  A pair is legal only if both cells have the same number of HRUs and, position by position,
 * equal HPI_BAND, HPI_VEG_CLASS, HPI_IS_GLACIER and HPI_IS_ARTIFICIAL_BARE.
 * Untouched: the parameters, the forcing map and the validity table (a retired destination stays retired; its columns still
 * take the copy), hru_err and the cell flag words, CO_* and CA_*, the un-aggregated output values and the aggregates, the
 * records configuration and the cell groups, the forcing chunks, the finite-difference workspace.
 * Order: the call takes effect after every step queued before it and before every step queued after it (it is queued on the
 * context's stream, which with the finite-difference pipeline waits for every cell chunk first).  It need not have finished
 * when it returns: vicgpu_synchronize waits for it, and so does every read-back.  Records of an earlier vicgpu_run_records that
 * are still on their way are not affected (they read the record slots, not these tables).
 * Two paths with identical results: when no destination is also the source of another pair (the fan-out from one member) one
 * kernel per table copies the columns in place; otherwise the columns go through a staging buffer, the rows in passes, so
 * that the staging memory stays within VICGPU_COPY_STAGE_MB (256; read per vicgpu_set_domain) whatever the number of pairs.
 * Every failing call leaves every table bit-identical; all pairs are checked before the first write.
 * VICGPU_ERR_ARG: a null handle, null lists with n > 0, n < 0, a cell outside [0, ncell), a repeated destination, `what` 0 or
 * with unknown bits, an incompatible pair; VICGPU_ERR_STATE: no domain, VICGPU_COPY_BALANCE without a put_data configuration;
 * VICGPU_ERR_HIP: the runtime refused an allocation -- nothing is left behind. */
#define VICGPU_COPY_STATE   1
#define VICGPU_COPY_BALANCE 2
int vicgpu_copy_cells(vicgpu_ctx *ctx, int n, const int *dst_cell, const int *src_cell, int what);

/* ---- cell and HRU parameters updated in place: the step of an ensemble loop in which the members get new parameter values
 * -- a calibration generation changes a handful of soil rows of every member, a sensitivity sweep one row, a coupled glacier
 * model the HPD_CV of the HRUs and CPB_AREAFRACT / CPB_BANDELEV of the bands once per coupling interval -- without the
 * teardown of vicgpu_set_domain.
 *   vicgpu_update_cell_params   for every k < nrow and i < n, row rows[k] of cell cells[i] of the cell parameter table takes
 *                               values[k * n + i].  rows: rows of the caller's table, each in [0, VICGPU_CP_NROW(Nnode, Nband)).
 *                               cells == NULL is the dense form: n must be ncell, and column i is cell i.
 *   vicgpu_update_hru_params    the same on the HPD_* rows of the HRU columns hrus[i]; hrus == NULL: n must be nhru.
 *   vicgpu_get_cell_params      the caller's rows [VICGPU_CP_NROW][ncell] as the library holds them
 *   vicgpu_get_hru_params       [HPD_NROW][nhru]
 * After the call the context is, in every table and in every later result, bit for bit the context vicgpu_set_domain would
 * have built from the updated tables, holding everything else the current context holds.  The listed entries take the new
 * values verbatim, and the library re-derives the rows it appends to its own copy of the table: the soil-conductivity layer
 * constants of every listed cell and, when put_data is configured, the tree-line adjustment factors of every listed cell and
 * of every cell that owns a listed HRU (a later vicgpu_put_data_config derives them for all cells anyway).
 * Untouched: state and fluxes, hru_err and the cell flag words, CO_* and CA_*, PB_*, the un-aggregated output values and the
 * aggregates, the validity table, the forcing map and both forcing chunks, the put_data and records configuration and the
 * cell groups, the finite-difference workspace and the cell chunks, the HPI_* rows (the structure of a domain is not
 * updatable) and the vegetation library.
 * What follows from that, and is the driver's to handle:
 *   - forcing chunks already uploaded keep the derived rows and the snowflag they were derived with: after a change of
 *     CP_MAX_SNOW_TEMP, CP_MIN_RAIN_TEMP, a CPB_TFACTOR / CPB_PFACTOR or the elevation, push the forcing again;
 *   - rows that the reference's readers derive from other rows are the caller's to keep consistent, exactly as with
 *     vicgpu_set_domain: CPL_MAX_MOIST from depth and porosity, the node CPN_ALPHA / CPN_BETA / CPN_GAMMA, the zwtvmoist curves;
 *   - nothing is rescaled: after an HPD_CV or depth change the state keeps its millimetres, and OUT_DELSOILMOIST /
 *     OUT_WATER_ERROR of the next record show the jump unless vicgpu_put_data_init is called again.
 * Order: the update takes effect after every step queued before it and before every step queued after it (it is queued on the
 * context's stream, which with the finite-difference pipeline waits for every cell chunk first).  The caller's buffers may be
 * reused when the call returns; vicgpu_synchronize and every read-back wait for the update.  Records of an earlier
 * vicgpu_run_records that are still on their way are not affected.
 * The values travel through a staging buffer on the device, the rows in passes, so that the staging memory stays within
 * VICGPU_COPY_STAGE_MB whatever the size of the update; the result does not depend on the budget.
 * nrow == 0 and n == 0 are legal and change nothing.  Every failing call leaves every table bit-identical; everything is
 * checked before the first write.
 * VICGPU_ERR_ARG: a null handle, nrow < 0 or n < 0, null rows or values with work to do, a row out of range or listed twice, a
 * cell / HRU out of range or listed twice, a NULL list with n other than ncell / nhru; VICGPU_ERR_STATE: no domain;
 * VICGPU_ERR_HIP: the runtime refused an allocation -- nothing is left behind. */
int vicgpu_update_cell_params(vicgpu_ctx *ctx, int nrow, const int *rows, int n, const int *cells, const double *values);
int vicgpu_update_hru_params(vicgpu_ctx *ctx, int nrow, const int *rows, int n, const int *hrus, const double *values);
int vicgpu_get_cell_params(vicgpu_ctx *ctx, double *cell_params);  /* [VICGPU_CP_NROW][ncell] */
int vicgpu_get_hru_params(vicgpu_ctx *ctx, double *hru_dparams);   /* [HPD_NROW][nhru] */

/* ---- model state read and changed in place, row by row, and its dependent soil rows re-derived: the analysis update of an
 * ensemble loop -- EnKF increments on soil moisture and SWE, direct insertion of an observed SWE, a perturbation of the node
 * temperatures -- reads a few state rows of every member, changes them and makes the rest of the state consistent with the
 * change, without moving the whole state through the host.  The same derive is the tail of a restart into a fresh context:
 * vicgpu_set_state_records scatters the persisted fields, vicgpu_derive_soil_state(all HRUs, NODES | LAYERS | FRONTS) gives
 * the rows initialize_model_state.c rebuilds after it has read a state file.
 *   vicgpu_get_state_rows      values[k * n + i] = row rows[k] of HRU hrus[i] of the SD table, for every k < nrow and i < n.
 *                              rows: each in [0, VICGPU_SD_NROW(Nnode)).  hrus == NULL is the dense form: n must be nhru, and
 *                              column i is HRU i.  The list rules are those of vicgpu_update_hru_params.
 *   vicgpu_get_state_rows_i    the same on the SI table, rows in [0, VICGPU_SI_NROW(Nnode)).
 *   vicgpu_update_state        VICGPU_STATE_SET: the listed SD entries take values[k * n + i] verbatim (NaN is legal:
 *                              SD_GLAC_CUM_MASS_BALANCE starts as NaN).  VICGPU_STATE_ADD: they take old + values[k * n + i],
 *                              one rounded double-precision add.  Nothing is clamped, and no other row follows: consistency is
 *                              vicgpu_derive_soil_state's, and the caller decides when.
 *   vicgpu_update_state_i      SET on the SI table.
 *   vicgpu_derive_soil_state   for every listed HRU (hrus == NULL: all, n must be nhru) the stages selected in `what` run in the
 *                              reference's order, each on what the earlier ones left:
 *     VICGPU_DERIVE_CAP_MOIST  per layer: moist > CPL_MAX_MOIST gives ice *= max_moist / moist, moist = max_moist; then ice >
 *                              moist gives ice = moist.  Writes SD_MOIST0..2 and SD_ICE0..2.  With GLACIER_DYNAMICS the
 *                              reference keeps the excess in cell.excess_moist, which no table carries: VICGPU_ERR_UNSUPPORTED.
 *     VICGPU_DERIVE_NODES      distribute_node_moisture_properties from SDN_T and SD_MOIST0..2: the SDN_MOIST, SDN_ICE,
 *                              SDN_KAPPA and SDN_CS blocks.  An HRU with HPD_CV <= 0, or CPB_AREAFRACT <= 0 in its band, gets
 *                              zeros in the four blocks, and neither of the two stages below runs for it.
 *     VICGPU_DERIVE_LAYERS     SD_ICE0..2 and SD_LAYER_T0..2 by estimate_layer_ice_content, or with QUICK_FLUX by
 *                              estimate_layer_ice_content_quick_flux from node temperatures 0 and 1.  Where the thermal nodes
 *                              do not reach below the bottom layer (the reference returns ERROR, soil_conduction.c:526-529)
 *                              the layers above the failing one take their values, the failing one zeros, the ones below keep
 *                              theirs, and VICGPU_CELLERR_NODES is OR-ed into the cell's flag word, as a step reports it
 *                              (vicgpu_get_cell_errors; vicgpu_reset_accum clears it).  No other flag is ever set here.
 *     VICGPU_DERIVE_FRONTS     only without QUICK_FLUX and in CP_FS_ACTIVE cells: find_0_degree_fronts gives SI_NFROST, SI_NTHAW,
 *                              FX_FDEPTH0..2 and FX_TDEPTH0..2 (NaN where there is no front).  Otherwise those rows stay.
 * The parameters are the context's own, the library's appended rows included: a derive after vicgpu_update_cell_params works
 * on the updated soil.  The functions are the step's own device functions: after a step, VICGPU_DERIVE_NODES reproduces the
 * node blocks the step left.  The cell validity table is not consulted: a listed HRU of a retired cell is updated and derived.
 * Untouched: everything vicgpu_update_cell_params leaves untouched (but the cell flag words as described), both parameter
 * tables, and every state and flux row that is neither listed nor produced by a selected stage.
 * Order: as for vicgpu_update_cell_params -- behind every step queued before (every cell chunk of the finite-difference
 * pipeline included), ahead of every step queued after.  The caller's buffers are free when a call returns; a get returns with
 * the values in place, so it waits for everything queued before it.
 * The values travel through a staging buffer on the device, the rows in passes within VICGPU_COPY_STAGE_MB, up and down; the
 * result does not depend on the budget.
 * nrow == 0 and n == 0 are legal and change nothing.  Every failing call leaves every table bit-identical; everything is
 * checked before the first write.
 * VICGPU_ERR_ARG: as for vicgpu_update_hru_params; a `mode` other than the two; `what` 0 or with unknown bits;
 * VICGPU_ERR_STATE: no domain; VICGPU_ERR_UNSUPPORTED: VICGPU_DERIVE_CAP_MOIST with GLACIER_DYNAMICS; VICGPU_ERR_HIP: the
 * runtime refused an allocation -- nothing is left behind. */
#define VICGPU_STATE_SET 0
#define VICGPU_STATE_ADD 1
#define VICGPU_DERIVE_CAP_MOIST 1   /* initialize_model_state.c:397-434 */
#define VICGPU_DERIVE_NODES     2   /* :712     distribute_node_moisture_properties */
#define VICGPU_DERIVE_LAYERS    4   /* :728-732 estimate_layer_ice_content(_quick_flux) */
#define VICGPU_DERIVE_FRONTS    8   /* :736-737 find_0_degree_fronts */
int vicgpu_get_state_rows(vicgpu_ctx *ctx, int nrow, const int *rows, int n, const int *hrus, double *values);
int vicgpu_get_state_rows_i(vicgpu_ctx *ctx, int nrow, const int *rows, int n, const int *hrus, int *values);
int vicgpu_update_state(vicgpu_ctx *ctx, int nrow, const int *rows, int n, const int *hrus, const double *values, int mode);
int vicgpu_update_state_i(vicgpu_ctx *ctx, int nrow, const int *rows, int n, const int *hrus, const int *values);
int vicgpu_derive_soil_state(vicgpu_ctx *ctx, int n, const int *hrus, int what);

/* ---- model state combined linearly across cells on the device: the step every ensemble filter has.  An ensemble transform
 * writes each member's analysis state as a weighted sum of the members' forecast states -- for member m at base cell j,
 * x_a[m] = sum over m' of W_j[m'][m] * x_f[m'], W global for an ETKF or an EnKF in ensemble space and per location for a
 * localised filter; inflation and recentring about the ensemble mean have the same form -- without pulling the rows
 * (vicgpu_get_state_rows), multiplying on the host and pushing them (vicgpu_update_state).  vicgpu_copy_cells is the special
 * case "one term, weight 1".
 *   vicgpu_mix_cells   acts on the listed rows of the SD table, each in [0, VICGPU_SD_NROW(Nnode)).  Destination dst_cell[i]
 *                      has the terms t = term_off[i] .. term_off[i + 1] - 1: cell term_cell[t] with weight term_weight[t].
 * Pairing: as in vicgpu_copy_cells, HRUs pair by position -- the j-th HRU of the destination cell, in cell_hru_list order,
 * combines the j-th HRUs of its term cells.  A term cell is legal for a destination under the pair rule of vicgpu_copy_cells:
 * the same number of HRUs and, position by position, equal HPI_BAND, HPI_VEG_CLASS, HPI_IS_GLACIER, HPI_IS_ARTIFICIAL_BARE.
 * Simultaneity: every source is read as it was before the call.  A destination may be a term of itself and of other
 * destinations (the dense member transform is all of that); a source may repeat across destinations and within one
 * destination; a destination must not repeat.
 * Arithmetic (part of the contract; the library is built without floating-point contraction): for one destination HRU and
 * one row, with the terms in list order, p = w_0 * x_0 (assigned, not added to zero), then p = p + (w_t * x_t) for t = 1, 2,
 * ...; every product and every sum is rounded once.  The result depends on nothing else -- not the staging budget, not the cell
 * chunks, not the kernel geometry.  A single term of weight 1.0 reproduces the source bit for bit, -0.0 included, so such a
 * call equals vicgpu_copy_cells(VICGPU_COPY_STATE) on the listed rows.  Nothing is dropped or clamped; a zero weight still
 * reads its operand (0 * NaN is NaN; SD_GLAC_CUM_MASS_BALANCE starts as NaN, and mixing it is the caller's decision).  No other
 * row follows: consistency is vicgpu_derive_soil_state's, and the caller decides when.
 * Untouched: everything vicgpu_update_state leaves untouched, the SI and FX tables, the cell flag words, and the unlisted rows
 * and columns of SD.  The validity table is not consulted: a retired destination still takes its values.
 * Order: as for vicgpu_copy_cells -- queued on the context's stream, behind every step queued before it (every cell chunk of
 * the finite-difference pipeline included), ahead of every step queued after it.  The caller's buffers are free when it
 * returns; vicgpu_synchronize and every read-back wait for it.  Records of an earlier vicgpu_run_records that are still on
 * their way are not affected.
 * The result always goes through a staging buffer on the device (sources are read before any destination is written), the
 * rows in passes within VICGPU_COPY_STAGE_MB.  The term lists stay per cell on the device: their size is that of the caller's.
 * nrow == 0 and ndst == 0 are legal and change nothing.  Every failing call leaves every table bit-identical; everything is
 * checked, and everything is allocated, before the first write.
 * VICGPU_ERR_ARG: a null handle; nrow < 0 or ndst < 0; null lists with work to do; a row out of range or listed twice; a
 * destination out of range or listed twice; term_off[0] != 0 or decreasing offsets; a destination with no term; a term cell
 * out of range; a weight that is not finite; an incompatible destination / term pair (vicgpu_last_error names the destination
 * and the term); VICGPU_ERR_STATE: no domain; VICGPU_ERR_HIP: the runtime refused an allocation -- nothing is left behind. */
int vicgpu_mix_cells(vicgpu_ctx *ctx, int nrow, const int *rows,
                     int ndst, const int *dst_cell,
                     const int *term_off,        /* [ndst+1], term_off[0] = 0, non-decreasing; nnz = term_off[ndst] */
                     const int *term_cell,       /* [nnz], each in [0, ncell) */
                     const double *term_weight); /* [nnz], finite */

/* ---- the per-column ensemble transform solved and applied on the device: the analysis of a localised filter (LETKF, Hunt et
 * al. 2007), one transform per base column, without an eigendecomposition on the host and without term lists.
 * Layout: the ensemble is member-major (domain.tile_members): ncell == nmember * ncol, and cell m * ncol + j is member m of base
 * column j.  T[j][m'][m] is the weight of forecast member m' in analysis member m of column j.
 * Lifetime: the context holds one stored transform, in device memory.  solve and set replace it, vicgpu_set_domain and
 * vicgpu_destroy drop it, get and apply without one return VICGPU_ERR_STATE.
 *   vicgpu_member_transform_solve   computes T_j for every column from the members' observation-space values.  For column j
 *       with the observations p in [obs_off[j], obs_off[j + 1]), M = nmember and rho = infl[j]:
 *         ybar_p = (sum over m of hx[p][m]) / M,  Y_p[m] = hx[p][m] - ybar_p,  d_p = yobs[p] - ybar_p,
 *         C[a][b] = sum over p of (rinv_p * Y_p[a]) * Y_p[b],  g[a] = sum over p of (rinv_p * Y_p[a]) * d_p,
 *         A = C + ((M - 1) / rho) I = U diag(lam) U^T,  wbar = U diag(1 / lam) U^T g,  Wa = U diag(sqrt((M - 1) / lam)) U^T,
 *         W[m'][m] = Wa[m'][m] + wbar[m'],  T[m'][m] = W[m'][m] + (1 - sum over m'' of W[m''][m]) / M.
 *       The last term folds "about the ensemble mean" into a pure member mix: x_a[m] = sum over m' of T[m'][m] * x_f[m'] is the
 *       LETKF analysis, and every column of T sums to 1.  The eigen-solver is a batched parallel cyclic Jacobi iteration, one
 *       wave per column.  Guaranteed: (a) the result is bit-identical from run to run; (b) T_j does not depend on which other
 *       columns are in the call; (c) a column with no observation, or with every rinv == 0, performs no rotation and gives
 *       exactly sqrt(rho) * I + (1 - sqrt(rho)) / M -- with rho == 1 the exact identity, which leaves finite state
 *       bit-identical (but for a -0.0, which the zero terms of the sum turn into +0.0); (d) a column that has not converged after VICGPU_TRANSFORM_SWEEPS sweeps (a tuning variable, default
 *       30) gets the exact identity and info[j] = -1, and the call still returns VICGPU_OK.  Beyond these the bits of T are
 *       not part of the contract; its accuracy is (that of a float64 LAPACK evaluation of the formulas).  info[j] otherwise
 *       counts the sweeps that rotated.  The solve touches no model table.
 *   vicgpu_member_transform_set     stores the caller's T.
 *   vicgpu_member_transform_get     the sizes and, unless T is NULL, the stored transform.
 *   vicgpu_member_transform_apply   applies the stored transform to the listed rows of the SD table for the listed base columns
 *       (cols NULL: all, n must be ncol).  The members of a listed column must satisfy the pair rule of vicgpu_copy_cells.
 *       Arithmetic (part of the contract): vicgpu_mix_cells' own.  For destination member m, column j, HRU position k and a
 *       listed row, p = T[j][0][m] * x_0, then p = p + T[j][m'][m] * x_m' for m' = 1 .. M - 1, every product and every sum
 *       rounded once; a zero weight still reads its operand; all sources are read before any destination is written.  The call
 *       equals vicgpu_mix_cells with the lists of domain.member_transform(M, ncol, T, cols) bit for bit, NaNs by position.
 *       Untouched tables, stream order and staging (row passes within VICGPU_COPY_STAGE_MB, the result independent of the
 *       budget) are vicgpu_mix_cells' as well.  nrow == 0 and n == 0 are legal and change nothing.
 * Every list is checked, and everything is allocated, before the first write; a failing call leaves every table and the stored
 * transform bit-identical.
 * VICGPU_ERR_ARG: a null handle; nmember outside [2, VICGPU_TRANSFORM_MAX_MEMBERS]; ncol < 1 or nmember * ncol != ncell; null
 * lists with work to do; obs_off[0] != 0 or decreasing offsets; a non-finite hx, yobs, rinv, infl or T; rinv < 0 or infl <= 0;
 * a row out of range or listed twice; a column out of range or listed twice; members of a listed column that break the pair
 * rule (vicgpu_last_error names the column and the member); VICGPU_ERR_STATE: no domain; get or apply without a stored
 * transform; VICGPU_ERR_HIP: the runtime refused an allocation -- nothing is left behind. */
#define VICGPU_TRANSFORM_MAX_MEMBERS 64
int vicgpu_member_transform_solve(vicgpu_ctx *ctx, int nmember, int ncol,
        const int *obs_off,     /* [ncol+1], obs_off[0] = 0, non-decreasing; nobs = obs_off[ncol] */
        const double *hx,       /* [nobs][nmember]  H x of every member, finite */
        const double *yobs,     /* [nobs]           the observation, finite */
        const double *rinv,     /* [nobs]           1 / error variance times the localisation taper; finite, >= 0 */
        const double *infl,     /* [ncol] or NULL (= 1.0): multiplicative covariance inflation rho_j, finite, > 0 */
        int *info);             /* [ncol] or NULL: sweeps the column took (>= 0), or -1: not converged */
int vicgpu_member_transform_set(vicgpu_ctx *ctx, int nmember, int ncol, const double *T); /* [ncol][nmember][nmember], finite */
int vicgpu_member_transform_get(vicgpu_ctx *ctx, int *nmember, int *ncol, double *T);     /* T may be NULL: sizes only */
int vicgpu_member_transform_apply(vicgpu_ctx *ctx, int nrow, const int *rows, int n, const int *cols); /* cols NULL: all, n must be ncol */

/* ---- plumbing for callers that own device memory / streams --------------- */
int   vicgpu_set_stream(vicgpu_ctx *ctx, void *hip_stream);       /* compute stream; NULL = library-owned */
int   vicgpu_set_write_fluxes(vicgpu_ctx *ctx, int on);           /* 0: skip the per-HRU flux table (accumulators still kept) */
void *vicgpu_device_ptr(vicgpu_ctx *ctx, int which);              /* VICGPU_PTR_* */
enum { VICGPU_PTR_STATE_D = 0, VICGPU_PTR_STATE_I, VICGPU_PTR_FLUX, VICGPU_PTR_FORCING, VICGPU_PTR_ACCUM, VICGPU_PTR_CELL_OUT };
/* ---- glacier mass balance: what accumulateGlacierMassBalance.c:53-66 does when an
 * accumulation interval ends (the date test stays with the driver, like the opening of the
 * window): per cell the quadratic best fit of the accumulated mass balance of its glacier
 * HRUs against band elevation (GlacierMassBalanceResult.c:34-73, GraphingEquation.c:8-125;
 * 1 point: constant, 2 points: line), then -- if reset -- cum_mass_balance = 0 for every
 * glacier HRU (resetAccumulationValues).  eq: double[GMB_NROW][ncell]; cells without a
 * valid point get the default equation (0, 0, 0, fitError -1). */
enum { GMB_B0 = 0, GMB_B1, GMB_B2, GMB_FIT_ERROR, GMB_NROW };
int   vicgpu_glacier_mass_balance_fit(vicgpu_ctx *ctx, double *eq, int reset);

/* ---- test hook: the pure functions of the path, evaluated one by one ----------
 * (SURVEY.md 8(c) fixture plan (i)).  in: double[n][VICGPU_PURE_NIN], out: double[n].
 * Functions that read cell parameters or options use cell 0 of the domain and the
 * context's options.  The reference harness (oracle/ref_build) and the oracle
 * export the same hook as vicref_pure / vicorc_pure. */
enum {
  VICGPU_PURE_SVP = 0,            /* svp.c:7: T */
  VICGPU_PURE_SVP_SLOPE,          /* svp.c:26: T */
  VICGPU_PURE_CALC_RAINONLY,      /* calc_rainonly.c:12: air_temp, prec, MAX_SNOW_TEMP, MIN_RAIN_TEMP */
  VICGPU_PURE_SNOW_ALBEDO,        /* snow_utility.c:229: new_snow, swq, depth, albedo, cold_content, dt, last_snow, MELTING */
  VICGPU_PURE_NEW_SNOW_DENSITY,   /* snow_utility.c:199: air_temp */
  VICGPU_PURE_STABILITY,          /* StabilityCorrection.c:44: Z, d, TSurf, Tair, Wind, Z0 */
  VICGPU_PURE_PENMAN,             /* penman.c:96: tair, elevation, rad, vpd, ra, rc, rarc */
  VICGPU_PURE_CALC_RC,            /* penman.c:44: rs, net_short, RGL, tair, vpd, lai, gsm_inv, ref_crop */
  VICGPU_PURE_ESTIMATE_T1,        /* estimate_T1.c:8: Ts, T1_old, T2, D1, D2, kappa1, kappa2, Cs2 (Cs1 is unused: = Cs2), dp, delta_t */
  VICGPU_PURE_SOIL_CONDUCTIVITY,  /* soil_conduction.c:7: moist, Wu, soil_dens_min, bulk_dens_min, quartz, soil_density, bulk_density, organic */
  VICGPU_PURE_VOL_HEAT_CAPACITY,  /* soil_conduction.c:108: soil_fract, water_fract, ice_fract, organic_fract */
  VICGPU_PURE_MAX_UNFROZEN_WATER, /* soil_conduction.c: T, max_moist, bubble, expt */
  VICGPU_PURE_LINEAR_INTERP,      /* x, lx, ux, ly, uy */
  VICGPU_PURE_VEG_HEIGHT,         /* calc_veg_params.c:26: displacement, L (NaN for L = 0) */
  VICGPU_PURE_NFN,
  /* device-only hook (no reference counterpart, not part of the golden vectors): soil_conductivity with the layer
   * constants the library derives once per domain (cell 0): moist, Wu, layer.  Must equal VICGPU_PURE_SOIL_CONDUCTIVITY
   * fed with that layer's parameters, bit for bit. */
  VICGPU_PURE_SOIL_CONDUCTIVITY_DERIVED = VICGPU_PURE_NFN,
  /* device-only: the math the frozen-node root finder rests on (vic_math.hpp) */
  VICGPU_PURE_LN_POS,             /* x */
  VICGPU_PURE_POW_POS,            /* x, y (with its library fallback outside 0 < x < 1e300) */
  VICGPU_PURE_POW_POS_APPROX,     /* x, y (y rounded to float as the predictor does) */
  VICGPU_PURE_RCP_REFINED,        /* d */
  VICGPU_PURE_NFN_DEVICE
};
#define VICGPU_PURE_NIN 10
int   vicgpu_debug_pure(vicgpu_ctx *ctx, int fn, int n, const double *in, double *out);

/* ---- test hook: one Gauss-Seidel visit of one frozen-soil node -----------------
 * The node's root find of the profile kernels (node_visit, vic_profile.hpp) for n
 * independent cases, on the record profile_item_store folds from the same inputs.
 * in: double[n][VICGPU_NODE_NIN] in the reference's terms (soil_thermal_eqn.c):
 *   A, B, C, D, E, T0, ice0, moist, max_moist, bubble, expt, TL, TU, oldT (the current iterate);
 * out: double[n][VICGPU_NODE_NOUT]: T, failed (1: the reference's root finder returns ERROR).
 * mode: an OR of the VICGPU_NODE_* bits, one value for the whole launch. */
enum { VICGPU_NODE_NODE1 = 1, VICGPU_NODE_NEWTON = 2, VICGPU_NODE_EXP_TRANS = 4 };
#define VICGPU_NODE_NIN 14
#define VICGPU_NODE_NOUT 2
int   vicgpu_debug_node_root(vicgpu_ctx *ctx, int mode, int n, const double *in, double *out);

/* ---- test hook: replay a recorded root find -------------------------------------
 * The model's root finders (vic_math.hpp) for n independent cases, one lane each:
 * mode 0 Brent (the surface, snow, canopy and glacier solves), mode 1 BrentLean (the
 * frozen-node visits).  Lane i starts from bounds[i][0], bounds[i][1]; at its k-th
 * residual request it writes the abscissa to xreq[off[i] + k] and is given
 * fvals[off[i] + k] instead of a residual evaluation.  off: int[n + 1], off[0] = 0,
 * non-decreasing; fvals and xreq hold off[n] values.
 * out: double[n][VICGPU_BRENT_NOUT]: values consumed, finished, failed, result (ERROR
 * on failure), the counters i, j, k, which_err (BrentLean: k = which_err = 0), and
 * overrun (1: the lane asked for more values than off[i + 1] - off[i]). */
enum { VICGPU_BRENT_FULL = 0, VICGPU_BRENT_LEAN = 1 };
#define VICGPU_BRENT_NOUT 9
int   vicgpu_debug_root_brent(vicgpu_ctx *ctx, int mode, int n, const double *bounds, const int *off, const double *fvals,
                              double *xreq, double *out);

/* GPU time (ms) per model step of the last vicgpu_step call, measured with
 * hipEvents on the library's streams: QUICK_FLUX: the step's HRU kernel, one
 * event pair per step; finite-difference pipeline: all kernels of all steps
 * of the call divided by the number of steps.  *nlaunch = steps covered. */
int   vicgpu_last_kernel_ms(vicgpu_ctx *ctx, double *ms_per_launch, int *nlaunch);

#ifdef __cplusplus
}
#endif
#endif /* VICGPU_H_ */
