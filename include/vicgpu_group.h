/*
 * vicgpu_group.h — several GPUs driven from one process: a device group.
 *
 * The reference's driver is one process (vicNl.c:506-610: the loop over cells, then write_data_all_cells).  A single
 * context (vicgpu.h) drives one device.  A group owns N shard contexts of ONE domain and takes and returns every table in
 * the caller's global layout, so a driver written against a single context changes only the handle type:
 *
 *     vicgpu_ctx *c;   vicgpu_create(&opt, 0, &c);          vicgpu_set_domain(c, ...);   vicgpu_step(c, 0, n);
 *     vicgpu_group *g; vicgpu_group_create(&opt, 8, 0, &g); vicgpu_group_set_domain(g, ...); vicgpu_group_step(g, 0, n);
 *
 * Shards.  vicgpu_group_set_domain cuts the domain into nshard contiguous cell blocks [b[k], b[k+1]) of near-equal HRU count
 * (vicgpu_group_partition, the same rule as vic_amd/shard.py partition_cells).  Shard k holds those cells and their HRUs in
 * the domain's HRU order restricted to the block, renumbered from 0; its cell_hru_list is the block's part of the caller's,
 * renumbered the same way.  Every shard must get at least one cell.
 *
 * Tables.  Per-HRU tables (state, fluxes: [nrow][nhru]) are in the caller's HRU numbering and are split / merged on the host.
 * Per-cell tables (forcing, raw forcing, output floats, balance, cell error flags, glacier fit) are the caller's
 * [..][ncell] tables: each shard's columns go to and from the caller's buffer by pitched copies, directly from and into
 * pinned memory (vicgpu_host_alloc).  State records ([nhru][VICGPU_SR_LEN], cell-major hruList order) are the shards'
 * record streams concatenated in shard order.
 *
 * Threads.  The group has one persistent host thread per shard; each entry runs the shards' calls on them at the same
 * time and returns when all have returned.  A finite-difference vicgpu_step blocks for most of the run time, so the shards
 * only overlap because of these threads.  With QUICK_FLUX vicgpu_group_step only enqueues; vicgpu_group_synchronize waits.
 * Like a context, a group is not thread-safe: one caller thread at a time.
 *
 * Errors.  The codes of vicgpu.h.  When a shard fails, the entry returns the first failing shard's code and
 * vicgpu_group_last_error reads "shard k (device d): <the context's message>".
 */
#ifndef VICGPU_GROUP_H_
#define VICGPU_GROUP_H_

#include "vicgpu.h"
#include "vicgpu_out.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vicgpu_group vicgpu_group;

/* The shard boundaries bounds[nshard+1] of a domain given by its CSR offsets cell_hru_offset[ncell+1]: bounds[0] = 0,
 * bounds[nshard] = ncell and, for 0 < r < nshard, the first cell c with cell_hru_offset[c] >= nhru * r / nshard, clamped to
 * [bounds[r-1], ncell].  Pure host function, no device needed.  VICGPU_ERR_ARG for nshard < 1 or nshard > ncell. */
int  vicgpu_group_partition(int ncell, const int *cell_hru_offset, int nshard, int *bounds);

/* nshard contexts with the same options; devices[nshard] may repeat an index (several shards on one device), NULL means
 * 0 .. nshard-1.  A device index outside hipGetDeviceCount is VICGPU_ERR_ARG; options vicgpu_create refuses are refused
 * with its code.  On failure nothing is left behind (*out = NULL). */
int  vicgpu_group_create(const vicgpu_options *opt, int nshard, const int *devices, vicgpu_group **out);
void vicgpu_group_destroy(vicgpu_group *g);
const char *vicgpu_group_last_error(const vicgpu_group *g);
int  vicgpu_group_shard_bounds(vicgpu_group *g, int *bounds);          /* [nshard+1], after vicgpu_group_set_domain */
vicgpu_ctx *vicgpu_group_shard_ctx(vicgpu_group *g, int k);           /* shard k's context (tuning, debug and stream entries) */

/* the entries of vicgpu.h / vicgpu_out.h on the whole domain, tables in the caller's global layout */
int vicgpu_group_set_veglib(vicgpu_group *g, int nrow, const double *veglib);
int vicgpu_group_set_domain(vicgpu_group *g, int ncell, int nhru, const double *cell_params, const int *hru_iparams,
                            const double *hru_dparams, const int *cell_hru_offset, const int *cell_hru_list);
int vicgpu_group_set_state(vicgpu_group *g, const double *state_d, const int *state_i);
int vicgpu_group_get_state(vicgpu_group *g, double *state_d, int *state_i);
int vicgpu_group_set_fluxes(vicgpu_group *g, const double *flux);
int vicgpu_group_get_fluxes(vicgpu_group *g, double *flux);
int vicgpu_group_push_forcing(vicgpu_group *g, int nsteps, const double *forcing, const unsigned char *snowflag, const int *dmy);
int vicgpu_group_prefetch_forcing(vicgpu_group *g, int nsteps, const double *forcing, const unsigned char *snowflag,
                                  const int *dmy);
int vicgpu_group_prefetch_forcing_raw(vicgpu_group *g, int nsteps, const double *raw, const int *dmy, double min_wind_speed,
                                      int plapse);
/* vicgpu_prefetch_forcing_perturbed (vicgpu.h) with col_src[ncol] and col_group[ncol] in the caller's global column order; the
 * whole call is checked on the whole domain before any shard uploads.  Shard k takes the forcing-column range it already holds
 * (from column lo_k on) and uploads the range of source columns those columns name, as the same pitched copy with leading
 * dimension nsrc; its col_src is rebased by that range's start.  Group numbers are not rebased: pert goes to every shard whole. */
int vicgpu_group_prefetch_forcing_perturbed(vicgpu_group *g, int nsteps, int nsrc, const double *raw, const int *col_src,
                                            int ngroup, const int *col_group, const double *pert, const int *dmy,
                                            double min_wind_speed, int plapse);
int vicgpu_group_swap_forcing(vicgpu_group *g);
/* forcing map (vicgpu.h): cell_col[ncell] in the caller's global cell order, the forcing and raw tables of the entries above
 * then ncol wide, the flags ncell wide.  Shard k takes the column range [lo_k, hi_k] its cells span, with its own map rebased
 * by lo_k: its uploads are the same pitched copies, leading dimension ncol, from column lo_k, hi_k - lo_k + 1 wide.
 * vicgpu_group_set_domain resets the map to the identity; so does a call that fails in a shard (VICGPU_ERR_HIP). */
int vicgpu_group_set_forcing_map(vicgpu_group *g, int ncol, const int *cell_col);
int vicgpu_group_get_forcing_map(vicgpu_group *g, int *ncol, int *cell_col);   /* cell_col may be NULL: ncol only */
int vicgpu_group_step(vicgpu_group *g, int step0, int nsteps);
int vicgpu_group_synchronize(vicgpu_group *g);
int vicgpu_group_put_data_config(vicgpu_group *g, int out_step_ratio);
int vicgpu_group_put_data_init(vicgpu_group *g);
int vicgpu_group_get_outputs(vicgpu_group *g, int nvar, const int *var_ids, float *out, int reset);
int vicgpu_group_get_balance(vicgpu_group *g, double *pb);
int vicgpu_group_get_cell_errors(vicgpu_group *g, int *flags);
/* cell validity (vicgpu.h): the mask goes to every shard; the validity table is in the caller's global cell order and
 * moves like the cell error flags */
int vicgpu_group_set_retire_on_error(vicgpu_group *g, int mask);
int vicgpu_group_set_cell_valid(vicgpu_group *g, const int *valid);
int vicgpu_group_get_cell_valid(vicgpu_group *g, int *valid);
/* vicgpu_copy_cells (vicgpu.h) with cell indices in the caller's global order.  The contract is the same and holds across the
 * whole group: a pair whose cells lie in different shards is legal (the fan-out from member 0 of a sharded ensemble always
 * has such pairs), every pair is checked before any shard writes, and every source is read before any destination is
 * written -- per table and row pass every shard first packs what leaves its cells into an export buffer, then, once all have,
 * fetches what it imports by plain device-to-device copies (no peer access is enabled, no kernel reads another device's
 * memory) and unpacks it.  The call returns when the copy has been made.  Errors: as vicgpu_copy_cells, and the rule for shard
 * failures above.  Copies between distinct devices have only been exercised as several shards on one device. */
int vicgpu_group_copy_cells(vicgpu_group *g, int n, const int *dst_cell, const int *src_cell, int what);
/* vicgpu_update_cell_params / vicgpu_update_hru_params (vicgpu.h) with cell / HRU indices in the caller's global order, and
 * the getters in the caller's global layout.  The contract is the same: the whole call is checked on the whole domain before
 * any shard writes; then every shard takes its own columns, rebased, on the group's threads.  The dense form (a NULL list)
 * needs n == ncell / nhru of the whole domain.  Errors: as the context entries, and the rule for shard failures above -- a
 * shard whose allocation the runtime refuses (VICGPU_ERR_HIP) is itself unchanged, the others have taken their columns. */
int vicgpu_group_update_cell_params(vicgpu_group *g, int nrow, const int *rows, int n, const int *cells, const double *values);
int vicgpu_group_update_hru_params(vicgpu_group *g, int nrow, const int *rows, int n, const int *hrus, const double *values);
int vicgpu_group_get_cell_params(vicgpu_group *g, double *cell_params);
int vicgpu_group_get_hru_params(vicgpu_group *g, double *hru_dparams);
/* vicgpu_get_state_rows / vicgpu_update_state / vicgpu_derive_soil_state and the int forms (vicgpu.h) with HRU indices in the
 * caller's global numbering.  The contract is the same: the whole call is checked on the whole domain before any shard writes;
 * then every shard takes its own columns, rebased, on the group's threads, and the get forms merge into the caller's
 * [nrow][n] buffer in list order.  The dense form needs n == nhru of the whole domain.  Errors: as the context entries, and the
 * rule for shard failures above -- a shard whose allocation the runtime refuses is itself unchanged, the others have run. */
int vicgpu_group_get_state_rows(vicgpu_group *g, int nrow, const int *rows, int n, const int *hrus, double *values);
int vicgpu_group_get_state_rows_i(vicgpu_group *g, int nrow, const int *rows, int n, const int *hrus, int *values);
int vicgpu_group_update_state(vicgpu_group *g, int nrow, const int *rows, int n, const int *hrus, const double *values, int mode);
int vicgpu_group_update_state_i(vicgpu_group *g, int nrow, const int *rows, int n, const int *hrus, const int *values);
int vicgpu_group_derive_soil_state(vicgpu_group *g, int n, const int *hrus, int what);
/* vicgpu_mix_cells (vicgpu.h) has no group form: under the group's contiguous sharding the members of a member-major ensemble
 * lie on different devices, so a transform would be an all-to-all between shards with a summation order of its own, which is a
 * decision of its own.  A shard's context (vicgpu_group_shard_ctx) takes vicgpu_mix_cells in its local numbering.
 * vicgpu_member_transform_solve, vicgpu_member_transform_set, vicgpu_member_transform_get and vicgpu_member_transform_apply
 * (vicgpu.h) have no group form for the same reason: a column's members would lie on different devices. */
int vicgpu_group_get_state_records(vicgpu_group *g, double *records);
int vicgpu_group_set_state_records(vicgpu_group *g, const double *records);   /* checks every record before any shard scatters */
int vicgpu_group_glacier_mass_balance_fit(vicgpu_group *g, double *eq, int reset);
/* the record entries of vicgpu_out.h: out [nrecords][nrow][ncell] and cell_err [nrecords][ncell] are the caller's global
 * tables in pinned memory, every shard delivers its own columns by pitched copies; wait(k) waits for every shard.
 * The cell groups of vicgpu_records_set_groups have no group form: a group of cells that spans shards would need a summation
 * order across devices, which is a decision of its own.  vicgpu_group_run_records returns VICGPU_ERR_STATE when a shard's
 * context (vicgpu_group_shard_ctx) has groups set. */
int vicgpu_group_records_config(vicgpu_group *g, int nvar, const int *var_ids, int depth);
int vicgpu_group_records_nrow(vicgpu_group *g);
int vicgpu_group_run_records(vicgpu_group *g, int step0, int nrecords, float *out, int *cell_err);
int vicgpu_group_records_wait(vicgpu_group *g, int k);

#ifdef __cplusplus
}
#endif
#endif /* VICGPU_GROUP_H_ */
