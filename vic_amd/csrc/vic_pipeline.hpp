// vic_pipeline.hpp — the host pipeline: the context (vicgpu_ctx), its tuning variables (Tuning), what lives as long as a
// domain (Domain, FdChunk) and the steps of vicgpu_set_domain that fill it, the kernel-argument structs filled from them,
// the launchers, the step of the finite-difference pipeline (fd_step: the round loop; fd_chunk_run: all steps of one
// vicgpu_step or vicgpu_run_records call for one cell chunk) and the end of an output record (Records, records_emit).
// Host code only, no kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <vector>
#include "vicgpu.h"
#include "vic_profile.hpp"
#include "vic_putdata.hpp"
#include "vic_host.hpp"
#include "vic_implicit.hpp"
#include "vic_ctx.hpp"
#include "vic_hru_io.hpp"
#include "vic_kernels.hpp"
#include "vic_aux_kernels.hpp"
#include "vic_records.hpp"
#include "vic_copy_cells.hpp"
#include "vic_params.hpp"
#include "vic_state_update.hpp"
#include "vic_mix_cells.hpp"
#include "vic_member_transform.hpp"

using namespace vic;

#define HIPIGN(call) do { hipError_t ign_ = (call); (void)ign_; } while (0)
#define HIPCHK(ctx, call)                                                                              \
  do {                                                                                                 \
    hipError_t e_ = (call);                                                                            \
    if (e_ != hipSuccess) {                                                                            \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                                  \
      return VICGPU_ERR_HIP;                                                                           \
    }                                                                                                  \
  } while (0)

// ------------------------------------------------------------------------------------------------ context
// A chunk of cells with all their HRUs.  Cells never interact, so every chunk runs the whole step sequence on its own
// stream, driven by its own host thread: while one chunk is in the thin tail of its Brent rounds (a few stragglers,
// latency bound) or in a stage kernel (memory / latency bound), the profile solves of the others fill the SIMDs.
// The host reads the round's list sizes back RB_LAG rounds late (fd_step): it stays that many rounds ahead of the device, so the
// thin tail rounds -- two short kernels each -- never wait for a host round trip; the price is RB_LAG rounds on empty lists at
// the end of the iteration (both kernels return at once).
constexpr int RB_LAG = 3, RB_DEPTH = RB_LAG + 1;
struct FdChunk {
  int c0 = 0, ccount = 0;          // cells [c0, c0 + ccount)
  DevBuf<int> d_glist;             // their HRUs, ascending
  int gcount = 0;
  LaunchMap map;                   // XCD-aware launch order when the chunk's list is regular (slot-major, every slot ccount cells)
  DevBuf<int> d_list[2];           // work lists (HRU ids)
  DevBuf<int> d_fb_list, d_fb_count;   // IMPLICIT: HRUs whose Newton iteration failed this round
  DevBuf<int> d_count;             // counter block (CNT_*): segment sizes of the two lists, profile cursor, pending total and prefix, stripe fills
  DevBuf<int> d_plist[2];          // flat pending lists: PEND_STRIPES stripes of pend_cap entries
  int list_cap = 0;                // entries per segment
  int pend_cap = 0;                // entries per stripe
  PinnedBuf<int> h_count;          // pinned read-back, RB_DEPTH slots of CNT_TOTAL
  Stream stream;
  Event done, readback[RB_DEPTH];
  std::string err;
  int status = 0;
  long long rounds = 0, steps = 0;
};

// Everything that lives exactly as long as a domain: vicgpu_set_domain builds it, free_domain drops it as a whole
struct Domain {
  int ncell = 0, nhru = 0;
  bool domain_ready = false;       // set at the end of a successful vicgpu_set_domain
  bool any_glacier = false;
  DevBuf<double> d_cp, d_hpd, d_sd, d_flux, d_cell_out, d_accum;
  DevBuf<int> d_hpi, d_si, d_cell_off, d_cell_list, d_hru_err, d_cell_err;
  // cell validity (vicgpu_set_cell_valid, vicgpu_set_retire_on_error): the words CELL_* of vic_types.hpp, all CELL_VALID after
  // vicgpu_set_domain.  valid_live: a word may differ from CELL_VALID -- the host has marked a cell invalid, or steps have run
  // with a retire mask; until then the kernels get a null table (valid_table) and take no load for it
  DevBuf<int> d_valid;
  bool valid_live = false;
  // forcing map (vicgpu_set_forcing_map): cell -> forcing column.  Identity after vicgpu_set_domain: ncol == ncell, no buffer,
  // and the kernels take the HPI_CELL row as the HRUs' column row (forcing_col_row).  With a map: the host copy, its device
  // copy for the kernels whose lane is a cell, and the derived row cell_col[HPI_CELL] for those whose lane is an HRU
  int ncol = 0;
  std::vector<int> cell_col;       // empty: identity
  DevBuf<int> d_cell_col;          // [ncell]
  DevBuf<int> d_hru_fcol;          // [nhru]
  // host copies for vicgpu_copy_cells, which plans on the host: the CSR lists and the HRU rows a pair of cells must agree in
  // (COPY_KEY_ROWS), [COPY_NKEY][nhru]
  std::vector<int> cell_off, cell_list, copy_key;
  std::vector<int> cell_class;     // [ncell] copy_cell_classes of them, built by the first vicgpu_mix_cells of the domain
  MixPlan mix_plan;                // ... and the plan of its last one, whose memory the next one reuses
  // the stored member transform (vicgpu_member_transform_solve / _set): [tf_ncol][tf_nmember][tf_nmember], empty when there is none
  int tf_nmember = 0, tf_ncol = 0;
  DevBuf<double> d_transform;
  TransformPlan transform_plan;    // the plan of the last vicgpu_member_transform_apply, reused like mix_plan
  // finite-difference pipeline workspace (allocated when QUICK_FLUX is off)
  bool fd = false;
  DevBuf<unsigned long long> d_ctx;
  DevBuf<double> d_pin, d_ts, d_pout;
  DevBuf<int> d_hstate, d_pslot, d_hkey, d_lastexp, d_jl;
  DevBuf<double> d_pimp;           // IMPLICIT only
  std::vector<FdChunk> chunks;     // cell chunks, each an independent pipeline on its own stream
  // put_data (vicgpu_out.h): output tables [nrow][ncell], allocated by vicgpu_put_data_config
  bool put_on = false;
  int out_nrow = 0;
  OutLayout out_lay;
  DevBuf<double> d_out_data, d_out_agg, d_pb;
  DevBuf<unsigned char> d_rowagg;  // [out_nrow] aggregation type of every output row
};

// the HRU parameter rows in which the cells of a vicgpu_copy_cells pair must agree, position by position
constexpr int COPY_NKEY = 4;
constexpr int COPY_KEY_ROWS[COPY_NKEY] = {HPI_BAND, HPI_VEG_CLASS, HPI_IS_GLACIER, HPI_IS_ARTIFICIAL_BARE};

// The tuning variables of the environment: overrides for A/B runs, profiles and traces, not API (table in DESIGN.md (d)).
// Read once per vicgpu_set_domain, so a domain runs on what the environment said when it was set, and a second
// vicgpu_set_domain starts from the defaults again.
struct Tuning {
  bool node_newton = false;        // VICGPU_NODE_SOLVER = "newton": the safeguarded Newton node root finder; default options.NODE_SOLVER
  int eval_list_pct = 75;          // VICGPU_EVAL_LIST_PCT, 0..100: sparse evaluation rounds once at most this share of the HRUs is pending; 0 = never
  int nchunk = 1;                  // VICGPU_CHUNKS, 1..16 and at most ncell: cell chunks as independent pipelines; default 2 from 20 000 cells up
  int profile_waves_pct = 100;     // VICGPU_PROFILE_WAVES_PCT, 5..100: a chunk's profile kernel's share of the resident wave slots; default 50 with chunks
  bool xcd_map = true;             // VICGPU_NO_XCD_MAP (set): plain instead of XCD-aware launch order
  bool trace_rounds = false;       // VICGPU_TRACE_ROUNDS (set): what every round leaves pending (a host round trip per round)
  bool trace = false;              // VICGPU_TRACE (set): per-step wall time and Brent rounds (a wait per step)
  bool stats = false;              // VICGPU_STATS (set): Brent rounds per step of every chunk, printed by vicgpu_destroy; the record groups' reduce time
  int copy_stage_mb = 256;         // VICGPU_COPY_STAGE_MB, 0..65536: staging memory of a vicgpu_copy_cells call on the staged path; 0 = one row per pass
  int transform_sweeps = 30;       // VICGPU_TRANSFORM_SWEEPS, 1..1000: Jacobi sweeps a column of vicgpu_member_transform_solve may take
};
static Tuning read_tuning(int node_solver, int ncell) {
  Tuning t;
  // frozen-node root finder (vic_profile.hpp): the option, overridable for A/B runs
  t.node_newton = node_solver == VIC_NODE_SOLVER_NEWTON;
  if (const char* ev = getenv("VICGPU_NODE_SOLVER")) t.node_newton = (strcmp(ev, "newton") == 0);
  if (const char* ev = getenv("VICGPU_EVAL_LIST_PCT")) {
    const int pct = atoi(ev);
    if (pct >= 0 && pct <= 100) t.eval_list_pct = pct;
  }
  // Cell chunks: every kernel of the pipeline is stalled most of its time (dependent fp64 chains in the profile kernel, memory
  // latency in the others: 15 % VALU-active per wave), so two pipelines side by side fill each other's gaps and thin tail
  // rounds: -6 % step time at 2.5 M HRUs (27.3 vs 29.0 ms, same-box A/B); three or more lose again.  Default: two chunks for
  // domains of 20k cells or more (VICGPU_CHUNKS=1 gives per-kernel profiles whose durations add up to the step).
  t.nchunk = (ncell >= 20000) ? 2 : 1;
  if (const char* ev = getenv("VICGPU_CHUNKS")) t.nchunk = atoi(ev);
  if (t.nchunk < 1) t.nchunk = 1;
  if (t.nchunk > 16) t.nchunk = 16;
  if (t.nchunk > ncell) t.nchunk = ncell;
  // A chunk's profile kernel takes half of the resident wave slots when chunks run side by side, so that the other chunk's
  // kernels find free SIMD slots beside it (26.5 vs 26.9 ms per step with two chunks, same box, both repetitions)
  t.profile_waves_pct = t.nchunk > 1 ? 50 : 100;
  if (const char* ev = getenv("VICGPU_PROFILE_WAVES_PCT")) {
    const int pct = atoi(ev);
    if (pct >= 5 && pct <= 100) t.profile_waves_pct = pct;
  }
  t.xcd_map = getenv("VICGPU_NO_XCD_MAP") == nullptr;
  t.trace_rounds = getenv("VICGPU_TRACE_ROUNDS") != nullptr;
  t.trace = getenv("VICGPU_TRACE") != nullptr;
  t.stats = getenv("VICGPU_STATS") != nullptr;
  // vicgpu_copy_cells, staged path: the rows of a table go through the stage in passes that fit this budget (at least a row)
  if (const char* ev = getenv("VICGPU_COPY_STAGE_MB")) {
    const int mb = atoi(ev);
    if (mb >= 0 && mb <= 65536) t.copy_stage_mb = mb;
  }
  // vicgpu_member_transform_solve: a column still rotating after this many sweeps gets the identity
  if (const char* ev = getenv("VICGPU_TRANSFORM_SWEEPS")) {
    const int n = atoi(ev);
    if (n >= 1 && n <= 1000) t.transform_sweeps = n;
  }
  return t;
}

// Output records (vicgpu_records_config / vicgpu_run_records): the selection, a ring of `depth` device slots and the events
// that order the packing kernel on the stream that ran a record's steps against the slot's copy on the download stream.
// A lane is what delivers columns on its own: the context's stream (QUICK_FLUX) or a cell chunk of the finite-difference
// pipeline.  Lives as long as the put_data configuration it was made for.
// The download stream: with QUICK_FLUX a stream of its own (`dl`; the copy stream carries the next forcing chunk, which would
// delay a record).  In the finite-difference pipeline the context's stream, which is idle while the chunks' streams run the
// steps: a fifth stream made two of them share one of the process's four hardware queues, and the two chunks of a 100k-cell
// domain then ran one after the other (28.9 instead of 22.1 ms per step).
//
// Cell groups (vicgpu_records_set_groups): the record that travels is [nrow][ngroup], reduced from the slot's packed
// [nrow][ncell] by one kernel on the download stream.  A group may span lanes, so record k's reduction is a join: it is
// queued once, behind every lane's `packed` event of record k, by the lane that arrives last (RecordsJoin), followed by one
// contiguous copy and `reduced[k]`.  It reads every lane's columns of the slot, so no lane may pack record k + depth before
// it: a lane that runs ahead waits on the host until the join of record k has been queued, then queues its wait for
// reduced[k].  Each lane still copies its own cell_err columns.

// Host-side order of the lanes around the joins of one vicgpu_run_records call.  hipStreamWaitEvent on an event that has not
// been recorded yet is a no-op, so who queues a join must know that every lane has recorded its `packed` event: the last of
// the nlane arrivals at record k does.  The joins are queued in record order (a lane arrives at k + 1 only after it has left
// k).  A lane that fails releases the others, which return its status.
struct RecordsJoin {
  std::mutex m;
  std::condition_variable cv;
  std::vector<int> arrived;        // [records of the call]: lanes that have queued their part of record k
  int queued = 0;                  // the joins of the records [0, queued) are on the download stream
  int status = 0;                  // != 0: a lane has failed
  std::string err;
  void start(int nrecords) { arrived.assign(nrecords, 0); queued = 0; status = 0; err.clear(); }
  // true for the last of nlane arrivals at record k
  bool arrive(int k, int nlane) { std::lock_guard<std::mutex> lk(m); return ++arrived[k] == nlane; }
  void join_queued(int k) { { std::lock_guard<std::mutex> lk(m); queued = k + 1; } cv.notify_all(); }
  // blocks until the join of record k is queued; the failing lane's status when one has failed
  int wait_queued(int k, std::string* why) {
    std::unique_lock<std::mutex> lk(m);
    cv.wait(lk, [&]() { return queued > k || status != 0; });
    if (status != 0) *why = err;
    return status;
  }
  void fail(int st, const std::string& why) {
    { std::lock_guard<std::mutex> lk(m); if (status == 0) { status = st; err = why; } }
    cv.notify_all();
  }
};

struct Records {
  int nrow = 0, depth = 0;         // rows of a record; depth == 0: not configured
  DevBuf<int> d_sel_pos;           // [out_nrow]: the record row of an aggregate row, or -1
  struct Slot {
    DevBuf<float> d_out;           // [nrow][ncell]
    DevBuf<int> d_err;             // [ncell]
    DevBuf<float> d_group;         // [nrow][ngroup], with groups
  };
  // cell groups: ngroup == 0: none.  CSR over the cells, the weights as given (1.0 where the caller passed none)
  int ngroup = 0, nnz = 0;
  float fill = 0.0f;
  bool lane_per_group = false;     // no group has more than one member: vic_out_group_reduce_lane
  DevBuf<int> d_group_off, d_group_cell;
  DevBuf<double> d_group_weight;
  std::vector<Event> reduced;      // [records of the largest call]: record k's [nrow][ngroup] is in the caller's table
  std::unique_ptr<RecordsJoin> join;
  Event reduce_t0, reduce_t1;      // VICGPU_STATS: around the reduction of a call's last record
  bool reduce_timed = false;       // ... both have been recorded
  std::vector<Slot> slot;
  int nlane = 0;
  std::vector<Event> packed;       // [nlane][depth]: the slot holds the lane's columns of its record
  std::vector<Event> landed;       // [nlane][records of the largest call]: the lane's columns of record k are in the caller's tables
  Stream dl;                       // QUICK_FLUX only
  Event drained;                   // download stream: every copy of the last call has been made
  int last_nrecords = 0;           // of the last vicgpu_run_records; 0: none yet
  bool follows = false;            // the call in flight follows another one, whose copies may still read the slots
  // the call in flight (set by vicgpu_run_records before the lanes start, read by them)
  float* out = nullptr;
  int* err = nullptr;
  int ld = 0;                      // cells per row of out / err
};

struct vicgpu_ctx {
  vicgpu_options opt;
  Opt o;
  int device;
  std::string err;
  Tuning tune;
  int nveg_rows = 0;
  DevBuf<double> d_veglib;
  Domain dom;
  // forcing: d_forcing / d_snowflag / dmy / chunk_steps describe the CURRENT chunk = slot[cur] (views into the slot, which
  // owns the memory and outlives a domain); the other slot takes the prefetch of the next one (vicgpu_prefetch_forcing*,
  // vicgpu_swap_forcing)
  double* d_forcing = nullptr;
  unsigned char* d_snowflag = nullptr;
  std::vector<int> dmy;            // host copy [nsteps][VIC_NDMY]
  int chunk_steps = 0;
  struct ForcingSlot {
    DevBuf<double> d_f, d_raw;     // d_raw: the raw table as uploaded, ncol wide or (vicgpu_prefetch_forcing_perturbed) nsrc wide
    DevBuf<unsigned char> d_s;
    DevBuf<double> d_pert;         // vicgpu_prefetch_forcing_perturbed: the factors and the two lists of the slot's last such call
    DevBuf<int> d_col_src, d_col_group;
    PinnedBuf<char> h_stage;       // pinned staging for pageable sources
    std::vector<int> dmy;
    int nsteps = 0;
    Event uploaded;                // copy stream: the chunk is in the slot
    Event released;                // context stream: every step that read the slot has been queued before it
    bool upload_pending = false, was_current = false;
    Event derive_t0, derive_t1;    // VICGPU_STATS: around the derivation kernels of the slot's last raw prefetch
    bool derive_timed = false;     // ... both have been recorded
  } slot[2];
  int cur = -1, staged = -1;
  Stream stream, copy_stream;      // `stream` may be borrowed (vicgpu_set_stream)
  Records rec;
  std::vector<Event> ev;           // start/stop pairs of the last vicgpu_step call
  int ev_used = 0;
  int write_fluxes = 1;
  int steps_done = 0;
  int profile_waves = 0;           // resident waves of the profile kernel
  int ev_steps = 0;                // steps covered by the event pair of the last vicgpu_step call
  int out_step_ratio = 1;
  int retire_mask = 0;             // vicgpu_set_retire_on_error; a setting of the context, not of the domain
};

// vicgpu_prefetch_forcing_perturbed as one context takes it: `raw` points at the first source column the context uploads, nsrc
// of them, out of a table ld columns wide (a group's shard takes the range its columns name); col_src is in the numbering of
// that table and is rebased by src_base on its way to the device; col_group and pert are never rebased
struct PertLists {
  int nsrc;
  const int* col_src;          // [ncol], or null: column i reads the i-th column uploaded
  int src_base;
  int ngroup;
  const int* col_group;        // [ncol], or null: column i is group group_base + i
  int group_base;
  const double* pert;          // [nsteps][VICGPU_NPERT][ngroup], or null: no perturbation
};

// the validity table as the kernels take it: null while every cell is known to be valid
static int* valid_table(const vicgpu_ctx* c) { return c->dom.valid_live ? c->dom.d_valid.get() : nullptr; }

// the stream that carries the output records to the host (see Records)
static hipStream_t records_stream(const vicgpu_ctx* c) { return c->rec.dl ? (hipStream_t)c->rec.dl : (hipStream_t)c->stream; }

// tuning (VICGPU_STATS): what the reduction over the groups in force took for the last record of the last call; the download
// stream has been waited for
static void records_report_reduce(vicgpu_ctx* c) {
  Records& R = c->rec;
  float ms = 0;
  if (R.reduce_timed && hipEventElapsedTime(&ms, R.reduce_t0, R.reduce_t1) == hipSuccess)
    fprintf(stderr, "[vicgpu] records reduce: %d groups, %d members, a %s per group, %d rows: %.4f ms\n", R.ngroup, R.nnz,
            R.lane_per_group ? "lane" : "wave", R.nrow, ms);
  R.reduce_timed = false;
}

// Drops the records configuration; nothing may be left on the download stream
static void free_records(vicgpu_ctx* c) {
  if (c->rec.depth > 0) HIPIGN(hipStreamSynchronize(records_stream(c)));
  records_report_reduce(c);
  c->rec = Records();
}

// A forcing chunk belongs to the domain and the forcing map it was pushed for (its rows are ncol resp. ncell wide): both
// slots are dropped, their memory stays
static void drop_forcing(vicgpu_ctx* c) {
  c->chunk_steps = 0;
  c->dmy.clear();
  c->cur = c->staged = -1;
  c->d_forcing = nullptr; c->d_snowflag = nullptr;
}

static void free_domain(vicgpu_ctx* c) {
  free_records(c);
  c->dom = Domain();
  drop_forcing(c);
}

// the HRUs' forcing columns as the kernels take them: the derived row of a map, the HPI_CELL row without one
static const int* forcing_col_row(const Domain& d) { return d.d_hru_fcol ? d.d_hru_fcol.get() : d.d_hpi.get() + (size_t)HPI_CELL * d.nhru; }

template <int NN>
static hipError_t launch_hru(const KArgs& ka, hipStream_t st, bool ordinary, bool glacier) {
  const int nblk = ka.map.nblocks(ka.gcount);
  // ordinary HRUs run the monolithic kernel with QUICK_FLUX only (Nnode == 3); the other node counts never instantiate it
  if constexpr (NN == 3) {
    if (ordinary) hipLaunchKernelGGL((vic_hru_step<NN, false>), dim3(nblk), dim3(64), 0, st, ka);
  }
  if (glacier) hipLaunchKernelGGL((vic_hru_step<NN, true>), dim3(nblk), dim3(64), 0, st, ka);
  return hipGetLastError();
}

template <int NN>
static hipError_t launch_fd_stage(const KArgs& ka, bool multi, hipStream_t st) {
  const dim3 grid(ka.map.nblocks(ka.gcount)), block(64);
  if (ka.phase == 0) {
    if (multi) hipLaunchKernelGGL((vic_fd_stage<NN, true, true>), grid, block, 0, st, ka);
    else hipLaunchKernelGGL((vic_fd_stage<NN, true, false>), grid, block, 0, st, ka);
  } else {
    if (multi) hipLaunchKernelGGL((vic_fd_stage<NN, false, true>), grid, block, 0, st, ka);
    else hipLaunchKernelGGL((vic_fd_stage<NN, false, false>), grid, block, 0, st, ka);
  }
  return hipGetLastError();
}

// The profile kernel of a node count: 10 nodes have the register-resident instantiation, every other count a generic one
using ProfileKernel = void (*)(const PArgs);
template <int NN>
constexpr ProfileKernel profile_kernel(bool newton) {
  if constexpr (NN == 10) return newton ? vic_profile_solve_reg<NN, true> : vic_profile_solve_reg<NN, false>;
  else return newton ? vic_profile_solve_lockstep<NN, true> : vic_profile_solve_lockstep<NN, false>;
}

template <int NN>
static hipError_t launch_profile(const PArgs& pa, int nmax, int resident_waves, bool newton, hipStream_t st) {
  int nblk = (nmax + 63) / 64;
  if (nblk > resident_waves) nblk = resident_waves;      // persistent waves pull from the work list
  if (nblk < 1) nblk = 1;                                // block 0 also clears the counters of the round
  hipLaunchKernelGGL(profile_kernel<NN>(newton), dim3(nblk), dim3(64), 0, st, pa);
  return hipGetLastError();
}

template <int NN>
static int profile_resident_waves(int device, bool newton) {
  int per_cu = 0, ncu = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, profile_kernel<NN>(newton), 64, 0);
  if (e != hipSuccess || per_cu <= 0) per_cu = 8;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ncu <= 0) ncu = 256;
  return per_cu * ncu;
}

// Counter block of a chunk.  Every group sits on its own 128-byte lines: the evaluation kernel's waves all read the pending
// count while others append to the next list with atomics, and reads that share a line with those atomics queue behind them
// in the L2 channel (measured: the dense evaluation rounds went from 0.6 to 1.4-2.5 ms when they did).
// The fill counters of the flat pending lists' stripes take a line each (one shared address cost 0.8 ms per step); the
// evaluation waves read the packed prefix of the current list, on lines nobody appends to.  The whole block is read back.
constexpr int CNT_LIST_STRIDE = 64, CNT_CURSOR = 128, CNT_NPEND = 160, CNT_PREFIX = 192, CNT_STRIPES = 288,
              CNT_STRIPES_STRIDE = PEND_STRIPES * PEND_CNT_STRIDE, CNT_TOTAL = CNT_STRIPES + 2 * CNT_STRIPES_STRIDE;
static_assert(NBUCKET <= CNT_LIST_STRIDE && CNT_PREFIX + PEND_STRIPES + 1 <= CNT_STRIPES && CNT_STRIPES % 32 == 0, "counter block layout");
static inline int* cnt_list(int* d_count, int l) { return d_count + l * CNT_LIST_STRIDE; }
static inline int* cnt_stripes(int* d_count, int l) { return d_count + CNT_STRIPES + l * CNT_STRIPES_STRIDE; }
// entries of flat list `l` in a read-back copy of the block
static inline int cnt_pending(const int* h_count, int l) {
  int n = 0;
  for (int s = 0; s < PEND_STRIPES; s++) n += h_count[CNT_STRIPES + l * CNT_STRIPES_STRIDE + s * PEND_CNT_STRIDE];
  return n;
}

// One model step of the finite-difference pipeline for one chunk (see the header of this file).  Blocks the calling
// host thread: the number of Brent rounds is data dependent, so the pending count is read back once the first rounds
// are through.
static int fd_read_count(FdChunk* ch, int which, int* nsolve, int* npending) {
  HIPCHK(ch, hipMemcpyAsync(ch->h_count, ch->d_count, sizeof(int) * CNT_TOTAL, hipMemcpyDeviceToHost, ch->stream));
  HIPCHK(ch, hipStreamSynchronize(ch->stream));
  int n = 0;
  for (int b = 0; b < NBUCKET; b++) n += ch->h_count[which * CNT_LIST_STRIDE + b];
  *nsolve = n;
  *npending = cnt_pending(ch->h_count, which);
  return VICGPU_OK;
}

// F<NN>(args) for the instantiation node count Nnode runs on (node_bound: 10, VIC_MID_NODES or VIC_MAX_NODES)
#define NODE_DISPATCH(Nnode, F, ...)                                                                                          \
  (node_bound(Nnode) == 10 ? F<10>(__VA_ARGS__)                                                                           \
                           : node_bound(Nnode) == VIC_MID_NODES ? F<VIC_MID_NODES>(__VA_ARGS__) : F<VIC_MAX_NODES>(__VA_ARGS__))

// The kernel-argument structs, as far as a domain (and a chunk of it) decides them; the rest stays zero for those who know it:
// the chunk's HRU list (fd_chunk_run), the step's forcing and date (set_step_inputs), the round's work lists and phase (fd_step).
static KArgs make_kargs(const vicgpu_ctx* c) {
  const Domain& d = c->dom;
  KArgs ka{};
  ka.o = c->o; ka.ncell = d.ncell; ka.nhru = d.nhru; ka.gcount = d.nhru; ka.nveg_rows = c->nveg_rows;
  ka.write_fluxes = (c->write_fluxes || d.put_on) ? 1 : 0;      // put_data reads every row of the flux table
  ka.veglib = c->d_veglib; ka.cell_params = d.d_cp; ka.hpi = d.d_hpi; ka.hpd = d.d_hpd; ka.sd = d.d_sd; ka.si = d.d_si; ka.flux = d.d_flux;
  ka.hru_err = d.d_hru_err; ka.ctx = d.d_ctx; ka.pin = d.d_pin; ka.ts = d.d_ts; ka.pout = d.d_pout; ka.pslot = d.d_pslot;
  ka.hstate = d.d_hstate; ka.hkey = d.d_hkey; ka.pimp = d.d_pimp; ka.lastexp = d.d_lastexp; ka.jl = d.d_jl;
  ka.valid = valid_table(c);
  ka.fcol = forcing_col_row(d); ka.ncol = d.ncol;
  return ka;
}
static CArgs make_cargs(const vicgpu_ctx* c) {
  const Domain& d = c->dom;
  CArgs ca{};
  ca.ncell = d.ncell; ca.nhru = d.nhru; ca.ccount = d.ncell; ca.cell_off = d.d_cell_off; ca.cell_list = d.d_cell_list; ca.hpd = d.d_hpd;
  ca.hpi_glac = d.d_hpi + (size_t)HPI_IS_GLACIER * d.nhru; ca.flux = d.d_flux; ca.sd = d.d_sd; ca.hru_err = d.d_hru_err;
  ca.cell_out = d.d_cell_out; ca.accum = d.d_accum; ca.cell_err = d.d_cell_err;
  ca.valid = valid_table(c); ca.retire_mask = c->retire_mask;
  return ca;
}
static PArgs profile_args(const vicgpu_ctx* c, const FdChunk* ch) {
  const Domain& d = c->dom;
  PArgs pa{};
  pa.pin = d.d_pin; pa.ts = d.d_ts; pa.pout = d.d_pout; pa.pslot = d.d_pslot; pa.jl = d.d_jl; pa.cap = ch->list_cap;
  pa.Nn = c->o.Nnode; pa.NOFLUX = c->o.NOFLUX; pa.EXP_TRANS = c->o.EXP_TRANS; pa.TFALLBACK = c->o.TFALLBACK;
  pa.next = ch->d_count + CNT_CURSOR; pa.pend_prefix = ch->d_count + CNT_PREFIX; pa.pend_out = ch->d_count + CNT_NPEND;
  return pa;
}
// ka: the step's stage-kernel arguments, for the forcing rows and the month
static EArgs eval_args(const vicgpu_ctx* c, const FdChunk* ch, const KArgs& ka) {
  const Domain& d = c->dom;
  EArgs ea{};
  ea.o = c->o; ea.ncell = d.ncell; ea.nhru = d.nhru; ea.Nn = c->o.Nnode; ea.glist = ch->d_glist; ea.gcount = ch->gcount; ea.map = ch->map;
  ea.cell_params = d.d_cp; ea.hpi = d.d_hpi; ea.ctx = d.d_ctx; ea.ctx_words = NODE_DISPATCH(c->o.Nnode, ctx_words);
  ea.pout = d.d_pout; ea.pslot = d.d_pslot; ea.ts = d.d_ts; ea.jl = d.d_jl; ea.hstate = d.d_hstate; ea.hkey = d.d_hkey;
  ea.list_cap = ch->list_cap; ea.pend_cap = ch->pend_cap; ea.profile_next = ch->d_count + CNT_CURSOR;
  ea.pend_prefix = ch->d_count + CNT_PREFIX; ea.npend_cur = ch->d_count + CNT_NPEND; ea.implicit = c->o.IMPLICIT;
  ea.veglib = c->d_veglib; ea.forcing = ka.forcing; ea.fcol = ka.fcol; ea.ncol = ka.ncol; ea.month = ka.dmy.month;
  return ea;
}
static IArgs implicit_args(const vicgpu_ctx* c, const FdChunk* ch) {
  const Domain& d = c->dom;
  IArgs ia{};
  ia.ncell = d.ncell; ia.nhru = d.nhru; ia.Nband = c->o.Nband; ia.pimp = d.d_pimp; ia.hpi = d.d_hpi; ia.cell_params = d.d_cp;
  ia.hkey = d.d_hkey; ia.lastexp = d.d_lastexp; ia.fb_list = ch->d_fb_list; ia.fb_count = ch->d_fb_count; ia.cursor = ch->d_fb_count + NBUCKET;
  return ia;
}

static int fd_step(vicgpu_ctx* c, FdChunk* ch, KArgs ka) {
  const int Nn = c->o.Nnode;
  hipStream_t st = ch->stream;
  if (c->dom.any_glacier) HIPCHK(ch, NODE_DISPATCH(Nn, launch_hru, ka, st, false, true));
  HIPCHK(ch, hipMemsetAsync(ch->d_count, 0, sizeof(int) * CNT_TOTAL, st));
  int cur = 0;
  ka.phase = 0; ka.list = ch->d_list[cur]; ka.count = cnt_list(ch->d_count, cur); ka.list_cap = ch->list_cap;
  HIPCHK(ch, NODE_DISPATCH(Nn, launch_fd_stage, ka, c->o.NF > 1, st));
  PArgs pa = profile_args(c, ch);
  EArgs ea = eval_args(c, ch, ka);
  const IArgs ia = c->o.IMPLICIT ? implicit_args(c, ch) : IArgs{};      // the fall-back lists exist with IMPLICIT only
  const int list_thr = (int)((long long)ch->gcount * c->tune.eval_list_pct / 100);
  const int FREE_ROUNDS = 6;       // a Brent solve needs two bracket evaluations, a few iterations and the final evaluation
  const int nsub = c->o.NF;
  for (int p = 1; p <= nsub; p++) {
    int nmax = ch->gcount;
    int npend = -1;                            // upper bound of the evaluations pending (solves + on-record finals), once known
    int rb_list[RB_DEPTH];                     // the list each read-back slot counts
    int rb_first = -1;                         // first round whose counts were read back
    for (int round = 0;; round++) {
      pa.list = ch->d_list[cur]; pa.count = cnt_list(ch->d_count, cur); pa.count_zero = cnt_list(ch->d_count, cur ^ 1);
      pa.pend_counts = cnt_list(ch->d_count, cur); pa.pend_stripes = cnt_stripes(ch->d_count, cur);
      pa.pend_stripes_zero = cnt_stripes(ch->d_count, cur ^ 1);
      if (c->o.IMPLICIT) {
        // the Newton iteration for every listed HRU; those it fails for go on the fall-back list, which the explicit kernel
        // (the same one, on that list) solves right after (func_surf_energy_bal.c:192-222)
        HIPCHK(ch, hipMemsetAsync(ch->d_fb_count, 0, sizeof(int) * (NBUCKET + 1), st));      // the fall-back segments and the work-list cursor
        // persistent waves, a few per SIMD: a lane takes the next solve when its own ends (vic_implicit.hpp)
        const int nblk = std::min(std::max((nmax + 63) / 64, 1), 4096);
        hipLaunchKernelGGL(vic_profile_solve_implicit, dim3(nblk), dim3(64), 0, st, pa, ia);
        HIPCHK(ch, hipGetLastError());
        pa.list = ch->d_fb_list; pa.count = ch->d_fb_count;
      }
      HIPCHK(ch, NODE_DISPATCH(Nn, launch_profile, pa, nmax, c->profile_waves, c->tune.node_newton, st));
      ea.list_next = ch->d_list[cur ^ 1]; ea.count_next = cnt_list(ch->d_count, cur ^ 1);
      ea.pend_list_next = ch->d_plist[cur ^ 1]; ea.pend_count_next = cnt_stripes(ch->d_count, cur ^ 1);
      ea.pend_list_cur = ch->d_plist[cur];
      ea.list_thr = round > 0 ? list_thr : -1;      // the stage kernel before round 0 fills the keyed list only
      // the device switches to the list by itself; once the host knows (RB_LAG rounds late) that it has, the grid shrinks too
      const bool sparse = npend >= 0 && npend <= ea.list_thr;
      hipLaunchKernelGGL(vic_surf_eval, dim3(sparse ? ((npend + 63) / 64 > 0 ? (npend + 63) / 64 : 1) : ea.map.nblocks(ch->gcount)), dim3(64), 0, st, ea);
      HIPCHK(ch, hipGetLastError());
      cur ^= 1;
      ch->rounds++;
      if (c->tune.trace_rounds) {       // tuning: what every round leaves pending (a host round trip per round)
        int n = 0, np = 0;
        if (fd_read_count(ch, cur, &n, &np) != VICGPU_OK) return VICGPU_ERR_HIP;
        fprintf(stderr, "vicgpu rounds: chunk %d sub-step %d round %d leaves %d solves + %d evaluation-only of %d\n", (int)(ch - &c->dom.chunks[0]), p, round, n, np - n, ch->gcount);
      }
      // The list sizes of this round travel to the host behind the kernels just launched; the host looks at the copy issued
      // RB_LAG rounds ago, which has long arrived, so waiting for it never leaves the GPU idle.  The counts only shrink from
      // round to round (an HRU either goes on or is through), so a stale count is a valid upper bound for the grid.
      if (round + 2 >= FREE_ROUNDS) {
        const int slot = round % RB_DEPTH;
        if (rb_first < 0) rb_first = round;
        HIPCHK(ch, hipMemcpyAsync(ch->h_count + slot * CNT_TOTAL, ch->d_count, sizeof(int) * CNT_TOTAL, hipMemcpyDeviceToHost, st));
        HIPCHK(ch, hipEventRecord(ch->readback[slot], st));
        rb_list[slot] = cur;
      }
      if (rb_first >= 0 && round - RB_LAG >= rb_first) {
        const int slot = (round - RB_LAG) % RB_DEPTH;
        HIPCHK(ch, hipEventSynchronize(ch->readback[slot]));
        const int* h = ch->h_count + slot * CNT_TOTAL;
        int n = 0;
        for (int b = 0; b < NBUCKET; b++) n += h[rb_list[slot] * CNT_LIST_STRIDE + b];
        const int np = cnt_pending(h, rb_list[slot]);      // solves + final evaluations on record
        if (np == 0) break;
        nmax = n;
        npend = np;
      }
    }
    ka.phase = p; ka.list = ch->d_list[cur]; ka.count = cnt_list(ch->d_count, cur);
    HIPCHK(ch, NODE_DISPATCH(Nn, launch_fd_stage, ka, c->o.NF > 1, st));
    if (p < nsub) {
      int n = 0, ne = 0;
      const int r = fd_read_count(ch, cur, &n, &ne);
      if (r != VICGPU_OK) return r;
      if (n == 0) break;
    }
  }
  ch->steps++;
  return VICGPU_OK;
}

// put_data for cells [c0, c0 + ccount) after step s of the forcing chunk (s < 0: the initialisation call)
static hipError_t launch_put_data(const vicgpu_ctx* c, hipStream_t st, int c0, int ccount, int s) {
  OArgs a;
  a.o = c->o; a.lay = c->dom.out_lay; a.ncell = c->dom.ncell; a.nhru = c->dom.nhru; a.c0 = c0; a.ccount = ccount;
  a.rec = s < 0 ? -1 : 0; a.out_step_ratio = c->out_step_ratio;
  a.cell_off = c->dom.d_cell_off; a.cell_list = c->dom.d_cell_list; a.cell_params = c->dom.d_cp; a.veglib = c->d_veglib;
  a.hpi = c->dom.d_hpi; a.hpd = c->dom.d_hpd; a.sd = c->dom.d_sd; a.si = c->dom.d_si; a.flux = c->dom.d_flux;
  a.forcing = s < 0 ? nullptr : c->d_forcing + (size_t)s * VIC_NFORCE * (c->o.NR + 1) * c->dom.ncol;
  a.cell_col = c->dom.d_cell_col; a.ncol = c->dom.ncol;
  a.cell_out = c->dom.d_cell_out; a.out_data = c->dom.d_out_data; a.out_agg = c->dom.d_out_agg; a.pb = c->dom.d_pb;
  a.valid = valid_table(c);
  const unsigned nblk = (unsigned)((ccount + 63) / 64);
  // zero_output_list: the columns of these cells in every row
  hipLaunchKernelGGL(vic_put_zero, dim3(nblk, (c->dom.out_nrow + PUT_AGG_ROWS - 1) / PUT_AGG_ROWS), dim3(64), 0, st, a);
  if (c->o.Nnode > VIC_MID_NODES) hipLaunchKernelGGL(vic_put_sum_deep, dim3(nblk, PUT_NPART), dim3(64), 0, st, a);
  else hipLaunchKernelGGL(vic_put_sum, dim3(nblk, PUT_NPART), dim3(64), 0, st, a);
  hipLaunchKernelGGL(vic_put_finish, dim3(nblk), dim3(64), 0, st, a);
  if (s >= 0)
    hipLaunchKernelGGL(vic_put_aggregate, dim3(nblk, (c->dom.out_nrow + PUT_AGG_ROWS - 1) / PUT_AGG_ROWS), dim3(64), 0, st, a, c->dom.d_rowagg);
  return hipGetLastError();
}

// nsteps steps from step0; with records, an output record ends after every `ratio` of them (nsteps = nrecords * ratio)
struct StepPlan {
  vicgpu_ctx* c;
  KArgs ka;
  CArgs ca;
  int step0, nsteps;
  bool records = false;
  int ratio = 0;
};

// The join of record k with cell groups, queued on the download stream by the last lane to arrive (RecordsJoin): behind every
// lane's packed event, reduce the slot over the groups, copy the [nrow][ngroup] table to the caller's and record reduced[k]
static hipError_t records_join(vicgpu_ctx* c, int k) {
  Records& R = c->rec;
  const hipStream_t dl = records_stream(c);
  const int s = k % R.depth;
  hipError_t e = hipSuccess;
  for (int lane = 0; lane < R.nlane; lane++)
    if ((e = hipStreamWaitEvent(dl, R.packed[(size_t)lane * R.depth + s], 0)) != hipSuccess) return e;
  RGArgs a;
  a.ncell = c->dom.ncell; a.nrow = R.nrow; a.ngroup = R.ngroup;
  a.off = R.d_group_off; a.cell = R.d_group_cell; a.weight = R.d_group_weight;
  a.slot_out = R.slot[s].d_out; a.group_out = R.slot[s].d_group; a.fill = R.fill;
  const bool timed = c->tune.stats && k == R.last_nrecords - 1;      // tuning: the reduction's own time (records_report_reduce)
  if (timed && (e = hipEventRecord(R.reduce_t0, dl)) != hipSuccess) return e;
  const unsigned ntile = (unsigned)((R.nrow + RG_ROWS - 1) / RG_ROWS);
  if (R.lane_per_group) hipLaunchKernelGGL(vic_out_group_reduce_lane, dim3((unsigned)((R.ngroup + 63) / 64), ntile), dim3(64), 0, dl, a);
  else hipLaunchKernelGGL(vic_out_group_reduce, dim3((unsigned)R.ngroup, ntile), dim3(64), 0, dl, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (timed && (e = hipEventRecord(R.reduce_t1, dl)) != hipSuccess) return e;
  R.reduce_timed = R.reduce_timed || timed;
  const size_t n = (size_t)R.nrow * R.ngroup;
  if ((e = hipMemcpyAsync(R.out + (size_t)k * n, R.slot[s].d_group, sizeof(float) * n, hipMemcpyDeviceToHost, dl)) != hipSuccess) return e;
  return hipEventRecord(R.reduced[k], dl);
}

// The end of record k for the cells [c0, c0 + ccount) of one lane, whose steps ran on `st`: once the slot's previous record
// has been downloaded (with groups: reduced), pack the aggregates into slot k % depth and zero them; the download stream
// copies the lane's columns into the caller's tables behind that (with groups: its cell_err columns, and the lane that
// arrives last queues the join).  A status, with the text in *err.
static int records_emit(vicgpu_ctx* c, std::string* err, int lane, hipStream_t st, int c0, int ccount, int k) {
  Records& R = c->rec;
  const hipStream_t dl = records_stream(c);
  const int s = k % R.depth;
  const size_t nc = c->dom.ncell, ld = R.ld;
  const bool groups = R.ngroup > 0;
  const auto failed = [&](hipError_t e) { *err = std::string("output record: ") + hipGetErrorString(e); return VICGPU_ERR_HIP; };
  hipError_t e = hipSuccess;
  if (k >= R.depth && groups) {
    // the reduction of the slot's last record reads every lane's columns: this lane can only wait for it once it is queued
    const int r = R.join->wait_queued(k - R.depth, err);
    if (r != VICGPU_OK) return r;
    e = hipStreamWaitEvent(st, R.reduced[k - R.depth], 0);
  } else if (k >= R.depth) e = hipStreamWaitEvent(st, R.landed[(size_t)lane * R.last_nrecords + (k - R.depth)], 0);
  else if (R.follows) e = hipStreamWaitEvent(st, R.drained, 0);      // the slot's last user is a copy of the call before
  if (e != hipSuccess) return failed(e);
  RPArgs a;
  a.ncell = c->dom.ncell; a.nrow = c->dom.out_nrow; a.c0 = c0; a.ccount = ccount;
  a.out_agg = c->dom.d_out_agg; a.sel_pos = R.d_sel_pos; a.cell_err = c->dom.d_cell_err;
  a.slot_out = R.slot[s].d_out; a.slot_err = R.slot[s].d_err;
  hipLaunchKernelGGL(vic_out_pack_reset, dim3((unsigned)((ccount + 63) / 64), (c->dom.out_nrow + PUT_AGG_ROWS - 1) / PUT_AGG_ROWS), dim3(64), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess) return failed(e);
  const hipEvent_t packed = R.packed[(size_t)lane * R.depth + s];
  if ((e = hipEventRecord(packed, st)) != hipSuccess) return failed(e);
  if ((e = hipStreamWaitEvent(dl, packed, 0)) != hipSuccess) return failed(e);
  if (!groups) {
    float* dst = R.out + (size_t)k * R.nrow * ld + c0;
    const float* src = R.slot[s].d_out + c0;
    if ((size_t)ccount == nc && ld == nc) e = hipMemcpyAsync(dst, src, sizeof(float) * nc * R.nrow, hipMemcpyDeviceToHost, dl);
    else e = hipMemcpy2DAsync(dst, sizeof(float) * ld, src, sizeof(float) * nc, sizeof(float) * ccount, R.nrow, hipMemcpyDeviceToHost, dl);
    if (e != hipSuccess) return failed(e);
  }
  if (R.err) e = hipMemcpyAsync(R.err + (size_t)k * ld + c0, R.slot[s].d_err + c0, sizeof(int) * ccount, hipMemcpyDeviceToHost, dl);
  if (e != hipSuccess) return failed(e);
  if (!groups) e = hipEventRecord(R.landed[(size_t)lane * R.last_nrecords + k], dl);
  else if (R.join->arrive(k, R.nlane)) {        // every lane has recorded its packed event of record k
    if ((e = records_join(c, k)) == hipSuccess) R.join->join_queued(k);
  }
  return e == hipSuccess ? VICGPU_OK : failed(e);
}

static void set_step_inputs(const vicgpu_ctx* c, KArgs& ka, int s) {
  const size_t nsub = c->o.NR + 1;
  ka.forcing = c->d_forcing + (size_t)s * VIC_NFORCE * nsub * c->dom.ncol;      // values per column, flags per cell
  ka.snowflag = c->d_snowflag + (size_t)s * nsub * c->dom.ncell;
  const int* d = &c->dmy[(size_t)s * VIC_NDMY];
  ka.dmy.month = d[VIC_DMY_MONTH]; ka.dmy.day_in_year = d[VIC_DMY_DAY_IN_YEAR]; ka.dmy.hour = d[VIC_DMY_HOUR];
  ka.dmy.day = d[VIC_DMY_DAY]; ka.dmy.year = d[VIC_DMY_YEAR];
}

// all steps of one vicgpu_step or vicgpu_run_records call for one chunk
static int fd_chunk_steps(const StepPlan& plan, FdChunk* ch) {
  vicgpu_ctx* c = plan.c;
  HIPCHK(ch, hipSetDevice(c->device));
  KArgs ka = plan.ka;
  CArgs ca = plan.ca;
  ka.glist = ch->d_glist; ka.gcount = ch->gcount; ka.map = ch->map;
  ca.c0 = ch->c0; ca.ccount = ch->ccount;
  const int lane = (int)(ch - &c->dom.chunks[0]);
  for (int s = plan.step0; s < plan.step0 + plan.nsteps; s++) {
    // the event pair of vicgpu_last_kernel_ms covers the last record, as after the loop of vicgpu_step calls: from where
    // the first chunk starts it
    if (plan.records && lane == 0 && s == plan.step0 + plan.nsteps - plan.ratio && s > plan.step0) HIPCHK(ch, hipEventRecord(c->ev[0], ch->stream));
    set_step_inputs(c, ka, s);
    const long long r0 = ch->rounds;
    const auto t0 = std::chrono::steady_clock::now();
    const int r = fd_step(c, ch, ka);
    if (r != VICGPU_OK) return r;
    if (c->tune.trace) {      // tuning: per-step wall time and Brent rounds
      HIPCHK(ch, hipStreamSynchronize(ch->stream));
      fprintf(stderr, "[vicgpu] step %d hour %d: %.2f ms, %lld rounds\n", s, ka.dmy.hour,
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), ch->rounds - r0);
    }
    hipLaunchKernelGGL(vic_cell_reduce, dim3((ch->ccount + 255) / 256), dim3(256), 0, ch->stream, ca);
    HIPCHK(ch, hipGetLastError());
    if (c->dom.put_on) HIPCHK(ch, launch_put_data(c, ch->stream, ch->c0, ch->ccount, s));
    if (plan.records && (s - plan.step0 + 1) % plan.ratio == 0) {
      const int re = records_emit(c, &ch->err, lane, ch->stream, ch->c0, ch->ccount, (s - plan.step0) / plan.ratio);
      if (re != VICGPU_OK) return re;
    }
  }
  HIPCHK(ch, hipEventRecord(ch->done, ch->stream));
  return VICGPU_OK;
}

// ... and, with grouped records, a chunk that fails releases the chunks that wait for its part of a record (RecordsJoin)
static int fd_chunk_run(const StepPlan& plan, FdChunk* ch) {
  const int r = fd_chunk_steps(plan, ch);
  Records& R = plan.c->rec;
  if (r != VICGPU_OK && plan.records && R.ngroup > 0) R.join->fail(r, ch->err);
  return r;
}

// ------------------------------------------------------------------------------------------------ vicgpu_set_domain, step by step
// The three steps after the argument check, on a context whose Domain is fresh and has its sizes.  Each table's shape is
// named once, where it is allocated; what starts as zero is filled on the context's stream without a wait of its own
// (vicgpu_set_domain waits once, before it returns or drops a half-built domain).

// the tables of the domain and of the model state
static int domain_tables(vicgpu_ctx* c, const double* cell_params, const int* hpi, const double* hpd, const int* cell_hru_offset,
                         const int* cell_hru_list) {
  Domain& d = c->dom;
  hipStream_t st = c->stream;
  const size_t ncell = d.ncell, nhru = d.nhru;
  const int Nn = c->opt.Nnode, Nb = c->opt.Nband;
  for (size_t g = 0; g < nhru; g++) if (hpi[HPI_IS_GLACIER * nhru + g]) d.any_glacier = true;
  HIPCHK(c, d.d_cp.alloc(VIC_CPX_NROW(Nn, Nb) * ncell));                       // the caller's rows + the derived rows
  HIPCHK(c, d.d_cp.upload(st, cell_params, 0, VICGPU_CP_NROW(Nn, Nb) * ncell));
  hipLaunchKernelGGL(vic_derive_cell_params, dim3((c->dom.ncell + 255) / 256), dim3(256), 0, st, c->dom.d_cp, c->dom.ncell, Nn, Nb);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, d.d_hpi.alloc(HPI_NROW * nhru));
  HIPCHK(c, d.d_hpi.upload(st, hpi));
  HIPCHK(c, d.d_hpd.alloc(HPD_NROW * nhru));
  HIPCHK(c, d.d_hpd.upload(st, hpd));
  HIPCHK(c, d.d_cell_off.alloc(ncell + 1));
  HIPCHK(c, d.d_cell_off.upload(st, cell_hru_offset));
  HIPCHK(c, d.d_cell_list.alloc(nhru));
  HIPCHK(c, d.d_cell_list.upload(st, cell_hru_list));
  d.cell_off.assign(cell_hru_offset, cell_hru_offset + ncell + 1);
  d.cell_list.assign(cell_hru_list, cell_hru_list + nhru);
  d.copy_key.resize(COPY_NKEY * nhru);
  d.cell_class.clear();
  d.mix_plan = MixPlan();
  for (int k = 0; k < COPY_NKEY; k++) std::copy(hpi + COPY_KEY_ROWS[k] * nhru, hpi + (COPY_KEY_ROWS[k] + 1) * nhru, d.copy_key.begin() + k * nhru);
  HIPCHK(c, d.d_sd.alloc_fill(VICGPU_SD_NROW(Nn) * nhru, 0, st));
  HIPCHK(c, d.d_si.alloc_fill(VICGPU_SI_NROW(Nn) * nhru, 0, st));
  HIPCHK(c, d.d_flux.alloc_fill(FX_NROW * nhru, 0, st));
  HIPCHK(c, d.d_cell_out.alloc_fill(CO_NROW * ncell, 0, st));
  HIPCHK(c, d.d_accum.alloc_fill(CA_NROW * ncell, 0, st));
  HIPCHK(c, d.d_hru_err.alloc_fill(nhru, 0, st));
  HIPCHK(c, d.d_cell_err.alloc_fill(ncell, 0, st));
  const std::vector<int> all_valid(ncell, CELL_VALID);
  HIPCHK(c, d.d_valid.alloc(ncell));
  HIPCHK(c, d.d_valid.upload(st, all_valid.data()));
  return VICGPU_OK;
}

// the workspace of the finite-difference pipeline (QUICK_FLUX off)
static int domain_fd_workspace(vicgpu_ctx* c) {
  Domain& d = c->dom;
  hipStream_t st = c->stream;
  const size_t nhru = d.nhru;
  const int Nn = c->o.Nnode;
  const size_t words = NODE_DISPATCH(Nn, ctx_words);
  HIPCHK(c, d.d_ctx.alloc(ctx_padded_words(words) * ((nhru + 63) / 64 * 64)));
  HIPCHK(c, d.d_ts.alloc(nhru));
  // item blocks and solution records: sector-multiple strides on hipMalloc's (256-byte aligned) bases, vic_layout.hpp
  HIPCHK(c, d.d_pin.alloc_fill((size_t)item_stride(Nn) * nhru, 0, st));
  HIPCHK(c, d.d_pout.alloc_fill((size_t)pout_hru_stride(Nn) * nhru, 0, st));
  HIPCHK(c, d.d_pslot.alloc_fill(nhru, 0, st));
  HIPCHK(c, d.d_hkey.alloc_fill(nhru, 0, st));
  HIPCHK(c, d.d_hstate.alloc_fill(nhru, 0, st));
  if (c->o.QUICK_SOLVE) HIPCHK(c, d.d_jl.alloc_fill(nhru, 0, st));
  if (c->o.IMPLICIT) {
    HIPCHK(c, d.d_pimp.alloc_fill((size_t)Nn * PIMP * nhru, 0, st));
    HIPCHK(c, d.d_lastexp.alloc_fill(nhru, 0xFF, st));
  }
  return VICGPU_OK;
}

// the cell chunks (Tuning::nchunk): independent pipelines on their own streams and host threads
static int domain_chunks(vicgpu_ctx* c, const int* hpi, const int* cell_hru_offset, const int* cell_hru_list) {
  Domain& d = c->dom;
  const int ncell = d.ncell, nhru = d.nhru, nchunk = c->tune.nchunk;
  const int waves = NODE_DISPATCH(c->o.Nnode, profile_resident_waves, c->device, c->tune.node_newton);
  c->profile_waves = std::max(waves * c->tune.profile_waves_pct / 100, 1);
  d.chunks.resize(nchunk);
  for (int k = 0; k < nchunk; k++) {
    FdChunk& ch = d.chunks[k];
    ch.c0 = (int)((long long)ncell * k / nchunk);
    ch.ccount = (int)((long long)ncell * (k + 1) / nchunk) - ch.c0;
    std::vector<int> gl(cell_hru_list + cell_hru_offset[ch.c0], cell_hru_list + cell_hru_offset[ch.c0 + ch.ccount]);
    std::sort(gl.begin(), gl.end());
    ch.gcount = (int)gl.size();
    ch.map = LaunchMap();
    if (ch.ccount > 0 && ch.gcount % ch.ccount == 0 && c->tune.xcd_map) {
      const int nslot = ch.gcount / ch.ccount;
      bool regular = true;
      for (int sl = 0; sl < nslot && regular; sl++)
        for (int i = 0; i < ch.ccount; i++)
          if (gl[(size_t)sl * ch.ccount + i] != sl * ncell + ch.c0 + i || hpi[(size_t)HPI_CELL * nhru + gl[(size_t)sl * ch.ccount + i]] != ch.c0 + i) {
            regular = false;
            break;
          }
      if (regular) { ch.map.nslot = nslot; ch.map.ccount = ch.ccount; }
    }
    const size_t gn = ch.gcount > 0 ? ch.gcount : 1;
    ch.list_cap = (int)gn;
    HIPCHK(c, ch.d_glist.alloc(gn));
    if (ch.gcount) HIPCHK(c, ch.d_glist.upload(c->stream, gl.data()));
    HIPCHK(c, ch.d_list[0].alloc(gn * NBUCKET));
    HIPCHK(c, ch.d_list[1].alloc(gn * NBUCKET));
    HIPCHK(c, ch.d_count.alloc(CNT_TOTAL));
    // a wave appends at most 64 entries to stripe blockIdx.x % PEND_STRIPES, and no evaluation grid is larger than the dense one
    ch.pend_cap = 64 * ((ch.map.nblocks(ch.gcount) + PEND_STRIPES - 1) / PEND_STRIPES);
    if (ch.pend_cap < 64) ch.pend_cap = 64;
    HIPCHK(c, ch.d_plist[0].alloc((size_t)ch.pend_cap * PEND_STRIPES));
    HIPCHK(c, ch.d_plist[1].alloc((size_t)ch.pend_cap * PEND_STRIPES));
    if (c->o.IMPLICIT) {
      HIPCHK(c, ch.d_fb_list.alloc(gn * NBUCKET));
      HIPCHK(c, ch.d_fb_count.alloc(NBUCKET + 1));
    }
    HIPCHK(c, ch.h_count.alloc((size_t)CNT_TOTAL * RB_DEPTH));
    HIPCHK(c, ch.stream.create());
    HIPCHK(c, ch.done.create(hipEventDisableTiming));
    for (Event& e : ch.readback) HIPCHK(c, e.create(hipEventDisableTiming));
  }
  return VICGPU_OK;
}

// ------------------------------------------------------------------------------------------------ vicgpu_copy_cells
// The tables a copy moves, in a fixed order: f(table, rows, columns per row, per_cell) for table t when `what` asks for it.
// per_cell: the columns are cells (the cell pairs of the plan), else HRUs.  f is generic over the element type.
constexpr int COPY_NTABLE = 4;
template <typename F>
static hipError_t copy_table(vicgpu_ctx* c, int t, int what, F&& f) {
  Domain& d = c->dom;
  const int Nn = c->opt.Nnode;
  const bool state = (what & VICGPU_COPY_STATE) != 0, balance = (what & VICGPU_COPY_BALANCE) != 0;
  switch (t) {
    case 0: return state ? f(d.d_sd.get(), (int)VICGPU_SD_NROW(Nn), (size_t)d.nhru, false) : hipSuccess;
    case 1: return state ? f(d.d_si.get(), (int)VICGPU_SI_NROW(Nn), (size_t)d.nhru, false) : hipSuccess;
    case 2: return state ? f(d.d_flux.get(), (int)FX_NROW, (size_t)d.nhru, false) : hipSuccess;
    default: return balance ? f(d.d_pb.get(), (int)PBX_NROW, (size_t)d.ncell, true) : hipSuccess;      // the public rows + put_data's own
  }
}

static std::string copy_fault_text(const CopyPlan& p) {
  const char* rule = p.fault == COPY_CELL_RANGE ? "a cell is outside the domain"
                     : p.fault == COPY_DST_REPEATS ? "the destination repeats"
                                                   : copy_pair_fault_text(p.fault);
  return "copy_cells: pair " + std::to_string(p.index) + ": " + rule;
}

// ------------------------------------------------------------------------------------------------ read-backs
// `count` elements from the start of a device table to the host (all of it when count is left out), after everything
// queued on the context's stream
template <typename T>
static int d2h(vicgpu_ctx* c, T* dst, const DevBuf<T>& src, size_t count) {
  if (!c || !dst || !src) return VICGPU_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, src.download(c->stream, dst, 0, count));
  return VICGPU_OK;
}
template <typename T>
static int d2h(vicgpu_ctx* c, T* dst, const DevBuf<T>& src) { return d2h(c, dst, src, src.size()); }

// the same for the first nrow rows of a per-cell table into the columns [0, ncell) of a host table whose rows are ld cells wide
template <typename T>
static int d2h_cols(vicgpu_ctx* c, T* dst, int ld, const DevBuf<T>& src, int nrow) {
  if (!c || !dst || !src || ld < c->dom.ncell) return VICGPU_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, src.download_cols(c->stream, dst, ld, nrow, c->dom.ncell));
  return VICGPU_OK;
}
