// vic_group.hpp — the device group of include/vicgpu_group.h: N shard contexts of one domain, stepped at the same time.
//
// Host code only: it builds on the single-context entries of include/vicgpu.h, on their pitched variants declared below and
// on d2h_cols (vic_pipeline.hpp), which copy one shard's columns straight between the device and the caller's global
// [..][ncell] table, and on the checks of vic_checks.hpp, which it makes on the whole domain.  No kernel lives here.
#pragma once
#include <condition_variable>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>
#include "vicgpu_group.h"
#include "vic_checks.hpp"
#include "vic_pipeline.hpp"

// static helpers of vicgpu_api.hip with a pitch (ld: cells per row of the caller's table)
static int prefetch_impl(vicgpu_ctx* c, int nsteps, const double* forcing, const unsigned char* snowflag, const double* raw,
                         const int* dmy, double min_wind, int plapse, int ld, int ld_flag, const PertLists* P = nullptr);
static int get_outputs_impl(vicgpu_ctx* c, int nvar, const int* var_ids, float* out, int reset, int ld);
static int glacier_fit_impl(vicgpu_ctx* c, double* eq, int reset, int ld);
static int run_records_impl(vicgpu_ctx* c, int step0, int nrecords, float* out, int* cell_err, int ld);
static int get_cell_params_impl(vicgpu_ctx* c, double* cell_params, int ld);

// One persistent host thread per shard.  run(fn) calls fn(k) on thread k for every shard and returns when all have returned.
// Each thread selects its shard's device once at start (every library entry selects it again anyway).
class ShardThreads {
 public:
  void start(const std::vector<int>& devices) {
    for (size_t k = 0; k < devices.size(); k++) th_.emplace_back([this, k, d = devices[k]]() { loop((int)k, d); });
  }
  void run(const std::function<void(int)>& fn) {
    std::unique_lock<std::mutex> lk(m_);
    job_ = &fn;
    pending_ = (int)th_.size();
    gen_++;
    go_.notify_all();
    done_.wait(lk, [this]() { return pending_ == 0; });
    job_ = nullptr;
  }
  void stop() {
    {
      std::lock_guard<std::mutex> lk(m_);
      quit_ = true;
    }
    go_.notify_all();
    for (std::thread& t : th_) t.join();
    th_.clear();
  }

 private:
  void loop(int k, int device) {
    HIPIGN(hipSetDevice(device));
    unsigned long long seen = 0;
    for (;;) {
      const std::function<void(int)>* fn;
      {
        std::unique_lock<std::mutex> lk(m_);
        go_.wait(lk, [&]() { return quit_ || gen_ != seen; });
        if (quit_) return;
        seen = gen_;
        fn = job_;
      }
      (*fn)(k);
      std::lock_guard<std::mutex> lk(m_);
      if (--pending_ == 0) done_.notify_one();
    }
  }
  std::vector<std::thread> th_;
  std::mutex m_;
  std::condition_variable go_, done_;
  const std::function<void(int)>* job_ = nullptr;
  unsigned long long gen_ = 0;
  int pending_ = 0;
  bool quit_ = false;
};

struct vicgpu_group {
  vicgpu_options opt;
  std::vector<int> device;
  std::vector<vicgpu_ctx*> ctx;
  ShardThreads threads;
  std::string err;
  bool domain_ready = false;
  int ncell = 0, nhru = 0;
  std::vector<int> bounds;                  // [nshard+1]: shard k holds the cells [bounds[k], bounds[k+1])
  std::vector<std::vector<int>> hru;        // shard k's HRUs: global id of its HRU j
  std::vector<int> rec_first;               // [nshard]: index of shard k's first state record = cell_hru_offset[bounds[k]]
  std::vector<int> rec_band, rec_veg;       // band and vegetation class of every state record (cell-major hruList order)
  // forcing map (vicgpu_group_set_forcing_map), in the caller's global cell order: shard k holds the columns from col_lo[k]
  // on that its cells span, its own map rebased by col_lo[k].  Identity: ncol == ncell, cell_col empty, col_lo[k] == bounds[k]
  int ncol = 0;
  std::vector<int> cell_col, col_lo;
  // for vicgpu_group_copy_cells, which plans on the whole domain: the caller's CSR lists, the HRU rows a pair of cells must
  // agree in ([COPY_NKEY][nhru])
  std::vector<int> cell_off, cell_list, copy_key;
  // every cell's and every HRU's shard and id within it: how a caller's list of columns is split (group_columns)
  std::vector<int> cell_shard, cell_local, hru_shard, hru_local;
  int nshard() const { return (int)ctx.size(); }
  int c0(int k) const { return bounds[k]; }
  void identity_map() { ncol = ncell; cell_col.clear(); col_lo.assign(bounds.begin(), bounds.end() - 1); }
};

// fn(k) -> status on every shard at the same time; the first failing shard's code and message
static int group_each(vicgpu_group* g, const std::function<int(int)>& fn) {
  std::vector<int> rc(g->nshard(), VICGPU_OK);
  g->threads.run([&](int k) { rc[k] = fn(k); });
  for (int k = 0; k < g->nshard(); k++)
    if (rc[k] != VICGPU_OK) {
      g->err = "shard " + std::to_string(k) + " (device " + std::to_string(g->device[k]) + "): " + vicgpu_last_error(g->ctx[k]);
      return rc[k];
    }
  return VICGPU_OK;
}

static int group_fail(vicgpu_group* g, int code, const std::string& msg) {
  g->err = msg;
  return code;
}

// The columns pos[0 .. nk) of the caller's values[nrow][n] <-> a shard's packed table [nrow][nk]
template <typename T>
static void take_columns(const T* values, int nrow, size_t n, const std::vector<int>& pos, std::vector<T>& packed) {
  const size_t nk = pos.size();
  packed.resize((size_t)nrow * nk);
  for (int r = 0; r < nrow; r++) {
    const T* src = values + (size_t)r * n;
    T* dst = packed.data() + (size_t)r * nk;
    for (size_t j = 0; j < nk; j++) dst[j] = src[pos[j]];
  }
}
template <typename T>
static void put_columns(T* values, int nrow, size_t n, const std::vector<int>& pos, const std::vector<T>& packed) {
  const size_t nk = pos.size();
  for (int r = 0; r < nrow; r++) {
    const T* src = packed.data() + (size_t)r * nk;
    T* dst = values + (size_t)r * n;
    for (size_t j = 0; j < nk; j++) dst[pos[j]] = src[j];
  }
}

// The per-HRU table [nrow][nhru] of the caller <-> shard k's [nrow][nhru_k] (its HRUs in its own numbering)
template <typename T>
static void split_hru_table(const vicgpu_group* g, int k, const T* global, int nrow, std::vector<T>& local) {
  take_columns(global, nrow, (size_t)g->nhru, g->hru[k], local);
}
template <typename T>
static void merge_hru_table(const vicgpu_group* g, int k, const std::vector<T>& local, int nrow, T* global) {
  put_columns(global, nrow, (size_t)g->nhru, g->hru[k], local);
}

// A caller's list of n columns, cells (per_cell) or HRUs in the global numbering, by shard: the entries of the list that are
// shard k's own (pos[k]) and their ids within it (local[k]).  cols == nullptr, the dense form: every column of the shard in
// pos[k] and no local list -- a shard's cells are a block of the caller's, its HRUs are numbered in the caller's order, so
// the call stays dense in every shard.  The list has been checked (check_param_update).
struct GroupColumns {
  std::vector<std::vector<int>> pos, local;
  const int* idx(int k) const { return local[k].empty() ? nullptr : local[k].data(); }
};

static GroupColumns group_columns(const vicgpu_group* g, bool per_cell, int n, const int* cols) {
  GroupColumns L;
  const int ns = g->nshard();
  L.pos.resize(ns); L.local.resize(ns);
  const std::vector<int>& shard = per_cell ? g->cell_shard : g->hru_shard;
  const std::vector<int>& local = per_cell ? g->cell_local : g->hru_local;
  if (cols) {
    for (int i = 0; i < n; i++) {
      L.pos[shard[cols[i]]].push_back(i);
      L.local[shard[cols[i]]].push_back(local[cols[i]]);
    }
  } else if (per_cell) {
    for (int k = 0; k < ns; k++)
      for (int i = g->bounds[k]; i < g->bounds[k + 1]; i++) L.pos[k].push_back(i);
  } else {
    L.pos = g->hru;
  }
  return L;
}

static bool group_ready(vicgpu_group* g) {
  if (g->domain_ready) return true;
  g->err = "no domain: call vicgpu_group_set_domain first";
  return false;
}

extern "C" {

int vicgpu_group_partition(int ncell, const int* off, int nshard, int* bounds) {
  if (ncell < 1 || !off || !bounds || nshard < 1 || nshard > ncell || off[0] != 0) return VICGPU_ERR_ARG;
  for (int i = 0; i < ncell; i++)
    if (off[i + 1] < off[i]) return VICGPU_ERR_ARG;
  const long long nhru = off[ncell];
  bounds[0] = 0;
  for (int r = 1; r < nshard; r++) {
    const double target = (double)(nhru * r) / nshard;                 // vic_amd/shard.py partition_cells
    const int c = (int)(std::lower_bound(off, off + ncell + 1, target, [](int a, double t) { return (double)a < t; }) - off);
    bounds[r] = std::min(std::max(c, bounds[r - 1]), ncell);
  }
  bounds[nshard] = ncell;
  return VICGPU_OK;
}

void vicgpu_group_destroy(vicgpu_group* g) {
  if (!g) return;
  g->threads.stop();
  for (vicgpu_ctx* c : g->ctx) vicgpu_destroy(c);
  delete g;
}

int vicgpu_group_create(const vicgpu_options* opt, int nshard, const int* devices, vicgpu_group** out) {
  if (!opt || !out || nshard < 1) return VICGPU_ERR_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return VICGPU_ERR_HIP;   // no CPU fallback, like vicgpu_create
  std::vector<int> dev(nshard);
  for (int k = 0; k < nshard; k++) {
    dev[k] = devices ? devices[k] : k;
    if (dev[k] < 0 || dev[k] >= ndev) return VICGPU_ERR_ARG;
  }
  vicgpu_group* g = new vicgpu_group();
  g->opt = *opt;
  g->device = dev;
  for (int k = 0; k < nshard; k++) {
    vicgpu_ctx* c = nullptr;
    const int r = vicgpu_create(opt, dev[k], &c);
    if (r != VICGPU_OK) {
      vicgpu_group_destroy(g);                    // no thread started yet: destroys the contexts made so far
      return r;
    }
    g->ctx.push_back(c);
  }
  try {
    g->threads.start(dev);
  } catch (...) {                                 // std::system_error: no thread could be started
    vicgpu_group_destroy(g);                      // joins the threads that did start
    return VICGPU_ERR_NOMEM;
  }
  *out = g;
  return VICGPU_OK;
}

const char* vicgpu_group_last_error(const vicgpu_group* g) { return g ? g->err.c_str() : "null group"; }

int vicgpu_group_shard_bounds(vicgpu_group* g, int* bounds) {
  if (!g || !bounds) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  std::copy(g->bounds.begin(), g->bounds.end(), bounds);
  return VICGPU_OK;
}

vicgpu_ctx* vicgpu_group_shard_ctx(vicgpu_group* g, int k) { return (g && k >= 0 && k < g->nshard()) ? g->ctx[k] : nullptr; }

int vicgpu_group_set_veglib(vicgpu_group* g, int nrow, const double* veglib) {
  if (!g) return VICGPU_ERR_ARG;
  return group_each(g, [&](int k) { return vicgpu_set_veglib(g->ctx[k], nrow, veglib); });
}

int vicgpu_group_set_domain(vicgpu_group* g, int ncell, int nhru, const double* cp, const int* hpi, const double* hpd, const int* off,
                            const int* list) {
  if (!g) return VICGPU_ERR_ARG;
  g->domain_ready = false;
  if (ncell <= 0 || nhru <= 0 || !cp || !hpi || !hpd || !off || !list) return group_fail(g, VICGPU_ERR_ARG, "set_domain: bad arguments");
  // the list check on the whole domain: every index used below to slice it is valid after it (bands and vegetation indices
  // are left to the shards' vicgpu_set_domain)
  const DomainFault f = check_domain_lists(ncell, nhru, off, list, hpi);
  if (f.rule == DOMAIN_OFFSET_SPAN) return group_fail(g, VICGPU_ERR_ARG, "set_domain: cell_hru_offset does not span the HRUs");
  if (f.rule == DOMAIN_OFFSET_DECREASES) return group_fail(g, VICGPU_ERR_ARG, "set_domain: cell_hru_offset decreases");
  if (f.rule != DOMAIN_OK)
    return group_fail(g, VICGPU_ERR_ARG, "set_domain: cell_hru_list entry " + std::to_string(f.index) + " does not match the domain");
  const int ns = g->nshard();
  std::vector<int> b(ns + 1);
  if (vicgpu_group_partition(ncell, off, ns, b.data()) != VICGPU_OK)
    return group_fail(g, VICGPU_ERR_ARG, "set_domain: " + std::to_string(ns) + " shards for " + std::to_string(ncell) + " cells");
  for (int k = 0; k < ns; k++)
    if (b[k + 1] == b[k]) return group_fail(g, VICGPU_ERR_ARG, "set_domain: shard " + std::to_string(k) + " gets no cell");
  // shard k: its cells' HRUs in the domain's HRU order, renumbered from 0 (vic_amd/shard.py shard_domain)
  g->hru.assign(ns, std::vector<int>());
  std::vector<int> shard_of(ncell), cell_id(ncell), new_id(nhru);
  for (int k = 0; k < ns; k++)
    for (int i = b[k]; i < b[k + 1]; i++) { shard_of[i] = k; cell_id[i] = i - b[k]; }
  for (int h = 0; h < nhru; h++) {
    std::vector<int>& ids = g->hru[shard_of[hpi[(size_t)HPI_CELL * nhru + h]]];
    new_id[h] = (int)ids.size();
    ids.push_back(h);
  }
  g->ncell = ncell; g->nhru = nhru; g->bounds = b;
  const int cp_nrow = VICGPU_CP_NROW(g->opt.Nnode, g->opt.Nband);
  const int r = group_each(g, [&](int k) {
    const int c0 = b[k], nc = b[k + 1] - b[k];
    const std::vector<int>& ids = g->hru[k];
    const int nh = (int)ids.size();
    std::vector<double> cpk((size_t)cp_nrow * nc), hpdk;
    for (int row = 0; row < cp_nrow; row++)
      std::copy(cp + (size_t)row * ncell + c0, cp + (size_t)row * ncell + c0 + nc, cpk.begin() + (size_t)row * nc);
    std::vector<int> hpik;
    split_hru_table(g, k, hpi, HPI_NROW, hpik);
    for (int j = 0; j < nh; j++) hpik[(size_t)HPI_CELL * nh + j] -= c0;
    split_hru_table(g, k, hpd, HPD_NROW, hpdk);
    std::vector<int> offk(nc + 1), listk(off[c0 + nc] - off[c0]);
    for (int i = 0; i <= nc; i++) offk[i] = off[c0 + i] - off[c0];
    for (size_t j = 0; j < listk.size(); j++) listk[j] = new_id[list[off[c0] + j]];
    return vicgpu_set_domain(g->ctx[k], nc, nh, cpk.data(), hpik.data(), hpdk.data(), offk.data(), listk.data());
  });
  if (r != VICGPU_OK) return r;
  g->rec_band.resize(nhru); g->rec_veg.resize(nhru);
  for (int j = 0; j < nhru; j++) {
    g->rec_band[j] = hpi[(size_t)HPI_BAND * nhru + list[j]];
    g->rec_veg[j] = hpi[(size_t)HPI_VEG_CLASS * nhru + list[j]];
  }
  g->rec_first.resize(ns);
  for (int k = 0; k < ns; k++) g->rec_first[k] = off[b[k]];
  g->cell_off.assign(off, off + ncell + 1);
  g->cell_list.assign(list, list + nhru);
  g->copy_key.resize((size_t)COPY_NKEY * nhru);
  for (int r = 0; r < COPY_NKEY; r++)
    std::copy(hpi + (size_t)COPY_KEY_ROWS[r] * nhru, hpi + (size_t)(COPY_KEY_ROWS[r] + 1) * nhru, g->copy_key.begin() + (size_t)r * nhru);
  g->cell_shard = shard_of; g->cell_local = cell_id;
  g->hru_local = new_id;
  g->hru_shard.resize(nhru);
  for (int h = 0; h < nhru; h++) g->hru_shard[h] = shard_of[hpi[(size_t)HPI_CELL * nhru + h]];
  g->identity_map();               // as every shard's vicgpu_set_domain has left it
  g->domain_ready = true;
  return VICGPU_OK;
}

// Forcing map (vicgpu.h) in the caller's global cell order.  Shard k takes the column range [lo_k, hi_k] its cells span and
// the map rebased by lo_k; the forcing and raw uploads below then start at column lo_k of the caller's ncol-wide tables.
int vicgpu_group_set_forcing_map(vicgpu_group* g, int ncol, const int* cell_col) {
  if (!g) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  if (!cell_col) {
    if (ncol != 0 && ncol != g->ncell) return group_fail(g, VICGPU_ERR_ARG, "set_forcing_map: no map, but ncol is neither 0 nor ncell");
    const int r = group_each(g, [&](int k) { return vicgpu_set_forcing_map(g->ctx[k], 0, nullptr); });
    if (r == VICGPU_OK) g->identity_map();
    return r;
  }
  if (ncol < 1) return group_fail(g, VICGPU_ERR_ARG, "set_forcing_map: ncol < 1");
  for (int i = 0; i < g->ncell; i++)
    if (cell_col[i] < 0 || cell_col[i] >= ncol) return group_fail(g, VICGPU_ERR_ARG, "set_forcing_map: entry " + std::to_string(i) + " is not a column");
  const int ns = g->nshard();
  std::vector<int> lo(ns), width(ns);
  for (int k = 0; k < ns; k++) {
    const int* first = cell_col + g->bounds[k];
    const int* last = cell_col + g->bounds[k + 1];
    lo[k] = *std::min_element(first, last);
    width[k] = *std::max_element(first, last) - lo[k] + 1;
  }
  const int r = group_each(g, [&](int k) {
    std::vector<int> local(cell_col + g->bounds[k], cell_col + g->bounds[k + 1]);
    for (int& v : local) v -= lo[k];
    return vicgpu_set_forcing_map(g->ctx[k], width[k], local.data());
  });
  if (r != VICGPU_OK) {            // a shard's allocation was refused: no shard keeps a map the others do not have
    std::string msg = g->err;
    group_each(g, [&](int k) { return vicgpu_set_forcing_map(g->ctx[k], 0, nullptr); });
    g->identity_map();
    g->err = msg + " (the group is back on the identity map)";
    return r;
  }
  g->ncol = ncol; g->cell_col.assign(cell_col, cell_col + g->ncell); g->col_lo = lo;
  return VICGPU_OK;
}

int vicgpu_group_get_forcing_map(vicgpu_group* g, int* ncol, int* cell_col) {
  if (!g || !ncol) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  *ncol = g->ncol;
  if (cell_col)
    for (int i = 0; i < g->ncell; i++) cell_col[i] = g->cell_col.empty() ? i : g->cell_col[i];
  return VICGPU_OK;
}

int vicgpu_group_set_state(vicgpu_group* g, const double* sd, const int* si) {
  if (!g || !sd || !si) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  return group_each(g, [&](int k) {
    std::vector<double> d;
    std::vector<int> i;
    split_hru_table(g, k, sd, VICGPU_SD_NROW(g->opt.Nnode), d);
    split_hru_table(g, k, si, VICGPU_SI_NROW(g->opt.Nnode), i);
    return vicgpu_set_state(g->ctx[k], d.data(), i.data());
  });
}

int vicgpu_group_get_state(vicgpu_group* g, double* sd, int* si) {
  if (!g || !sd || !si) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  return group_each(g, [&](int k) {
    const size_t n = g->hru[k].size();
    std::vector<double> d((size_t)VICGPU_SD_NROW(g->opt.Nnode) * n);
    std::vector<int> i((size_t)VICGPU_SI_NROW(g->opt.Nnode) * n);
    const int r = vicgpu_get_state(g->ctx[k], d.data(), i.data());
    if (r == VICGPU_OK) {
      merge_hru_table(g, k, d, VICGPU_SD_NROW(g->opt.Nnode), sd);
      merge_hru_table(g, k, i, VICGPU_SI_NROW(g->opt.Nnode), si);
    }
    return r;
  });
}

int vicgpu_group_set_fluxes(vicgpu_group* g, const double* flux) {
  if (!g || !flux) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  return group_each(g, [&](int k) {
    std::vector<double> f;
    split_hru_table(g, k, flux, FX_NROW, f);
    return vicgpu_set_fluxes(g->ctx[k], f.data());
  });
}

int vicgpu_group_get_fluxes(vicgpu_group* g, double* flux) {
  if (!g || !flux) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  return group_each(g, [&](int k) {
    std::vector<double> f((size_t)FX_NROW * g->hru[k].size());
    const int r = vicgpu_get_fluxes(g->ctx[k], f.data());
    if (r == VICGPU_OK) merge_hru_table(g, k, f, FX_NROW, flux);
    return r;
  });
}

int vicgpu_group_prefetch_forcing(vicgpu_group* g, int nsteps, const double* forcing, const unsigned char* snowflag, const int* dmy) {
  if (!g || !forcing || !snowflag || !dmy) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  return group_each(g, [&](int k) {
    return prefetch_impl(g->ctx[k], nsteps, forcing + g->col_lo[k], snowflag + g->c0(k), nullptr, dmy, 0.0, 1, g->ncol, g->ncell);
  });
}

int vicgpu_group_prefetch_forcing_raw(vicgpu_group* g, int nsteps, const double* raw, const int* dmy, double min_wind_speed, int plapse) {
  if (!g || !raw || !dmy) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  return group_each(g, [&](int k) {
    return prefetch_impl(g->ctx[k], nsteps, nullptr, nullptr, raw + g->col_lo[k], dmy, min_wind_speed, plapse, g->ncol, g->ncell);
  });
}

// vicgpu_prefetch_forcing_perturbed (vicgpu.h) with the lists in the caller's global column order, checked on the whole domain
// before any shard uploads.  Shard k derives the forcing columns it holds (col_lo[k] on) and uploads the range of source
// columns those columns name -- the same pitched copy, leading dimension nsrc -- with its col_src rebased by that range's
// start; its slice of col_group and the whole of pert go unrebased (a group per column: group = global column).
int vicgpu_group_prefetch_forcing_perturbed(vicgpu_group* g, int nsteps, int nsrc, const double* raw, const int* col_src, int ngroup,
                                            const int* col_group, const double* pert, const int* dmy, double min_wind_speed, int plapse) {
  if (!g || !raw || !dmy || nsteps <= 0 || nsrc < 1) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  const std::string why = check_forcing_perturbed(g->ncol, nsteps, nsrc, col_src, ngroup, col_group, pert, dmy);
  if (!why.empty()) return group_fail(g, VICGPU_ERR_ARG, why);
  if (!col_src && ngroup == 0) return vicgpu_group_prefetch_forcing_raw(g, nsteps, raw, dmy, min_wind_speed, plapse);
  return group_each(g, [&](int k) {
    const int lo = g->col_lo[k], width = g->ctx[k]->dom.ncol;
    int src_lo = lo, src_n = width;              // no col_src: the shard's own columns
    if (col_src) {
      src_lo = *std::min_element(col_src + lo, col_src + lo + width);
      src_n = *std::max_element(col_src + lo, col_src + lo + width) - src_lo + 1;
    }
    const PertLists P{src_n, col_src ? col_src + lo : nullptr, src_lo, ngroup, col_group ? col_group + lo : nullptr, lo, pert};
    return prefetch_impl(g->ctx[k], nsteps, nullptr, nullptr, raw + src_lo, dmy, min_wind_speed, plapse, nsrc, g->ncell, &P);
  });
}

int vicgpu_group_swap_forcing(vicgpu_group* g) {
  if (!g) return VICGPU_ERR_ARG;
  return group_each(g, [&](int k) { return vicgpu_swap_forcing(g->ctx[k]); });
}

int vicgpu_group_push_forcing(vicgpu_group* g, int nsteps, const double* forcing, const unsigned char* snowflag, const int* dmy) {
  const int r = vicgpu_group_prefetch_forcing(g, nsteps, forcing, snowflag, dmy);
  return r == VICGPU_OK ? vicgpu_group_swap_forcing(g) : r;
}

int vicgpu_group_step(vicgpu_group* g, int step0, int nsteps) {
  if (!g) return VICGPU_ERR_ARG;
  return group_each(g, [&](int k) { return vicgpu_step(g->ctx[k], step0, nsteps); });
}

int vicgpu_group_synchronize(vicgpu_group* g) {
  if (!g) return VICGPU_ERR_ARG;
  return group_each(g, [&](int k) { return vicgpu_synchronize(g->ctx[k]); });
}

int vicgpu_group_put_data_config(vicgpu_group* g, int out_step_ratio) {
  if (!g) return VICGPU_ERR_ARG;
  return group_each(g, [&](int k) { return vicgpu_put_data_config(g->ctx[k], out_step_ratio); });
}

int vicgpu_group_put_data_init(vicgpu_group* g) {
  if (!g) return VICGPU_ERR_ARG;
  return group_each(g, [&](int k) { return vicgpu_put_data_init(g->ctx[k]); });
}

int vicgpu_group_get_outputs(vicgpu_group* g, int nvar, const int* var_ids, float* out, int reset) {
  if (!g || nvar < 0 || (nvar > 0 && (!var_ids || !out))) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  for (int v = 0; v < nvar; v++)
    if (var_ids[v] < 0 || var_ids[v] >= VOUT_NVAR) return group_fail(g, VICGPU_ERR_ARG, "get_outputs: unknown variable id");
  return group_each(g, [&](int k) { return get_outputs_impl(g->ctx[k], nvar, var_ids, nvar > 0 ? out + g->c0(k) : out, reset, g->ncell); });
}

int vicgpu_group_get_balance(vicgpu_group* g, double* pb) {
  if (!g || !pb) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  return group_each(g, [&](int k) {
    vicgpu_ctx* c = g->ctx[k];
    if (!c->dom.put_on) return (int)VICGPU_ERR_STATE;
    return d2h_cols(c, pb + g->c0(k), g->ncell, c->dom.d_pb, PB_NROW);
  });
}

int vicgpu_group_get_cell_errors(vicgpu_group* g, int* flags) {
  if (!g || !flags) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  return group_each(g, [&](int k) { return d2h_cols(g->ctx[k], flags + g->c0(k), g->ncell, g->ctx[k]->dom.d_cell_err, 1); });
}

// Cell validity (vicgpu.h): the mask is every shard's; shard k's part of the validity table is the caller's [c0(k), c0(k + 1))
int vicgpu_group_set_retire_on_error(vicgpu_group* g, int mask) {
  if (!g) return VICGPU_ERR_ARG;
  return group_each(g, [&](int k) { return vicgpu_set_retire_on_error(g->ctx[k], mask); });
}

int vicgpu_group_set_cell_valid(vicgpu_group* g, const int* valid) {
  if (!g || !valid) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  return group_each(g, [&](int k) { return vicgpu_set_cell_valid(g->ctx[k], valid + g->c0(k)); });
}

int vicgpu_group_get_cell_valid(vicgpu_group* g, int* valid) {
  if (!g || !valid) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  return group_each(g, [&](int k) { return vicgpu_get_cell_valid(g->ctx[k], valid + g->c0(k)); });
}

int vicgpu_group_glacier_mass_balance_fit(vicgpu_group* g, double* eq, int reset) {
  if (!g || !eq) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  return group_each(g, [&](int k) { return glacier_fit_impl(g->ctx[k], eq + g->c0(k), reset, g->ncell); });
}

// Model state copied between cells (vicgpu_copy_cells, vicgpu.h) in the caller's global cell order; a pair's cells may lie in
// different shards.  The plan is made on the whole domain, so every pair is checked before any shard writes.  Per table and
// row pass, two phases of all shards, every read before every write:
//   1. shard k packs what leaves its cells into its export buffer, one block [rows][pairs k -> s] per destination shard s
//      (its own staged pairs are the block k -> k), and waits for that;
//   2. shard s fetches the blocks k -> s of the other shards into its import buffer by plain device-to-device hipMemcpyAsync
//      (the runtime routes it between devices; no peer access is enabled, no kernel dereferences another device's memory)
//      and unpacks them and its own block s -> s into its tables, and waits for that.
// The row passes keep both buffers within the staging budget (VICGPU_COPY_STAGE_MB of the first shard's context).
struct GroupCopyKind {             // the pairs of one kind of column (HRUs or cells), by shard, in shard-local ids
  std::vector<std::vector<int>> src, dst;      // [k * ns + s]: pairs whose source is in shard k and whose destination in shard s
  std::vector<size_t> exp_off, imp_off;        // [k * ns + s]: first pair of the block in k's export list / in s's import list
  std::vector<size_t> exp_n, imp_n;            // [shard]: pairs it exports / imports from others
};

static void group_copy_kind(int ns, const CopyPairs& pairs, const std::vector<int>& shard, const std::vector<int>& local, GroupCopyKind& K) {
  K.src.assign((size_t)ns * ns, std::vector<int>()); K.dst.assign((size_t)ns * ns, std::vector<int>());
  for (size_t i = 0; i < pairs.size(); i++) {                // dst ascending, and so within every block
    const size_t b = (size_t)shard[pairs.src[i]] * ns + shard[pairs.dst[i]];
    K.src[b].push_back(local[pairs.src[i]]); K.dst[b].push_back(local[pairs.dst[i]]);
  }
  K.exp_off.assign((size_t)ns * ns, 0); K.imp_off.assign((size_t)ns * ns, 0);
  K.exp_n.assign(ns, 0); K.imp_n.assign(ns, 0);
  for (int k = 0; k < ns; k++)
    for (int s = 0; s < ns; s++) {
      const size_t b = (size_t)k * ns + s;
      K.exp_off[b] = K.exp_n[k]; K.exp_n[k] += K.src[b].size();
      if (k != s) { K.imp_off[b] = K.imp_n[s]; K.imp_n[s] += K.src[b].size(); }
    }
}

int vicgpu_group_copy_cells(vicgpu_group* g, int n, const int* dst_cell, const int* src_cell, int what) {
  if (!g || n < 0 || (n > 0 && (!dst_cell || !src_cell))) return VICGPU_ERR_ARG;
  if (what == 0 || (what & ~(VICGPU_COPY_STATE | VICGPU_COPY_BALANCE))) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  if (what & VICGPU_COPY_BALANCE)
    for (vicgpu_ctx* c : g->ctx)
      if (!c->dom.put_on) return group_fail(g, VICGPU_ERR_STATE, "copy_cells: VICGPU_COPY_BALANCE without a put_data configuration");
  const CopyPlan p = plan_cell_copy(g->ncell, g->nhru, g->cell_off.data(), g->cell_list.data(), g->copy_key.data(), COPY_NKEY, n, dst_cell, src_cell);
  if (p.fault != COPY_OK) return group_fail(g, VICGPU_ERR_ARG, copy_fault_text(p));
  if (p.cell.size() == 0) return VICGPU_OK;
  const int ns = g->nshard();
  GroupCopyKind kind[2];           // [0] HRUs, [1] cells
  group_copy_kind(ns, p.hru, g->hru_shard, g->hru_local, kind[0]);
  group_copy_kind(ns, p.cell, g->cell_shard, g->cell_local, kind[1]);
  // rows per pass of every table: the largest export or import list of its kind within the budget
  const size_t budget = (size_t)g->ctx[0]->tune.copy_stage_mb << 20;
  int rpp[COPY_NTABLE] = {0, 0, 0, 0};
  int nrow_of[COPY_NTABLE] = {0, 0, 0, 0};
  std::vector<size_t> exp_bytes(ns, 0), imp_bytes(ns, 0);
  for (int t = 0; t < COPY_NTABLE; t++)
    HIPIGN(copy_table(g->ctx[0], t, what, [&](auto* table, int nrow, size_t, bool per_cell) {
      const GroupCopyKind& K = kind[per_cell ? 1 : 0];
      size_t most = 0;
      for (int k = 0; k < ns; k++) most = std::max(most, std::max(K.exp_n[k], K.imp_n[k]));
      rpp[t] = rows_per_pass(budget, most, sizeof(*table), nrow);
      nrow_of[t] = nrow;
      for (int k = 0; k < ns; k++) {
        exp_bytes[k] = std::max(exp_bytes[k], (size_t)rpp[t] * K.exp_n[k] * sizeof(*table));
        imp_bytes[k] = std::max(imp_bytes[k], (size_t)rpp[t] * K.imp_n[k] * sizeof(*table));
      }
      return hipSuccess;
    }));
  // phase 0: every shard allocates what it needs and uploads its lists; nothing has been written when one of them is refused.
  // A shard's list: per kind, the sources of its export blocks, then the destinations of the blocks it unpacks (k -> s by k).
  std::vector<DevBuf<int>> idx(ns);
  std::vector<DevBuf<double>> exp_buf(ns), imp_buf(ns);
  std::vector<size_t> dst_at((size_t)2 * ns * ns, 0), src_at((size_t)2 * ns, 0);      // [kind][k][s] / [kind][shard]: position in the shard's list
  int r = group_each(g, [&](int s) {
    vicgpu_ctx* c = g->ctx[s];
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<int> h;
    for (int q = 0; q < 2; q++) {
      const GroupCopyKind& K = kind[q];
      src_at[(size_t)q * ns + s] = h.size();
      for (int to = 0; to < ns; to++) h.insert(h.end(), K.src[(size_t)s * ns + to].begin(), K.src[(size_t)s * ns + to].end());
      for (int k = 0; k < ns; k++) {
        dst_at[((size_t)q * ns + k) * ns + s] = h.size();
        h.insert(h.end(), K.dst[(size_t)k * ns + s].begin(), K.dst[(size_t)k * ns + s].end());
      }
    }
    if (h.empty()) return (int)VICGPU_OK;
    HIPCHK(c, idx[s].alloc(h.size()));
    if (exp_bytes[s]) HIPCHK(c, exp_buf[s].alloc((exp_bytes[s] + 7) / 8));
    if (imp_bytes[s]) HIPCHK(c, imp_buf[s].alloc((imp_bytes[s] + 7) / 8));
    HIPCHK(c, idx[s].upload(c->stream, h.data()));       // waits for the steps queued so far
    return (int)VICGPU_OK;
  });
  for (int t = 0; t < COPY_NTABLE && r == VICGPU_OK; t++)
    r = for_row_passes(nrow_of[t], rpp[t], [&](int r0, int nr) {
      const size_t cap = rpp[t];                       // rows a block is laid out for
      const int packed_all = group_each(g, [&](int k) {      // 1. pack
        vicgpu_ctx* c = g->ctx[k];
        HIPCHK(c, hipSetDevice(c->device));
        const hipError_t packed = copy_table(c, t, what, [&](auto* table, int, size_t ld, bool per_cell) {
          using T = typename std::remove_pointer<decltype(table)>::type;
          const int q = per_cell ? 1 : 0;
          const GroupCopyKind& K = kind[q];
          hipError_t e = hipSuccess;
          for (int s = 0; s < ns && e == hipSuccess; s++) {
            const size_t b = (size_t)k * ns + s;
            e = copy_pack<T>(c->stream, table, ld, r0, nr, idx[k].get() + src_at[(size_t)q * ns + k] + K.exp_off[b], (int)K.src[b].size(),
                             reinterpret_cast<T*>(exp_buf[k].get()) + cap * K.exp_off[b]);
          }
          return e;
        });
        HIPCHK(c, packed);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return (int)VICGPU_OK;
      });
      if (packed_all != VICGPU_OK) return packed_all;
      return group_each(g, [&](int s) {                // 2. fetch and unpack
        vicgpu_ctx* c = g->ctx[s];
        HIPCHK(c, hipSetDevice(c->device));
        const hipError_t unpacked = copy_table(c, t, what, [&](auto* table, int, size_t ld, bool per_cell) {
          using T = typename std::remove_pointer<decltype(table)>::type;
          const int q = per_cell ? 1 : 0;
          const GroupCopyKind& K = kind[q];
          hipError_t e = hipSuccess;
          for (int k = 0; k < ns && e == hipSuccess; k++) {
            const size_t b = (size_t)k * ns + s, np = K.src[b].size();
            if (np == 0) continue;
            const T* block = reinterpret_cast<const T*>(exp_buf[k].get()) + cap * K.exp_off[b];
            if (k != s) {
              T* mine = reinterpret_cast<T*>(imp_buf[s].get()) + cap * K.imp_off[b];
              e = hipMemcpyAsync(mine, block, sizeof(T) * nr * np, hipMemcpyDeviceToDevice, c->stream);
              block = mine;
            }
            if (e == hipSuccess) e = copy_unpack<T>(c->stream, table, ld, r0, nr, idx[s].get() + dst_at[((size_t)q * ns + k) * ns + s], (int)np, block);
          }
          return e;
        });
        HIPCHK(c, unpacked);
        HIPCHK(c, hipStreamSynchronize(c->stream));    // the next pass packs into the buffers the others have just read
        return (int)VICGPU_OK;
      });
    });
  if (r != VICGPU_OK)              // a shard's stream may still hold kernels on the buffers that go now
    for (vicgpu_ctx* c : g->ctx) vicgpu_synchronize(c);
  return r;
}

// Parameters updated in place (vicgpu_update_cell_params / vicgpu_update_hru_params, vicgpu.h) in the caller's global cell /
// HRU order.  The call is checked on the whole domain, so nothing is written when any entry is refused; then every shard
// takes its own columns, rebased, with their values gathered into a table of its own, on the group's threads.  The dense form
// stays dense in every shard (its cells are a block of the caller's, its HRUs are numbered in the caller's order).  The
// group keeps no host copy of the parameter tables: there is nothing else to keep in step.
static int group_update_params(vicgpu_group* g, bool per_cell, int nrow, const int* rows, int n, const int* cols, const double* values) {
  if (!g || nrow < 0 || n < 0) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  if (nrow == 0 || n == 0) return VICGPU_OK;
  if (!rows || !values) return group_fail(g, VICGPU_ERR_ARG, "update params: null rows or values");
  const int table_rows = per_cell ? (int)VICGPU_CP_NROW(g->opt.Nnode, g->opt.Nband) : (int)HPD_NROW;
  const char* name = per_cell ? "update_cell_params" : "update_hru_params";
  const ParamFault f = check_param_update(table_rows, per_cell ? g->ncell : g->nhru, nrow, rows, n, cols);
  if (f.rule != PARAM_OK) return group_fail(g, VICGPU_ERR_ARG, param_fault_message(name, f));
  const GroupColumns L = group_columns(g, per_cell, n, cols);
  return group_each(g, [&](int k) {
    const size_t nk = L.pos[k].size();
    if (nk == 0) return (int)VICGPU_OK;
    std::vector<double> v;
    take_columns(values, nrow, (size_t)n, L.pos[k], v);
    return per_cell ? vicgpu_update_cell_params(g->ctx[k], nrow, rows, (int)nk, L.idx(k), v.data())
                    : vicgpu_update_hru_params(g->ctx[k], nrow, rows, (int)nk, L.idx(k), v.data());
  });
}

int vicgpu_group_update_cell_params(vicgpu_group* g, int nrow, const int* rows, int n, const int* cells, const double* values) {
  return group_update_params(g, true, nrow, rows, n, cells, values);
}

int vicgpu_group_update_hru_params(vicgpu_group* g, int nrow, const int* rows, int n, const int* hrus, const double* values) {
  return group_update_params(g, false, nrow, rows, n, hrus, values);
}

int vicgpu_group_get_cell_params(vicgpu_group* g, double* cell_params) {
  if (!g || !cell_params) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  return group_each(g, [&](int k) { return get_cell_params_impl(g->ctx[k], cell_params + g->c0(k), g->ncell); });
}

int vicgpu_group_get_hru_params(vicgpu_group* g, double* hru_dparams) {
  if (!g || !hru_dparams) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  return group_each(g, [&](int k) {
    std::vector<double> p((size_t)HPD_NROW * g->hru[k].size());
    const int r = vicgpu_get_hru_params(g->ctx[k], p.data());
    if (r == VICGPU_OK) merge_hru_table(g, k, p, HPD_NROW, hru_dparams);
    return r;
  });
}

// Model state rows read and changed in place, the soil rows derived from them (vicgpu_get_state_rows / vicgpu_update_state /
// vicgpu_derive_soil_state, vicgpu.h) with HRU ids in the caller's global numbering.  The call is checked on the whole domain
// before any shard writes; then every shard takes its own columns, rebased, on the group's threads.
}  // extern "C": the helpers are templates

// op: ROWS_GET / ROWS_SET / ROWS_ADD of the context entries; INT: the SI table
template <typename T>
static int group_state_rows(vicgpu_group* g, const char* name, bool INT, int op, int nrow, const int* rows, int n, const int* hrus, T* values) {
  if (!g || nrow < 0 || n < 0) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  if (nrow == 0 || n == 0) return VICGPU_OK;
  if (!rows || !values) return group_fail(g, VICGPU_ERR_ARG, std::string(name) + ": null rows or values");
  const int table_rows = INT ? (int)VICGPU_SI_NROW(g->opt.Nnode) : (int)VICGPU_SD_NROW(g->opt.Nnode);
  const ParamFault f = check_param_update(table_rows, g->nhru, nrow, rows, n, hrus);
  if (f.rule != PARAM_OK) return group_fail(g, VICGPU_ERR_ARG, param_fault_message(name, f));
  const GroupColumns L = group_columns(g, false, n, hrus);
  return group_each(g, [&](int k) {
    const size_t nk = L.pos[k].size();
    if (nk == 0) return (int)VICGPU_OK;
    std::vector<T> v((size_t)nrow * nk);
    if (op != ROWS_GET) take_columns(values, nrow, (size_t)n, L.pos[k], v);
    const int* idx = L.idx(k);
    int rc;
    if constexpr (std::is_same<T, int>::value)
      rc = op == ROWS_GET ? vicgpu_get_state_rows_i(g->ctx[k], nrow, rows, (int)nk, idx, v.data()) : vicgpu_update_state_i(g->ctx[k], nrow, rows, (int)nk, idx, v.data());
    else
      rc = op == ROWS_GET ? vicgpu_get_state_rows(g->ctx[k], nrow, rows, (int)nk, idx, v.data())
                          : vicgpu_update_state(g->ctx[k], nrow, rows, (int)nk, idx, v.data(), op == ROWS_ADD ? VICGPU_STATE_ADD : VICGPU_STATE_SET);
    if (rc == VICGPU_OK && op == ROWS_GET) put_columns(values, nrow, (size_t)n, L.pos[k], v);      // the shards' positions in the caller's list are disjoint
    return rc;
  });
}

extern "C" {

int vicgpu_group_get_state_rows(vicgpu_group* g, int nrow, const int* rows, int n, const int* hrus, double* values) {
  return group_state_rows<double>(g, "get_state_rows", false, ROWS_GET, nrow, rows, n, hrus, values);
}

int vicgpu_group_get_state_rows_i(vicgpu_group* g, int nrow, const int* rows, int n, const int* hrus, int* values) {
  return group_state_rows<int>(g, "get_state_rows_i", true, ROWS_GET, nrow, rows, n, hrus, values);
}

int vicgpu_group_update_state(vicgpu_group* g, int nrow, const int* rows, int n, const int* hrus, const double* values, int mode) {
  if (mode != VICGPU_STATE_SET && mode != VICGPU_STATE_ADD) return VICGPU_ERR_ARG;
  return group_state_rows<double>(g, "update_state", false, mode == VICGPU_STATE_ADD ? ROWS_ADD : ROWS_SET, nrow, rows, n, hrus, const_cast<double*>(values));
}

int vicgpu_group_update_state_i(vicgpu_group* g, int nrow, const int* rows, int n, const int* hrus, const int* values) {
  return group_state_rows<int>(g, "update_state_i", true, ROWS_SET, nrow, rows, n, hrus, const_cast<int*>(values));
}

int vicgpu_group_derive_soil_state(vicgpu_group* g, int n, const int* hrus, int what) {
  if (!g || n < 0) return VICGPU_ERR_ARG;
  const int rule = check_derive_what(what, g->opt.GLACIER_DYNAMICS);
  if (rule == DERIVE_WHAT) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  if (rule == DERIVE_UNSUPPORTED) return group_fail(g, VICGPU_ERR_UNSUPPORTED, "derive_soil_state: VICGPU_DERIVE_CAP_MOIST with GLACIER_DYNAMICS");
  if (n == 0) return VICGPU_OK;
  const ParamFault f = check_param_update(0, g->nhru, 0, nullptr, n, hrus);
  if (f.rule != PARAM_OK) return group_fail(g, VICGPU_ERR_ARG, param_fault_message("derive_soil_state", f));
  const GroupColumns L = group_columns(g, false, n, hrus);
  return group_each(g, [&](int k) {
    const size_t nk = L.pos[k].size();
    if (nk == 0) return (int)VICGPU_OK;
    return vicgpu_derive_soil_state(g->ctx[k], (int)nk, L.idx(k), what);
  });
}

// Output records (vicgpu_out.h): every shard packs its own records and copies its columns into the caller's global tables
int vicgpu_group_records_config(vicgpu_group* g, int nvar, const int* var_ids, int depth) {
  if (!g || nvar < 0 || (nvar > 0 && !var_ids)) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  return group_each(g, [&](int k) { return vicgpu_records_config(g->ctx[k], nvar, var_ids, depth); });
}

int vicgpu_group_records_nrow(vicgpu_group* g) {
  if (!g) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  return vicgpu_records_nrow(g->ctx[0]);             // the same selection on every shard
}

int vicgpu_group_run_records(vicgpu_group* g, int step0, int nrecords, float* out, int* cell_err) {
  if (!g || !out) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  // cell groups (vicgpu_records_set_groups on a shard's context) have no group form: a shard's records are its columns
  for (vicgpu_ctx* c : g->ctx)
    if (c->rec.ngroup > 0) return group_fail(g, VICGPU_ERR_STATE, "a shard's records are reduced over cell groups: not supported in a device group");
  // the shards make the same checks on the same arguments before they queue anything, so either all of them run or none
  const int r = group_each(g, [&](int k) {
    return run_records_impl(g->ctx[k], step0, nrecords, out + g->c0(k), cell_err ? cell_err + g->c0(k) : nullptr, g->ncell);
  });
  if (r != VICGPU_OK)              // a shard that did start must leave no copy in flight either
    for (vicgpu_ctx* c : g->ctx) vicgpu_synchronize(c);
  return r;
}

int vicgpu_group_records_wait(vicgpu_group* g, int k) {
  if (!g) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  return group_each(g, [&](int s) { return vicgpu_records_wait(g->ctx[s], k); });
}

// State records: shard k's records are the global records [cell_hru_offset[b[k]], cell_hru_offset[b[k+1]]), in the same order
int vicgpu_group_get_state_records(vicgpu_group* g, double* rec) {
  if (!g || !rec) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  const size_t L = VICGPU_SR_LEN(g->opt.Nnode);
  return group_each(g, [&](int k) { return vicgpu_get_state_records(g->ctx[k], rec + (size_t)g->rec_first[k] * L); });
}

int vicgpu_group_set_state_records(vicgpu_group* g, const double* rec) {
  if (!g || !rec) return VICGPU_ERR_ARG;
  if (!group_ready(g)) return VICGPU_ERR_STATE;
  // every record of every shard first: a reader that throws changes nothing (vicgpu_set_state_records)
  const size_t L = VICGPU_SR_LEN(g->opt.Nnode);
  for (int j = 0; j < g->nhru; j++) {
    const std::string bad = check_state_record(rec + j * L, j, g->rec_band[j], g->rec_veg[j]);
    if (!bad.empty()) return group_fail(g, VICGPU_ERR_ARG, bad);
  }
  return group_each(g, [&](int k) { return vicgpu_set_state_records(g->ctx[k], rec + (size_t)g->rec_first[k] * L); });
}

}  // extern "C"
