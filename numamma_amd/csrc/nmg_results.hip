// nmg_results.hip -- result getters (global and per-object counters, page
// cells), the merge arrays of the multi-GPU chain (export / import, packed page
// histogram, sparse cells, per-buffer counts).
#include <chrono>
#include "nmg_engine_impl.h"

namespace nmg {
int engine_download(nmg_engine* h, HostResults& r, bool entries, bool buffer_found) {
  if (buffer_found && !h->counts_override && !h->multi) {
    // per-buffer matched counts of the partition-first path: found_kernel
    // over the match bits (only for callers of the per-buffer counts; the
    // total below is counted by the analysis itself)
    HIP_TRY(h, hipSetDevice(h->device));
    const int rc = route_settle(h);
    if (rc) return rc;
  }
  int rc = nmg_synchronize(h);
  if (rc) return rc;
  // (entries == false: the global counters and per-buffer counts only, not
  // the per-entry arrays -- 40 MB at 1M entries)
  const uint64_t ns = entries ? h->cnt.n_sum64 : kCwBase, nm = entries ? h->cnt.n_min64 : kFirstBase;
  std::vector<uint64_t> sum(ns), mn(nm), mx(h->cnt.n_max64);
  HIP_TRY(h, hipMemcpy(sum.data(), h->cnt.d_sum64, ns * 8, hipMemcpyDeviceToHost));
  HIP_TRY(h, hipMemcpy(mn.data(), h->cnt.d_min64, nm * 8, hipMemcpyDeviceToHost));
  HIP_TRY(h, hipMemcpy(mx.data(), h->cnt.d_max64, h->cnt.n_max64 * 8, hipMemcpyDeviceToHost));
  global_counters(sum.data(), mn.data(), mx.data(), r.global);
  const uint64_t E = entries ? h->E : 0;
  r.first.assign(mn.begin() + first_index(0), mn.begin() + first_index(E));
  r.count_weight.resize(kCwRows * E);  // SoA [2][2][E] -> [E][2][2]
  for (uint64_t e = 0; e < E; e++)
    for (uint32_t a = 0; a < 2; a++)
      for (uint32_t w = 0; w < 2; w++) r.count_weight[e * kCwRows + a * 2 + w] = sum[objcw_index(e, a, w, E)];
  if ((h->flags & NMG_F_OBJECT_LEVELS) && entries)
    r.levels.assign(sum.begin() + levels_base(E), sum.end());
  else
    r.levels.clear();
  // mem_sampling_finalize accumulates the per-buffer int counters (:334-335);
  // a buffer holds < 2^29 records (< 4 GiB, Q14), so their sum is the
  // matched-sample total the kernels count (Params::found)
  r.nb_samples_total = 0;
  r.nb_found_total = 0;
  if (h->multi) {
    r.buf_samples = h->ov_samples;
    r.buf_bytes = h->ov_bytes;
    r.buf_found.assign(r.buf_samples.size(), 0);
    if (buffer_found && !r.buf_samples.empty()) {
      const int frc = multi_buffer_found(h, r.buf_found);
      if (frc) return frc;
    }
    r.nb_found_total = h->multi_found;
  } else if (h->counts_override) {
    r.buf_samples = h->ov_samples;
    r.buf_found = h->ov_found;
    r.buf_bytes = h->ov_bytes;
    for (size_t b = 0; b < r.buf_found.size(); b++) r.nb_found_total += (uint64_t)(int64_t)(int32_t)r.buf_found[b];
  } else {
    const size_t n = h->descs.size();
    r.buf_samples.assign(n, 0);
    r.buf_found.assign(n, 0);
    if (n) {
      HIP_TRY(h, hipMemcpy(r.buf_samples.data(), h->d_bufcnt, n * 4, hipMemcpyDeviceToHost));
      if (buffer_found)
        HIP_TRY(h, hipMemcpy(r.buf_found.data(), h->d_bufcnt + h->bufcnt_stride, n * 4, hipMemcpyDeviceToHost));
    }
    r.buf_bytes = h->buf_bytes;
    uint64_t found = 0;
    if (h->d_found) HIP_TRY(h, hipMemcpy(&found, h->d_found, 8, hipMemcpyDeviceToHost));
    r.nb_found_total = found;
  }
  for (size_t b = 0; b < r.buf_samples.size(); b++) r.nb_samples_total += (uint64_t)(int64_t)(int32_t)r.buf_samples[b];
  return NMG_OK;
}

int engine_download_hist(nmg_engine* h, std::vector<uint32_t>& cells) {
  int rc = nmg_synchronize(h);
  if (rc) return rc;
  cells.resize(h->tab.cells() * h->T);
  if (h->tab.cells()) HIP_TRY(h, hipMemcpy(cells.data(), h->cnt.d_hist, cells.size() * 4, hipMemcpyDeviceToHost));
  return NMG_OK;
}
}  // namespace nmg

extern "C" int nmg_get_global_counters(nmg_engine* h, nmg_mem_counters out[2], uint64_t* nb_samples,
                                       uint64_t* nb_found) {
  if (!h || !out) return NMG_ERR_INVALID;
  if (!h->have_table) return fail(h, NMG_ERR_STATE, "no object table");
  HostResults r;
  int rc = engine_download(h, r, false, false);
  if (rc) return rc;
  out[0] = r.global[0];
  out[1] = r.global[1];
  if (nb_samples) *nb_samples = r.nb_samples_total;
  if (nb_found) *nb_found = r.nb_found_total;
  return NMG_OK;
}

extern "C" int nmg_get_buffer_counts(nmg_engine* h, uint32_t* nb_samples, uint32_t* nb_found) {
  if (!h) return NMG_ERR_INVALID;
  if (!h->have_table) return fail(h, NMG_ERR_STATE, "no object table");
  HostResults r;
  int rc = engine_download(h, r, false, true);
  if (rc) return rc;
  if (nb_samples) memcpy(nb_samples, r.buf_samples.data(), r.buf_samples.size() * 4);
  if (nb_found) memcpy(nb_found, r.buf_found.data(), r.buf_found.size() * 4);
  return NMG_OK;
}

extern "C" int nmg_get_object_counters(nmg_engine* h, uint64_t* first_ordinal, uint64_t* count_weight) {
  if (!h) return NMG_ERR_INVALID;
  if (!h->have_table) return fail(h, NMG_ERR_STATE, "no object table");
  int rc = nmg_synchronize(h);
  if (rc) return rc;
  if (first_ordinal && h->E)
    HIP_TRY(h, hipMemcpy(first_ordinal, h->cnt.d_min64 + kFirstBase, (size_t)h->E * 8, hipMemcpyDeviceToHost));
  if (count_weight && h->E) {  // the SoA rows laid out per entry on the device, then one copy
    static_assert(objcw_index(1, 0, 0, 8) - objcw_index(0, 0, 0, 8) == 1 && objcw_index(0, 0, 1, 8) - objcw_index(0, 0, 0, 8) == 8 &&
                      objcw_index(0, 1, 0, 8) - objcw_index(0, 0, 0, 8) == 16,
                  "objcw_aos_kernel reads rows access * 2 + w");
    HIP_TRY(h, h->cnt.d_objcw.reserve((size_t)h->E * 4));
    HIP_TRY(h, launch_objcw_aos(h->stream, h->cnt.d_sum64 + kCwBase, h->E, h->cnt.d_objcw));
    HIP_TRY(h, hipMemcpyAsync(count_weight, h->cnt.d_objcw, (size_t)h->E * 32, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
  }
  return NMG_OK;
}

extern "C" int nmg_get_object_levels(nmg_engine* h, uint64_t* levels) {
  if (!h || !levels) return NMG_ERR_INVALID;
  if (!(h->flags & NMG_F_OBJECT_LEVELS)) return fail(h, NMG_ERR_STATE, "engine created without NMG_F_OBJECT_LEVELS");
  int rc = nmg_synchronize(h);
  if (rc) return rc;
  if (h->E)
    HIP_TRY(h, hipMemcpy(levels, h->cnt.d_sum64 + levels_base(h->E),
                         (size_t)h->E * 2 * kLevelWords * 8, hipMemcpyDeviceToHost));
  return NMG_OK;
}


// ---- the table's page-cell layout, shared by the synchronous getters
// (dense_rows / cells_fill) and the results snapshot

int CellLayout::ensure(nmg_engine* h, uint64_t newE, uint64_t new_nsent) {
  if (newE != E || !d_cnt) {  // (d_cnt: the last one allocated)
    HIP_TRY(h, d_base.alloc(newE + 1));
    HIP_TRY(h, d_off.alloc(newE + 1));
    HIP_TRY(h, d_part.alloc(scan_parts(newE) + 1));
    HIP_TRY(h, d_np.alloc(newE + 1));
    HIP_TRY(h, d_cnt.alloc(newE + 1));
    E = newE;
    meta_dirty = true;
  }
  if (new_nsent > nsent || !d_soff) {
    HIP_TRY(h, d_sent.alloc(new_nsent + 1));
    HIP_TRY(h, d_soff.alloc(new_nsent + 1));
    nsent = new_nsent;
    meta_dirty = true;
  }
  return NMG_OK;
}

// The table's cell layout into L, once per table: the entries' first cells,
// their dense pages (0: sparse) and the sparse entries as the current table
// has them (sparse idx -> entry; in sent_entry ~0 for one that is no longer
// sparse -- an online update gave it dense cells).  copy(h, dst, src, bytes) is
// the caller's H2D copy.
template <class Copy>
static int layout_upload(nmg_engine* h, CellLayout& L, std::vector<uint32_t>& sent_entry, Copy copy) {
  if (!L.meta_dirty) return NMG_OK;
  const uint64_t E = h->E, nsent = h->tab.sparse_entries.size();
  std::vector<uint32_t> np(E);
  for (uint64_t e = 0; e < E; e++) np[e] = h->tab.hist_base[e] == kHistSparse ? 0u : (uint32_t)h->tab.npages[e];
  sent_entry.resize(nsent);
  for (uint64_t s = 0; s < nsent; s++) {
    const uint32_t e = h->tab.sparse_entries[s];
    sent_entry[s] = h->tab.hist_base[e] == kHistSparse ? e : ~0u;
  }
  int rc = copy(h, L.d_base.get(), h->tab.hist_base.data(), E * 8);
  if (!rc) rc = copy(h, L.d_np.get(), np.data(), E * 4);
  if (!rc) rc = copy(h, L.d_sent.get(), h->tab.sparse_entries.data(), nsent * 4);
  if (!rc) L.meta_dirty = false;
  return rc;
}

// One page-cell row pass over a layout, each step enqueued on the engine
// stream: the synchronous getters (dense_rows) and nmg_results_begin run these.
// pass_count: per entry the rows of `cells` (the page histogram, or the cost
// cells at its index; null: no dense cell), then those of the sparse entries in
// the compacted words sw (null: none), into L.d_cnt; its scan gives L.d_off.
template <class CELL>
static hipError_t pass_count(nmg_engine* h, CellLayout& L, const CELL* cells, const SparseWords* sw) {
  hipError_t e = cells ? launch_cells_count(h->stream, cells, h->tab.cells(), h->T, L.d_base, L.d_np, h->E, L.d_cnt)
                       : hipMemsetAsync(L.d_cnt, 0, h->E * 4, h->stream);
  if (e == hipSuccess && sw)
    e = launch_cells_sparse_count(h->stream, sw->words(), sw->count(), sw->cap, L.d_sent,
                                  (uint32_t)h->tab.sparse_entries.size(), L.d_base, L.d_cnt);
  return e;
}
// the dense rows at their offsets (launch_cells_emit writes a page-cell row as one uint4)
static uint4* emit_rows(uint32_t* rows) { return reinterpret_cast<uint4*>(rows); }
template <class ROW>
static ROW* emit_rows(ROW* rows) { return rows; }
template <class CELL, class ROW>
static hipError_t pass_emit(nmg_engine* h, CellLayout& L, const CELL* cells, ROW* rows) {
  return launch_cells_emit(h->stream, cells, h->tab.cells(), h->T, L.d_base, L.d_np, h->E, L.d_off, emit_rows(rows));
}
// the sparse entries' first rows into L.d_soff
static hipError_t pass_soff(nmg_engine* h, CellLayout& L) {
  return launch_gather_off(h->stream, L.d_off, L.d_sent, (uint32_t)h->tab.sparse_entries.size(), L.d_soff);
}

// cprep.lay for the current table (the page cells' and the page cost cells' row passes)
static int cprep_layout(nmg_engine* h) {
  auto& P = h->cprep;
  const int rc = P.lay.ensure(h, h->E, h->tab.sparse_entries.size());
  return rc ? rc : layout_upload(h, P.lay, P.sent_entry, [](nmg_engine* h, void* dst, const void* src, size_t n) -> int {
    if (n) HIP_TRY(h, hipMemcpy(dst, src, n, hipMemcpyHostToDevice));
    return NMG_OK;
  });
}

struct Lap {  // NMG_CELLS_TIMING: the page cells' phase times on stderr
  bool on;
  std::chrono::steady_clock::time_point tp = std::chrono::steady_clock::now();
  void operator()(const char* what) {
    const auto now = std::chrono::steady_clock::now();
    if (on) fprintf(stderr, "cells_prepare: %-10s %.3f ms\n", what, std::chrono::duration<double, std::milli>(now - tp).count());
    tp = now;
  }
};

// The rows of one synchronous prepare over cprep's layout and work arrays:
// counted per entry -- the dense cells of `cells`, and the sparse table's from
// the words sw that the caller has just compacted and downloaded (null: none)
// -- scanned into row offsets, the dense ones emitted into s.d_rows; the sparse
// entries' first rows are read back into soff[nsent] for the fill (cells_fill /
// cost_fill).  A pass ends before it returns, so the page cells' and the cost
// cells' passes share the work arrays without meeting.
template <class CELL, class RS>
static int dense_rows(nmg_engine* h, const CELL* cells, RS& s, const SparseWords* sw, uint64_t* soff, Lap lap) {
  const uint64_t E = h->E, nsent = h->tab.sparse_entries.size();
  CellLayout& C = h->cprep.lay;
  uint64_t n = 0;
  if (E) {
    HIP_TRY(h, pass_count(h, C, cells, sw));
    const int rc = scan_total(h, C.d_cnt, E, C.d_off, C.d_part, &n, [&]() -> hipError_t {
      if (!sw) return hipSuccess;
      const hipError_t e = pass_soff(h, C);
      return e != hipSuccess ? e : hipMemcpyAsync(soff, C.d_soff, nsent * 8, hipMemcpyDeviceToHost, h->stream);
    });
    if (rc) return rc;
    lap("count");
    if (n) HIP_TRY(h, s.reserve(n));  // (sparse rows included: the fill copies s.n rows out)
    if (cells && n) {
      HIP_TRY(h, pass_emit(h, C, cells, s.d_rows.get()));
      HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    lap("emit");
  }
  s.n = (int64_t)n;
  return NMG_OK;
}

int SparseWords::download(nmg_engine* h, std::vector<uint64_t>& kv, const uint64_t* known) const {
  uint64_t n = known ? *known : 0;
  if (!known) {
    HIP_TRY(h, hipMemcpyAsync(&n, count(), 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
  }
  kv.resize(2 * n);
  if (n) HIP_TRY(h, hipMemcpy(kv.data(), words(), 2 * n * 8, hipMemcpyDeviceToHost));
  return NMG_OK;
}

// The table's used slots over vals (the counts, or the sparse cost cells) as
// words on the host, none while nothing was inserted since the last reset:
// compacted on the device into cnt.d_sparse_ck, so only they cross PCIe (the
// whole table is 12 MB at the default capacity)
template <class V>
static int sparse_fetch(nmg_engine* h, const V* vals, std::vector<uint64_t>& kv) {
  kv.clear();
  bool any = false;
  const int rc = sparse_nonempty(h, &any);
  if (rc || !any) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  SparseWords& sw = h->cnt.d_sparse_ck;
  HIP_TRY(h, sw.reserve(h->sparse_cap));
  HIP_TRY(h, sw.compact(h->stream, h->cnt.d_sparse_keys.get(), vals));
  return sw.download(h, kv);
}

// Every non-zero (entry, thread, page) cell, entries in id order, each
// entry's cells in (thread, page) order: the dense rows stay on the device
// until copied out, so only they cross PCIe, once; the sparse table's cells
// (entries past the dense budget, e.g. [stack]) are downloaded compacted and
// placed at their entries' offsets by cells_fill.
int cells_prepare(nmg_engine* h) {
  Lap lap{getenv("NMG_CELLS_TIMING") != nullptr};
  int rc = nmg_synchronize(h);
  if (rc) return rc;
  lap("sync");
  auto& P = h->cprep;
  rc = cprep_layout(h);
  if (rc) return rc;
  lap("meta");
  rc = sparse_download(h, P.sparse_kv);
  if (rc) return rc;
  lap("sparse");
  P.soff.assign(h->tab.sparse_entries.size(), 0);
  rc = dense_rows(h, h->tab.cells() && h->E ? h->cnt.d_hist.get() : nullptr, P.rows,
                  P.sparse_kv.empty() ? nullptr : &h->cnt.d_sparse_ck, P.soff.data(), lap);
  if (rc) return rc;
  if (lap.on) fprintf(stderr, "cells_prepare: %llu rows\n", (unsigned long long)P.rows.n);
  return NMG_OK;
}

// rows[s.n * 4]: dense rows D2H (none where the table has no dense cell), sparse rows placed
int cells_fill(nmg_engine* h, const RowSet<uint32_t, 4>& s, uint32_t* rows) {
  const auto t0 = std::chrono::steady_clock::now();
  const auto& P = h->cprep;
  if (h->tab.cells() && h->E) {
    const int rc = RowsCopy()(h, s, rows);
    if (rc) return rc;
  }
  if (getenv("NMG_CELLS_TIMING"))
    fprintf(stderr, "cells_fill: rows D2H %.3f ms\n",
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  place_sparse_rows(P.sparse_kv.data(), P.sparse_kv.size() / 2, P.sent_entry, P.soff.data(), rows);
  return NMG_OK;
}

extern "C" int64_t nmg_count_page_cells(nmg_engine* h) {
  if (!h || !h->have_table) return NMG_ERR_INVALID;
  return rows_count(h, h->cprep.rows, cells_prepare);
}

extern "C" int nmg_get_page_cells(nmg_engine* h, uint32_t* rows, int64_t n) {
  if (!h || !h->have_table || (n && !rows)) return NMG_ERR_INVALID;
  return rows_get(h, h->cprep.rows, cells_prepare, rows, n, cells_fill);
}

// ---- page cost rows: the dense rows of the u64 array (the options are the
// cells' own: nmg_set_page_cost bumps the epoch)
int cost_prepare(nmg_engine* h) {
  PageCost& c = h->cost;
  if (!c.on) return fail(h, NMG_ERR_STATE, "no page cost cells set (nmg_set_page_cost)");
  int rc = nmg_synchronize(h);
  if (rc) return rc;
  rc = cprep_layout(h);
  if (rc) return rc;
  c.rows.n = 0;
  // NMG_COST_SCOPE_ALL: the slots with a non-zero cost as (key, cost) words --
  // counted per entry by dense_rows, kept for cost_fill
  c.soff.assign(h->tab.sparse_entries.size(), 0);
  c.sparse_kv.clear();
  if (c.d_sparse) rc = sparse_fetch(h, c.d_sparse.get(), c.sparse_kv);
  if (rc) return rc;
  const bool any = !c.sparse_kv.empty();
  if (!c.d_cells && !any) return NMG_OK;
  return dense_rows(h, c.d_cells.get(), c.rows, any ? &h->cnt.d_sparse_ck : nullptr, c.soff.data(), Lap{false});
}

// rows[s.n * 4]: the rows D2H (the dense ones; none where the table has no dense cell), the sparse rows placed
int cost_fill(nmg_engine* h, const RowSet<uint64_t, 4>& s, uint64_t* rows) {
  const PageCost& c = h->cost;
  if (c.d_cells) {
    const int rc = RowsCopy()(h, s, rows);
    if (rc) return rc;
  }
  place_sparse_rows(c.sparse_kv.data(), c.sparse_kv.size() / 2, h->cprep.sent_entry, c.soff.data(), rows);
  return NMG_OK;
}

extern "C" int64_t nmg_count_cost_cells(nmg_engine* h) {
  if (!h) return NMG_ERR_INVALID;
  return rows_count(h, h->cost.rows, cost_prepare);
}

extern "C" int nmg_get_cost_cells(nmg_engine* h, uint64_t* rows, int64_t n) {
  if (!h || (n && !rows)) return NMG_ERR_INVALID;
  return rows_get(h, h->cost.rows, cost_prepare, rows, n, cost_fill);
}

// The timeline sparse table's used slots as (key, count) words on the host,
// sorted by key; none without such a table (the getters' rows and the merge's export)
static int timeline_sparse_fetch(nmg_engine* h, std::vector<uint64_t>& kv) {
  Timeline& t = h->tl;
  kv.clear();
  if (!t.on || !t.sp_cap) return NMG_OK;
  HIP_TRY(h, t.d_sp_ck.reserve(t.sp_cap));
  HIP_TRY(h, t.d_sp_ck.compact(h->stream, t.d_sp_keys.get(), t.d_sp_vals.get()));
  const int rc = t.d_sp_ck.download(h, kv);
  if (rc) return rc;
  sparse_words_sort(kv);
  return NMG_OK;
}

// ---- access timeline rows: counted per segment, scanned and emitted on the
// device (the page cells' pattern)
int timeline_prepare(nmg_engine* h) {
  Timeline& t = h->tl;
  if (!t.on) return fail(h, NMG_ERR_STATE, "no timeline set (nmg_set_timeline)");
  int rc = nmg_synchronize(h);
  if (rc) return rc;
  uint64_t n = 0;
  const uint64_t nseg = (t.ncells + kTlSeg - 1) / kTlSeg;
  if (nseg) {
    hipStream_t st = h->stream;
    HIP_TRY(h, t.d_cnt.reserve(nseg));
    HIP_TRY(h, t.d_off.reserve(nseg + 1));
    HIP_TRY(h, t.d_part.reserve(scan_parts(nseg) + 1));
    HIP_TRY(h, launch_tl_count(st, t.d_cells, t.ncells, t.d_cnt));
    rc = scan_total(h, t.d_cnt, nseg, t.d_off, t.d_part, &n);
    if (rc) return rc;
    if (n) {
      HIP_TRY(h, t.rows.reserve(n));
      HIP_TRY(h, launch_tl_emit(st, t.d_cells, t.ncells, t.d_ids, t.d_base, t.d_nrows, (uint32_t)t.ids.size(), h->T,
                                t.d_off, t.rows.d_rows));
      HIP_TRY(h, hipStreamSynchronize(st));
    }
  }
  t.nd = (int64_t)n;
  // NMG_TL_SCOPE_ALL: the timeline sparse table's used slots, compacted on the
  // device so that only they cross PCIe, sorted by key -- (entry, bin, thread,
  // row) order -- and kept for timeline_fill
  rc = timeline_sparse_fetch(h, t.sp_kv);
  if (rc) return rc;
  t.rows.n = t.nd + (int64_t)(t.sp_kv.size() / 2);
  return NMG_OK;
}

// rows[s.n * 5]: the dense rows D2H into the tail, then merged with the sparse
// table's rows from the front (tl_merge_rows: each at its entry's position)
int timeline_fill(nmg_engine* h, const RowSet<uint32_t, 5>& s, uint32_t* rows) {
  const Timeline& t = h->tl;
  const uint64_t ns = t.sp_kv.size() / 2;
  uint32_t* dense = rows + ns * 5;
  if (t.nd) HIP_TRY(h, hipMemcpy(dense, s.d_rows, (size_t)t.nd * 5 * 4, hipMemcpyDeviceToHost));
  if (ns) tl_merge_rows(dense, (uint64_t)t.nd, t.sp_kv.data(), ns, t.sp_ids, rows);
  return NMG_OK;
}

extern "C" int64_t nmg_count_timeline_cells(nmg_engine* h) {
  if (!h) return NMG_ERR_INVALID;
  return rows_count(h, h->tl.rows, timeline_prepare);
}

extern "C" int nmg_get_timeline_cells(nmg_engine* h, uint32_t* rows, int64_t n) {
  if (!h || (n && !rows)) return NMG_ERR_INVALID;
  return rows_get(h, h->tl.rows, timeline_prepare, rows, n, timeline_fill);
}

// ---- multi-GPU merge support

extern "C" uint64_t nmg_array_size(nmg_engine* h, int which) {
  if (!h || !h->have_table) return 0;
  switch (which) {
    case NMG_ARR_SUM64: return h->cnt.n_sum64;
    case NMG_ARR_MIN64: return h->cnt.n_min64;
    case NMG_ARR_MAX64: return h->cnt.n_max64;
    case NMG_ARR_HIST32: return h->tab.cells() * h->T;
    case NMG_ARR_COST64: return h->cost.on ? h->tab.cells() * h->T : 0;
    case NMG_ARR_TL32: return h->tl.on ? h->tl.ncells : 0;
    default: return 0;
  }
}

void* array_ptr(nmg_engine* h, int which, size_t* bytes) {
  switch (which) {
    case NMG_ARR_SUM64: *bytes = h->cnt.n_sum64 * 8; return h->cnt.d_sum64;
    case NMG_ARR_MIN64: *bytes = h->cnt.n_min64 * 8; return h->cnt.d_min64;
    case NMG_ARR_MAX64: *bytes = h->cnt.n_max64 * 8; return h->cnt.d_max64;
    case NMG_ARR_HIST32: *bytes = h->tab.cells() * h->T * 4; return h->cnt.d_hist;
    case NMG_ARR_COST64: *bytes = h->cost.on ? h->tab.cells() * h->T * 8 : 0; return h->cost.d_cells;
    case NMG_ARR_TL32: *bytes = h->tl.on ? h->tl.ncells * 4 : 0; return h->tl.d_cells;
    default: *bytes = 0; return nullptr;
  }
}

extern "C" int nmg_export_array(nmg_engine* h, int which, void* d_dst) {
  Range range("nmg_export_array");
  if (!h || !h->have_table) return NMG_ERR_INVALID;
  size_t bytes = 0;
  void* src = array_ptr(h, which, &bytes);
  if (!bytes) return NMG_OK;
  if (!src || !d_dst) return NMG_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemcpyAsync(d_dst, src, bytes, hipMemcpyDeviceToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return NMG_OK;
}

extern "C" int nmg_import_array(nmg_engine* h, int which, const void* d_src) {
  if (h) h->epoch++;
  if (h) h->counters_fresh = false;
  Range range("nmg_import_array");
  if (!h || !h->have_table) return NMG_ERR_INVALID;
  size_t bytes = 0;
  void* dst = array_ptr(h, which, &bytes);
  if (!bytes) return NMG_OK;
  if (!dst || !d_src) return NMG_ERR_INVALID;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return NMG_OK;
}

int scratch_u64(nmg_engine* h) {
  HIP_TRY(h, h->d_scratch.reserve(2 + 1024 / 2));  // + nmg_hist_pack's 1024 u32 range counts
  return NMG_OK;
}

extern "C" int nmg_hist_pack(nmg_engine* h, uint32_t threshold, void* d_u8, void* d_ovf, uint64_t ovf_cap,
                             uint64_t* n_ovf) {
  Range range("nmg_hist_pack");
  if (!h || !h->have_table || !n_ovf || threshold > 255) return NMG_ERR_INVALID;
  const uint64_t cells = h->tab.cells() * h->T;
  *n_ovf = 0;
  if (!cells) return NMG_OK;
  if (!d_u8 || (ovf_cap && !d_ovf)) return NMG_ERR_INVALID;
  if (cells > (1ull << 32)) return fail(h, NMG_ERR_RANGE, "nmg_hist_pack: more than 2^32 cells");
  int rc = scratch_u64(h);
  if (rc) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemsetAsync(h->d_scratch, 0, 8, h->stream));
  HIP_TRY(h, launch_hist_pack(h->stream, h->cnt.d_hist, cells, threshold, d_u8, d_ovf, ovf_cap,
                              reinterpret_cast<unsigned long long*>(h->d_scratch.get()),
                              reinterpret_cast<uint32_t*>(h->d_scratch + 2)));
  HIP_TRY(h, hipMemcpyAsync(n_ovf, h->d_scratch, 8, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return NMG_OK;
}

extern "C" int nmg_hist_unpack(nmg_engine* h, const void* d_u8, const void* d_ovf, uint64_t n_ovf) {
  if (h) h->epoch++;
  if (h) h->counters_fresh = false;
  Range range("nmg_hist_unpack");
  if (!h || !h->have_table || (n_ovf && !d_ovf)) return NMG_ERR_INVALID;
  const uint64_t cells = h->tab.cells() * h->T;
  if (!cells) return NMG_OK;
  if (!d_u8) return NMG_ERR_INVALID;
  int rc = scratch_u64(h);
  if (rc) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemsetAsync(h->d_scratch + 1, 0, 8, h->stream));
  HIP_TRY(h, launch_hist_unpack(h->stream, h->cnt.d_hist, cells, d_u8, d_ovf, n_ovf,
                                reinterpret_cast<unsigned long long*>(h->d_scratch + 1)));
  uint64_t bad = 0;
  HIP_TRY(h, hipMemcpyAsync(&bad, h->d_scratch + 1, 8, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (bad) return fail(h, NMG_ERR_RANGE, "nmg_hist_unpack: overflow entries outside the histogram");
  return NMG_OK;
}

// ---- packed cells: the page cost array (u64) or the timeline array (u32) as a
// list of its non-zero cells
static bool cells_array(int which) { return which == NMG_ARR_COST64 || which == NMG_ARR_TL32; }

extern "C" int nmg_cells_pack(nmg_engine* h, int which, void* d_list, uint64_t cap, uint64_t* n) {
  Range range("nmg_cells_pack");
  if (!h || !h->have_table || !n || !cells_array(which)) return NMG_ERR_INVALID;
  *n = 0;
  const uint64_t cells = nmg_array_size(h, which);
  if (!cells) return NMG_OK;
  if (cap && !d_list) return NMG_ERR_INVALID;
  int rc = scratch_u64(h);
  if (rc) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemsetAsync(h->d_scratch, 0, 8, h->stream));
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(h->d_scratch.get());
  uint32_t* wgcnt = reinterpret_cast<uint32_t*>(h->d_scratch + 2);
  if (which == NMG_ARR_COST64) HIP_TRY(h, launch_cells_pack(h->stream, h->cost.d_cells.get(), cells, d_list, cap, cnt, wgcnt));
  else HIP_TRY(h, launch_cells_pack(h->stream, h->tl.d_cells.get(), cells, d_list, cap, cnt, wgcnt));
  HIP_TRY(h, hipMemcpyAsync(n, h->d_scratch, 8, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return NMG_OK;
}

extern "C" int nmg_cells_unpack_add(nmg_engine* h, int which, const void* d_list, uint64_t n) {
  if (h) h->epoch++;
  if (h) h->counters_fresh = false;
  Range range("nmg_cells_unpack_add");
  if (!h || !h->have_table || !cells_array(which)) return NMG_ERR_INVALID;
  const uint64_t cells = nmg_array_size(h, which);
  if (!cells || !n) return NMG_OK;
  if (!d_list) return NMG_ERR_INVALID;
  int rc = scratch_u64(h);
  if (rc) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemsetAsync(h->d_scratch + 1, 0, 8, h->stream));
  unsigned long long* bad_w = reinterpret_cast<unsigned long long*>(h->d_scratch + 1);
  if (which == NMG_ARR_COST64) HIP_TRY(h, launch_cells_add(h->stream, h->cost.d_cells.get(), cells, d_list, n, bad_w));
  else HIP_TRY(h, launch_cells_add(h->stream, h->tl.d_cells.get(), cells, d_list, n, bad_w));
  uint64_t bad = 0;
  HIP_TRY(h, hipMemcpyAsync(&bad, h->d_scratch + 1, 8, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (bad) return fail(h, NMG_ERR_RANGE, "nmg_cells_unpack_add: pairs outside the array");
  return NMG_OK;
}

extern "C" int nmg_objcw_pack(nmg_engine* h, const void* d_sum64, uint64_t threshold, void* d_u32, void* d_ovf,
                              uint64_t ovf_cap, uint64_t* n_ovf) {
  Range range("nmg_objcw_pack");
  if (!h || !h->have_table || !n_ovf || !threshold) return NMG_ERR_INVALID;
  const uint64_t n = 4ull * h->E;
  *n_ovf = 0;
  if (!n) return NMG_OK;
  if (!d_sum64 || !d_u32 || (ovf_cap && !d_ovf)) return NMG_ERR_INVALID;
  int rc = scratch_u64(h);
  if (rc) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemsetAsync(h->d_scratch, 0, 8, h->stream));
  const uint64_t* rows = reinterpret_cast<const uint64_t*>(d_sum64) + objcw_index(0, 0, 0, h->E);
  HIP_TRY(h, launch_objcw_pack(h->stream, rows, n, threshold, d_u32, d_ovf, ovf_cap,
                               reinterpret_cast<unsigned long long*>(h->d_scratch.get())));
  HIP_TRY(h, hipMemcpyAsync(n_ovf, h->d_scratch, 8, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return NMG_OK;
}

extern "C" int nmg_objcw_unpack(nmg_engine* h, void* d_sum64, const void* d_u32, const void* d_ovf, uint64_t n_ovf) {
  Range range("nmg_objcw_unpack");
  if (!h || !h->have_table || (n_ovf && !d_ovf)) return NMG_ERR_INVALID;
  const uint64_t n = 4ull * h->E;
  if (!n) return NMG_OK;
  if (!d_sum64 || !d_u32) return NMG_ERR_INVALID;
  int rc = scratch_u64(h);
  if (rc) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemsetAsync(h->d_scratch + 1, 0, 8, h->stream));
  uint64_t* rows = reinterpret_cast<uint64_t*>(d_sum64) + objcw_index(0, 0, 0, h->E);
  HIP_TRY(h, launch_objcw_unpack(h->stream, rows, n, d_u32, d_ovf, n_ovf,
                                 reinterpret_cast<unsigned long long*>(h->d_scratch + 1)));
  uint64_t bad = 0;
  HIP_TRY(h, hipMemcpyAsync(&bad, h->d_scratch + 1, 8, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (bad) return fail(h, NMG_ERR_RANGE, "nmg_objcw_unpack: overflow entries outside the rows");
  return NMG_OK;
}

// The sparse cells can be non-empty only when something was inserted (or
// imported) since the last reset: that reset cleared the table if it had been
// written, and the flag of the analyses after it is d_sparse_dirty[nreset & 1]
// (reset_kernel).  A 4-byte read instead of the whole table.
int sparse_nonempty(nmg_engine* h, bool* out) {
  *out = false;
  if (!h->cnt.d_sparse_keys) return NMG_OK;
  uint32_t dirty = 1;
  HIP_TRY(h, hipMemcpy(&dirty, h->cnt.d_sparse_dirty + (h->nreset & 1), 4, hipMemcpyDeviceToHost));
  *out = dirty != 0;
  return NMG_OK;
}

int sparse_download(nmg_engine* h, std::vector<uint64_t>& kv) {
  const int rc = nmg_synchronize(h);
  return rc ? rc : sparse_fetch(h, h->cnt.d_sparse_vals.get(), kv);
}

extern "C" int64_t nmg_sparse_count(nmg_engine* h) {
  if (!h || !h->have_table) return NMG_ERR_INVALID;
  std::vector<uint64_t> kv;
  int rc = sparse_download(h, kv);
  return rc ? rc : (int64_t)(kv.size() / 2);
}

extern "C" int nmg_sparse_export(nmg_engine* h, uint64_t* keys, uint32_t* counts, int64_t n) {
  if (!h || !h->have_table || (n && (!keys || !counts))) return NMG_ERR_INVALID;
  std::vector<uint64_t> kv;
  int rc = sparse_download(h, kv);
  if (rc) return rc;
  if ((int64_t)(kv.size() / 2) != n) return fail(h, NMG_ERR_INVALID, "sparse count mismatch");
  // in key order (the device compaction reserves its output slots per wave
  // with an atomic, so its order varies from run to run; keys are unique)
  sparse_words_sort(kv);
  for (int64_t i = 0; i < n; i++) {
    keys[i] = kv[2 * i];
    counts[i] = (uint32_t)kv[2 * i + 1];
  }
  return NMG_OK;
}

// nmg_sparse_import over n words (the callers end the results epoch): the table cleared and the
// words inserted on the device (sparse_add's hash and probing), so only they cross PCIe
int sparse_import_words(nmg_engine* h, const uint64_t* kv, uint64_t n) {
  if (!h->cnt.d_sparse_keys) return n ? fail(h, NMG_ERR_STATE, "no sparse table") : NMG_OK;
  if (n > h->sparse_cap) return fail(h, NMG_ERR_CAPACITY, "sparse table too small");
  HIP_TRY(h, hipSetDevice(h->device));
  int rc = nmg_synchronize(h);
  if (rc) return rc;
  SparseWords& sw = h->cnt.d_sparse_ck;  // (the words' staging)
  HIP_TRY(h, sw.reserve(h->sparse_cap));
  HIP_TRY(h, hipMemsetAsync(h->cnt.d_sparse_keys, 0xff, h->sparse_cap * 8, h->stream));
  HIP_TRY(h, hipMemsetAsync(h->cnt.d_sparse_vals, 0, h->sparse_cap * 4, h->stream));
  // (the slots move: the sparse cost cells start again -- the merge follows with nmg_sparse_import_ex(NMG_SPARSE_PAGE_COST))
  if (h->cost.d_sparse) HIP_TRY(h, hipMemsetAsync(h->cost.d_sparse, 0, h->sparse_cap * 8, h->stream));
  if (n) {
    HIP_TRY(h, hipMemcpyAsync(sw.words(), kv, 2 * n * 8, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, launch_sparse_insert(h->stream, h->cnt.d_sparse_keys, h->cnt.d_sparse_vals, h->sparse_cap, sw.words(), n));
    HIP_TRY(h, hipStreamSynchronize(h->stream));  // (kv is pageable)
  }
  const uint32_t one = 1;  // imported cells: the next reset must clear the table
  HIP_TRY(h, hipMemcpy(h->cnt.d_sparse_dirty + (h->nreset & 1), &one, 4, hipMemcpyHostToDevice));
  return NMG_OK;
}

extern "C" int nmg_sparse_import(nmg_engine* h, const uint64_t* keys, const uint32_t* counts, int64_t n) {
  if (h) h->epoch++;
  if (!h || !h->have_table || (n && (!keys || !counts))) return NMG_ERR_INVALID;
  std::vector<uint64_t> kv;  // (the import refuses the other n without reading a word)
  if (h->cnt.d_sparse_keys && (uint64_t)n <= h->sparse_cap)
    for (int64_t i = 0; i < n; i++) kv.insert(kv.end(), {keys[i], (uint64_t)counts[i]});
  return sparse_import_words(h, kv.data(), (uint64_t)n);
}

// ---- the sparse parts by kind (nmg_sparse_*_ex): the page counts, the sparse
// cost cells at the page table's keys, the timeline sparse table

// kind `which` as (key, value) words sorted by key: the used slots with a
// non-zero value, through the getters' compaction (SparseWords::compact)
static int sparse_words_ex(nmg_engine* h, uint32_t which, std::vector<uint64_t>& kv) {
  kv.clear();
  int rc = nmg_synchronize(h);
  if (rc) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  switch (which) {
    case NMG_SPARSE_PAGE_COUNTS: rc = sparse_fetch(h, h->cnt.d_sparse_vals.get(), kv); break;
    case NMG_SPARSE_PAGE_COST:
      if (h->cost.on && h->cost.d_sparse) rc = sparse_fetch(h, h->cost.d_sparse.get(), kv);
      break;
    case NMG_SPARSE_TIMELINE: return timeline_sparse_fetch(h, kv);  // (sorted there)
    default: return fail(h, NMG_ERR_INVALID, "nmg_sparse_*_ex: which is NMG_SPARSE_PAGE_COUNTS, _PAGE_COST or _TIMELINE");
  }
  if (!rc) sparse_words_sort(kv);
  return rc;
}

extern "C" int64_t nmg_sparse_count_ex(nmg_engine* h, uint32_t which) {
  if (!h || !h->have_table) return NMG_ERR_INVALID;
  std::vector<uint64_t> kv;
  const int rc = sparse_words_ex(h, which, kv);
  return rc ? rc : (int64_t)(kv.size() / 2);
}

extern "C" int nmg_sparse_export_ex(nmg_engine* h, uint32_t which, uint64_t* keys, uint64_t* vals, int64_t n) {
  if (!h || !h->have_table || n < 0 || (n && (!keys || !vals))) return NMG_ERR_INVALID;
  std::vector<uint64_t> kv;
  const int rc = sparse_words_ex(h, which, kv);
  if (rc) return rc;
  if ((int64_t)(kv.size() / 2) != n) return fail(h, NMG_ERR_INVALID, "sparse count mismatch");
  for (int64_t i = 0; i < n; i++) {
    keys[i] = kv[2 * i];
    vals[i] = kv[2 * i + 1];
  }
  return NMG_OK;
}

// n interleaved (key, value) words to the staging sw on the device (enqueued; kv pageable: the caller waits)
static int stage_words(nmg_engine* h, SparseWords& sw, uint64_t slots, const std::vector<uint64_t>& kv) {
  HIP_TRY(h, sw.reserve(slots));
  if (!kv.empty()) HIP_TRY(h, hipMemcpyAsync(sw.words(), kv.data(), kv.size() * 8, hipMemcpyHostToDevice, h->stream));
  return NMG_OK;
}

// NMG_SPARSE_PAGE_COST: every sparse cost cell zeroed, then each key's cost stored at its slot of the page table
static int sparse_cost_import(nmg_engine* h, const std::vector<uint64_t>& kv) {
  PageCost& c = h->cost;
  const uint64_t n = kv.size() / 2;
  if (!c.on || !c.d_sparse || !h->cnt.d_sparse_keys)
    return n ? fail(h, NMG_ERR_STATE, "nmg_sparse_import_ex: no sparse cost cells (nmg_set_page_cost_ex with "
                                      "NMG_COST_SCOPE_ALL on an engine with a sparse page table)")
             : NMG_OK;
  int rc = nmg_synchronize(h);
  if (rc) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemsetAsync(c.d_sparse, 0, h->sparse_cap * 8, h->stream));
  uint64_t bad = n > h->sparse_cap ? n - h->sparse_cap : 0;  // (unique keys past the slots: absent, whatever they are)
  if (n && !bad) {
    rc = scratch_u64(h);
    if (!rc) rc = stage_words(h, h->cnt.d_sparse_ck, h->sparse_cap, kv);
    if (rc) return rc;
    HIP_TRY(h, hipMemsetAsync(h->d_scratch + 1, 0, 8, h->stream));
    HIP_TRY(h, launch_sparse_cost_store(h->stream, h->cnt.d_sparse_keys, c.d_sparse, h->sparse_cap,
                                        h->cnt.d_sparse_ck.words(), n,
                                        reinterpret_cast<unsigned long long*>(h->d_scratch + 1)));
    HIP_TRY(h, hipMemcpyAsync(&bad, h->d_scratch + 1, 8, hipMemcpyDeviceToHost, h->stream));
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (bad) {
    HIP_TRY(h, hipMemset(c.d_sparse, 0, h->sparse_cap * 8));
    char msg[160];
    snprintf(msg, sizeof(msg), "nmg_sparse_import_ex: %llu cost keys absent from the sparse page table "
                               "(import the page counts first)", (unsigned long long)bad);
    return fail(h, NMG_ERR_INVALID, msg);
  }
  return NMG_OK;
}

// NMG_SPARSE_TIMELINE: the timeline sparse table cleared, then the pairs inserted with its own hash
static int timeline_sparse_import(nmg_engine* h, const std::vector<uint64_t>& kv) {
  Timeline& t = h->tl;
  const uint64_t n = kv.size() / 2;
  if (!t.on || !t.sp_cap)
    return n ? fail(h, NMG_ERR_STATE, "nmg_sparse_import_ex: no timeline sparse table (nmg_set_timeline_ex with "
                                      "NMG_TL_SCOPE_ALL and a sparse entry selected)")
             : NMG_OK;
  if (n > t.sp_cap) return fail(h, NMG_ERR_CAPACITY, "timeline sparse table too small");
  for (uint64_t i = 0; i < n; i++)
    if (kv[2 * i + 1] >> 32) return fail(h, NMG_ERR_RANGE, "nmg_sparse_import_ex: a timeline count of 2^32 or more");
  int rc = nmg_synchronize(h);
  if (rc) return rc;
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipMemsetAsync(t.d_sp_keys, 0xff, t.sp_cap * 8, h->stream));
  HIP_TRY(h, hipMemsetAsync(t.d_sp_vals, 0, t.sp_cap * 4, h->stream));
  rc = stage_words(h, t.d_sp_ck, t.sp_cap, kv);
  if (rc) return rc;
  HIP_TRY(h, launch_tl_sparse_insert(h->stream, t.d_sp_keys, t.d_sp_vals, t.sp_cap, t.d_sp_ck.words(), n));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  t.sp_touched = true;  // imported cells: the next reset must clear the table
  return NMG_OK;
}

extern "C" int nmg_sparse_import_ex(nmg_engine* h, uint32_t which, const uint64_t* keys, const uint64_t* vals,
                                    int64_t n) {
  if (h) h->epoch++;
  if (!h || !h->have_table || n < 0 || (n && (!keys || !vals))) return NMG_ERR_INVALID;
  if (which > NMG_SPARSE_TIMELINE)
    return fail(h, NMG_ERR_INVALID, "nmg_sparse_import_ex: which is NMG_SPARSE_PAGE_COUNTS, _PAGE_COST or _TIMELINE");
  std::vector<uint64_t> kv;
  kv.reserve(2 * (size_t)n);
  for (int64_t i = 0; i < n; i++) kv.insert(kv.end(), {keys[i], vals[i]});
  if (which == NMG_SPARSE_PAGE_COST) return sparse_cost_import(h, kv);
  if (which == NMG_SPARSE_TIMELINE) return timeline_sparse_import(h, kv);
  if (h->cnt.d_sparse_keys && (uint64_t)n <= h->sparse_cap)  // (sparse_import_words refuses the other n)
    for (int64_t i = 0; i < n; i++)
      if (vals[i] >> 32) return fail(h, NMG_ERR_RANGE, "nmg_sparse_import_ex: a page count of 2^32 or more");
  return sparse_import_words(h, kv.data(), (uint64_t)n);
}

extern "C" int nmg_set_buffer_counts(nmg_engine* h, uint32_t nb_buffers, const uint32_t* nb_samples,
                                     const uint32_t* nb_found, const uint64_t* buffer_bytes) {
  if (h) h->epoch++;
  if (!h || (nb_buffers && (!nb_samples || !nb_found || !buffer_bytes))) return NMG_ERR_INVALID;
  h->counts_override = true;
  h->ov_samples.assign(nb_samples, nb_samples + nb_buffers);
  h->ov_found.assign(nb_found, nb_found + nb_buffers);
  h->ov_bytes.assign(buffer_bytes, buffer_bytes + nb_buffers);
  return NMG_OK;
}

// ---- results snapshot (include/numamma_gpu.h: nmg_results_begin / end)

namespace nmg {
// device and pinned buffers of the snapshot, (re)allocated when the table or
// the buffer list outgrows them
static int snap_alloc(nmg_engine* h) {
  auto& S = h->snap;
  const uint64_t E = h->E, nb = h->descs.size(), nsent = h->tab.sparse_entries.size();
  const uint64_t rows = h->tab.cells() * h->T + (h->cnt.d_sparse_keys ? h->sparse_cap : 0);
  if (!S.stream) {
    HIP_TRY(h, hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking));
    HIP_TRY(h, hipEventCreateWithFlags(&S.ready, hipEventDisableTiming));
    HIP_TRY(h, hipEventCreateWithFlags(&S.copied, hipEventDisableTiming));
  }
  if (E != S.lay.E || !S.d_objcw) {
    HIP_TRY(h, S.d_min.alloc(min64_words(E)));
    HIP_TRY(h, S.d_objcw.alloc((E + 1) * 4));
  }
  const int rc = S.lay.ensure(h, E, nsent);
  if (rc) return rc;
  HIP_TRY(h, S.d_sum.reserve(kCwBase));
  HIP_TRY(h, S.d_max.reserve(max64_words()));
  HIP_TRY(h, S.d_found.reserve(1));
  HIP_TRY(h, S.d_bufcnt.reserve(2 * nb + 1));
  HIP_TRY(h, S.d_rows.reserve(rows + 1));
  if (h->cnt.d_sparse_keys) HIP_TRY(h, S.d_ck.reserve(h->sparse_cap));
  // pinned host copies (the rows grow on demand in nmg_results_end)
  HIP_TRY(h, S.h_sum.reserve(kCwBase));
  HIP_TRY(h, S.h_max.reserve(max64_words()));
  HIP_TRY(h, S.h_small.reserve(4));
  HIP_TRY(h, S.h_min.reserve(min64_words(E)));
  HIP_TRY(h, S.h_objcw.reserve((E + 1) * 4));
  HIP_TRY(h, S.h_bufcnt.reserve(2 * nb + 1));
  HIP_TRY(h, S.h_soff.reserve(nsent + 1));
  return NMG_OK;
}

}  // namespace nmg

extern "C" int nmg_results_begin(nmg_engine* h) {
  Range range("nmg_results_begin");
  if (!h) return NMG_ERR_INVALID;
  if (!h->have_table) return fail(h, NMG_ERR_STATE, "nmg_results_begin before nmg_set_objects");
  if (h->multi || h->counts_override)
    return fail(h, NMG_ERR_STATE, "nmg_results_begin: a multi-GPU handle or merged per-buffer counts");
  if (h->streaming) return fail(h, NMG_ERR_STATE, "nmg_results_begin while streaming");
  auto& S = h->snap;
  HIP_TRY(h, hipSetDevice(h->device));
  if (S.pending) {  // (a snapshot nobody ended: its copy must finish before the buffers are reused)
    HIP_TRY(h, hipStreamSynchronize(S.stream));
    S.pending = false;
  }
  int rc = route_settle(h);  // (the per-buffer matched counts of the last route analysis, enqueued)
  if (rc) return rc;
  rc = snap_alloc(h);
  if (rc) return rc;
  const uint64_t E = h->E, nb = h->descs.size(), nsent = h->tab.sparse_entries.size();
  hipStream_t st = h->stream;
  CellLayout& L = S.lay;
  // the table's cell layout through the pinned staging on the engine stream
  // (begin never waits for it), with the sparse entries as this table has them:
  // nmg_results_end places the sparse rows with these, whatever table the
  // engine holds by then
  rc = layout_upload(h, L, S.sent_entry, stage_h2d);
  if (rc) return rc;
  // the device snapshot, behind the enqueued analyses
  HIP_TRY(h, hipMemcpyAsync(S.d_sum, h->cnt.d_sum64, kCwBase * 8, hipMemcpyDeviceToDevice, st));
  HIP_TRY(h, hipMemcpyAsync(S.d_min, h->cnt.d_min64, first_index(E) * 8, hipMemcpyDeviceToDevice, st));
  HIP_TRY(h, hipMemcpyAsync(S.d_max, h->cnt.d_max64, max64_words() * 8, hipMemcpyDeviceToDevice, st));
  if (nb) {
    HIP_TRY(h, hipMemcpyAsync(S.d_bufcnt, h->d_bufcnt, nb * 4, hipMemcpyDeviceToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(S.d_bufcnt + nb, h->d_bufcnt + h->bufcnt_stride, nb * 4, hipMemcpyDeviceToDevice, st));
  }
  if (h->d_found) HIP_TRY(h, hipMemcpyAsync(S.d_found, h->d_found, 8, hipMemcpyDeviceToDevice, st));
  else HIP_TRY(h, hipMemsetAsync(S.d_found, 0, 8, st));
  if (E) HIP_TRY(h, launch_objcw_aos(st, h->cnt.d_sum64 + kCwBase, E, S.d_objcw));
  // page-cell rows, the synchronous getters' pass without a wait: per-entry
  // counts (dense, then the sparse table's from its words compacted here),
  // their exclusive scan, the dense rows; the sparse ones are placed by the host
  const uint32_t* hist = h->tab.cells() ? h->cnt.d_hist.get() : nullptr;
  const SparseWords* sw = h->cnt.d_sparse_keys ? &S.d_ck : nullptr;  // (d_ck may outlive a table that had sparse cells)
  if (sw) HIP_TRY(h, sw->compact(st, h->cnt.d_sparse_keys.get(), h->cnt.d_sparse_vals.get()));
  if (E) {
    HIP_TRY(h, pass_count(h, L, hist, sw));
    HIP_TRY(h, launch_scan_u32(st, L.d_cnt, E, L.d_off, L.d_part));
    if (hist) HIP_TRY(h, pass_emit(h, L, hist, S.d_rows.get()));
    HIP_TRY(h, pass_soff(h, L));
  } else {
    HIP_TRY(h, hipMemsetAsync(L.d_off, 0, 8, st));
  }
  HIP_TRY(h, hipEventRecord(S.ready, st));
  // the copy to pinned host memory, on the snapshot's own stream
  hipStream_t cs = S.stream;
  HIP_TRY(h, hipStreamWaitEvent(cs, S.ready, 0));
  HIP_TRY(h, hipMemcpyAsync(S.h_sum, S.d_sum, kCwBase * 8, hipMemcpyDeviceToHost, cs));
  HIP_TRY(h, hipMemcpyAsync(S.h_min, S.d_min, first_index(E) * 8, hipMemcpyDeviceToHost, cs));
  HIP_TRY(h, hipMemcpyAsync(S.h_max, S.d_max, max64_words() * 8, hipMemcpyDeviceToHost, cs));
  if (nb) HIP_TRY(h, hipMemcpyAsync(S.h_bufcnt, S.d_bufcnt, 2 * nb * 4, hipMemcpyDeviceToHost, cs));
  HIP_TRY(h, hipMemcpyAsync(S.h_small, S.d_found, 8, hipMemcpyDeviceToHost, cs));
  HIP_TRY(h, hipMemcpyAsync(S.h_small + 1, L.d_off + E, 8, hipMemcpyDeviceToHost, cs));
  if (sw) HIP_TRY(h, hipMemcpyAsync(S.h_small + 2, sw->count(), 8, hipMemcpyDeviceToHost, cs));
  else S.h_small[2] = 0;
  if (E) HIP_TRY(h, hipMemcpyAsync(S.h_objcw, S.d_objcw, E * 32, hipMemcpyDeviceToHost, cs));
  if (nsent) HIP_TRY(h, hipMemcpyAsync(S.h_soff, L.d_soff, nsent * 8, hipMemcpyDeviceToHost, cs));
  if (S.h_rows) {  // (the rows' number is on the device: a kernel copies them)
    void* dst = nullptr;
    HIP_TRY(h, hipHostGetDevicePointer(&dst, S.h_rows, 0));
    HIP_TRY(h, launch_copy_rows(cs, S.d_rows, L.d_off + E, S.h_rows.cap() / 4, dst));
  }
  HIP_TRY(h, hipEventRecord(S.copied, cs));
  S.pending = true;
  h->snap_nb = nb;
  return NMG_OK;
}

extern "C" int nmg_results_end(nmg_engine* h, nmg_results_view* out) {
  Range range("nmg_results_end");
  if (!h || !out) return NMG_ERR_INVALID;
  auto& S = h->snap;
  if (!S.pending) return fail(h, NMG_ERR_STATE, "nmg_results_end without nmg_results_begin");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipEventSynchronize(S.copied));
  S.pending = false;
  const uint64_t E = S.lay.E, nb = h->snap_nb;  // (the begin-time table's)
  const uint64_t nrows = S.h_small[1], nspc = S.h_small[2];
  if (nrows * 4 > S.h_rows.cap()) {  // (the pinned rows outgrown: grown, and this time copied here)
    HIP_TRY(h, S.h_rows.reserve((nrows + nrows / 4 + 1024) * 4));
    HIP_TRY(h, hipMemcpy(S.h_rows, S.d_rows, nrows * 16, hipMemcpyDeviceToHost));
  }
  if (nspc) {  // the sparse cells, each entry's in (thread, page) order at its rows
    std::vector<uint64_t> kv;
    const int rc = S.d_ck.download(h, kv, &nspc);
    if (rc) return rc;
    place_sparse_rows<uint32_t>(kv.data(), nspc, S.sent_entry, S.h_soff, S.h_rows);
  }
  memset(out, 0, sizeof(*out));
  global_counters(S.h_sum, S.h_min, S.h_max, out->global);
  uint64_t ns = 0;
  for (uint64_t b = 0; b < nb; b++) ns += (uint64_t)(int64_t)(int32_t)S.h_bufcnt[b];
  out->nb_samples = ns;
  out->nb_found = S.h_small[0];
  out->nb_buffers = (uint32_t)nb;
  out->nb_entries = (uint32_t)E;
  out->buffer_samples = S.h_bufcnt;
  out->buffer_found = S.h_bufcnt + nb;
  out->first_ordinal = S.h_min + kFirstBase;
  out->count_weight = S.h_objcw;
  out->nb_cells = (int64_t)nrows;
  out->cells = S.h_rows;
  return NMG_OK;
}
