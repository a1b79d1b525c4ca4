// nmg_table.hip -- object tables on the device: the sorted keys and LIFO
// entries of mem_list (FOREACH_HASH order, src/mem_analyzer.c:1820-1823), the
// lookup structures of lower_key (ht_lower_key, tools/hash.c:63-77), the
// partition-first path's partitions, and online table updates.
#include "nmg_engine_impl.h"

// The builders' 8 B and 16 B words (nmg_table_build.h) are what the kernels
// read as uint2 and uint4
static_assert(sizeof(Word8) == sizeof(uint2) && offsetof(Word8, x) == offsetof(uint2, x) &&
                  offsetof(Word8, y) == offsetof(uint2, y),
              "Word8 is uint2");
static_assert(sizeof(Word16) == sizeof(uint4) && offsetof(Word16, x) == offsetof(uint4, x) &&
                  offsetof(Word16, y) == offsetof(uint4, y) && offsetof(Word16, z) == offsetof(uint4, z) &&
                  offsetof(Word16, w) == offsetof(uint4, w),
              "Word16 is uint4");
static hipError_t alloc_copy(nmg_engine* h, DevBuf<uint2>& b, const std::vector<Word8>& src) {
  return alloc_copy(h, b, reinterpret_cast<const uint2*>(src.data()), src.size());
}
static hipError_t alloc_copy(nmg_engine* h, DevBuf<uint4>& b, const std::vector<Word16>& src) {
  return alloc_copy(h, b, reinterpret_cast<const uint4*>(src.data()), src.size());
}

// Lookup structures of a flattened table whose entries, in table order, are
// chain[] (ids in DevEntry::id): node records, then the LDS Eytzinger tree
// (<= kLdsNodes keys) or the fences + directory of the large-table path.
// chain_dev: chain already on the device (the by-id array), else uploaded.
int build_lookup(nmg_engine* h, LookupSet& l, const uint64_t* keys, const uint32_t* entry_off, uint32_t nb_keys,
                 const std::vector<DevEntry>& chain, DevEntry* chain_dev) {
  l.K = nb_keys;
  const std::vector<DevEntry> nodes = node_records(entry_off, nb_keys, chain);
  HIP_TRY(h, alloc_copy(h, l.keys, keys, nb_keys));
  HIP_TRY(h, alloc_copy(h, l.nodes, nodes));
  if (!chain_dev) HIP_TRY(h, alloc_copy(h, l.own_chain, chain));
  l.chain = chain_dev ? chain_dev : l.own_chain.get();
  l.elevels = l.nb_fences = l.fence_log2 = l.dir_log2 = 0;
  if (nb_keys <= kLdsNodes) {
    const SmallLookup sl = build_small_lookup(keys, nb_keys, nodes);
    l.elevels = sl.elevels;
    HIP_TRY(h, alloc_copy(h, l.efences, sl.ekeys));
    HIP_TRY(h, alloc_copy(h, l.enodes, sl.enodes));
  } else {
    BigLookup bl;
    build_big_lookup(keys, nb_keys, (h->flags & kDbgNoDir) != 0, bl);
    l.nb_fences = bl.nb_fences;
    l.fence_log2 = bl.fence_log2;
    l.dir_log2 = bl.dir_log2;
    HIP_TRY(h, alloc_copy(h, l.ffences, bl.efences));
    HIP_TRY(h, alloc_copy(h, l.fshift, bl.shift));
    HIP_TRY(h, alloc_copy(h, l.dir, bl.dir));
  }
  return NMG_OK;
}

// The partition-first path's tables (build_part_tables) of the table whose
// entries, in table order, are dev[]; `ids`: an online table's entry id per
// table position (nmg_update_objects), else null.  NMG_OK with h->rt.ok false:
// the table keeps the single-pass attribute_kernel.  Only for engines that
// count per object (NMG_F_MATCH_SAMPLES); the dump modes' per-sample output and
// the per-object levels are outputs of the local pass too (local_kernel's
// extras).  The engine's route table is replaced once every upload succeeded.
int build_partitions(nmg_engine* h, const uint64_t* keys, const uint32_t* entry_off, uint32_t K,
                     const std::vector<DevEntry>& dev, const uint32_t* ids) {
  h->rt = RouteTable();
  if (!(h->flags & NMG_F_MATCH_SAMPLES)) return NMG_OK;
  const PartTables pt =
      build_part_tables(TableInput{keys, entry_off, K, dev.data(), h->tab.npages.data(), ids, h->T, h->tab.cells()});
  if (!pt.ok) return NMG_OK;
  RouteTable rt;
  HIP_TRY(h, alloc_copy(h, rt.d_pdead, pt.pdead));
  HIP_TRY(h, alloc_copy(h, rt.d_parts, pt.parts));
  HIP_TRY(h, alloc_copy(h, rt.d_pbounds, pt.pbounds));
  HIP_TRY(h, alloc_copy(h, rt.d_pdir, pt.route.dir));
  HIP_TRY(h, alloc_copy(h, rt.d_pe_keys, pt.pe_keys));
  HIP_TRY(h, alloc_copy(h, rt.d_pe_nodes, pt.pe_nodes));
  HIP_TRY(h, alloc_copy(h, rt.d_pe_pnode, pt.pe_pnode));
  HIP_TRY(h, alloc_copy(h, rt.d_pe_old, pt.pe_old));
  HIP_TRY(h, alloc_copy(h, rt.d_pe_oinf, pt.pe_oinf));
  HIP_TRY(h, alloc_copy(h, rt.d_pe_info, pt.pe_info));
  HIP_TRY(h, alloc_copy(h, rt.d_pe_dir, pt.pe_dir));
  if (pt.online) {
    HIP_TRY(h, alloc_copy(h, rt.d_pe_ids, ids, entry_off[K]));
    HIP_TRY(h, alloc_copy(h, rt.d_pe_lrel, pt.pe_lrel));
    if (!pt.pe_cmap.empty()) HIP_TRY(h, alloc_copy(h, rt.d_pe_cmap, pt.pe_cmap));
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // (pageable sources)
  std::copy(pt.route.seg, pt.route.seg + kRouteSegs, rt.rsegs);
  rt.nrsegs = pt.route.nseg;
  rt.tbase = pt.tbase;
  rt.nparts = pt.nparts;
  rt.ok = true;
  h->rt = std::move(rt);
  return NMG_OK;
}

extern "C" int nmg_set_objects(nmg_engine* h, const uint64_t* keys, const uint32_t* entry_off,
                               uint32_t nb_keys, const nmg_object* entries, uint32_t nb_entries) {
  if (h) h->epoch++;
  if (h) h->counters_fresh = false;
  if (h) h->snap.lay.meta_dirty = h->cprep.lay.meta_dirty = h->place.obj_dirty = true;
  Range range("nmg_set_objects");
  if (!h || (nb_keys && (!keys || !entry_off)) || (nb_entries && !entries))
    return NMG_ERR_INVALID;
  int rc = check_table(h, keys, entry_off, nb_keys, nb_entries);
  if (rc) return rc;
  if (nb_entries >= (1u << 31)) return fail(h, NMG_ERR_RANGE, "too many entries");
  HIP_TRY(h, hipSetDevice(h->device));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  free_table(h);  // (released before the new ones are allocated: no second table's worth of HBM)
  h->cnt = Counters();
  h->tl = Timeline();  // (a timeline is laid out for one table)
  h->cost = PageCost();  // (and so are the page cost cells)
  h->lk.K = nb_keys;
  h->E = nb_entries;

  // page-histogram layout: dense [page][thread] block per entry within the
  // budget, otherwise sparse hashed cells (e.g. the 412 GB [stack] range)
  EntryTable& tab = h->tab;
  tab = EntryTable();
  tab.cur.threads = h->T;
  tab.cur.budget_cells = h->hist_budget / 4;
  tab.resize(nb_entries);
  h->order.clear();
  const bool want_hist = (h->flags & NMG_F_PAGE_HIST) && (h->flags & NMG_F_MATCH_SAMPLES);
  for (uint32_t e = 0; e < nb_entries; e++) {
    const nmg_object& o = entries[e];
    tab.describe(e, o);
    tab.npages[e] = o.buffer_size / kPageSize + 1;
    if (want_hist && tab.place(e, tab.npages[e], false) == kPlaceSparseFull)
      return fail(h, NMG_ERR_CAPACITY, "too many sparse entries");
    tab.dev_entries[e] = tab.dev_entry(e, o);
  }
  tab.cur.cells = tab.cur.padded_cells();
  HIP_TRY(h, alloc_copy(h, h->d_entries, tab.dev_entries));
  rc = build_lookup(h, h->lk, keys, entry_off, nb_keys, tab.dev_entries, h->d_entries);
  if (rc) return rc;
  rc = build_partitions(h, keys, entry_off, nb_keys, tab.dev_entries, nullptr);
  if (rc) return rc;
  h->cnt.set_sizes(nb_entries, h->flags & NMG_F_OBJECT_LEVELS);
  HIP_TRY(h, h->cnt.d_sum64.alloc(h->cnt.n_sum64));
  HIP_TRY(h, h->cnt.d_min64.alloc(h->cnt.n_min64));
  HIP_TRY(h, h->cnt.d_max64.alloc(h->cnt.n_max64));
  HIP_TRY(h, h->d_found.reserve(1));
  if (nb_entries > kObjSlots) {  // hashed object mode (see launch_attribution)
    HIP_TRY(h, h->cnt.d_pk64.alloc((size_t)nb_entries * 2));
    HIP_TRY(h, hipMemset(h->cnt.d_pk64, 0, (size_t)nb_entries * 2 * 8));
  }
  if (h->tab.cells()) HIP_TRY(h, h->cnt.d_hist.alloc(h->tab.cells() * h->T));
  if (!h->tab.sparse_entries.empty()) {
    HIP_TRY(h, h->cnt.d_sparse_keys.alloc(h->sparse_cap));
    HIP_TRY(h, h->cnt.d_sparse_vals.alloc(h->sparse_cap));
    HIP_TRY(h, h->cnt.d_sparse_dirty.alloc(2));
    const uint32_t ones[2] = {1u, 1u};  // the first reset clears the fresh table
    HIP_TRY(h, hipMemcpy(h->cnt.d_sparse_dirty, ones, 8, hipMemcpyHostToDevice));
  }
  h->have_table = true;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (nmg_engine* w : h->workers) {  // multi-GPU: the table on every device
    const int rc = nmg_set_objects(w, keys, entry_off, nb_keys, entries, nb_entries);
    if (rc) return fail(h, rc, w->last_error);
  }
  return nmg_reset_counters(h);
}


// The access timeline's cells for the current table: every entry with dense
// page cells (CellCursor::place) and at least min_object_bytes gets
// nb_bins * T * R cells, in id order; its base and R go into pad1 of its
// by-id record (tl_pad; kTlNone for the others), which is what the kernels
// gather.  The table-order copies of an nmg_update_objects table (chain, node
// records) carry pad1 too but nothing reads it there, so a later accepted
// update -- it rebuilds those from the host records -- keeps the bases.
extern "C" int nmg_set_timeline(nmg_engine* h, const nmg_timeline_options* o) {
  return nmg_set_timeline_ex(h, o, NMG_TL_SCOPE_DENSE);
}

// scope NMG_TL_SCOPE_ALL: the sparse entries of at least min_object_bytes are
// selected too.  They get no block: each gets an ordinal, in id order, into
// its pad1 (tl_pad_sparse), and their non-zero cells live in the timeline
// sparse table (Timeline::d_sp_keys / d_sp_vals), sparse_capacity slots of 12
// bytes within the same budget, allocated only when there is such an entry.
extern "C" int nmg_set_timeline_ex(nmg_engine* h, const nmg_timeline_options* o, uint32_t scope) {
  if (!h) return NMG_ERR_INVALID;
  h->epoch++;
  if (scope > NMG_TL_SCOPE_ALL)
    return fail(h, NMG_ERR_INVALID, "nmg_set_timeline_ex: scope is NMG_TL_SCOPE_DENSE or NMG_TL_SCOPE_ALL");
  if (h->multi || !h->workers.empty()) return fail(h, NMG_ERR_INVALID, "nmg_set_timeline: not on a multi-GPU handle");
  constexpr uint32_t kNeed = NMG_F_MATCH_SAMPLES | NMG_F_PAGE_HIST;
  if ((h->flags & kNeed) != kNeed)
    return fail(h, NMG_ERR_INVALID, "nmg_set_timeline needs an engine created with NMG_F_MATCH_SAMPLES | NMG_F_PAGE_HIST");
  if (o && (o->bin_shift > 63 || o->nb_bins < 1 || o->nb_bins > 4096 || o->row_shift > 20 || o->reserved != 0))
    return fail(h, NMG_ERR_INVALID, "nmg_set_timeline: option out of range (bin_shift <= 63, nb_bins 1..4096, "
                                    "row_shift <= 20, reserved 0)");
  if (!h->have_table) return fail(h, NMG_ERR_STATE, "nmg_set_timeline before nmg_set_objects");
  if (h->streaming) return fail(h, NMG_ERR_STATE, "nmg_set_timeline while a stream is open");
  HIP_TRY(h, hipSetDevice(h->device));
  int rc = route_settle(h);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // launches in flight read the entries and the cells
  if (!o) {
    h->tl = Timeline();
    return NMG_OK;
  }
  EntryTable& tab = h->tab;
  const uint32_t E = h->E, T = h->T;
  Timeline t;
  t.opt = *o;
  t.scope = scope;
  if (const char* r = getenv("NMG_TL_ROUNDS")) t.rounds = (uint32_t)std::min(64, std::max(0, atoi(r)));  // (see kTlRounds)
  const uint64_t budget = o->budget_bytes ? o->budget_bytes : (1ull << 30);
  unsigned __int128 need = 0;
  uint64_t nsparse = 0;  // selected sparse entries (past kTlMaxSparse refused below: only counted)
  for (uint32_t e = 0; e < E; e++) {
    if (tab.buffer_size[e] < o->min_object_bytes) continue;
    if (tab.hist_base[e] == kHistSparse) {
      if (scope == NMG_TL_SCOPE_ALL && nsparse++ < kTlMaxSparse) t.sp_ids.push_back(e);
      continue;
    }
    const uint64_t R = (tab.buffer_size[e] / kPageSize + 1 + (1ull << o->row_shift) - 1) >> o->row_shift;
    if (need <= 0xffffffffull) {  // (past it the layout is refused below: only the size is still summed)
      t.ids.push_back(e);
      t.base.push_back((uint32_t)need);
      t.nrows.push_back((uint32_t)R);  // (dense: R <= pages <= kMaxEntryCells)
    }
    need += (unsigned __int128)R * o->nb_bins * T;
  }
  if (nsparse > kTlMaxSparse) {
    char msg[224];
    snprintf(msg, sizeof(msg), "nmg_set_timeline_ex: %llu sparse entries selected, at most %u (raise min_object_bytes, "
                               "or the engine's hist_budget_bytes so that fewer entries are sparse)",
             (unsigned long long)nsparse, kTlMaxSparse);
    return fail(h, NMG_ERR_CAPACITY, msg);
  }
  t.sp_cap = t.sp_ids.empty() ? 0 : h->sparse_cap;
  const unsigned __int128 bytes = need * 4 + (unsigned __int128)t.sp_cap * 12;
  if (need > 0xffffffffull || bytes > budget) {
    char msg[224];
    if (t.sp_cap)
      snprintf(msg, sizeof(msg), "nmg_set_timeline_ex: the cells and the sparse table (%llu slots of 12 bytes) need %llu "
                                 "bytes (budget %llu, at most 2^32 - 1 cells)",
               (unsigned long long)t.sp_cap, bytes > ~0ull ? ~0ull : (unsigned long long)bytes, (unsigned long long)budget);
    else
      snprintf(msg, sizeof(msg), "nmg_set_timeline: the cells need %llu bytes (budget %llu, at most 2^32 - 1 cells)",
               bytes > ~0ull ? ~0ull : (unsigned long long)bytes, (unsigned long long)budget);
    return fail(h, NMG_ERR_CAPACITY, msg);
  }
  t.ncells = (uint64_t)need;
  t.base.push_back((uint32_t)t.ncells);
  // the new layout beside the current one; committed once everything is uploaded
  std::vector<DevEntry> dev = tab.dev_entries;
  for (DevEntry& d : dev) d.pad1 = kTlNone;
  for (size_t k = 0; k < t.ids.size(); k++) dev[t.ids[k]].pad1 = tl_pad(t.base[k], t.nrows[k]);
  for (size_t k = 0; k < t.sp_ids.size(); k++) dev[t.sp_ids[k]].pad1 = tl_pad_sparse((uint32_t)k);
  // (Params::tl switches the kernels' timeline code on; it is never null,
  // with sparse entries alone selected either: DevBuf::alloc(0))
  HIP_TRY(h, t.d_cells.alloc(t.ncells));
  HIP_TRY(h, hipMemsetAsync(t.d_cells, 0, t.ncells * 4, h->stream));
  HIP_TRY(h, alloc_copy(h, t.d_ids, t.ids));
  HIP_TRY(h, alloc_copy(h, t.d_base, t.base));
  HIP_TRY(h, alloc_copy(h, t.d_nrows, t.nrows));
  if (t.sp_cap) {
    HIP_TRY(h, t.d_sp_keys.alloc(t.sp_cap));
    HIP_TRY(h, t.d_sp_vals.alloc(t.sp_cap));
    HIP_TRY(h, hipMemsetAsync(t.d_sp_keys, 0xff, t.sp_cap * 8, h->stream));
    HIP_TRY(h, hipMemsetAsync(t.d_sp_vals, 0, t.sp_cap * 4, h->stream));
  }
  if (E) HIP_TRY(h, hipMemcpyAsync(h->d_entries, dev.data(), (size_t)E * sizeof(DevEntry), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // (pageable sources)
  tab.dev_entries = std::move(dev);
  t.on = true;
  h->tl = std::move(t);
  return NMG_OK;
}

// The page cost cells for the current table (the rule is in
// include/numamma_gpu.h): one u64 per cell of the page histogram, at its
// index, zeroed.  Nothing in the table changes: the kernels find a cell from
// the entry's histogram base, which they have.
extern "C" int nmg_set_page_cost(nmg_engine* h, const nmg_page_cost_options* o) {
  return nmg_set_page_cost_ex(h, o, NMG_COST_SCOPE_DENSE);
}

// scope NMG_COST_SCOPE_ALL: also one u64 per slot of the sparse page table
// (PageCost::d_sparse), within the same budget, whenever that table exists.
extern "C" int nmg_set_page_cost_ex(nmg_engine* h, const nmg_page_cost_options* o, uint32_t scope) {
  if (!h) return NMG_ERR_INVALID;
  h->epoch++;
  h->place.obj_dirty = true;  // (the object groups' members depend on the scope)
  if (scope > NMG_COST_SCOPE_ALL)
    return fail(h, NMG_ERR_INVALID, "nmg_set_page_cost_ex: scope is NMG_COST_SCOPE_DENSE or NMG_COST_SCOPE_ALL");
  if (h->multi || !h->workers.empty()) return fail(h, NMG_ERR_INVALID, "nmg_set_page_cost: not on a multi-GPU handle");
  constexpr uint32_t kNeed = NMG_F_MATCH_SAMPLES | NMG_F_PAGE_HIST;
  if ((h->flags & kNeed) != kNeed)
    return fail(h, NMG_ERR_INVALID, "nmg_set_page_cost needs an engine created with NMG_F_MATCH_SAMPLES | NMG_F_PAGE_HIST");
  if (o && (o->bucket_mask == 0 || o->bucket_mask >= (1u << 19) || o->access_mask == 0 || o->access_mask > 3 ||
            o->metric > NMG_COST_WEIGHT || o->reserved != 0))
    return fail(h, NMG_ERR_INVALID, "nmg_set_page_cost: option out of range (bucket_mask 1..2^19 - 1, access_mask 1..3, "
                                    "metric 0 or 1, reserved 0)");
  if (!h->have_table) return fail(h, NMG_ERR_STATE, "nmg_set_page_cost before nmg_set_objects");
  if (h->streaming) return fail(h, NMG_ERR_STATE, "nmg_set_page_cost while a stream is open");
  HIP_TRY(h, hipSetDevice(h->device));
  int rc = route_settle(h);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // launches in flight add to the cells
  if (!o) {
    h->cost = PageCost();
    return NMG_OK;
  }
  PageCost c;
  c.opt = *o;
  c.budget = o->budget_bytes ? o->budget_bytes : (1ull << 30);
  if (const char* r = getenv("NMG_COST_ROUNDS")) c.rounds = (uint32_t)std::min(64, std::max(0, atoi(r)));  // (see kCostRounds)
  c.scope = scope;
  const uint64_t ncells = h->tab.cells() * h->T;  // (within the histogram's budget: no overflow)
  const uint64_t nsparse = scope == NMG_COST_SCOPE_ALL && h->cnt.d_sparse_keys ? h->sparse_cap : 0;  // (<= 2^31)
  if ((ncells + nsparse) * 8 > c.budget) {
    char msg[160];
    snprintf(msg, sizeof(msg), "nmg_set_page_cost: the cells need %llu bytes (budget %llu)",
             (unsigned long long)((ncells + nsparse) * 8), (unsigned long long)c.budget);
    return fail(h, NMG_ERR_CAPACITY, msg);
  }
  if (ncells) {
    HIP_TRY(h, c.d_cells.alloc(ncells));
    HIP_TRY(h, hipMemsetAsync(c.d_cells, 0, ncells * 8, h->stream));
  }
  if (nsparse) {
    HIP_TRY(h, c.d_sparse.alloc(nsparse));
    HIP_TRY(h, hipMemsetAsync(c.d_sparse, 0, nsparse * 8, h->stream));
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  c.on = true;
  h->cost = std::move(c);
  return NMG_OK;
}

// A live --online-analysis table (nmg_update_objects) may hold entries the
// engine has not seen: objects created since the previous alarm (ids E ..
// newE - 1, _init_mem_info's next id, mem_analyzer.c:567-568, with their
// counters from creation, :569-572), and objects whose size at free
// (ma_record_free, :1287) outgrew their page cells.  New entries get page
// cells like nmg_set_objects gives them (dense within the budget, sparse
// otherwise); a dense entry that outgrew its cells moves to a new range with
// its counts.  Every id-indexed counter array is re-laid out on the device
// for the new entry count, counters kept.  (The stream is idle here.)
int grow_entries(nmg_engine* h, uint32_t newE, const uint32_t* ids, const nmg_object* objs, uint32_t n) {
  const uint32_t oldE = h->E;
  const uint64_t T = h->T;
  const bool want_hist = (h->flags & NMG_F_PAGE_HIST) && (h->flags & NMG_F_MATCH_SAMPLES);
  const bool levels = h->flags & NMG_F_OBJECT_LEVELS;
  EntryTable& tab = h->tab;
  const CellCursor cur0 = tab.cur;
  const uint64_t oldCells = cur0.cells;
  // The table is changed in place below, the cells and pages of every old
  // entry that grows journalled first; every error return undoes it (the new
  // entries dropped, the journal put back), so that a failed update keeps the
  // engine as it was.
  struct Old {
    uint32_t id;
    uint64_t hist, np;
  };
  std::vector<Old> changed;
  auto fail_rb = [&](int code, const std::string& msg) {
    for (auto it = changed.rbegin(); it != changed.rend(); ++it) {
      tab.dev_entries[it->id].hist = tab.hist_base[it->id] = it->hist;
      tab.npages[it->id] = it->np;
    }
    tab.truncate(oldE, cur0);
    return fail(h, code, msg);
  };
  tab.resize(newE);
  for (uint32_t j = 0; j < n; j++) {
    const uint32_t id = ids[j];
    const uint64_t np = objs[j].buffer_size / kPageSize + 1;
    if (id >= oldE) {
      tab.npages[id] = np;
      if (want_hist && tab.place(id, np, false) == kPlaceSparseFull)
        return fail_rb(NMG_ERR_CAPACITY, "too many sparse entries");
    } else if (np > tab.npages[id]) {
      changed.push_back({id, tab.hist_base[id], tab.npages[id]});
      if (want_hist && tab.hist_base[id] != kHistSparse && tab.place(id, np, true) != kPlaceDense)
        return fail_rb(NMG_ERR_CAPACITY, "an object outgrew its page cells past the histogram budget");
      tab.npages[id] = np;
    }
  }
  const uint64_t cells = tab.cur.cells = tab.cur.padded_cells();
  // the page cost cells follow the histogram's layout, within their own budget
  const bool with_cost = h->cost.on;
  const bool new_sparse = cur0.nsparse == 0 && tab.cur.nsparse && !h->cnt.d_sparse_keys;
  // (NMG_COST_SCOPE_ALL: plus the sparse table's, the one this update brings included)
  const bool cost_sparse = with_cost && h->cost.scope == NMG_COST_SCOPE_ALL && (h->cnt.d_sparse_keys || new_sparse);
  const uint64_t cost_bytes = (cells * T + (cost_sparse ? h->sparse_cap : 0)) * 8;
  if (with_cost && cost_bytes > h->cost.budget) {
    char msg[160];
    snprintf(msg, sizeof(msg), "nmg_update_objects: the page cost cells need %llu bytes (budget %llu)",
             (unsigned long long)cost_bytes, (unsigned long long)h->cost.budget);
    return fail_rb(NMG_ERR_CAPACITY, msg);
  }
  // id-indexed counters, re-laid out for newE entries
  const uint64_t n_sum = sum64_words(newE, levels), n_min = min64_words(newE);
  DevBuf<uint64_t> sum, mn, skeys, cost, scost;
  DevBuf<uint32_t> hist, svals, sdirty;
  DevBuf<unsigned long long> pk;
  DevBuf<DevEntry> ent;
  // (the new arrays are released on return, after the copies into them have drained)
  auto undo = [&](hipError_t e, const char* what) {
    (void)hipStreamSynchronize(h->stream);
    return fail_rb(NMG_ERR_HIP, std::string("nmg_update_objects: ") + what + ": " + hipGetErrorString(e));
  };
  hipError_t e;
  if ((e = sum.alloc(n_sum)) != hipSuccess) return undo(e, "counters");
  if ((e = mn.alloc(n_min)) != hipSuccess) return undo(e, "ordinals");
  if (cells && cells * T != oldCells * T && (e = hist.alloc(cells * T)) != hipSuccess)
    return undo(e, "page histogram");
  if (hist && with_cost && (e = cost.alloc(cells * T)) != hipSuccess) return undo(e, "page cost cells");
  if (newE > kObjSlots && (e = pk.alloc((size_t)newE * 2)) != hipSuccess) return undo(e, "packed counters");
  if ((e = ent.alloc(newE)) != hipSuccess) return undo(e, "entries");
  hipStream_t st = h->stream;
  if (new_sparse) {  // the first sparse entry: its table
    if ((e = skeys.alloc(h->sparse_cap)) != hipSuccess || (e = svals.alloc(h->sparse_cap)) != hipSuccess ||
        (e = sdirty.alloc(2)) != hipSuccess || (e = hipMemsetAsync(skeys, 0xff, h->sparse_cap * 8, st)) != hipSuccess ||
        (e = hipMemsetAsync(svals, 0, h->sparse_cap * 4, st)) != hipSuccess ||
        (e = hipMemsetAsync(sdirty, 0, 2 * 4, st)) != hipSuccess)
      return undo(e, "sparse page table");
    if (cost_sparse && ((e = scost.alloc(h->sparse_cap)) != hipSuccess ||
                        (e = hipMemsetAsync(scost, 0, h->sparse_cap * 8, st)) != hipSuccess))
      return undo(e, "sparse page cost cells");
  }
  // the global words as they are, the count/weight rows with the new stride,
  // the level rows and ordinals behind them, the error word at its new place
  const uint64_t* osum = h->cnt.d_sum64;
  const uint64_t* omin = h->cnt.d_min64;
  if ((e = hipMemsetAsync(sum, 0, n_sum * 8, st)) != hipSuccess ||
      (e = hipMemcpyAsync(sum, osum, kCwBase * 8, hipMemcpyDeviceToDevice, st)) != hipSuccess ||
      (oldE && (e = hipMemcpy2DAsync(sum + kCwBase, (size_t)newE * 8, osum + kCwBase, (size_t)oldE * 8, (size_t)oldE * 8,
                                     kCwRows, hipMemcpyDeviceToDevice, st)) != hipSuccess) ||
      (levels && oldE &&
       (e = hipMemcpyAsync(sum + levels_base(newE), osum + levels_base(oldE), (size_t)oldE * 2 * kLevelWords * 8,
                           hipMemcpyDeviceToDevice, st)) != hipSuccess) ||
      (e = hipMemsetAsync(mn, 0xff, n_min * 8, st)) != hipSuccess ||
      (e = hipMemcpyAsync(mn, omin, first_index(oldE) * 8, hipMemcpyDeviceToDevice, st)) != hipSuccess ||
      (e = hipMemcpyAsync(mn + error_index(newE), omin + error_index(oldE), 8, hipMemcpyDeviceToDevice, st)) !=
          hipSuccess ||
      (pk && (e = hipMemsetAsync(pk, 0, (size_t)newE * 2 * 8, st)) != hipSuccess) ||
      (e = hipMemcpyAsync(ent, tab.dev_entries.data(), (size_t)newE * sizeof(DevEntry), hipMemcpyHostToDevice, st)) !=
          hipSuccess)
    return undo(e, "re-layout");
  if (hist) {  // [thread][cell] rows with the new stride; moved entries' counts to their new range
    if ((e = hipMemsetAsync(hist, 0, cells * T * 4, st)) != hipSuccess ||
        (oldCells && (e = hipMemcpy2DAsync(hist, cells * 4, h->cnt.d_hist, oldCells * 4, oldCells * 4, T,
                                           hipMemcpyDeviceToDevice, st)) != hipSuccess))
      return undo(e, "page histogram re-layout");
    for (const Old& m : changed)  // (hist_base changed: a dense entry that moved)
      if (m.hist != tab.hist_base[m.id] &&
          ((e = hipMemcpy2DAsync(hist + tab.hist_base[m.id], cells * 4, hist + m.hist, cells * 4, m.np * 4, T,
                                 hipMemcpyDeviceToDevice, st)) != hipSuccess ||
           (e = hipMemset2DAsync(hist + m.hist, cells * 4, 0, m.np * 4, T, st)) != hipSuccess))
        return undo(e, "page cells of a grown object");
  }
  if (cost) {  // the same re-layout with 8-byte cells
    const uint64_t* ocost = h->cost.d_cells;
    if ((e = hipMemsetAsync(cost, 0, cells * T * 8, st)) != hipSuccess ||
        (oldCells && ocost && (e = hipMemcpy2DAsync(cost, cells * 8, ocost, oldCells * 8, oldCells * 8, T,
                                                    hipMemcpyDeviceToDevice, st)) != hipSuccess))
      return undo(e, "page cost re-layout");
    for (const Old& m : changed)
      if (m.hist != tab.hist_base[m.id] &&
          ((e = hipMemcpy2DAsync(cost + tab.hist_base[m.id], cells * 8, cost + m.hist, cells * 8, m.np * 8, T,
                                 hipMemcpyDeviceToDevice, st)) != hipSuccess ||
           (e = hipMemset2DAsync(cost + m.hist, cells * 8, 0, m.np * 8, T, st)) != hipSuccess))
        return undo(e, "page cost cells of a grown object");
  }
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return undo(e, "re-layout");
  // commit: the old arrays are released as the new ones move in
  if (!h->lk.own_chain) h->lk.chain = ent;  // (the table order is still the id order)
  h->cnt.d_sum64 = std::move(sum);
  h->cnt.d_min64 = std::move(mn);
  h->cnt.d_pk64 = std::move(pk);
  h->d_entries = std::move(ent);
  if (hist) h->cnt.d_hist = std::move(hist);
  if (cost) h->cost.d_cells = std::move(cost);
  h->cnt.set_sizes(newE, levels);
  h->E = newE;
  if (new_sparse) {
    h->cnt.d_sparse_keys = std::move(skeys);
    h->cnt.d_sparse_vals = std::move(svals);
    h->cnt.d_sparse_dirty = std::move(sdirty);
    if (scost) h->cost.d_sparse = std::move(scost);
  }
  return NMG_OK;
}

// --online-analysis: the table at an alarm, counters kept (mem_sampling.c:953-954
// against the live mem_list).  Entry ids index the counters: ids of the
// nmg_set_objects table, and (live hosts) ids past it for objects created
// since (grow_entries).  The report describes each entry as the latest table
// lists it, in the order of the latest table that lists every entry.
extern "C" int nmg_update_objects(nmg_engine* h, const uint64_t* keys, const uint32_t* entry_off,
                                  uint32_t nb_keys, const uint32_t* entry_ids, const nmg_object* objects) {
  if (h) h->epoch++;
  if (h) h->counters_fresh = false;  // (grown objects' page cells move)
  if (h) h->snap.lay.meta_dirty = h->cprep.lay.meta_dirty = h->place.obj_dirty = true;
  Range range("nmg_update_objects");
  if (!h || (nb_keys && (!keys || !entry_off || !entry_ids || !objects))) return NMG_ERR_INVALID;
  if (!h->have_table) return fail(h, NMG_ERR_STATE, "nmg_update_objects before nmg_set_objects");
  const uint32_t n = nb_keys ? entry_off[nb_keys] : 0;
  int rc = check_table(h, keys, nb_keys ? entry_off : nullptr, nb_keys, n);
  if (rc) return rc;
  // with a timeline set, its layout stands: no new entry, no size other than the one it was laid out for
  if (h->tl.on)
    for (uint32_t j = 0; j < n; j++)
      if (entry_ids[j] >= h->E || objects[j].buffer_size != h->tab.buffer_size[entry_ids[j]])
        return fail(h, NMG_ERR_STATE, "nmg_update_objects: with a timeline set, a table may only list existing "
                                      "entries with their sizes unchanged (drop it with nmg_set_timeline(h, NULL))");
  // ids: each at most once; new ones (>= E) consecutive from E
  uint32_t newE = h->E;
  for (uint32_t j = 0; j < n; j++) newE = std::max(newE, entry_ids[j] + 1);
  if (entry_ids && n && (uint64_t)newE > (1ull << 31)) return fail(h, NMG_ERR_RANGE, "too many entries");
  uint64_t nb_grown = 0;
  {
    std::vector<uint8_t> seen(newE, 0);
    for (uint32_t j = 0; j < n; j++) {
      const uint32_t id = entry_ids[j];
      if (seen[id]) return fail(h, NMG_ERR_INVALID, "an entry id listed twice in one table");
      seen[id] = 1;
      if (id < h->E && objects[j].buffer_size / kPageSize + 1 > h->tab.npages[id]) nb_grown++;
    }
    for (uint32_t id = h->E; id < newE; id++)
      if (!seen[id]) return fail(h, NMG_ERR_RANGE, "new entry ids must be consecutive from the current entry count");
  }
  HIP_TRY(h, hipSetDevice(h->device));
  if (h->streaming) {  // the open chunk belongs to the previous alarms' table
    rc = stream_flush(h);
    if (rc) return rc;
  }
  rc = route_settle(h);  // (reads the pool only, not the table)
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));  // launches in flight read the old table and counters
  if (h->multi_pending) {  // merges in flight write the counters being re-laid out
    rc = multi_finish(h);
    if (rc) return rc;
  }
  if (newE > h->E || nb_grown) {
    rc = grow_entries(h, newE, entry_ids, objects, n);
    if (rc) return rc;
  }
  std::vector<DevEntry> chain(n);
  for (uint32_t j = 0; j < n; j++) chain[j] = h->tab.dev_entry(entry_ids[j], objects[j]);
  h->rt = RouteTable();  // (the partitions describe the previous table)
  // build the alarm's lookup beside the current one; keep the current one if that fails
  LookupSet next;
  rc = build_lookup(h, next, keys, entry_off, nb_keys, chain, nullptr);
  if (rc == NMG_OK && hipStreamSynchronize(h->stream) != hipSuccess)
    rc = fail(h, NMG_ERR_HIP, "nmg_update_objects: table upload failed");
  if (rc) {
    (void)hipStreamSynchronize(h->stream);  // (`next` is released on return, after its uploads)
    return rc;
  }
  h->lk = std::move(next);
  // the report's view: every listed entry as this table lists it, and this
  // table's order when it lists every entry (ma_finalize walks the table it
  // has at exit, FOREACH_HASH, mem_analyzer.c:1381-1383)
  for (uint32_t j = 0; j < n; j++) h->tab.describe(entry_ids[j], objects[j]);
  if (n == h->E) {
    bool identity = true;
    for (uint32_t j = 0; j < n && identity; j++) identity = entry_ids[j] == j;
    if (identity) h->order.clear();
    else h->order.assign(entry_ids, entry_ids + n);
  } else if (!h->order.empty()) {
    // a partial table that brought new entries: they follow the known ones,
    // in id order, until a table lists every entry
    for (uint32_t id = (uint32_t)h->order.size(); id < h->E; id++) h->order.push_back(id);
  }
  // the alarm table's partitions.  The new table is committed above, so a
  // failure here is not the update's: the table stays on attribute_kernel
  // (no partitions) and the update goes on to the workers, which must get
  // the same table (a half-applied update would leave them on the old one).
  if (build_partitions(h, keys, entry_off, nb_keys, chain, entry_ids) != NMG_OK) {
    (void)hipGetLastError();
    h->rt = RouteTable();
  }
  for (nmg_engine* w : h->workers) {  // multi-GPU: the table on every device
    rc = nmg_update_objects(w, keys, entry_off, nb_keys, entry_ids, objects);
    if (rc) return fail(h, rc, w->last_error);
  }
  return NMG_OK;
}
