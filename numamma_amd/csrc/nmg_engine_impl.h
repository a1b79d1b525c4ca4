// nmg_engine_impl.h -- the host engine's internals, shared by its translation
// units (not part of the C-ABI):
//   nmg_engine.hip      C-ABI core: create / destroy / reset, analyze / synchronize,
//                       timers, nmg_report, debug getters
//   nmg_table.hip       object tables: upload, lookup structures, partitions,
//                       nmg_set_objects / nmg_update_objects (online growth)
//   nmg_submit.hip      buffer submission, zero-copy registration, the streaming
//                       pipeline, schedules and the single-pass launch
//   nmg_route_host.hip  the partition-first path's host side (pools, launches)
//   nmg_results.hip     result getters, page cells, merge arrays, sparse cells
//   nmg_multi.hip       multi-GPU handles (RCCL group reduce / device merge)
// Device and pinned host memory is held in DevBuf / PinBuf members
// (nmg_buffer.h): the engine and its sub-structs own their blocks, a group is
// released by assigning an empty one, and `delete` releases the rest.
#pragma once

#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <rocprofiler-sdk-roctx/roctx.h>

#include <algorithm>
#include <chrono>
#include <cinttypes>
#include <functional>
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <cstring>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "nmg_buffer.h"
#include "nmg_kernels.h"
#include "nmg_pool_layout.h"
#include "nmg_route.h"
#include "nmg_walk_order.h"

using namespace nmg;

// roctx range over one host-side stage (rocprofv3 --marker-trace): stage,
// attribution enqueue, merge, table swap, report
struct Range {
  explicit Range(const char* what) { roctxRangePushA(what); }
  ~Range() { roctxRangePop(); }
  Range(const Range&) = delete;
  Range& operator=(const Range&) = delete;
};

// Persistent host threads for the staging copies of nmg_submit_buffers (a
// batch per alarm in streaming mode would otherwise pay a thread start per
// copy thread per batch).
struct CopyPool {
  std::vector<std::thread> workers;
  std::mutex m;
  std::condition_variable wake, idle;
  std::function<void(uint32_t)> job;
  uint64_t gen = 0;
  uint32_t pending = 0;
  bool stop = false;

  explicit CopyPool(uint32_t n) {
    for (uint32_t w = 1; w < n; w++)
      workers.emplace_back([this, w] {
        uint64_t seen = 0;
        for (;;) {
          std::function<void(uint32_t)> f;
          {
            std::unique_lock<std::mutex> lk(m);
            wake.wait(lk, [&] { return stop || gen != seen; });
            if (stop) return;
            seen = gen;
            f = job;
          }
          f(w);
          std::lock_guard<std::mutex> lk(m);
          if (--pending == 0) idle.notify_one();
        }
      });
  }
  // run f(0..n-1) with worker w taking part w (the caller runs part 0)
  void run(const std::function<void(uint32_t)>& f) {
    {
      std::lock_guard<std::mutex> lk(m);
      job = f;
      pending = (uint32_t)workers.size();
      gen++;
    }
    wake.notify_all();
    f(0);
    std::unique_lock<std::mutex> lk(m);
    idle.wait(lk, [&] { return pending == 0; });
  }
  ~CopyPool() {
    {
      std::lock_guard<std::mutex> lk(m);
      stop = true;
    }
    wake.notify_all();
    for (auto& t : workers) t.join();
  }
};

struct nmg_engine;

// The lookup structures of one table and their shape (keys, node records, LDS
// tree or fences + directory, table-order entries).  Built beside the current
// one and moved in on success (nmg_update_objects).
struct LookupSet {
  DevBuf<uint64_t> keys;
  DevBuf<DevEntry> nodes;
  DevBuf<uint64_t> efences;  // small tables: Eytzinger-ordered keys / node records
  DevBuf<DevEntry> enodes;
  DevBuf<uint64_t> ffences;  // large tables: Eytzinger fences, directory shifts, directory
  DevBuf<uint8_t> fshift;
  DevBuf<uint2> dir;
  DevBuf<DevEntry> own_chain;  // table-order entries of an nmg_update_objects table; empty while
                               // the table order is the id order (nmg_set_objects)
  DevEntry* chain = nullptr;   // what the kernels read: own_chain, or the engine's d_entries
  uint32_t K = 0, elevels = 0, nb_fences = 0, fence_log2 = 0, dir_log2 = 0;
};

// the partitions of the partition-first path (nmg_route.h), built with the table
struct RouteTable {
  bool ok = false;  // partitions built for the current table
  uint32_t nparts = 0;
  RSeg rsegs[kRouteSegs] = {};  // the route pass's directory segments
  uint32_t nrsegs = 0;
  uint64_t tbase = 0;  // compact records: timestamps relative to this (XLayout)
  DevBuf<PartInfo> d_parts;
  DevBuf<uint64_t> d_pbounds;  // [kMaxParts + 1] partition starts, ascending
  DevBuf<uint16_t> d_pdir;     // [kRouteDir] the route pass's directory over them
  DevBuf<uint32_t> d_pdead;    // [(kMaxParts + 1) / 32] partitions no sample with ts != 0 can match
  DevBuf<uint64_t> d_pe_keys;  // [nparts][kPartSlots]
  DevBuf<uint4> d_pe_nodes;    // [nparts][kPartSlots][2]
  DevBuf<uint4> d_pe_pnode;    // [nparts][kPartSlots] packed node records (PackedNode)
  DevBuf<uint4> d_pe_old;      // [nparts][kOldLds] older entries, packed
  DevBuf<uint32_t> d_pe_oinf;  // [nparts][kOldLds]
  DevBuf<uint2> d_pe_info;     // [nparts][kPartSlots]
  DevBuf<uint4> d_pe_dir;      // [nparts][kPartDir] (PartDir)
  DevBuf<uint32_t> d_pe_ids;   // [table entries] entry id per table position (online tables; else empty)
  DevBuf<uint32_t> d_pe_lrel;  // [table entries] first packed LDS cell (online tables)
  DevBuf<uint32_t> d_pe_cmap;  // packed cell -> histogram cell (online tables)
};

// the per-analysis buffers of the partition-first path, sized together
// (route_pool): chunks = d_cmeta.cap(), grid = d_used.cap()
struct RoutePool {
  // chunk pool: (addr, ts) and X words of chunk id at pieces[id >> K][(id & (2^K - 1)) * kChunk ...]
  // (nmg_pool_layout.h); d_pieces = the pieces' base pointers, uploaded when the pool is built
  std::vector<DevBuf<uint4>> pieces;
  DevBuf<uint4*> d_pieces;
  uint4* pool0 = nullptr;  // the lowest piece
  uint32_t K = 0;
  uint64_t ids = 0, asked = 0;  // the last layout: chunk ids with the skipped ones, and the workgroups' capacities
  DevBuf<uint32_t> d_cmeta;   // [chunks], and so cmatch and clist: dense over the padded id space
  DevBuf<unsigned long long> d_cmatch;
  DevBuf<uint2> d_clist;      // per list entry: chunk id | fill, and the chunk's distance from pool0, in chunks
  DevBuf<uint4> d_items;
  DevBuf<uint32_t> d_chunk0;  // [grid + 1]
  DevBuf<uint32_t> d_used;    // [grid]
  DevBuf<uint32_t> d_pcnt;    // [grid][nparts]
  DevBuf<uint32_t> d_pbase;   // [nparts]
  DevBuf<uint32_t> d_ctl;     // [3] items, dequeue head, overflow records
  DevBuf<uint4> d_ovf16;      // overflow list (route pass, pool exhausted)
  DevBuf<unsigned long long> d_ovfx;
};

// The sparse table's used slots compacted on the device: n interleaved (key,
// value) u64 words (nmg_internal.h) in a block of 2 * cap + 1, n itself in the
// last one.  Only reserve / words / count know that layout.
struct SparseWords {
  DevBuf<uint64_t> d;
  uint64_t cap = 0;  // the table's slots
  hipError_t reserve(uint64_t slots) { return d.reserve(2 * (cap = slots) + 1); }
  uint64_t* words() const { return d; }
  unsigned long long* count() const { return reinterpret_cast<unsigned long long*>(d + 2 * cap); }
  // enqueued: the slots of (keys, vals)[cap] with a key and a non-zero value
  // (u32 counts, or u64 costs) into words(), their number into count()
  template <class V>
  hipError_t compact(hipStream_t st, const uint64_t* keys, const V* vals) const {
    const hipError_t e = hipMemsetAsync(count(), 0, 8, st);
    return e != hipSuccess ? e : launch_sparse_compact(st, keys, vals, cap, words(), count());
  }
  // the words on the host: count() read behind the engine stream's work (the
  // one wait; not where the caller has it in *known), then the 2n words copied
  int download(nmg_engine* h, std::vector<uint64_t>& kv, const uint64_t* known = nullptr) const;
};

// the counter arrays of one table (nmg_set_objects releases them with it),
// n_* their word counts (nmg_internal.h's layout for the table's entries)
struct Counters {
  DevBuf<uint64_t> d_sum64, d_min64, d_max64;
  uint64_t n_sum64 = 0, n_min64 = 0, n_max64 = 0;
  void set_sizes(uint64_t E, bool levels) {
    n_sum64 = sum64_words(E, levels);
    n_min64 = min64_words(E);
    n_max64 = max64_words();
  }
  DevBuf<uint32_t> d_hist;
  DevBuf<uint64_t> d_sparse_keys;
  DevBuf<uint32_t> d_sparse_vals;
  DevBuf<uint64_t> d_objcw;         // [entries][4] per-object counters laid out for the D2H
  SparseWords d_sparse_ck;          // the synchronous getters' compaction: (key, count) or (key, cost) words
  DevBuf<uint32_t> d_sparse_dirty;  // [2] parity flags (see reset_kernel)
  DevBuf<unsigned long long> d_pk64;  // hashed object mode: packed long-tail counters (0 between launches)
  DevBuf<uint4> d_tlog;             // hashed object mode: long-tail log (see Params::tlog)
  DevBuf<uint32_t> d_tlog_cnt;
};

// The table's page-cell layout on the device and the per-entry work arrays of
// one page-cell pass over it: the synchronous getters (CellsPrep) and the
// results snapshot (ResSnap) each keep one.
struct CellLayout {
  uint64_t E = 0, nsent = 0;
  bool meta_dirty = true;  // hist_base / npages / sparse entries changed: re-upload
  DevBuf<uint64_t> d_base, d_off, d_part, d_soff;
  DevBuf<uint32_t> d_np, d_cnt, d_sent;
  int ensure(nmg_engine* h, uint64_t E, uint64_t nsent);  // (re)allocated when the table outgrows them
};

// The rows of one product (DESIGN.md "Row sets"): n rows of WORDS words on the
// device and the results epoch they were prepared in (0: none).  Served by
// rows_count / rows_get / rows_collect below.
template <class W, uint32_t WORDS>
struct RowSet {
  using word = W;
  static constexpr uint32_t kWords = WORDS;
  DevBuf<W> d_rows;
  uint64_t epoch = 0;
  int64_t n = 0;
  hipError_t reserve(uint64_t rows) { return d_rows.reserve(rows * WORDS); }
};

// The access timeline (nmg_set_timeline): the cell array, the selected entries
// in id order (their cells lie in that order; each entry's base and rows are
// also in its DevEntry::pad1, tl_pad) and the getters' work arrays.
struct Timeline {
  bool on = false;
  nmg_timeline_options opt{};
  uint64_t ncells = 0;
  uint32_t rounds = kTlRounds;  // Params::tl_rounds
  DevBuf<uint32_t> d_cells;
  std::vector<uint32_t> ids, base, nrows;  // base has one more: ncells
  DevBuf<uint32_t> d_ids, d_base, d_nrows;
  RowSet<uint32_t, 5> rows;  // (entry, bin, thread, row, count)
  DevBuf<uint32_t> d_cnt;    // their per-segment counts, offsets and the scan's partial sums
  DevBuf<uint64_t> d_off, d_part;
  // NMG_TL_SCOPE_ALL: the selected sparse entries in id order (ordinal ->
  // entry; such an entry's pad1 is tl_pad_sparse(ordinal)) and their cells, the
  // timeline sparse table: sp_cap slots of a tl_sparse_key and a u32 count,
  // allocated only when sp_ids is not empty.  rows.n counts dense and sparse
  // rows; rows.d_rows holds the nd dense ones, sp_kv the table's used slots as
  // sorted (key, count) words: timeline_fill merges the two.
  uint32_t scope = NMG_TL_SCOPE_DENSE;
  std::vector<uint32_t> sp_ids;
  uint64_t sp_cap = 0;
  DevBuf<uint64_t> d_sp_keys;
  DevBuf<uint32_t> d_sp_vals;
  bool sp_touched = false;  // an analysis may have inserted since the table was last cleared
  SparseWords d_sp_ck;      // the getters' compaction
  std::vector<uint64_t> sp_kv;
  int64_t nd = 0;
};

// The page cost cells (nmg_set_page_cost): one u64 array parallel to the page
// histogram, cell (e, t, p) at t * tab.cells() + hist_base[e] + p -- the
// histogram's index, so it has no layout of its own and grow_entries re-lays
// it out with d_hist -- and the getters' rows.
struct PageCost {
  bool on = false;
  nmg_page_cost_options opt{};
  uint64_t budget = 0;             // bytes the array may take (opt.budget_bytes, or the default)
  uint32_t rounds = kCostRounds;   // Params::cost_rounds
  DevBuf<uint64_t> d_cells;        // [T * tab.cells()]; empty while the table has no dense cell
  RowSet<uint64_t, 4> rows;        // (entry, thread, page, value); the per-entry work arrays are cprep.lay's
  // NMG_COST_SCOPE_ALL: the sparse entries' cells, [sparse_cap] parallel to
  // cnt.d_sparse_keys / d_sparse_vals -- the cost of a key at the slot the
  // count table gave it; empty while the engine has no sparse page table.
  // The rows then hold dense and sparse rows, the sparse ones placed by
  // cost_fill from the compacted (key, cost) words and first rows kept here.
  uint32_t scope = NMG_COST_SCOPE_DENSE;
  DevBuf<uint64_t> d_sparse;
  std::vector<uint64_t> sparse_kv, soff;
};

// NUMA placement (nmg_placement.hip): groups on the device (PlaceParams'
// arrays), and the engine's state -- the object groups of the current table,
// the kernels' work arrays and the object blocks of the current results epoch.
struct PlaceDev {
  uint32_t G = 0;
  uint64_t pages = 0;
  DevBuf<uint32_t> gid, m_off, m_np;
  DevBuf<uint64_t> pg_off, m_base;
  // NMG_PLACE_HUGE: the H groups with a sparse member (PlaceHugeParams' arrays)
  uint32_t H = 0, DM = 0, nsent = 0;
  uint64_t dcells = 0;
  DevBuf<uint32_t> h_group, s_rank, s_lim, dm_rank;
  DevBuf<uint64_t> dm_off, dm_base;
};
struct PlaceState {
  bool obj_dirty = true;  // hist_base / npages changed: the object groups are built and uploaded again
  bool obj_huge = false;  // the object groups were built with every member (NMG_PLACE_HUGE, or the cost source
                          // on an engine with NMG_COST_SCOPE_ALL: place_all_members)
  PlaceDev obj;
  DevBuf<uint32_t> d_thr, d_noff, d_bcnt;
  DevBuf<uint64_t> d_pvcnt, d_boff, d_part;
  DevBuf<uint8_t> d_pvnode;
  // the huge groups' work arrays (run_huge)
  DevBuf<uint32_t> d_tnode, d_hflag, d_hpnode, d_hlnode;
  DevBuf<uint64_t> d_hkeys, d_hvals, d_hskeys, d_hsvals, d_hpcnt, d_hoff, d_hpart, d_hgfirst, d_hn;
  DevBuf<uint8_t> d_htmp;
  RowSet<uint64_t, 5> rows;  // (entry, node, start, end, count), made for the options below: others clear rows.epoch
  uint32_t N = 0, D = 0;
  uint64_t source = 0;  // nmg_placement_options::source of those rows
  std::vector<uint32_t> node;  // the thread -> node map of those rows (PlaceMap::node)
};

struct nmg_engine {
  int device = 0;
  uint32_t flags = NMG_F_DEFAULT;
  uint32_t T = 1;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  static constexpr int kRing = 64;  // per-launch timing events (nmg_get_launch_times)
  hipEvent_t ring0[kRing] = {}, ring1[kRing] = {};
  hipEvent_t ringm[kRing] = {};  // after the attribution kernel (before the log reduce)
  hipEvent_t ringr[kRing] = {};  // after the first kernel (route_kernel / attribute_kernel)
  uint64_t nlaunch = 0;
  int num_cus = 256;
  int blocks_per_cu = 0;
  bool launched = false;

  // object table
  bool have_table = false;
  // results epoch: bumped by every call that can change a counter; the row
  // sets (RowSet) prepared in one are served until the next
  uint64_t epoch = 1;
  // the counter arrays hold what the last reset wrote (no analysis, import or
  // table update since): the local pass may store instead of adding
  bool counters_fresh = false;
  // host memory registered with nmg_register_host (device-visible, pinned):
  // a submitted buffer inside it is read by the kernels in place over PCIe
  // (zc_dev[i] = its device address, 0 = staged)
  struct HostReg {
    uintptr_t lo, hi;  // the caller's range
    uint64_t dev;      // device address of lo
    void* pages;       // the registered whole pages around it
  };
  std::vector<HostReg> hostregs;
  std::vector<uint64_t> zc_dev;
  // results snapshot (nmg_results_begin / nmg_results_end, nmg_results.hip)
  struct ResSnap {
    hipStream_t stream = nullptr;
    hipEvent_t ready = nullptr, copied = nullptr;
    bool pending = false;
    CellLayout lay;
    DevBuf<uint64_t> d_sum, d_min, d_max, d_objcw, d_found;
    DevBuf<uint32_t> d_bufcnt;
    SparseWords d_ck;  // the sparse table's (key, count) words at nmg_results_begin
    DevBuf<uint4> d_rows;
    // pinned host copies
    PinBuf<uint64_t> h_sum, h_min, h_max, h_objcw, h_small, h_soff;  // h_small: [0] matched total, [1] rows,
                                                                     // [2] sparse cells
    PinBuf<uint32_t> h_bufcnt;
    PinBuf<uint32_t> h_rows;           // [rows][4], mapped: copy_rows_kernel writes it
    std::vector<uint32_t> sent_entry;  // begin-time table: sparse idx -> entry (~0: no longer sparse)
  } snap;
  uint64_t snap_nb = 0;  // buffers of the snapshot in flight
  // the synchronous page-cell getters' state (cells_prepare), kept across calls
  struct CellsPrep {
    CellLayout lay;
    RowSet<uint32_t, 4> rows;  // (entry, thread, page, count): n dense and sparse rows, the dense ones on the device
    // the sparse table's cells as downloaded ((key, count) words), the sparse
    // entries of that table and their first rows: placed by cells_fill
    std::vector<uint64_t> sparse_kv, soff;
    std::vector<uint32_t> sent_entry;
  } cprep;
  uint32_t E = 0;
  LookupSet lk;
  DevBuf<DevEntry> d_entries;  // by entry id (the nmg_set_objects table)
  EntryTable tab;  // E entries
  std::vector<uint32_t> order;      // report walk order (position -> id) when it is not the id order:
                                    // the latest table that listed every entry (nmg_update_objects)
  uint64_t hist_budget = 4ull << 30;
  uint64_t sparse_cap = 1u << 20;

  // counters
  Counters cnt;
  DevBuf<unsigned long long> d_found;  // matched SAMPLEs since the last reset (Params::found)
  DevBuf<uint64_t> d_scratch;          // [2] small device results (nmg_hist_pack / unpack) + range counts
  DevBuf<uint32_t> d_smatch;           // NMG_F_SAMPLE_MATCHES: per 8 B of the arena span
  Timeline tl;                         // nmg_set_timeline (dropped with the table)
  PageCost cost;                       // nmg_set_page_cost (dropped with the table)
  PlaceState place;                    // nmg_count_object_blocks / nmg_report_placement
  uint64_t nreset = 0;

  // buffers
  std::vector<BufDesc> descs;
  std::vector<uint64_t> buf_bytes;
  PinBuf<uint8_t> h_stage;
  size_t stage_len = 0;
  DevBuf<uint8_t> d_arena;
  const uint8_t* d_data = nullptr;
  bool external = false;
  bool staged_dirty = false;
  DevBuf<BufDesc> d_descs;
  DevBuf<BufDesc> d_sdescs;   // descriptors in stream-sorted schedule order
  DevBuf<uint32_t> d_ranges;  // per-workgroup [begin, end) in d_order
  // pinned staging of an analysis' small uploads (descriptors, schedule,
  // chunk pools): copied on the engine stream without a host wait
  PinBuf<uint8_t> up_pin;
  size_t up_off = 0;
  hipEvent_t up_ev = nullptr;
  bool up_recorded = false;
  uint32_t sched_grid = 0;       // grid the current schedule was built for
  bool descs_dirty = false;
  bool multi_staged = false;  // the workers' arenas hold the current buffers (multi_analyze)
  DevBuf<uint32_t> d_bufcnt;  // per-buffer counts, [2][bufcnt_stride] u32 of [2][d_bufcnt.cap() / 2]
  size_t bufcnt_stride = 0;

  // streaming (nmg_stream_begin): two staging halves, each a chunk in flight
  struct StreamSlot {
    PinBuf<uint8_t> h_stage;
    size_t len = 0;
    DevBuf<uint8_t> d_arena;
    PinBuf<uint8_t> h_sched;      // pinned schedule (sorted descriptors, then ranges)
    DevBuf<uint8_t> d_sched;
    std::vector<BufDesc> descs;   // this chunk: offset in the slot, global seq, .pad = global index
    hipEvent_t copied = nullptr;  // H2D of the chunk done: the host may refill h_stage
    hipEvent_t done = nullptr;    // kernel of the chunk done: the device may refill d_arena
    bool used = false;
  };
  bool streaming = false, streamed = false;
  uint64_t chunk_cap = 0;
  uint32_t copy_threads = 1;
  std::unique_ptr<CopyPool> pool;  // copy_threads - 1 workers, started on first use
  StreamSlot slots[2];
  int cur_slot = 0;
  hipStream_t copy_stream = nullptr;

  // multi-GPU override of per-buffer counts (rank 0 reporting)
  bool counts_override = false;
  std::vector<uint32_t> ov_samples, ov_found;
  std::vector<uint64_t> ov_bytes;

  std::string last_error;
  float last_ms = 0.f;

  // multi-GPU (nmg_options.nb_gpus > 1): this handle holds the submitted
  // buffers, the table and the merged counters; `workers` (one engine per
  // device, worker 0 on this handle's device) analyse contiguous ranges
  std::vector<nmg_engine*> workers;
  std::vector<int> devices;
  bool multi = false, multi_distinct = false, multi_pending = false;
  uint64_t multi_found = 0;  // matched SAMPLEs of the workers (multi_finish)
  // the merge of the last multi_analyze, timed on the root device's stream that
  // carries it (worker 0's for RCCL, this handle's for device merges): from
  // the end of worker 0's analysis to the end of the merges (nmg_get_merge_stats)
  hipEvent_t merge_ev0 = nullptr, merge_ev1 = nullptr;
  bool merge_timed = false;
  uint64_t merge_bytes = 0;  // counter bytes each worker contributes per merge
  std::vector<void*> comms;  // ncclComm_t per worker (distinct devices)
  std::vector<DevBuf<uint8_t>> warena;  // each on its worker's device

  // partition-first path for large tables (nmg_route.h): the partitions of
  // the current table, and the per-analysis chunk pool
  RouteTable rt;
  uint64_t route_launches = 0;    // analyses (or streamed chunks) that took the partition-first path
  RoutePool rpool;
  bool sched_route = false;       // d_sdescs / d_ranges hold the analysis-order schedule
  uint32_t route_sched_key = 0;   // what the pools were laid out for (route_key)
  bool route_pending = false;     // per-buffer match counts of the last route analysis not yet summed
  uint32_t route_grid = 0;
  XLayout route_xl{};
  XLayout route_last_xl{};        // the layout of the last route launch, streamed chunks included (nmg_debug_route_layout)

  // kDbgTiming (internal): per-wave phase cycles of the last launch
  DevBuf<uint64_t> d_dbg;
  size_t dbg_len = 0;
};

// what a schedule's workgroup pools depend on besides the buffers: nparts, the
// pool switches and the piece size of the pool they were laid out in
inline uint32_t route_key(const nmg_engine* h) {
  return h->rt.nparts | (h->rpool.K << 16) | ((h->flags & kDbgTinyPieces) ? 0x40000000u : 0u) |
         ((h->flags & kDbgTinyPool) ? 0x80000000u : 0u);
}

#define HIP_TRY(h, expr)                                                        \
  do {                                                                          \
    hipError_t _e = (expr);                                                     \
    if (_e != hipSuccess) {                                                     \
      (h)->last_error = std::string(#expr) + ": " + hipGetErrorString(_e);      \
      return NMG_ERR_HIP;                                                       \
    }                                                                           \
  } while (0)

// a host copy into pinned staging, run by one of the copy threads
struct CopyTask {
  uint8_t* dst;
  const uint8_t* src;
  uint64_t len;
};

// One partition-first analysis: a buffer set in HBM with its analysis-order
// schedule (the submitted buffers, or a streamed chunk whose per-buffer count
// slots start at index_base; a chunk settles its per-buffer matched counts at
// once, before the next chunk reuses the pool).
struct RouteJob {
  const std::vector<BufDesc>* descs;
  const uint8_t* data;
  const BufDesc* sdescs;
  const uint32_t* ranges;
  const uint32_t* chunk0;
  uint32_t grid, index_base;
  bool settle_now;
};

// engine-internal functions (hidden: not exported from the library)
#pragma GCC visibility push(hidden)
extern thread_local std::string g_create_error;  // detail of the last failed nmg_create (no handle holds it)
int fail(nmg_engine* h, int code, const std::string& msg);
// an H2D copy of n bytes from host memory the caller may reuse at once:
// through the pinned staging, on the engine stream, no host wait
int stage_h2d(nmg_engine* h, void* d_dst, const void* src, size_t n);
void stage_reset(nmg_engine* h);  // (an analysis' first upload: the staging from its start again)
void free_table(nmg_engine* h);  // the table's device structures: partitions, lookup, entries
// b = n elements of src, uploaded on the engine stream (src is read until the stream is synchronised)
template <class T>
hipError_t alloc_copy(nmg_engine* h, DevBuf<T>& b, const T* src, size_t n) {
  const hipError_t e = b.alloc(n);
  if (e != hipSuccess || !n) return e;
  return hipMemcpyAsync(b, src, n * sizeof(T), hipMemcpyHostToDevice, h->stream);
}
template <class T>
hipError_t alloc_copy(nmg_engine* h, DevBuf<T>& b, const std::vector<T>& src) {
  return alloc_copy(h, b, src.data(), src.size());
}
int check_table(nmg_engine* h, const uint64_t* keys, const uint32_t* entry_off, uint32_t nb_keys,
                       uint32_t n);
int build_lookup(nmg_engine* h, LookupSet& l, const uint64_t* keys, const uint32_t* entry_off, uint32_t nb_keys,
                 const std::vector<DevEntry>& chain, DevEntry* chain_dev);
int build_partitions(nmg_engine* h, const uint64_t* keys, const uint32_t* entry_off, uint32_t K,
                            const std::vector<DevEntry>& dev, const uint32_t* ids);
int grow_entries(nmg_engine* h, uint32_t newE, const uint32_t* ids, const nmg_object* objs, uint32_t n);
int stage_reserve(nmg_engine* h, size_t need);
int append_desc(nmg_engine* h, uint64_t len, uint32_t thread_rank, uint32_t access);
uint64_t zero_copy_dev(nmg_engine* h, const void* p, uint64_t len);
int append_desc_zc(nmg_engine* h, uint64_t dev, uint64_t len, uint32_t thread_rank, uint32_t access);
int check_buffer_args(nmg_engine* h, uint64_t len, uint32_t thread_rank, uint32_t access);
void run_copies(nmg_engine* h, const std::vector<CopyTask>& tasks);
int slot_acquire(nmg_engine* h, int s);
int ensure_bufcnt(nmg_engine* h, size_t need);
int ensure_dbg(nmg_engine* h, size_t words);  // the timing buffer: `words` u64, zeroed on the engine stream
int stream_flush(nmg_engine* h);
int stream_dst(nmg_engine* h, uint64_t len, uint8_t** dst, std::vector<CopyTask>* pending);
int stream_append(nmg_engine* h, uint64_t len, uint32_t thread_rank, uint32_t access);
int upload_buffers(nmg_engine* h);
void make_schedule(const std::vector<BufDesc>& descs, uint32_t grid, uint32_t index_base, BufDesc* sorted,
                          uint32_t* ranges, bool by_stream);
int build_schedule(nmg_engine* h, uint32_t grid, bool by_stream = true);
void ensure_occupancy(nmg_engine* h);
uint32_t attribution_grid(nmg_engine* h, uint32_t nb);
Params base_params(nmg_engine* h, const uint8_t* data, const BufDesc* sdescs, const uint32_t* ranges);
int launch_events(nmg_engine* h, int* slot_out);
int launch_attribution(nmg_engine* h, const uint8_t* data, const BufDesc* sdescs, const uint32_t* ranges,
                              uint32_t nb, uint32_t grid, uint64_t nbytes);
uint32_t bits_for(uint64_t v);
bool route_layout(nmg_engine* h, const std::vector<BufDesc>& descs, XLayout& xl);
bool route_eligible(nmg_engine* h, const std::vector<BufDesc>& descs);
bool route_eligible(nmg_engine* h);
int route_pool(nmg_engine* h, const std::vector<BufDesc>& descs, uint32_t grid, const uint32_t* ranges,
                      std::vector<uint32_t>& c0);
int route_prepare(nmg_engine* h, uint32_t grid, const std::vector<uint32_t>& ranges);
int route_analyze(nmg_engine* h, uint32_t nb, uint32_t grid);
int route_analyze_job(nmg_engine* h, const RouteJob& job);
int route_settle(nmg_engine* h);
int decode_error_word(nmg_engine* h, uint64_t w);
int cells_prepare(nmg_engine* h);
int cells_fill(nmg_engine* h, const RowSet<uint32_t, 4>& s, uint32_t* rows);  // rows_get's fill for the page cells
int timeline_prepare(nmg_engine* h);
int timeline_fill(nmg_engine* h, const RowSet<uint32_t, 5>& s, uint32_t* rows);  // rows_get's fill for the timeline
int cost_prepare(nmg_engine* h);
int cost_fill(nmg_engine* h, const RowSet<uint64_t, 4>& s, uint64_t* rows);  // rows_get's fill for the page cost cells
// What a report has before its rows: the counters downloaded, and res zeroed
// but for nb_threads, match_samples = 1 and what the call-site registry reads
// per entry, in the report's walk order (nmg_walk_order.h; meta follows it).
struct ReportInput { HostResults r; nmg_host_results res; WalkCounters w; };
int report_begin(nmg_engine* h, ReportInput& in);
// cnt[n] scanned into off[n + 1] and the total read back: the one host wait of
// a prepare before its emit; `also` enqueues what else the wait should cover.
inline hipError_t scan_nothing() { return hipSuccess; }
template <class Also = hipError_t (*)()>
int scan_total(nmg_engine* h, const uint32_t* cnt, uint64_t n, uint64_t* off, uint64_t* part, uint64_t* total,
               Also also = scan_nothing) {
  HIP_TRY(h, launch_scan_u32(h->stream, cnt, n, off, part));
  HIP_TRY(h, hipMemcpyAsync(total, off + n, 8, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, also());
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return NMG_OK;
}
void* array_ptr(nmg_engine* h, int which, size_t* bytes);
int scratch_u64(nmg_engine* h);
int sparse_nonempty(nmg_engine* h, bool* out);
int sparse_download(nmg_engine* h, std::vector<uint64_t>& kv);  // the (key, count) words, in the device's order
int sparse_import_words(nmg_engine* h, const uint64_t* kv, uint64_t n);  // nmg_sparse_import over n such words
int multi_create(nmg_engine* h, const nmg_options* opt);
void multi_destroy(nmg_engine* h);
int multi_analyze(nmg_engine* h);
int multi_finish(nmg_engine* h);
int multi_buffer_found(nmg_engine* h, std::vector<uint32_t>& nf);
#pragma GCC visibility pop

// ---- row sets: prepare(h) leaves s.n rows of the current results epoch in
// s.d_rows, or fails; it runs once per epoch, whichever call comes first
template <class RS, class Prepare>
int rows_prepare(nmg_engine* h, RS& s, Prepare&& prepare) {
  if (s.epoch == h->epoch) return NMG_OK;
  s.epoch = 0;
  const int rc = prepare(h);
  if (!rc) s.epoch = h->epoch;
  return rc;
}
template <class RS, class Prepare>
int64_t rows_count(nmg_engine* h, RS& s, Prepare&& prepare) {
  const int rc = rows_prepare(h, s, prepare);
  return rc ? rc : s.n;
}
// the prepared rows, device to host: the `fill` of every product but the page cells (cells_fill)
struct RowsCopy {
  template <class RS>
  int operator()(nmg_engine* h, const RS& s, typename RS::word* rows) const {
    if (s.n) HIP_TRY(h, hipMemcpy(rows, s.d_rows, (size_t)s.n * RS::kWords * sizeof(*rows), hipMemcpyDeviceToHost));
    return NMG_OK;
  }
};
template <class RS, class Prepare, class Fill = RowsCopy>
int rows_get(nmg_engine* h, RS& s, Prepare&& prepare, typename RS::word* rows, int64_t n, Fill fill = Fill()) {
  const int rc = rows_prepare(h, s, prepare);
  if (rc) return rc;
  if (s.n != n) return fail(h, NMG_ERR_INVALID, "row count mismatch");
  return n ? fill(h, s, rows) : NMG_OK;
}
template <class RS, class Prepare, class Fill = RowsCopy>
int rows_collect(nmg_engine* h, RS& s, Prepare&& prepare, std::vector<typename RS::word>* rows, Fill fill = Fill()) {
  const int rc = rows_prepare(h, s, prepare);
  if (rc) return rc;
  rows->resize((size_t)s.n * RS::kWords);
  return fill(h, s, rows->data());
}
