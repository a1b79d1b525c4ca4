// nmg_internal.h -- engine internals shared by the HIP engine, the host report
// writer and the replay driver.  Not part of the C-ABI.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "numamma_gpu.h"

namespace nmg {

// Layout of the flat merge arrays (see nmg_export_array), in u64 words.  This
// is the one description of it: device code, host code and the Python mirror
// (numamma_amd/results.py) take every offset and size from the names below.
//   sum64: [2 access][kGlobalSums]     global sums: total_count, total_weight,
//                                       na_miss_count, kBuckets x (count, sum_weight)
//          [2 access][2][E]             per-entry count, weight (SoA: a flush in
//                                       entry order coalesces its atomics)
//          [E][2 access][kLevelWords]   per-entry levels: na_miss_count,
//                                       kBuckets x (count, sum_weight); NMG_F_OBJECT_LEVELS only
//   min64: [2 access][kBuckets]         global bucket min_weight
//          [E]                          first-match ordinal
//          [1]                          error word
//   max64: [2 access][kBuckets]         global bucket max_weight
constexpr uint32_t kBuckets = NMG_NB_BUCKETS;
constexpr uint32_t kGlobalSums = 3 + 2 * kBuckets;  // per access
constexpr uint32_t kLevelWords = 1 + 2 * kBuckets;  // per entry and access
constexpr uint32_t kGlobalMinMax = 2 * kBuckets;    // min64's and max64's global words
constexpr uint32_t kCwBase = 2 * kGlobalSums;       // sum64: the count/weight rows start here
constexpr uint32_t kCwRows = 4;                     // [2 access][2] rows of E words
constexpr uint32_t kFirstBase = kGlobalMinMax;      // min64: the first ordinals start here
// a mem_counters' words are its sums plus a min and a max per bucket
static_assert(sizeof(nmg_count) == 4 * 8 && sizeof(nmg_mem_counters) == (kGlobalSums + 2 * kBuckets) * 8,
              "the merge arrays hold struct nmg_mem_counters word for word");
constexpr uint64_t kHistSparse = ~0ull;
constexpr uint32_t kPageSize = 4096;  // src/mem_analyzer.c:471

constexpr uint64_t gsum_index(uint32_t access, uint32_t i) { return access * kGlobalSums + i; }
constexpr uint64_t objcw_index(uint64_t e, uint32_t access, uint32_t w, uint64_t nb_entries) {
  return kCwBase + (uint64_t(access) * 2 + w) * nb_entries + e;
}
constexpr uint64_t levels_base(uint64_t nb_entries) { return kCwBase + kCwRows * nb_entries; }
constexpr uint64_t levels_index(uint64_t e, uint32_t access, uint64_t nb_entries) {
  return levels_base(nb_entries) + (e * 2 + access) * kLevelWords;
}
constexpr uint64_t gminmax_index(uint32_t access, uint32_t bucket) { return access * kBuckets + bucket; }
constexpr uint64_t first_index(uint64_t e) { return kFirstBase + e; }
constexpr uint64_t error_index(uint64_t nb_entries) { return kFirstBase + nb_entries; }
constexpr uint64_t sum64_words(uint64_t nb_entries, bool levels) {
  return levels_base(nb_entries) + (levels ? nb_entries * 2 * kLevelWords : 0);
}
constexpr uint64_t min64_words(uint64_t nb_entries) { return error_index(nb_entries) + 1; }
constexpr uint64_t max64_words() { return kGlobalMinMax; }
// both access types' struct mem_counters from the arrays' global words
inline void global_counters(const uint64_t* sum, const uint64_t* mn, const uint64_t* mx, nmg_mem_counters out[2]) {
  for (uint32_t a = 0; a < 2; a++) {
    nmg_mem_counters& c = out[a];
    const uint64_t* s = sum + gsum_index(a, 0);
    c.total_count = s[0];
    c.total_weight = s[1];
    c.na_miss_count = s[2];
    for (uint32_t k = 0; k < kBuckets; k++)
      c.b[k] = nmg_count{s[3 + 2 * k], mn[gminmax_index(a, k)], mx[gminmax_index(a, k)], s[4 + 2 * k]};
  }
}

// Page cells of the table's entries.  An entry of np pages gets a dense block
// of np cells per thread (histogram index = thread * cells + base + page)
// while the block, the budget and the 32-bit cell index allow it; otherwise
// it becomes a sparse entry, its cells hashed on demand.
constexpr uint64_t kMaxEntryCells = 1ull << 24;   // np * threads of one dense entry
constexpr uint64_t kMaxCellIndex = 0xffffffffull;  // dense cells per thread stay below it
constexpr uint32_t kMaxSparse = 1u << 22;         // sparse entries (sparse_key's index field)
enum Placement { kPlaceDense, kPlaceSparse, kPlaceOverBudget, kPlaceSparseFull };
struct CellCursor {
  uint64_t threads = 1, budget_cells = 0;  // budget: dense cells over all threads
  uint64_t cells = 0;                      // dense cells per thread handed out so far
  uint32_t nsparse = 0;                    // sparse entries so far
  // Place an entry of np pages: kPlaceDense with *base its first cell,
  // kPlaceSparse with *sidx its sparse index, or why neither (the cursor is
  // then unchanged).  must_be_dense: an entry that already has dense cells
  // (its counts move with it) never turns sparse.
  Placement place(uint64_t np, bool must_be_dense, uint64_t* base, uint32_t* sidx) {
    if (np * threads <= kMaxEntryCells && (cells + np) * threads <= budget_cells && cells + np < kMaxCellIndex) {
      *base = cells;
      cells += np;
      return kPlaceDense;
    }
    if (must_be_dense) return kPlaceOverBudget;
    if (nsparse >= kMaxSparse) return kPlaceSparseFull;
    *sidx = nsparse++;
    return kPlaceSparse;
  }
  // the dense arena is zeroed in 16 B units: a multiple of 4 cells per thread
  uint64_t padded_cells() const { return (cells + 3) & ~uint64_t(3); }
};

// Error word: min over ((seq << 40) | (byte offset << 8) | code) so the first
// failing record in analysis order wins, as the reference's abort() would.
enum ErrCode : uint32_t {
  kErrNone = 0,
  kErrZeroSize = 1,
  kErrTruncated = 2,
  kErrUnaligned = 3,
  kErrCapacity = 4,
  kErrRange = 5,
  kErrRouteOverflow = 6,  // partition-first path: more short SAMPLE records than its overflow list holds
};

struct HostResults {
  nmg_mem_counters global[2];
  uint64_t nb_samples_total = 0, nb_found_total = 0;
  std::vector<uint32_t> buf_samples, buf_found;
  std::vector<uint64_t> buf_bytes;
  std::vector<uint64_t> first;        // [E]
  std::vector<uint64_t> count_weight; // [E][2][2] (kCwRows words per entry)
  std::vector<uint64_t> levels;       // [E][2][kLevelWords] (empty unless NMG_F_OBJECT_LEVELS)
};

// ---- engine accessors used by the report writer (implemented in nmg_engine.hip)
uint32_t engine_nb_threads(nmg_engine* h);
uint32_t engine_nb_entries(nmg_engine* h);
uint32_t engine_flags(nmg_engine* h);
const std::vector<uint64_t>& engine_hist_base(nmg_engine* h);  // per entry, kHistSparse if sparse/none
const std::vector<uint64_t>& engine_npages(nmg_engine* h);     // per entry: buffer_size/4096 + 1
const std::vector<uint32_t>& engine_sparse_entries(nmg_engine* h);  // sparse idx -> entry
// entries: the per-entry arrays too; buffer_found: the per-buffer matched
// counts too (the report needs only their total, nb_found_total)
int engine_download(nmg_engine* h, HostResults& out, bool entries = true, bool buffer_found = true);
int engine_download_hist(nmg_engine* h, std::vector<uint32_t>& cells);
void engine_set_error(nmg_engine* h, const std::string& msg);

// sparse key packing: (sparse idx:22 | thread:10 | page:32)
constexpr uint64_t sparse_key(uint32_t sidx, uint32_t th, uint32_t page) {
  return (uint64_t(sidx) << 42) | (uint64_t(th) << 32) | page;
}
constexpr uint32_t sparse_key_idx(uint64_t k) { return uint32_t(k >> 42); }
constexpr uint32_t sparse_key_thread(uint64_t k) { return uint32_t((k >> 32) & 0x3ff); }
constexpr uint32_t sparse_key_page(uint64_t k) { return uint32_t(k); }

// The sparse table's cells on the host: interleaved u64 words, kv[2i] a key and
// kv[2i + 1] its value (a u32 count, or a u64 cost) -- as the device compacts
// them (SparseWords, nmg_engine_impl.h).  Plain C++: the engine and
// tests/c/nmg_sparse_words_host.cpp use what follows.
// By key; merge: each key once, the counts of equal keys summed in u32 as the table's cells are.
inline void sparse_words_sort(std::vector<uint64_t>& kv, bool merge = false) {
  std::vector<std::pair<uint64_t, uint64_t>> p(kv.size() / 2);
  for (size_t i = 0; i < p.size(); i++) p[i] = {kv[2 * i], kv[2 * i + 1]};
  std::sort(p.begin(), p.end());
  size_t m = 0;
  for (const auto& w : p) {
    if (merge && m && kv[m - 2] == w.first) {
      kv[m - 1] = uint32_t(kv[m - 1] + w.second);
      continue;
    }
    kv[m++] = w.first;
    kv[m++] = w.second;
  }
  kv.resize(m);
}

// The n words as rows (entry, thread, page, value): each sparse entry's cells
// in (thread, page) order from row soff[sparse idx] on.  sent_entry: sparse idx
// -> entry, ~0 for one that is no longer sparse.  W: u32 the page cells, u64
// the page cost cells.
template <class W>
void place_sparse_rows(const uint64_t* kv, uint64_t n, const std::vector<uint32_t>& sent_entry, const uint64_t* soff,
                       W* rows) {
  const uint64_t nsent = sent_entry.size();
  std::vector<std::vector<std::pair<uint64_t, W>>> per(nsent);
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t k = kv[2 * i];
    const W v = (W)kv[2 * i + 1];
    const uint32_t s = sparse_key_idx(k);
    if (k == ~0ull || !v || s >= nsent || sent_entry[s] == ~0u) continue;
    per[s].push_back({(uint64_t(sparse_key_thread(k)) << 32) | sparse_key_page(k), v});
  }
  for (uint64_t s = 0; s < nsent; s++) {
    auto& l = per[s];
    if (l.empty()) continue;
    std::sort(l.begin(), l.end());
    W* r = rows + soff[s] * 4;
    for (const auto& c : l) {
      r[0] = sent_entry[s];
      r[1] = (uint32_t)(c.first >> 32);
      r[2] = (uint32_t)c.first;
      r[3] = c.second;
      r += 4;
    }
  }
}

// ---- timeline sparse table (nmg_set_timeline_ex, NMG_TL_SCOPE_ALL): the
// timeline cells of the selected sparse entries, keyed by one 64-bit word
//   row:32 | thread:10 << 32 | bin:12 << 42 | ordinal:10 << 54
// ordinal: the entry's rank among the selected sparse entries, in id order,
// 0..kTlMaxSparse - 1 -- so key order is (entry, bin, thread, row) order, and
// the all-ones word (the table's empty marker) needs ordinal 1023 and is never
// a key.  Host and device (constexpr, as sparse_key); tests/timeline_all_expect.py
// mirrors it.
constexpr uint32_t kTlMaxSparse = 1023;
constexpr uint64_t tl_sparse_key(uint32_t ord, uint32_t bin, uint32_t th, uint32_t row) {
  return (uint64_t(ord) << 54) | (uint64_t(bin) << 42) | (uint64_t(th) << 32) | row;
}
constexpr uint32_t tl_sparse_key_ord(uint64_t k) { return uint32_t(k >> 54); }
constexpr uint32_t tl_sparse_key_bin(uint64_t k) { return uint32_t(k >> 42) & 0xfff; }
constexpr uint32_t tl_sparse_key_thread(uint64_t k) { return uint32_t(k >> 32) & 0x3ff; }
constexpr uint32_t tl_sparse_key_row(uint64_t k) { return uint32_t(k); }
// A full 64-bit mix for the table's start slot (the murmur3 finaliser): the
// ordinal and the bin sit in the key's high bits, which sparse_slot's
// multiplicative hash does not see.
constexpr uint64_t tl_sparse_hash(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

// The timeline's rows: the nd dense rows (entry, bin, thread, row, count), in
// entry order, merged with the table's n (key, count) words, sorted by key and
// decoded through sp_ids (ordinal -> entry), into out[(nd + n) * 5] -- one
// list in (entry, bin, thread, row) order (an entry is dense or sparse, never
// both).  out may hold the dense rows in its own tail (dense == out + n * 5):
// the write position never passes the dense read position.
inline void tl_merge_rows(const uint32_t* dense, uint64_t nd, const uint64_t* kv, uint64_t n,
                          const std::vector<uint32_t>& sp_ids, uint32_t* out) {
  uint64_t i = 0, j = 0;
  uint32_t* w = out;
  while (i < nd || j < n) {
    const uint32_t es = j < n ? sp_ids[tl_sparse_key_ord(kv[2 * j])] : ~0u;
    if (i < nd && (j == n || dense[5 * i] < es)) {
      for (int k = 0; k < 5; k++) w[k] = dense[5 * i + k];
      i++;
    } else {
      const uint64_t k = kv[2 * j];
      w[0] = es;
      w[1] = tl_sparse_key_bin(k);
      w[2] = tl_sparse_key_thread(k);
      w[3] = tl_sparse_key_row(k);
      w[4] = (uint32_t)kv[2 * j + 1];
      j++;
    }
    w += 5;
  }
}

// ---- dump modes: what the report writer needs besides the counters
struct DumpBuffer {
  const uint8_t* data;    // the linearised buffer
  uint64_t len;
  uint32_t thread_rank, access;
  const uint32_t* match;  // [byte offset / 8] = entry + 1 for SAMPLE records, 0 = unmatched
};
struct DumpInput {
  std::vector<DumpBuffer> buffers;  // analysis order
  const uint64_t* entry_addr;       // [E] buffer_addr (sample offsets)
  const uint64_t* levels;           // [E][2][kLevelWords] (callsite_summary_<id>.dat)
};

// ---- report writer (nmg_report.cpp)
// found_total: the matched-sample total when r->buf_found is not filled in
// (the engine's report: the analysis counts it, Params::found)
int write_report(const nmg_host_results* r, const nmg_object_meta* meta, const nmg_report_options* opts,
                 const char* stdout_path, std::string& err, const DumpInput* dump = nullptr,
                 const uint64_t* found_total = nullptr);
// callsite_timeline_<id>.dat files from (entry, bin, thread, row, count) rows
int write_timeline(const nmg_host_results* r, const nmg_object_meta* meta, const nmg_report_options* opts,
                   const nmg_timeline_options* tl, const uint32_t* rows, int64_t n, std::string& err);

// ---- NUMA placement (include/numamma_gpu.h): what the device path
// (nmg_placement.hip), the host path and the writer (nmg_report.cpp) share.
// The thread map as the fold reads it: thread ranks sorted by node, node n's
// at thr[node_off[n] .. node_off[n + 1]).
struct PlaceMap {
  uint32_t N = 0, D = 0;
  std::vector<uint32_t> thr, node_off;
  std::vector<uint32_t> node;  // [T] the map itself: thread rank -> node
};
// p checked (NMG_ERR_INVALID) and laid out for T threads
int placement_map(const nmg_placement_options* p, uint32_t T, PlaceMap& out);
// Groups in ascending gid order, group g's members at [m_off[g], m_off[g + 1]).
// rows[g] = min(R, the longest member): the pages past every member count
// nothing and never qualify.  Groups without a dense member or a row are left
// out.  all (NMG_PLACE_HUGE): the sparse entries are members too, and a group
// that has one is huge[g]: it gets no per-page array, on the device or on the
// host, and is walked over its members' cells instead.
constexpr uint64_t kPlaceMaxPages = 0xffffffffull;  // a page number is the sparse key's 32-bit page field
struct PlaceGroups {
  std::vector<uint32_t> gid, rows, m_off{0};
  std::vector<uint32_t> m_entry, m_np;  // member: its entry (report position), pages clipped to R
  std::vector<uint8_t> huge;            // [groups] the group has a sparse member
  std::vector<uint8_t> m_dense;         // [members]
  void add(uint32_t id, uint64_t R, const std::vector<uint32_t>& entries, const uint64_t* npages,
           const uint8_t* dense, bool all = false);
  bool any_huge() const { return std::find(huge.begin(), huge.end(), 1) != huge.end(); }
};
struct PlaceSite {  // a call site that may get blocks
  uint32_t id;
  std::string caller, ident;
  uint64_t size;
};
// every entry with dense cells (all: every entry) its own group
void placement_object_groups(uint32_t E, const uint64_t* npages, const uint8_t* dense, PlaceGroups& g,
                             bool all = false);
// the call sites of r (nmg_report's ids) that blocks.dat may list, one group each
int placement_site_groups(const nmg_host_results* r, const nmg_object_meta* meta, bool online,
                          const uint64_t* npages, const uint8_t* dense, PlaceGroups& g,
                          std::vector<PlaceSite>& sites, std::string& err, bool all = false);
// the rule on the host, from (entry, thread, page, count) cells sorted by entry: [n][5] rows appended
// (a huge group from its members' cells alone: memory follows the cells, not the group's pages)
void placement_blocks_host(const PlaceGroups& g, const PlaceMap& m, const uint32_t* cells, int64_t nb_cells,
                           uint32_t nb_entries, std::vector<uint64_t>& rows);
// blocks.dat from the sites (ascending id) and their rows (group = site id)
int write_blocks(const std::vector<PlaceSite>& sites, const uint64_t* rows, int64_t n,
                 const nmg_report_options* opts, std::string& err);

// callsite_cost_<id>.dat files from (entry, thread, page, value) rows
int write_page_cost(const nmg_host_results* r, const nmg_object_meta* meta, const nmg_report_options* opts,
                    const uint64_t* rows, int64_t n, std::string& err);

}  // namespace nmg
