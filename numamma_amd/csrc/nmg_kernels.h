// nmg_kernels.h -- what the device code (nmg_kernels.hip) and the host engine
// (nmg_engine.hip) share: layout constants, the kernels' parameter blocks and
// the launchers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "nmg_internal.h"
#include "nmg_table_build.h"

namespace nmg {

constexpr int kWG = 1024;                      // one workgroup per CU
constexpr uint32_t kSampleType = 9;            // PERF_RECORD_SAMPLE
constexpr uint32_t kRecBytes = 40;             // perf_event_header (8) + struct mem_sample (32)
constexpr uint32_t kWinBytes = kWG * kRecBytes;  // one 40 B stride slot per lane per window
// One LDS region holds the lookup structure of either mode:
//   <= kLdsNodes keys: Eytzinger keys (8 KiB) | node records (32 KiB) | node info (8 KiB)
//   larger tables:     Eytzinger fences (32 KiB) | per-bucket directory shift (4 KiB)
constexpr uint32_t kTabBytes = 48 * 1024;
static_assert((kLdsNodes + 1) * (8 + 32 + 8) <= kTabBytes, "small-table LDS layout");
static_assert((kMaxFences + 1) * (8 + 1) <= kTabBytes, "fence LDS layout");
constexpr uint32_t kMaxList = kWG;             // slow path: SAMPLE offsets listed per step
// per-stream LDS aggregation tables (flushed to global at a stream change and
// on a window cadence)
constexpr uint32_t kObjSlots = 2048;           // entry -> (count, weight, first ordinal)
// long-tail log (hashed object mode): per workgroup, kLogParts sub-logs by
// entry range of 24 B records {entry | access << 31, count, weight, ordinal}
constexpr uint32_t kLogParts = 256;
// Long-tail log slots (16 B, one store): a sample (count 1, weight < 2^32)
// is {entry | access << 31, weight, offset, seq}; anything else takes two
// slots, {entry | access << 31, count, kTlogHead, ord >> 32} then
// {weight lo, weight hi, kTlogCont, ord & ~0u}.  Offsets are 8-aligned, so
// the two marks never occur as a sample's offset.
constexpr uint32_t kTlogHead = 0xFFFFFFFFu, kTlogCont = 0xFFFFFFFEu;
constexpr uint32_t kLogChunk = 4096;   // entries per LDS pass of tlog_reduce_kernel
constexpr uint32_t kLogMaxGrid = 1024;  // attribution workgroups a log can serve
constexpr uint32_t kPageBuckets = 896;         // dense page cell -> count: 8-slot buckets
constexpr uint32_t kPageSlots = kPageBuckets * 8;  // 7168 cells (56 KiB)
constexpr uint32_t kObjBuckets = kObjSlots / 8;
// hashed (non-dense) tables are flushed at least every kTableWindows windows:
// u32 counts stay far from overflow and the first-come slots are re-learnt
constexpr uint32_t kTableWindows = 128;  // (256: configs[2] +4 %, 64: c4 +3 %; 128 neutral at c4)
// Dense modes (template flags of attribute_kernel):
//   kModeDenseObj:  nb_entries <= kObjSlots: slot = entry id, no key check;
//   kModeDensePage: dense histogram cells per thread <= kDensePageCells: u16
//                   counts, two per LDS word, flushed at least every
//                   kDensePageWindows windows (<= 1024 samples per cell each,
//                   so a u16 cannot overflow into its neighbour)
constexpr int kModeDenseObj = 1, kModeDensePage = 2;
constexpr int kModeLarge = 4;  // more than kLdsNodes keys: LDS fences + directory + node records in global memory
constexpr uint32_t kDensePageCells = kPageSlots * 4;  // the page table's 56 KiB as u16 cells
constexpr uint32_t kDensePageWindows = 62;
constexpr bool kPackObj = true;
constexpr uint32_t kPackShift = 44;  // kModeDenseObj: per-entry count << 44 | weight sum
static_assert((uint64_t)kDensePageWindows * kWG < (1ull << (64 - kPackShift)), "packed count");
static_assert(kDensePageWindows * kWG < 65536u, "u16 page counts");
constexpr uint64_t kEmpty64 = ~0ull;
// internal ablation switches (tools/ablate.py only; not part of the C-ABI)
constexpr uint32_t kDbgLoadOnly = 0x100;   // stage + validate windows, decode nothing
constexpr uint32_t kDbgNoGlobal = 0x200;   // skip the global mem_counters update
constexpr uint32_t kDbgNoFlush = 0x400;    // LDS tables filled but never written to global
constexpr uint32_t kDbgNoTables = 0x800;   // lookup only: no per-object / per-page accumulation
constexpr uint32_t kDbgTiming = 0x1000;    // per-wave phase cycle counts (tools/phase_timing.py)
constexpr uint32_t kDbgTinyLog = 0x2000;   // long-tail sub-logs of 2 records: exercises the overflow path (tests)
constexpr uint32_t kDbgNoPack = 0x4000;    // overflow through plain atomics, not packed ones (tests)
constexpr uint32_t kDbgNoDir = 0x8000;     // large tables: no fence-bucket directory, binary search only (tests)
constexpr uint32_t kDbgMultiRccl = 0x40000;  // nmg_create: a multi-GPU handle even for nb_gpus <= 1, merged through
                                             // RCCL (a one-rank communicator on a one-GPU box: tests of that branch)
constexpr int kTimingWords = 24;           // per wave: load+check, barrier, process, rest, total, windows, -, -,
                                           // then (wave 0) 8 x 2 words of window trace


// PERF_MEM_LVL_* (/usr/include/linux/perf_event.h:1250-1263)
constexpr uint32_t LVL_NA = 0x01, LVL_HIT = 0x02, LVL_MISS = 0x04;

struct BufDesc {
  uint64_t offset;  // byte offset in the data arena (16-aligned)
  uint32_t len;     // linearised length (< 4 GiB, mem_sampling.c:831-834)
  uint32_t thread_rank;
  uint32_t access;
  uint32_t pad;  // (schedule copy) index of the buffer in submission order
  uint64_t seq;  // analysis-order index (global across shards)
};
static_assert(sizeof(BufDesc) == 32, "BufDesc");

struct Params {
  const uint8_t* data;
  const BufDesc* sbufs;    // descriptors in schedule order (sorted by stream; .pad = buffer index)
  const uint32_t* ranges;  // [gridDim.x + 1]: workgroup w takes sbufs[ranges[w] .. ranges[w+1])
  uint32_t nb_bufs;
  uint32_t nb_keys;
  const uint64_t* keys;      // [nb_keys] sorted unique keys
  const DevEntry* nodes;     // [nb_keys] node records
  const DevEntry* entries;   // [nb_entries] by entry id (hist, sidx)
  const DevEntry* chain;     // entries in table order (node i's: [first, first + count)); the table
                             // of the last nmg_set_objects / nmg_update_objects
  // large tables (nb_keys > kLdsNodes): fence b = keys[b * fence_step]
  const uint64_t* ffences;   // [2^kFenceLevels] fences in Eytzinger order, [0] unused, ~0 padding
  const uint8_t* fshift;     // [nb_fences] slot width log2 of bucket b's directory, or kShiftSearch
  const uint2* dir;          // [nb_fences << dir_log2] {lo | cnt << 16, offset of the slot's first key}
  uint32_t nb_fences;
  uint32_t fence_log2;       // fence_step = 2^fence_log2 keys per bucket
  uint32_t dir_log2;         // directory slots per bucket = 2^dir_log2 (0: fence_step == 1, no directory)
  uint32_t nb_threads;
  uint32_t flags;
  uint32_t nb_entries;
  uint32_t lds_nodes;    // nb_keys <= kLdsNodes: keys + node records in LDS, Eytzinger order
                         // (arrays of kLdsNodes + 1 = 2^10 slots, index 0 unused)
  uint32_t elevels;      // levels of the Eytzinger tree (2^elevels - 1 >= nb_keys)
  const uint64_t* efences;   // [2^elevels] keys in Eytzinger (BFS) order, [0] unused, ~0 padding
  const DevEntry* enodes;    // [2^elevels] node records in the same order
  uint32_t sparse_mask;  // capacity - 1 (power of two)
  uint64_t hist_cells;   // dense cells per thread: histogram index = thread * hist_cells + cell
  uint64_t* sum64;
  uint64_t* min64;
  uint64_t* max64;
  uint32_t* hist;
  uint32_t* bufcnt;  // [2][nb_bufs]: samples, found
  // matched SAMPLEs of every analysis since the last reset (the report's
  // nb_found_samples_total, mem_sampling.c:335, 357-360): added by each kernel
  // that attributes, so that an analysis leaves it final
  unsigned long long* found;
  uint64_t* sparse_keys;
  uint32_t* sparse_vals;
  uint32_t* sparse_dirty;  // set on any sparse insert: the next reset must clear the table
  uint32_t* smatch;        // NMG_F_SAMPLE_MATCHES: [(buffer offset + record offset) / 8] = entry + 1, 0 = none
  unsigned long long* dbg;  // kDbgTiming: [grid][waves][kTimingWords]
  // hashed object mode: per-launch packed [2 access][E] (count << pk_shift |
  // weight) for the global path, one atomic instead of two; exact because
  // samples per launch < 2^(64 - pk_shift) and only weights < pk_wlim are
  // packed (their sum < 2^pk_shift); unpack_kernel adds it into sum64
  unsigned long long* pk64;  // null: packing off
  uint32_t pk_shift;
  uint64_t pk_wlim;
  // long-tail log: instead of scattered global atomics, table-full samples
  // and flushed slots append to sub-log (workgroup, entry >> tlog_rshift);
  // tlog_reduce_kernel sums each entry range from LDS.  A full sub-log falls
  // back to the atomics.
  uint4* tlog;               // [grid][tlog_parts][tlog_cap] 16 B slots (kTlogHead layouts); null: off
  uint32_t* tlog_cnt;        // [grid][tlog_parts] records written
  uint32_t tlog_cap, tlog_rshift, tlog_parts;
  // access timeline (nmg_set_timeline): u32 cells [bin][thread][row] per
  // selected entry from the base in its DevEntry::pad1 (tl_pad); null: off
  uint32_t* tl;
  uint64_t tl_t0;
  uint32_t tl_bin_shift, tl_nb_bins, tl_row_shift;
  uint32_t tl_rounds;  // timeline_add's merge rounds (kTlRounds)
  // the timeline sparse table (nmg_set_timeline_ex, NMG_TL_SCOPE_ALL): the
  // cells of the selected sparse entries, tl_sparse_key -> u32 count, open
  // addressing over tls_mask + 1 slots (timeline_sparse_add); null unless a
  // sparse entry is selected.  Such an entry's pad1 is tl_pad_sparse(ordinal).
  uint64_t* tls_keys;
  uint32_t* tls_vals;
  uint32_t tls_mask;
  // page cost cells (nmg_set_page_cost): u64 cells at the page histogram's
  // index, thread * hist_cells + cell; null: off.  The rule is in
  // include/numamma_gpu.h (cost_selected / cost_add in nmg_device.h).
  uint64_t* cost;
  uint32_t cost_bucket_mask, cost_access_mask, cost_metric;
  uint32_t cost_rounds;  // cost_add's merge rounds (kCostRounds)
  // the sparse entries' cost cells (NMG_COST_SCOPE_ALL): one u64 per slot of
  // the sparse page table, the cost of key k at the slot the count table gave
  // k (sparse_slot); null unless that scope is set and the table exists.  Not
  // tied to `cost`: a table without a dense cell has this array only.
  uint64_t* sparse_cost;
};

// merge rounds of cost_add (nmg_device.h) before the remaining lanes add
// their own cell: Params::cost_rounds, kCostRounds unless the environment
// variable NMG_COST_ROUNDS (0..64) says otherwise when the cells are set.
// Measured at the configs[3] shard (tools/cost_timing.py), a
// step of 2.60 ms without the cells: (NMG_COST_MEMORY, both, weight) 6.02 /
// 5.78 / 5.51 / 5.53 ms at 0 / 1 / 4 / 64 rounds -- the fastest is the
// default; 64 is within its spread.  A mask that selects nearly every record
// (all buckets | N/A, count) puts the L1 hits of the hot objects on few
// cells and keeps gaining: 37.5 / 33.5 / 21.0 / 9.7 ms; such a caller sets
// NMG_COST_ROUNDS=64.
constexpr uint32_t kCostRounds = 4;

// DevEntry::pad1 of the by-id entries (Params::entries): the entry's first
// timeline cell and its rows R, or kTlNone (no timeline, or the entry is not
// selected).  Cell of (bin, thread, page) = base + (bin * nb_threads + thread) * R
// + (page >> row_shift), below 2^32.
constexpr uint64_t kTlNone = ~0ull;
constexpr uint64_t tl_pad(uint32_t base, uint32_t rows) { return (uint64_t(rows) << 32) | base; }
// ... or, for a selected sparse entry (NMG_TL_SCOPE_ALL), a tagged word with
// its ordinal in the timeline sparse table's keys: bit 63 set, which no dense
// pad has (its rows field R <= 2^24), and not kTlNone (the low word is the
// ordinal, at most kTlMaxSparse - 1).
constexpr uint64_t tl_pad_sparse(uint32_t ord) { return (1ull << 63) | ord; }
constexpr bool tl_pad_is_sparse(uint64_t pad) { return pad != kTlNone && (pad >> 63) != 0; }

// merge rounds of timeline_add (nmg_device.h) before the remaining lanes add
// their own cell: Params::tl_rounds, kTlRounds unless the environment variable
// NMG_TL_ROUNDS (0..64) says otherwise when the timeline is set.  0 is an
// atomic per record, the fastest at the configs[3] shard with 64 bins and
// page rows (3.84 ms a step against 3.90 / 3.91 / 3.96 / 4.19 for 1 / 2 / 4 /
// 16 rounds: the cells of a hot object spread over bins and rows).  Merging
// pays only where the options put a hot object's records on one cell (one
// bin, one row: 17.0 ms at 0 rounds, 14.1 ms at 4); DESIGN 7.0r8.
constexpr uint32_t kTlRounds = 0;

// tlog_reduce_kernel (long-tail log, see Params::tlog)
struct TlogParams {
  const uint4* tlog;
  const uint32_t* tlog_cnt;
  uint64_t* sum64;
  uint64_t* min64;
  unsigned long long* pk64;  // may be null
  uint32_t grid, parts, cap, rshift, nb_entries, pk_shift;
};

// reset_kernel: INIT_COUNTER semantics for every counter array
struct ResetParams {
  uint64_t* sum64;
  uint64_t n_sum64;
  uint64_t* min64;
  uint64_t n_min64;
  uint64_t* max64;
  uint64_t n_max64;
  uint4* hist;  // zeroed in 16 B units
  uint64_t n_hist16;
  uint64_t* sparse_keys;
  uint32_t* sparse_vals;
  uint64_t sparse_cap;
  const uint32_t* sparse_read;  // dirty flag of the analyses since the previous reset
  uint32_t* sparse_clear;       // the flag the analyses after this reset will set
  uint32_t* bufcnt;
  uint64_t n_bufcnt;
  unsigned long long* found;  // zeroed
  uint64_t* sparse_cost;      // cleared with the sparse table (a reused slot keeps no old cost); may be null
};

// Launchers (nmg_kernels.hip).  `mode` = kModeDenseObj | kModeDensePage.
hipError_t launch_attribute(bool timing, int mode, uint32_t grid, hipStream_t s, const Params& p);
int attribute_blocks_per_cu();  // resident attribute_kernel workgroups per CU (>= 1)
hipError_t launch_tlog_reduce(uint32_t grid, hipStream_t s, const TlogParams& r);
hipError_t launch_unpack(uint32_t grid, hipStream_t s, uint64_t* sum64, unsigned long long* pk64,
                         uint32_t nb_entries, uint32_t shift);
hipError_t launch_reset(uint32_t grid, hipStream_t s, const ResetParams& r);
hipError_t launch_merge(hipStream_t s, void* dst, const void* src, uint64_t n, int op);
// packed page histogram (nmg_hist_pack / nmg_hist_unpack); ncells a multiple of 4
// sparse_download: the used slots of the sparse table as (key, count) u64 pairs, *cnt of them
hipError_t launch_sparse_compact(hipStream_t s, const uint64_t* keys, const uint32_t* vals, uint64_t cap,
                                 uint64_t* out, unsigned long long* cnt);
// the same over the sparse cost cells: (key, cost) pairs of the slots with a non-zero cost
hipError_t launch_sparse_compact(hipStream_t s, const uint64_t* keys, const uint64_t* cost, uint64_t cap,
                                 uint64_t* out, unsigned long long* cnt);
hipError_t launch_sparse_insert(hipStream_t s, uint64_t* keys, uint32_t* vals, uint64_t cap, const uint64_t* pairs,
                                uint64_t n);
// the same into the timeline sparse table (tl_sparse_hash)
hipError_t launch_tl_sparse_insert(hipStream_t s, uint64_t* keys, uint32_t* vals, uint64_t cap, const uint64_t* pairs,
                                   uint64_t n);
// the sparse cost cells' import: cost[slot of key] = value per pair, the keys absent from the page table into *bad
hipError_t launch_sparse_cost_store(hipStream_t s, const uint64_t* keys, uint64_t* cost, uint64_t cap,
                                    const uint64_t* pairs, uint64_t n, unsigned long long* bad);
// packed cells (nmg_cells_pack / nmg_cells_unpack_add): the non-zero cells of the timeline (u32) or the page cost
// (u64) array as 16 B (cell index, value) pairs in cell order, *cnt of them, at most cap written
hipError_t launch_cells_pack(hipStream_t s, const uint32_t* cells, uint64_t ncells, void* list, uint64_t cap,
                             unsigned long long* cnt, uint32_t* wgcnt);  // wgcnt: [1024] workspace
hipError_t launch_cells_pack(hipStream_t s, const uint64_t* cells, uint64_t ncells, void* list, uint64_t cap,
                             unsigned long long* cnt, uint32_t* wgcnt);
hipError_t launch_cells_add(hipStream_t s, uint32_t* cells, uint64_t ncells, const void* list, uint64_t n,
                            unsigned long long* bad);
hipError_t launch_cells_add(hipStream_t s, uint64_t* cells, uint64_t ncells, const void* list, uint64_t n,
                            unsigned long long* bad);
hipError_t launch_hist_pack(hipStream_t s, const uint32_t* hist, uint64_t ncells, uint32_t thr, void* u8, void* ovf,
                            uint64_t cap, unsigned long long* cnt, uint32_t* wgcnt);  // wgcnt: [1024] workspace
hipError_t launch_hist_unpack(hipStream_t s, uint32_t* hist, uint64_t ncells, const void* u8, const void* ovf,
                              uint64_t n, unsigned long long* bad);
// packed per-object counters (nmg_objcw_pack / nmg_objcw_unpack): n row words
hipError_t launch_objcw_pack(hipStream_t s, const uint64_t* rows, uint64_t n, uint64_t thr, void* u32, void* ovf,
                             uint64_t cap, unsigned long long* cnt);
hipError_t launch_objcw_unpack(hipStream_t s, uint64_t* rows, uint64_t n, const void* u32, const void* ovf,
                               uint64_t m, unsigned long long* bad);
// per-object counts and weights, SoA rows -> [E][access][w] (aos: E * 32 B)
hipError_t launch_objcw_aos(hipStream_t s, const uint64_t* soa, uint64_t E, void* aos);
// page-cell rows on the device (nmg_get_page_cells / nmg_report): per dense
// entry the number of non-zero cells, then the (entry, thread, page, count)
// rows at each entry's offset, in (thread, page) order
hipError_t launch_cells_sparse_count(hipStream_t s, const uint64_t* ck, const unsigned long long* n_ptr, uint64_t cap,
                                     const uint32_t* sent, uint32_t nsent, const uint64_t* base, uint32_t* cnt);
uint32_t scan_parts(uint64_t n);  // partial sums launch_scan_u32 needs (+ 1)
hipError_t launch_scan_u32(hipStream_t s, const uint32_t* in, uint64_t n, uint64_t* out /* [n + 1] */, uint64_t* part);
hipError_t launch_gather_off(hipStream_t s, const uint64_t* off, const uint32_t* sent, uint32_t nsent, uint64_t* out);
hipError_t launch_copy_rows(hipStream_t s, const void* src, const uint64_t* n_ptr, uint64_t cap, void* dst);
hipError_t launch_cells_count(hipStream_t s, const uint32_t* hist, uint64_t hist_cells, uint32_t T,
                              const uint64_t* base, const uint32_t* np, uint32_t E, uint32_t* cnt);
hipError_t launch_cells_emit(hipStream_t s, const uint32_t* hist, uint64_t hist_cells, uint32_t T,
                             const uint64_t* base, const uint32_t* np, uint32_t E, const uint64_t* off, uint4* rows);
// the same over the page cost cells (u64, at the histogram's index): rows of four u64
hipError_t launch_cells_count(hipStream_t s, const uint64_t* cost, uint64_t hist_cells, uint32_t T,
                              const uint64_t* base, const uint32_t* np, uint32_t E, uint32_t* cnt);
hipError_t launch_cells_emit(hipStream_t s, const uint64_t* cost, uint64_t hist_cells, uint32_t T,
                             const uint64_t* base, const uint32_t* np, uint32_t E, const uint64_t* off, uint64_t* rows);
// timeline rows on the device (nmg_get_timeline_cells): the cell array in
// segments of kTlSeg cells, per segment the number of non-zero cells, then
// (after a scan) the (entry, bin, thread, row, count) rows at each segment's
// offset.  The selected entries' cells lie in entry order, each entry's in
// (bin, thread, row) order, so cell order is row order.  ids / base / nrows:
// the n selected entries, base[n] = ncells.
constexpr uint32_t kTlSeg = 2048;
hipError_t launch_tl_count(hipStream_t s, const uint32_t* tl, uint64_t ncells, uint32_t* cnt);
hipError_t launch_tl_emit(hipStream_t s, const uint32_t* tl, uint64_t ncells, const uint32_t* ids,
                          const uint32_t* base, const uint32_t* nrows, uint32_t n, uint32_t T, const uint64_t* off,
                          uint32_t* rows);

// NUMA placement blocks on the device (nmg_placement.hip; the rule is in
// include/numamma_gpu.h).  The groups' pages are numbered consecutively:
// group g's page p is group page pg_off[g] + p, pg_off[G] of them in all.
struct PlaceParams {
  const uint32_t* hist;  // the page histogram: cell (t, c) at t * hist_cells + c
  const uint64_t* cost;  // NMG_PLACE_PAGE_COST: the page cost cells at the same index, folded instead (else null)
  uint64_t hist_cells;
  const uint32_t* thr;       // [T] thread ranks sorted by node
  const uint32_t* node_off;  // [N + 1] node n's ranks at thr[node_off[n] .. node_off[n + 1])
  uint32_t N, D, G;
  const uint32_t* gid;      // [G] ascending
  const uint64_t* pg_off;   // [G + 1] ascending; a group without pages here is a huge one (below)
  const uint32_t* m_off;    // [G + 1] group g's members [m_off[g], m_off[g + 1])
  const uint64_t* m_base;   // [M] member's first cell
  const uint32_t* m_np;     // [M] member's pages (<= the group's rows)
  uint64_t* pv_cnt;         // [pages] cnt(p)
  uint8_t* pv_node;         // [pages] dom(p) of a qualifying page, kPlaceNoNode otherwise
  uint32_t* bcnt;           // [G] blocks per group
  const uint64_t* boff;     // [G + 1] their exclusive scan
  uint64_t* rows;           // [blocks][5], zeroed before the emit pass
};
constexpr uint32_t kPlaceNoNode = 0xff;
hipError_t launch_place_fold(hipStream_t s, const PlaceParams& p, uint64_t pages);
hipError_t launch_place_count(hipStream_t s, const PlaceParams& p);
hipError_t launch_place_emit(hipStream_t s, const PlaceParams& p);

// NMG_PLACE_HUGE: the groups that have a sparse member ("huge": rank 0..H-1 in
// group order) are computed from their touched pages alone.  Extract appends
// one (key, count) item per non-zero cell of their members, key = rank << 38 |
// page << 6 | node; the items are sorted by key; reduce gives every (rank,
// page) head item the page's cnt and dom; the qualifying pages are compacted
// into a list in (rank, page) order; a list item whose rank or node differs
// from the item before it starts a block.  The blocks per group go into
// PlaceParams::bcnt beside the dense groups', so that one scan places both
// kinds' rows in one array.
constexpr uint32_t kPlaceRankShift = 38, kPlaceNodeBits = 6;
struct PlaceHugeParams {
  // the sparse table and the sparse entries of the current table
  const uint64_t* sparse_keys;
  const uint32_t* sparse_vals;
  uint64_t sparse_cap;
  uint32_t nsent;           // sparse indices
  const uint32_t* s_rank;   // [nsent] the huge group of the entry, ~0: none (not a member, or no longer sparse)
  const uint32_t* s_lim;    // [nsent] the member's pages
  // the dense members of huge groups: member d's cells [dm_off[d], dm_off[d + 1]) of dcells per thread
  const uint32_t* hist;
  uint64_t hist_cells;
  uint32_t DM;
  uint64_t dcells;
  const uint64_t* dm_off;   // [DM + 1]
  const uint64_t* dm_base;  // [DM] first histogram cell
  const uint32_t* dm_rank;  // [DM]
  const uint32_t* tnode;    // [T] thread rank -> node
  uint32_t T, D, H;
  const uint32_t* h_group;  // [H] rank -> group index (PlaceParams' arrays)
  const uint32_t* gid;      // [G]
  // items: cap of them at most, *n_items appended
  unsigned long long* n_items;
  uint64_t cap;
  uint64_t* keys;           // extract's output; after the sort the list's (rank << 32 | page)
  uint64_t* vals;           // ... and the list's cnt
  const uint64_t* skeys;    // [n] sorted
  const uint64_t* svals;
  uint64_t* pcnt;           // [n] head items: cnt(p)
  uint32_t* pnode;          // [n] head items: dom(p)
  uint32_t* flag;           // [n] 1: a head item whose page qualifies; later [m] 1: the list item starts a block
  const uint64_t* off;      // [n + 1] / [m + 1] exclusive scan of flag
  uint32_t* lnode;          // [m] the list's nodes
  uint64_t* gfirst;         // [H] the first block (over all huge groups) of the group
  uint32_t* bcnt;           // PlaceParams::bcnt
  const uint64_t* boff;     // PlaceParams::boff
  uint64_t* rows;           // PlaceParams::rows
  // NMG_PLACE_PAGE_COST on an engine with NMG_COST_SCOPE_ALL: the cost cells folded instead
  // (sparse_cost parallel to sparse_vals, cost at the histogram's index; `cost` null: no dense cell)
  const uint64_t* sparse_cost;
  const uint64_t* cost;
};
// from_cost: the items' values are the cost cells (the u64 instances)
hipError_t launch_place_huge_extract(hipStream_t s, const PlaceHugeParams& p, bool sparse, bool from_cost = false);
// the n items of keys / vals sorted by key into skeys / svals (tmp: tmp_bytes of workspace)
size_t place_huge_sort_bytes(uint64_t n);
hipError_t launch_place_huge_sort(hipStream_t s, const PlaceHugeParams& p, uint64_t n, void* tmp, size_t tmp_bytes);
hipError_t launch_place_huge_reduce(hipStream_t s, const PlaceHugeParams& p, uint64_t n);
hipError_t launch_place_huge_compact(hipStream_t s, const PlaceHugeParams& p, uint64_t n);
hipError_t launch_place_huge_starts(hipStream_t s, const PlaceHugeParams& p, uint64_t m);
hipError_t launch_place_huge_count(hipStream_t s, const PlaceHugeParams& p, uint64_t m);
hipError_t launch_place_huge_emit(hipStream_t s, const PlaceHugeParams& p, uint64_t m);

}  // namespace nmg
