// nmg_route.h -- the partition-first path for large object tables (DESIGN.md
// "Partition-first"): what nmg_route.hip and the host engine share.
//
// The reference looks every sample up in one global AVL tree
// (ma_find_mem_info_from_sample, src/mem_analyzer.c:249-306; ht_lower_key,
// tools/hash.c:63-77).  At 10^5..10^6 intervals that is one or two random
// HBM lines per sample on a GPU.  This path first routes the samples by
// address range, then attributes each range with its slice of the table in
// LDS:
//   1. route2_kernel  streams the buffers in analysis order (the byte cursor of
//                     __analyze_buffer, mem_sampling.c:815-927), counts the
//                     SAMPLEs per buffer, and appends a 16 B compact record of
//                     every SAMPLE to a chunk of its partition (partition = a run of
//                     <= kPartKeys consecutive keys; chunks of kChunk records
//                     from the workgroup's private pool);
//      overflow_kernel  the records a full pool turned away, with global lookups;
//   2. count_kernel   chunks per (workgroup, partition), from the chunks' tags,
//                     and the global counters of every routed record from its X
//                     word (update_counters, mem_sampling.c:508-592);
//      plan_kernel    per-partition chunk counts -> list offsets and work items;
//   3. scatter_kernel chunk ids into per-partition lists;
//   4. local_kernel   one work item (<= kItemChunks chunks of one partition) per
//                     workgroup at a time: the partition's keys and node records
//                     in LDS, its object and page counters in LDS, flushed once
//                     per item (__match_sample, :594-673; ma_get_block,
//                     mem_analyzer.c:494-534); with NMG_F_OBJECT_LEVELS /
//                     NMG_F_SAMPLE_MATCHES also the matched records' level
//                     buckets (data_src re-read from the raw record) and every
//                     record's match (Params::smatch);
//   5. found_kernel   per-buffer matched-sample counts from the match bits
//                     local_kernel leaves per chunk (on demand: the reference
//                     only sums them, mem_sampling.c:334-335, 357-361).
#pragma once

#include "nmg_kernels.h"
#include "nmg_pool_layout.h"
#include "nmg_table_build.h"

namespace nmg {

constexpr uint32_t kChunk = 64;            // compact records per chunk (one wave processes one chunk)
constexpr uint32_t kItemChunks = 1023;     // chunks per work item (one workgroup): fewer than 2^16 records, so
                                           // neither the packed object counters nor a u16 page cell can
                                           // overflow before the item's flush
static_assert((uint64_t)kItemChunks * kChunk < (1ull << (64 - kPackShift)), "packed count per item");
static_assert((uint64_t)kItemChunks * kChunk < 65536u, "a u16 page cell cannot wrap within one item");
constexpr uint32_t kChunkIdBits = 25;      // route pass LDS: chunk id << 7 | fill
constexpr uint32_t kFoundLds = 16384;      // found_kernel: per-buffer LDS counters of one workgroup
// internal switches (tests / A/B only)
constexpr uint32_t kDbgNoRoute = 0x10000;  // large tables: the single-pass attribute_kernel instead
constexpr uint32_t kDbgTinyPool = 0x20000; // route pass: private pools of 2 chunks, so the pool-overflow
                                           // (direct attribution) path runs
constexpr uint32_t kDbgTinyPieces = 0x200000;  // chunk pool: the smallest pieces that hold the largest workgroup pool,
                                               // not kPieceLog2: small workloads span pieces and padding (tests)
// ablation switches (tools/ablate.py; results are wrong with them)
constexpr uint32_t kDbgTinyOvf = 0x80000;  // route pass: an overflow list of 64 records, the rest attributed directly
                                           // (tests, with kDbgTinyPool)
constexpr uint32_t kDbgLapNoWait = 0x100000;   // route pass: a partition's LDS line is given up by a record one
                                                // line ahead of the staged one (tests: the given-up path)
constexpr uint32_t kDbgLocalNoWork = 0x400000;   // local pass: chunk loads only
constexpr uint32_t kDbgRouteTiming = 0x800000;   // route pass: per-wave phase cycles in Params::dbg
constexpr uint32_t kDbgLocalNoObj = 0x1000000;   // local pass: no object counters / first ordinals
constexpr uint32_t kDbgLocalNoPage = 0x2000000;  // local pass: no page cells
constexpr uint32_t kDbgLocalNoGlobal = 0x4000000;  // local pass: no global counters
constexpr uint32_t kDbgLocalNoSearch = 0x8000000;  // local pass: no lookup (nothing matches)
constexpr uint32_t kDbgNoLines = 0x20000000;      // route pass: no LDS line stage (every record stored to its
                                                  // slot; tests and A/B)
constexpr uint32_t kDbgLocalAtomics = 0x80000000u;  // local pass: every flush through atomics (A/B)
constexpr uint32_t kDbgLocalTiming = 0x10000000;  // local pass: per-wave phase cycles in Params::dbg
                                                   // (wait, global, search, match, object, page per chunk;
                                                   // dequeue, setup, flush per item; chunks, items)
constexpr int kRouteTimingWords = 16;            // route2: wait, check+loads, global, search, encode, claim, staged,
                                                 // direct, lap waits, windows, broken, line rounds, stores
                                                 // -, windows, -, -

// compact record: 16 B, two u64 words (everything the local pass needs; the
// global counters were done by the route pass)
//   lo = addr - partition start (kAddrBits) | (ts - tbase) << kAddrBits (low 24 bits)
//   hi = (ts - tbase) >> 24 (16 bits) | min(weight, wesc) << 16 (wbits)
//        | location << (16 + wbits): byte offset / 8 (obits), then buffer
//          index g (gbits) -- ordered as the analysis position, so the local
//          pass keeps first matches as locations --
//        | thread rank << (63 - tbits) | access type << 63
// A record whose address, timestamp or weight does not fit carries wesc: the
// local pass re-reads all three from the raw record (rare).
// narrowest weight field of a compact record: weights up to 2046 cycles (the
// bulk of PEBS load latencies) never escape; a buffer set whose location
// fields leave fewer bits keeps the single-pass kernel (route_layout)
constexpr uint32_t kMinWeightBits = 11;
constexpr uint32_t kTsBits = 40;
struct XLayout {
  uint32_t gbits, obits, tbits, wbits;  // wbits = min(48 - (gbits + obits + tbits + 1), 16) >= kMinWeightBits
  uint64_t wesc;   // 2^wbits - 1
  uint64_t tbase;  // smallest non-zero alloc_date of the table (earlier samples escape)
};

struct RouteParams {
  Params p;                  // data, sbufs (= descriptors in analysis order, .pad = index), ranges,
                             // global counters, per-buffer counts, and the table for direct attribution
  const uint64_t* pbounds;   // [kMaxParts + 1] partition start keys, ascending, ~0 padding
  const uint16_t* pdir;      // [kRouteDir] directory slots of every segment
  const uint32_t* pdead;     // [(kMaxParts + 1) / 32] bit q: every entry of partition q has free_date 0,
                             // so only a sample with timestamp 0 can match one (alloc <= ts <= free,
                             // is_sample_in_buffer, mem_analyzer.c:148-149): the [stack] range after
                             // warn_non_freed_buffers (Q4), an online table's live objects (Q3)
  RSeg seg[kRouteSegs];      // segments of the partition starts, ascending
  uint32_t nseg;
  uint32_t nparts;
  XLayout xl;
  uint64_t seq0;             // analysis index of descriptor 0 (seq = seq0 + index)
  uint4* const* pieces;      // chunk pool: compact records of chunk id at pieces[id >> pk][(id & (2^pk - 1)) * kChunk ...]
  uint32_t pk;               // (nmg_pool_layout.h; a workgroup's range [chunk0[w], chunk0[w + 1]) lies in one piece)
  uint32_t* cmeta;           // [chunks] partition | fill << 24
  const uint32_t* chunk0;    // [grid + 1] private chunk range of each workgroup
  uint32_t* used;            // [grid] chunks taken
  uint4* ovf16;              // overflow list: records that found no chunk (overflow_kernel)
  unsigned long long* ovfx;  // and their partition's start
  uint32_t* ovf_cnt;         // (= ctl[2]; zeroed by plan_kernel after overflow_kernel read it)
  uint32_t ovf_cap;
};

struct PlanParams {
  uint32_t* pcnt;        // in: [grid][nparts] chunk counts; out: exclusive prefix over workgroups
  uint32_t* pbase;       // out: [nparts] first list slot of each partition (plan_cols_kernel: the totals)
  uint4* items;          // out: {partition, list begin, list end, 0}
  uint32_t* ctl;         // out: [0] number of items, [1] dequeue head (zeroed), [2] overflow records (zeroed), [3] their number for local_kernel
  uint32_t grid, nparts;
};

struct ScatterParams {
  const uint32_t* cmeta;
  const uint32_t* chunk0;
  const uint32_t* used;
  const uint32_t* pcnt;   // exclusive prefixes (plan_kernel)
  const uint32_t* pbase;
  uint2* clist;           // [chunks] grouped by partition: x = chunk id | fill << kChunkIdBits, y = coff: the
                          // chunk lies at pool0 + coff * kChunk records (one 8 B store per chunk)
  uint4* const* pieces;   // chunk pool (RouteParams::pieces, ::pk)
  uint64_t pool0;         // the lowest piece's address: every chunk lies less than 2^32 chunks above it
  uint32_t pk;
  uint32_t nparts;
};

struct LocalParams {
  Params p;                  // table (nodes, chain, entries), counters, hist, sparse, flags
  const PartInfo* parts;
  const uint64_t* pe_keys;   // [nparts][kPartSlots] keys, ascending
  const uint4* pe_nodes;     // [nparts][kPartSlots][2] (addr, end), (alloc, free) of each key's newest entry (exact)
  const uint4* pe_pnode;     // [nparts][kPartSlots] the same, packed (PackedNode)
  const uint4* pe_old;       // [nparts][kOldLds] older entries, packed (kOldLds)
  const uint32_t* pe_oinf;   // [nparts][kOldLds] their page cells
  const uint2* pe_info;      // [nparts][kPartSlots] (cell - cb, or packed cell, or ~0 sparse; buffer_addr - first key)
  const uint4* pe_dir;       // [nparts][kPartDir] directory slots (PartDir)
  const uint32_t* pe_ids;    // [table entries] entry id of each table position (an online table,
                             // nmg_update_objects), or null: the id is the position (nmg_set_objects)
  const uint32_t* pe_lrel;   // [table entries] an entry's first packed cell (PartInfo::cmap != ~0)
  const uint32_t* pe_cmap;   // packed cell -> histogram cell
  const uint4* pool0;        // chunk pool: the lowest piece (ScatterParams::pool0)
  const uint32_t* cmeta;
  const uint2* clist;        // (chunk id | fill << kChunkIdBits, the chunk's place above pool0 in chunks), grouped
                             // by partition
  const uint4* items;
  uint32_t* ctl;             // [0] items, [1] dequeue head, [3] records of the overflow path (plan_kernel)
  unsigned long long* cmatch;  // [chunks] match bit per record
  const BufDesc* descs;      // analysis order (escaped weights are re-read from the record)
  XLayout xl;
  uint64_t seq0;
  uint32_t fresh;            // the counters are as the last reset left them (no analysis since): an
                             // item alone on its partition stores its counters without reading them,
                             // unless the overflow path or a large weight wrote to them
};

struct FoundParams {
  const uint32_t* ranges;    // [grid + 1] descriptor range of each route workgroup
  const uint32_t* chunk0;
  const uint32_t* used;
  const uint32_t* cmeta;
  const unsigned long long* cmatch;
  uint4* const* pieces;      // chunk pool (RouteParams::pieces)
  uint32_t pk;
  uint32_t* bufcnt;          // [2][nb_bufs]
  uint32_t nb_bufs, gbits, gshift;
};

hipError_t launch_route(uint32_t grid, hipStream_t s, const RouteParams& r);
hipError_t launch_overflow(hipStream_t s, const RouteParams& r);
// count_kernel: per route workgroup, chunks per partition (pcnt, from the
// chunks' tags)
struct CountParams {
  ScatterParams sc;
};
hipError_t launch_count(uint32_t grid, hipStream_t s, const CountParams& r);
hipError_t launch_plan(hipStream_t s, const PlanParams& r);
hipError_t launch_scatter(uint32_t grid, hipStream_t s, const ScatterParams& r);
hipError_t launch_local(uint32_t grid, hipStream_t s, const LocalParams& r);
hipError_t launch_found(uint32_t grid, hipStream_t s, const FoundParams& r);

}  // namespace nmg
