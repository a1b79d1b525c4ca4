// nmg_report_dump_host.cpp -- the file products of nmg_report.cpp pinned byte
// for byte, stand-alone: built with nmg_report.cpp by
// tests/test_report_dump_host.py (under the address and undefined-behaviour
// sanitizers where the compiler has them, leak detection on) and run as a child
// process in an empty directory.
//
//  1. write_report with every dump mode over a crafted DumpInput (which only
//     the engine builds otherwise): the lazily opened callsite_dump_<id>.dat,
//     the __remove_site walk's callsite_summary_<id>.dat (quirk Q10: the site
//     the walk stops at, not the one removed), all_memory_accesses.dat,
//     all_memory_objects.dat, unmatched_samples.log with and without the
//     repeated last maps line, callsite_counters_<id>.dat; then without the
//     per-site files, online, and to stdout.
//  2. write_timeline, write_page_cost, write_blocks.
//  3. every error return: the code, the text, the files left behind, and no
//     descriptor left open.
//
// T = 2.  Entries: 0, 1, 2 heap objects of three call sites, 3 [stack], 4 never
// matched.  Sites in first-match order: 1 = entry 1, 2 = entry 0, 3 = [stack],
// 4 = entry 2; read weights 50, 300, 10, 100, so the report order is 2, 4, 1, 3
// and the walk removes 3, 1, 4, 2: it stops at 4, then at 2, and site 1, though
// it has a dump file, gets no summary.
#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "nmg_internal.h"

using namespace nmg;

#define CHECK(c)                                            \
  do {                                                      \
    if (!(c)) {                                             \
      printf("%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      exit(1);                                              \
    }                                                       \
  } while (0)

typedef std::vector<std::pair<std::string, std::string>> Files;  // (name, bytes), sorted by name

static std::vector<std::string> names_in(const std::string& dir) {
  std::vector<std::string> v;
  DIR* d = opendir(dir.c_str());
  CHECK(d);
  while (dirent* e = readdir(d))
    if (strcmp(e->d_name, ".") && strcmp(e->d_name, "..")) v.push_back(e->d_name);
  closedir(d);
  std::sort(v.begin(), v.end());
  return v;
}
static size_t open_fds() { return names_in("/proc/self/fd").size(); }
static bool exists(const std::string& p) {
  struct stat st;
  return stat(p.c_str(), &st) == 0;
}
static std::string slurp(const std::string& path) {
  FILE* f = fopen(path.c_str(), "rb");
  CHECK(f);
  std::string s;
  char buf[4096];
  for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) s.append(buf, n);
  fclose(f);
  return s;
}
// the directory holds exactly these files with exactly these bytes ("/": a directory, put there by the test)
static void expect_dir(const char* what, const std::string& dir, const Files& want) {
  const std::vector<std::string> got = names_in(dir);
  bool same = got.size() == want.size();
  for (size_t i = 0; same && i < got.size(); i++) same = got[i] == want[i].first;
  if (!same) {
    printf("%s: %s holds", what, dir.c_str());
    for (const std::string& n : got) printf(" %s", n.c_str());
    printf("\n");
    exit(1);
  }
  for (const auto& w : want) {
    if (w.second == "/") continue;
    const std::string s = slurp(dir + "/" + w.first);
    if (s != w.second) {
      printf("%s: %s/%s is\n%s<<<\nnot\n%s<<<\n", what, dir.c_str(), w.first.c_str(), s.c_str(), w.second.c_str());
      exit(1);
    }
  }
}
// `base` with some files replaced and some left out
static Files with(Files base, const Files& repl, const std::vector<std::string>& without = {}) {
  for (const auto& r : repl) {
    bool found = false;
    for (auto& b : base)
      if (b.first == r.first) b.second = r.second, found = true;
    if (!found) base.push_back(r);
  }
  Files out;
  for (const auto& b : base)
    if (std::find(without.begin(), without.end(), b.first) == without.end()) out.push_back(b);
  std::sort(out.begin(), out.end());
  return out;
}

// ---- the scenario
static const uint32_t T = 2, E = 5;
static const uint64_t kAddr[E] = {0x10000, 0x20000, 0x30000, 0x7ffc00000000ull, 0x50000};
static const uint64_t kSize[E] = {8192 + 100, 100, 4096, 8ull << 20, 64};
static const uint64_t kStack0[5] = {1, 2, 3, 0x401000, 0x7f0000001234ull};

struct Rec {
  uint32_t type;
  uint16_t size;
  uint32_t match;  // entry + 1, 0 = unmatched
  uint64_t ts, addr, weight, data_src;
};
static void pack(const std::vector<Rec>& recs, std::vector<uint8_t>& data, std::vector<uint32_t>& match) {
  for (const Rec& q : recs) {
    const size_t at = data.size();
    data.resize(at + q.size, 0);
    const uint16_t misc = 0;
    memcpy(&data[at], &q.type, 4);
    memcpy(&data[at + 4], &misc, 2);
    memcpy(&data[at + 6], &q.size, 2);
    if (q.size >= 40) {
      memcpy(&data[at + 8], &q.ts, 8);
      memcpy(&data[at + 16], &q.addr, 8);
      memcpy(&data[at + 24], &q.weight, 8);
      memcpy(&data[at + 32], &q.data_src, 8);
    }
    match.resize(data.size() / 8, 0);
    match[at / 8] = q.match;
  }
}
static constexpr uint64_t lvl(uint32_t bits) { return (uint64_t)bits << 5; }  // perf_mem_data_src.mem_lvl

struct Scenario {
  nmg_host_results r;
  nmg_object_meta meta[E];
  nmg_object objects[E];
  uint32_t buf_samples[2] = {5, 4}, buf_found[2] = {4, 3};
  uint64_t buf_bytes[2] = {0, 0};
  uint64_t first[E] = {1, 0, 3, 2, ~0ull};
  // [E][read count, read weight, write count, write weight]
  uint64_t cw[E * 4] = {1, 300, 1, 0, 1, 50, 1, 5, 1, 100, 1, 20, 1, 10, 0, 0, 0, 0, 0, 0};
  std::vector<uint64_t> levels;
  // (entry, thread, page, count), sorted by entry
  std::vector<uint32_t> cells = {0, 0, 1, 3, 0, 1, 2, 4, 0, 1, 1, 2, 0, 0, 3, 9,  // entry 0: page 3 is past its 3 rows
                                 1, 0, 0, 1, 1, 1, 5, 7,                          // entry 1: page 5 is past its row
                                 2, 0, 0, 6, 2, 2, 1, 9, 2, 1, 1, 1,              // entry 2: thread 2 is no thread
                                 3, 0, 7, 5};                                     // [stack]: no file
  std::vector<uint8_t> rd, wr;
  std::vector<uint32_t> rd_match, wr_match;
  DumpInput dump;
  nmg_module modules[1] = {{0x400000, 0x500000, 0x400000, "/bin/app"}};

  Scenario() {
    memset(&r, 0, sizeof(r));
    memset(meta, 0, sizeof(meta));
    const char* callers[E] = {"main.c:10 (alloc_a)", "lib.c:20 (alloc_b)", nullptr, "[stack]", "never.c:1"};
    const uint64_t rips[E] = {0x401000, 0x402000, 0x403000, 0, 0x405000};
    for (uint32_t e = 0; e < E; e++) {
      meta[e].initial_buffer_size = kSize[e];
      meta[e].caller_rip = rips[e];
      meta[e].mem_type = e == 3 ? 2 : 3;
      meta[e].caller = callers[e];
      meta[e].id = 100 + e;
      objects[e] = nmg_object{kAddr[e], kSize[e], e == 3 ? 0 : 10 + e, e == 3 ? 0 : 900 + e};
    }
    meta[0].callstack = kStack0;
    meta[0].callstack_size = 5;
    pack({{9, 40, 2, 1000, kAddr[1] + 0x10, 50, lvl(0x08 | 0x02)},          // site 1 is created here
          {9, 40, 1, 1001, kAddr[0] + 4096 + 8, 300, lvl(0x40 | 0x02)},     // site 2
          {1, 24, 0, 0, 0, 0, 0},                                           // not a SAMPLE record
          {9, 40, 4, 1002, kAddr[3] + 0x100, 10, lvl(0x80 | 0x02)},         // [stack]: site 3, no dump lines
          {9, 40, 0, 1003, 0xdead000, 7, lvl(0x20 | 0x04)},                 // unmatched
          {9, 40, 3, 1004, kAddr[2] + 4095, 100, lvl(0x10 | 0x02)}},        // site 4
         rd, rd_match);
    pack({{9, 40, 1, 2000, kAddr[0], 0, lvl(0x01)},
          {9, 40, 3, 2001, kAddr[2] + 4096, 20, lvl(0x100 | 0x04)},
          {9, 40, 0, 2002, 0x1, 0, 0},                                      // unmatched, no level bit
          {9, 40, 2, 2003, kAddr[1] + 99, 5, lvl(0x2000 | 0x02)},
          {9, 8, 0, 0, 0, 0, 0}},                                           // a SAMPLE header cut short
         wr, wr_match);
    buf_bytes[0] = rd.size();
    buf_bytes[1] = wr.size();
    levels.assign((size_t)E * 2 * kLevelWords, 0);
    auto level = [&](uint32_t e, uint32_t a, uint32_t bucket, uint64_t count, uint64_t weight) {
      uint64_t* lv = &levels[((size_t)e * 2 + a) * kLevelWords];
      lv[1 + 2 * bucket] = count;
      lv[2 + 2 * bucket] = weight;
    };
    level(0, 0, 2, 1, 300);   // entry 0 read: L3 Hit
    levels[(0 * 2 + 1) * kLevelWords] = 1;  // entry 0 write: N/A
    level(1, 0, 0, 1, 50);
    level(1, 1, 8, 1, 5);
    level(2, 0, 3, 1, 100);   // entry 2 read: LFB Hit
    level(2, 1, 9 + 5, 1, 20);  // entry 2 write: Remote RAM Miss
    level(3, 0, 4, 1, 10);

    r.global[0].total_count = 5;
    r.global[0].total_weight = 467;
    r.global[0].b[0] = nmg_count{1, 50, 50, 50};
    r.global[0].b[2] = nmg_count{1, 300, 300, 300};
    r.global[0].b[3] = nmg_count{1, 100, 100, 100};
    r.global[0].b[4] = nmg_count{1, 10, 10, 10};
    r.global[0].b[9 + 4] = nmg_count{1, 7, 7, 7};
    r.global[1].total_count = 4;
    r.global[1].total_weight = 25;
    r.global[1].na_miss_count = 1;
    r.global[1].b[8] = nmg_count{1, 5, 5, 5};
    r.global[1].b[9 + 5] = nmg_count{1, 20, 20, 20};
    r.nb_buffers = 2;
    r.nb_entries = E;
    r.buf_samples = buf_samples;
    r.buf_found = buf_found;
    r.buf_bytes = buf_bytes;
    r.buffer_size = kSize;
    r.first_ordinal = first;
    r.count_weight = cw;
    r.cells = cells.data();
    r.nb_cells = (int64_t)(cells.size() / 4);
    r.nb_threads = T;
    r.match_samples = 1;
    r.objects = objects;
    dump.buffers = {DumpBuffer{rd.data(), rd.size(), 0, NMG_ACCESS_READ, rd_match.data()},
                    DumpBuffer{wr.data(), wr.size(), 1, NMG_ACCESS_WRITE, wr_match.data()}};
    dump.entry_addr = kAddr;
    dump.levels = levels.data();
  }
  nmg_report_options opts(const char* dir, int flags, int single = 1) const {
    nmg_report_options o;
    memset(&o, 0, sizeof(o));
    o.output_dir = dir;
    o.dump_single_items = single;
    o.dump_flags = flags;
    o.maps_path = "/proc/42/maps";
    o.maps_text = "00400000-00500000 r-xp /bin/app\n7ffc00000000-7ffc00800000 rw-p [stack]\n";
    o.modules = modules;
    o.nb_modules = 1;
    return o;
  }
};

static const int kAllDumps = NMG_DUMP_CALLSITES | NMG_DUMP_ALL | NMG_DUMP_UNMATCHED;

// ---- the expected bytes (the formats are restated in oracle/nmg_oracle.c)
static const char kOutBanner[] =  // mem_sampling_finalize's messages and the banner
    "Analyzing 2 sample buffers\n"
    "\rAnalyzing sample buffer 0/2. Total samples so far: 0\n"
    "392 bytes processed\n"
    "---------------------------------\n"
    "         MEM ANALYZER\n"
    "---------------------------------\n";
static const char kOutCounters[] =  // __print_counters of the global counters, the headings of ma_finalize
    "\n"
    "# --------------------------------------\n"
    "# Summary of all the read memory access:\n"
    "# Total count          : \t 5\n"
    "# Total weigh          : \t 467\n"
    "# L1 Hit\t: 1 (20.000000 %) \tmin: 50 cycles\tmax: 50 cycles\t avg: 50 cycles\ttotal weight: 50 (10.706638 %)\n"
    "# L3 Hit\t: 1 (20.000000 %) \tmin: 300 cycles\tmax: 300 cycles\t avg: 300 cycles\ttotal weight: 300 (64.239829 %)\n"
    "# LFB Hit\t: 1 (20.000000 %) \tmin: 100 cycles\tmax: 100 cycles\t avg: 100 cycles\ttotal weight: 100 (21.413276 %)\n"
    "# Local RAM Hit\t: 1 (20.000000 %) \tmin: 10 cycles\tmax: 10 cycles\t avg: 10 cycles\ttotal weight: 10 (2.141328 %)\n"
    "\n"
    "# Local RAM Miss\t: 1 (20.000000 %) \tmin: 7 cycles\tmax: 7 cycles\t avg: 7 cycles\ttotal weight: 7 (1.498929 %)\n"
    "# --------------------------------------\n"
    "# Summary of all the write memory access:\n"
    "# Total count          : \t 4\n"
    "# Total weigh          : \t 25\n"
    "# N/A                  : \t 1 (25.000000 %)\n"
    "# Uncached memory Hit\t: 1 (25.000000 %) \tmin: 5 cycles\tmax: 5 cycles\t avg: 5 cycles\ttotal weight: 5 (20.000000 %)\n"
    "\n"
    "# Remote RAM Miss\t: 1 (25.000000 %) \tmin: 20 cycles\tmax: 20 cycles\t avg: 20 cycles\ttotal weight: 20 (80.000000 %)\n"
    "Summary of the call sites:\n"
    "--------------------------\n"
    "Sorting call sites\n";
static const char kSiteLines[] =  // print_call_site_summary: on stdout and in call_sites.log
    "2\tmain.c:10 (alloc_a) (size=8292) - 1 buffers. 1 read access (total weight: 300, avg weight: 300.000000). 1 wr_access\n"
    "4\t[0x403000] (size=4096) - 1 buffers. 1 read access (total weight: 100, avg weight: 100.000000). 1 wr_access\n"
    "1\tlib.c:20 (alloc_b) (size=100) - 1 buffers. 1 read access (total weight: 50, avg weight: 50.000000). 1 wr_access\n"
    "3\t[stack] (size=8388608) - 1 buffers. 1 read access (total weight: 10, avg weight: 10.000000). 0 wr_access\n";
static const char kOutTrailer[] =  // mem_sampling_statistics
    "9 samples (including 2 samples that do not match a known memory buffer / 22.222221%)\n";
static const char kUnmatched[] =  // the maps file's last line twice (feof after fgets)
    "# /proc/42/maps content:\n"
    "# 00400000-00500000 r-xp /bin/app\n"
    "# 7ffc00000000-7ffc00800000 rw-p [stack]\n"
    "# 7ffc00000000-7ffc00800000 rw-p [stack]\n"
    "#\n"
    "#\n"
    "#\n"
    "#thread_rank timestamp address mem_level access_weight access_type\n"
    "0 1003 0xdead000 L2_Miss 7 r\n"
    "1 2002 0x1 Unknown 0 w\n";
static const char kUnmatchedNoNewline[] =
    "# /proc/42/maps content:\n"
    "# 00400000-00500000 r-xp /bin/app\n"
    "# 7ffc00000000-7ffc00800000 rw-p [stack]#\n"
    "#\n"
    "#\n"
    "#thread_rank timestamp address mem_level access_weight access_type\n"
    "0 1003 0xdead000 L2_Miss 7 r\n"
    "1 2002 0x1 Unknown 0 w\n";
static const char kAllAccesses[] =
    "#thread_rank timestamp object_id offset mem_level access_weight access_type\n"
    "0 1000 101 16 L1_Hit 50 r\n"
    "0 1001 100 4104 L3_Hit 300 r\n"
    "0 1004 102 4095 LFB_Hit 100 r\n"
    "1 2000 100 0 NA 0 w\n"
    "1 2001 102 4096 Remote_RAM_1_hop_Miss 20 w\n"
    "1 2003 101 99 Uncached_Memory_Hit 5 w\n";
static const char kAllAccessesTwo[] =  // as far as the second record
    "#thread_rank timestamp object_id offset mem_level access_weight access_type\n"
    "0 1000 101 16 L1_Hit 50 r\n"
    "0 1001 100 4104 L3_Hit 300 r\n";
static const char kObjects[] =  // every row twice (quirk Q20)
    "#object_id\taddress\tsize\tallocation_date\tdeallocation_date\tcallstack_rip\tcallstack_offsets\tcallsite_rip\tcallsite\n"
    "100\t0x10000\t8292\t10\t900\t0x401000,0x7f0000001234\t/bin/app:4096,(null):139637976732212\t0x401000\tmain.c:10 (alloc_a)\n"
    "101\t0x20000\t100\t11\t901\tNULL\tNULL\t0x402000\tlib.c:20 (alloc_b)\n"
    "102\t0x30000\t4096\t12\t902\tNULL\tNULL\t0x403000\t[0x403000]\n"
    "103\t0x7ffc00000000\t8388608\t0\t0\tNULL\tNULL\t0x0\t[stack]\n"
    "104\t0x50000\t64\t14\t904\tNULL\tNULL\t0x405000\tnever.c:1\n"
    "100\t0x10000\t8292\t10\t900\t0x401000,0x7f0000001234\t/bin/app:4096,(null):139637976732212\t0x401000\tmain.c:10 (alloc_a)\n"
    "101\t0x20000\t100\t11\t901\tNULL\tNULL\t0x402000\tlib.c:20 (alloc_b)\n"
    "102\t0x30000\t4096\t12\t902\tNULL\tNULL\t0x403000\t[0x403000]\n"
    "103\t0x7ffc00000000\t8388608\t0\t0\tNULL\tNULL\t0x0\t[stack]\n"
    "104\t0x50000\t64\t14\t904\tNULL\tNULL\t0x405000\tnever.c:1\n";
static const char kDump1[] =
    "#thread_rank timestamp offset mem_level access_weight access_type\n"
    "0 1000 16 L1_Hit 50 r\n"
    "1 2003 99 Uncached_Memory_Hit 5 w\n";
static const char kDump1Read[] =
    "#thread_rank timestamp offset mem_level access_weight access_type\n"
    "0 1000 16 L1_Hit 50 r\n";
static const char kDump2[] =
    "#thread_rank timestamp offset mem_level access_weight access_type\n"
    "0 1001 4104 L3_Hit 300 r\n"
    "1 2000 0 NA 0 w\n";
static const char kDump4[] =
    "#thread_rank timestamp offset mem_level access_weight access_type\n"
    "0 1004 4095 LFB_Hit 100 r\n"
    "1 2001 4096 Remote_RAM_1_hop_Miss 20 w\n";
static const char kSummary2[] =  // min and max stay 0 (quirk Q8)
    "\n"
    "# --------------------------------------\n"
    "# Summary of all the read memory access:\n"
    "# Total count          : \t 1\n"
    "# Total weigh          : \t 300\n"
    "# L3 Hit\t: 1 (100.000000 %) \tmin: 0 cycles\tmax: 0 cycles\t avg: 300 cycles\ttotal weight: 300 (100.000000 %)\n"
    "\n"
    "# --------------------------------------\n"
    "# Summary of all the write memory access:\n"
    "# Total count          : \t 1\n"
    "# Total weigh          : \t 0\n"
    "# N/A                  : \t 1 (100.000000 %)\n"
    "\n";
static const char kSummary4[] =
    "\n"
    "# --------------------------------------\n"
    "# Summary of all the read memory access:\n"
    "# Total count          : \t 1\n"
    "# Total weigh          : \t 100\n"
    "# LFB Hit\t: 1 (100.000000 %) \tmin: 0 cycles\tmax: 0 cycles\t avg: 100 cycles\ttotal weight: 100 (100.000000 %)\n"
    "\n"
    "# --------------------------------------\n"
    "# Summary of all the write memory access:\n"
    "# Total count          : \t 1\n"
    "# Total weigh          : \t 20\n"
    "\n"
    "# Remote RAM Miss\t: 1 (100.000000 %) \tmin: 0 cycles\tmax: 0 cycles\t avg: 20 cycles\ttotal weight: 20 (100.000000 %)\n";
static const char kCounters1[] =  // buffer_size / 4096 + 1 rows x T
    "\t1\t0\n";
static const char kCounters2[] =
    "\t0\t0\n"
    "\t3\t2\n"
    "\t0\t4\n";
static const char kCounters4[] =
    "\t6\t0\n"
    "\t0\t1\n";
static const char kTimeline2[] =
    "#thread_rank timestamp offset count\n"
    "1 1000 8192 1\n"
    "0 1016 16384 7\n";
static const char kTimeline4[] =
    "#thread_rank timestamp offset count\n"
    "1 1000 0 5\n"
    "1 1112 8192 2\n";
static const char kCost2[] =
    "\t0\t0\n"
    "\t0\t0\n"
    "\t0\t1099511627781\n";
static const char kCost4[] =
    "\t0\t0\n"
    "\t7\t0\n";
static const char kBlocks[] =
    "#site 2 main.c:10 (alloc_a)\n"
    "begin_block\n"
    "malloc 8292 2\n"
    "0 0 1 30\n"
    "1 2 2 12\n"
    "end_block\n"
    "#site 4 ???\n"
    "begin_block\n"
    "malloc 4096 1\n"
    "1 0 0 8589934592\n"
    "end_block\n";

// a call: its code, its text, nothing left open
#define EXPECT_RC(call, code, text)                                                                                 \
  do {                                                                                                              \
    std::string err;                                                                                                \
    const size_t fds = open_fds();                                                                                  \
    const int rc = (call);                                                                                          \
    if (rc != (code) || err != (text) || open_fds() != fds) {                                                       \
      printf("%s:%d: %s gave %d \"%s\", %zu -> %zu descriptors\n", __FILE__, __LINE__, #call, rc, err.c_str(), fds, \
             open_fds());                                                                                           \
      exit(1);                                                                                                      \
    }                                                                                                               \
  } while (0)

static void block(const std::string& dir, const char* name) {  // a directory where a file is to be opened
  mkdir(dir.c_str(), S_IRWXU);
  CHECK(mkdir((dir + "/" + name).c_str(), S_IRWXU) == 0);
}

int main() {
  const Scenario s;
  const nmg_host_results* r = &s.r;
  const Files full = {{"all_memory_accesses.dat", kAllAccesses}, {"all_memory_objects.dat", kObjects},
                      {"call_sites.log", kSiteLines},            {"callsite_counters_1.dat", kCounters1},
                      {"callsite_counters_2.dat", kCounters2},   {"callsite_counters_4.dat", kCounters4},
                      {"callsite_dump_1.dat", kDump1},           {"callsite_dump_2.dat", kDump2},
                      {"callsite_dump_4.dat", kDump4},           {"callsite_summary_2.dat", kSummary2},
                      {"callsite_summary_4.dat", kSummary4},     {"unmatched_samples.log", kUnmatched}};
  const std::vector<std::string> per_site = {"callsite_counters_1.dat", "callsite_counters_2.dat",
                                             "callsite_counters_4.dat", "callsite_dump_1.dat",
                                             "callsite_dump_2.dat",     "callsite_dump_4.dat",
                                             "callsite_summary_2.dat",  "callsite_summary_4.dat"};
  const std::string out_dumped = std::string(kOutBanner), out_sorted = out_dumped + kOutCounters,
                    out_listed = out_sorted + kSiteLines, out_full = out_listed + kOutTrailer;

  // ---- 1. the report
  {
    nmg_report_options o = s.opts("a", kAllDumps);
    EXPECT_RC(write_report(r, s.meta, &o, "a.txt", err, &s.dump), NMG_OK, "");
    expect_dir("every dump mode", "a", full);
    CHECK(slurp("a.txt") == out_full);

    o = s.opts("b", kAllDumps);  // the maps file does not end with a newline: its last line is not repeated
    o.maps_text = "00400000-00500000 r-xp /bin/app\n7ffc00000000-7ffc00800000 rw-p [stack]";
    EXPECT_RC(write_report(r, s.meta, &o, "b.txt", err, &s.dump), NMG_OK, "");
    expect_dir("maps without a last newline", "b", with(full, {{"unmatched_samples.log", kUnmatchedNoNewline}}));
    CHECK(slurp("b.txt") == out_full);

    o = s.opts("c", kAllDumps, 0);  // dump_single_items = 0: no per-site file
    EXPECT_RC(write_report(r, s.meta, &o, "c.txt", err, &s.dump), NMG_OK, "");
    expect_dir("no single items", "c", with(full, {}, per_site));
    CHECK(slurp("c.txt") == out_full);

    o = s.opts("d", NMG_DUMP_CALLSITES);  // online: no dump mode; the stdout file is opened before the check
    o.online = 1;
    EXPECT_RC(write_report(r, s.meta, &o, "d.txt", err, &s.dump), NMG_ERR_INVALID,
              "dump modes are not available with online analysis (mem_sampling.c:644, 764, 799)");
    CHECK(slurp("d.txt") == "" && !exists("d"));

    o = s.opts("e", 0);  // no dump mode, to stdout: flushed, not closed (the last line of this program still gets out)
    EXPECT_RC(write_report(r, s.meta, &o, nullptr, err), NMG_OK, "");
    expect_dir("no dump mode", "e",
               {{"call_sites.log", kSiteLines}, {"callsite_counters_1.dat", kCounters1},
                {"callsite_counters_2.dat", kCounters2}, {"callsite_counters_4.dat", kCounters4}});
  }

  // ---- 2. the other writers
  // (entry, bin, thread, row, count): equal keys summed; [stack], a zero and the unmatched entry dropped
  const uint32_t tl_rows[] = {0, 1, 0, 2, 3, 2, 0, 1, 0, 5, 0, 1, 0, 2, 4, 3, 0, 0, 0, 9,
                              0, 0, 1, 1, 1, 1, 2, 0, 0, 0, 4, 0, 0, 0, 8, 2, 7, 1, 1, 2};
  const int64_t tl_n = sizeof(tl_rows) / sizeof(tl_rows[0]) / 5;
  const nmg_timeline_options tl = {1000, 4, 8, 1, 0, 0, 0};
  // (entry, thread, page, value): equal cells summed; pages past the site's rows, [stack] and zeros dropped
  const uint64_t pc_rows[] = {0, 1, 2, 1ull << 40, 2, 0, 1, 7, 0, 1, 2, 5, 0, 0, 3, 9,
                              3, 0, 0, 4,          2, 1, 0, 0, 1, 0, 1, 6, 4, 0, 0, 3};
  const int64_t pc_n = sizeof(pc_rows) / sizeof(pc_rows[0]) / 4;
  const std::vector<PlaceSite> sites = {{2, "main.c:10 (alloc_a)", "malloc", 8292}, {3, "g", "g", 64}, {4, "???", "malloc", 4096}};
  const uint64_t bl_rows[] = {2, 0, 0, 1, 30, 2, 1, 2, 2, 12, 4, 1, 0, 0, 1ull << 33};  // (site, node, first, last, count)
  {
    const nmg_report_options o = s.opts("w", 0);
    EXPECT_RC(write_timeline(r, s.meta, &o, &tl, tl_rows, tl_n, err), NMG_OK, "");
    EXPECT_RC(write_page_cost(r, s.meta, &o, pc_rows, pc_n, err), NMG_OK, "");
    EXPECT_RC(write_blocks(sites, bl_rows, 3, &o, err), NMG_OK, "");
    expect_dir("the other writers", "w",
               {{"blocks.dat", kBlocks}, {"callsite_cost_2.dat", kCost2}, {"callsite_cost_4.dat", kCost4},
                {"callsite_timeline_2.dat", kTimeline2}, {"callsite_timeline_4.dat", kTimeline4}});
  }

  // ---- 3. the error returns
  {  // the output directory under a missing parent
    const nmg_report_options o = s.opts("missing/x", kAllDumps);
    EXPECT_RC(write_report(r, s.meta, &o, "m.txt", err, &s.dump), NMG_ERR_IO,
              "cannot open missing/x/unmatched_samples.log");
    CHECK(slurp("m.txt") == out_dumped);
    EXPECT_RC(write_timeline(r, s.meta, &o, &tl, tl_rows, tl_n, err), NMG_ERR_IO,
              "cannot open missing/x/callsite_timeline_2.dat");
    EXPECT_RC(write_page_cost(r, s.meta, &o, pc_rows, pc_n, err), NMG_ERR_IO,
              "cannot open missing/x/callsite_cost_2.dat");
    EXPECT_RC(write_blocks(sites, bl_rows, 3, &o, err), NMG_ERR_IO, "cannot open missing/x/blocks.dat");
    CHECK(!exists("missing"));
  }
  {  // the second site's dump file: the lazy open fails with `out`, two dump files and a site's file open
    block("f1", "callsite_dump_2.dat");
    const nmg_report_options o = s.opts("f1", kAllDumps);
    EXPECT_RC(write_report(r, s.meta, &o, "f1.txt", err, &s.dump), NMG_ERR_IO, "cannot open f1/callsite_dump_2.dat");
    expect_dir("callsite_dump_2.dat", "f1",
               {{"all_memory_accesses.dat", kAllAccessesTwo}, {"callsite_dump_1.dat", kDump1Read},
                {"callsite_dump_2.dat", "/"}, {"unmatched_samples.log", ""}});
    CHECK(slurp("f1.txt") == out_dumped);
  }
  {
    block("f2", "all_memory_accesses.dat");
    const nmg_report_options o = s.opts("f2", kAllDumps);
    EXPECT_RC(write_report(r, s.meta, &o, "f2.txt", err, &s.dump), NMG_ERR_IO,
              "cannot open f2/all_memory_accesses.dat");
    expect_dir("all_memory_accesses.dat", "f2", {{"all_memory_accesses.dat", "/"}, {"unmatched_samples.log", ""}});
    CHECK(slurp("f2.txt") == out_dumped);
  }
  {
    block("f3", "call_sites.log");
    const nmg_report_options o = s.opts("f3", kAllDumps);
    EXPECT_RC(write_report(r, s.meta, &o, "f3.txt", err, &s.dump), NMG_ERR_IO, "cannot open f3/call_sites.log");
    expect_dir("call_sites.log", "f3",
               with(full, {{"call_sites.log", "/"}},
                    {"all_memory_objects.dat", "callsite_counters_1.dat", "callsite_counters_2.dat",
                     "callsite_counters_4.dat"}));
    CHECK(slurp("f3.txt") == out_sorted);
  }
  {  // the walk stops at site 4 first
    block("f4", "callsite_summary_4.dat");
    const nmg_report_options o = s.opts("f4", kAllDumps);
    EXPECT_RC(write_report(r, s.meta, &o, "f4.txt", err, &s.dump), NMG_ERR_IO,
              "cannot open f4/callsite_summary_4.dat");
    expect_dir("callsite_summary_4.dat", "f4",
               with(full, {{"callsite_summary_4.dat", "/"}},
                    {"all_memory_objects.dat", "call_sites.log", "callsite_counters_1.dat", "callsite_counters_2.dat",
                     "callsite_counters_4.dat", "callsite_summary_2.dat"}));
    CHECK(slurp("f4.txt") == out_sorted);
  }
  for (const char* threads : {"1", "3"}) {  // the page-file pool stops and the first error wins
    const std::string dir = std::string("f5_") + threads;
    block(dir, "callsite_counters_4.dat");
    setenv("NMG_REPORT_THREADS", threads, 1);
    const nmg_report_options o = s.opts(dir.c_str(), kAllDumps);
    EXPECT_RC(write_report(r, s.meta, &o, "f5.txt", err, &s.dump), NMG_ERR_IO,
              "cannot open " + dir + "/callsite_counters_4.dat");
    unsetenv("NMG_REPORT_THREADS");
    CHECK(slurp("f5.txt") == out_listed);
    CHECK(!exists(dir + "/all_memory_objects.dat") && slurp(dir + "/call_sites.log") == kSiteLines);
    if (threads[0] == '1')  // the report order is 2, 4, 1: one thread wrote site 2's file and never reached site 1's
      expect_dir("callsite_counters_4.dat", dir,
                 with(full, {{"callsite_counters_4.dat", "/"}}, {"all_memory_objects.dat", "callsite_counters_1.dat"}));
  }
  {
    block("f6", "blocks.dat");
    const nmg_report_options o = s.opts("f6", 0);
    EXPECT_RC(write_blocks(sites, bl_rows, 3, &o, err), NMG_ERR_IO, "cannot open f6/blocks.dat");
  }
  printf("nmg_report_dump_host: ok\n");
  return 0;
}
