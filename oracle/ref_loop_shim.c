/*
 * ref_loop_shim.c -- TEST INFRASTRUCTURE ONLY.
 *
 * ctypes-friendly harness around the reference's own sample loop.  The
 * reference's src/mem_sampling.c and src/mem_analyzer.c are compiled
 * unchanged, from where they lie, by being #included below (which is how the
 * shim reaches their static functions: __copy_buffer, __analyze_buffer and,
 * through them, __match_sample); oracle/Makefile adds tools/hash.c and builds
 * oracle/_ref/libref_loop.so.  What the reference needs from numap, libpfm,
 * its interposer (mem_intercept.c, numamma.c) and its symboliser
 * (mem_tools.c) is supplied here: no-op sampling calls, the globals, and a
 * get_caller_rip / get_caller_function_from_rip pair that needs no
 * libbacktrace and gives every object the same caller, so that call sites
 * differ by size alone.
 *
 * The reference's abort() and failed assert() calls come back to the caller
 * of the shim as a status (RL_ABORT, RL_ASSERT) instead of ending the
 * process: abort is a macro here, and the library's own __assert_fail is
 * bound with -Bsymbolic-functions.
 *
 * Objects are numbered by the shim in the order they were added; the dates
 * of an object are set by the caller after the reference created it, since
 * the reference stamps new_date() (the wall clock).
 */
#define _GNU_SOURCE
#include <assert.h>
#include <dlfcn.h>
#include <errno.h>
#include <execinfo.h>
#include <fcntl.h>
#include <gelf.h>
#include <inttypes.h>
#include <link.h>
#include <pthread.h>
#include <setjmp.h>
#include <signal.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <sys/types.h>
#include <time.h>
#include <unistd.h>

enum { RL_OK = 0, RL_ABORT = 1, RL_ASSERT = 2, RL_BAD_ARG = 3 };

static jmp_buf rl_jmp;
static int rl_armed;

static void rl_leave(int status) {
  if (rl_armed) longjmp(rl_jmp, status);
  _exit(70 + status);
}

/* (every system header that declares abort is already in: the macro only
 * meets the reference's calls) */
static void rl_abort(void) { rl_leave(RL_ABORT); }
#define abort() rl_abort()

void __assert_fail(const char *expr, const char *file, unsigned int line, const char *func) {
  (void)expr, (void)file, (void)line, (void)func;
  rl_leave(RL_ASSERT);
  for (;;) {
  }
}

/* ---- the reference, unchanged ------------------------------------------ */
#include "mem_sampling.c"
#include "mem_analyzer.c"

/* ---- what mem_intercept.c / numamma.c / mem_tools.c own ----------------- */
struct numamma_settings settings;
void *(*libcalloc)(size_t, size_t) = calloc;
void *(*libmalloc)(size_t) = malloc;
void (*libfree)(void *) = free;
void *(*librealloc)(void *, size_t) = realloc;
int (*libpthread_create)(pthread_t *, const pthread_attr_t *, void *(*)(void *), void *) = pthread_create;
void (*libpthread_exit)(void *) = pthread_exit;
__thread volatile int is_recurse_unsafe = 0;
FILE *dump_file = NULL;
FILE *dump_unmatched_file = NULL;

static char rl_log_dir[] = "/tmp";
char *get_log_dir() { return rl_log_dir; }
void create_log_filename(char *basename, char *filename, int length) {
  snprintf(filename, (size_t)length, "%s/%s", rl_log_dir, basename);
}
void unset_ld_preload() {}
void reset_ld_preload() {}

/* one caller for every object: no call stack, one fixed rip */
void **get_caller_rip(int depth, int *size_callstack, void **caller_rip) {
  (void)depth;
  *size_callstack = 0;
  *caller_rip = (void *)(uintptr_t)0x1000;
  return NULL;
}
static char rl_caller[] = "ref_loop_shim";
char *get_caller_function_from_rip(void *rip) {
  (void)rip;
  return rl_caller;
}
char *get_caller_function(int depth) {
  (void)depth;
  return rl_caller;
}

/* ---- numap: nothing samples -------------------------------------------- */
int numap_init(void) { return 0; }
const char *numap_error_message(int error) {
  (void)error;
  return "numap stand-in";
}
int numap_sampling_init_measure(struct numap_sampling_measure *m, int nb_threads, int rate, int mmap_pages) {
  (void)nb_threads, (void)rate, (void)mmap_pages;
  memset(m, 0, sizeof(*m));
  return 0;
}
int numap_sampling_set_measure_handler(struct numap_sampling_measure *m, numap_stub_handler_t h, int nb_refresh) {
  (void)m, (void)h, (void)nb_refresh;
  return 0;
}
int numap_sampling_read_start_generic(struct numap_sampling_measure *m, uint64_t t) {
  (void)m, (void)t;
  return 0;
}
int numap_sampling_write_start_generic(struct numap_sampling_measure *m, uint64_t t) {
  (void)m, (void)t;
  return 0;
}
int numap_sampling_read_stop(struct numap_sampling_measure *m) {
  (void)m;
  return 0;
}
int numap_sampling_write_stop(struct numap_sampling_measure *m) {
  (void)m;
  return 0;
}
int numap_sampling_resume(struct numap_sampling_measure *m) {
  (void)m;
  return 0;
}
int numap_sampling_end(struct numap_sampling_measure *m) {
  (void)m;
  return 0;
}
int numap_sampling_write_supported(void) { return 0; }
static char rl_level[] = "?";
char *get_data_src_level(union perf_mem_data_src data_src) { /* (dump modes only: never on) */
  (void)data_src;
  return rl_level;
}
/* declared by the reference's header, defined nowhere in it (do_get_at_analysis stays 0) */
void ma_get_lib_variables() {}
void ma_get_global_variables() {}

/* ---- the shim's own state ---------------------------------------------- */
struct rl_object {
  struct mem_block_info *info; /* malloc'd objects: what the interposer would hold */
  struct memory_info *mi;      /* the record the reference created */
};
static struct rl_object *rl_objs;
static int rl_nb_objs, rl_cap_objs;
static int rl_started;

#define RL_GUARD(status_var)                 \
  int status_var = setjmp(rl_jmp);           \
  rl_armed = (status_var == 0);              \
  if (status_var == 0)

static void rl_free_blocks(struct memory_info *mi) {
  if (!mi->blocks) return;
  for (int t = 0; t < MAX_THREADS; t++) {
    struct block_info *b = mi->blocks[t];
    while (b) {
      struct block_info *n = b->next;
      free(b);
      b = n;
    }
  }
  free(mi->blocks);
  mi->blocks = NULL;
}

/* Reset: drop everything the last run left, then ma_init() with the given
 * settings (offline analysis; no flush handler, no alarm). */
int rl_reset(int match_samples) {
  RL_GUARD(st) {
    if (rl_started) {
      for (int i = 0; i < rl_nb_objs; i++) {
        rl_free_blocks(rl_objs[i].mi);
        free(rl_objs[i].info);
      }
      while (call_sites) {
        struct call_site *s = call_sites;
        call_sites = s->next;
        rl_free_blocks(&s->mem_info);
        free(s);
      }
      while (samples) {
        struct sample_list *s = samples;
        samples = s->next;
        free(s->buffer);
      }
      if (mem_list) ht_release(mem_list);
      mem_list = NULL;
      mem_allocator_finalize(mem_info_allocator);
      mem_allocator_finalize(string_allocator);
      mem_allocator_finalize(sample_mem);
      nb_sample_buffers = 0;
      nb_samples_total = nb_found_samples_total = 0;
      is_sampling = 0;
    }
    rl_nb_objs = 0;
    memset(&settings, 0, sizeof(settings));
    settings.sampling_rate = SETTINGS_SAMPLING_RATE_DEFAULT;
    settings.buffer_size = SETTINGS_BUFFER_SIZE_DEFAULT;
    settings.match_samples = match_samples;
    settings.dump_single_items = SETTINGS_DUMP_SINGLE_ITEMS;
    ma_init();
    rl_started = 1;
  }
  rl_armed = 0;
  return st;
}

static int rl_push(struct mem_block_info *info, struct memory_info *mi) {
  if (rl_nb_objs == rl_cap_objs) {
    rl_cap_objs = rl_cap_objs ? 2 * rl_cap_objs : 1024;
    rl_objs = realloc(rl_objs, sizeof(*rl_objs) * (size_t)rl_cap_objs);
  }
  rl_objs[rl_nb_objs].info = info;
  rl_objs[rl_nb_objs].mi = mi;
  return rl_nb_objs++;
}

/* Add an object.  kind 0: malloc'd (ma_record_malloc); 1: a global variable
 * (insert_memory_info, the path ma_get_variables takes); 2: the [stack]
 * (ma_register_stack: the reference's own fixed range, addr and size are not
 * read).  Returns the object's number, or -1 - status. */
int rl_add(int kind, uint64_t addr, uint64_t size, uint64_t alloc_date, uint64_t free_date) {
  int idx = -1;
  RL_GUARD(st) {
    struct memory_info *mi = NULL;
    struct mem_block_info *info = NULL;
    if (kind == 0) {
      info = calloc(1, sizeof(*info));
      info->u_ptr = (void *)(uintptr_t)addr;
      info->size = size;
      ma_record_malloc(info);
      mi = info->record_info;
    } else if (kind == 1) {
      mi = insert_memory_info(global_symbol, size, (void *)(uintptr_t)addr, "global");
    } else if (kind == 2) {
      ma_register_stack();
      mi = ma_find_mem_info_from_addr((uint64_t)(uintptr_t)0x7fa000000000);
    }
    if (!mi) {
      st = RL_BAD_ARG;
    } else {
      mi->alloc_date = alloc_date;
      mi->free_date = free_date;
      idx = rl_push(info, mi);
    }
  }
  rl_armed = 0;
  return st ? -1 - st : idx;
}

/* realloc moved the object (ma_update_buffer_address) */
int rl_move(int idx, uint64_t new_addr) {
  if (idx < 0 || idx >= rl_nb_objs || !rl_objs[idx].info) return RL_BAD_ARG;
  RL_GUARD(st) {
    struct mem_block_info *info = rl_objs[idx].info;
    ma_update_buffer_address(info, info->u_ptr, (void *)(uintptr_t)new_addr);
    info->u_ptr = (void *)(uintptr_t)new_addr;
  }
  rl_armed = 0;
  return st;
}

/* free() of an object whose size is now `size` (ma_record_free) */
int rl_free(int idx, uint64_t size, uint64_t free_date) {
  if (idx < 0 || idx >= rl_nb_objs || !rl_objs[idx].info) return RL_BAD_ARG;
  RL_GUARD(st) {
    rl_objs[idx].info->size = size;
    ma_record_free(rl_objs[idx].info);
    rl_objs[idx].mi->free_date = free_date;
  }
  rl_armed = 0;
  return st;
}

/* what the reference holds for an object: addr, size, initial size, alloc, free, mem_type */
int rl_object(int idx, uint64_t out[6]) {
  if (idx < 0 || idx >= rl_nb_objs) return RL_BAD_ARG;
  struct memory_info *mi = rl_objs[idx].mi;
  out[0] = (uint64_t)(uintptr_t)mi->buffer_addr;
  out[1] = mi->buffer_size;
  out[2] = mi->initial_buffer_size;
  out[3] = mi->alloc_date;
  out[4] = mi->free_date;
  out[5] = (uint64_t)mi->mem_type;
  return RL_OK;
}

static int rl_index_of(const struct memory_info *mi) {
  for (int i = 0; i < rl_nb_objs; i++)
    if (rl_objs[i].mi == mi) return i;
  return -2;
}

/* ma_find_mem_info_from_sample on n (addr, timestamp) pairs: the object's
 * number per sample, -1 for no match */
int rl_find(int64_t n, const uint64_t *addr, const uint64_t *ts, int32_t *out) {
  RL_GUARD(st) {
    for (int64_t i = 0; i < n; i++) {
      struct mem_sample s;
      memset(&s, 0, sizeof(s));
      s.addr = addr[i];
      s.timestamp = ts[i];
      struct memory_info *mi = ma_find_mem_info_from_sample(&s);
      out[i] = mi ? rl_index_of(mi) : -1;
    }
  }
  rl_armed = 0;
  return st;
}

/* Feed one buffer: a perf_event_mmap_page in front of a copy of the ring,
 * described to the reference as __process_samples describes it to
 * __copy_buffer; then the copy the reference queued goes through
 * __analyze_buffer, as mem_sampling_finalize does for every queued buffer.
 * counts[0..1] = samples seen / found in this buffer (also when the walk
 * stopped on abort()). */
int rl_feed(const uint8_t *ring, uint64_t ring_size, uint64_t data_tail, uint64_t data_head, unsigned rank,
            int access, int32_t counts[2]) {
  static int nb, found; /* (not locals: read after a longjmp) */
  static uint8_t *area;
  nb = found = 0;
  if (rank >= MAX_THREADS || access < 0 || access >= ACCESS_MAX || ring_size == 0) return RL_BAD_ARG;
  size_t page = 4096;
  area = calloc(1, page + ring_size);
  RL_GUARD(st) {
    struct perf_event_mmap_page *meta = (struct perf_event_mmap_page *)area;
    meta->data_offset = page;
    meta->data_size = ring_size;
    meta->data_head = data_head;
    meta->data_tail = data_tail;
    memcpy(area + page, ring, ring_size);
    struct numap_sampling_measure m;
    memset(&m, 0, sizeof(m));
    m.nb_threads = 1;
    m.metadata_pages_per_tid[0] = meta;

    struct perf_event_mmap_page *mp = m.metadata_pages_per_tid[0];
    struct sample_list in;
    memset(&in, 0, sizeof(in));
    in.buffer = (struct perf_event_header *)((uint8_t *)mp + mp->data_offset);
    in.data_tail = mp->data_tail;
    in.data_head = mp->data_head % mp->data_size;
    in.buffer_size = mp->data_size;
    in.access_type = (enum access_type)access;
    in.thread_rank = rank;
    int before = nb_sample_buffers;
    __copy_buffer(&in, &nb, &found);
    if (nb_sample_buffers != before) {
      __analyze_buffer(samples, &nb, &found);
    }
  }
  rl_armed = 0;
  /* drop what was queued, analysed or not */
  while (samples) {
    struct sample_list *s = samples;
    samples = s->next;
    free(s->buffer);
    mem_allocator_free(sample_mem, s);
  }
  free(area);
  area = NULL;
  counts[0] = nb;
  counts[1] = found;
  nb_samples_total += (uint64_t)nb;
  nb_found_samples_total += (uint64_t)found;
  return st;
}

/* both global_counters as raw bytes, then the sample / found totals */
int rl_globals(uint8_t *out, uint64_t totals[2]) {
  memcpy(out, global_counters, sizeof(global_counters));
  totals[0] = nb_samples_total;
  totals[1] = nb_found_samples_total;
  return (int)sizeof(global_counters);
}

int rl_counters_bytes(void) { return (int)sizeof(struct mem_counters); }

/* An object's page blocks with a count: rows of 2 + 2 * words u64 (thread,
 * block id, counters[READ], counters[WRITE] as they lie in memory), threads
 * ascending, blocks in list order.  Returns the number of such rows (all of
 * them, also past cap), -1 if the object never matched. */
int64_t rl_blocks(int idx, uint64_t *out, int64_t cap) {
  if (idx < 0 || idx >= rl_nb_objs) return -3;
  struct memory_info *mi = rl_objs[idx].mi;
  if (!mi->blocks) return -1;
  const size_t words = sizeof(struct mem_counters) / 8;
  int64_t n = 0;
  for (int t = 0; t < MAX_THREADS; t++)
    for (struct block_info *b = mi->blocks[t]; b; b = b->next) {
      if (!b->counters[0].total_count && !b->counters[1].total_count) continue;
      if (n < cap) {
        uint64_t *row = out + (size_t)n * (2 + 2 * words);
        row[0] = (uint64_t)t;
        row[1] = b->block_id;
        memcpy(row + 2, b->counters, 2 * sizeof(struct mem_counters));
      }
      n++;
    }
  return n;
}

/* update_counters called directly.  fresh != 0: both counters are
 * initialised (init_mem_counter) before every sample and written to
 * out[i] (2 * sizeof(struct mem_counters) bytes each); fresh == 0: they
 * are initialised once, take all n samples, and out holds the one pair. */
int rl_update_counters(int64_t n, const uint64_t *data_src, const uint64_t *weight, int access, int fresh,
                       uint8_t *out) {
  if (access < 0 || access >= ACCESS_MAX) return RL_BAD_ARG;
  RL_GUARD(st) {
    struct mem_counters c[2];
    init_mem_counter(&c[0]);
    init_mem_counter(&c[1]);
    for (int64_t i = 0; i < n; i++) {
      struct mem_sample s;
      memset(&s, 0, sizeof(s));
      s.weight = weight[i];
      memcpy(&s.data_src, &data_src[i], sizeof(uint64_t));
      if (fresh) {
        init_mem_counter(&c[0]);
        init_mem_counter(&c[1]);
      }
      update_counters(c, &s, (enum access_type)access);
      if (fresh) memcpy(out + (size_t)i * sizeof(c), c, sizeof(c));
    }
    if (!fresh) memcpy(out, c, sizeof(c));
  }
  rl_armed = 0;
  return st;
}
