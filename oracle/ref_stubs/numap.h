/* TEST INFRASTRUCTURE ONLY -- stand-in for numap's header: the fields of a
 * sampling measure and the calls that the reference's mem_sampling.c touches.
 * oracle/ref_loop_shim.c defines the calls as no-ops; no sampling happens. */
#ifndef NMG_REF_STUB_NUMAP_H
#define NMG_REF_STUB_NUMAP_H
#include <stddef.h>
#include <stdint.h>
#include <sys/types.h>
#include <linux/perf_event.h>

#define NMG_STUB_MAX_TIDS 4
#define ERROR_PERF_EVENT_OPEN (-3)
#define rmb() __asm__ volatile("" ::: "memory")

struct numap_sampling_measure {
  unsigned nb_threads;
  pid_t tids[NMG_STUB_MAX_TIDS];
  struct perf_event_mmap_page *metadata_pages_per_tid[NMG_STUB_MAX_TIDS];
};

typedef void (*numap_stub_handler_t)(struct numap_sampling_measure *, int);

int numap_init(void);
const char *numap_error_message(int error);
int numap_sampling_init_measure(struct numap_sampling_measure *m, int nb_threads, int rate, int mmap_pages);
int numap_sampling_set_measure_handler(struct numap_sampling_measure *m, numap_stub_handler_t h, int nb_refresh);
int numap_sampling_read_start_generic(struct numap_sampling_measure *m, uint64_t sample_type);
int numap_sampling_write_start_generic(struct numap_sampling_measure *m, uint64_t sample_type);
int numap_sampling_read_stop(struct numap_sampling_measure *m);
int numap_sampling_write_stop(struct numap_sampling_measure *m);
int numap_sampling_resume(struct numap_sampling_measure *m);
int numap_sampling_end(struct numap_sampling_measure *m);
int numap_sampling_write_supported(void);
char *get_data_src_level(union perf_mem_data_src data_src);

#endif
