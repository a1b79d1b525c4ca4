/* TEST INFRASTRUCTURE ONLY -- stand-in for libpfm4's header of this name: the
 * reference's hot path takes only the kernel's perf ABI from it. */
#include <inttypes.h>
#include <sys/syscall.h>
#include <unistd.h>
#include <linux/perf_event.h>
