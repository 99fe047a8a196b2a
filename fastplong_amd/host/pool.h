/*
 * pool.h -- the worker pool of the host library and what this process may use of the machine.
 */
#ifndef FPLH_POOL_H
#define FPLH_POOL_H

#include <stdint.h>

#include <functional>

namespace fplh {

/* Persistent worker threads for the short parallel phases of the host pipeline (window refill, record location,
 * line copies, output formatting, gzip members): a phase lasts a few milliseconds, so starting threads for it costs
 * as much as the work.  run(n, fn) executes fn(0) .. fn(n-1) on the workers and the calling thread and returns when
 * all are done; any number of threads may call it at the same time. */
void parallel_run(int tasks, const std::function<void(int)>& fn);
/* CPUs this process may actually use: the hardware threads, cut down to the scheduler affinity mask and to the cgroup's
   CPU bandwidth quota (cpu.max / cpu.cfs_quota_us) -- a container on a 256-thread node with a 16-CPU quota is throttled,
   not sped up, by 64 busy threads (FPLH_CPUS overrides) */
int effective_cpus();
uint64_t memory_budget(); /* bytes this process may still take: MemAvailable and the cgroup's limit */

}  // namespace fplh
#endif
