/*
 * timing.h -- what FPLH_TIMING=1 reports when the process ends (TimingDump, fastq.cpp): the units of the host library add to
 * these counters, nobody outside it sees them.  All of them are trivially destructible, so the dump does not depend on the
 * order in which the units' statics go away.
 */
#ifndef FPLH_TIMING_H
#define FPLH_TIMING_H

#include <stdint.h>
#include <stdlib.h>

#include <atomic>
#include <chrono>

#pragma GCC visibility push(hidden)
namespace fplh {

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
inline const bool g_timing = getenv("FPLH_TIMING") != nullptr;
inline std::atomic<uint64_t> g_chunk_us[3]; /* microseconds the chunk parsers spent reading / locating / copying */
inline std::atomic<uint64_t> g_alloc_seconds_x1000{0}, g_alloc_bytes{0}; /* microseconds / bytes spent in the page-locked allocator */
inline double g_t_pull = 0, g_t_scan = 0, g_t_copy = 0; /* the sequential reader's phases, seconds */

}  // namespace fplh
#pragma GCC visibility pop
#endif
