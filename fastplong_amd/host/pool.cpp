#include "pool.h"

#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

using namespace std;

namespace fplh {

/* the first two words of a small file (cgroup settings): how many of them there were */
static int file_words(const char* path, char (&a)[64], char (&b)[64]) {
    a[0] = b[0] = 0;
    FILE* f = fopen(path, "r");
    if (!f) return 0;
    const int n = fscanf(f, "%63s %63s", a, b);
    fclose(f);
    return n;
}

int effective_cpus() {
    static const int cached = []() {
        if (const char* e = getenv("FPLH_CPUS"))
            if (atoi(e) > 0) return atoi(e);
        int n = max(1, (int)std::thread::hardware_concurrency());
        cpu_set_t set;
        CPU_ZERO(&set);
        if (sched_getaffinity(0, sizeof(set), &set) == 0 && CPU_COUNT(&set) > 0) n = min(n, (int)CPU_COUNT(&set));
        auto quota = [](const char* path, bool v2) -> double {
            char a[64], b[64];
            const int n = file_words(path, a, b);
            if (v2) return n == 2 && strcmp(a, "max") != 0 && atof(b) > 0 ? atof(a) / atof(b) : 0; /* "max 100000" or "<quota> <period>" */
            return n >= 1 ? atof(a) : 0; /* microseconds per period, -1 = none */
        };
        double q = quota("/sys/fs/cgroup/cpu.max", true);
        if (q <= 0) {
            const double us = quota("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", false), per = quota("/sys/fs/cgroup/cpu/cpu.cfs_period_us", false);
            if (us > 0 && per > 0) q = us / per;
        }
        if (q > 0) n = min(n, max(1, (int)(q + 0.5)));
        return n;
    }();
    return cached;
}

/* Bytes of memory this process may still take: the smaller of what the machine has available (MemAvailable) and what its
   cgroup leaves (memory.max - memory.current, v2; limit_in_bytes - usage_in_bytes, v1) -- a container's limit is usually far
   below the node's RAM, and going over it is a kill, not an error.  FPLH_MEM_BYTES overrides (tests). */
uint64_t memory_budget() {
    if (const char* e = getenv("FPLH_MEM_BYTES"))
        if (atoll(e) > 0) return (uint64_t)atoll(e);
    auto number = [](const char* path, uint64_t& v) -> bool {
        char a[64], b[64];
        if (file_words(path, a, b) < 1 || a[0] < '0' || a[0] > '9') return false; /* "max": no limit */
        v = strtoull(a, nullptr, 10);
        return true;
    };
    uint64_t best = (uint64_t)sysconf(_SC_PHYS_PAGES) * (uint64_t)sysconf(_SC_PAGE_SIZE);
    if (FILE* f = fopen("/proc/meminfo", "r")) {
        char line[256];
        while (fgets(line, sizeof(line), f)) {
            unsigned long long kb = 0;
            if (sscanf(line, "MemAvailable: %llu kB", &kb) == 1) best = min<uint64_t>(best, (uint64_t)kb << 10);
        }
        fclose(f);
    }
    uint64_t lim = 0, use = 0;
    if (number("/sys/fs/cgroup/memory.max", lim) || number("/sys/fs/cgroup/memory/memory.limit_in_bytes", lim)) {
        if (!number("/sys/fs/cgroup/memory.current", use)) number("/sys/fs/cgroup/memory/memory.usage_in_bytes", use);
        if (lim < (1ull << 60)) best = min<uint64_t>(best, lim > use ? lim - use : 0);
    }
    return best;
}

namespace {
class Pool {
   public:
    Pool() {
        const int hw = effective_cpus();
        int n = min(64, max(1, hw - 1));
        if (const char* e = getenv("FPLH_POOL_THREADS"))
            if (atoi(e) >= 0) n = atoi(e);
        for (int i = 0; i < n; i++) workers_.emplace_back([this]() { work(); });
    }
    ~Pool() {
        {
            lock_guard<mutex> g(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : workers_) t.join();
    }
    void run(int tasks, const function<void(int)>& fn) {
        if (tasks <= 0) return;
        if (tasks == 1 || workers_.empty()) {
            for (int i = 0; i < tasks; i++) fn(i);
            return;
        }
        Job job{&fn, tasks, 0, {0}};
        {
            lock_guard<mutex> g(m_);
            jobs_.push_back(&job);
        }
        cv_.notify_all();
        for (;;) { /* the caller works too */
            int i;
            {
                lock_guard<mutex> g(m_);
                i = claim(&job);
            }
            if (i < 0) break;
            fn(i);
            job.done.fetch_add(1);
        }
        unique_lock<mutex> g(m_);
        done_cv_.wait(g, [&]() { return job.done.load() == tasks; });
    }

   private:
    struct Job {
        const function<void(int)>* fn;
        int n, next;
        atomic<int> done;
    };
    /* next index of job j, or -1 when all are handed out (m_ held); a job leaves the queue with its last index, so
       nobody looks at it once its caller may have returned */
    int claim(Job* j) {
        if (j->next >= j->n) return -1;
        const int i = j->next++;
        if (j->next == j->n) jobs_.erase(std::find(jobs_.begin(), jobs_.end(), j));
        return i;
    }
    void work() {
        unique_lock<mutex> g(m_);
        for (;;) {
            cv_.wait(g, [&]() { return stop_ || !jobs_.empty(); });
            if (stop_) return;
            Job* j = jobs_.front();
            const int i = claim(j);
            if (i < 0) continue;
            const function<void(int)>* fn = j->fn;
            const int n = j->n;
            g.unlock();
            (*fn)(i);
            const bool last = j->done.fetch_add(1) + 1 == n; /* j may be gone right after this */
            g.lock();
            if (last) done_cv_.notify_all();
        }
    }
    mutex m_;
    condition_variable cv_, done_cv_;
    deque<Job*> jobs_;
    vector<std::thread> workers_;
    bool stop_ = false;
};
}  // namespace

void parallel_run(int tasks, const function<void(int)>& fn) {
    static Pool pool;
    pool.run(tasks, fn);
}

}  // namespace fplh
