/*
 * split.h -- the --split / --split_by_lines writer
 * (reference src/threadconfig.cpp:72-120, src/seprocessor.cpp:297-316), shared by the CLI and the host tests.
 */
#ifndef FPLH_SPLIT_H
#define FPLH_SPLIT_H

#include <sys/uio.h>

#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace fplh {

/* --split / --split_by_lines.  Each of the reference's workers owns a writer and walks through the file numbers
 * t, t + T, t + 2T, ... as its current file fills up (ThreadConfig::initWriterForSplit / markProcessed /
 * writeEmptyFilesForSplitting, src/threadconfig.cpp:72-120); packs of PACK_SIZE = 16 reads reach the workers
 * round-robin (src/seprocessor.cpp:343-378), so which file a read lands in is a function of its input index.  The
 * one writer thread of this host replays that, pack by pack: write(t, text) is the worker's
 * getWriter1()->writeString(outstr), mark(t, n) its markProcessed(n), close() the ThreadConfig destructors.
 * Pinned against the real ThreadConfig / Writer objects of the reference (tests/test_host_split.py).
 *
 * What the pin leaves open is timing, not logic: with --split, a worker whose files are used up while
 * number % threads != 0 and id >= number % threads gets mCanBeStopped (src/threadconfig.cpp:103-107) and leaves
 * its loop the next time it finds its input queue EMPTY (src/seprocessor.cpp:432-441) -- packs that reach it later are
 * never processed, so how many reads the reference loses there depends on how far its reader thread is ahead.  This
 * writer reproduces the reference run in which the reader stays ahead (the worker never sees an empty queue before
 * the input ends): nothing is lost and the worker's last file takes the rest, exactly what the real objects do when
 * every pack is handed to them (the S_* commands of the test harness). */
class SplitOutput {
   public:
    /* bgzf: .gz files are BGZF blocks (bgzf_into) ended by the EOF block instead of gzip members */
    SplitOutput(const std::string& out, int digits, int workers, bool by_lines, int number, long size, int gz_level, bool bgzf = false);
    ~SplitOutput();
    void write(int t, const std::string& text);
    /* the same bytes as a gather list (plain files only): what is pending for worker t goes out first, then the list, by
       writev -- no copy of the text in user space */
    void write_gather(int t, struct iovec* iov, size_t cnt);
    void mark(int t, long reads);
    void close();
    bool gzipped() const { return gz_; }
    std::vector<std::string> names; /* the files opened, in the order they were opened (threaded: per worker, then merged) */

    /* One thread per worker -- the reference's writers ARE per worker (ThreadConfig owns its Writer, src/threadconfig.cpp:72-87),
     * and one file on tmpfs takes 6-9 GB/s whoever writes it while fifteen files take 60 (tools/file_write_probe.cpp).
     * start_threads() once; post(t, job) hands worker t's thread a job that calls write / write_gather / mark for worker t ONLY
     * (jobs of one worker run in the order they were posted, so every file gets the bytes the one-thread replay gives it);
     * close() drains the queues, runs the workers' clean-up and joins. */
    void start_threads();
    void post(int t, std::function<void()> job);
    bool threaded() const { return !threads_.empty(); }

   private:
    struct Worker {
        int working = 0;
        long current = 0;
        int fd = -1;
        bool wrote = false;
        std::string pending;
        std::vector<std::string> opened;
        /* threaded mode */
        std::mutex m;
        std::condition_variable cv;
        std::deque<std::function<void()>> q;
        bool stop = false;
    };
    void flush(Worker& w);
    void shut(Worker& w);
    void open(Worker& w);
    void finish(Worker& w);
    void put(Worker& w, const char* p, size_t n);
    std::string out_;
    int digits_, T_;
    bool by_lines_;
    int number_;
    long size_;
    int level_;
    bool gz_ = false;
    bool bgzf_ = false;
    std::vector<Worker> w_;
    std::vector<std::thread> threads_;
    bool closed_ = false;
};

}  // namespace fplh
#endif
