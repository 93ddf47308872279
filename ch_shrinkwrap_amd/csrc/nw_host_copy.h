// The host half of handing a block's result back (nanowrap.hip: nw_search_end, nw_write_back, nw_host_copy_rows): the copy threads, the
// row copier and the chunked copy-out that follows the flag word.  Plain host C++ -- no HIP header and no HIP call, so that
// tests/test_host_copy_cpu.py can compile it into a program of its own and run it under ThreadSanitizer and AddressSanitizer.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

// The flag word in pinned memory (k_block_done, k_copy_slice: written last, after the data it announces).  The acquire orders the reads
// of the staging buffer that follow a successful wait behind this load; on x86-64 it is a plain load.
inline int nw_flag_load(const int *flag) { return __atomic_load_n(flag, __ATOMIC_ACQUIRE); }

// rows [v0, v1) of `src` (float[3] each) -> `contiguous` (may be null) and / or the records `rows` of `row_stride_bytes` each (may be
// null), the records only where valid[v] != 0 (`valid` may be null: all of them)
inline void nw_copy_rows(const float *src, int64_t v0, int64_t v1, float *contiguous, void *rows, int64_t row_stride_bytes, const unsigned char *valid)
{
    if (contiguous) memcpy(contiguous + 3 * v0, src + 3 * v0, (size_t)(v1 - v0) * 12);
    if (rows) {
        char *dst = (char *)rows;
        for (int64_t v = v0; v < v1; ++v)
            if (!valid || valid[v]) memcpy(dst + v * row_stride_bytes, src + 3 * v, 12);
    }
}

// Small persistent host thread pool for the write-back (the strided copy into the caller's vertex records is host-memory bound: one
// thread moves ~0.4 GB/s of 12-byte rows).  A job is a number of CHUNKS taken from a shared counter by whoever is awake -- the calling
// thread included -- and it ends when every chunk has been done, not when every thread has shown up: a thread the scheduler wakes late
// (the GPU boxes' hosts are shared; a woken thread can arrive 15 ms later) finds the counter exhausted and goes back to sleep, instead
// of holding the block up (round 5).  arm(): work is about to come -- the threads wake now and spin for it for a bounded time.
struct NwHostPool {
    struct Job { std::function<void(int)> fn; int n = 0; std::atomic<int> next{0}, done{0}; };
    std::vector<std::thread> th;
    std::mutex m;
    std::condition_variable cv_work;
    std::shared_ptr<Job> job;
    std::atomic<unsigned long> generation{0};
    unsigned long arm_generation = 0;
    bool stop = false;
    int n = 1;
    // on_thread_start: what every thread of the pool does first (the library binds it to its device)
    void start(int threads, const std::function<void()> &on_thread_start = nullptr)
    {
        n = threads < 1 ? 1 : threads;
        for (int t = 1; t < n; ++t)
            th.emplace_back([this, on_thread_start] {
                if (on_thread_start) on_thread_start();
                unsigned long seen = 0, seen_arm = 0;
                for (;;) {
                    std::shared_ptr<Job> j;
                    {
                        std::unique_lock<std::mutex> lk(m);
                        cv_work.wait(lk, [&] { return stop || generation.load() != seen || arm_generation != seen_arm; });
                        if (stop) return;
                        if (generation.load() == seen) {
                            // armed: spin for the job (bounded), then take it like a woken thread
                            seen_arm = arm_generation;
                            lk.unlock();
                            const auto t0 = std::chrono::steady_clock::now();
                            while (generation.load(std::memory_order_acquire) == seen) {
                                for (int k = 0; k < 32; ++k) __builtin_ia32_pause();
                                if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(1500)) break;
                            }
                            lk.lock();
                            if (stop) return;
                            if (generation.load() == seen) continue;          // nothing came: back to sleep
                        }
                        seen_arm = arm_generation;
                        seen = generation.load();
                        j = job;
                    }
                    if (j) work(*j);
                }
            });
    }
    void arm()
    {
        if (n <= 1) return;
        {
            std::lock_guard<std::mutex> lk(m);
            ++arm_generation;
        }
        cv_work.notify_all();
    }
    // a job in the BACKGROUND: the pool's threads work through it while the caller goes on (a block's strided mesh records, written
    // while the next block runs on the GPU); wait_posted() lends a hand with what is left and returns when it is done
    void post_chunks(int nchunks, const std::function<void(int)> &f)
    {
        wait_posted();
        if (nchunks <= 0) return;
        if (n <= 1) { for (int c = 0; c < nchunks; ++c) f(c); return; }
        posted = publish(nchunks, f);
    }
    void wait_posted()
    {
        if (!posted) return;
        std::shared_ptr<Job> j = posted;
        posted.reset();
        finish(j);
    }
    // f(c) for c in [0, nchunks), each exactly once, on whichever threads are awake; returns when all have been done
    void run_chunks(int nchunks, const std::function<void(int)> &f)
    {
        wait_posted();
        if (nchunks <= 0) return;
        if (n <= 1 || nchunks == 1) { for (int c = 0; c < nchunks; ++c) f(c); return; }
        finish(publish(nchunks, f));
    }
    void run(const std::function<void(int)> &f) { run_chunks(n, f); }
    void shutdown()
    {
        {
            std::lock_guard<std::mutex> lk(m);
            stop = true;
        }
        cv_work.notify_all();
        for (auto &t : th) t.join();
        th.clear();
    }

private:
    std::shared_ptr<Job> posted;
    static void work(Job &j)
    {
        for (;;) {
            const int c = j.next.fetch_add(1, std::memory_order_relaxed);
            if (c >= j.n) break;
            j.fn(c);
            j.done.fetch_add(1, std::memory_order_release);
        }
    }
    // the job becomes the one the pool's threads take, and they are woken
    std::shared_ptr<Job> publish(int nchunks, const std::function<void(int)> &f)
    {
        auto j = std::make_shared<Job>();
        j->fn = f; j->n = nchunks;
        {
            std::lock_guard<std::mutex> lk(m);
            job = j;
            generation.fetch_add(1, std::memory_order_release);
        }
        cv_work.notify_all();
        return j;
    }
    // the calling thread helps, waits until every chunk has been done and takes the job away
    void finish(const std::shared_ptr<Job> &j)
    {
        work(*j);
        while (j->done.load(std::memory_order_acquire) < j->n)
            for (int k = 0; k < 8; ++k) __builtin_ia32_pause();
        std::lock_guard<std::mutex> lk(m);
        if (job == j) job.reset();
    }
};

// The staged result `src` (M rows) -> the caller's arrays, in chunks of 8192 rows taken from a counter by the copy threads and the
// calling thread (NwHostPool::run_chunks; `pool` may be null: the calling thread alone).  slice_rows > 0: the staging buffer is being
// filled slice by slice (k_copy_slice launches behind the block's last kernel); the flag word reads flag_base + 1 + (slices complete),
// and a chunk waits for its slice.  false: a slice did not arrive within `give_up` (a slice is tens of microseconds of PCIe: seconds of
// silence mean the device is not going to answer; a parameter for the tests' sake).
// defer_rows (NW_FLAG_ROWS_ASYNC): the contiguous result now, the strided records behind the caller's back (the pool's threads;
// nw_synchronize, the next block's copy-out and everything that touches the staging buffer or the records' description wait for them).
inline bool nw_copy_out_chunks(const float *src, int64_t M, float *contiguous, void *rows, int64_t row_stride_bytes, const unsigned char *valid,
                               NwHostPool *pool, int64_t slice_rows, int flag_base, const int *flag, bool defer_rows,
                               std::chrono::steady_clock::duration give_up = std::chrono::seconds(10))
{
    const int64_t chunk = slice_rows > 0 ? std::max<int64_t>(4096, slice_rows / 2) : 8192;
    const int nchunks = (int)((M + chunk - 1) / chunk);
    defer_rows = defer_rows && rows && pool && pool->n > 1;
    void *rows_now = defer_rows ? nullptr : rows;
    std::atomic<bool> failed(false);
    auto work = [&](int c) {
        const int64_t v0 = (int64_t)c * chunk, v1 = std::min<int64_t>(M, v0 + chunk);
        if (slice_rows > 0) {
            const int need = flag_base + 1 + (int)((v1 - 1) / slice_rows) + 1;      // the chunk's last slice complete
            long spins = 0;
            const auto t0 = std::chrono::steady_clock::now();
            while (nw_flag_load(flag) - need < 0 && !failed.load(std::memory_order_relaxed)) {
                for (int k = 0; k < 8; ++k) __builtin_ia32_pause();
                if ((++spins & 4095) == 0 && std::chrono::steady_clock::now() - t0 > give_up) failed = true;
            }
            if (failed.load()) return;
        }
        nw_copy_rows(src, v0, v1, contiguous, rows_now, row_stride_bytes, valid);
    };
    if (!pool) { for (int c = 0; c < nchunks; ++c) work(c); return !failed.load(); }
    if (contiguous || !defer_rows || slice_rows > 0) pool->run_chunks(nchunks, work);
    if (failed.load()) return false;
    if (defer_rows) {
        const int64_t rchunk = 8192;
        pool->post_chunks((int)((M + rchunk - 1) / rchunk), [=](int c) {           // (by value: the job outlives this frame)
            nw_copy_rows(src, (int64_t)c * rchunk, std::min<int64_t>(M, (int64_t)c * rchunk + rchunk), nullptr, rows, row_stride_bytes, valid);
        });
    }
    return true;
}
