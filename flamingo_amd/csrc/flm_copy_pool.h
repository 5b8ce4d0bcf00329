// flm_copy_pool.h -- the CPU side of the host runtime's pinned-buffer copies (HostCopies and upload_rows in
// flm_runtime.hip, the store's adds).  Plain C++ threads, no HIP: checked under the host sanitizers (tools/planner_check.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

namespace flm {
namespace rt __attribute__((visibility("hidden"))) {  // the library exports nothing of this header

// Host copies between the caller's pageable arrays and the pinned bounce buffer (HostCopies), split
// over a context's few worker threads and the calling thread: a 4 MiB in + 4 MiB out client mask
// takes 0.34 ms of wall this way against 0.47 ms with one thread (profiles/r06_host_path_ab.txt).
// Cutting the copies into 1 MiB pieces pipelined with the DMA, with workers spinning between pieces,
// measured the same (0.34 ms) and was dropped.  Workers start lazily, on the first large copy.
class CopyPool {
  public:
    static constexpr int kWorkers = 3;                      // + the calling thread
    static constexpr size_t kMinSplit = size_t(256) << 10;  // below it the calling thread copies alone
    ~CopyPool() {
        {
            std::lock_guard<std::mutex> g(m_);
            stop_ = true;
        }
        work_.notify_all();
        for (auto &t : th_) t.join();
    }
    // rows x width bytes, src rows at spitch, dst rows at dpitch; returns once every byte is copied
    void copy2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t rows) {
        const size_t n = width * rows;
        if (n < kMinSplit) return part(dst, dpitch, src, spitch, width, 0, n);
        std::lock_guard<std::mutex> one_job(call_);  // a context's callers are one thread, a store's adds too
        if (th_.empty())
            for (int i = 0; i < kWorkers; ++i) th_.emplace_back([this, i] { run(i + 1); });
        {
            std::lock_guard<std::mutex> g(m_);
            job_ = {dst, dpitch, src, spitch, width, n};
            pending_ = kWorkers;
            ++gen_;
        }
        work_.notify_all();
        slice(0);
        std::unique_lock<std::mutex> l(m_);
        done_.wait(l, [this] { return pending_ == 0; });
    }

  private:
    struct Job {
        void *dst;
        size_t dpitch;
        const void *src;
        size_t spitch, width, n;
    };
    // bytes [b, e) of the packed rows x width range
    static void part(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t b, size_t e) {
        while (b < e) {
            const size_t r = b / width, c = b % width, m = std::min(width - c, e - b);
            std::memcpy(static_cast<uint8_t *>(dst) + r * dpitch + c, static_cast<const uint8_t *>(src) + r * spitch + c, m);
            b += m;
        }
    }
    void slice(int i) {  // slice i of kWorkers + 1, 4 KiB-aligned bounds
        const size_t per = ((job_.n + kWorkers) / (kWorkers + 1) + 4095) / 4096 * 4096;
        const size_t b = std::min(job_.n, per * i), e = std::min(job_.n, b + per);
        part(job_.dst, job_.dpitch, job_.src, job_.spitch, job_.width, b, e);
    }
    void run(int i) {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> l(m_);
                work_.wait(l, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
            }
            slice(i);
            bool last;
            {
                std::lock_guard<std::mutex> g(m_);
                last = --pending_ == 0;
            }
            if (last) done_.notify_one();
        }
    }
    std::mutex call_, m_;
    std::condition_variable work_, done_;
    std::vector<std::thread> th_;
    Job job_{};
    uint64_t gen_ = 0;
    int pending_ = 0;
    bool stop_ = false;
};

}  // namespace rt
}  // namespace flm
