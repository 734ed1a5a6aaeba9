// ws_copy_pool.h -- the host copies of the staging path (ws_staging.cpp): a pool of helper threads and the AVX2
// streaming forms.  No HIP here: tests/cxx/copy_pool_check.cpp builds it with g++ under ThreadSanitizer.
#pragma once

#if defined(__x86_64__)
#include <immintrin.h>
#endif
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#pragma GCC visibility push(hidden) // (internal to the library: nothing here is exported)
namespace wsamd {

// The stages' host copies: several threads for big buffers (one core moves ~12 GB/s, PCIe 50: a 9 MB image pair would
// spend longer in memcpy than on the bus).  A small pool of helper threads, started at the first big copy and shared by
// all contexts (one copy at a time uses it) -- a banded call copies a megabyte at a time, too little to start threads for
// (tests/cxx/copy_pool_check.cpp runs this class under ThreadSanitizer).  A job is a run of ELEMENTS moved as they are or
// widened on the way (the wire formats of ws_staging.h): int16 -> float / double, float -> double.
enum CopyKind { kCopyBytes, kCopyI16F32, kCopyI16F64, kCopyF32F64 };

// Streaming forms (AVX2, non-temporal stores) for the copies that WIDEN TO DOUBLES -- the one host copy that writes far
// more than it reads (config 2, CV_64F: 3 MB of int16 in, 12 MB of doubles out): an ordinary store first reads the line
// it overwrites.  A/B on one GPU box's host (EPYC 9575F, 8 copy threads, 3 x 30 calls each, profiles/r04/host_trace.txt):
// the CV_64F call 0.455 -> 0.437 ms with every copy streaming, but the CV_32F call 0.400 -> 0.420 -- the stage copies
// and the float map are better off in the cache, where the copy engine and the caller find them.  WS_COPY_STREAM=0
// turns the streaming forms off, =2 applies them to every copy.
#if defined(__x86_64__)
#define WS_AVX2 __attribute__((target("avx2")))
WS_AVX2 inline void stream_bytes(uint8_t *dst, const uint8_t *src, size_t n)
{
    const size_t head = (32 - (reinterpret_cast<uintptr_t>(dst) & 31)) & 31;
    if (n < 256 + head) { memcpy(dst, src, n); return; }
    memcpy(dst, src, head);
    size_t i = head;
    for (; i + 128 <= n; i += 128) {
        const __m256i a = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i));
        const __m256i b = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i + 32));
        const __m256i c = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i + 64));
        const __m256i d = _mm256_loadu_si256(reinterpret_cast<const __m256i *>(src + i + 96));
        _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i), a);
        _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i + 32), b);
        _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i + 64), c);
        _mm256_stream_si256(reinterpret_cast<__m256i *>(dst + i + 96), d);
    }
    memcpy(dst + i, src + i, n - i);
    _mm_sfence();
}
WS_AVX2 inline void stream_i16_f64(double *d, const int16_t *s, size_t n)
{
    size_t i = 0;
    for (; i < n && (reinterpret_cast<uintptr_t>(d + i) & 31); ++i) d[i] = (double)s[i];
    for (; i + 8 <= n; i += 8) {
        const __m256i v = _mm256_cvtepi16_epi32(_mm_loadu_si128(reinterpret_cast<const __m128i *>(s + i)));
        _mm256_stream_pd(d + i, _mm256_cvtepi32_pd(_mm256_castsi256_si128(v)));
        _mm256_stream_pd(d + i + 4, _mm256_cvtepi32_pd(_mm256_extracti128_si256(v, 1)));
    }
    for (; i < n; ++i) d[i] = (double)s[i];
    _mm_sfence();
}
WS_AVX2 inline void stream_i16_f32(float *d, const int16_t *s, size_t n)
{
    size_t i = 0;
    for (; i < n && (reinterpret_cast<uintptr_t>(d + i) & 31); ++i) d[i] = (float)s[i];
    for (; i + 8 <= n; i += 8)
        _mm256_stream_ps(d + i, _mm256_cvtepi32_ps(_mm256_cvtepi16_epi32(_mm_loadu_si128(reinterpret_cast<const __m128i *>(s + i)))));
    for (; i < n; ++i) d[i] = (float)s[i];
    _mm_sfence();
}
WS_AVX2 inline void stream_f32_f64(double *d, const float *s, size_t n)
{
    size_t i = 0;
    for (; i < n && (reinterpret_cast<uintptr_t>(d + i) & 31); ++i) d[i] = (double)s[i];
    for (; i + 4 <= n; i += 4) _mm256_stream_pd(d + i, _mm256_cvtps_pd(_mm_loadu_ps(s + i)));
    for (; i < n; ++i) d[i] = (double)s[i];
    _mm_sfence();
}
inline int stream_mode() // 0 = never, 1 = the copies that widen to doubles, 2 = every copy
{
    static const int v = [] {
        if (!__builtin_cpu_supports("avx2")) return 0;
        const char *e = getenv("WS_COPY_STREAM");
        return e ? std::max(0, std::min(2, atoi(e))) : 1;
    }();
    return v;
}
#else
inline int stream_mode() { return 0; }
inline void stream_bytes(uint8_t *, const uint8_t *, size_t) {}
inline void stream_i16_f64(double *, const int16_t *, size_t) {}
inline void stream_i16_f32(float *, const int16_t *, size_t) {}
inline void stream_f32_f64(double *, const float *, size_t) {}
#endif

inline void copy_piece(uint8_t *dst, const uint8_t *src, size_t first, size_t count, CopyKind kind)
{
    const int sm = stream_mode();
    const bool fast = count >= 4096 && (sm == 2 || (sm == 1 && (kind == kCopyI16F64 || kind == kCopyF32F64)));
    switch (kind) {
    case kCopyBytes:
        if (fast) stream_bytes(dst + first, src + first, count);
        else memcpy(dst + first, src + first, count);
        break;
    case kCopyI16F32: {
        const int16_t *s = reinterpret_cast<const int16_t *>(src) + first;
        float *d = reinterpret_cast<float *>(dst) + first;
        if (fast) { stream_i16_f32(d, s, count); break; }
        for (size_t i = 0; i < count; ++i) d[i] = (float)s[i];
        break;
    }
    case kCopyI16F64: {
        const int16_t *s = reinterpret_cast<const int16_t *>(src) + first;
        double *d = reinterpret_cast<double *>(dst) + first;
        if (fast) { stream_i16_f64(d, s, count); break; }
        for (size_t i = 0; i < count; ++i) d[i] = (double)s[i];
        break;
    }
    case kCopyF32F64: {
        const float *s = reinterpret_cast<const float *>(src) + first;
        double *d = reinterpret_cast<double *>(dst) + first;
        if (fast) { stream_f32_f64(d, s, count); break; }
        for (size_t i = 0; i < count; ++i) d[i] = (double)s[i];
        break;
    }
    }
}

class CopyPool {
public:
    static CopyPool &get()
    {
        // (never destroyed: its threads wait on members of it, and a process that exits must not join them)
        static CopyPool *pool = [] {
            CopyPool *p = new CopyPool;
            // a forked child has the object but none of its threads (and whatever state a helper was in): it copies alone
            pthread_atfork(nullptr, nullptr, [] { if (instance_) instance_->orphaned(); });
            instance_ = p;
            return p;
        }();
        return *pool;
    }
    // n elements (bytes for kCopyBytes)
    void copy(uint8_t *dst, const uint8_t *src, size_t n, CopyKind kind = kCopyBytes)
    {
        if (n < 2 * kPiece || workers_.empty()) { copy_piece(dst, src, 0, n, kind); return; }
        std::lock_guard<std::mutex> one_at_a_time(submit_);
        {
            // (a helper that woke up late for the copy before is still inside work(): the job's fields are its to read)
            std::unique_lock<std::mutex> lk(m_);
            cv_done_.wait(lk, [&] { return active_ == 0; });
            dst_ = dst; src_ = src; n_ = n; kind_ = kind;
            pieces_ = (n + kPiece - 1) / kPiece;
            next_.store(0);
            done_ = 0;
            ++generation_;
        }
        cv_.notify_all();
        const size_t mine = work();
        std::unique_lock<std::mutex> lk(m_);
        done_ += mine;
        cv_done_.wait(lk, [&] { return done_ == pieces_ && active_ == 0; });
    }
    ~CopyPool()
    {
        {
            std::lock_guard<std::mutex> lk(m_);
            stop_ = true;
        }
        cv_.notify_all();
        for (std::thread &t : workers_) t.join();
    }

private:
    static constexpr size_t kPiece = (size_t)128 << 10; // elements per piece
    static inline CopyPool *instance_ = nullptr;
    CopyPool()
    {
        unsigned cores = std::thread::hardware_concurrency();
        // one process per GPU on a node (torchrun / mpirun export the local world size): the ranks share the host's cores
        for (const char *name : {"LOCAL_WORLD_SIZE", "OMPI_COMM_WORLD_LOCAL_SIZE", "MPI_LOCALNRANKS"})
            if (const char *e = getenv(name)) {
                const int ranks = atoi(e);
                if (ranks > 1) cores /= (unsigned)ranks;
                break;
            }
        unsigned n = cores >= 16 ? 7 : cores >= 8 ? 3 : cores >= 4 ? 1 : 0; // helpers beside the calling thread
        if (const char *e = getenv("WS_COPY_THREADS")) n = (unsigned)std::max(0, std::min(31, atoi(e) - 1));
        for (unsigned i = 0; i < n; ++i) {
            try { workers_.emplace_back([this] { loop(); }); }
            catch (...) { break; }
        }
    }
    void orphaned() // in the child of a fork: no helper exists here, whatever the parent's were doing
    {
        // (the std::thread objects are the parent's: dropped without a join, their destructors never run -- `new`ed state)
        new (&workers_) std::vector<std::thread>();
        new (&submit_) std::mutex();
        new (&m_) std::mutex();
        new (&cv_) std::condition_variable();
        new (&cv_done_) std::condition_variable();
        active_ = 0;
        done_ = pieces_ = 0;
        generation_ = 0;
    }
    size_t work()
    {
        size_t count = 0;
        for (;;) {
            const size_t i = next_.fetch_add(1);
            if (i >= pieces_) break;
            const size_t off = i * kPiece;
            copy_piece(dst_, src_, off, std::min(kPiece, n_ - off), kind_);
            ++count;
        }
        return count;
    }
    void loop()
    {
        unsigned long long seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return stop_ || generation_ != seen; });
                if (stop_) return;
                seen = generation_;
                ++active_;
            }
            const size_t count = work();
            std::lock_guard<std::mutex> lk(m_);
            done_ += count;
            --active_;
            cv_done_.notify_all();
        }
    }
    std::vector<std::thread> workers_;
    std::mutex submit_, m_;
    std::condition_variable cv_, cv_done_;
    uint8_t *dst_ = nullptr;
    const uint8_t *src_ = nullptr;
    size_t n_ = 0, pieces_ = 0, done_ = 0;
    CopyKind kind_ = kCopyBytes;
    int active_ = 0; // helpers inside work()
    std::atomic<size_t> next_{0};
    unsigned long long generation_ = 0;
    bool stop_ = false;
};

} // namespace wsamd
#pragma GCC visibility pop
