// Device buffers and helper threads of the plans.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "common.h"

namespace slu {

using std::vector;

template <typename T> struct DevBuf {
    T *p = nullptr;
    size_t n = 0, guard = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p - guard);
        p = nullptr;
        n = guard = 0;
    }
    void alloc(size_t cnt) {
        release();
        n = cnt;
        if (cnt) HIPCHK(hipMalloc(&p, cnt * sizeof(T)));
    }
    // cnt elements with g more allocated on either side: a kernel may read
    // (and mask) up to g elements outside [p, p + cnt) without a clamp
    void alloc_guarded(size_t cnt, size_t g) {
        release();
        HIPCHK(hipMalloc(&p, (cnt + 2 * g) * sizeof(T)));
        HIPCHK(hipMemset(p, 0, g * sizeof(T)));
        HIPCHK(hipMemset(p + g + cnt, 0, g * sizeof(T)));
        p += g;
        n = cnt;
        guard = g;
    }
    void swap(DevBuf &o) {
        std::swap(p, o.p);
        std::swap(n, o.n);
        std::swap(guard, o.guard);
    }
    void upload(const vector<T> &v) { upload(v.data(), v.size()); }
    void upload(const RawVec<T> &v) { upload(v.data(), v.size()); }
    void upload(const T *h, size_t cnt) {
        alloc(cnt);
        if (cnt) HIPCHK(hipMemcpy(p, h, cnt * sizeof(T), hipMemcpyHostToDevice));
    }
    size_t bytes() const { return n * sizeof(T); }
};

// A helper thread of a plan.  It touches the plan's DevBuf members, so the
// plans declare their HelperThreads after those members (members are
// destroyed in reverse order: the join comes before the buffers go).
struct HelperThread {
    std::thread t;
    std::string err;
    // runs hipSetDevice(device), then body; keeps the text of an exception
    template <typename F> void start(int device, F body) {
        t = std::thread([this, device, body]() mutable {
            try {
                HIPCHK(hipSetDevice(device));
                body();
            } catch (const std::exception &e) {
                err = e.what();
            }
        });
    }
    bool running() const { return t.joinable(); }
    void wait() { // joins; the error stays for join()
        if (t.joinable()) t.join();
    }
    // joins, and throws the thread's error once
    void join() {
        wait();
        if (err.empty()) return;
        std::string e;
        e.swap(err);
        throw Error(e);
    }
    ~HelperThread() { wait(); } // never throws
};

} // namespace slu
