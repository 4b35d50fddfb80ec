// hip_owned.h — move-only owners of the HIP resources the engine's host half holds (engine.hip): device and pinned host buffers,
// events, streams.  Each frees what it holds when it goes (or is assigned over), so no path — least of all an early return between two
// allocations — can leak a resource or free one twice.  Kernels and HIP calls keep receiving the raw pointer / handle (implicit conversion).
// Also how the host half reports a failed HIP call: HIP_TRY, over the C ABI's last-error text (set_error).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <string>
#include <utility>

extern "C" void mc_set_error_internal(const char *msg);   // engine.hip, translation unit 0: the C ABI's last-error text

namespace mc {

inline void set_error(const std::string &s) { mc_set_error_internal(s.c_str()); }

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            mc::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                      \
            return MC_EHIP;                                                                        \
        }                                                                                          \
    } while (0)

// n elements of T in device memory (PINNED: in page-locked host memory)
template <class T, bool PINNED = false>
struct HipBuf {
    T *p = nullptr;
    size_t n = 0;  // elements held: 0 whenever p is null
    HipBuf() = default;
    HipBuf(HipBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    HipBuf &operator=(HipBuf &&o) noexcept { std::swap(p, o.p); std::swap(n, o.n); return *this; }
    ~HipBuf() { reset(); }
    void reset() { if (p) PINNED ? hipHostFree(p) : hipFree(p); p = nullptr; n = 0; }
    // a fresh buffer of `count` elements; what was held goes first
    hipError_t alloc(size_t count) {
        reset();
        const hipError_t e = PINNED ? hipHostMalloc((void **)&p, count * sizeof(T)) : hipMalloc((void **)&p, count * sizeof(T));
        if (e == hipSuccess) n = count; else p = nullptr;
        return e;
    }
    // at least `count` elements: grows (contents lost), never shrinks, and touches nothing when there is room already
    hipError_t reserve(size_t count) { return count > n ? alloc(count) : hipSuccess; }
    operator T *() const { return p; }
    T *operator->() const { return p; }
};
template <class T> using DevBuf = HipBuf<T, false>;
template <class T> using PinnedBuf = HipBuf<T, true>;

// an event, created on the first get() (most of the engine's are needed by one kind of run only)
struct Event {
    hipEvent_t e = nullptr;
    unsigned flags;
    explicit Event(unsigned flags_ = hipEventDisableTiming) : flags(flags_) {}
    Event(Event &&o) noexcept : e(o.e), flags(o.flags) { o.e = nullptr; }
    Event &operator=(Event &&o) noexcept { std::swap(e, o.e); std::swap(flags, o.flags); return *this; }
    ~Event() { if (e) hipEventDestroy(e); }
    hipError_t create() { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
    hipEvent_t get() { create(); return e; }  // (null after a failed creation: the HIP call it is handed to reports that)
    bool made() const { return e != nullptr; }  // get() was called: the event may have been recorded
};

struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream &&o) noexcept : s(o.s) { o.s = nullptr; }
    Stream &operator=(Stream &&o) noexcept { std::swap(s, o.s); return *this; }
    ~Stream() { if (s) hipStreamDestroy(s); }
    hipError_t create() { return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    hipError_t create(int priority) { return hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority); }
    operator hipStream_t() const { return s; }
};

}  // namespace mc
