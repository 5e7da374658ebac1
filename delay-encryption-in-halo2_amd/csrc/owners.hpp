// owners.hpp -- who frees what on the host side of libdehalo.so.  Every device allocation, page-locked host buffer, event, stream, host-memory registration and
// object behind an opaque handle of include/dehalo.h is a member or a local of one of these types and is released by its destructor, nowhere else.  All of them are
// move-only and null-safe, with get() / release() as std::unique_ptr has them.  Includes HIP headers: not for guard.hpp, msm_plan.hpp or witness.hip (g++ builds).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/dehalo.h"

// what the fallible members below need of the context (internal.hpp): its last error and its stream
inline int dh_fail(dehalo_ctx* ctx, int code, const std::string& msg) noexcept;
inline hipStream_t dh_ctx_stream(dehalo_ctx* ctx);

#define HIP_TRY(ctx, expr)                                                                   \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            int code_ = (e_ == hipErrorOutOfMemory) ? DEHALO_ERR_OOM : DEHALO_ERR_HIP;        \
            return dh_fail(ctx, code_, std::string(#expr) + ": " + hipGetErrorString(e_));   \
        }                                                                                    \
    } while (0)

#define TRY(expr)                 \
    do {                          \
        int rc_ = (expr);         \
        if (rc_ != 0) return rc_; \
    } while (0)

// ---- device memory, typed by element (DevMem = DevArray<fe>, internal.hpp) ----
template <class T>
struct DevArray {
    T* p = nullptr;
    size_t elems = 0;
    DevArray() = default;
    DevArray(DevArray&& o) noexcept : p(std::exchange(o.p, nullptr)), elems(std::exchange(o.elems, 0)) {}
    DevArray& operator=(DevArray&& o) noexcept {
        if (this != &o) { reset(); p = std::exchange(o.p, nullptr); elems = std::exchange(o.elems, 0); }
        return *this;
    }
    ~DevArray() { reset(); }
    void reset() { if (p) (void)hipFree(p); p = nullptr; elems = 0; }
    T* get() const { return p; }
    T* release() { elems = 0; return std::exchange(p, nullptr); }
    int alloc(dehalo_ctx* ctx, size_t n_elems, bool zero = true) {
        reset();
        if (!n_elems) return 0;
        HIP_TRY(ctx, hipMalloc((void**)&p, n_elems * sizeof(T)));
        elems = n_elems;
        if (zero) HIP_TRY(ctx, hipMemsetAsync(p, 0, n_elems * sizeof(T), dh_ctx_stream(ctx)));
        return 0;
    }
    T* at(size_t elem) const { return p + elem; }
    uint64_t* u64(size_t elem = 0) const { return (uint64_t*)(p + elem); }
};

// ---- a grow-only workspace buffer of the context, in bytes (dh_ensure, internal.hpp) ----
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { if (p) (void)hipFree(p); p = std::exchange(o.p, nullptr); cap = std::exchange(o.cap, 0); }
        return *this;
    }
    ~DevBuf() { if (p) (void)hipFree(p); }
    void* get() const { return p; }
    void* release() { cap = 0; return std::exchange(p, nullptr); }
    // room for `bytes`: a buffer that is too small is freed only after the context's stream and the device have drained, then replaced by one an eighth larger
    int ensure(dehalo_ctx* ctx, size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) {
            HIP_TRY(ctx, hipStreamSynchronize(dh_ctx_stream(ctx)));
            HIP_TRY(ctx, hipDeviceSynchronize());
            HIP_TRY(ctx, hipFree(p));
            p = nullptr; cap = 0;
        }
        size_t want = bytes + bytes / 8 + 256;
        HIP_TRY(ctx, hipMalloc(&p, want));
        cap = want;
        return 0;
    }
};

// ---- events, streams, page-locked host memory: unique_ptr over the runtime's handle, filled by the make_ function ----
struct EventDestroy { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
struct StreamDestroy { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
struct HostFree { void operator()(void* p) const { (void)hipHostFree(p); } };
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventDestroy>;
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, StreamDestroy>;
template <class T>
using Pinned = std::unique_ptr<T, HostFree>;

inline hipError_t make_event(Event& out, unsigned flags) {
    hipEvent_t e = nullptr;
    const hipError_t rc = hipEventCreateWithFlags(&e, flags);
    out.reset(e);
    return rc;
}
inline hipError_t make_stream(Stream& out, unsigned flags) {
    hipStream_t s = nullptr;
    const hipError_t rc = hipStreamCreateWithFlags(&s, flags);
    out.reset(s);
    return rc;
}
template <class T>
hipError_t make_pinned(Pinned<T>& out, size_t bytes) {
    void* p = nullptr;
    const hipError_t rc = hipHostMalloc(&p, bytes, hipHostMallocDefault);
    out.reset((T*)p);
    return rc;
}

// ---- the objects behind dehalo_bases* / dehalo_graph* / dehalo_fixed_base*: released as dehalo_bases_release / dehalo_graph_release / dehalo_fixed_base_release release them (under the context's lock, after a
// device synchronise), also when they never reached the caller.  adopt(ctx, dst) stands for the out-parameter of the function that creates one:
// TRY(dehalo_graph_create(ctx, ..., adopt(ctx, g))) leaves the new handle, or none, in g. ----
struct BasesFree { dehalo_ctx* ctx = nullptr; void operator()(dehalo_bases* b) const { (void)dehalo_bases_release(ctx, b); } };
struct GraphFree { dehalo_ctx* ctx = nullptr; void operator()(dehalo_graph* g) const { (void)dehalo_graph_release(ctx, g); } };
struct FixedBaseFree { dehalo_ctx* ctx = nullptr; void operator()(dehalo_fixed_base* f) const { (void)dehalo_fixed_base_release(ctx, f); } };
using BasesPtr = std::unique_ptr<dehalo_bases, BasesFree>;
using GraphPtr = std::unique_ptr<dehalo_graph, GraphFree>;
using FixedBasePtr = std::unique_ptr<dehalo_fixed_base, FixedBaseFree>;

template <class Ptr>
struct Adopt {
    Ptr& dst;
    dehalo_ctx* ctx;
    typename Ptr::pointer raw = nullptr;
    ~Adopt() { dst = Ptr(raw, typename Ptr::deleter_type{ctx}); }
    operator typename Ptr::pointer*() { return &raw; }
};
template <class Ptr>
Adopt<Ptr> adopt(dehalo_ctx* ctx, Ptr& dst) { return {dst, ctx}; }

// ---- the page-locking of a caller's buffer for the duration of a call ----
// Caller buffers of the host entry points are ordinary pageable memory (a Rust Vec<F>): large ones are pinned for the duration of the
// call so that the copy engine reads / writes them directly instead of going through the runtime's bounce buffers (measured on
// MI355X, profiles/r02_host_path_measurements.txt: dehalo_ntt at 2^20, 32 MiB each way, 5.73 -> 1.35 ms), and so that the lifetime of the device's mapping of
// caller memory is this object's and nothing else's (the pin ends only after the stream that copies has been synchronised).  Registration failing (already
// pinned, exotic mapping) just leaves the pageable path.
// Several threads may hand over the SAME host buffer at once (batch proving: one witness array, four provers): the first registers it, the others count
// themselves in, and the pages are released by whoever leaves last -- a copy that found the buffer page-locked by another thread's registration must not
// lose that registration in flight.  A range that only partly overlaps a registered one registers (or falls back to the pageable path) independently.
struct HostPinRegistry {
    struct Entry { uintptr_t a, b; int refs; };
    std::mutex mu;
    std::vector<Entry> entries;
};
inline HostPinRegistry& host_pin_registry() { static HostPinRegistry r; return r; }

struct HostPin {
    void* p = nullptr;          // the caller's pointer when its pages are page-locked through this object (by its own registration or one it shares)
    uintptr_t key = 0;          // start of the registration it holds a reference to
    HostPin(const void* ptr, size_t bytes) {
        if (!ptr || bytes < HOST_PIN_MIN_BYTES) return;
        HostPinRegistry& reg = host_pin_registry();
        std::lock_guard<std::mutex> lk(reg.mu);
        const uintptr_t a = (uintptr_t)ptr, b = a + bytes;
        for (auto& e : reg.entries)
            if (e.a <= a && b <= e.b) { e.refs++; key = e.a; p = const_cast<void*>(ptr); return; }
        if (hipHostRegister(const_cast<void*>(ptr), bytes, hipHostRegisterDefault) == hipSuccess) {
            reg.entries.push_back({a, b, 1});
            key = a; p = const_cast<void*>(ptr);
        } else (void)hipGetLastError();
    }
    HostPin(const HostPin&) = delete;
    HostPin& operator=(const HostPin&) = delete;
    ~HostPin() {
        if (!p) return;
        HostPinRegistry& reg = host_pin_registry();
        std::lock_guard<std::mutex> lk(reg.mu);
        for (size_t i = 0; i < reg.entries.size(); i++)
            if (reg.entries[i].a == key) {
                if (--reg.entries[i].refs == 0) {
                    (void)hipHostUnregister((void*)key);
                    reg.entries.erase(reg.entries.begin() + i);
                }
                return;
            }
    }
    static constexpr size_t HOST_PIN_MIN_BYTES = 4u << 20;
};
