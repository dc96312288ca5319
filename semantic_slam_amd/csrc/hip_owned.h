// hip_owned.h -- move-only owners of HIP device memory, pinned host memory, events, streams and graphs: the only place in
// csrc that calls the HIP release functions.  An owner converts implicitly to the raw pointer or handle, so kernel arguments
// and HIP calls take it as they took the raw value; it releases what it holds when reset, assigned over or destroyed (with
// the resource's device current: the destroy functions of the library see to that).  A lazily allocated group of resources
// is built in local owners and moved into the handle only once every part exists.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace hip_owned {

struct DevFree { void operator()(void *p) const { (void)hipFree(p); } };
struct HostFree { void operator()(void *p) const { (void)hipHostFree(p); } };
struct EventDestroy { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
struct StreamDestroy { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
struct GraphDestroy { void operator()(hipGraph_t g) const { (void)hipGraphDestroy(g); } };
struct GraphExecDestroy { void operator()(hipGraphExec_t g) const { (void)hipGraphExecDestroy(g); } };

// H: a pointer or one of HIP's opaque handle types; null = holds nothing.
template <typename H, typename Release>
class Owned {
public:
    Owned() = default;
    Owned(Owned &&o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Owned &operator=(Owned &&o) noexcept
    {
        if (this != &o) { reset(); h_ = std::exchange(o.h_, nullptr); }
        return *this;
    }
    ~Owned() { reset(); }
    operator H() const { return h_; }
    H get() const { return h_; }
    void reset() { if (h_) Release()(std::exchange(h_, nullptr)); }
    H *put() { reset(); return &h_; }     // the out-parameter of the call that creates the resource
private:
    H h_ = nullptr;
};

template <typename T> using DevPtr = Owned<T *, DevFree>;
template <typename T> using HostPtr = Owned<T *, HostFree>;
using Event = Owned<hipEvent_t, EventDestroy>;
using Stream = Owned<hipStream_t, StreamDestroy>;
using Graph = Owned<hipGraph_t, GraphDestroy>;
using GraphExec = Owned<hipGraphExec_t, GraphExecDestroy>;

// Each releases what the owner held first; on failure the owner holds nothing.
template <typename T> hipError_t dev_alloc(DevPtr<T> &p, size_t bytes) { return hipMalloc(reinterpret_cast<void **>(p.put()), bytes); }
template <typename T> hipError_t host_alloc(HostPtr<T> &p, size_t bytes, unsigned int flags)
{
    return hipHostMalloc(reinterpret_cast<void **>(p.put()), bytes, flags);
}
inline hipError_t event_create(Event &e, unsigned int flags = hipEventDisableTiming) { return hipEventCreateWithFlags(e.put(), flags); }
inline hipError_t stream_create(Stream &s) { return hipStreamCreateWithFlags(s.put(), hipStreamNonBlocking); }

}  // namespace hip_owned
