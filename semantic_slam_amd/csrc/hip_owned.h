// hip_owned.h -- move-only owners of HIP device memory, pinned host memory, events, streams and graphs: the only place in
// csrc that calls the HIP release functions.  An owner converts implicitly to the raw pointer or handle, so kernel arguments
// and HIP calls take it as they took the raw value; it releases what it holds when reset, assigned over or destroyed (with
// the resource's device current: the destroy functions of the library see to that).  A lazily allocated group of resources
// is built in local owners and moved into the handle only once every part exists.  Also: Growable buffers, StageRing.
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

// A buffer of T that grows on demand and never shrinks: ensure(n) leaves room for n elements.  A reallocation does not keep the
// contents and knows nothing of streams (what may still use the old block is the caller's to wait for: fits); on failure the
// buffer holds nothing and its capacity is 0.
template <typename T, typename Owner>
class Growable {
public:
    operator T *() const { return p_; }
    T *get() const { return p_.get(); }
    size_t capacity() const { return cap_; }
    bool fits(size_t n) const { return n <= cap_; }     // ensure(n) would not reallocate
    hipError_t ensure(size_t n)
    {
        if (fits(n)) return hipSuccess;
        cap_ = 0;
        const hipError_t e = alloc(p_, n * sizeof(T));
        if (e == hipSuccess) cap_ = n;
        return e;
    }
private:
    static hipError_t alloc(DevPtr<T> &p, size_t bytes) { return dev_alloc(p, bytes); }
    static hipError_t alloc(HostPtr<T> &p, size_t bytes) { return host_alloc(p, bytes, hipHostMallocDefault); }
    Owner p_;
    size_t cap_ = 0;
};
template <typename T> using DevBuf = Growable<T, DevPtr<T>>;
template <typename T> using HostBuf = Growable<T, HostPtr<T>>;     // pinned

// A block the host fills in pinned memory and a kernel reads from its copy in HBM.
template <typename T> struct Staged { HostPtr<T> host; DevPtr<T> dev; };

// N staging slots used in turn.  A slot is its payload (allocated by the user: lazily per slot, or all at creation), the event
// of its last consumer and whether one was ever queued.
template <typename Payload, int N>
struct StageRing {
    struct Slot : Payload { Event done; bool used = false; };
    Slot slots[N];
    int next = 0;
    // the next slot in turn, once the consumer queued at its last use has run: the host may refill it
    hipError_t take(Slot **out)
    {
        Slot *s = *out = &slots[next];
        next = (next + 1) % N;
        return s->used ? hipEventSynchronize(s->done) : hipSuccess;
    }
    // the slot's consumer has been queued on `stream`
    static hipError_t consumed(Slot *s, hipStream_t stream)
    {
        const hipError_t e = hipEventRecord(s->done, stream);
        if (e == hipSuccess) s->used = true;
        return e;
    }
};

// A lazily allocated slot of a ring of staged blocks: both blocks of `bytes` and the event, all three or none.
template <typename T> hipError_t staged_alloc(Staged<T> &s, Event &done, size_t bytes)
{
    Staged<T> t;
    Event ev;
    hipError_t e = host_alloc(t.host, bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = dev_alloc(t.dev, bytes);
    if (e == hipSuccess) e = event_create(ev);
    if (e == hipSuccess) { s = std::move(t); done = std::move(ev); }
    return e;
}

}  // namespace hip_owned
