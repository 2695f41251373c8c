// Host-side owners of what a context allocates: device buffers, page-locked host memory, events.  Each is move-only (declaring the moves deletes the copies) and frees
// what it holds when it goes out of scope, so a struct of them needs no clean-up code of its own, and std::swap and std::vector
// growth hand the allocation over.  Nothing here synchronises: whoever destroys an owner has made sure that no stream still uses
// it (vc_destroy drains every stream before it deletes the context).
// The three macros name the calls that free; a host-only test of the lifetimes defines them (and hipEvent_t) before the include.
#pragma once

#include <cstddef>
#include <utility>

#ifndef VC_OWNED_DEVICE_FREE
#define VC_OWNED_DEVICE_FREE(p) ((void)hipFree(p))
#define VC_OWNED_HOST_FREE(p) ((void)hipHostFree(p))
#define VC_OWNED_EVENT_DESTROY(e) ((void)hipEventDestroy(e))
#endif

namespace vc {

struct DeviceMem { static void release(void *p) { VC_OWNED_DEVICE_FREE(p); } };
struct HostMem { static void release(void *p) { VC_OWNED_HOST_FREE(p); } };

// `cap` elements at `ptr`, allocated by whoever fills the two in (ensure, ensure_pinned) and freed here.
template <typename T, typename Mem>
struct Block {
    T *ptr = nullptr;
    size_t cap = 0;     // elements
    Block() = default;
    Block(Block &&o) noexcept : ptr(std::exchange(o.ptr, nullptr)), cap(std::exchange(o.cap, 0)) {}
    Block &operator=(Block &&o) noexcept
    {
        if (this != &o) { reset(); ptr = std::exchange(o.ptr, nullptr); cap = std::exchange(o.cap, 0); }
        return *this;
    }
    ~Block() { reset(); }
    void reset() { if (ptr) Mem::release(ptr); ptr = nullptr; cap = 0; }
};

template <typename T>
using DevBuf = Block<T, DeviceMem>;

// Page-locked host memory; reads like the T * it replaces (h[i], h + k, !h).
template <typename T>
struct Pinned : Block<T, HostMem> {
    operator T *() const { return this->ptr; }
};

// An event the holder created; reads like the hipEvent_t it replaces.  Borrowed events stay plain hipEvent_t.
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(std::exchange(o.e, nullptr)) {}
    Event &operator=(Event &&o) noexcept
    {
        if (this != &o) { reset(); e = std::exchange(o.e, nullptr); }
        return *this;
    }
    ~Event() { reset(); }
    void reset() { if (e) VC_OWNED_EVENT_DESTROY(e); e = nullptr; }
    operator hipEvent_t() const { return e; }
};

}  // namespace vc
