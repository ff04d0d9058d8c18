// Owning handles for what the HIP runtime hands out: device buffers, pinned host buffers, events.  Host code only.
// One move-only template; the release function is a template argument, so a handle is one pointer wide and a struct of
// handles releases everything it holds, once, wherever it goes out of scope.  hipFree waits for the whole device: a handle
// frees exactly where its owner dies, is reset() or is alloc()'d again -- arrays that solves in flight may still read are
// release()d into a list that dies later (ipc_engine::retired).
// A handle converts to T* so that call sites read as they did with raw pointers -- which also lets hipFree(handle) and
// hipEventDestroy(handle) compile: never release by hand what a handle holds, it would be released twice.
#pragma once
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstddef>

namespace ipc {

// live objects of the process by kind (ipc_debug_live_resources)
inline std::atomic<int> g_live_devbufs{0}, g_live_pinned{0}, g_live_events{0};

template <class T, auto Release, std::atomic<int>& Live>
class Owned {
public:
    Owned() = default;
    explicit Owned(T* p) : p_(p) { if (p_) ++Live; }
    Owned(Owned&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    Owned& operator=(Owned&& o) noexcept
    {
        if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; }
        return *this;
    }
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned() { reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
    void reset(T* p = nullptr)
    {
        if (p_) { Release(p_); --Live; }
        p_ = p;
        if (p_) ++Live;
    }
    T* release()                                       // gives the pointer up: the caller owns it now
    {
        T* p = p_;
        if (p_) --Live;
        p_ = nullptr;
        return p;
    }

protected:
    template <class Make>
    hipError_t acquire(Make&& make)                    // frees what the handle holds, then make(&p); on an error the handle is empty
    {
        reset();
        T* p = nullptr;
        const hipError_t e = make(&p);
        if (e == hipSuccess) reset(p);
        return e;
    }

private:
    T* p_ = nullptr;
};

template <class T>
struct DevBuf : Owned<T, hipFree, g_live_devbufs> {
    using Owned<T, hipFree, g_live_devbufs>::Owned;
    hipError_t alloc(size_t count) { return this->acquire([&](T** p) { return hipMalloc(p, sizeof(T) * count); }); }
};

template <class T>
struct PinnedBuf : Owned<T, hipHostFree, g_live_pinned> {
    using Owned<T, hipHostFree, g_live_pinned>::Owned;
    hipError_t alloc(size_t count, unsigned flags = hipHostMallocDefault) { return this->acquire([&](T** p) { return hipHostMalloc(p, sizeof(T) * count, flags); }); }
};

struct Event : Owned<ihipEvent_t, hipEventDestroy, g_live_events> {
    using Owned<ihipEvent_t, hipEventDestroy, g_live_events>::Owned;
    hipError_t create(unsigned flags = hipEventDefault) { return acquire([&](hipEvent_t* ev) { return hipEventCreateWithFlags(ev, flags); }); }
};

// Scratch buffers that grow together, and the capacity they were sized for: the capacity stands next to its members in one
// struct and every growth names them all,
//     HIPCHK(g.cap.grow(need, sized(g.a, need), sized(g.b, need + 1)));
// Nothing is allocated or freed while need <= capacity.  A growth releases every member before it allocates the first (the
// contents are scratch and are not kept) and the capacity reads 0 until the last member is there: after a failure part way the
// next call grows again from scratch.  Sub-arrays of one member are cut at the capacity (part), never at the need of a call.
// A member is anything with reset() and alloc(count) -> hipError_t -- which a ScratchCap is itself: a group with a second
// capacity, in another unit, lists that one as its last member.
template <class Buf>
struct Sized { Buf& buf; size_t count; };
template <class Buf>
Sized<Buf> sized(Buf& buf, size_t count) { return {buf, count}; }

class ScratchCap {
public:
    size_t size() const { return cap_; }
    template <class... Buf>
    hipError_t grow(size_t need, Sized<Buf>... members) { return need <= cap_ ? hipSuccess : regrow(need, members...); }
    template <class... Buf>
    hipError_t regrow(size_t cap, Sized<Buf>... members)           // whatever it holds: for a caller with a growth rule of its own
    {
        cap_ = 0;
        (members.buf.reset(), ...);
        hipError_t e = hipSuccess;
        (void)(((e = members.buf.alloc(members.count)) == hipSuccess) && ...);
        if (e == hipSuccess) cap_ = cap;
        return e;
    }
    template <class Buf>
    auto part(const Buf& buf, size_t k) const { return buf.get() + k * cap_; }     // the k-th sub-array of `buf`, [parts][capacity]

    void reset() { cap_ = 0; }
    hipError_t alloc(size_t count) { cap_ = count; return hipSuccess; }

private:
    size_t cap_ = 0;
};

}  // namespace ipc
