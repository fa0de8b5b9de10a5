// resource.h -- move-only owners of the runtime's HIP resources.  Each frees
// its handle exactly once, when it is reset or destroyed, and converts
// implicitly to the raw handle, so launch sites read c->X, c->stream.  The
// only place of the runtime that frees a buffer or destroys an event or stream.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace svgd_amd {

template <class H, hipError_t (*Free)(H)> class Owned {
  public:
    Owned() = default;
    Owned(Owned &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Owned &operator=(Owned &&o) noexcept
    {
        if (this != &o) {
            reset();
            h_ = o.h_;
            o.h_ = nullptr;
        }
        return *this;
    }
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { reset(); }
    operator H() const { return h_; }
    void reset()
    {
        if (h_) (void)Free(h_);
        h_ = nullptr;
    }

  protected:
    H h_ = nullptr;
};

template <class T> hipError_t free_device(T *p) { return hipFree((void *)p); }
template <class T> hipError_t free_pinned(T *p) { return hipHostFree((void *)p); }

// `count` elements of device memory (contents undefined; svgd_ctx's dalloc zeroes)
template <class T> struct DevBuf : Owned<T *, free_device<T>> {
    hipError_t alloc(size_t count)
    {
        this->reset();
        return hipMalloc((void **)&this->h_, sizeof(T) * count);
    }
};

// `count` elements of pinned host memory (flags: hipHostMallocDefault / Coherent)
template <class T> struct HostBuf : Owned<T *, free_pinned<T>> {
    hipError_t alloc(size_t count, unsigned flags)
    {
        this->reset();
        return hipHostMalloc((void **)&this->h_, sizeof(T) * count, flags);
    }
};

struct Event : Owned<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags = hipEventDefault)
    {
        reset();
        return hipEventCreateWithFlags(&h_, flags);
    }
};

struct Stream : Owned<hipStream_t, hipStreamDestroy> {
    hipError_t create() // (non-blocking: never ordered against the null stream)
    {
        reset();
        return hipStreamCreateWithFlags(&h_, hipStreamNonBlocking);
    }
};

// The timing events of a context: the pool creates every one, lends plain
// handles (take) and takes them back (give); each is destroyed once, with
// the pool, whoever holds its handle then.
class EventPool {
  public:
    hipEvent_t take()
    {
        if (free_.empty()) {
            all_.emplace_back();
            (void)all_.back().create();
            return all_.back();
        }
        hipEvent_t e = free_.back();
        free_.pop_back();
        return e;
    }
    void give(hipEvent_t e) { free_.push_back(e); }

  private:
    std::vector<Event> all_;
    std::vector<hipEvent_t> free_;
};

} // namespace svgd_amd
