// owned.h -- the one owner of a resource that a plain function releases (device memory, pinned memory: devmem.h).
// Nothing of HIP in here: host/selftest.cpp checks the semantics on malloc'ed blocks under sanitizers.
#pragma once
#include <stddef.h>

namespace cm {

// Move-only owner of a T * that Free releases.  It converts to T * implicitly, so kernel launches and pointer arithmetic
// read as with a raw pointer; it has no copy, so a struct that holds one cannot be passed to a kernel by value.
template <typename T, void (*Free)(void *)>
class Owned {
public:
    Owned() = default;
    Owned(Owned &&o) noexcept : p_(o.release()) {}
    Owned &operator=(Owned &&o) noexcept
    {
        if (this != &o) adopt(o.release());      // frees the old contents here, not earlier
        return *this;
    }
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { reset(); }

    void reset()
    {
        if (p_) Free((void *)p_);
        p_ = nullptr;
    }
    T *release()
    {
        T *p = p_;
        p_ = nullptr;
        return p;
    }
    void adopt(T *p)
    {
        if (p == p_) return;
        reset();
        p_ = p;
    }
    T *get() const { return p_; }
    operator T *() const { return p_; }

protected:
    T *p_ = nullptr;
};

}  // namespace cm
