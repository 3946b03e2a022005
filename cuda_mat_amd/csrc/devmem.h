// devmem.h -- the one allocator of device memory and the owners of device and pinned memory (owned.h).  Part of common.h,
// which includes it after the declarations used here: include common.h, not this file.
#pragma once
#include "owned.h"

namespace cm {

// `count` elements of device memory (one for count == 0).  Out of memory keeps its own code: the retries of dropin.hip and
// many_room key on it.
template <typename T>
int dev_alloc(T **p, size_t count)
{
    *p = nullptr;
    hipError_t e = hipMalloc((void **)p, sizeof(T) * (count ? count : 1));
    if (e != hipSuccess) {
        set_error("hipMalloc(%zu bytes) failed: %s", sizeof(T) * count, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? CUDAMAT_ERR_NOMEM : CUDAMAT_ERR_HIP;
    }
    return CUDAMAT_OK;
}

// the pooled free (pool.cpp): a device-wide synchronisation point like the runtime's own; a failure has no remedy
inline void dev_free(void *p) { CM_DROP(hipFree(p)); }
inline void pinned_free(void *p) { CM_DROP(hipHostFree(p)); }

template <typename T>
struct DevBuf : Owned<T, dev_free> {
    int alloc(size_t count)
    {
        this->reset();
        return dev_alloc(&this->p_, count);
    }
};
template <typename T>
using PinnedBuf = Owned<T, pinned_free>;

}  // namespace cm
