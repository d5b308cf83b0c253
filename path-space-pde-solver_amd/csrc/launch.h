// The one launch point of the library: every kernel of csrc/ is enqueued through launch<> or launch_lds<>, with the kernel as
// a template argument, so an instantiation is named once per site.  launch_lds<> raises the kernel's dynamic-LDS limit to the
// launch's own byte count first -- on every launch, nothing is cached.  Stands alone: the HIP runtime is all it needs.
#pragma once
#include <hip/hip_runtime.h>

namespace psp {

template <auto Kernel, typename... Args>
inline hipError_t launch(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s, const Args&... args) {
    hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, s, args...);
    return hipGetLastError();
}

template <auto Kernel, typename... Args>
inline hipError_t launch_lds(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s, const Args&... args) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    return e != hipSuccess ? e : launch<Kernel>(grid, block, lds_bytes, s, args...);
}

}  // namespace psp
