// nm_host.inc -- host-side plumbing shared by every translation unit of libnmhip.so: the argument checks the launches
// have in common, the one place a kernel is launched from, and the read-out of a __device__ counter array.
#pragma once
#include <hip/hip_runtime.h>
#include "nmhip.h"

namespace {

// Launch `kernel`, raising its dynamic-LDS limit first when it uses dynamic LDS (on every launch: nothing is remembered
// between calls).  Returns the attribute's error, else the launch's (NM_OK = hipSuccess = 0).
template <typename... P, typename... A>
inline int launch_kernel(void (*kernel)(P...), dim3 grid, dim3 block, int lds_bytes, void* stream, A... args) {
  if (lds_bytes > 0) {
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, (hipStream_t)stream, args...);
  return (int)hipGetLastError();
}

// What the launches over (job, tile) grids check alike: the descriptor array, n_jobs / n_tiles / n_steps >= 1, `first`
// (the first step or tile, or the smaller of both) >= 0, and that several tiles run forward only -- concurrent tiles of
// one job share its parameters, moments and gradient buffer.
inline int check_launch_geometry(const void* jobs_dev, int n_jobs, int n_tiles, int n_steps, int first, int flags) {
  if (!jobs_dev) return NM_E_NULL;
  if (n_jobs < 1 || n_tiles < 1 || n_steps < 1 || first < 0) return NM_E_GEOMETRY;
  if (n_tiles > 1 && (flags & (NM_F_BACKWARD | NM_F_ADAM | NM_F_GRADS))) return NM_E_GEOMETRY;
  return NM_OK;
}

// Compute units of the current device; 0 if the runtime cannot tell.  A launch whose workgroups wait for each other
// must be resident at once: one workgroup per CU (LDS), so at most this many.
inline int cu_count() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return 0;
  return cus;
}

// Copy a __device__ array of counters to `out` (as many bytes as the symbol has); reset != 0 zeroes it afterwards.
template <typename T>
inline int read_counters(unsigned long long* out, const T& symbol, int reset) {
  if (!out) return NM_E_NULL;
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(symbol), sizeof(T));
  if (e != hipSuccess) return (int)e;
  if (reset) {
    static const T zeros = {};
    e = hipMemcpyToSymbol(HIP_SYMBOL(symbol), zeros, sizeof(T));
  }
  return (int)e;
}

}  // namespace
