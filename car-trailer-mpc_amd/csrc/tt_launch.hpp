// Launch helpers of the elementwise kernels (tt_sim.hip, tt_sim_vjp.hip) and the launch check the LQR pair shares.
#pragma once
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdio.h>

namespace ttmpc {

constexpr int kThreads = 256;

__host__ __device__ inline int grid_for(long long n) { return (int)((n + kThreads - 1) / kThreads); }

// 0, or -EIO with the launch error of kernel `where` on stderr
inline int launched(const char* where) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        fprintf(stderr, "ttmpc: %s launch failed: %s\n", where, hipGetErrorString(e));
        return -EIO;
    }
    return 0;
}

// A flat elementwise launch: one thread per element of n, kThreads per block, on `stream`.  0 or -EIO as launched();
// the caller has validated its arguments and dealt with an empty batch.
template <typename... P, typename... A>
inline int launch_flat(void (*kernel)(P...), const char* name, long long n, void* stream, A... args) {
    hipLaunchKernelGGL(kernel, dim3(grid_for(n)), dim3(kThreads), 0, (hipStream_t)stream, args...);
    return launched(name);
}

}  // namespace ttmpc
