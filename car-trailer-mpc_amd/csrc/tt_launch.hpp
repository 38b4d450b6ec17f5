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

}  // namespace ttmpc
