// Sensitivity of a tracking solution to x_init on gfx950 (tt_solve_batch_ex, tt_track_sens_device).
//
// The Newton matrix at the returned primal-dual point and the backward Riccati sweep over it (P_k, G_k, K_k) are
// described where they live, in tt_sens_stage.hpp.  A unit perturbation of the x_0 - x_init row (sIPOPT's parametric
// step) is that sweep followed by
//   Phi_0 = I;  dU_k = -K_k Phi_k;  Phi_{k+1} = A_k Phi_k + B dU_k.
// gain = dU_0 = -K_0.
//
// Mapping: one 64-lane wavefront per instance, like the solver.  The pre-pass is stage-parallel (lane k linearises
// stage k: 3 sincos, the 9 + 7 model entries and Sigma, into LDS); the two sweeps are serial in k and entry-parallel:
// lane 6i + j owns entry (i, j) of the 6x6 tiles (P, P A, Phi), lanes 36..47 the 2x6 gain.  Everything between the
// loads and the stores lives in LDS (24 doubles per stage + 12 per gain + five tiles: 7.7 KB at N = 20).
// The arithmetic is plain IEEE (division, no contraction): the kernel is checked against a numpy model of the same
// recursion (tests/sens_reference.py) and is nowhere near the cost of a solve.
#include <math.h>

#include "tt_kernel.hpp"
#include "tt_sens_stage.hpp"

#pragma clang fp contract(off)

namespace ttmpc {
namespace {

using sens::W;
using sens::sAJ;
using sens::d_idx;
// tiles behind the stage and gain records: P, M = P A, A, two Phi buffers, 2 R_w  (sens_lds_doubles: 24 S + 12 N + 192)
struct Layout {
    static constexpr bool kVec = false;
    static constexpr int kStage = 24;  // per stage: dt*J (9) | curvature (7) | Sigma (8), tt_sens_stage.hpp
    static constexpr int tP = 0, tM = 36, tA = 72, tF0 = 108, tF1 = 144, tRW = 180;
};
constexpr int kStage = Layout::kStage, tM = Layout::tM, tF0 = Layout::tF0, tF1 = Layout::tF1;

__device__ __forceinline__ void zero_outputs(const SensArgs& a, int b, int lane) {
    const int N = a.N, S = N + 1;
    if (a.gain)
        for (int t = lane; t < 12; t += W) a.gain[(size_t)b * 12 + t] = 0.0;
    if (a.dxdx0)
        for (int t = lane; t < S * 36; t += W) a.dxdx0[(size_t)b * S * 36 + t] = 0.0;
    if (a.dudx0)
        for (int t = lane; t < N * 12; t += W) a.dudx0[(size_t)b * N * 12 + t] = 0.0;
}

__global__ __launch_bounds__(W) void track_sens_kernel(SensArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int N = a.N, S = N + 1;
    if (a.status[b] > 1) {  // > TT_ACCEPTABLE: no optimum to differentiate
        zero_outputs(a, b, lane);
        if (a.sens_status && lane == 0) a.sens_status[b] = 2;
        return;
    }
    double* stg = sm;                    // [S][kStage]
    double* Ks = sm + kStage * S;        // [N][2][6]
    double* T = Ks + 12 * N;             // tiles
    const double* x = a.x + (size_t)b * S * 6;
    const double* u = a.u + (size_t)b * N * 2;
    const double* dl = a.dual + (size_t)b * S * kDualPerStage;
    const double* wq = a.wqwr ? a.wqwr + (size_t)b * 8 : nullptr;
    const double dt = a.dt;

    // ---- stage-parallel pre-pass ----
    for (int k = lane; k <= N; k += W)
        sens::linearise_stage(a, stg + k * kStage, x + k * 6, u + k * 2, dl + k * kDualPerStage, k == N);
    // ---- backward sweep (entry-parallel) ----
    const sens::Roles ro(lane);
    const bool ent = ro.ent, gl = ro.gl;
    const int i = ro.i, j = ro.j, gr = ro.gr, gc = ro.gc;
    bool bad = false;
    sens::backward_sweep<Layout>(a, ro, wq, stg, Ks, T, lane, bad);
    if (__ballot(bad) != 0ull) {
        zero_outputs(a, b, lane);
        if (a.sens_status && lane == 0) a.sens_status[b] = 1;
        return;
    }
    if (a.gain && gl) a.gain[(size_t)b * 12 + (lane - 36)] = -Ks[lane - 36];
    // ---- forward sweep ----
    if (a.dxdx0 || a.dudx0) {
        double* dX = a.dxdx0 ? a.dxdx0 + (size_t)b * S * 36 : nullptr;
        double* dU = a.dudx0 ? a.dudx0 + (size_t)b * N * 12 : nullptr;
        if (ent) {
            T[tF0 + lane] = i == j ? 1.0 : 0.0;
            if (dX) dX[lane] = i == j ? 1.0 : 0.0;
        }
        __syncthreads();
        int cur = tF0, nxt = tF1;
        for (int k = 0; k < N; ++k) {
            const double* r = stg + k * kStage;
            if (gl) {  // dU_k = -K_k Phi_k  (kept in the M tile for the lanes of rows 4, 5)
                double s = 0.0;
                for (int l = 0; l < 6; ++l) s += Ks[k * 12 + gr * 6 + l] * T[cur + l * 6 + gc];
                s = -s;
                bad |= !isfinite(s);
                T[tM + gr * 6 + gc] = s;
                if (dU) dU[k * 12 + gr * 6 + gc] = s;
            }
            __syncthreads();
            if (ent) {  // Phi_{k+1} = A_k Phi_k + B dU_k
                double s = T[cur + lane];
                for (int l = 0; l < 6; ++l) {
                    const int di = d_idx(i, l);
                    if (di >= 0) s += r[sAJ + di] * T[cur + l * 6 + j];
                }
                if (i == 5) s += dt * T[tM + j];
                if (i == 4) s += dt * T[tM + 6 + j];
                bad |= !isfinite(s);
                T[nxt + lane] = s;
                if (dX) dX[(k + 1) * 36 + lane] = s;
            }
            __syncthreads();
            const int t = cur; cur = nxt; nxt = t;
        }
        if (__ballot(bad) != 0ull) {
            zero_outputs(a, b, lane);
            if (a.sens_status && lane == 0) a.sens_status[b] = 1;
            return;
        }
    }
    if (a.sens_status && lane == 0) a.sens_status[b] = 0;
}

}  // namespace

hipError_t launch_track_sens(const SensArgs& a, hipStream_t stream) {
    const int bytes = 8 * sens_lds_doubles(a.N);
    if (bytes > 64 * 1024) return hipErrorInvalidValue;  // (the tracking horizon limit keeps it below 52 KB)
    hipLaunchKernelGGL(track_sens_kernel, dim3(a.B), dim3(W), bytes, stream, a);
    return hipGetLastError();
}

}  // namespace ttmpc
