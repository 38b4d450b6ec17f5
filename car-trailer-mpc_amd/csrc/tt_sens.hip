// Sensitivity of a tracking solution to x_init on gfx950 (tt_solve_batch_ex, tt_track_sens_device).
//
// At the returned primal-dual point (x, u, y, z_L, z_U) of the tracking NLP (tt_track.hip) the Newton matrix of the
// barrier problem with the bound multipliers eliminated is the KKT matrix of an equality-constrained LQ problem:
//   stage Hessians  W_k + Sigma_x,k  (states)  and  R_k = 2 R_w + Sigma_u,k  (inputs),
//     W_k = 2 Q_w - dt sum_i y_{k+1,i} d2f_i/dx2 (x_k)  (k < N; the 7 curvature entries of tt_track.hip),  W_N = 2 Q_w,
//     Sigma = z_L / (v - lb) + z_U / (ub - v) with the relaxed bounds of the solver,
//   dynamics  dx_{k+1} = A_k dx_k + B du_k,  A_k = I + dt J_f(x_k),  B = dt B_F  (B[5][0] = B[4][1] = dt).
// A unit perturbation of the x_0 - x_init row (sIPOPT's parametric step) is therefore one un-iterated, un-regularised
// Riccati pass:
//   P_N = W_N + Sigma_x,N;  G_k = R_k + B' P_{k+1} B;  K_k = G_k^-1 B' P_{k+1} A_k;
//   P_k = W_k + Sigma_x,k + A_k' P_{k+1} (A_k - B K_k)            (P_0 is not needed: x_0 is pinned)
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
using sens::sWC;
using sens::sSG;
using sens::d_idx;
using sens::w_idx;
constexpr int kStage = 24;  // per stage: dt*J (9) | curvature (7) | Sigma (8), tt_sens_stage.hpp
// tiles behind the stage and gain records: P, M = P A, A, two Phi buffers, 2 R_w  (sens_lds_doubles: 24 S + 12 N + 192)
constexpr int tP = 0, tM = 36, tA = 72, tF0 = 108, tF1 = 144, tRW = 180;

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
    // ---- entry-parallel roles ----
    const bool ent = lane < 36, gl = lane >= 36 && lane < 48;
    const int i = ent ? lane / 6 : 0, j = ent ? lane % 6 : 0;
    const int gr = gl ? (lane - 36) / 6 : 0, gc = gl ? (lane - 36) % 6 : 0;
    const int wi = w_idx(i, j);
    double q2 = 0.0;  // 2 Q_w (i, j)
    if (ent) {
        const double q = 0.5 * (a.Q[i * 6 + j] + a.Q[j * 6 + i]);
        q2 = 2.0 * (wq ? q * wq[i] * wq[j] : q);
    }
    if (lane < 4) {  // 2 R_w
        const int ri = lane / 2, rj = lane % 2;
        const double rr = 0.5 * (a.R[ri * 2 + rj] + a.R[rj * 2 + ri]);
        T[tRW + lane] = 2.0 * (wq ? rr * wq[6 + ri] * wq[6 + rj] : rr);
    }
    __syncthreads();
    bool bad = false;
    if (ent) {
        const double p = q2 + (i == j ? stg[N * kStage + sSG + i] : 0.0);
        T[tP + lane] = p;
        bad |= !isfinite(p);
    }
    __syncthreads();
    // ---- backward sweep ----
    for (int k = N - 1; k >= 0; --k) {
        const double* r = stg + k * kStage;
        if (ent) {
            const int di = d_idx(i, j);
            T[tA + lane] = (i == j ? 1.0 : 0.0) + (di >= 0 ? r[sAJ + di] : 0.0);
        }
        __syncthreads();
        if (ent) {  // M = P A
            double m = 0.0;
            for (int l = 0; l < 6; ++l) m += T[tP + i * 6 + l] * T[tA + l * 6 + j];
            T[tM + lane] = m;
        }
        __syncthreads();
        if (gl) {  // K = G^-1 B' M, G = R_k + B' P B
            const double g00 = T[tRW + 0] + r[sSG + 6] + dt * dt * T[tP + 5 * 6 + 5];
            const double g01 = T[tRW + 1] + dt * dt * T[tP + 5 * 6 + 4];
            const double g11 = T[tRW + 3] + r[sSG + 7] + dt * dt * T[tP + 4 * 6 + 4];
            const double det = g00 * g11 - g01 * g01;
            const double h0 = dt * T[tM + 5 * 6 + gc], h1 = dt * T[tM + 4 * 6 + gc];
            const double kv = gr == 0 ? (g11 * h0 - g01 * h1) / det : (g00 * h1 - g01 * h0) / det;
            if (!(g00 > 0.0) || !(det > 0.0) || !isfinite(g00) || !isfinite(det) || !isfinite(kv)) bad = true;
            Ks[k * 12 + gr * 6 + gc] = kv;
        }
        __syncthreads();
        if (ent && k > 0) {  // P_k = W_k + Sigma_x + A' M - H' K,  H = B' M
            double p = q2 + (wi >= 0 ? r[sWC + wi] : 0.0) + (i == j ? r[sSG + i] : 0.0);
            double am = 0.0;
            for (int l = 0; l < 6; ++l) am += T[tA + l * 6 + i] * T[tM + l * 6 + j];
            const double hk = dt * T[tM + 5 * 6 + i] * Ks[k * 12 + j] + dt * T[tM + 4 * 6 + i] * Ks[k * 12 + 6 + j];
            p = p + (am - hk);
            bad |= !isfinite(p);
            T[tP + lane] = p;  // (the reads of P of this stage are behind the barriers above)
        }
        __syncthreads();
    }
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
