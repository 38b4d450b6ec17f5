// Adjoint (vector-Jacobian product) of a tracking solution on gfx950 (tt_track_vjp_device).
//
// For a scalar loss L(X, U) with upstream gradient g = (gX, gU), the gradient with respect to the parameters of the
// solve comes from ONE solve with the Newton matrix K of tt_sens.hip (it is symmetric):
//   K (lam_z, lam_y) = (g, 0),   dL/dtheta = -lam' dF/dtheta,   F = (grad f + J' y - z_L + z_U, c).
// The backward sweep (tt_sens_stage.hpp: P_k, G_k, K_k as track_sens_kernel forms them, with p_k and kappa_k of the
// right-hand side g beside them) is followed by one vector sweep forward:
//   lx_0 = 0;    lu_k = -K_k lx_k + kappa_k;            lx_{k+1} = A_k lx_k + B lu_k                        k = 0 .. N-1
// and the gradients are (Q_w = D_q Q_s D_q, R_w likewise, e_k = x_k - xref_k, f_k = u_k - uref_k):
//   dL/dx_init = p_0;   dL/dxref_k = 2 Q_w lx_k;   dL/duref_k = 2 R_w lu_k;
//   dL/dwq_i = -2 sum_k ( lx_k,i (Q_s D_q e_k)_i + (Q_s D_q lx_k)_i e_k,i ),   dL/dwr_i likewise with lu, R_s, D_r, f.
//
// Mapping: one 64-lane wavefront per instance.  The pre-pass is stage-parallel and shared with track_sens_kernel
// (tt_sens_stage.hpp); lane k also brings g_k into its stage record.  The backward sweep is the shared one with its
// vector lanes switched on (lanes 48..53 carry p, lanes 54, 55 kappa): the same four barriers per stage.
// The forward sweep is six lanes and one barrier per stage.  The output phase is
// stage-parallel again, and the eight weight gradients are butterfly reductions over the lanes.
// LDS: lx_k | lu_k overlay Sigma_k (dead once the backward sweep is through) and kappa_k overlays gU_k (dead once
// kappa_k is formed), so a stage costs the sensitivity record plus g: 61.3 KB at the horizon limit, below the 64 KB a
// launch gets without asking.  Plain IEEE arithmetic, no contraction: tests/vjp_reference.py is the numpy model.
#include <math.h>

#include "tt_kernel.hpp"
#include "tt_sens_stage.hpp"

#pragma clang fp contract(off)

namespace ttmpc {
namespace {

using sens::W;
using sens::sAJ;
using sens::sSG;
using sens::d_idx;
// tiles behind the stage and gain records: P, M = P A, A, 2 Q_w, 2 R_w, two p buffers, kappa
struct Layout {
    static constexpr bool kVec = true;
    static constexpr int kStage = kVjpStage;  // the sensitivity record (24) | g: gX 6, gU 2 (then kappa) | pad
    static constexpr int sG = 24;
    static constexpr int tP = 0, tM = 36, tA = 72, tQW = 108, tRW = 144, tPV0 = 148, tPV1 = 154, tKP = 160;
};
constexpr int kStage = Layout::kStage, sG = Layout::sG, tQW = Layout::tQW, tRW = Layout::tRW;
static_assert(Layout::tKP + 2 <= kVjpTiles, "tiles");

__device__ __forceinline__ void zero_outputs(const VjpArgs& a, int b, int lane) {
    const int N = a.N, S = N + 1;
    if (a.g_x0)
        for (int t = lane; t < 6; t += W) a.g_x0[(size_t)b * 6 + t] = 0.0;
    if (a.g_xref)
        for (int t = lane; t < S * 6; t += W) a.g_xref[(size_t)b * S * 6 + t] = 0.0;
    if (a.g_uref)
        for (int t = lane; t < N * 2; t += W) a.g_uref[(size_t)b * N * 2 + t] = 0.0;
    if (a.g_wqwr)
        for (int t = lane; t < 8; t += W) a.g_wqwr[(size_t)b * 8 + t] = 0.0;
}

__device__ __forceinline__ double wave_sum(double v) {
    for (int m = W / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, W);
    return v;
}

__global__ __launch_bounds__(W) void track_vjp_kernel(VjpArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int N = a.N, S = N + 1;
    if (a.status[b] > 1) {  // > TT_ACCEPTABLE: no optimum to differentiate
        zero_outputs(a, b, lane);
        if (a.vjp_status && lane == 0) a.vjp_status[b] = 2;
        return;
    }
    double* stg = sm;                    // [S][kStage]
    double* Ks = sm + kStage * S;        // [N][2][6]
    double* T = Ks + 12 * N;             // tiles
    const double* x = a.x + (size_t)b * S * 6;
    const double* u = a.u + (size_t)b * N * 2;
    const double* dl = a.dual + (size_t)b * S * kDualPerStage;
    const double* wq = a.wqwr ? a.wqwr + (size_t)b * 8 : nullptr;
    const double* gx = a.gx ? a.gx + (size_t)b * S * 6 : nullptr;
    const double* gu = a.gu ? a.gu + (size_t)b * N * 2 : nullptr;
    const double dt = a.dt;
    bool bad = false;

    // ---- stage-parallel pre-pass ----
    for (int k = lane; k <= N; k += W) {
        double* r = stg + k * kStage;
        sens::linearise_stage(a, r, x + k * 6, u + k * 2, dl + k * kDualPerStage, k == N);
        for (int v = 0; v < 8; ++v) {
            double g = 0.0;
            if (v < 6) {
                if (gx) g = gx[k * 6 + v];
            } else if (gu && k < N) {
                g = gu[k * 2 + (v - 6)];
            }
            bad |= !isfinite(g);
            r[sG + v] = g;
        }
    }
    // ---- backward sweep (entry-parallel, p and kappa beside the matrix lanes) ----
    const sens::Roles ro(lane);
    const int pc = sens::backward_sweep<Layout>(a, ro, wq, stg, Ks, T, lane, bad);  // T[pc ..]: p_0
    // ---- forward sweep: lx_k | lu_k into the Sigma slots of stage k ----
    if (lane < 6) stg[sSG + lane] = 0.0;
    __syncthreads();
    for (int k = 0; k < N; ++k) {
        double* r = stg + k * kStage;
        if (lane < 6) {
            double lx[6];
            for (int l = 0; l < 6; ++l) lx[l] = r[sSG + l];
            double s0 = 0.0, s1 = 0.0;
            for (int l = 0; l < 6; ++l) {
                s0 += Ks[k * 12 + l] * lx[l];
                s1 += Ks[k * 12 + 6 + l] * lx[l];
            }
            const double lu0 = -s0 + r[sG + 6], lu1 = -s1 + r[sG + 7];
            double s = r[sSG + lane];  // lx_{k+1} = A lx_k + B lu_k, row `lane`
            for (int l = 0; l < 6; ++l) {
                const int di = d_idx(lane, l);
                if (di >= 0) s += r[sAJ + di] * lx[l];
            }
            if (lane == 5) s += dt * lu0;
            if (lane == 4) s += dt * lu1;
            bad |= !isfinite(s) || !isfinite(lu0) || !isfinite(lu1);
            r[kStage + sSG + lane] = s;  // stage k + 1
            if (lane < 2) r[sSG + 6 + lane] = lane == 0 ? lu0 : lu1;
        }
        __syncthreads();
    }
    if (__ballot(bad) != 0ull) {
        zero_outputs(a, b, lane);
        if (a.vjp_status && lane == 0) a.vjp_status[b] = 1;
        return;
    }
    // ---- outputs ----
    if (a.g_x0 && ro.pl) a.g_x0[(size_t)b * 6 + ro.pi] = T[pc + ro.pi];
    const double* xr = a.xref ? a.xref + (size_t)b * S * 6 : nullptr;
    const double* ur = a.uref ? a.uref + (size_t)b * N * 2 : nullptr;
    const bool wgrad = a.g_wqwr && xr && ur;
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = lane; k <= N; k += W) {
        const double* r = stg + k * kStage;
        double lx[6];
        for (int l = 0; l < 6; ++l) lx[l] = r[sSG + l];
        if (a.g_xref) {
            for (int ii = 0; ii < 6; ++ii) {
                double s = 0.0;
                for (int l = 0; l < 6; ++l) s += T[tQW + ii * 6 + l] * lx[l];
                bad |= !isfinite(s);
                a.g_xref[((size_t)b * S + k) * 6 + ii] = s;
            }
        }
        if (wgrad) {
            double e[6], de[6], dlx[6];
            for (int l = 0; l < 6; ++l) {
                const double w = wq ? wq[l] : 1.0;
                e[l] = x[k * 6 + l] - xr[k * 6 + l];
                de[l] = w * e[l];
                dlx[l] = w * lx[l];
            }
            for (int ii = 0; ii < 6; ++ii) {
                double qe = 0.0, ql = 0.0;
                for (int l = 0; l < 6; ++l) {
                    const double q = 0.5 * (a.Q[ii * 6 + l] + a.Q[l * 6 + ii]);
                    qe += q * de[l];
                    ql += q * dlx[l];
                }
                acc[ii] += lx[ii] * qe + ql * e[ii];
            }
        }
        if (k < N) {
            const double lu[2] = {r[sSG + 6], r[sSG + 7]};
            if (a.g_uref) {
                for (int ii = 0; ii < 2; ++ii) {
                    const double s = T[tRW + ii * 2 + 0] * lu[0] + T[tRW + ii * 2 + 1] * lu[1];
                    bad |= !isfinite(s);
                    a.g_uref[((size_t)b * N + k) * 2 + ii] = s;
                }
            }
            if (wgrad) {
                double f[2], df[2], dlu[2];
                for (int l = 0; l < 2; ++l) {
                    const double w = wq ? wq[6 + l] : 1.0;
                    f[l] = u[k * 2 + l] - ur[k * 2 + l];
                    df[l] = w * f[l];
                    dlu[l] = w * lu[l];
                }
                for (int ii = 0; ii < 2; ++ii) {
                    double rf = 0.0, rl = 0.0;
                    for (int l = 0; l < 2; ++l) {
                        const double q = 0.5 * (a.R[ii * 2 + l] + a.R[l * 2 + ii]);
                        rf += q * df[l];
                        rl += q * dlu[l];
                    }
                    acc[6 + ii] += lu[ii] * rf + rl * f[ii];
                }
            }
        }
    }
    if (a.g_wqwr) {
        for (int t = 0; t < 8; ++t) {
            const double s = -2.0 * wave_sum(acc[t]);
            bad |= !isfinite(s);
            if (lane == 0) a.g_wqwr[(size_t)b * 8 + t] = s;
        }
    }
    const bool late = __ballot(bad) != 0ull;  // an overflow in the output products, or a non-finite reference
    if (late) {
        __syncthreads();  // the zeros below go behind the stores above
        zero_outputs(a, b, lane);
    }
    if (a.vjp_status && lane == 0) a.vjp_status[b] = late ? 1 : 0;
}

}  // namespace

hipError_t launch_track_vjp(const VjpArgs& a, hipStream_t stream) {
    const int bytes = 8 * vjp_lds_doubles(a.N);
    if (bytes > 64 * 1024) return hipErrorInvalidValue;  // (the tracking horizon limit keeps it below 62 KB)
    hipLaunchKernelGGL(track_vjp_kernel, dim3(a.B), dim3(W), bytes, stream, a);
    return hipGetLastError();
}

}  // namespace ttmpc
