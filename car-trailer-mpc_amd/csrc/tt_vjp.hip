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
//
// The model instantiation (tt_track_vjp_model_device, kModel) adds the gradient in the geometry theta = (L1, L2, Mh).
// Only the dynamics rows and the -A_k' y_{k+1} part of the stationarity rows depend on theta:
//   dL/dtheta = dt sum_{k<N} [ lx_k' (dJ_f(x_k)/dtheta)' y_{k+1} + ly_{k+1}' df(x_k, u_k)/dtheta ]
// and lam_y comes from the x-rows of K, one more six-lane sweep (model_gradient below): ly_N = gX_N - H_N lx_N,
// ly_k = gX_k - H_k lx_k + A_k' ly_{k+1}, H_k = W_k + Sigma_x,k.  ly overlays gX, so the LDS record is the same; the
// plain instantiation's code is what it was.  tests/model_vjp_reference.py is the numpy model.
//
// The bounds instantiations (tt_track_vjp_bounds_device, kBounds, with or without kModel) add the gradient in the box
// (xlb, xub, ulb, uub).  The bounds enter F only through z_L = mu / (v - l_rel) and z_U = mu / (u_rel - v), so
//   dL/dl_v = rho_l sum_k Sigma_L,k,v lam_k,v,   dL/du_v = rho_u sum_k Sigma_U,k,v lam_k,v,
// Sigma_L = z_L / (v - l_rel) and Sigma_U = z_U / (u_rel - v) the two halves of linearise_stage's Sigma, lam the
// lam_x | lam_u of the forward sweep, rho the derivative of the bound relaxation (bounds_gradient below).  One more
// stage-parallel pass and sixteen butterflies; nothing new in LDS.  tests/bounds_vjp_reference.py is the numpy model.
#include <math.h>

#include <type_traits>

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

// g_model of an instance that gives no gradient: zeros, or with `accumulate` the accumulator as it is
__device__ __forceinline__ void zero_model(const VjpModelArgs& a, int b, int lane) {
    if (!a.accumulate && lane < 3) a.g_model[(size_t)b * 3 + lane] = 0.0;
}

// Sigma_x,k entry v (< 6) again, with linearise_stage's own expressions: lam_x | lam_u have overwritten the record's
__device__ __forceinline__ double sigma_x(const DiffArgs& a, double val, const double* dk, int v) {
    double sg = 0.0;
    const double l = a.xlb[v], ub = a.xub[v];
    if (isfinite(l) && l > -1e19) sg += dk[6 + v] / (val - (l - 1e-8 * fmax(1.0, fabs(l))));
    if (isfinite(ub) && ub < 1e19) sg += dk[14 + v] / ((ub + 1e-8 * fmax(1.0, fabs(ub))) - val);
    return sg;
}

// The model instantiation's three phases, behind the forward sweep (the record holds lam_x | lam_u in the Sigma slots,
// gX in sG .. sG + 5, dt*J and the curvature untouched; T[tQW ..] = 2 Q_w):
//   1. stage-parallel: r_k = gX_k - H_k lam_x,k over gX_k,  H_k = 2 Q_w + curvature_k (k < N) + Sigma_x,k
//   2. serial, six lanes, one barrier per stage: lam_y,k = r_k + A_k' lam_y,k+1 in place, k = N - 1 .. 0
//   3. stage-parallel: lane k < N forms lam_x,k' (dJ_f/dtheta)' y_{k+1} + lam_y,k+1' df/dtheta for theta = L1, L2, Mh;
//      three butterflies, every lane leaves with dt * sum in m[]
__device__ __forceinline__ void model_gradient(const DiffArgs& a, double* stg, const double* T, const double* x,
                                               const double* dl, int lane, bool& bad, double* m) {
    const int N = a.N;
    for (int k = lane; k <= N; k += W) {
        double* r = stg + k * kStage;
        const double* xk = x + k * 6;
        const double* dk = dl + k * kDualPerStage;
        double lx[6], h[6];
        for (int l = 0; l < 6; ++l) lx[l] = r[sSG + l];
        for (int i = 0; i < 6; ++i) {
            double s = 0.0;
            for (int l = 0; l < 6; ++l) s += T[tQW + i * 6 + l] * lx[l];
            if (k < N)
                for (int l = 0; l < 6; ++l) {
                    const int wi = sens::w_idx(i, l);
                    if (wi >= 0) s += r[sens::sWC + wi] * lx[l];
                }
            h[i] = s + sigma_x(a, xk[i], dk, i) * lx[i];
        }
        for (int i = 0; i < 6; ++i) {
            const double v = r[sG + i] - h[i];
            bad |= !isfinite(v);
            r[sG + i] = v;
        }
    }
    __syncthreads();
    for (int k = N - 1; k >= 0; --k) {
        double* r = stg + k * kStage;
        if (lane < 6) {
            const double* ln = r + kStage + sG;  // lam_y,k+1
            double s = ln[lane];
            for (int l = 0; l < 6; ++l) {
                const int di = d_idx(l, lane);
                if (di >= 0) s += r[sAJ + di] * ln[l];
            }
            s = r[sG + lane] + s;
            bad |= !isfinite(s);
            r[sG + lane] = s;
        }
        __syncthreads();
    }
    const double iL1 = 1.0 / a.L1, iL2 = 1.0 / a.L2, iL1L2 = iL1 * iL2, Mh = a.Mh;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int k = lane; k < N; k += W) {
        const double* r = stg + k * kStage;
        const double* xk = x + k * 6;
        const double* y = dl + (k + 1) * kDualPerStage;  // y_{k+1}
        const double* ly = r + kStage + sG;               // lam_y,k+1
        const double lx3 = r[sSG + 3], lx4 = r[sSG + 4], lx5 = r[sSG + 5];
        double sps, cps, sph, cph;
        sincos(xk[3], &sps, &cps);
        sincos(xk[4], &sph, &cph);
        const double v = xk[5], ic = 1.0 / cph, t = sph * ic, c2 = ic * ic;
        const double kk = 1.0 + Mh * iL2 * cps;
        // rows 2 and 3 of f and the entries (2,4) (2,5) (3,3) (3,4) (3,5) of J_f, differentiated
        const double y2 = y[2], y3 = y[3], l2 = ly[2], l3 = ly[3];
        const double a24 = v * c2 * iL1, a25 = t * iL1, vt = v * t * iL1;
        acc[0] += y2 * (-(a24 * iL1) * lx4 + -(a25 * iL1) * lx5)
                + y3 * (-(vt * Mh * sps * iL1L2) * lx3 + (a24 * kk * iL1) * lx4 + (a25 * kk * iL1) * lx5)
                + (l2 * -(vt * iL1) + l3 * (vt * kk * iL1));
        const double mc = Mh * cps * iL2 * iL2, s2 = sps * iL2 * iL2;
        acc[1] += y3 * ((v * cps * iL2 * iL2 - vt * Mh * sps * iL2 * iL2) * lx3 + (a24 * mc) * lx4 + (a25 * mc + s2) * lx5)
                + l3 * (vt * mc + v * s2);
        acc[2] += y3 * ((vt * sps * iL2) * lx3 + -(a24 * cps * iL2) * lx4 + -(a25 * cps * iL2) * lx5)
                + l3 * -(vt * cps * iL2);
    }
    for (int t = 0; t < 3; ++t) {
        m[t] = a.dt * wave_sum(acc[t]);
        bad |= !isfinite(m[t]);
    }
}

// g_bounds of an instance that gives no gradient: zeros, or with `accumulate` the accumulator as it is
__device__ __forceinline__ void zero_bounds(const VjpBoundsArgs& a, int b, int lane) {
    if (!a.accumulate && lane < 16) a.g_bounds[(size_t)b * 16 + lane] = 0.0;
}

// The bounds instantiations' phase, behind the forward sweep (the record holds lam_x | lam_u in the Sigma slots), stage-
// parallel: lane k forms Sigma_L,k,v lam_k,v rho_l and Sigma_U,k,v lam_k,v rho_u of its stages, Sigma_L and Sigma_U
// again with linearise_stage's own expressions, rho = d(relaxed bound)/d(bound).  A bound the kernel takes as infinite
// adds nothing (exactly 0).  The states of stage 0 are skipped: x_0 is pinned to x_init and may sit on or beyond a
// relaxed bound (lam_x,0 = 0, but Sigma is inf or negative there); the last stage has no inputs.  Sixteen butterflies;
// lane t < 16 leaves with entry t (lower bounds of x 6, u 2, then the upper bounds) in the return value.
__device__ __forceinline__ double bounds_gradient(const DiffArgs& a, const double* stg, const double* x, const double* u,
                                                  const double* dl, int lane, bool& bad) {
    const int N = a.N;
    double acc[16] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = lane; k <= N; k += W) {
        const double* r = stg + k * kStage;
        const double* dk = dl + k * kDualPerStage;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            if (v < 6 ? k == 0 : k == N) continue;
            const double lam = r[sSG + v];
            const double val = v < 6 ? x[k * 6 + v] : u[k * 2 + (v - 6)];
            const double l = v < 6 ? a.xlb[v] : a.ulb[v - 6], ub = v < 6 ? a.xub[v] : a.uub[v - 6];
            if (isfinite(l) && l > -1e19) {
                const double sg = dk[6 + v] / (val - (l - 1e-8 * fmax(1.0, fabs(l))));
                const double rho = fabs(l) > 1.0 ? 1.0 - (l > 0.0 ? 1e-8 : -1e-8) : 1.0;
                acc[v] += sg * lam * rho;
            }
            if (isfinite(ub) && ub < 1e19) {
                const double sg = dk[14 + v] / ((ub + 1e-8 * fmax(1.0, fabs(ub))) - val);
                const double rho = fabs(ub) > 1.0 ? 1.0 + (ub > 0.0 ? 1e-8 : -1e-8) : 1.0;
                acc[8 + v] += sg * lam * rho;
            }
        }
    }
    double mine = 0.0;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const double s = wave_sum(acc[t]);
        bad |= !isfinite(s);
        if (lane == t) mine = s;
    }
    return mine;
}

template <bool kModel, bool kBounds>
struct KernelArgs {
    using type = std::conditional_t<kBounds, VjpBoundsArgs, std::conditional_t<kModel, VjpModelArgs, VjpArgs>>;
};

// kModel: also dL/d(L1, L2, Mh) into a.g_model (VjpModelArgs); kBounds: also dL/d(bounds) into a.g_bounds
// (VjpBoundsArgs).  The plain instantiation is the kernel as it was
template <bool kModel, bool kBounds = false>
__global__ __launch_bounds__(W) void track_vjp_kernel(typename KernelArgs<kModel, kBounds>::type a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int N = a.N, S = N + 1;
    if (a.status[b] > 1) {  // > TT_ACCEPTABLE: no optimum to differentiate
        zero_outputs(a, b, lane);
        if constexpr (kModel) zero_model(a, b, lane);
        if constexpr (kBounds) zero_bounds(a, b, lane);
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
        if constexpr (kModel) zero_model(a, b, lane);
        if constexpr (kBounds) zero_bounds(a, b, lane);
        if (a.vjp_status && lane == 0) a.vjp_status[b] = 1;
        return;
    }
    // ---- model geometry: lam_y over gX, then the stage sums (p_0 stays in T, lam_x | lam_u in the records) ----
    double gm[3] = {0.0, 0.0, 0.0};
    if constexpr (kModel) model_gradient(a, stg, T, x, dl, lane, bad, gm);
    // ---- bounds: the stage sums of Sigma_L lam and Sigma_U lam (entry `lane` of the sixteen in lanes 0 .. 15) ----
    double gb = 0.0;
    if constexpr (kBounds) gb = bounds_gradient(a, stg, x, u, dl, lane, bad);
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
    if constexpr (kModel) {  // one writer per instance: lanes 0 .. 2 of its only wavefront
        if (late) {
            zero_model(a, b, lane);
        } else if (lane < 3) {
            double* g = a.g_model + (size_t)b * 3 + lane;
            const double v = lane == 0 ? gm[0] : lane == 1 ? gm[1] : gm[2];
            *g = a.accumulate ? *g + v : v;
        }
    }
    if constexpr (kBounds) {  // one writer per instance: lanes 0 .. 15 of its only wavefront
        if (late) {
            zero_bounds(a, b, lane);
        } else if (lane < 16) {
            double* g = a.g_bounds + (size_t)b * 16 + lane;
            *g = a.accumulate ? *g + gb : gb;
        }
    }
    if (a.vjp_status && lane == 0) a.vjp_status[b] = late ? 1 : 0;
}

}  // namespace

hipError_t launch_track_vjp(const VjpArgs& a, hipStream_t stream) {
    const int bytes = 8 * vjp_lds_doubles(a.N);
    if (bytes > 64 * 1024) return hipErrorInvalidValue;  // (the tracking horizon limit keeps it below 62 KB)
    hipLaunchKernelGGL(track_vjp_kernel<false>, dim3(a.B), dim3(W), bytes, stream, a);
    return hipGetLastError();
}

hipError_t launch_track_vjp_model(const VjpModelArgs& a, hipStream_t stream) {
    const int bytes = 8 * vjp_lds_doubles(a.N);  // the same record: lam_y overlays gX
    if (bytes > 64 * 1024 || !a.g_model) return hipErrorInvalidValue;
    hipLaunchKernelGGL(track_vjp_kernel<true>, dim3(a.B), dim3(W), bytes, stream, a);
    return hipGetLastError();
}

hipError_t launch_track_vjp_bounds(const VjpBoundsArgs& a, hipStream_t stream) {
    const int bytes = 8 * vjp_lds_doubles(a.N);  // the same record: nothing of the bounds gradient lives in LDS
    if (bytes > 64 * 1024 || !a.g_bounds) return hipErrorInvalidValue;
    if (a.g_model)
        hipLaunchKernelGGL((track_vjp_kernel<true, true>), dim3(a.B), dim3(W), bytes, stream, a);
    else
        hipLaunchKernelGGL((track_vjp_kernel<false, true>), dim3(a.B), dim3(W), bytes, stream, a);
    return hipGetLastError();
}

}  // namespace ttmpc
