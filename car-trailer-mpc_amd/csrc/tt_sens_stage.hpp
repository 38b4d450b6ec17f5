// What track_sens_kernel (tt_sens.hip) and track_vjp_kernel (tt_vjp.hip) share: the head of a stage record in LDS
// (dt*J 9 | curvature 7 | Sigma 8), the lane that linearises one stage into it, the sparsity maps of dt*J and of the
// curvature, the lane roles of the serial sweeps and the backward Riccati sweep itself.  Both kernels differentiate
// at the same primal-dual point, so they read the same Newton matrix.
//
// At the returned primal-dual point (x, u, y, z_L, z_U) of the tracking NLP (tt_track.hip) the Newton matrix of the
// barrier problem with the bound multipliers eliminated is the KKT matrix of an equality-constrained LQ problem:
//   stage Hessians  W_k + Sigma_x,k  (states)  and  R_k = 2 R_w + Sigma_u,k  (inputs),
//     W_k = 2 Q_w - dt sum_i y_{k+1,i} d2f_i/dx2 (x_k)  (k < N; the 7 curvature entries of tt_track.hip),  W_N = 2 Q_w,
//     Sigma = z_L / (v - lb) + z_U / (ub - v) with the relaxed bounds of the solver,
//   dynamics  dx_{k+1} = A_k dx_k + B du_k,  A_k = I + dt J_f(x_k),  B = dt B_F  (B[5][0] = B[4][1] = dt).
// backward_sweep is one un-iterated, un-regularised Riccati pass over it:
//   P_N = W_N + Sigma_x,N;  G_k = R_k + B' P_{k+1} B;  K_k = G_k^-1 B' P_{k+1} A_k;
//   P_k = W_k + Sigma_x,k + A_k' P_{k+1} (A_k - B K_k)            (P_0 is not needed: x_0 is pinned)
// and, for the adjoint (L::kVec), the right-hand side g = (gX, gU) beside it:
//   p_N = gX_N;  kappa_k = G_k^-1 (gU_k + B' p_{k+1});  p_k = gX_k + A_k' (p_{k+1} - P_{k+1} B kappa_k)
// Serial in k and entry-parallel: lane 6i + j owns entry (i, j) of the 6x6 tiles (P, M = P A, A), lanes 36..47 the 2x6
// gain, lanes 48..53 p and lanes 54, 55 kappa.  Four barriers per stage with or without the vector lanes: kappa's
// division runs beside K's, and p_k is formed beside P_k as gX_k + A' p_{k+1} - (B' M)' kappa (A' P B = M' B because P
// is symmetric).  Plain IEEE arithmetic (division, no contraction).
//
// A layout that has a member sDH adds a dense symmetric 4x4 block r[sDH + 4 i + j] to the pose entries (i, j < 4:
// X, Y, theta, psi) of every stage Hessian: the eliminated OBCA blocks of tt_obca_vjp.hip.  Layouts without it compile
// to the code they compiled to before.  With the addend the 2x2 solves with G_k eliminate on the larger diagonal.
#pragma once
#include <math.h>

#include <type_traits>

#include "tt_kernel.hpp"

#pragma clang fp contract(off)

namespace ttmpc {
namespace sens {

constexpr int W = 64;
constexpr int sAJ = 0, sWC = 9, sSG = 16;  // offsets in a stage record; a kernel's own fields start at 24

// nonzero of dt*J at (r, c) (the order of tt_track.hip's rAJ rows), or -1
__device__ __forceinline__ int d_idx(int r, int c) {
    return (r == 0 && c == 2) ? 0 : (r == 0 && c == 5) ? 1 : (r == 1 && c == 2) ? 2 : (r == 1 && c == 5) ? 3
         : (r == 2 && c == 4) ? 4 : (r == 2 && c == 5) ? 5 : (r == 3 && c == 3) ? 6 : (r == 3 && c == 4) ? 7
         : (r == 3 && c == 5) ? 8 : -1;
}
// nonzero of the curvature at (i, j), symmetric (the order of tt_track.hip's rWC rows), or -1
__device__ __forceinline__ int w_idx(int i, int j) {
    if (i > j) { const int t = i; i = j; j = t; }
    return (i == 2 && j == 2) ? 0 : (i == 2 && j == 5) ? 1 : (i == 3 && j == 3) ? 2 : (i == 3 && j == 4) ? 3
         : (i == 3 && j == 5) ? 4 : (i == 4 && j == 4) ? 5 : (i == 4 && j == 5) ? 6 : -1;
}

// One lane linearises one stage: Sigma of (x_k, u_k) from the stage's bound multipliers dk[6..21] and, unless it is the
// last stage, dt*J_f(x_k) and the curvature -dt sum_i y_{k+1,i} d2f_i/dx2 (x_k).
__device__ __forceinline__ void linearise_stage(const DiffArgs& a, double* r, const double* xk, const double* uk,
                                                const double* dk, bool last) {
    const double dt = a.dt;
    for (int v = 0; v < 8; ++v) {
        double sg = 0.0;
        if (v < 6 || !last) {
            const double val = v < 6 ? xk[v] : uk[v - 6];
            const double l = v < 6 ? a.xlb[v] : a.ulb[v - 6], ub = v < 6 ? a.xub[v] : a.uub[v - 6];
            if (isfinite(l) && l > -1e19) sg += dk[6 + v] / (val - (l - 1e-8 * fmax(1.0, fabs(l))));
            if (isfinite(ub) && ub < 1e19) sg += dk[14 + v] / ((ub + 1e-8 * fmax(1.0, fabs(ub))) - val);
        }
        r[sSG + v] = sg;
    }
    if (!last) {
        const double* y = dk + kDualPerStage;  // y_{k+1}
        const double iL1 = 1.0 / a.L1, iL2 = 1.0 / a.L2, iL1L2 = iL1 * iL2, Mh = a.Mh;
        double sth, cth, sps, cps, sph, cph;
        sincos(xk[2], &sth, &cth);
        sincos(xk[3], &sps, &cps);
        sincos(xk[4], &sph, &cph);
        const double v = xk[5], ic = 1.0 / cph, t = sph * ic, c2 = ic * ic;
        const double kk = 1.0 + Mh * iL2 * cps;
        r[sAJ + 0] = dt * (-v * sth);
        r[sAJ + 1] = dt * cth;
        r[sAJ + 2] = dt * (v * cth);
        r[sAJ + 3] = dt * sth;
        r[sAJ + 4] = dt * (v * c2 * iL1);
        r[sAJ + 5] = dt * (t * iL1);
        r[sAJ + 6] = dt * (v * t * Mh * sps * iL1L2 - v * cps * iL2);
        r[sAJ + 7] = dt * (-v * c2 * iL1 * kk);
        r[sAJ + 8] = dt * (-t * iL1 * kk - sps * iL2);
        const double s = -dt;
        r[sWC + 0] = s * (y[0] * (-v * cth) + y[1] * (-v * sth));
        r[sWC + 1] = s * (y[0] * (-sth) + y[1] * cth);
        r[sWC + 2] = s * (y[3] * (v * t * Mh * cps * iL1L2 + v * sps * iL2));
        r[sWC + 3] = s * (y[3] * (v * c2 * Mh * sps * iL1L2));
        r[sWC + 4] = s * (y[3] * (t * Mh * sps * iL1L2 - cps * iL2));
        r[sWC + 5] = s * (y[2] * (2.0 * v * t * c2 * iL1) + y[3] * (-2.0 * v * t * c2 * kk * iL1));
        r[sWC + 6] = s * (y[2] * (c2 * iL1) + y[3] * (-c2 * kk * iL1));
    }
}

template <class L, class = void>
struct has_dense : std::false_type {};
template <class L>
struct has_dense<L, std::void_t<decltype(L::sDH)>> : std::true_type {};

// entry-parallel roles of the serial sweeps: matrix entry (i, j), gain entry (gr, gc), p entry pi, kappa entry kr
struct Roles {
    bool ent, gl, pl, kl;
    int i, j, gr, gc, pi, kr;
    __device__ __forceinline__ explicit Roles(int lane)
        : ent(lane < 36), gl(lane >= 36 && lane < 48), pl(lane >= 48 && lane < 54), kl(lane >= 54 && lane < 56),
          i(ent ? lane / 6 : 0), j(ent ? lane % 6 : 0), gr(gl ? (lane - 36) / 6 : 0), gc(gl ? (lane - 36) % 6 : 0),
          pi(pl ? lane - 48 : 0), kr(kl ? lane - 54 : 0) {}
};

// The backward sweep over the linearised stage records stg[S][L::kStage]: K_k into Ks[N][2][6], the tiles in T.
// L gives the layout: kStage, the tile offsets tP, tM, tA, tRW, and kVec; with kVec also tQW (2 Q_w is kept for the
// output phase), tPV0, tPV1 (two p buffers: every p lane reads all of the one while it writes its entry of the other),
// tKP and sG, the offset of g = (gX 6, gU 2) in a stage record; kappa_k then overwrites gU_k.  wq: the instance's
// weights or nullptr.  Non-finite entries and an indefinite G set `bad`.  Returns the tile offset of p_0 (kVec).
template <class L>
__device__ __forceinline__ int backward_sweep(const DiffArgs& a, const Roles& ro, const double* wq, double* stg,
                                              double* Ks, double* T, int lane, bool& bad) {
    constexpr int kStage = L::kStage, tP = L::tP, tM = L::tM, tA = L::tA, tRW = L::tRW;
    const int N = a.N;
    const double dt = a.dt;
    const bool ent = ro.ent, gl = ro.gl;
    const int i = ro.i, j = ro.j, gr = ro.gr, gc = ro.gc;
    const int wi = w_idx(i, j);
    double q2 = 0.0;  // 2 Q_w (i, j)
    if (ent) {
        const double q = 0.5 * (a.Q[i * 6 + j] + a.Q[j * 6 + i]);
        q2 = 2.0 * (wq ? q * wq[i] * wq[j] : q);
        if constexpr (L::kVec) T[L::tQW + lane] = q2;
    }
    if (lane < 4) {  // 2 R_w
        const int ri = lane / 2, rj = lane % 2;
        const double rr = 0.5 * (a.R[ri * 2 + rj] + a.R[rj * 2 + ri]);
        T[tRW + lane] = 2.0 * (wq ? rr * wq[6 + ri] * wq[6 + rj] : rr);
    }
    __syncthreads();
    if (ent) {
        double p = q2 + (i == j ? stg[N * kStage + sSG + i] : 0.0);
        if constexpr (has_dense<L>::value)
            if (i < 4 && j < 4) p += stg[N * kStage + L::sDH + i * 4 + j];
        T[tP + lane] = p;
        bad |= !isfinite(p);
    }
    int pc = 0, pn = 0;  // p_{k+1} and p_k
    if constexpr (L::kVec) {
        pc = L::tPV0;
        pn = L::tPV1;
        if (ro.pl) T[pc + ro.pi] = stg[N * kStage + L::sG + ro.pi];  // p_N = gX_N
    }
    __syncthreads();
    for (int k = N - 1; k >= 0; --k) {
        double* r = stg + k * kStage;
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
        if (gl || (L::kVec && ro.kl)) {  // K = G^-1 B' M and kappa = G^-1 (gU + B' p), G = R_k + B' P B: side by side
            const double g00 = T[tRW + 0] + r[sSG + 6] + dt * dt * T[tP + 5 * 6 + 5];
            const double g01 = T[tRW + 1] + dt * dt * T[tP + 5 * 6 + 4];
            const double g11 = T[tRW + 3] + r[sSG + 7] + dt * dt * T[tP + 4 * 6 + 4];
            const double det = g00 * g11 - g01 * g01;
            double h0 = dt * T[tM + 5 * 6 + gc], h1 = dt * T[tM + 4 * 6 + gc];
            int row = gr;
            if constexpr (L::kVec) {
                h0 = gl ? h0 : r[L::sG + 6] + dt * T[pc + 5];
                h1 = gl ? h1 : r[L::sG + 7] + dt * T[pc + 4];
                row = gl ? gr : ro.kr;
            }
            double kv;
            if constexpr (has_dense<L>::value) {
                // The eliminated blocks put entries of 1e13 on P, and B' P B is then close to rank one: the determinant
                // form cancels.  Eliminate on the larger diagonal instead (G is positive definite or the solve fails).
                const bool sw = g11 > g00;
                const double d0 = sw ? g11 : g00, d1 = sw ? g00 : g11, b0 = sw ? h1 : h0, b1 = sw ? h0 : h1;
                const double m = g01 / d0, sc = d1 - m * g01;
                const double x1 = (b1 - m * b0) / sc, x0 = (b0 - g01 * x1) / d0;
                kv = (row == 0) == sw ? x1 : x0;
                if (!(d0 > 0.0) || !(sc > 0.0) || !isfinite(d0) || !isfinite(sc) || !isfinite(kv)) bad = true;
            } else {
                kv = row == 0 ? (g11 * h0 - g01 * h1) / det : (g00 * h1 - g01 * h0) / det;
                if (!(g00 > 0.0) || !(det > 0.0) || !isfinite(g00) || !isfinite(det) || !isfinite(kv)) bad = true;
            }
            if (gl) Ks[k * 12 + gr * 6 + gc] = kv;
            if constexpr (L::kVec)
                if (!gl) T[L::tKP + ro.kr] = kv;
        }
        __syncthreads();
        if (ent && k > 0) {  // P_k = W_k + Sigma_x + A' M - H' K,  H = B' M
            double p = q2 + (wi >= 0 ? r[sWC + wi] : 0.0) + (i == j ? r[sSG + i] : 0.0);
            if constexpr (has_dense<L>::value)
                if (i < 4 && j < 4) p += r[L::sDH + i * 4 + j];
            double am = 0.0;
            for (int l = 0; l < 6; ++l) am += T[tA + l * 6 + i] * T[tM + l * 6 + j];
            const double hk = dt * T[tM + 5 * 6 + i] * Ks[k * 12 + j] + dt * T[tM + 4 * 6 + i] * Ks[k * 12 + 6 + j];
            p = p + (am - hk);
            bad |= !isfinite(p);
            T[tP + lane] = p;  // (the reads of P of this stage are behind the barriers above)
        }
        if constexpr (L::kVec) {
            if (ro.pl) {  // p_k = gX_k + A' p_{k+1} - (B' M)' kappa   (M outlives this phase, P does not)
                const int pi = ro.pi;
                double s = 0.0;
                for (int l = 0; l < 6; ++l) s += T[tA + l * 6 + pi] * T[pc + l];
                const double hk = dt * T[tM + 5 * 6 + pi] * T[L::tKP + 0] + dt * T[tM + 4 * 6 + pi] * T[L::tKP + 1];
                s = r[L::sG + pi] + (s - hk);
                bad |= !isfinite(s);
                T[pn + pi] = s;
            }
            if (ro.kl) r[L::sG + 6 + ro.kr] = T[L::tKP + ro.kr];  // kappa_k takes gU_k's place for the forward sweep
        }
        __syncthreads();
        const int t = pc; pc = pn; pn = t;
    }
    return pc;
}

}  // namespace sens
}  // namespace ttmpc
