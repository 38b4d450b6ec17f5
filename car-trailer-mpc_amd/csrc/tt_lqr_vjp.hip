// Reverse mode of the batched LQR terminal score on gfx950: the vector-Jacobian product of tt_lqr_score_device
// (tt_lqr.hip) at the P it returned.
//
//   forward   A = I + dt df/dx(x_goal),  B = dt [e5 e4],  P = DARE(A, B, Q, R) symmetrised,  score = dx' P dx
//   K = (R + B'PB)^-1 B'PA (2x2 inverse in closed form: B'PB = dt^2 P[{5,4},{5,4}]),  Ac = A - BK
//   DARE differentiated at its stabilising solution:  dP = Ac' dP Ac + dQ + K' dR K + dA' P Ac + Ac' P dA
//   upstream gs = dL/dscore, GP = dL/dP:  G = gs dx dx' + (GP + GP')/2,   S = Ac S Ac' + G
//   dL/dx_cur = 2 gs P dx,  dL/dQ = S,  dL/dR = K S K',  dL/dA = 2 P Ac S,
//   dL/dx_goal[m] = -2 gs (P dx)[m] + dt sum_ij (dL/dA)_ij d2f_i/dq_j dq_m
//
// The Lyapunov equation is solved by Smith doubling, S <- S + T S T', T <- T^2 from S = G, T = Ac: quadratic because
// rho(Ac) < 1, with the forward's stopping shape.  Layout as the forward: one 64-lane workgroup per instance, the 6x6
// matrices in LDS, lane (i, j) < 36 owns entry (i, j) of every product; every sum runs in a fixed order and nothing
// is accumulated across workgroups, so two launches give the same bits.
#include <errno.h>
#include <hip/hip_runtime.h>
#include <math.h>

#include "tt_lqr_model.hpp"
#include "ttmpc.h"

using namespace ttmpc;

namespace {

struct LqrVjpArgs {
    tt_plant p;
    double R[4];
    const double* xc;
    const double* xg;
    const double* P;
    const int* fwd_iters;
    const double* gs;
    const double* GP;
    tt_lqr_vjp_out out;
    int B;
};

__device__ __forceinline__ bool wave_any(bool v) { return __ballot(v) != 0ull; }

// (X Y')[i][j]
__device__ __forceinline__ double mmt(const double* X, const double* Y, int i, int j) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) s += X[i * 6 + k] * Y[j * 6 + k];
    return s;
}

__global__ void __launch_bounds__(64) lqr_vjp_kernel(LqrVjpArgs a) {
    __shared__ double sA[36], sP[36], sAc[36], sS[36], sT[36], sX[36], sK[12], sKS[12], sdx[6], sPdx[6];
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= a.B) return;
    const int i = lane / 6, j = lane % 6;
    const bool own = lane < 36;
    const size_t b6 = (size_t)b * 6, b36 = (size_t)b * 36;
    if (a.fwd_iters && a.fwd_iters[b] < 0) {   // the forward's DARE did not converge: nothing to differentiate
        if (own && a.out.g_Q) a.out.g_Q[b36 + lane] = 0.0;
        if (lane < 6 && a.out.g_x_cur) a.out.g_x_cur[b6 + lane] = 0.0;
        if (lane < 6 && a.out.g_x_goal) a.out.g_x_goal[b6 + lane] = 0.0;
        if (lane < 4 && a.out.g_R) a.out.g_R[(size_t)b * 4 + lane] = 0.0;
        if (lane == 0 && a.out.vjp_status) a.out.vjp_status[b] = 2;
        if (lane == 0 && a.out.iters) a.out.iters[b] = 0;
        return;
    }
    const double dt = a.p.dt, L1 = a.p.L1, L2 = a.p.L2, Mh = a.p.Mh;
    const double* xg = a.xg + b6;
    const double* xc = a.xc + b6;
    const double gs = a.gs ? a.gs[b] : 0.0;
    const GoalTrig gt(xg);
    const double v = gt.v, sth = gt.sth, cth = gt.cth, sps = gt.sps, cps = gt.cps, c2 = gt.c2, t = gt.t;
    bool bad = !isfinite(gs);
    // A = I + dt J(x_goal), the forward's expressions; P; G = gs dx dx' + (GP + GP') / 2
    if (own) {
        const double Aij = (i == j ? 1.0 : 0.0) + dt * goal_jacobian(i, j, gt, L1, L2, Mh), Pij = a.P[b36 + lane];
        double Gij = gs * (xc[i] - xg[i]) * (xc[j] - xg[j]);
        if (a.GP) Gij += 0.5 * (a.GP[b36 + lane] + a.GP[b36 + j * 6 + i]);
        sA[lane] = Aij;
        sP[lane] = Pij;
        sS[lane] = Gij;
        if (lane < 6) sdx[lane] = xc[lane] - xg[lane];
        bad = bad || !isfinite(Aij) || !isfinite(Pij) || !isfinite(Gij);
    }
    __syncthreads();
    // K = (R + B'PB)^-1 B'PA, rows of B'PA = dt (PA)[5], dt (PA)[4]
    const double h00 = a.R[0] + dt * dt * sP[35], h01 = a.R[1] + dt * dt * sP[34];
    const double h10 = a.R[2] + dt * dt * sP[29], h11 = a.R[3] + dt * dt * sP[28];
    const double det = h00 * h11 - h01 * h10;
    bad = bad || !(det > 0.0) || !isfinite(det);
    if (own) sX[lane] = mm(sP, sA, i, j);
    __syncthreads();
    if (lane < 6) {
        const double r0 = dt * sX[30 + lane], r1 = dt * sX[24 + lane];
        sK[lane] = (h11 * r0 - h01 * r1) / det;
        sK[6 + lane] = (h00 * r1 - h10 * r0) / det;
    }
    __syncthreads();
    // Ac = A - BK: only rows 5 (a -> v) and 4 (omega -> phi) change
    if (own) {
        double Acij = sA[lane];
        if (i == 5) Acij -= dt * sK[j];
        if (i == 4) Acij -= dt * sK[6 + j];
        sAc[lane] = Acij;
        sT[lane] = Acij;
        bad = bad || !isfinite(Acij);
    }
    bad = wave_any(bad);
    __syncthreads();
    // Smith doubling: S <- S + T S T', T <- T^2
    int it = 0;
    bool done = false;
    for (; it < kMaxDoublings && !done && !bad; ++it) {
        if (own) sX[lane] = mm(sT, sS, i, j);
        __syncthreads();
        double D = 0.0, Sn = 0.0, Tn = 0.0;
        if (own) {
            D = mmt(sX, sT, i, j);
            Sn = sS[lane] + D;
            Tn = mm(sT, sT, i, j);
        }
        const double dS = wave_max(fabs(D)), nS = wave_max(fabs(Sn));
        bad = wave_any(!isfinite(Sn) || !isfinite(Tn));
        __syncthreads();
        if (own) {
            sS[lane] = Sn;
            sT[lane] = Tn;
        }
        __syncthreads();
        done = !(dS > 1e-14 * nS) || !isfinite(nS);
    }
    bad = bad || !done;
    // S = (S + S') / 2 once; dL/dQ = S
    const double Sij = own ? 0.5 * (sS[lane] + sS[j * 6 + i]) : 0.0;
    __syncthreads();
    if (own) sS[lane] = Sij;
    __syncthreads();
    // K S (2x6), Ac S, P dx
    if (own) sX[lane] = mm(sAc, sS, i, j);
    if (lane < 12) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) s += sK[i * 6 + k] * sS[k * 6 + j];
        sKS[lane] = s;
    }
    if (lane < 6) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) s += sP[lane * 6 + k] * sdx[k];
        sPdx[lane] = s;
    }
    __syncthreads();
    // dL/dA = 2 P (Ac S) into sT (T is no longer needed); dL/dR = (K S) K'
    double gR = 0.0;
    if (own) sT[lane] = 2.0 * mm(sP, sX, i, j);
    if (lane < 4) {
        const int r = lane / 2, c = lane % 2;
#pragma unroll
        for (int k = 0; k < 6; ++k) gR += sKS[r * 6 + k] * sK[c * 6 + k];
    }
    __syncthreads();
    // dL/dx_cur = 2 gs P dx; dL/dx_goal = -2 gs P dx + dt sum_ij gA_ij d2f_i/dq_j dq_m (theta, psi, phi, v only)
    double gxc = 0.0, gxg = 0.0;
    if (lane < 6) {
        const double* gA = sT;
        const double hk = 1 + Mh / L2 * cps;
        const double H33 = v * t * Mh * cps / (L1 * L2) + v * sps / L2;       // d2f3 / dpsi2
        const double H34 = v * c2 * Mh * sps / (L1 * L2);                     // d2f3 / dpsi dphi
        const double H35 = t * Mh * sps / (L1 * L2) - cps / L2;               // d2f3 / dpsi dv
        const double H44 = -2 * v * t * c2 * hk / L1;                         // d2f3 / dphi2
        const double H45 = -c2 * hk / L1;                                     // d2f3 / dphi dv
        double h = 0.0;
        if (lane == 2) h = gA[2] * (-v * cth) + gA[5] * (-sth) + gA[8] * (-v * sth) + gA[11] * cth;
        if (lane == 3) h = gA[21] * H33 + gA[22] * H34 + gA[23] * H35;
        if (lane == 4)
            h = gA[16] * (2 * v * t * c2 / L1) + gA[17] * (c2 / L1) + gA[21] * H34 + gA[22] * H44 + gA[23] * H45;
        if (lane == 5) h = gA[2] * (-sth) + gA[8] * cth + gA[16] * (c2 / L1) + gA[21] * H35 + gA[22] * H45;
        gxc = 2.0 * gs * sPdx[lane];
        gxg = -gxc + dt * h;
    }
    bad = wave_any(bad || !isfinite(Sij) || !isfinite(gR) || !isfinite(gxc) || !isfinite(gxg));
    if (own && a.out.g_Q) a.out.g_Q[b36 + lane] = bad ? 0.0 : Sij;
    if (lane < 6 && a.out.g_x_cur) a.out.g_x_cur[b6 + lane] = bad ? 0.0 : gxc;
    if (lane < 6 && a.out.g_x_goal) a.out.g_x_goal[b6 + lane] = bad ? 0.0 : gxg;
    if (lane < 4 && a.out.g_R) a.out.g_R[(size_t)b * 4 + lane] = bad ? 0.0 : gR;
    if (lane == 0 && a.out.vjp_status) a.out.vjp_status[b] = bad ? 1 : 0;
    if (lane == 0 && a.out.iters) a.out.iters[b] = it;
}

}  // namespace

extern "C" int tt_lqr_score_vjp_device(int B, const tt_plant* p, const double* R, const double* x_cur,
                                       const double* x_goal, const double* P, const int* fwd_iters,
                                       const double* grad_score, const double* grad_P, const tt_lqr_vjp_out* out,
                                       void* stream) {
    if (B < 0 || !p || !R || !out) return -EINVAL;
    if (R[0] * R[3] - R[1] * R[2] == 0.0) return -EINVAL;
    if (B == 0) return 0;
    if (!x_cur || !x_goal || !P || (!grad_score && !grad_P)) return -EINVAL;
    LqrVjpArgs a;
    a.p = *p;
    for (int k = 0; k < 4; ++k) a.R[k] = R[k];
    a.xc = x_cur;
    a.xg = x_goal;
    a.P = P;
    a.fwd_iters = fwd_iters;
    a.gs = grad_score;
    a.GP = grad_P;
    a.out = *out;
    a.B = B;
    hipLaunchKernelGGL(lqr_vjp_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
    return launched("lqr_vjp_kernel");
}
