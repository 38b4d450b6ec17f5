// What track_sens_kernel (tt_sens.hip) and track_vjp_kernel (tt_vjp.hip) share: the head of a stage record in LDS
// (dt*J 9 | curvature 7 | Sigma 8), the lane that linearises one stage into it, and the sparsity maps of dt*J and of the
// curvature.  Both kernels differentiate at the same primal-dual point, so they read the same Newton matrix.
#pragma once
#include <math.h>

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
// last stage, dt*J_f(x_k) and the curvature -dt sum_i y_{k+1,i} d2f_i/dx2 (x_k).  Args: SensArgs or VjpArgs.
template <class Args>
__device__ __forceinline__ void linearise_stage(const Args& a, double* r, const double* xk, const double* uk,
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

}  // namespace sens
}  // namespace ttmpc
