// What lqr_kernel (tt_lqr.hip) and lqr_vjp_kernel (tt_lqr_vjp.hip) share: the Jacobian of the model at the goal state,
// the 6x6 product, the wave maximum of the stopping tests and the doubling limit.  The Jacobian is in the division
// form (x / L1, not x * (1 / L1) as tt_sens_stage.hpp has it): the two differ in the last bit, and the adjoint must
// rebuild the forward's A exactly.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "tt_launch.hpp"

namespace ttmpc {

constexpr int kMaxDoublings = 64;

// trigonometry of a goal state (theta, psi, phi at xg[2..4], v at xg[5])
struct GoalTrig {
    double v, sth, cth, sps, cps, c2, t;
    __device__ __forceinline__ explicit GoalTrig(const double* xg)
        : v(xg[5]), sth(sin(xg[2])), cth(cos(xg[2])), sps(sin(xg[3])), cps(cos(xg[3])),
          c2(1.0 / (cos(xg[4]) * cos(xg[4]))), t(tan(xg[4])) {}
};

// df_i/dx_j at the goal (truck_trailer_model.py:8-24 differentiated; u enters f linearly)
__device__ __forceinline__ double goal_jacobian(int i, int j, const GoalTrig& g, double L1, double L2, double Mh) {
    const double v = g.v, t = g.t, c2 = g.c2;
    double J = 0.0;
    if (i == 0 && j == 2) J = -v * g.sth;
    if (i == 0 && j == 5) J = g.cth;
    if (i == 1 && j == 2) J = v * g.cth;
    if (i == 1 && j == 5) J = g.sth;
    if (i == 2 && j == 4) J = v * c2 / L1;
    if (i == 2 && j == 5) J = t / L1;
    if (i == 3 && j == 3) J = v * t * Mh * g.sps / (L1 * L2) - v * g.cps / L2;
    if (i == 3 && j == 4) J = -v * c2 / L1 * (1 + Mh / L2 * g.cps);
    if (i == 3 && j == 5) J = -t / L1 * (1 + Mh / L2 * g.cps) - g.sps / L2;
    return J;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// (X Y)[i][j] over 6x6 row-major LDS matrices; lanes < 36
__device__ __forceinline__ double mm(const double* X, const double* Y, int i, int j) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) s += X[i * 6 + k] * Y[k * 6 + j];
    return s;
}

}  // namespace ttmpc
