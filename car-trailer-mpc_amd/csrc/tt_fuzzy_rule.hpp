// The fuzzy weight rule as data (tt_fuzzy_rule, include/ttmpc.h) and its adjoint for one instance, shared by
// tt_fuzzy.hip (the rule forward and the stand-alone adjoint) and tt_sim_vjp.hip (the adjoint fused into the window
// adjoint of a backward step).
#pragma once
#include <math.h>
#include <hip/hip_runtime.h>

#include "ttmpc.h"

namespace ttmpc {

// mpc_control_fuzzy.py:90-119
__host__ __device__ inline tt_fuzzy_rule fuzzy_rule_defaults() {
    return tt_fuzzy_rule{0.35, 2.0, 1.2, 1.5, 1.1, 1.1, 1.2, 1.0, 3.5, -0.1};
}

// what the entries accept: every field finite, psi_full > 0, w_min <= w_max
inline bool fuzzy_rule_valid(const tt_fuzzy_rule& r) {
    const double f[10] = {r.psi_full, r.gain_hitch, r.gain_steer, r.gain_rate, r.rev_hitch,
                          r.rev_steer, r.rev_rate, r.w_min, r.w_max, r.v_rev};
    for (double v : f)
        if (!isfinite(v)) return false;
    return r.psi_full > 0.0 && r.w_min <= r.w_max;
}

// Adjoint of the rule at (psi, v, ref_v) for the upstream gradient gw (8) of the weights: returns dL/dpsi and writes
// gth (7) = dL/d(psi_full, gain_hitch, gain_steer, gain_rate, rev_hitch, rev_steer, rev_rate).  A channel passes its
// gradient where neither the max(1, .) nor the clip holds it: raw > 1 and w_min < max(1, raw) < w_max.  d|x|/dx =
// sign(x) (0 at 0); d min(s, 1)/ds = 1 for s < 1, else 0; v and ref_v only switch.
__device__ __forceinline__ double fuzzy_rule_vjp(const tt_fuzzy_rule& r, double psi, double v, double ref_v,
                                                 const double* gw, double* gth) {
#pragma clang fp contract(off)
    const double s = fabs(psi) / r.psi_full;
    const double h = fmin(s, 1.0);
    const bool rev = (ref_v < r.v_rev) || (v < r.v_rev);
    const double gain[3] = {r.gain_hitch, r.gain_steer, r.gain_rate};
    const double fac[3] = {rev ? r.rev_hitch : 1.0, rev ? r.rev_steer : 1.0, rev ? r.rev_rate : 1.0};
    const double G[3] = {gw[3], gw[2] + gw[4], gw[7]};
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double lin = 1.0 + gain[c] * h;
        const double raw = lin * fac[c];
        const double m = fmax(1.0, raw);
        const bool pass = raw > 1.0 && r.w_min < m && m < r.w_max;
        gth[1 + c] = pass ? G[c] * h * fac[c] : 0.0;
        gth[4 + c] = pass && rev ? G[c] * lin : 0.0;
        if (pass) acc = acc + G[c] * gain[c] * fac[c];
    }
    if (!(s < 1.0)) {
        gth[0] = 0.0;
        return 0.0;
    }
    const double sg = psi > 0.0 ? 1.0 : (psi < 0.0 ? -1.0 : 0.0);
    gth[0] = -(acc * fabs(psi) / (r.psi_full * r.psi_full));
    return acc * sg / r.psi_full;
}

}  // namespace ttmpc
