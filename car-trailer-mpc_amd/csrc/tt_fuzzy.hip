// The fuzzy weight rule (mpc_control_fuzzy.py:90-119) with its constants as data, and its adjoint: what a gradient
// with respect to the rule's parameters needs around fuzzy_kernel (tt_sim.hip), whose literals are the defaults here.
// Both kernels are one instance per thread, a few dozen bytes each way and launch bound; no atomics.
//
//   fuzzy_rule_kernel       wq_wr = rule(x_meas, xref[0]) for a tt_fuzzy_rule; with the defaults the expressions, their
//                           order and the contraction setting are fuzzy_kernel's, so the bits are too
//   fuzzy_rule_vjp_kernel   g_x[b][3] += dL/dpsi, g_rule_acc[b] += dL/dtheta from the upstream g_wq_wr; an instance
//                           whose accepted solve was the unit-weight retry adds nothing
#include <errno.h>
#include <math.h>
#include <hip/hip_runtime.h>

#include "tt_fuzzy_rule.hpp"
#include "tt_launch.hpp"
#include "ttmpc.h"

using namespace ttmpc;

namespace {

__global__ void __launch_bounds__(kThreads) fuzzy_rule_kernel(int B, int N, tt_fuzzy_rule r,
                                                              const double* __restrict__ x,
                                                              const double* __restrict__ xref, double* __restrict__ w) {
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= B) return;
    const double psi = x[(size_t)b * 6 + 3], v = x[(size_t)b * 6 + 5];
    const double ref_v = xref[(size_t)b * (N + 1) * 6 + 5];
    const double h = fmin(fabs(psi) / r.psi_full, 1.0);
    const bool reversing = (ref_v < r.v_rev) || (v < r.v_rev);
    double hitch = 1.0 + r.gain_hitch * h, steer = 1.0 + r.gain_steer * h, steer_rate = 1.0 + r.gain_rate * h;
    if (reversing) { hitch *= r.rev_hitch; steer *= r.rev_steer; steer_rate *= r.rev_rate; }
    const double lo = r.w_min, hi = r.w_max;
    auto clip = [lo, hi](double t) { return fmin(fmax(t, lo), hi); };
    double* o = w + (size_t)b * 8;
    o[0] = 1.0; o[1] = 1.0;
    o[2] = clip(fmax(1.0, steer));
    o[3] = clip(fmax(1.0, hitch));
    o[4] = clip(fmax(1.0, steer));
    o[5] = 1.0;
    o[6] = 1.0;
    o[7] = clip(fmax(1.0, steer_rate));
}

__global__ void __launch_bounds__(kThreads) fuzzy_rule_vjp_kernel(int B, int N, tt_fuzzy_rule r,
                                                                  const double* __restrict__ x,
                                                                  const double* __restrict__ xref,
                                                                  const int* __restrict__ retried,
                                                                  const double* __restrict__ g_w,
                                                                  double* __restrict__ g_x,
                                                                  double* __restrict__ g_rule_acc) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= B) return;
    if (retried && retried[b] != 0) return;
    double gth[7];
    const double g_psi = fuzzy_rule_vjp(r, x[(size_t)b * 6 + 3], x[(size_t)b * 6 + 5],
                                        xref[(size_t)b * (N + 1) * 6 + 5], g_w + (size_t)b * 8, gth);
    if (g_x) g_x[(size_t)b * 6 + 3] = g_x[(size_t)b * 6 + 3] + g_psi;
    if (g_rule_acc)
#pragma unroll
        for (int i = 0; i < 7; ++i) g_rule_acc[(size_t)b * 7 + i] += gth[i];
}

}  // namespace

extern "C" {

int tt_fuzzy_weights_rule_device(int B, int N, const tt_fuzzy_rule* rule, const double* x, const double* xref,
                                 double* wq_wr, void* stream) {
    if (B <= 0 || N < 1 || N > tt_max_horizon() || !x || !xref || !wq_wr || (rule && !fuzzy_rule_valid(*rule)))
        return -EINVAL;
    return launch_flat(fuzzy_rule_kernel, "fuzzy_rule_kernel", B, stream, B, N, rule ? *rule : fuzzy_rule_defaults(), x,
                       xref, wq_wr);
}

int tt_fuzzy_weights_vjp_device(int B, int N, const tt_fuzzy_rule* rule, const double* x, const double* xref,
                                const int* retried, const double* g_wq_wr, double* g_x, double* g_rule_acc,
                                void* stream) {
    if (B <= 0 || N < 1 || N > tt_max_horizon() || (rule && !fuzzy_rule_valid(*rule))) return -EINVAL;
    if (!x || !xref || !g_wq_wr || (!g_x && !g_rule_acc)) return 0;   // nothing to read or nothing to write
    return launch_flat(fuzzy_rule_vjp_kernel, "fuzzy_rule_vjp_kernel", B, stream, B, N,
                       rule ? *rule : fuzzy_rule_defaults(), x, xref, retried, g_wq_wr, g_x, g_rule_acc);
}

}  // extern "C"
