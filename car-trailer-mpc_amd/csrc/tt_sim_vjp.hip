// Reverse mode of the closed-loop glue in tt_sim.hip: the adjoints of policy_plant_kernel (+ plant_apply) and of
// sim_window_kernel, the two pieces a backward sweep over a taped closed loop needs around tt_track_vjp_device
// (include/ttmpc.h, "Reverse mode of the closed loop").  Both kernels are tiny and HBM / launch bound, like their
// forward twins; no atomics anywhere, so two sweeps over one tape are bitwise equal.
//
//   policy_plant_vjp_kernel   one instance per thread: a <- J_q' a, the seed g_u0 of the solve adjoint, the adjoint
//                             of u_last, dL/d(in-plant noise)
//   sim_window_vjp_kernel     one thread per (instance, window row): the window's scatter into the plan gradient
//                             with the forward's end padding, and the per-instance accumulation of the step; its
//                             fuzzy instantiation first applies the adjoint of the weight rule (tt_fuzzy_rule.hpp)
#include <errno.h>
#include <math.h>
#include <hip/hip_runtime.h>

#include "tt_fuzzy_rule.hpp"
#include "tt_launch.hpp"
#include "ttmpc.h"

using namespace ttmpc;

namespace {

__device__ __forceinline__ double sign0(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); }

// Adjoint of plant_apply (tt_sim.hip) at the pre-update state q: a (6) <- J_q' a, cu (2) = J_u' a with u the control
// before the friction / slippage scaling.  d|x|/dx = sign(x) (0 at 0); d min(s, 0.3)/ds = 1 for s < 0.3, else 0.
__device__ __forceinline__ void plant_vjp(const tt_plant& p, const double* q, double* a, double* cu) {
#pragma clang fp contract(off)
    const double dt = p.dt;
    const double th = q[2], ps = q[3], ph = q[4], v = q[5];
    const double fc = p.enable ? p.friction_coeff : 1.0, sc = p.enable ? p.slippage_coeff : 1.0;
    cu[0] = a[5] * dt * fc;
    cu[1] = a[4] * dt * sc;
    const double cth = cos(th), sth = sin(th), cps = cos(ps), sps = sin(ps), tph = tan(ph);
    const double sec2 = 1.0 + tph * tph;
    const double hk = 1 + p.Mh / p.L2 * cps;
    const double f2 = v * tph / p.L1;                         // q_dot[2], q_dot[3] before the slip factor
    const double f3 = -v * tph / p.L1 * hk - v * sps / p.L2;
    const double f2_ph = v * sec2 / p.L1, f2_v = tph / p.L1;
    const double f3_ps = v * tph / p.L1 * (p.Mh / p.L2 * sps) - v * cps / p.L2;
    const double f3_ph = -v * sec2 / p.L1 * hk;
    const double f3_v = -tph / p.L1 * hk - sps / p.L2;
    double slip = 1.0, slip_ph = 0.0, slip_v = 0.0;
    if (p.enable) {
        const double s = fabs(ph) * fabs(v) * p.slip_angle_max;
        slip = 1.0 - fmin(s, 0.3);
        if (s < 0.3) {
            slip_ph = -(sign0(ph) * fabs(v) * p.slip_angle_max);
            slip_v = -(fabs(ph) * sign0(v) * p.slip_angle_max);
        }
    }
    double g_th = a[0] * (-v * sth) + a[1] * (v * cth);
    const double g_ps = a[3] * (slip * f3_ps);
    double g_ph = a[2] * (slip * f2_ph + f2 * slip_ph) + a[3] * (slip * f3_ph + f3 * slip_ph);
    double g_v = a[0] * cth + a[1] * sth + a[2] * (slip * f2_v + f2 * slip_v) + a[3] * (slip * f3_v + f3 * slip_v);
    if (p.enable) {                                           // lateral slip, formed from the pre-update th, ph, v
        const double cl = cos(th + M_PI / 2), sl = sin(th + M_PI / 2);
        const double mag = p.lateral_slip_gain * fabs(v) * fabs(ph);
        const double along = a[0] * cl + a[1] * sl;
        g_th += mag * (a[1] * cl - a[0] * sl);
        g_ph += p.lateral_slip_gain * fabs(v) * sign0(ph) * along;
        g_v += p.lateral_slip_gain * sign0(v) * fabs(ph) * along;
    }
    a[2] = a[2] + g_th * dt;
    a[3] = a[3] + g_ps * dt;
    a[4] = a[4] + g_ph * dt;
    a[5] = a[5] + g_v * dt;
}

// a' dS_{t+1}/d(L1, L2, Mh) of plant_apply at the pre-update state q, a taken before the J_q product: only rows 2 and 3
// of the Euler step depend on the geometry, dt slip (a_2 df_2/dtheta + a_3 df_3/dtheta) with the forward's slip factor;
// the lateral-slip and friction terms do not.
__device__ __forceinline__ void plant_model_vjp(const tt_plant& p, const double* q, const double* a, double* gm) {
#pragma clang fp contract(off)
    const double ps = q[3], ph = q[4], v = q[5];
    const double cps = cos(ps), sps = sin(ps), tph = tan(ph);
    const double hk = 1 + p.Mh / p.L2 * cps;
    const double f2 = v * tph / p.L1;
    double slip = 1.0;
    if (p.enable) slip = 1.0 - fmin(fabs(ph) * fabs(v) * p.slip_angle_max, 0.3);
    const double f2_L1 = -(f2 / p.L1);
    const double f3_L1 = f2 * hk / p.L1;
    const double f3_L2 = f2 * (p.Mh / p.L2 * cps) / p.L2 + v * sps / p.L2 / p.L2;
    const double f3_Mh = -f2 * (cps / p.L2);
    const double s = p.dt * slip;
    gm[0] = s * (a[2] * f2_L1 + a[3] * f3_L1);
    gm[1] = s * (a[3] * f3_L2);
    gm[2] = s * (a[3] * f3_Mh);
}

// The branch of policy_plant_kernel an instance took is read from the logs: active before / after the step, the
// step's status and the consecutive-failure count after the step (include/ttmpc.h has the table).
// kModel: also g_model_acc [B][3] += a' dS_{t+1}/d(L1, L2, Mh) for every instance that moved; the plain instantiation
// behind policy_plant_vjp_kernel is the kernel as it was.
template <bool kModel>
__device__ __forceinline__ void policy_plant_vjp_body(
    int B, int N, const tt_plant& p, int policy, const double* __restrict__ state, const int* __restrict__ status,
    const int* __restrict__ act_before, const int* __restrict__ act_after, const int* __restrict__ consec,
    const double* __restrict__ grad_ua, double* __restrict__ adj, double* __restrict__ adj_last,
    double* __restrict__ grad_u, double* __restrict__ g_noise, double* __restrict__ g_model_acc) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * kThreads + threadIdx.x;
    if (b >= B) return;
    double* gu0 = grad_u + (size_t)b * 2 * N;
    const bool before = act_before ? act_before[b] != 0 : true;
    if (!before || act_after[b] == 0) {   // stopped: the state is kept and nothing of the solve is applied
        gu0[0] = 0.0;
        gu0[1] = 0.0;
        if (before && policy == TT_POLICY_NMPC) adj_last[(size_t)b * 2] = adj_last[(size_t)b * 2 + 1] = 0.0;
        if (g_noise)
#pragma unroll
            for (int i = 0; i < 6; ++i) g_noise[(size_t)b * 6 + i] = 0.0;
        return;
    }
    double q[6], a[6], c[2];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        q[i] = state[(size_t)b * 6 + i];
        a[i] = adj[(size_t)b * 6 + i];
    }
    if (g_noise)
#pragma unroll
        for (int i = 0; i < 6; ++i) g_noise[(size_t)b * 6 + i] = p.dt * a[i];
    if constexpr (kModel) {
        double gm[3];
        plant_model_vjp(p, q, a, gm);
#pragma unroll
        for (int i = 0; i < 3; ++i) g_model_acc[(size_t)b * 3 + i] += gm[i];
    }
    plant_vjp(p, q, a, c);
    if (grad_ua) {
        c[0] = c[0] + grad_ua[(size_t)b * 2];
        c[1] = c[1] + grad_ua[(size_t)b * 2 + 1];
    }
    double l0 = adj_last[(size_t)b * 2], l1 = adj_last[(size_t)b * 2 + 1];
    double g0 = 0.0, g1 = 0.0;
    if (status[b] <= TT_ACCEPTABLE) {             // u = U[0], u_last = u
        g0 = c[0] + l0;
        g1 = c[1] + l1;
        l0 = l1 = 0.0;
    } else if (policy == TT_POLICY_NMPC) {        // u = 0, u_last = 0
        l0 = l1 = 0.0;
    } else if (policy == TT_POLICY_FUZZY) {       // u = u_last (zero after 15 consecutive failures)
        if (consec[b] <= 15) {
            l0 = l0 + c[0];
            l1 = l1 + c[1];
        }
    } else {                                      // u = U[0] of a failed solve: tt_track_vjp_device zeroes it
        g0 = c[0];
        g1 = c[1];
    }
    gu0[0] = g0;
    gu0[1] = g1;
    adj_last[(size_t)b * 2] = l0;
    adj_last[(size_t)b * 2 + 1] = l1;
#pragma unroll
    for (int i = 0; i < 6; ++i) adj[(size_t)b * 6 + i] = a[i];
}

__global__ void __launch_bounds__(kThreads) policy_plant_vjp_kernel(
    int B, int N, tt_plant p, int policy, const double* __restrict__ state, const int* __restrict__ status,
    const int* __restrict__ act_before, const int* __restrict__ act_after, const int* __restrict__ consec,
    const double* __restrict__ grad_ua, double* __restrict__ adj, double* __restrict__ adj_last,
    double* __restrict__ grad_u, double* __restrict__ g_noise) {
    policy_plant_vjp_body<false>(B, N, p, policy, state, status, act_before, act_after, consec, grad_ua, adj, adj_last,
                                 grad_u, g_noise, nullptr);
}

__global__ void __launch_bounds__(kThreads) policy_plant_vjp_model_kernel(
    int B, int N, tt_plant p, int policy, const double* __restrict__ state, const int* __restrict__ status,
    const int* __restrict__ act_before, const int* __restrict__ act_after, const int* __restrict__ consec,
    const double* __restrict__ grad_ua, double* __restrict__ adj, double* __restrict__ adj_last,
    double* __restrict__ grad_u, double* __restrict__ g_noise, double* __restrict__ g_model_acc) {
    policy_plant_vjp_body<true>(B, N, p, policy, state, status, act_before, act_after, consec, grad_ua, adj, adj_last,
                                grad_u, g_noise, g_model_acc);
}

// Adjoint of sim_window_kernel, one thread per (instance, window row j).  State row j went to plan row min(k+j, Np),
// input row j to min(k+j, Np-1) while k < Np (else the input window is zeros).  A destination row belongs to the thread
// of the first window row that lands on it; the padded tail is summed by that thread in ascending j.  The thread of
// j = N also does the step's per-instance accumulation: adj += g_x0 + grad_s, g_w_acc += g_w, g_noise = g_x0.
// kFuzzy: the weights of the step came from the rule, w = rule(x_meas, xref[0]), so that thread first adds the rule's
// dL/dpsi to g_x0[3] (as it reads it: the buffer is left alone) and the rule's dL/dtheta to g_rule_acc [B][7], unless
// the instance's accepted solve was the unit-weight retry; the plain instantiation behind sim_window_vjp_kernel is the
// kernel as it was.
struct FuzzyVjpArgs {
    tt_fuzzy_rule rule;
    const double* x_meas;
    const double* xref;
    const int* retried;
    double* g_rule_acc;
};

template <bool kFuzzy>
__device__ __forceinline__ void sim_window_vjp_body(
    int B, int N, int k, int Np, const double* __restrict__ g_xref, const double* __restrict__ g_uref,
    double* __restrict__ g_plan_x, double* __restrict__ g_plan_u, const double* __restrict__ g_x0,
    const double* __restrict__ grad_s, double* __restrict__ adj, const double* __restrict__ g_w,
    double* __restrict__ g_w_acc, double* __restrict__ g_noise, const FuzzyVjpArgs* fz) {
#pragma clang fp contract(off)
    const long long t = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (t >= (long long)B * (N + 1)) return;
    const int b = (int)(t / (N + 1)), j = (int)(t % (N + 1));
    if (g_xref && g_plan_x) {
        const double* src = g_xref + (size_t)b * (N + 1) * 6;
        const long long r = (long long)k + j;
        if (r < Np) {
            double* dst = g_plan_x + ((size_t)b * (Np + 1) + r) * 6;
#pragma unroll
            for (int i = 0; i < 6; ++i) dst[i] += src[(size_t)j * 6 + i];
        } else if (r == Np || j == 0) {   // first window row on plan row Np: it owns the padded tail
            double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (int jj = j; jj <= N; ++jj)
#pragma unroll
                for (int i = 0; i < 6; ++i) s[i] = s[i] + src[(size_t)jj * 6 + i];
            double* dst = g_plan_x + ((size_t)b * (Np + 1) + Np) * 6;
#pragma unroll
            for (int i = 0; i < 6; ++i) dst[i] += s[i];
        }
    }
    if (g_uref && g_plan_u && j < N && k < Np) {
        const double* src = g_uref + (size_t)b * N * 2;
        const long long r = (long long)k + j;
        if (r < Np - 1) {
            double* dst = g_plan_u + ((size_t)b * Np + r) * 2;
            dst[0] += src[(size_t)j * 2];
            dst[1] += src[(size_t)j * 2 + 1];
        } else if (r == Np - 1) {         // k < Np: row j = Np-1-k >= 0 exists and owns the padded tail
            double s0 = 0.0, s1 = 0.0;
            for (int jj = j; jj < N; ++jj) {
                s0 = s0 + src[(size_t)jj * 2];
                s1 = s1 + src[(size_t)jj * 2 + 1];
            }
            double* dst = g_plan_u + ((size_t)b * Np + (Np - 1)) * 2;
            dst[0] += s0;
            dst[1] += s1;
        }
    }
    if (j == N) {
        double x0[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (g_x0)
#pragma unroll
            for (int i = 0; i < 6; ++i) x0[i] = g_x0[(size_t)b * 6 + i];
        if constexpr (kFuzzy) {
            if (g_x0 && g_w && !(fz->retried && fz->retried[b] != 0)) {
                double gth[7];
                const double g_psi = fuzzy_rule_vjp(fz->rule, fz->x_meas[(size_t)b * 6 + 3], fz->x_meas[(size_t)b * 6 + 5],
                                                    fz->xref[(size_t)b * (N + 1) * 6 + 5], g_w + (size_t)b * 8, gth);
                x0[3] = x0[3] + g_psi;
                if (fz->g_rule_acc)
#pragma unroll
                    for (int i = 0; i < 7; ++i) fz->g_rule_acc[(size_t)b * 7 + i] += gth[i];
            }
        }
        if (adj)
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                double v = adj[(size_t)b * 6 + i];
                if (g_x0) v = v + x0[i];
                if (grad_s) v = v + grad_s[(size_t)b * 6 + i];
                adj[(size_t)b * 6 + i] = v;
            }
        if (g_noise && g_x0)
#pragma unroll
            for (int i = 0; i < 6; ++i) g_noise[(size_t)b * 6 + i] = x0[i];
        if (g_w && g_w_acc)
#pragma unroll
            for (int i = 0; i < 8; ++i) g_w_acc[(size_t)b * 8 + i] += g_w[(size_t)b * 8 + i];
    }
}

__global__ void __launch_bounds__(kThreads) sim_window_vjp_kernel(
    int B, int N, int k, int Np, const double* __restrict__ g_xref, const double* __restrict__ g_uref,
    double* __restrict__ g_plan_x, double* __restrict__ g_plan_u, const double* __restrict__ g_x0,
    const double* __restrict__ grad_s, double* __restrict__ adj, const double* __restrict__ g_w,
    double* __restrict__ g_w_acc, double* __restrict__ g_noise) {
    sim_window_vjp_body<false>(B, N, k, Np, g_xref, g_uref, g_plan_x, g_plan_u, g_x0, grad_s, adj, g_w, g_w_acc, g_noise,
                               nullptr);
}

__global__ void __launch_bounds__(kThreads) sim_window_vjp_fuzzy_kernel(
    int B, int N, int k, int Np, const double* __restrict__ g_xref, const double* __restrict__ g_uref,
    double* __restrict__ g_plan_x, double* __restrict__ g_plan_u, const double* __restrict__ g_x0,
    const double* __restrict__ grad_s, double* __restrict__ adj, const double* __restrict__ g_w,
    double* __restrict__ g_w_acc, double* __restrict__ g_noise, FuzzyVjpArgs fz) {
    sim_window_vjp_body<true>(B, N, k, Np, g_xref, g_uref, g_plan_x, g_plan_u, g_x0, grad_s, adj, g_w, g_w_acc, g_noise,
                              &fz);
}

// What the two policy-plant adjoint entries, and the two window adjoint entries, ask of their arguments.
bool policy_plant_vjp_args_ok(int B, int N, const tt_plant* p, int policy, const double* state, const int* status,
                              const int* active_after, const int* consecutive, const double* adj_state,
                              const double* adj_u_last, const double* grad_u) {
    return B > 0 && N >= 1 && N <= tt_max_horizon() && p && state && status && active_after && consecutive &&
           adj_state && adj_u_last && grad_u && policy >= TT_POLICY_TRACK && policy <= TT_POLICY_FUZZY;
}

bool window_vjp_args_ok(int B, int N, int k, int Np) {
    return B > 0 && N >= 1 && N <= tt_max_horizon() && Np >= 1 && k >= 0;
}

}  // namespace

extern "C" {

int tt_policy_plant_vjp_device(int B, int N, const tt_plant* p, int policy, const double* state, const int* status,
                               const int* active_before, const int* active_after, const int* consecutive,
                               const double* grad_u_applied, double* adj_state, double* adj_u_last,
                               double* grad_u, double* g_state_noise, void* stream) {
    if (!policy_plant_vjp_args_ok(B, N, p, policy, state, status, active_after, consecutive, adj_state, adj_u_last,
                                  grad_u))
        return -EINVAL;
    return launch_flat(policy_plant_vjp_kernel, "policy_plant_vjp_kernel", B, stream, B, N, *p, policy, state, status,
                       active_before, active_after, consecutive, grad_u_applied, adj_state, adj_u_last, grad_u,
                       g_state_noise);
}

int tt_policy_plant_vjp_model_device(int B, int N, const tt_plant* p, int policy, const double* state,
                                     const int* status, const int* active_before, const int* active_after,
                                     const int* consecutive, const double* grad_u_applied, double* adj_state,
                                     double* adj_u_last, double* grad_u, double* g_state_noise, double* g_model_acc,
                                     void* stream) {
    if (!g_model_acc)
        return tt_policy_plant_vjp_device(B, N, p, policy, state, status, active_before, active_after, consecutive,
                                          grad_u_applied, adj_state, adj_u_last, grad_u, g_state_noise, stream);
    if (!policy_plant_vjp_args_ok(B, N, p, policy, state, status, active_after, consecutive, adj_state, adj_u_last,
                                  grad_u))
        return -EINVAL;
    return launch_flat(policy_plant_vjp_model_kernel, "policy_plant_vjp_model_kernel", B, stream, B, N, *p, policy,
                       state, status, active_before, active_after, consecutive, grad_u_applied, adj_state, adj_u_last,
                       grad_u, g_state_noise, g_model_acc);
}

int tt_sim_window_vjp_device(int B, int N, int k, int Np, const double* g_xref, const double* g_uref, double* g_plan_x,
                             double* g_plan_u, const double* g_x0, const double* grad_state, double* adj_state,
                             const double* g_wq_wr, double* g_wq_wr_acc, double* g_meas_noise, void* stream) {
    if (!window_vjp_args_ok(B, N, k, Np)) return -EINVAL;
    return launch_flat(sim_window_vjp_kernel, "sim_window_vjp_kernel", (long long)B * (N + 1), stream, B, N, k, Np,
                       g_xref, g_uref, g_plan_x, g_plan_u, g_x0, grad_state, adj_state, g_wq_wr, g_wq_wr_acc,
                       g_meas_noise);
}

int tt_sim_window_vjp_fuzzy_device(int B, int N, int k, int Np, const double* g_xref, const double* g_uref,
                                   double* g_plan_x, double* g_plan_u, const double* g_x0, const double* grad_state,
                                   double* adj_state, const double* g_wq_wr, double* g_wq_wr_acc, double* g_meas_noise,
                                   const tt_fuzzy_rule* rule, const double* x_meas, const double* xref,
                                   const int* retried, double* g_rule_acc, void* stream) {
    if (!rule)
        return tt_sim_window_vjp_device(B, N, k, Np, g_xref, g_uref, g_plan_x, g_plan_u, g_x0, grad_state, adj_state,
                                        g_wq_wr, g_wq_wr_acc, g_meas_noise, stream);
    if (!window_vjp_args_ok(B, N, k, Np) || !fuzzy_rule_valid(*rule) || !x_meas || !xref) return -EINVAL;
    const FuzzyVjpArgs fz{*rule, x_meas, xref, retried, g_rule_acc};
    return launch_flat(sim_window_vjp_fuzzy_kernel, "sim_window_vjp_fuzzy_kernel", (long long)B * (N + 1), stream, B, N,
                       k, Np, g_xref, g_uref, g_plan_x, g_plan_u, g_x0, grad_state, adj_state, g_wq_wr, g_wq_wr_acc,
                       g_meas_noise, fz);
}

}  // extern "C"
