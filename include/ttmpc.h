/* ttmpc -- MI355X-native batched truck-trailer NMPC solver, C ABI (drop-in boundary).
 *
 * The reference (Avan1ko/car-trailer-mpc) solves one NLP per controller call through CasADi:
 *     sol = self._solver(x0=vars_guess, lbx, ubx, lbg, ubg, p)          python-files/mpc_control.py:80-89
 *     self._solver.stats()['success']                                     python-files/mpc_control.py:106
 * and exposes it to its drivers as
 *     MPCTrackingControl.solve(initial_state, reference_states, reference_inputs)
 *                                                                          python-files/mpc_control.py:67-110
 *     TruckTrailerNMPC.solve(...)                                          python-files/mpc_control_nmpc.py:90-113
 *     MPCTrackingControlFuzzy.solve(...)                                   python-files/mpc_control_fuzzy.py:121-167
 * This library replaces the CasADi/IPOPT call with a batched solve of B independent instances on
 * one GPU.  The Python mirror (car-trailer-mpc_amd/ttmpc) binds it with ctypes; the binding a
 * maintainer adds to the reference is in INTEGRATION.md.
 *
 * Conventions
 *  - plain C types only; every array is C-contiguous float64, instance-major:
 *      x0    [B][nx]            initial_state                      (mpc_control.py:67)
 *      xref  [B][N+1][nx]       reference_states.T                 (p layout, mpc_control.py:45-52, 86)
 *      uref  [B][N][nu]         reference_inputs.T                 (p layout, mpc_control.py:86-87)
 *      wq_wr [B][nx+nu]         fuzzy weights w_q, w_r             (mpc_control_fuzzy.py:54-58) or NULL
 *      z_guess [B][n], n=(nx+nu)N+nx, the reference's interleaved decision vector
 *                               [x0,u0,...,x_{N-1},u_{N-1},x_N]    (trajectory_planning.py:38-58) or NULL
 *                               (NULL = reference-copy guess, mpc_control.py:58-65)
 *      x_out [B][N+1][nx], u_out [B][N][nu]  = states.T / inputs.T of _split_decision_variables
 *                                                                  (trajectory_planning.py:62-84)
 *  - nx = 6 (x, y, theta, psi, phi, v), nu = 2 (a, omega)          (truck_trailer_model.py:4-5)
 *  - bounds: +-HUGE_VAL (or |b| >= 1e19) = free (ca.inf in simulation.py:411-414)
 *  - return value: 0 ok, negative errno-style code on API errors (-EINVAL bad dims/pointers,
 *    -ENOMEM, -EIO HIP error, -ENOSYS not built); text from tt_last_error(handle).
 *  - per-instance status: TT_CONVERGED (IPOPT tol), TT_ACCEPTABLE (acceptable_tol x acc_iter),
 *    TT_MAX_ITER, TT_INFEASIBLE (x_init outside the state box -> x_0 = x_init unsatisfiable),
 *    TT_NONFINITE, TT_STEP_FAILED (inertia correction exceeded IPOPT's max_hessian_perturbation 1e20),
 *    TT_HANDOFF_TIMEOUT (OBCA only: an instance waited longer than the spin limit, 5 s, for the helper workgroups
 *    that run chunks of its block passes; a synchronisation failure of the launch, not a numerical one -- the
 *    outputs are the last iterate, possibly partial; INTEGRATION.md "Helper workgroups").
 *    CasADi's stats()['success'] == (status <= TT_ACCEPTABLE).
 *  - a handle is not thread-safe (like the reference objects, which mutate _last_solution); use
 *    one handle per host thread.  Every host-pointer call (tt_solve_batch, tt_solve_batch_ex, tt_plan_batch,
 *    tt_obca_solve_batch, tt_obca_solve_batch_iterate) is synchronous for its caller: its outputs are complete
 *    when it returns.  A tracking tt_solve_batch of a small batch (B <= 64, N < 64) returns as soon as every
 *    instance has published its outputs to host memory, which can be before its kernel has retired on the
 *    handle's private stream: later host calls on the handle are ordered behind it on that stream and
 *    tt_destroy waits for it, but an asynchronous error of that kernel would be reported by a later call.
 *    tt_solve_batch_ex with any extra output always copies and waits for the stream.  Device-pointer calls
 *    (*_device) are asynchronous on the given HIP stream and return after enqueueing.
 *  - GPU only: there is no CPU fallback; tt_create fails (-ENODEV) without a usable gfx950 device.
 */
#ifndef TTMPC_H
#define TTMPC_H

#ifdef __cplusplus
extern "C" {
#endif

enum { TT_CONVERGED = 0, TT_ACCEPTABLE = 1, TT_MAX_ITER = 2, TT_INFEASIBLE = 3, TT_NONFINITE = 4,
       TT_STEP_FAILED = 5 /* IPOPT Error_In_Step_Computation: delta_w > max_hessian_perturbation (1e20) */,
       TT_HANDOFF_TIMEOUT = 6 /* OBCA helper hand-off timed out (no IPOPT counterpart; see above) */ };

enum {
    TT_VARIANT_TRACK = 0,      /* MPCTrackingControl       mpc_control.py       (max_iter 5000, tol 1e-8)  */
    TT_VARIANT_TRACK_OBCA = 1, /* MPCTrackingControlObs    mpc_control_obs.py   (max_iter 5000, tol 1e-8)  */
    TT_VARIANT_NMPC = 2,       /* TruckTrailerNMPC         mpc_control_nmpc.py  (tol 1e-3, acc 1e-2 x5)    */
    TT_VARIANT_FUZZY = 3,      /* MPCTrackingControlFuzzy  mpc_control_fuzzy.py (tol 1e-3, per-instance w) */
    TT_VARIANT_OBCA_PLAN = 4   /* TrajectoryOptimization   trajectory_optimization.py (max_iter 5000)      */
};

typedef struct {
    int nx, nu, N, M;                 /* nx=6, nu=2, horizon N (params['horizon']), obstacles M       */
    double dt, L1, L2, Mh, W1, W2;    /* params dict keys dt, L1, L2, M, W1, W2 (simulation.py:391)  */
    int variant;                      /* TT_VARIANT_*                                                 */
    double tol, acc_tol;              /* IPOPT tol / acceptable_tol (<=0 -> variant default)          */
    int max_iter, acc_iter;           /* IPOPT max_iter / acceptable_iter (<=0 -> variant default)    */
    int warm_shift_compat;            /* reserved: warm-shift guesses are built host-side (ttmpc.nlp) */
    int dual_init;                    /* OBCA variants: 1 = start mu/lam from the separating-axis
                                         certificate of each body/obstacle pair at the guess pose,
                                         0 = from z_guess's mu/lam as the reference does            */
} tt_config;

/* Replaces the controller constructors (mpc_control.py:6-15 -> _build_solver 27-56; the CasADi
 * graph + IPOPT object).  Q: nx*nx row-major, R: nu*nu row-major (symmetrised), bounds nx / nu.
 * obstacles: M*4 (cx, cy, w, h) or NULL.  device: HIP device ordinal (>= 0). */
int tt_create(const tt_config* cfg, const double* Q, const double* R, const double* xlb, const double* xub,
              const double* ulb, const double* uub, const double* obstacles, int device, void** handle);

/* Replaces the per-call IPOPT solve + split (mpc_control.py:67-110) for B instances at once.
 * Host pointers; synchronous.  kkt_res (may be NULL): IPOPT's scaled optimality error at exit. */
int tt_solve_batch(void* handle, int B, const double* x0, const double* xref, const double* uref,
                   const double* wq_wr, const double* z_guess, double* x_out, double* u_out, int* status,
                   int* iters, double* kkt_res);

/* Same with DEVICE pointers (already resident in HBM), enqueued on `stream` (hipStream_t; NULL = the
 * default stream, as in every HIP API -- e.g. torch's default stream); asynchronous.  Used by the bench
 * and by device-resident callers. */
int tt_solve_batch_device(void* handle, int B, const double* d_x0, const double* d_xref, const double* d_uref,
                          const double* d_wq_wr, const double* d_z_guess, double* d_x_out, double* d_u_out,
                          int* d_status, int* d_iters, double* d_kkt_res, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Multipliers and first-order sensitivities of a tracking solve (TT_VARIANT_TRACK, _NMPC, _FUZZY; an OBCA
 * handle returns -EINVAL).  CasADi's `sol` carries lam_g and lam_x next to x; these calls return the same
 * multipliers, and the sensitivity of the solution to the measured state x_init that a parametric-NLP user
 * (sIPOPT, advanced-step NMPC) takes from the same KKT factorisation.
 *
 * dual [B][N+1][22], tt_track_dual_len(N) = 22 (N+1) doubles per instance; per stage k = 0..N:
 *     y_k   (6)  multiplier of the equality row whose left side is x_k:  x_0 - x_init for k = 0, else
 *                x_k - x_{k-1} - dt f(x_{k-1}, u_{k-1})                  (the reference's g, trajectory_planning.py:28-36)
 *     z_L   (8)  multipliers of the lower bounds of (x_k 6, u_k 2)
 *     z_U   (8)  multipliers of the upper bounds
 *   The u entries are 0 at k = N, entries of free variables are 0, and an instance with status TT_INFEASIBLE has
 *   all zeros.  Sign convention: IPOPT's and CasADi's,  grad f + J' y - z_L + z_U = 0,  z >= 0  (so CasADi's
 *   lam_g = y and lam_x = z_U - z_L; the Python mirror's layout.casadi_multipliers reorders them).  They are the
 *   solver's final iterate: multipliers of the bounds relaxed by IPOPT's bound_relax_factor (1e-8), at a point
 *   that meets IPOPT's stopping test, not exact multipliers of an exact optimum.
 *
 * Sensitivities, as sIPOPT defines them: the Newton matrix of the primal-dual system at the returned point,
 * solved for a unit perturbation of the x_0 - x_init row (one Riccati pass, no regularisation):
 *     gain   [B][2][6]        du_0 / dx_init   (the feedback gain K: u_0(x_init + d) ~ u_0 + K d)
 *     dxdx0  [B][N+1][6][6]   dx_k / dx_init   (k = 0: the identity)
 *     dudx0  [B][N][2][6]     du_k / dx_init   (k = 0: the gain)
 *     sens_status [B]         0 ok; 1 a reduced input Hessian was not positive definite or a value was not
 *                             finite (the sensitivity is undefined there); 2 the solve's status is above
 *                             TT_ACCEPTABLE (skipped).  For 1 and 2 the instance's three arrays are zeroed.
 *   First order only: a variable sitting on a bound has (numerically) zero sensitivity and stays there; the
 *   active set is taken as fixed.
 *
 * Every member of tt_track_extra may be NULL; extra == NULL or all members NULL is exactly the plain call.
 * A sensitivity output without `dual` keeps the multipliers in a buffer of the handle (grown, never shrunk:
 * like the other workspaces, calls on one handle must be serialised on ONE stream).  The solve, the export
 * and the sensitivity kernel are enqueued on the same stream in that order.
 * tt_solve_batch_ex: host pointers (also inside `extra`), synchronous.  tt_solve_batch_ex_device: device
 * pointers inside a host-side struct, asynchronous on `stream`.  tt_track_sens_device: the sensitivity alone
 * from device arrays x [B][N+1][6], u [B][N][2], dual, wq_wr (the solve's, or NULL) and status of an earlier
 * tt_solve_batch_ex_device; the same kernel, so bitwise the fused call's outputs. */
typedef struct { double* dual; double* gain; double* dxdx0; double* dudx0; int* sens_status; } tt_track_extra;
long long tt_track_dual_len(int N);
int tt_solve_batch_ex(void* handle, int B, const double* x0, const double* xref, const double* uref,
                      const double* wq_wr, const double* z_guess, double* x_out, double* u_out, int* status,
                      int* iters, double* kkt_res, const tt_track_extra* extra);
int tt_solve_batch_ex_device(void* handle, int B, const double* d_x0, const double* d_xref, const double* d_uref,
                             const double* d_wq_wr, const double* d_z_guess, double* d_x_out, double* d_u_out,
                             int* d_status, int* d_iters, double* d_kkt_res, const tt_track_extra* d_extra,
                             void* stream);
int tt_track_sens_device(void* handle, int B, const double* d_x, const double* d_u, const double* d_dual,
                         const double* d_wq_wr, const int* d_status, double* d_gain, double* d_dxdx0,
                         double* d_dudx0, int* d_sens_status, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Reverse mode (vector-Jacobian product) of a tracking solve: for a scalar loss L(X, U) over the outputs of a
 * solve, its gradient with respect to the solve's inputs x_init, xref, uref and wq_wr in one pass.  Same
 * variants as above (an OBCA handle returns -EINVAL), same Newton matrix K = [[W + Sigma, J'], [J, 0]] at the
 * returned primal-dual point, same definition as sIPOPT's sensitivity ds/dtheta = -K^-1 dF/dtheta.  K is
 * symmetric, so with the upstream gradient g = dL/d(X, U):
 *     K (lam_z, lam_y) = (g, 0),     dL/dtheta = -lam' dF/dtheta          (one Riccati pass, no regularisation)
 *
 * Inputs: x [B][N+1][6], u [B][N][2], dual [B][N+1][22], wq_wr [B][8] or NULL and status [B] exactly as
 * tt_solve_batch_ex* returned or took them, xref [B][N+1][6] and uref [B][N][2] of that solve, and
 *     grad_x [B][N+1][6]  dL/dx_k          grad_u [B][N][2]  dL/du_k
 *   A NULL grad_x or grad_u stands for zeros; both NULL is -EINVAL.
 * Outputs (tt_track_vjp_out; every member may be NULL):
 *     g_x0    [B][6]        dL/dx_init
 *     g_xref  [B][N+1][6]   dL/dxref_k = 2 Q_w lam_x,k   (row k = 0 is exactly 0: x_0 is pinned to x_init)
 *     g_uref  [B][N][2]     dL/duref_k = 2 R_w lam_u,k
 *     g_wq_wr [B][8]        dL/dwq_i (6), dL/dwr_i (2), Q_w = diag(wq) Q_s diag(wq), R_w likewise, Q_s the
 *                           symmetrised Q.  With wq_wr == NULL the weights are ones and this is the gradient with
 *                           respect to such a diagonal scaling of Q and R.  xref and uref are read for this
 *                           output only (without it they may be NULL).
 *     vjp_status [B]        as sens_status: 0 ok; 1 a reduced input Hessian was not positive definite or a value
 *                           (an upstream gradient entry included) was not finite; 2 the solve's status is above
 *                           TT_ACCEPTABLE (skipped).  For 1 and 2 the instance's four arrays are zeroed, so a
 *                           failed instance contributes nothing to a batch gradient.
 *   Signs: the arrays are gradients of L (descent moves a parameter against them); a positive g_x0 entry means
 *   L grows with that x_init entry.
 *   First order only, as above: the active set is taken as fixed, and a variable sitting on a bound carries
 *   (numerically) zero lam, so a loss on it has no gradient in these inputs: it goes to the bound itself
 *   (tt_track_vjp_bounds below).
 *
 * tt_track_vjp_device: device pointers (inside the host-side struct too), asynchronous on `stream`.  It uses
 * no buffer of the handle, so it may run on any stream, also beside a solve of the same handle on another
 * stream; the caller orders it behind the solve whose outputs it reads.  tt_track_vjp: the same with host
 * pointers, synchronous (it stages through a buffer of the handle: one host call per handle at a time). */
typedef struct { double* g_x0; double* g_xref; double* g_uref; double* g_wq_wr; int* vjp_status; } tt_track_vjp_out;
int tt_track_vjp_device(void* handle, int B, const double* d_x, const double* d_u, const double* d_dual,
                        const double* d_xref, const double* d_uref, const double* d_wq_wr, const int* d_status,
                        const double* d_grad_x, const double* d_grad_u, const tt_track_vjp_out* d_out, void* stream);
int tt_track_vjp(void* handle, int B, const double* x, const double* u, const double* dual, const double* xref,
                 const double* uref, const double* wq_wr, const int* status, const double* grad_x,
                 const double* grad_u, const tt_track_vjp_out* out);

/* The same adjoint with the gradient in the model geometry theta = (L1, L2, Mh) of the handle (tt_config, or the
 * last tt_set_model).  Only the dynamics rows c_{k+1} = x_{k+1} - x_k - dt f(x_k, u_k) and the -A_k' y_{k+1} part of
 * the stationarity rows depend on theta, so with lam of the same solve K (lam_z, lam_y) = (g, 0)
 *     dL/dtheta = dt sum_{k<N} [ lam_x,k' (dJ_f(x_k)/dtheta)' y_{k+1} + lam_y,k+1' df(x_k, u_k)/dtheta ],
 * closed forms in rows 2, 3 of f and five entries of J_f.  lam_y comes from the x-rows of K behind the forward
 * sweep (lam_y,N = gX_N - H_N lam_x,N; lam_y,k = gX_k - H_k lam_x,k + A_k' lam_y,k+1): no second factorisation,
 * the same LDS record (track_vjp_kernel's model instantiation, tt_vjp.hip).  dt is not a parameter here.
 *     g_model [B][3]        dL/dL1, dL/dL2, dL/dMh per instance; the sum over B for the geometry the batch shares
 *                           is the caller's, as for g_Q and g_R of the LQR adjoint
 *   accumulate == 0: g_model[b] = value, zeros for vjp_status 1 and 2.  accumulate != 0: g_model[b] += value (one
 *   writer per instance, no atomics); a failed instance adds nothing.  accumulate concerns g_model only.
 *   g_model == NULL: the call is tt_track_vjp[_device] (the same kernel instantiation, the same bits); with it the
 *   other four arrays and vjp_status are bitwise what that call writes.
 * tt_track_vjp_model: host pointers, synchronous, as tt_track_vjp (with accumulate the host's g_model is read). */
typedef struct { double* g_x0; double* g_xref; double* g_uref; double* g_wq_wr;
                 double* g_model;   /* [B][3]  dL/dL1, dL/dL2, dL/dMh per instance */
                 int* vjp_status; } tt_track_vjp_model_out;
int tt_track_vjp_model_device(void* handle, int B, const double* d_x, const double* d_u, const double* d_dual,
                              const double* d_xref, const double* d_uref, const double* d_wq_wr, const int* d_status,
                              const double* d_grad_x, const double* d_grad_u, const tt_track_vjp_model_out* d_out,
                              int accumulate, void* stream);
int tt_track_vjp_model(void* handle, int B, const double* x, const double* u, const double* dual, const double* xref,
                       const double* uref, const double* wq_wr, const int* status, const double* grad_x,
                       const double* grad_u, const tt_track_vjp_model_out* out, int accumulate);

/* The geometry of a tracking handle (TT_VARIANT_TRACK, _NMPC, _FUZZY) without rebuilding it.  tt_set_model applies
 * tt_create's validation (L1, L2 > 0, Mh finite; else -EINVAL and the handle keeps its values); an OBCA handle returns
 * -EINVAL (its geometry also enters the H-representations).  It changes host-side state only: L1, L2 and Mh are
 * launch arguments of every kernel of the handle (solves, their exporting twins, the sensitivity and adjoint kernels,
 * host and device entry points alike), so every later call runs with the new values and a solve is bitwise that of
 * a fresh handle created with them.  Calls on one handle stay serialised as before: work already enqueued keeps
 * the values it was launched with, and so does a captured graph (hipGraph, ClosedLoop.run_graph): capture again
 * after a change.  tt_get_model reads the current values (NULL pointers are skipped). */
int tt_set_model(void* handle, double L1, double L2, double Mh);
int tt_get_model(void* handle, double* L1, double* L2, double* Mh);

/* The same adjoint with the gradient in the box (xlb, xub, ulb, uub) of the handle (tt_create, or the last
 * tt_set_bounds).  The bounds enter F only through z_L = mu / (v - l_rel) and z_U = mu / (u_rel - v) (l_rel, u_rel:
 * the relaxed bounds l - 1e-8 max(1, |l|), u + 1e-8 max(1, |u|)), so with lam of the same solve K (lam_z, lam_y) = (g, 0)
 *     dL/dl_v = rho_l sum_k Sigma_L,k,v lam_k,v,      dL/du_v = rho_u sum_k Sigma_U,k,v lam_k,v,
 * Sigma_L = z_L / (v - l_rel) and Sigma_U = z_U / (u_rel - v) the two halves of Sigma, rho the derivative of the
 * relaxation (1 -+ 1e-8 sign(bound) beyond |bound| > 1, else 1); the sums run over the stages k >= 1 for a state
 * bound (x_0 is pinned to x_init) and k < N for an input bound.  This is where the loss on a saturated variable goes:
 * on a hard-active bound Sigma is huge, lam = g / Sigma, and the product is the upstream gradient g itself.  An inactive
 * bound's entry is mu / slack^2 lam, numerically zero; a weakly active bound's entry depends on the final mu.  First
 * order, as above: a bound that becomes active or inactive inside a step of the bound is a kink.
 *     g_bounds [B][16]      dL/dxlb (6), dL/dulb (2), dL/dxub (6), dL/duub (2) per instance: the order of z_L | z_U in
 *                           the multiplier export; the sum over B for the box the batch shares is the caller's.  The
 *                           entry of a bound the solver treats as infinite (not finite, or beyond +-1e19) is exactly 0.
 *   accumulate: as for tt_track_vjp_model, and it concerns g_model and g_bounds only (zeros or an untouched
 *   accumulator for vjp_status 1 and 2).
 *   g_bounds == NULL: the call is tt_track_vjp_model[_device] (the same kernel instantiation, the same bits); with it
 *   the other arrays (g_model included, which may be NULL) and vjp_status are bitwise what that call writes.  One
 *   launch either way (track_vjp_kernel's bounds instantiations, tt_vjp.hip): no second factorisation, the same LDS
 *   record.
 * tt_track_vjp_bounds: host pointers, synchronous, as tt_track_vjp_model. */
typedef struct { double* g_x0; double* g_xref; double* g_uref; double* g_wq_wr; double* g_model;
                 double* g_bounds;  /* [B][16]  dL/d(xlb 6, ulb 2, xub 6, uub 2) per instance */
                 int* vjp_status; } tt_track_vjp_bounds_out;
int tt_track_vjp_bounds_device(void* handle, int B, const double* d_x, const double* d_u, const double* d_dual,
                               const double* d_xref, const double* d_uref, const double* d_wq_wr, const int* d_status,
                               const double* d_grad_x, const double* d_grad_u, const tt_track_vjp_bounds_out* d_out,
                               int accumulate, void* stream);
int tt_track_vjp_bounds(void* handle, int B, const double* x, const double* u, const double* dual, const double* xref,
                        const double* uref, const double* wq_wr, const int* status, const double* grad_x,
                        const double* grad_u, const tt_track_vjp_bounds_out* out, int accumulate);

/* The box of a tracking handle (TT_VARIANT_TRACK, _NMPC, _FUZZY) without rebuilding it: xlb, xub [6], ulb, uub [2], raw
 * bounds as tt_create takes them (not finite, or beyond +-1e19: free).  tt_set_bounds applies tt_create's validation (no
 * NaN, lb <= ub; else -EINVAL and the handle keeps its values); an OBCA handle returns -EINVAL.  It changes host-side
 * state only: the box is a launch argument of every kernel of the handle, and the tracking kernel's build (the MPC
 * pattern, the OBCA pattern, or the one that reads its bound pattern at run time) is chosen from it at every launch.
 * So every later call, host or device, zero-copy or not, runs with the new box, and a solve is bitwise that of a fresh
 * handle created with it, also when the change moves the handle from one build to another.  Calls on one handle stay
 * serialised as before: work already enqueued keeps the box it was launched with, and so does a captured graph
 * (hipGraph, ClosedLoop.run_graph): capture again after a change.  tt_get_bounds reads the current values (NULL
 * pointers are skipped). */
int tt_set_bounds(void* handle, const double* xlb, const double* xub, const double* ulb, const double* uub);
int tt_get_bounds(void* handle, double* xlb, double* xub, double* ulb, double* uub);

/* Replaces TrajectoryOptimization.plan (trajectory_optimization.py:311-331) for B scenarios of a
 * TT_VARIANT_OBCA_PLAN handle.  x0, xgoal [B][6] (ca.vertcat(initial_state, goal_state), 316-323);
 * z_guess [B][n], n = N(8+16M)+6+16M, the reference's interleaved [x_k,u_k,mu_k,lam_k] vector
 * (55-91), built host-side as _hybrid_a_star_initial_trajectory does (227-274), or NULL for
 * _generate_initial_trajectory_guess (209-225).  Host pointers; synchronous.  Like plan(), success is
 * reported (status) but never enforced (326-331). */
int tt_plan_batch(void* handle, int B, const double* x0, const double* xgoal, const double* z_guess,
                  double* x_out, double* u_out, int* status, int* iters);

/* Both OBCA variants with every output: z_out [B][n] (x, u, mu, lam; _split_decision_variables,
 * trajectory_optimization.py:277-309) and the scaled KKT error.  Plan variant: xgoal [B][6], xref/uref
 * NULL.  MPC+OBCA variant (mpc_control_obs.py:290-322): xref [B][N+1][6], uref [B][N][2], xgoal NULL;
 * z_guess NULL = _get_initial_guess (216-239).  x_out/u_out/z_out/iters/kkt may be NULL. */
int tt_obca_solve_batch(void* handle, int B, const double* x0, const double* xgoal, const double* xref,
                        const double* uref, const double* z_guess, double* x_out, double* u_out, double* z_out,
                        int* status, int* iters, double* kkt_res);
/* Same with DEVICE pointers, asynchronous on `stream` (NULL = the default stream).  The solver
 * workspace belongs to the handle (grown, never shrunk, when B exceeds its capacity): calls on one
 * handle must be serialised on ONE stream; use one handle per stream for concurrent solves. */
int tt_obca_solve_batch_device(void* handle, int B, const double* d_x0, const double* d_xgoal, const double* d_xref,
                               const double* d_uref, const double* d_z_guess, double* d_x_out, double* d_u_out,
                               double* d_z_out, int* d_status, int* d_iters, double* d_kkt_res, void* stream);
/* decision-vector length n of the OBCA variants, and device workspace bytes one instance needs */
long long tt_obca_n(int N, int M);
long long tt_obca_workspace_bytes(int N, int M);
/* Diagnostic variants of the two calls above that also export each instance's FINAL PRIMAL-DUAL ITERATE, so that
 * IPOPT's optimality error can be re-evaluated independently at the returned point (tests; the reference's IPOPT keeps
 * these multipliers internal -- CasADi returns only their lam_x / lam_g combinations).  iterate_out [B][L],
 * L = tt_obca_iterate_len(N, M) = 30(N+1) + 64M(N+1) + 24 doubles:
 *   per stage k = 0..N (30): x 6, u 2, z_L(x) 6, z_U(x) 6, z_L(u) 2, z_U(u) 2, y of the 6 dynamics rows
 *                            (u, z_L(u), z_U(u) are 0 at k = N);
 *   per OBCA block (k, j), j = 2 obstacle + body, in k-major order (32): mu|lam 8, their bound multipliers 8,
 *                            the 4 rows' slacks s, slack-bound multipliers v_L, v_U and row multipliers y_d;
 *   final-box rows (24, plan variant; zeros otherwise): slacks, v_L, v_U, y of x_N - x_goal.
 * The multipliers are IPOPT's internal ones (bound multipliers >= 0 of the relaxed bounds; rows of the slack form
 * d(x) - s = 0). */
long long tt_obca_iterate_len(int N, int M);
int tt_obca_solve_batch_iterate(void* handle, int B, const double* x0, const double* xgoal, const double* xref,
                                const double* uref, const double* z_guess, double* x_out, double* u_out, double* z_out,
                                int* status, int* iters, double* kkt_res, double* iterate_out);
int tt_obca_solve_batch_iterate_device(void* handle, int B, const double* d_x0, const double* d_xgoal,
                                       const double* d_xref, const double* d_uref, const double* d_z_guess,
                                       double* d_x_out, double* d_u_out, double* d_z_out, int* d_status, int* d_iters,
                                       double* d_kkt_res, double* d_iterate_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Reverse mode (vector-Jacobian product) of an MPC+OBCA solve (TT_VARIANT_TRACK_OBCA): for a scalar loss L(X, U) over
 * the outputs of a solve, its gradient with respect to x_init, xref and uref in one pass.  The definition is the
 * tracking adjoint's: with K the Newton matrix of the barrier problem at the exported primal-dual iterate (over
 * x, u, the OBCA duals w, the row slacks s | the dynamics and OBCA row multipliers; bound multipliers eliminated into
 * Sigma with the solver's relaxed bounds) and the upstream gradient g = dL/d(X, U),
 *     K lam = (g, 0),     dL/dtheta = -lam' dF/dtheta.
 * Every OBCA block (w 8, s 4, y_d 4) is eliminated onto the pose (X, Y, theta, psi) of its stage by a partially
 * pivoted elimination, the stage system is solved by one un-regularised Riccati pass, and three refinement steps on
 * the un-condensed system follow (obca_vjp_kernel).
 *
 * Inputs: iterate [B][tt_obca_iterate_len(N, M)] and status [B] exactly as tt_obca_solve_batch_iterate* returned
 * them, and
 *     grad_x [B][N+1][6]  dL/dx_k          grad_u [B][N][2]  dL/du_k
 *   A NULL grad_x or grad_u stands for zeros; both NULL is -EINVAL.  Obstacles, geometry, bounds, Q and R are the
 *   handle's.  xref and uref are not inputs: no output needs them.
 * Outputs (tt_obca_vjp_out; every member may be NULL):
 *     g_x0    [B][6]        dL/dx_init
 *     g_xref  [B][N+1][6]   dL/dxref_k = 2 Q lam_x,k   (row k = 0 is exactly 0: x_0 is pinned to x_init)
 *     g_uref  [B][N][2]     dL/duref_k = 2 R lam_u,k
 *     vjp_status [B]        0 ok; 1 a block pivot or a reduced input Hessian failed, or a value (an upstream gradient
 *                           entry included) was not finite; 2 the solve's status is above TT_ACCEPTABLE (skipped).
 *                           For 1 and 2 the instance's three arrays are zeroed, so a failed instance contributes
 *                           nothing to a batch gradient.
 *   Signs: the arrays are gradients of L (descent moves a parameter against them).
 *   First order only, the active set fixed: an obstacle row that is active stays active, one that is not stays out,
 *   and a variable sitting on a bound carries (numerically) zero lam.
 *   Only TT_VARIANT_TRACK_OBCA: a plan handle and a tracking handle return -EINVAL.  Gradients with respect to the
 *   obstacles, d_min, Q and R come from tt_obca_vjp_params* below; those with respect to the geometry (L1, L2, M, W1,
 *   W2) from tt_obca_vjp_geometry*.  The horizon must keep the instance's record in 64 KB of LDS
 *   (N <= 76), else -EINVAL.
 *
 * tt_obca_vjp_device: device pointers (inside the host-side struct too), asynchronous on `stream`.  It uses no buffer
 * of the handle, so it may run on any stream; the caller orders it behind the solve whose iterate it reads.
 * tt_obca_vjp: the same with host pointers, synchronous (it stages through a buffer of the handle: one host call per
 * handle at a time). */
typedef struct { double* g_x0; double* g_xref; double* g_uref; int* vjp_status; } tt_obca_vjp_out;
int tt_obca_vjp_device(void* handle, int B, const double* d_iterate, const int* d_status, const double* d_grad_x,
                       const double* d_grad_u, const tt_obca_vjp_out* d_out, void* stream);
int tt_obca_vjp(void* handle, int B, const double* iterate, const int* status, const double* grad_x,
                const double* grad_u, const tt_obca_vjp_out* out);

/* The same adjoint plus the gradient with respect to the scene and the weights (tt_obca_vjp_params_out; every member
 * may be NULL; the first four are tt_obca_vjp_out's):
 *     g_obstacles [B][M][4]  dL/d(cx, cy, w, h) of every obstacle      g_dmin [B]  dL/dd_min
 *     g_Q [B][6][6], g_R [B][2][2]  gradients in the raw entries given to tt_create (which symmetrises), so
 *                                   g_Q[a][b] = -sum_k (lam_x,k[a] e_k[b] + lam_x,k[b] e_k[a]), e_k = x_k - xref_k
 *   With v the 16 entries of lam of one block (stage k >= 1, obstacle m, body), y_d1 and lam the block's iterate values
 *   and b = (cx + w/2, cy + h/2, -cx + w/2, -cy + h/2) the obstacle's half-space offsets, only row 1 of the block
 *   (g' mu - (A p - b)' lam + d_min - s_1 = 0) and the stationarity rows of lam depend on b and d_min, linearly:
 *     g_b[i] = -sum (y_d1 v_lam[i] + lam[i] v_yd1),   g_dmin = -sum v_yd1,
 *     g_cx = g_b0 - g_b2, g_cy = g_b1 - g_b3, g_w = (g_b0 + g_b2) / 2, g_h = (g_b1 + g_b3) / 2.
 *   On a face contact g_cx = -g_dmin and g_w = g_dmin / 2: moving the face and widening the margin are one motion.
 *   The block unknowns are carried across the refinement steps in d_work ([B] x tt_obca_vjp_params_work_bytes(N, M),
 *   one 128-byte record per block; contents undefined afterwards): recomputing them from the final pose adjoint loses
 *   three to four digits where a row is active.  The x0 / xref / uref members agree with tt_obca_vjp's to
 *   rounding, not bitwise.
 *   xref, uref: as given to the solve; read for g_Q and g_R only (NULL while one of those is wanted: -EINVAL).
 *   d_work NULL: -EINVAL.  Failed or skipped instances get zeros in every array.  Only TT_VARIANT_TRACK_OBCA, N <= 76.
 * tt_obca_vjp_params_device uses no buffer of the handle; tt_obca_vjp_params stages through the handle (its work
 * buffer included), synchronous. */
typedef struct { double* g_x0; double* g_xref; double* g_uref; int* vjp_status;
                 double* g_obstacles; double* g_dmin; double* g_Q; double* g_R; } tt_obca_vjp_params_out;
long long tt_obca_vjp_params_work_bytes(int N, int M);  /* per instance */
int tt_obca_vjp_params_device(void* handle, int B, const double* d_iterate, const int* d_status, const double* d_xref,
                              const double* d_uref, const double* d_grad_x, const double* d_grad_u,
                              const tt_obca_vjp_params_out* d_out, void* d_work, void* stream);
int tt_obca_vjp_params(void* handle, int B, const double* iterate, const int* status, const double* xref,
                       const double* uref, const double* grad_x, const double* grad_u,
                       const tt_obca_vjp_params_out* out);

/* The scene of an OBCA handle (both variants) without rebuilding it: obstacles M x (cx, cy, w, h) (M is fixed at
 * tt_create; NULL keeps them) and the safety margin d_min (default 0.2; NULL keeps it).  Applies to every later call;
 * a handle that never calls it solves bitwise as before.  -EINVAL on a tracking handle, on a non-finite value, on
 * w or h <= 0 and on d_min < 0 (nothing is changed then).  tt_get_scene: either pointer may be NULL. */
int tt_set_scene(void* handle, const double* obstacles, const double* d_min);
int tt_get_scene(void* handle, double* obstacles, double* d_min);

/* ---------------------------------------------------------------------------------------------
 * Per-instance scenes: every instance of one launch solves against its own obstacle list and its own d_min.  They
 * replace one handle per scene with B = 1 solves (Monte-Carlo over obstacle layouts, a per-instance safety margin).
 * M stays the handle's: pad a shorter list with far-away obstacles.
 *     obstacles [B][M][4] (cx, cy, w, h), or NULL: the handle's obstacles for every instance
 *     d_min     [B],                      or NULL: the handle's d_min for every instance
 * A NULL struct, or both members NULL, is exactly the call without scenes.  With every row equal to the handle's scene
 * the results are bitwise those of the call without scenes, and row b's results are bitwise those of a B = 1 call on a
 * handle whose tt_set_scene got row b.
 *
 * tt_obca_solve_batch_scenes / _device: tt_obca_solve_batch_iterate / _device (both OBCA variants; iterate_out may be
 *   NULL) plus the scenes.  The host entry validates every scene by tt_set_scene's rule (finite, w, h > 0, d_min finite
 *   and >= 0): -EINVAL, nothing launched, no output written.  The device entry cannot read device memory on the host:
 *   each instance checks its own row when it starts, and one that fails ends with status TT_NONFINITE, 0 iterations and
 *   the initial guess in its outputs; the other instances are unaffected.  A tracking handle: -EINVAL.
 * tt_obca_vjp_scenes / _device: tt_obca_vjp_params / _device plus the scenes the solve was given (the adjoint reads the
 *   obstacles only: d_min is in no coefficient of its system).  With g_obstacles, g_dmin, g_Q, g_R (and, on the device
 *   entry, d_work) all NULL they run tt_obca_vjp's kernel and need no work buffer; otherwise tt_obca_vjp_params's.
 *   g_obstacles [B][M][4] and g_dmin [B] are then the gradient in each instance's OWN scene: the caller sums nothing.
 *   The host entry validates as above.  An instance the solve ended with TT_NONFINITE is skipped (vjp_status 2, zeros).
 * tt_collision_scenes_device: tt_collision_device with obstacles [B][M][4], instance b against its own list. */
typedef struct { const double* obstacles; /* [B][M][4] (cx, cy, w, h), or NULL: the handle's */
                 const double* d_min;     /* [B], or NULL: the handle's */ } tt_obca_scenes;
int tt_obca_solve_batch_scenes(void* handle, int B, const double* x0, const double* xgoal, const double* xref,
                               const double* uref, const double* z_guess, double* x_out, double* u_out, double* z_out,
                               int* status, int* iters, double* kkt_res, double* iterate_out,
                               const tt_obca_scenes* scenes);
int tt_obca_solve_batch_scenes_device(void* handle, int B, const double* d_x0, const double* d_xgoal,
                                      const double* d_xref, const double* d_uref, const double* d_z_guess,
                                      double* d_x_out, double* d_u_out, double* d_z_out, int* d_status, int* d_iters,
                                      double* d_kkt_res, double* d_iterate_out, const tt_obca_scenes* d_scenes,
                                      void* stream);
int tt_obca_vjp_scenes(void* handle, int B, const double* iterate, const int* status, const double* xref,
                       const double* uref, const double* grad_x, const double* grad_u,
                       const tt_obca_vjp_params_out* out, const tt_obca_scenes* scenes);
int tt_obca_vjp_scenes_device(void* handle, int B, const double* d_iterate, const int* d_status, const double* d_xref,
                              const double* d_uref, const double* d_grad_x, const double* d_grad_u,
                              const tt_obca_vjp_params_out* d_out, void* d_work, const tt_obca_scenes* d_scenes,
                              void* stream);

/* The same adjoint plus the gradient with respect to the geometry the batch shares (tt_obca_vjp_geometry_out: the
 * eight members of tt_obca_vjp_params_out, then g_geometry):
 *     g_geometry [B][5]  dL/d(L1, L2, Mh, W1, W2) per instance, at the handle's current geometry; the sum over B is
 *                        the caller's
 *   dL/dtheta = -lam' dF/dtheta at the exported iterate.  Two parts of F depend on theta.  The dynamics rows and the
 *   -A_k' y_{k+1} part of the x-stationarity rows (L1, L2, Mh): tt_track_vjp_model's sum
 *   dt sum_{k<N} [lam_x,k' (dJ_f/dtheta)' y_{k+1} + lam_y,k+1' df/dtheta] with this solve's lam.  And of every block
 *   (stage k >= 1, obstacle m, body) the d_min row d_0, through g = (L/2, W/2, L/2, W/2) and through the body centre
 *   p (truck: rear axle + L1/2 along the heading; trailer: rear axle - Mh along the heading - L2/2 along the trailer);
 *   with l_b = y_d0 d_0 and v the block's 16 entries of lam its share is
 *   -[(lam_pose, v_w)' d/dtheta grad_(pose, w) l_b + v_yd0 dd_0/dtheta]; truck blocks feed L1 and W1, trailer blocks
 *   L2, Mh and W2.  The block terms are read from the carried v (d_work, as tt_obca_vjp_params).
 *   With g_geometry NULL the calls are tt_obca_vjp_scenes / _device: the same kernel, the same bits.  With it set the
 *   other eight outputs are bitwise what tt_obca_vjp_scenes* writes with a work buffer, and d_work is needed (NULL:
 *   -EINVAL).  Failed or skipped instances get zeros.  Only TT_VARIANT_TRACK_OBCA, N <= 76.
 * tt_obca_vjp_geometry_device uses no buffer of the handle; tt_obca_vjp_geometry stages through the handle (its work
 * buffer included), synchronous. */
typedef struct { double* g_x0; double* g_xref; double* g_uref; int* vjp_status;
                 double* g_obstacles; double* g_dmin; double* g_Q; double* g_R;
                 double* g_geometry; /* [B][5] dL/d(L1, L2, Mh, W1, W2) per instance */ } tt_obca_vjp_geometry_out;
int tt_obca_vjp_geometry_device(void* handle, int B, const double* d_iterate, const int* d_status,
                                const double* d_xref, const double* d_uref, const double* d_grad_x,
                                const double* d_grad_u, const tt_obca_vjp_geometry_out* d_out, void* d_work,
                                const tt_obca_scenes* d_scenes /* NULL: the handle's */, void* stream);
int tt_obca_vjp_geometry(void* handle, int B, const double* iterate, const int* status, const double* xref,
                         const double* uref, const double* grad_x, const double* grad_u,
                         const tt_obca_vjp_geometry_out* out, const tt_obca_scenes* scenes);

/* The geometry of an OBCA handle (both variants) without rebuilding it: the lengths L1, L2, the hitch offset Mh and
 * the widths W1, W2, which are the dynamics' parameters and the H-representations of the two bodies.  tt_create's
 * validation: L1, L2, W1, W2 finite and > 0, Mh finite, else -EINVAL and nothing is changed.  Host-side state only:
 * every later solve and adjoint of the handle is bitwise that of a fresh handle created with these values; work already
 * enqueued keeps the old ones.  A tracking handle: -EINVAL (it has tt_set_model, which keeps refusing OBCA handles).
 * tt_get_geometry: any pointer may be NULL. */
int tt_set_geometry(void* handle, double L1, double L2, double Mh, double W1, double W2);
int tt_get_geometry(void* handle, double* L1, double* L2, double* Mh, double* W1, double* W2);

/* ---------------------------------------------------------------------------------------------
 * Closed-loop simulation step, device pointers, asynchronous on `stream`.
 * The per-timestep glue of python-files/simulation.py:484-531 around the solve, batched over B
 * Monte-Carlo instances so that the whole loop stays in HBM:
 *   window -> [collision check] -> [warm start] -> tt_solve_batch_device -> [record] -> plant update.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    double dt, L1, L2, Mh, W1, W2;     /* params dict (simulation.py:391-397)                         */
    int enable;                        /* ENABLE_DISTURBANCES (simulation.py:21): 0 = update(q, u, p) */
    double friction_coeff;             /* DISTURBANCE_PARAMS (simulation.py:26-32)                    */
    double slippage_coeff;
    double process_noise_std;          /* std of the measurement noise the caller draws (509-513)     */
    double lateral_slip_gain;
    double slip_angle_max;
} tt_plant;

/* Reference window at step k with end padding (simulation.py:486-501) from a plan of Np inputs
 * (plan_x [P][Np+1][6], plan_u [P][Np][2]; P = 1 shared plan or B per-instance plans), and the
 * measured state x_meas = state + meas_noise (simulation.py:509-513; meas_noise NULL = exact state;
 * x_meas NULL = skip).  Outputs xref [B][N+1][6], uref [B][N][2]. */
int tt_sim_window_device(int B, int N, int k, int Np, const double* plan_x, const double* plan_u, int per_instance,
                         const double* state, const double* meas_noise, double* x_meas, double* xref, double* uref,
                         void* stream);
/* Graph-replayable closed-loop step (hipGraph capture of window -> check -> solve -> plant -> log):
 * the step index lives on the device.  tt_sim_window_indexed_device reads k = ks[*step] (the reference's
 * step sequence, precomputed host-side) and the measurement noise noise_all[*step] ([K][B][6] or NULL);
 * tt_sim_log_advance_device writes S[*step+1] = state [K+1][B][6], Ua[*step] = u_applied [K][B][2], the
 * status / iterations / collision flag [K][B] (iters, flag may be NULL), then increments *step. */
int tt_sim_window_indexed_device(int B, int N, const int* ks, const int* step, int Np, const double* plan_x,
                                 const double* plan_u, int per_instance, const double* state, const double* noise_all,
                                 double* x_meas, double* xref, double* uref, void* stream);
int tt_sim_log_advance_device(int B, int* step, const double* state, const double* u_applied, const int* status,
                              const int* iters, const int* flag, double* S, double* Ua, int* Ss, int* Si, int* Sc,
                              void* stream);
/* check_trajectory_collision (simulation.py:363-385) of K poses per instance, pose (b, j) at
 * poses + b*stride_b + j*stride_k (doubles; x, y, theta, psi first), against M axis-aligned obstacles
 * (device [M][4]: cx, cy, w, h).  flag[b] = 1 if any pose's truck or trailer touches an obstacle. */
int tt_collision_device(int B, int K, const double* poses, long long stride_b, int stride_k, const double* obstacles,
                        int M, const tt_plant* p, int* flag, void* stream);
/* The same with per-instance obstacle lists (device [B][M][4]): instance b is tested against obstacles + b*4M. */
int tt_collision_scenes_device(int B, int K, const double* poses, long long stride_b, int stride_k,
                               const double* obstacles, int M, const tt_plant* p, int* flag, void* stream);
/* update(q, u, params[, DISTURBANCE_PARAMS]) (simulation.py:167-199) in place on state [B][6] with
 * u = u[b*u_stride + 0..1] (u_out of a solve: u_stride = 2N applies inputs[:, 0]).  zero_on_fail:
 * instances with status > TT_ACCEPTABLE apply zero control (simulation_nmpc.py:204-214).
 * u_applied [B][2] (may be NULL) receives the control before friction/slippage scaling. */
int tt_plant_update_device(int B, const tt_plant* p, double* state, const double* u, long long u_stride,
                           const int* status, int zero_on_fail, double* u_applied, void* stream);
/* Closed-loop failure policy of the driver, fused with the plant update (one launch per step):
 * success (status <= TT_ACCEPTABLE): u = u[b*u_stride + 0..1], u_last = u, consecutive = 0.  Failure:
 * failures++, consecutive++, then TT_POLICY_TRACK applies u as returned (simulation.py:519-527),
 * TT_POLICY_NMPC zero control and u_last = 0, stop after 20 consecutive (simulation_nmpc.py:206-216),
 * TT_POLICY_FUZZY u_last, zero after 15 consecutive, stop after 30 (simulation_fuzzy.py:207-221).
 * Stopping (the reference's `break` before update) clears active[b]; inactive instances keep their state.
 * u_last [B][2], consecutive / failures / active [B] are device state owned by the caller (active = 1 and
 * the rest 0 at the start); u_applied [B][2] (may be NULL) receives the applied control. */
enum { TT_POLICY_TRACK = 0, TT_POLICY_NMPC = 1, TT_POLICY_FUZZY = 2 };
int tt_policy_plant_device(int B, const tt_plant* p, int policy, double* state, const double* u, long long u_stride,
                           const int* status, double* u_last, int* consecutive, int* failures, int* active,
                           double* u_applied, void* stream);
/* The NMPC and fuzzy drivers' plant (simulation_nmpc.py:94-105, simulation_fuzzy.py:94-105): the same update plus
 * the process noise inside the plant, q_ += state_noise * dt right after the Euler step (before the lateral slip);
 * those drivers solve from the exact state (no measurement noise).  state_noise [B][6] device, drawn by the caller
 * (the reference draws N(0, process_noise_std) in apply_disturbances), or NULL = none (then identical to the
 * functions above). */
int tt_plant_update_noise_device(int B, const tt_plant* p, double* state, const double* u, long long u_stride,
                                 const int* status, int zero_on_fail, const double* state_noise, double* u_applied,
                                 void* stream);
int tt_policy_plant_noise_device(int B, const tt_plant* p, int policy, double* state, const double* u,
                                 long long u_stride, const int* status, double* u_last, int* consecutive, int* failures,
                                 int* active, const double* state_noise, double* u_applied, void* stream);
/* _compute_fuzzy_weights (mpc_control_fuzzy.py:90-119) per instance from the measured state x [B][6]
 * and the window's reference xref [B][N+1][6] (speed of stage 0): wq_wr [B][8] = (q0..q5, r0, r1), the
 * per-instance weights of a TT_VARIANT_FUZZY solve. */
int tt_fuzzy_weights_device(int B, int N, const double* x, const double* xref, double* wq_wr, void* stream);
/* NMPC / fuzzy warm start (mpc_control_nmpc.py:90-100): z_guess [B][8N+6] = shift(last) where have[b],
 * else the reference-copy guess from xref / uref.  bug_compatible = the reference's last-stage slicing
 * (mpc_control_nmpc.py:83-84). */
int tt_warm_start_device(int B, int N, const double* last, const int* have, const double* xref, const double* uref,
                         int bug_compatible, double* z_guess, void* stream);
/* After a solve: last[b] = pack(x_out[b], u_out[b]) and have[b] = 1 where status <= TT_ACCEPTABLE
 * (the reference keeps _last_solution only on success, mpc_control_nmpc.py:107-111). */
int tt_record_solution_device(int B, int N, const double* x_out, const double* u_out, const int* status, double* last,
                              int* have, void* stream);
/* do_interpolation (simulation.py:201-218) of B plans: state_traj [B][Np+1][6], input_traj [B][Np][2]
 * -> [B][factor*Np+1][6], [B][factor*Np][2]; factor = floor(dt_1 / dt_2) (OBCA dt 0.1 -> MPC 0.05: 2). */
int tt_interpolate_device(int B, int Np, int factor, const double* state_traj, const double* input_traj,
                          double* state_out, double* input_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Reverse mode of the closed loop: the adjoints of the glue around the solve, for a backward sweep over a taped
 * run (ttmpc.simulation.ClosedLoop.run_tape / backward).  With S (K+1 states), Ua (K applied controls) the logs
 * and GS = dL/dS, GU = dL/dUa, the sweep carries a = dL/dS_{t+1} [B][6] and abar = the adjoint of u_last [B][2]
 * (a = GS[K], abar = 0 at the start) and does, for t = K-1 .. 0:
 *     tt_policy_plant_vjp_device   plant and failure-policy adjoint: a <- J_q' a, seed g_u0, abar
 *     tt_sim_window_device         xref_t, uref_t again (they are not taped)
 *     tt_track_vjp_device          on step t's taped x, u, dual, status with grad_x = NULL, grad_u = the buffer
 *                                  whose row 0 holds g_u0 (rows 1.. zeroed once by the caller)
 *     tt_sim_window_vjp_device     a += g_x0 + GS[t], weight and plan gradients accumulated
 *       (a rule loop: tt_sim_window_vjp_fuzzy_device, which first sends the solve's g_wq_wr through the adjoint of
 *        the fuzzy weight rule into g_x0[3] and the rule parameters; the window call before it also rebuilds x_meas)
 * and dL/dx_init = a at the end.  Device pointers, asynchronous on `stream`, no atomics: two sweeps over one
 * tape give the same bits.  Both calls return -EINVAL for B <= 0 or N outside 1..tt_max_horizon().
 *
 * tt_policy_plant_vjp_device: the adjoint of tt_policy_plant[_noise]_device for one step, one instance per thread.
 *   state [B][6] is S_t (before the step), status [B] the step's solve status, active_before / active_after [B] the
 *   `active` flags before (NULL: all 1, the first step) and after the step, consecutive [B] the consecutive-failure
 *   count after the step, grad_u_applied [B][2] = GU[t] or NULL.  The applied control itself is not needed: the
 *   plant is linear in it.  With J_q = dS_{t+1}/dS_t, J_u = dS_{t+1}/du_t (u_t before the friction / slippage
 *   scaling) and c = J_u' a + GU[t]:
 *       branch                                        g_u0      abar
 *       not active before the step, or stopped in it  0         unchanged (TT_POLICY_NMPC: 0 on the stopping step)
 *       success (status <= TT_ACCEPTABLE)             c + abar  0
 *       failure, TT_POLICY_TRACK                      c         unchanged   (tt_track_vjp_device zeroes a failed
 *                                                                            instance: nothing to differentiate)
 *       failure, TT_POLICY_NMPC                       0         0           (u_last was overwritten with 0)
 *       failure, TT_POLICY_FUZZY, count <= 15         0         abar + c    (u_last was re-applied)
 *       failure, TT_POLICY_FUZZY, count > 15          0         unchanged
 *   and a <- J_q' a for every instance that moved; a stopped instance keeps a.  adj_state [B][6] = a and
 *   adj_u_last [B][2] = abar are updated in place; g_u0 goes to grad_u[b * 2N + 0..1] (row 0 of a [B][N][2] array).
 *   g_state_noise [B][6] (may be NULL) receives dL/d(state_noise) = dt a, taken before the J_q product, for the
 *   in-plant noise of tt_policy_plant_noise_device (0 for a stopped instance).
 *   Kinks: d|x|/dx = sign(x) with 0 at 0 (the |phi| |v| terms of the slip factor and of the lateral slip);
 *   d min(s, 0.3)/ds = 1 for s < 0.3 and 0 otherwise.  Plain IEEE arithmetic without contraction, as the plant.
 *
 * tt_sim_window_vjp_device: the adjoint of tt_sim_window_device at step index k plus the step's accumulation.
 *   g_xref [B][N+1][6], g_uref [B][N][2] (tt_track_vjp_device's) are scatter-added into the per-instance plan
 *   gradients g_plan_x [B][Np+1][6], g_plan_u [B][Np][2] with the forward's end padding: state row j to plan row
 *   min(k+j, Np), input row j to min(k+j, Np-1) while k < Np (for k >= Np the input window is zeros and nothing
 *   reaches g_plan_u).  Each plan row is written by one thread; the rows that the padding folds onto the last plan
 *   row are summed in ascending j first.  A shared plan's gradient is the sum of the [B] slices (the caller's).
 *   Then, per instance: adj_state += g_x0 + grad_state (GS[t]), g_wq_wr_acc [B][8] += g_wq_wr, and g_meas_noise
 *   [B][6] = g_x0 (the measurement noise enters x_meas = S_t + n_t).  Accumulators are `+=` into buffers the
 *   caller zeroes.  Every pointer may be NULL (that part is skipped). */
int tt_policy_plant_vjp_device(int B, int N, const tt_plant* p, int policy, const double* state, const int* status,
                               const int* active_before, const int* active_after, const int* consecutive,
                               const double* grad_u_applied, double* adj_state, double* adj_u_last, double* grad_u,
                               double* g_state_noise, void* stream);
int tt_sim_window_vjp_device(int B, int N, int k, int Np, const double* g_xref, const double* g_uref, double* g_plan_x,
                             double* g_plan_u, const double* g_x0, const double* grad_state, double* adj_state,
                             const double* g_wq_wr, double* g_wq_wr_acc, double* g_meas_noise, void* stream);
/* tt_policy_plant_vjp_device plus the plant's share of the gradient in its geometry (L1, L2, Mh of tt_plant):
 *     g_model_acc [B][3] += a' dS_{t+1}/dtheta = dt slip (a_2 df_2/dtheta + a_3 df_3/dtheta),
 * a = adj_state before the J_q product and slip the forward's factor (the lateral-slip and friction terms do not
 * depend on the geometry).  An accumulator the caller zeroes; stopped and inactive instances add nothing.  The sum
 * over the steps of a sweep is dL/d(plant geometry) per instance; the controller's share comes from
 * tt_track_vjp_model_device.  g_model_acc == NULL is tt_policy_plant_vjp_device, the same kernel and bits. */
int tt_policy_plant_vjp_model_device(int B, int N, const tt_plant* p, int policy, const double* state,
                                     const int* status, const int* active_before, const int* active_after,
                                     const int* consecutive, const double* grad_u_applied, double* adj_state,
                                     double* adj_u_last, double* grad_u, double* g_state_noise, double* g_model_acc,
                                     void* stream);

/* ---------------------------------------------------------------------------------------------
 * The fuzzy weight rule as data, and its adjoint.  tt_fuzzy_weights_device evaluates the rule of
 * mpc_control_fuzzy.py:90-119 with the reference's constants; here they are a struct, so that a closed loop can be
 * differentiated with respect to them (ttmpc.simulation.ClosedLoop(fuzzy_rule=...), backward(rule=True)).
 * The first seven fields, in this order, are the differentiable rule vector theta; w_min, w_max and v_rev are
 * settings without a gradient (at the defaults the clip bounds sit on a kink, and v_rev is a switch).
 * With psi = x[3], v = x[5], ref_v = xref[0][5], for one instance:
 *     s = |psi| / psi_full,  h = min(s, 1),  rev = (ref_v < v_rev) or (v < v_rev)
 *     per channel c in {hitch, steer, rate}:  f_c = rev ? rev_c : 1,  raw_c = (1 + gain_c h) f_c,
 *                                             m_c = max(1.0, raw_c),  w_c = min(max(m_c, w_min), w_max)
 *     wq_wr = (1, 1, w_steer, w_hitch, w_steer, 1, 1, w_rate)
 * Adjoint, for the upstream g_w [8]: G_steer = g_w[2] + g_w[4], G_hitch = g_w[3], G_rate = g_w[7],
 * pass_c = (raw_c > 1) and (w_min < m_c < w_max), in = (s < 1), d|x|/dx = sign(x) with 0 at 0:
 *     g_psi      = sum_c G_c pass_c gain_c f_c in sign(psi) / psi_full
 *     g_psi_full = -sum_c G_c pass_c gain_c f_c in |psi| / psi_full^2
 *     g_gain_c   = G_c pass_c h f_c
 *     g_rev_c    = G_c pass_c (rev ? 1 + gain_c h : 0)
 * and zero for every other input: v and ref_v only switch, the constant channels carry nothing.  The adjoint is
 * plain IEEE arithmetic without contraction, as the plant adjoint; no atomics.
 * ------------------------------------------------------------------------------------------- */
typedef struct { double psi_full;                          /* 0.35 */
                 double gain_hitch, gain_steer, gain_rate; /* 2.0, 1.2, 1.5 */
                 double rev_hitch, rev_steer, rev_rate;    /* 1.1, 1.1, 1.2 */
                 double w_min, w_max, v_rev;               /* 1.0, 3.5, -0.1: no gradient */ } tt_fuzzy_rule;
/* tt_fuzzy_weights_device for a rule; rule == NULL means the defaults, and with the defaults the weights are
 * bitwise those of tt_fuzzy_weights_device. */
int tt_fuzzy_weights_rule_device(int B, int N, const tt_fuzzy_rule* rule, const double* x, const double* xref,
                                 double* wq_wr, void* stream);
/* The rule's adjoint alone, one instance per thread: g_x [B][6] gets g_x[b][3] += g_psi, g_rule_acc [B][7] += the
 * theta gradients (an accumulator the caller zeroes).  retried [B] (may be NULL: none): an instance with
 * retried[b] != 0 adds nothing, because its accepted solve used unit weights.  Any pointer may be NULL (that part is
 * skipped). */
int tt_fuzzy_weights_vjp_device(int B, int N, const tt_fuzzy_rule* rule, const double* x, const double* xref,
                                const int* retried, const double* g_wq_wr, double* g_x, double* g_rule_acc,
                                void* stream);
/* tt_sim_window_vjp_device for a step whose weights came from the rule, w_t = rule(x_meas_t, xref_t[0]): the thread
 * that does the per-instance accumulation first applies the rule adjoint to g_x0 (as it reads it; the buffer itself is
 * not written), then accumulates, so adj_state and g_meas_noise receive the rule's term and g_rule_acc [B][7] the
 * theta gradients, and a backward step stays four launches.  Bitwise "tt_fuzzy_weights_vjp_device on g_x0, then
 * tt_sim_window_vjp_device".  The rule part needs g_x0 and g_wq_wr; x_meas [B][6] and xref [B][N+1][6] are the step's.
 * rule == NULL is tt_sim_window_vjp_device: the same kernel and bits.
 * All three return -EINVAL for B <= 0, N outside 1..tt_max_horizon(), a non-finite rule, psi_full <= 0 or
 * w_min > w_max. */
int tt_sim_window_vjp_fuzzy_device(int B, int N, int k, int Np, const double* g_xref, const double* g_uref,
                                   double* g_plan_x, double* g_plan_u, const double* g_x0, const double* grad_state,
                                   double* adj_state, const double* g_wq_wr, double* g_wq_wr_acc, double* g_meas_noise,
                                   const tt_fuzzy_rule* rule, const double* x_meas, const double* xref,
                                   const int* retried, double* g_rule_acc, void* stream);

/* lqr_distance (LQR_cost.py:7-41) for B instances: A, B of the forward-Euler map at (x_goal, u_goal),
 * P = DARE(A, B, Q, R) symmetrised, score[b] = (x_cur - x_goal)' P (x_cur - x_goal).  Q (6x6), R (2x2) are
 * HOST row-major arrays; x_cur, x_goal [B][6], u_goal [B][2] (may be NULL: the map is linear in u) are device
 * pointers.  P_out [B][36] and iters [B] (doublings used, -1 = not converged in 64) may be NULL. */
int tt_lqr_score_device(int B, const tt_plant* p, const double* Q, const double* R, const double* x_cur,
                        const double* x_goal, const double* u_goal, double* P_out, double* score, int* iters,
                        void* stream);

/* Reverse mode of tt_lqr_score_device: for a scalar loss L(score, P) over its outputs, the gradient with respect
 * to x_cur, x_goal, Q and R in one launch (lqr_vjp_kernel), at the P the forward returned (the DARE is not rerun).
 * With B = dt [e5 e4] (constant), K = (R + B'PB)^-1 B'PA and Ac = A - BK, the DARE differentiates at its
 * stabilising solution to
 *     dP = Ac' dP Ac + M,     M = dQ + K' dR K + dA' P Ac + Ac' P dA.
 * The upstream gradients gs = dL/dscore and GP = dL/dP combine to G = gs dx dx' + (GP + GP')/2 (the forward
 * symmetrises P; dx = x_cur - x_goal), one discrete Lyapunov equation S = Ac S Ac' + G is solved by Smith doubling
 * (S <- S + T S T', T <- T^2 from S = G, T = Ac; the forward's stopping rule, at most 64 doublings; S symmetrised
 * once at the end), and
 *     g_x_cur  [B][6]    2 gs P dx
 *     g_x_goal [B][6]    -2 gs (P dx)[m] + dt sum_ij (dL/dA)_ij d2f_i/dq_j dq_m,   dL/dA = 2 P Ac S
 *     g_Q      [B][36]   S        symmetric: the gradient for a symmetric Q, i.e. <g_Q, dQ> for a symmetric dQ
 *     g_R      [B][4]    K S K'   symmetric, in the same sense
 *     vjp_status [B]     0 ok; 1 undefined: a value (an upstream gradient included) was not finite,
 *                        det(R + B'PB) <= 0, or the doubling did not converge in 64; 2 skipped: fwd_iters[b] < 0
 *                        (the forward's DARE did not converge).  For 1 and 2 the instance's four arrays are zeros.
 *     iters    [B]       the Lyapunov doublings run (0 for a skipped instance)
 * Every member of tt_lqr_vjp_out may be NULL.  The gradients are per instance: the sum over B for a Q and R shared
 * by the batch is the caller's.  The model parameters (tt_plant) get no gradient, and u_goal does not enter, as in
 * the forward.
 * Inputs: R HOST 2x2 row-major; x_cur, x_goal [B][6], P [B][36] (the forward's P_out) device; fwd_iters [B] (the
 * forward's iters) device or NULL; grad_score [B], grad_P [B][36] device, either may be NULL and stands for zeros.
 * Returns -EINVAL for B < 0, a NULL p, R or out, a singular R (the forward's check), and, for B > 0, a NULL x_cur,
 * x_goal or P or both upstream gradients NULL; B = 0 returns 0.  Asynchronous on `stream`; no handle, no shared
 * buffer, no atomics: two launches on the same inputs give the same bits. */
typedef struct { double* g_x_cur; double* g_x_goal; double* g_Q; double* g_R;
                 int* vjp_status; int* iters; } tt_lqr_vjp_out;
int tt_lqr_score_vjp_device(int B, const tt_plant* p, const double* R, const double* x_cur, const double* x_goal,
                            const double* P, const int* fwd_iters, const double* grad_score, const double* grad_P,
                            const tt_lqr_vjp_out* out, void* stream);

void tt_destroy(void* handle);
const char* tt_last_error(void* handle);

/* Introspection: LDS bytes one instance needs at horizon N; max horizon supported; version. */
int tt_lds_bytes(int N);
int tt_max_horizon(void);
const char* tt_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TTMPC_H */
