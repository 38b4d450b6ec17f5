// Internal interface between the C-ABI layer (tt_api.hip) and the gfx950 kernels (tt_track.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace ttmpc {

// IPOPT's convergence test (OptimalityErrorConvergenceCheck, defaults): besides the scaled error E_0 <= tol, the
// unscaled dual infeasibility, constraint violation and complementarity must be below these (acceptable: the second set)
constexpr double kDualInfTol = 1.0, kConstrViolTol = 1e-4, kComplInfTol = 1e-4;
constexpr double kAccDualInfTol = 1e10, kAccConstrViolTol = 1e-2, kAccComplInfTol = 1e-2;

// Everything one launch needs; passed by value as the kernel argument (< 1 KB).
struct TrackArgs {
    int N, B, max_iter, acc_iter;
    double dt, L1, L2, Mh, tol, acc_tol;
    double Q[36], R[4];                   // row-major, symmetrised in-kernel
    double xlb[6], xub[6], ulb[2], uub[2];  // raw bounds; |b| >= 1e19 or inf = free
    const double* x0;                     // [B][6]
    const double* xref;                   // [B][N+1][6]
    const double* uref;                   // [B][N][2]
    const double* wqwr;                   // [B][8] or nullptr
    const double* zg;                     // [B][8N+6] or nullptr
    double* xout;                         // [B][N+1][6]
    double* uout;                         // [B][N][2]
    double* kkt;                          // [B] or nullptr
    int* status;                          // [B]
    int* iters;                           // [B] or nullptr
    unsigned long long* stamps;           // [B][kNumPhases] cycle sums (TT_STAMPS diagnostic build only)
    double* prow;                         // [B][N+1][kGlobalRows]: the stage rows a build keeps in HBM, or nullptr
    int host_done;                        // 1: status[b] is the instance's completion flag for a polling host (zero-copy
                                          //    host calls): written last, after a system-scope release of the rest
    double* dual;                         // [B][N+1][kDualPerStage]: y 6, z_L 8, z_U 8 per stage (ttmpc.h), or nullptr
};

// phases timed by the TT_STAMPS diagnostic build
// PH_NRIC / PH_NTRIAL: counts (Riccati attempts, line-search trials), not cycles
// PH_X0..PH_X7: sub-phase slots for finer TT_STAMPS instrumentation inside a phase (SUBSTAMP in tt_track.hip)
enum { PH_LOAD = 0, PH_LIN, PH_MU_BAR, PH_RIC, PH_FWD, PH_STEP, PH_MERIT, PH_SOC, PH_UPDATE, PH_NRIC, PH_NTRIAL,
       PH_X0, PH_X1, PH_X2, PH_X3, PH_X4, PH_X5, PH_X6, PH_X7, PH_TOTAL, kNumPhases };

// LDS: fixed head + rows per stage (doubles); see tt_track.hip for the map.
// 116 used + 1 zero pad + 1 unused.  The even stride (= 2 mod 4, 944 B) keeps every stage record 16-B aligned and makes
// the lane-pair phases' reads conflict-free (lanes 2k, 2k+1 -> rows R, R+1 of stage k); bitwise the same as 117, C2
// -2.5 %, C3 -1.7 % (profiles/r04/stride118/).
constexpr int kRowsPerStage = 118;
constexpr int kTrackFilter = 16;  // filter line search entries (theta, phi) kept in the LDS head
constexpr int kHead = 256;  // 64 head values + 32 dump slots + 2x16 filter entries + two 8x8 Riccati tiles
constexpr int kScratch = kHead;
constexpr int kMaxLdsBytes = 160 * 1024;

inline int lds_doubles(int N) { return kRowsPerStage * (N + 1) + kScratch; }
inline int lds_bytes(int N) { return 8 * lds_doubles(N); }
inline int max_horizon() { return (kMaxLdsBytes / 8 - kScratch) / kRowsPerStage - 1; }

// The N = 50 build keeps the 28 stage rows of the Riccati factor (P, p) and of its overlay (Sigma, dB: linearise ..
// ric_prep) in HBM instead of LDS: a 38.8 KB record, four instances per CU instead of three (tt_track.hip, round 6).
constexpr int kGlobalRows = 28;
// bytes of TrackArgs::prow the launch of `a` needs (0: every stage row stays in LDS)
size_t track_global_bytes(const TrackArgs& a);

hipError_t launch_track(const TrackArgs& a, hipStream_t stream);
// the exporting twins of the same builds (tt_track_dual.hip); launch_track forwards to it when a.dual is set
hipError_t launch_track_dual(const TrackArgs& a, hipStream_t stream);

// ---------------- derivatives of a tracking solution (tt_sens.hip, tt_vjp.hip, tt_sens_stage.hpp) ----------------
constexpr int kDualPerStage = 22;  // y 6 | z_L 8 | z_U 8: the stage rows rY .. rZU + 7 of tt_track.hip, in that order
// what both derivative kernels read: the model and the primal-dual point of the solve they differentiate
struct DiffArgs {
    int N, B;
    double dt, L1, L2, Mh;
    double Q[36], R[4];
    double xlb[6], xub[6], ulb[2], uub[2];  // raw bounds (relaxed in-kernel as track_kernel relaxes them)
    const double* x;      // [B][N+1][6]
    const double* u;      // [B][N][2]
    const double* dual;   // [B][N+1][kDualPerStage]
    const int* status;    // [B] of the solve
    const double* wqwr;   // [B][8] or nullptr  (last: with wqwr before status the adjoint kernel's SGPR spills, which
                          //  otherwise all fit VGPR lanes, leave it a 36-byte private segment)
};

// sensitivity to x_init (tt_sens.hip)
struct SensArgs : DiffArgs {
    double* gain;         // [B][2][6] or nullptr
    double* dxdx0;        // [B][N+1][6][6] or nullptr
    double* dudx0;        // [B][N][2][6] or nullptr
    int* sens_status;     // [B] or nullptr
};
// LDS doubles of one instance: 24 per stage (dt*J 9, curvature 7, Sigma 8), 12 per input stage (K), and the tiles
inline int sens_lds_doubles(int N) { return 24 * (N + 1) + 12 * N + 192; }
hipError_t launch_track_sens(const SensArgs& a, hipStream_t stream);

// adjoint: dL/d(x_init, xref, uref, weights) (tt_vjp.hip)
struct VjpArgs : DiffArgs {
    const double* xref;   // [B][N+1][6]; read for g_wqwr only
    const double* uref;   // [B][N][2];   read for g_wqwr only
    const double* gx;     // [B][N+1][6] upstream dL/dX, or nullptr (zeros)
    const double* gu;     // [B][N][2]   upstream dL/dU, or nullptr (zeros)
    double* g_x0;         // [B][6] or nullptr
    double* g_xref;       // [B][N+1][6] or nullptr
    double* g_uref;       // [B][N][2] or nullptr
    double* g_wqwr;       // [B][8] or nullptr
    int* vjp_status;      // [B] or nullptr
};
// LDS doubles of one instance: 33 per stage (the 24 of the sensitivity record, the upstream gradient 8, one pad that
// keeps the stage-parallel phases free of bank conflicts), 12 per input stage (K), and the tiles: 61.3 KB at N = 170
constexpr int kVjpStage = 33, kVjpTiles = 164;
inline int vjp_lds_doubles(int N) { return kVjpStage * (N + 1) + 12 * N + kVjpTiles; }
hipError_t launch_track_vjp(const VjpArgs& a, hipStream_t stream);
// the same adjoint plus dL/d(L1, L2, Mh): the kernel's model instantiation (the same LDS record).  The two members
// sit behind VjpArgs so that the plain instantiation's argument block, and with it its code, stays what it was
struct VjpModelArgs : VjpArgs {
    double* g_model;      // [B][3], never nullptr here
    int accumulate;       // != 0: g_model[b] += (a failed instance adds nothing); 0: g_model[b] = (zeros if failed)
};
hipError_t launch_track_vjp_model(const VjpModelArgs& a, hipStream_t stream);
// the same adjoint plus dL/d(xlb, xub, ulb, uub): the kernel's bounds instantiations (the same LDS record; with
// g_model also set, the model and the bounds gradient of one launch).  The member sits behind VjpModelArgs so that the
// plain and the model instantiations' argument blocks, and with them their code, stay what they were
struct VjpBoundsArgs : VjpModelArgs {
    double* g_bounds;     // [B][16]: lower bounds of (x 6, u 2), then upper bounds; never nullptr here.  g_model may
                          //  be nullptr (then the bounds gradient alone); `accumulate` concerns both
};
hipError_t launch_track_vjp_bounds(const VjpBoundsArgs& a, hipStream_t stream);

}  // namespace ttmpc

namespace ttmpc {

// ---------------- OBCA NLPs (tt_obca.hip) ----------------
constexpr int kObcaMaxM = 16;
constexpr int kObcaThreads = 256;  // one workgroup (4 waves) per instance
constexpr int kObcaMaxFilter = 64;
enum { OBCA_PLAN = 0, OBCA_TRACK = 1 };

// ObcaArgs::opts bits (diagnostics / A-B builds; 0 = IPOPT's algorithm): the same switches as the oracle's TTO_OPT_*
// (PD_BLOCKS: round 2's positive-definite block test instead of the exact block inertia; NO_REFINE: no iterative
// refinement)
enum { OBCA_OPT_NO_RESTO = 1, OBCA_OPT_NO_SOFT_RESTO = 2, OBCA_OPT_NO_LSQ_MULT = 4, OBCA_OPT_PD_BLOCKS = 32,
       OBCA_OPT_NO_REFINE = 64 };

struct ObcaArgs {
    int N, M, B, mode, max_iter, acc_iter, dual_init, opts;
    double dt, L1, L2, Mh, W1, W2, tol, acc_tol, dmin, eq_tol, fin_tol, tfac;
    double Q[36], R[4];
    double xlb[6], xub[6], ulb[2], uub[2];
    double obs[4 * kObcaMaxM];      // cx, cy, w, h
    const double* x0;               // [B][6]
    const double* xgoal;            // [B][6]          (plan mode)
    const double* xref;             // [B][N+1][6]     (track mode)
    const double* uref;             // [B][N][2]       (track mode)
    const double* zg;               // [B][n] reference layout, or nullptr
    double* xout;                   // [B][N+1][6]
    double* uout;                   // [B][N][2]
    double* zout;                   // [B][n] or nullptr
    int* status;                    // [B]
    int* iters;                     // [B] or nullptr
    double* kkt;                    // [B] or nullptr
    double* itout;                  // [B][obca_iterate_len] final primal-dual iterate (diagnostic export) or nullptr
    double* ws;                     // per-instance workspace, obca_ws_doubles(N, M) each
    unsigned long long* stamps;     // [B][kObcaPhases] cycle sums (diagnostics), or nullptr
    // helper workgroups (tt_obca.hip, "helper workgroups"): nhelp extra workgroups after the B instances run the block
    // passes of the instances still solving; board: (B + 1) x kObcaBoardStride words, zeroed before every launch
    unsigned long long* board;
    int nhelp;
    // hand-off diagnostics (ttx_obca_set_handoff_debug): spin limit of an instance waiting for helper chunks in
    // s_memrealtime ticks (0: kSpinTicks, 5 s), and one instance whose hand-offs never complete (-1: none), which
    // forces the TT_HANDOFF_TIMEOUT path (tests/test_gpu_obca.py)
    unsigned long long spin_ticks;
    int fail_b;
    // per-instance scenes (tt_obca_solve_batch_scenes*): row b replaces obs[0..4M) / dmin in the workgroup's LDS copy
    // of this block; nullptr: the value above for every instance.  Written before the launch, never during it
    const double* obs_b;            // [B][M][4] or nullptr
    const double* dmin_b;           // [B] or nullptr
};
constexpr int kObcaBoardStride = 16;  // 128-B line per instance (+ one header line)
// claim word of an instance's board line: epoch << 40 | chunks << 20 | next chunk (20 + 20 bits: a pass of
// N = 100000 at M = 16 has 12,501 chunks, and the claim counter overshoots by at most one per claiming workgroup)
constexpr int kClaimChunkShift = 20;
constexpr unsigned long long kClaimFieldMask = (1ull << kClaimChunkShift) - 1ull;
// phase clocks, then event counters (diagnostics, tools/obca_stamps.py / obca_tail.py): factorisations (inertia
// attempts incl. the SOC and pretend-singular refactorisations), restoration-phase iterations, soft-restoration steps,
// refinement corrections, second-order corrections, pretend-singular re-solves, line-search trial points
enum { OPH_LIN = 0, OPH_COMPL, OPH_FACTOR, OPH_RIC, OPH_FWD, OPH_REC, OPH_TRIAL, OPH_UPD, OPH_RIC_SOFT, OPH_FWD_SOFT, OPH_REF_SWEEP, OPH_REF_REC,
       OPH_REF_STAGE, OPH_TOTAL,
       OCNT_FACTOR, OCNT_RESTO_IT, OCNT_SOFT, OCNT_CORR, OCNT_SOC, OCNT_PRETEND, OCNT_TRIAL, kObcaPhases };

// workspace layout (doubles): stage fields [f][k] then block fields [f][j][k], k in 0..N
constexpr int kObcaStageFields = 353;
constexpr int kObcaBlockFields = 229;
__host__ __device__ inline size_t obca_ws_doubles(int N, int M) {
    return (size_t)(kObcaStageFields + kObcaBlockFields * 2 * M) * (size_t)(N + 1);
}
__host__ __device__ inline size_t obca_n(int N, int M) { return (size_t)N * (8 + 16 * M) + 6 + 16 * M; }
// diagnostic export of the final iterate (include/ttmpc.h tt_obca_iterate_len): 30 per stage, 32 per block, 24 final rows
__host__ __device__ inline size_t obca_iterate_len(int N, int M) { return (size_t)(30 + 64 * M) * (N + 1) + 24; }

hipError_t launch_obca(const ObcaArgs& a, hipStream_t stream);

// adjoint of an MPC+OBCA solve: dL/d(x_init, xref, uref) (tt_obca_vjp.hip).  The DiffArgs head carries the model, the
// weights, the bounds and the solve's status; its x, u, dual and wqwr stay nullptr: the point comes from `iterate`
struct ObcaVjpArgs : DiffArgs {
    int M;
    double W1, W2, eq_tol;
    double obs[4 * kObcaMaxM];  // cx, cy, w, h
    const double* iterate;      // [B][obca_iterate_len(N, M)]
    const double* gx;           // [B][N+1][6] upstream dL/dX, or nullptr (zeros)
    const double* gu;           // [B][N][2]   upstream dL/dU, or nullptr (zeros)
    double* g_x0;               // [B][6] or nullptr
    double* g_xref;             // [B][N+1][6] or nullptr
    double* g_uref;             // [B][N][2] or nullptr
    int* vjp_status;            // [B] or nullptr
    // per-instance scenes (tt_obca_vjp_scenes*): row b replaces obs; nullptr: obs for every b.  (d_min is not an
    // input of the adjoint: it shifts a residual and is in no coefficient of the system)
    const double* obs_b;        // [B][M][4] or nullptr
};
constexpr int kObcaVjpThreads = 256;  // sixteen 16-lane groups: one OBCA block each per round
// LDS doubles of one instance: the adjoint's stage record, the dense 4x4 pose addend and the refinement's fields (87
// per stage), 12 per input stage (K), the tiles, one slot per group and the obstacle list: 43.1 KB at N = 50 for any M
constexpr int kObcaVjpStage = 87;
constexpr int kObcaVjpFixed = kVjpTiles + 16 * (kObcaVjpThreads / 16) + 4 * kObcaMaxM;  // tiles, slots, obstacles
inline int obca_vjp_lds_doubles(int N) { return kObcaVjpStage * (N + 1) + 12 * N + kObcaVjpFixed; }
inline int obca_vjp_max_horizon() {  // (512 bytes stay free for the compiler's own LDS)
    return ((64 * 1024 - 512) / 8 - kObcaVjpFixed - kObcaVjpStage) / (kObcaVjpStage + 12);
}
// the same adjoint plus dL/d(obstacles, d_min, Q, R): the kernel's params instantiation (the same LDS record).  The
// members sit behind ObcaVjpArgs so that the plain instantiation's argument block, and with it its code, stays what it
// was.  The block unknowns (16 per block) are carried across the refinement steps in `work`
struct ObcaVjpParamsArgs : ObcaVjpArgs {
    const double* xref;   // [B][N+1][6]; read for g_Q only
    const double* uref;   // [B][N][2];   read for g_R only
    double* g_obs;        // [B][M][4] (cx, cy, w, h) or nullptr
    double* g_dmin;       // [B] or nullptr
    double* g_Q;          // [B][6][6] or nullptr
    double* g_R;          // [B][2][2] or nullptr
    double* work;         // [B][2M(N+1)][16]: one 128-byte record per block, never nullptr here
};
__host__ __device__ inline size_t obca_vjp_params_work_doubles(int N, int M) { return (size_t)32 * M * (N + 1); }
// the params adjoint plus dL/d(L1, L2, Mh, W1, W2): the kernel's geometry instantiation (the same LDS record and the
// same workspace).  The member sits behind ObcaVjpParamsArgs so that the plain and the params instantiations'
// argument blocks, and with them their code, stay what they were
struct ObcaVjpGeomArgs : ObcaVjpParamsArgs {
    double* g_geom;       // [B][5] (L1, L2, Mh, W1, W2), never nullptr here
};
// one launch for the three instantiations: the widest block, of which each kernel takes its own base (work is needed
// by the params and geometry kinds, g_geom by the geometry kind)
enum ObcaVjpKind { kObcaVjpPlain, kObcaVjpParams, kObcaVjpGeom };
hipError_t launch_obca_vjp(const ObcaVjpGeomArgs& a, ObcaVjpKind kind, hipStream_t stream);

}  // namespace ttmpc
