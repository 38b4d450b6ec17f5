// Adjoint (vector-Jacobian product) of an MPC+OBCA solution on gfx950 (tt_obca_vjp_device).
//
// For a scalar loss L(X, U) with upstream gradient g = (gX, gU) the gradient with respect to x_init, xref and uref
// comes from ONE solve with the Newton matrix K of the barrier problem at the exported primal-dual iterate
// (ttmpc.h tt_obca_iterate_len), the bound multipliers eliminated into Sigma:
//   K lam = (g, 0);   dL/dx_init = lam_y,0;   dL/dxref_k = 2 Q lam_x,k;   dL/duref_k = 2 R lam_u,k.
// Unknowns per stage: x 6, u 2 and, per OBCA block (obstacle x body), the duals w 8, the row slacks s 4 and the row
// multipliers y_d 4; a block couples to the pose (X, Y, theta, psi) of its stage only.
//
// Block phase.  One 16-lane group per block, sixteen blocks per round over the flat block index f = k 2M + j (from
// f = 2M: x_0 is pinned, so the blocks of stage 0 do not enter).  Lane r builds row r of
//   [ K_b | C ],   K_b = [[W_ww + Sigma_w, 0, J_w'], [0, Sigma_s, -I], [J_w, -I, 0]],   C = [H_wx; 0; J_x]
// at (x_k, w, y_d) in registers (Sigma_w = z_w / (w + 1e-8); Sigma_s from v_L, v_U and the relaxed row bounds: rows 0
// and 3 below +1e-8, rows 1, 2 inside -+(eq_tol + 1e-8)).  The group eliminates with partial pivoting (the pivot row is the
// lane with the largest entry of the column among the lanes not yet used; rows never move), back-substitutes the four
// right-hand sides and reduces the pose addend H_xx - C' K_b^-1 C with a butterfly.  The addends of a round go through
// one LDS slot per group and are added to their stages in block order by sixteen lanes: no atomics, so a launch is
// deterministic.
//
// Stage phase.  track_vjp_kernel's sweeps (tt_sens_stage.hpp, tt_vjp.hip) with the dense 4x4 pose addend in the stage
// Hessian 2 Q + Sigma_x - dt curvature(y_{k+1}): one backward Riccati pass with the vector lanes, one forward vector
// sweep, a stage-parallel output phase.  All 256 threads walk the sweeps; the lanes above 55 only meet the barriers.
// An active block puts entries of 1e13 on P, so B' P B can be close to rank one: with the addend the sweep's 2x2
// solves eliminate on the larger diagonal instead of dividing by the determinant.
//
// Refinement.  The float64 pass over such entries loses 1e-7 .. 1e-4 relative, so kRefine = 3 refinement steps on the
// un-condensed system follow (three digits per step on the hardest golden window).  In each a block pass factors K_b
// again (factor_rows: the same pivoting, the multipliers kept in place), recovers v = -K_b^-1 C lx_pose, forms the block rows' residual r = -(C lx_pose + K_b v) against the
// un-eliminated rows and t = K_b^-1 r, and leaves per stage w = sum_b (H_xx lx_pose + C' v) and fold = -sum_b C' t.
// lam_y comes from the x-rows (ly_k = gX_k - H0_k lx_k - w_k + A_k' ly_{k+1}), so only the input rows
// (ru_k = gU_k - R_k lu_k + B' ly_{k+1}) and the folded block rows carry a residual; the same two sweeps on
// (fold, ru) give the correction, and dL/dx_init = ly_0 + the last correction's p_0.
//
// LDS: 87 doubles per stage (the adjoint's record 33, the addend 16, the refinement's fields 38), 12 per input stage,
// 164 tile doubles, 256 slot doubles and the 64 obstacle doubles: 43.1 KB at N = 50 for any M.  No buffer of the handle
// is used.  Plain IEEE arithmetic, no contraction: tests/obca_vjp_reference.py (model_obca_vjp) is the numpy model.
//
// The params instantiation (tt_obca_vjp_params_device) also forms dL/d(obstacles, d_min, Q, R).  Only row 1 of a block
// and the stationarity rows of lam depend on the obstacle's offsets b and on d_min, linearly, so the gradients are sums
// over the blocks of entries of v, the block's 16 entries of lam.  Recomputing v from the final pose adjoint loses three
// to four digits where a row is active (v_yd1 is 4e13 times a 1e-12 component of the pose adjoint), so this
// instantiation CARRIES v across the refinement steps (carry_block): u = v + t per block in a caller-provided HBM
// workspace, one 128-byte record per block; a pass takes v = u - K_b^-1 C dlx_pose with the last correction, then the
// residual against that v; one closing pass after the last step applies the last correction and reduces the blocks'
// five terms per obstacle in block order (slots, then registers: no atomics, no LDS beyond the record above).
// tests/obca_scene_reference.py (model_scene_vjp) is its numpy model.
//
// The geometry instantiation (tt_obca_vjp_geometry_device) is the params one plus dL/d(L1, L2, Mh, W1, W2), for a
// geometry the batch shares.  Two parts of F depend on it.  Of a block only the d_min row d_0 does (build_row,
// cls == 3, i == 0): linearly through g = (hl, hw, hl, hw) and through the body centre p, so the closing pass forms
// the block's two (truck: L1, W1) or three (trailer: L2, W2, Mh) terms from the carried v, the stage's pose adjoint and
// the block's iterate values (geometry_block_terms) and reduces them in flat block order as the scene terms: slot
// entries 5 .. 7, then one register in each of five fixed threads, no atomics.  The dynamics rows and the
// -A_k' y_{k+1} part of the x-rows (L1, L2, Mh) give tt_vjp.hip's model_gradient sum with this solve's lam: the final
// lx (sL) and the last step's ly (sY; only ly_0 is corrected again, and the numpy model meets the cap with it), the
// stage terms through the dead w field, summed over k by three of the five threads.  Same LDS record, same workspace;
// the other outputs are bitwise the params instantiation's.  tests/obca_geometry_reference.py (model_geometry_vjp) is
// its numpy model.
#include <math.h>

#include <type_traits>

#include "tt_kernel.hpp"
#include "tt_sens_stage.hpp"

#pragma clang fp contract(off)

namespace ttmpc {
namespace {

using sens::sAJ;
using sens::sSG;
using sens::d_idx;

constexpr int kT = kObcaVjpThreads, kGL = 16, kGroups = kT / kGL;
struct Layout {
    static constexpr bool kVec = true;
    // the sensitivity record (24) | g 8 | one spare | dense pose addend 16 | the refinement's fields (below)
    static constexpr int kStage = kObcaVjpStage;
    static constexpr int sG = 24, sDH = 33;
    static constexpr int tP = 0, tM = 36, tA = 72, tQW = 108, tRW = 144, tPV0 = 148, tPV1 = 154, tKP = 160;
};
constexpr int kStage = Layout::kStage, sG = Layout::sG, sDH = Layout::sDH, tQW = Layout::tQW, tRW = Layout::tRW;
// refinement: Sigma 8 and gU 2 as linearised (the sweeps overwrite them), the blocks' pose sums w 4 | fold 4, the first
// solve's lx | lu 8, lam_y 6, gX 6 (the correction's right-hand side takes its place in g)
constexpr int sSV = 49, sGU = 57, sW = 59, sF = 63, sL = 67, sY = 75, sGX = 81;
constexpr int kRefine = 3;  // steps: the golden window with active rows gains three digits per step
static_assert(Layout::tKP + 2 <= kVjpTiles && sDH + 16 <= sSV && sGX + 6 <= kStage, "layout");

__device__ __forceinline__ void zero_outputs(const ObcaVjpArgs& a, int b, int tid) {
    const int N = a.N, S = N + 1;
    if (a.g_x0)
        for (int t = tid; t < 6; t += kT) a.g_x0[(size_t)b * 6 + t] = 0.0;
    if (a.g_xref)
        for (int t = tid; t < S * 6; t += kT) a.g_xref[(size_t)b * S * 6 + t] = 0.0;
    if (a.g_uref)
        for (int t = tid; t < N * 2; t += kT) a.g_uref[(size_t)b * N * 2 + t] = 0.0;
}

// Row r (0 .. 15: w 8, s 4, y_d 4) of [K_b | C] of block j at pose xk and the block's iterate q (w 8, z_w 8, s 4,
// v_L 4, v_U 4, y_d 4) into row[20]; hxx: the three nonzeros (2,2), (2,3), (3,3) of H_xx.  The expressions are those of
// the solver's block linearisation (oracle/c/tt_obca.c blk_lin restates them on the CPU).
__device__ __forceinline__ void build_row(const ObcaVjpArgs& p, const double* obs, const double* xk, int j,
                                          const double* q, int r, double (&row)[20], double (&hxx)[3]) {
    const double X = xk[0], Y = xk[1], th = xk[2], ps = xk[3];
    double st, ct;
    sincos(th, &st, &ct);
    double ca, sa, angp, hl, hw, p0, p1, dpt0, dpt1, dpp0, dpp1, ppt0, ppt1, ptp0, ptp1, ppp0, ppp1;
    if ((j & 1) == 0) {  // truck: centre = rear axle + L1/2 (cos th, sin th)
        const double h1 = 0.5 * p.L1;
        ca = ct; sa = st; angp = 0.0; hl = 0.5 * p.L1; hw = 0.5 * p.W1;
        p0 = X + h1 * ct; p1 = Y + h1 * st;
        dpt0 = -h1 * st; dpt1 = h1 * ct;
        dpp0 = 0.0; dpp1 = 0.0;
        ppt0 = -h1 * ct; ppt1 = -h1 * st;
        ptp0 = ptp1 = ppp0 = ppp1 = 0.0;
    } else {  // trailer: centre = hitch - L2/2 (cos(th+psi), sin(th+psi)), hitch = rear axle - M (cos th, sin th)
        const double h2 = 0.5 * p.L2, M = p.Mh;
        sincos(th + ps, &sa, &ca);
        angp = 1.0; hl = 0.5 * p.L2; hw = 0.5 * p.W2;
        p0 = X - M * ct - h2 * ca; p1 = Y - M * st - h2 * sa;
        dpt0 = M * st + h2 * sa; dpt1 = -M * ct - h2 * ca;
        dpp0 = h2 * sa; dpp1 = -h2 * ca;
        ppt0 = M * ct + h2 * ca; ppt1 = M * st + h2 * sa;
        ptp0 = h2 * ca; ptp1 = h2 * sa;
        ppp0 = h2 * ca; ppp1 = h2 * sa;
    }
    const double* ob = obs + 4 * (j >> 1);
    const double cx = ob[0], cy = ob[1], hwo = 0.5 * ob[2], hho = 0.5 * ob[3];
    const double* l = q + 4;
    const double a = l[0] - l[2], c = l[1] - l[3];
    double nr = sqrt(a * a + c * c);
    if (nr < 1e-12) nr = 1e-12;
    const double ex = p0 - cx, ey = p1 - cy;
    const double e2 = -sa * a + ca * c, e3 = -ca * a - sa * c;
    const double y1 = q[28], y2 = q[29], y3 = q[30], y4 = q[31];
    const double rot = y2 * (-ca * a - sa * c) + y3 * (sa * a - ca * c);
    hxx[0] = -y1 * (a * ppt0 + c * ppt1) + rot;
    hxx[1] = -y1 * (a * ptp0 + c * ptp1) + rot * angp;
    hxx[2] = -y1 * (a * ppp0 + c * ppp1) + rot * angp;
    const int cls = r >> 2, i = r & 3;
#pragma unroll
    for (int t = 0; t < 20; ++t) row[t] = 0.0;
    const double an = a / nr, cn = c / nr;
    const double sgn = i < 2 ? 1.0 : -1.0;  // a dual lam_i enters through a = l0 - l2 (even i) or c = l1 - l3 (odd i)
    const bool par = (i & 1) != 0;
    if (cls < 2) {  // a dual: Sigma_w and (lam only) W_ww, H_wx; its column of J_w
        const double sg = q[8 + r] / (q[r] + 1e-8);
#pragma unroll
        for (int t = 0; t < 8; ++t) row[t] = t == r ? sg : 0.0;
        if (cls == 0) {
            row[12] = par ? hw : hl;
            row[13] = par ? 0.0 : sgn;
            row[14] = par ? sgn : 0.0;
        } else {
            row[12] = par ? (i < 2 ? -(ey - hho) : ey + hho) : (i < 2 ? -(ex - hwo) : ex + hwo);
            row[13] = sgn * (par ? sa : ca);
            row[14] = sgn * (par ? ca : -sa);
            row[15] = sgn * (par ? cn : an);
            // lam-lam: y4 T' H4 T, H4 = (1/n^3) [[c^2, -ac], [-ac, a^2]], T = [[1, 0, -1, 0], [0, 1, 0, -1]]
            const double n3 = nr * nr * nr, haa = y4 * c * c / n3, hac = -y4 * a * c / n3, hcc = y4 * a * a / n3;
            const double h0 = sgn * (par ? hac : haa), h1 = sgn * (par ? hcc : hac);
            row[4] += h0;
            row[5] += h1;
            row[6] += -h0;
            row[7] += -h1;
            const double r0 = -y2 * sa - y3 * ca, r1 = y2 * ca - y3 * sa;  // d(y2 e2 + y3 e3) / d(a, c)
            row[16] = par ? 0.0 : -sgn * y1;
            row[17] = par ? -sgn * y1 : 0.0;
            row[18] = sgn * (par ? -y1 * dpt1 + r1 : -y1 * dpt0 + r0);
            row[19] = sgn * (par ? -y1 * dpp1 + angp * r1 : -y1 * dpp0 + angp * r0);
        }
    } else if (cls == 2) {  // a row slack: Sigma_s and -1 against its multiplier
        const double e = p.eq_tol + 1e-8, sv = q[16 + i], vl = q[20 + i], vu = q[24 + i];
        const double sg = (i == 0 || i == 3) ? vu / (1e-8 - sv) : vl / (sv + e) + vu / (e - sv);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            row[8 + t] = t == i ? sg : 0.0;
            row[12 + t] = t == i ? -1.0 : 0.0;
        }
    } else {  // a row multiplier: its rows of J_w and J_x, -1 against its slack
        row[0] = i == 0 ? hl : i == 1 ? 1.0 : 0.0;
        row[1] = i == 0 ? hw : i == 2 ? 1.0 : 0.0;
        row[2] = i == 0 ? hl : i == 1 ? -1.0 : 0.0;
        row[3] = i == 0 ? hw : i == 2 ? -1.0 : 0.0;
        row[4] = i == 0 ? -(ex - hwo) : i == 1 ? ca : i == 2 ? -sa : an;
        row[5] = i == 0 ? -(ey - hho) : i == 1 ? sa : i == 2 ? ca : cn;
        row[6] = i == 0 ? ex + hwo : i == 1 ? -ca : i == 2 ? sa : -an;
        row[7] = i == 0 ? ey + hho : i == 1 ? -sa : i == 2 ? -ca : -cn;
#pragma unroll
        for (int t = 0; t < 4; ++t) row[8 + t] = t == i ? -1.0 : 0.0;
        row[16] = i == 0 ? -a : 0.0;
        row[17] = i == 0 ? -c : 0.0;
        row[18] = i == 0 ? -(a * dpt0 + c * dpt1) : i == 1 ? e2 : i == 2 ? e3 : 0.0;
        row[19] = i == 0 ? -(a * dpp0 + c * dpp1) : i == 1 ? e2 * angp : i == 2 ? e3 * angp : 0.0;
    }
}

// The group's LU elimination of the rows (one per lane) with partial pivoting, over the columns c < 16 of K_b and the
// trailing columns up to kCols: the pivot of column c is the lane with the largest entry among the lanes not yet used
// (the lowest lane among equals); rows never move.  kKeep: the multipliers stay in place of the eliminated entries.
// mycol: the column this lane pivoted on; rows: the pivot lane of column c in bits 4c .. 4c + 3, the same in every
// lane.  Both block passes factor through this routine, so they pivot alike.  false: a zero or non-finite pivot.
template <int kCols, bool kKeep>
__device__ __forceinline__ bool factor_rows(double (&row)[20], int r, int& mycol, unsigned long long& rows) {
    bool ok = true, used = false;
    mycol = -1;
    rows = 0ull;
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        double bm = used ? -1.0 : fabs(row[c]);
        int bl = r;
        for (int m = 1; m < kGL; m <<= 1) {
            const double om = __shfl_xor(bm, m, kGL);
            const int ol = __shfl_xor(bl, m, kGL);
            if (om > bm || (om == bm && ol < bl)) {
                bm = om;
                bl = ol;
            }
        }
        const double piv = __shfl(row[c], bl, kGL);
        ok = ok && isfinite(piv) && piv != 0.0 && bm > 0.0;
        if (bl == r) {
            used = true;
            mycol = c;
        }
        rows |= (unsigned long long)bl << (4 * c);
        const double f = row[c] / piv;
        if (kKeep && !used) row[c] = f;
#pragma unroll
        for (int t = c + 1; t < kCols; ++t) {
            const double pv = __shfl(row[t], bl, kGL);
            if (!used) row[t] = row[t] - f * pv;
        }
    }
    return ok;
}

// The group's elimination of [K_b | C] (one row per lane) and the pose addend H_xx - C' K_b^-1 C: every lane of the
// group leaves with the ten upper entries (a <= b) in add[]; false if a pivot is zero or not finite.
__device__ __forceinline__ bool eliminate_block(double (&row)[20], const double (&hxx)[3], int r, double (&add)[10]) {
    double c0[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) c0[t] = row[16 + t];
    int mycol;
    unsigned long long rows;
    bool ok = factor_rows<20, false>(row, r, mycol, rows);
    bool done = false;
#pragma unroll
    for (int c = 15; c >= 0; --c) {
        const int src = (int)((rows >> (4 * c)) & 15ull);
        if (mycol == c) {
#pragma unroll
            for (int t = 0; t < 4; ++t) row[16 + t] = row[16 + t] / row[c];
            done = true;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const double xv = __shfl(row[16 + t], src, kGL);
            if (!done) row[16 + t] = row[16 + t] - row[c] * xv;
        }
    }
    // lane r holds row `mycol` of X = K_b^-1 C; C's row of that unknown sits in lane `mycol`
    double cs[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) cs[t] = __shfl(c0[t], mycol < 0 ? r : mycol, kGL);
    int e = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = a; b < 4; ++b) {
            double s = cs[a] * row[16 + b];
            for (int m = kGL / 2; m > 0; m >>= 1) s += __shfl_xor(s, m, kGL);
            const double h = a < 2 ? 0.0 : hxx[a + b - 4];  // (2,2), (2,3), (3,3)
            add[e] = h - s;
            ok = ok && isfinite(add[e]);
            ++e;
        }
    return ok;
}

// The refinement pass of one block (one row of K_b per lane, C in row[16 ..]) for the first solve's pose part lxp:
// factor K_b (factor_rows, the multipliers kept in place); v = -K_b^-1 C lxp; the block rows' residual
// r = -(C lxp + K_b v) against the un-eliminated rows; t = K_b^-1 r.  Every lane leaves with
// out[0..3] = H_xx lxp + C' v and out[4..7] = -C' t; false if a pivot is zero or a value is not finite.
__device__ __forceinline__ bool refine_block(double (&row)[20], const double (&hxx)[3], int r, const double (&lxp)[4],
                                             double (&out)[8]) {
    double orig[16], c0[4];
#pragma unroll
    for (int t = 0; t < 16; ++t) orig[t] = row[t];
#pragma unroll
    for (int t = 0; t < 4; ++t) c0[t] = row[16 + t];
    int mycol;
    unsigned long long rows;
    bool ok = factor_rows<16, true>(row, r, mycol, rows);
    // one right-hand side (equation r in lane r) through the factors; the lane leaves with the unknown `mycol`
    auto solve = [&](double y) {
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const double yp = __shfl(y, (int)((rows >> (4 * c)) & 15ull), kGL);
            if (mycol > c) y = y - row[c] * yp;
        }
#pragma unroll
        for (int c = 15; c >= 0; --c) {
            if (mycol == c) y = y / row[c];
            const double xc = __shfl(y, (int)((rows >> (4 * c)) & 15ull), kGL);
            if (mycol < c) y = y - row[c] * xc;
        }
        return y;
    };
    double b0 = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) b0 += c0[t] * lxp[t];
    b0 = -b0;
    const double v = solve(b0);
    double kv = 0.0;
#pragma unroll
    for (int jn = 0; jn < 16; ++jn) kv += orig[jn] * __shfl(v, (int)((rows >> (4 * jn)) & 15ull), kGL);
    const double tt = solve(b0 - kv);
    const int src = mycol < 0 ? r : mycol;
#pragma unroll
    for (int aa = 0; aa < 4; ++aa) {
        const double cs = __shfl(c0[aa], src, kGL);
        double sv = cs * v, st = cs * tt;
        for (int m = kGL / 2; m > 0; m >>= 1) {
            sv += __shfl_xor(sv, m, kGL);
            st += __shfl_xor(st, m, kGL);
        }
        const double h = aa < 2 ? 0.0 : hxx[aa - 2] * lxp[2] + hxx[aa - 1] * lxp[3];  // rows 2, 3 of H_xx
        out[aa] = h + sv;
        out[4 + aa] = -st;
        ok = ok && isfinite(out[aa]) && isfinite(out[4 + aa]);
    }
    return ok;
}

// The params instantiation's block pass (one row of K_b per lane, C in row[16 ..]), with the block unknowns carried:
// uin is entry r of the block's record u = v + t of the previous pass (zero before the first), dlx the pose part of the
// last correction (of the first solve before the first pass), lxp the running pose adjoint.  Factor K_b; the previous
// step's correction v = u - K_b^-1 C dlx (it enters through dlx, never through the rounded sum lxp: v_yd1 is 4e13 times
// a 1e-12 component of the pose adjoint); then the residual r = -(C lxp + K_b v) against the carried v and
// t = K_b^-1 r.  Lane r leaves with entry r of v in vr and of v + t in ur (the order of the unknowns: w 8, s 4, y_d 4),
// every lane with out[0..3] = H_xx lxp + C' v and out[4..7] = -C' t.  kClosing: v alone (the pass after the last step).
template <bool kClosing>
__device__ __forceinline__ bool carry_block(double (&row)[20], const double (&hxx)[3], int r, const double (&dlx)[4],
                                            const double (&lxp)[4], double uin, double& vr, double& ur,
                                            double (&out)[8]) {
    double orig[16], c0[4];
#pragma unroll
    for (int t = 0; t < 16; ++t) orig[t] = row[t];
#pragma unroll
    for (int t = 0; t < 4; ++t) c0[t] = row[16 + t];
    int mycol;
    unsigned long long rows;
    bool ok = factor_rows<16, true>(row, r, mycol, rows);
    const int holder = (int)((rows >> (4 * r)) & 15ull);  // the lane that pivoted on column r holds unknown r
    // one right-hand side (equation r in lane r) through the factors; lane r leaves with the unknown r
    auto solve = [&](double y) {
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            const double yp = __shfl(y, (int)((rows >> (4 * c)) & 15ull), kGL);
            if (mycol > c) y = y - row[c] * yp;
        }
#pragma unroll
        for (int c = 15; c >= 0; --c) {
            if (mycol == c) y = y / row[c];
            const double xc = __shfl(y, (int)((rows >> (4 * c)) & 15ull), kGL);
            if (mycol < c) y = y - row[c] * xc;
        }
        return __shfl(y, holder, kGL);
    };
    double bd = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) bd += c0[t] * dlx[t];
    vr = uin + solve(-bd);
    ur = vr;
    ok = ok && isfinite(vr);
    if (kClosing) return ok;
    double b0 = 0.0, kv = 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) b0 += c0[t] * lxp[t];
    b0 = -b0;
#pragma unroll
    for (int jn = 0; jn < 16; ++jn) kv += orig[jn] * __shfl(vr, jn, kGL);
    const double tt = solve(b0 - kv);
    ur = vr + tt;
#pragma unroll
    for (int aa = 0; aa < 4; ++aa) {
        double sv = c0[aa] * vr, st = c0[aa] * tt;  // (K is symmetric: row r of C belongs to unknown r)
        for (int m = kGL / 2; m > 0; m >>= 1) {
            sv += __shfl_xor(sv, m, kGL);
            st += __shfl_xor(st, m, kGL);
        }
        const double h = aa < 2 ? 0.0 : hxx[aa - 2] * lxp[2] + hxx[aa - 1] * lxp[3];  // rows 2, 3 of H_xx
        out[aa] = h + sv;
        out[4 + aa] = -st;
        ok = ok && isfinite(out[aa]) && isfinite(out[4 + aa]);
    }
    return ok && isfinite(ur);
}

__device__ __forceinline__ void zero_geom(const ObcaVjpGeomArgs& a, int b, int tid) {
    if (tid < 5) a.g_geom[(size_t)b * 5 + tid] = 0.0;
}

// The geometry instantiation's share of one block (lane-uniform within the group): the terms of -lam' dF/dtheta the
// block's d_min row d_0 = g' mu - (a, c) . (p - centre) + ... contributes through g = (hl, hw, hl, hw) and the body
// centre p.  xk: the stage's state; q: the block's iterate (mu 4, lam 4 first, y_d0 at 28); v0 .. v7, vy: the entries
// mu 4, lam 4 and y_d0 of the block's carried unknowns; lp2, lp3: the stage's pose adjoint in theta and psi.
// t[0]: the length (L1 truck, L2 trailer), t[1]: the width (W1, W2), t[2]: Mh (trailer; 0 for the truck).
// tests/obca_geometry_reference.py (block_share) has the derivation.
__device__ __forceinline__ void geometry_block_terms(const double* xk, int j, const double* q, const double (&v)[8],
                                                     double vy, double lp2, double lp3, double (&t)[3]) {
    const double th = xk[2], ps = xk[3];
    const double a = q[4] - q[6], c = q[5] - q[7], yd0 = q[28];
    const double va = v[4] - v[6], vc = v[5] - v[7], ve = v[0] + v[2], vo = v[1] + v[3];
    const double me = q[0] + q[2], mo = q[1] + q[3];
    double st, ct;
    sincos(th, &st, &ct);
    t[1] = -(yd0 * (0.5 * vo) + vy * (0.5 * mo));
    if ((j & 1) == 0) {  // truck: dp/dL1 = (ct, st) / 2, d2p/dth dL1 = (-st, ct) / 2
        const double dp0 = 0.5 * ct, dp1 = 0.5 * st, rot = a * (-0.5 * st) + c * (0.5 * ct);
        t[0] = -(yd0 * (0.5 * ve - (dp0 * va + dp1 * vc) - rot * lp2) + vy * (0.5 * me - (a * dp0 + c * dp1)));
        t[2] = 0.0;
    } else {  // trailer: dp/dL2 = -(ca, sa) / 2, d2p/d(th, psi) dL2 = (sa, -ca) / 2; dp/dMh = -(ct, st), d2p/dth dMh = (st, -ct)
        double sa, ca;
        sincos(th + ps, &sa, &ca);
        const double dp0 = -0.5 * ca, dp1 = -0.5 * sa, rot = a * (0.5 * sa) + c * (-0.5 * ca);
        t[0] = -(yd0 * (0.5 * ve - (dp0 * va + dp1 * vc) - rot * lp2 - rot * lp3) + vy * (0.5 * me - (a * dp0 + c * dp1)));
        const double rm = a * st + c * -ct;
        t[2] = -(yd0 * (-(-ct * va + -st * vc) - rm * lp2) + vy * (-(a * -ct + c * -st)));
    }
}

__device__ __forceinline__ void zero_params(const ObcaVjpParamsArgs& a, int b, int tid) {
    if (a.g_obs)
        for (int t = tid; t < 4 * a.M; t += kT) a.g_obs[(size_t)b * 4 * a.M + t] = 0.0;
    if (a.g_dmin && tid == 0) a.g_dmin[b] = 0.0;
    if (a.g_Q)
        for (int t = tid; t < 36; t += kT) a.g_Q[(size_t)b * 36 + t] = 0.0;
    if (a.g_R)
        for (int t = tid; t < 4; t += kT) a.g_R[(size_t)b * 4 + t] = 0.0;
}

// forward sweep: lx_0 = 0; lu_k = -K_k lx_k + kappa_k; lx_{k+1} = A_k lx_k + B lu_k, into the Sigma slots of the stages
__device__ __forceinline__ void forward_sweep(double* stg, const double* Ks, int N, double dt, int tid, bool& bad) {
    if (tid < 6) stg[sSG + tid] = 0.0;
    __syncthreads();
    for (int k = 0; k < N; ++k) {
        double* r = stg + k * kStage;
        if (tid < 6) {
            double lx[6];
#pragma unroll
            for (int l = 0; l < 6; ++l) lx[l] = r[sSG + l];
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int l = 0; l < 6; ++l) {
                s0 += Ks[k * 12 + l] * lx[l];
                s1 += Ks[k * 12 + 6 + l] * lx[l];
            }
            const double lu0 = -s0 + r[sG + 6], lu1 = -s1 + r[sG + 7];
            double s = r[sSG + tid];  // row `tid`
#pragma unroll
            for (int l = 0; l < 6; ++l) {
                const int di = d_idx(tid, l);
                if (di >= 0) s += r[sAJ + di] * lx[l];
            }
            if (tid == 5) s += dt * lu0;
            if (tid == 4) s += dt * lu1;
            bad |= !isfinite(s) || !isfinite(lu0) || !isfinite(lu1);
            r[kStage + sSG + tid] = s;  // stage k + 1
            if (tid < 2) r[sSG + 6 + tid] = tid == 0 ? lu0 : lu1;
        }
        __syncthreads();
    }
}

// kParams: the instantiation that also forms dL/d(obstacles, d_min, Q, R) (tt_obca_vjp_params*); everything it adds sits
// behind `if constexpr`, so the plain instantiation is the kernel it was.  kGeom (with kParams): the instantiation that
// also forms dL/d(L1, L2, Mh, W1, W2) (tt_obca_vjp_geometry*), behind `if constexpr` again
template <bool kParams, bool kGeom = false>
__global__ __launch_bounds__(kT) void obca_vjp_kernel(
    std::conditional_t<kGeom, ObcaVjpGeomArgs, std::conditional_t<kParams, ObcaVjpParamsArgs, ObcaVjpArgs>> a) {
    static_assert(kParams || !kGeom, "the geometry terms read the carried block unknowns");
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.N, S = N + 1, nbk = 2 * a.M, nblk = S * nbk;
    if (a.status[b] > 1) {  // > TT_ACCEPTABLE: no optimum to differentiate
        zero_outputs(a, b, tid);
        if constexpr (kParams) zero_params(a, b, tid);
        if constexpr (kGeom) zero_geom(a, b, tid);
        if (a.vjp_status && tid == 0) a.vjp_status[b] = 2;
        return;
    }
    double* stg = sm;                  // [S][kStage]
    double* Ks = sm + kStage * S;      // [N][2][6]
    double* T = Ks + 12 * N;           // tiles
    double* slot = T + kVjpTiles;      // [kGroups][16]
    double* obs = slot + 16 * kGroups; // [kObcaMaxM][4]: the lanes index the obstacles by their block
    const double* it = a.iterate + (size_t)b * obca_iterate_len(N, a.M);
    const double* blk = it + 30 * (size_t)S;
    const double* gx = a.gx ? a.gx + (size_t)b * S * 6 : nullptr;
    const double* gu = a.gu ? a.gu + (size_t)b * N * 2 : nullptr;
    const double dt = a.dt;
    bool bad = false;

    if (tid == 0) {
#pragma unroll
        for (int t = 0; t < 4 * kObcaMaxM; ++t) obs[t] = a.obs[t];
        // per-instance scenes: row b over the launch's scene (the adjoint's system does not hold d_min: it only shifts
        // the residual of row 1, so a per-instance d_min has nothing to replace here)
        if (a.obs_b)
            for (int t = 0; t < 4 * a.M; ++t) obs[t] = a.obs_b[(size_t)b * 4 * a.M + t];
    }
    // ---- stage-parallel pre-pass: the tracking record from the iterate's stage fields, g, a zero addend ----
    for (int k = tid; k <= N; k += kT) {
        double* r = stg + k * kStage;
        const double* q = it + 30 * (size_t)k;  // x 6, u 2, zLx 6, zUx 6, zLu 2, zUu 2, y_c 6
        double dk[kDualPerStage + 6];           // linearise_stage's view: y_k | z_L 8 | z_U 8 | y_{k+1}
#pragma unroll
        for (int v = 0; v < 6; ++v) {
            dk[v] = q[24 + v];
            dk[6 + v] = q[8 + v];
            dk[14 + v] = q[14 + v];
            dk[kDualPerStage + v] = k < N ? q[30 + 24 + v] : 0.0;
        }
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            dk[12 + v] = q[20 + v];
            dk[20 + v] = q[22 + v];
        }
        sens::linearise_stage(a, r, q, q + 6, dk, k == N);
#pragma unroll
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
#pragma unroll
        for (int v = 0; v < 17; ++v) r[sG + 8 + v] = 0.0;
#pragma unroll
        for (int v = 0; v < 8; ++v) r[sSV + v] = r[sSG + v];
        r[sGU] = r[sG + 6];
        r[sGU + 1] = r[sG + 7];
#pragma unroll
        for (int v = 0; v < 6; ++v) r[sGX + v] = r[sG + v];
#pragma unroll
        for (int v = 0; v < 8; ++v) r[sW + v] = 0.0;
    }
    __syncthreads();
    // ---- block phase: sixteen blocks per round, their addends into the stages in block order ----
    const int grp = tid / kGL, r16 = tid % kGL;
    for (int f0 = nbk; f0 < nblk; f0 += kGroups) {
        const int f = min(f0 + grp, nblk - 1);  // (a group past the end repeats the last block and stores nothing)
        const int k = f / nbk, j = f - k * nbk;
        double row[20], hxx[3], add[10];
        build_row(a, obs, it + 30 * (size_t)k, j, blk + 32 * (size_t)f, r16, row, hxx);
        const bool ok = eliminate_block(row, hxx, r16, add);
        if (f0 + grp < nblk) {
            bad |= !ok;
            if (r16 == 0) {
                int e = 0;
                for (int i = 0; i < 4; ++i)
                    for (int jj = i; jj < 4; ++jj) {
                        slot[grp * 16 + i * 4 + jj] = add[e];
                        slot[grp * 16 + jj * 4 + i] = add[e];
                        ++e;
                    }
            }
        }
        __syncthreads();
        if (tid < 16) {
            const int ng = min(kGroups, nblk - f0);
            for (int g = 0; g < ng; ++g) {
                const int kk = (f0 + g) / nbk;
                stg[kk * kStage + sDH + tid] += slot[g * 16 + tid];
            }
        }
        __syncthreads();
    }
    // ---- backward sweep (entry-parallel, p and kappa beside the matrix lanes) ----
    const sens::Roles ro(tid);
    sens::backward_sweep<Layout>(a, ro, nullptr, stg, Ks, T, tid, bad);  // (its p_0 is not used: lam_y,0 below)
    // ---- forward sweep: lx_k | lu_k into the Sigma slots of stage k ----
    forward_sweep(stg, Ks, N, dt, tid, bad);
    if (__syncthreads_or(bad)) {
        zero_outputs(a, b, tid);
        if constexpr (kParams) zero_params(a, b, tid);
        if constexpr (kGeom) zero_geom(a, b, tid);
        if (a.vjp_status && tid == 0) a.vjp_status[b] = 1;
        return;
    }
    for (int k = tid; k <= N; k += kT) {  // the running solution lx | lu
        double* r = stg + k * kStage;
#pragma unroll
        for (int l = 0; l < 8; ++l) r[sL + l] = k == N && l >= 6 ? 0.0 : r[sSG + l];
    }
    __syncthreads();
    int pc2 = 0;
    for (int step = 0; step < kRefine; ++step) {
        // ---- block pass: w = sum_b (H_xx lx_pose + C' v) and fold = -sum_b C' t per stage, in block order ----
        for (int k = tid; k <= N; k += kT) {
#pragma unroll
            for (int v = 0; v < 8; ++v) stg[k * kStage + sW + v] = 0.0;
        }
        __syncthreads();
        if constexpr (kParams) {
            // the carried pass: the records of the next round are loaded before this round's are stored (a load issued
            // behind a store waits for it)
            double* wk = a.work + (size_t)b * nblk * 16;
            double ucur = step > 0 ? wk[(size_t)min(nbk + grp, nblk - 1) * 16 + r16] : 0.0;
            for (int f0 = nbk; f0 < nblk; f0 += kGroups) {
                const int f = min(f0 + grp, nblk - 1);
                const int k = f / nbk, j = f - k * nbk;
                double unext = 0.0;
                if (step > 0 && f0 + kGroups < nblk) unext = wk[(size_t)min(f0 + kGroups + grp, nblk - 1) * 16 + r16];
                double row[20], hxx[3], dlx[4], lxp[4], out[8], vr, ur;
                build_row(a, obs, it + 30 * (size_t)k, j, blk + 32 * (size_t)f, r16, row, hxx);
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    lxp[t] = stg[k * kStage + sL + t];
                    dlx[t] = stg[k * kStage + sSG + t];  // (the last correction; the first solve itself in step 0)
                }
                const bool ok = carry_block<false>(row, hxx, r16, dlx, lxp, ucur, vr, ur, out);
                if (f0 + grp < nblk) {
                    bad |= !ok;
                    wk[(size_t)f * 16 + r16] = ur;
                    if (r16 == 0) {
#pragma unroll
                        for (int t = 0; t < 8; ++t) slot[grp * 16 + t] = out[t];
                    }
                }
                __syncthreads();
                if (tid < 8) {
                    const int ng = min(kGroups, nblk - f0);
                    for (int g = 0; g < ng; ++g) {
                        const int kk = (f0 + g) / nbk;
                        stg[kk * kStage + sW + tid] += slot[g * 16 + tid];
                    }
                }
                __syncthreads();
                ucur = unext;
            }
        } else {
            for (int f0 = nbk; f0 < nblk; f0 += kGroups) {
                const int f = min(f0 + grp, nblk - 1);
                const int k = f / nbk, j = f - k * nbk;
                double row[20], hxx[3], lxp[4], out[8];
                build_row(a, obs, it + 30 * (size_t)k, j, blk + 32 * (size_t)f, r16, row, hxx);
#pragma unroll
                for (int t = 0; t < 4; ++t) lxp[t] = stg[k * kStage + sL + t];
                const bool ok = refine_block(row, hxx, r16, lxp, out);
                if (f0 + grp < nblk) {
                    bad |= !ok;
                    if (r16 == 0) {
#pragma unroll
                        for (int t = 0; t < 8; ++t) slot[grp * 16 + t] = out[t];
                    }
                }
                __syncthreads();
                if (tid < 8) {
                    const int ng = min(kGroups, nblk - f0);
                    for (int g = 0; g < ng; ++g) {
                        const int kk = (f0 + g) / nbk;
                        stg[kk * kStage + sW + tid] += slot[g * 16 + tid];
                    }
                }
                __syncthreads();
            }
        }
        // ---- stage part: lam_y from the x-rows, the input rows' residual, the correction's right-hand side ----
        for (int k = tid; k <= N; k += kT) {  // rr_k = gX_k - H0_k lx_k - w_k into sY
            double* r = stg + k * kStage;
            double lx[6];
#pragma unroll
            for (int l = 0; l < 6; ++l) lx[l] = r[sL + l];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                double s = 0.0;
#pragma unroll
                for (int l = 0; l < 6; ++l) s += T[tQW + i * 6 + l] * lx[l];
                if (k < N) {
#pragma unroll
                    for (int l = 0; l < 6; ++l) {
                        const int wi = sens::w_idx(i, l);
                        if (wi >= 0) s += r[sens::sWC + wi] * lx[l];
                    }
                }
                s = s + r[sSV + i] * lx[i];
                double v = r[sGX + i] - s;
                if (i < 4) v = v - r[sW + i];
                bad |= !isfinite(v);
                r[sY + i] = v;
            }
        }
        __syncthreads();
        for (int k = N - 1; k >= 0; --k) {  // ly_k = rr_k + A_k' ly_{k+1}
            double* r = stg + k * kStage;
            if (tid < 6) {
                const double* ln = r + kStage + sY;
                double s = ln[tid];
#pragma unroll
                for (int l = 0; l < 6; ++l) {
                    const int di = d_idx(l, tid);
                    if (di >= 0) s += r[sAJ + di] * ln[l];
                }
                s = r[sY + tid] + s;
                bad |= !isfinite(s);
                r[sY + tid] = s;
            }
            __syncthreads();
        }
        for (int k = tid; k <= N; k += kT) {  // right-hand side of the correction: fold on the pose, ru on the inputs
            double* r = stg + k * kStage;
            double ru0 = 0.0, ru1 = 0.0;
            if (k < N) {
                const double* ln = r + kStage + sY;
                const double lu0 = r[sL + 6], lu1 = r[sL + 7];
                ru0 = r[sGU] - (T[tRW + 0] * lu0 + T[tRW + 1] * lu1 + r[sSV + 6] * lu0) + dt * ln[5];
                ru1 = r[sGU + 1] - (T[tRW + 2] * lu0 + T[tRW + 3] * lu1 + r[sSV + 7] * lu1) + dt * ln[4];
            }
            bad |= !isfinite(ru0) || !isfinite(ru1);
#pragma unroll
            for (int v = 0; v < 4; ++v) r[sG + v] = r[sF + v];
            r[sG + 4] = 0.0;
            r[sG + 5] = 0.0;
            r[sG + 6] = ru0;
            r[sG + 7] = ru1;
#pragma unroll
            for (int v = 0; v < 8; ++v) r[sSG + v] = r[sSV + v];
        }
        __syncthreads();
        // ---- the correction: the same sweeps on the residual ----
        pc2 = sens::backward_sweep<Layout>(a, ro, nullptr, stg, Ks, T, tid, bad);
        forward_sweep(stg, Ks, N, dt, tid, bad);
        for (int k = tid; k <= N; k += kT) {
            double* r = stg + k * kStage;
            const int nl = k < N ? 8 : 6;
            for (int l = 0; l < nl; ++l) r[sL + l] = r[sL + l] + r[sSG + l];
        }
        __syncthreads();
    }
    // ---- the closing block pass: the last correction into v; the blocks' scene terms per obstacle in block order ----
    double acc = 0.0;  // thread 5 m + i: g_b[i] (i < 4) or the d_min sum (i = 4) of obstacle m
    // (geometry) thread kGeomT + i: the block sum of L1, L2, Mh, W1, W2; its slot entry and its body (1: trailer)
    constexpr int kGeomT = 5 * kObcaMaxM;
    [[maybe_unused]] double gacc = 0.0;
    [[maybe_unused]] const int gi = tid - kGeomT, gslot = gi < 2 ? 5 : gi == 2 ? 7 : 6, gbody = (gi == 1 || gi == 2 || gi == 4) ? 1 : 0;
    if constexpr (kParams) {
        const double* wk = a.work + (size_t)b * nblk * 16;
        const int am = tid / 5, ai = tid - 5 * am;
        for (int f0 = nbk; f0 < nblk; f0 += kGroups) {
            const int f = min(f0 + grp, nblk - 1);
            const int k = f / nbk, j = f - k * nbk;
            const double uin = wk[(size_t)f * 16 + r16];
            double row[20], hxx[3], dlx[4], out[8], vr, ur;
            const double* q = blk + 32 * (size_t)f;
            build_row(a, obs, it + 30 * (size_t)k, j, q, r16, row, hxx);
#pragma unroll
            for (int t = 0; t < 4; ++t) dlx[t] = stg[k * kStage + sSG + t];
            const bool ok = carry_block<true>(row, hxx, r16, dlx, dlx, uin, vr, ur, out);
            const double vl = __shfl(vr, 4 + (r16 & 3), kGL), vy = __shfl(vr, 12, kGL);
            if (f0 + grp < nblk) {
                bad |= !ok;
                // row 1 of the block: g' mu - (A p - b)' lam + d_min - s_1 = 0, and b also in the lam rows through y_d1
                if (r16 < 4) slot[grp * 16 + r16] = -(q[28] * vl + q[4 + r16] * vy);
                if (r16 == 4) slot[grp * 16 + 4] = -vy;
            }
            if constexpr (kGeom) {
                double v8[8], gt[3];
#pragma unroll
                for (int t = 0; t < 8; ++t) v8[t] = __shfl(vr, t, kGL);
                geometry_block_terms(it + 30 * (size_t)k, j, q, v8, vy, stg[k * kStage + sL + 2],
                                     stg[k * kStage + sL + 3], gt);
                if (f0 + grp < nblk && r16 >= 5 && r16 < 8) slot[grp * 16 + r16] = r16 == 5 ? gt[0] : r16 == 6 ? gt[1] : gt[2];
            }
            __syncthreads();
            if (tid < 5 * kObcaMaxM) {
                const int ng = min(kGroups, nblk - f0);
                int jj = f0 % nbk;
                for (int g = 0; g < ng; ++g) {
                    if ((jj >> 1) == am) acc += slot[g * 16 + ai];
                    if (++jj == nbk) jj = 0;
                }
            }
            if constexpr (kGeom) {
                if (gi >= 0 && gi < 5) {
                    const int ng = min(kGroups, nblk - f0);
                    int jj = f0 % nbk;
                    for (int g = 0; g < ng; ++g) {
                        if ((jj & 1) == gbody) gacc += slot[g * 16 + gslot];
                        if (++jj == nbk) jj = 0;
                    }
                }
            }
            __syncthreads();
        }
    }
    // ---- (geometry) the dynamics share: dt sum_k [lx_k' (dJ_f/dtheta)' y_{k+1} + ly_{k+1}' df/dtheta], tt_vjp.hip's
    // model_gradient expressions with the final lx and the last step's ly (sY); the stage terms go through the dead w field
    if constexpr (kGeom) {
        const double iL1 = 1.0 / a.L1, iL2 = 1.0 / a.L2, iL1L2 = iL1 * iL2, Mh = a.Mh;
        for (int k = tid; k < N; k += kT) {
            double* r = stg + k * kStage;
            const double* xk = it + 30 * (size_t)k;
            const double* y = it + 30 * (size_t)(k + 1) + 24;  // y_{k+1}
            const double* ly = r + kStage + sY;                // lam_y,k+1
            const double lx3 = r[sL + 3], lx4 = r[sL + 4], lx5 = r[sL + 5];
            double sps, cps, sph, cph;
            sincos(xk[3], &sps, &cps);
            sincos(xk[4], &sph, &cph);
            const double v = xk[5], ic = 1.0 / cph, t = sph * ic, c2 = ic * ic;
            const double kk = 1.0 + Mh * iL2 * cps;
            const double y2 = y[2], y3 = y[3], l2 = ly[2], l3 = ly[3];
            const double a24 = v * c2 * iL1, a25 = t * iL1, vt = v * t * iL1;
            const double mc = Mh * cps * iL2 * iL2, s2 = sps * iL2 * iL2;
            r[sW + 0] = y2 * (-(a24 * iL1) * lx4 + -(a25 * iL1) * lx5)
                      + y3 * (-(vt * Mh * sps * iL1L2) * lx3 + (a24 * kk * iL1) * lx4 + (a25 * kk * iL1) * lx5)
                      + (l2 * -(vt * iL1) + l3 * (vt * kk * iL1));
            r[sW + 1] = y3 * ((v * cps * iL2 * iL2 - vt * Mh * sps * iL2 * iL2) * lx3 + (a24 * mc) * lx4 + (a25 * mc + s2) * lx5)
                      + l3 * (vt * mc + v * s2);
            r[sW + 2] = y3 * ((vt * sps * iL2) * lx3 + -(a24 * cps * iL2) * lx4 + -(a25 * cps * iL2) * lx5)
                      + l3 * -(vt * cps * iL2);
        }
        __syncthreads();
        if (gi >= 0 && gi < 3) {
            double s = 0.0;
            for (int k = 0; k < N; ++k) s += stg[k * kStage + sW + gi];
            gacc = gacc + dt * s;
        }
        if (gi >= 0 && gi < 5) bad |= !isfinite(gacc);
    }
    if (__syncthreads_or(bad)) {
        zero_outputs(a, b, tid);
        if constexpr (kParams) zero_params(a, b, tid);
        if constexpr (kGeom) zero_geom(a, b, tid);
        if (a.vjp_status && tid == 0) a.vjp_status[b] = 1;
        return;
    }
    // ---- outputs ----
    // dL/dx_init = ly_0 + the last correction's p_0
    if (a.g_x0 && ro.pl) a.g_x0[(size_t)b * 6 + ro.pi] = stg[sY + ro.pi] + T[pc2 + ro.pi];
    for (int k = tid; k <= N; k += kT) {
        const double* r = stg + k * kStage;
        if (a.g_xref) {
            for (int ii = 0; ii < 6; ++ii) {
                double s = 0.0;
                for (int l = 0; l < 6; ++l) s += T[tQW + ii * 6 + l] * r[sL + l];
                bad |= !isfinite(s);
                a.g_xref[((size_t)b * S + k) * 6 + ii] = s;
            }
        }
        if (a.g_uref && k < N) {
            for (int ii = 0; ii < 2; ++ii) {
                const double s = T[tRW + ii * 2 + 0] * r[sL + 6] + T[tRW + ii * 2 + 1] * r[sL + 7];
                bad |= !isfinite(s);
                a.g_uref[((size_t)b * N + k) * 2 + ii] = s;
            }
        }
    }
    if constexpr (kGeom) {
        if (gi >= 0 && gi < 5) a.g_geom[(size_t)b * 5 + gi] = gacc;
    }
    if constexpr (kParams) {
        if (tid < 5 * kObcaMaxM) slot[tid] = acc;
        __syncthreads();
        if (tid < a.M) {  // b = (cx + w/2, cy + h/2, -cx + w/2, -cy + h/2)
            const double g0 = slot[5 * tid], g1 = slot[5 * tid + 1], g2 = slot[5 * tid + 2], g3 = slot[5 * tid + 3];
            const double o0 = g0 - g2, o1 = g1 - g3, o2 = 0.5 * (g0 + g2), o3 = 0.5 * (g1 + g3);
            bad |= !isfinite(o0) || !isfinite(o1) || !isfinite(o2) || !isfinite(o3);
            if (a.g_obs) {
                double* go = a.g_obs + ((size_t)b * a.M + tid) * 4;
                go[0] = o0;
                go[1] = o1;
                go[2] = o2;
                go[3] = o3;
            }
        }
        if (tid == 64) {
            double s = 0.0;
            for (int m = 0; m < a.M; ++m) s += slot[5 * m + 4];
            bad |= !isfinite(s);
            if (a.g_dmin) a.g_dmin[b] = s;
        }
        // dL/dQ[i][l] = -sum_k (lx_k[i] e_k[l] + lx_k[l] e_k[i]), e = x - xref; dL/dR alike on the inputs
        if (a.g_Q && tid >= 128 && tid < 164) {
            const int i = (tid - 128) / 6, l = (tid - 128) % 6;
            const double* xr = a.xref + (size_t)b * S * 6;
            double s = 0.0;
            for (int k = 0; k <= N; ++k) {
                const double* r = stg + k * kStage + sL;
                const double* q = it + 30 * (size_t)k;
                s = s - (r[i] * (q[l] - xr[k * 6 + l]) + r[l] * (q[i] - xr[k * 6 + i]));
            }
            bad |= !isfinite(s);
            a.g_Q[(size_t)b * 36 + tid - 128] = s;
        }
        if (a.g_R && tid >= 192 && tid < 196) {
            const int i = (tid - 192) / 2, l = (tid - 192) % 2;
            const double* ur = a.uref + (size_t)b * N * 2;
            double s = 0.0;
            for (int k = 0; k < N; ++k) {
                const double* r = stg + k * kStage + sL + 6;
                const double* q = it + 30 * (size_t)k + 6;
                s = s - (r[i] * (q[l] - ur[k * 2 + l]) + r[l] * (q[i] - ur[k * 2 + i]));
            }
            bad |= !isfinite(s);
            a.g_R[(size_t)b * 4 + tid - 192] = s;
        }
    }
    const bool late = __syncthreads_or(bad) != 0;  // an overflow in the output products (the barrier orders the stores)
    if (late) zero_outputs(a, b, tid);
    if constexpr (kParams) {
        if (late) zero_params(a, b, tid);
    }
    if constexpr (kGeom) {
        if (late) zero_geom(a, b, tid);
    }
    if (a.vjp_status && tid == 0) a.vjp_status[b] = late ? 1 : 0;
}

}  // namespace

hipError_t launch_obca_vjp(const ObcaVjpGeomArgs& a, ObcaVjpKind kind, hipStream_t stream) {
    const int bytes = 8 * obca_vjp_lds_doubles(a.N);
    if (bytes > 64 * 1024 - 512 || a.M < 1 || a.M > kObcaMaxM) return hipErrorInvalidValue;
    if ((kind != kObcaVjpPlain && !a.work) || (kind == kObcaVjpGeom && !a.g_geom)) return hipErrorInvalidValue;
    // each instantiation takes its own base of the block: the narrower ones' arguments are what they were
    if (kind == kObcaVjpPlain)
        hipLaunchKernelGGL(obca_vjp_kernel<false>, dim3(a.B), dim3(kT), bytes, stream,
                           static_cast<const ObcaVjpArgs&>(a));
    else if (kind == kObcaVjpParams)
        hipLaunchKernelGGL(obca_vjp_kernel<true>, dim3(a.B), dim3(kT), bytes, stream,
                           static_cast<const ObcaVjpParamsArgs&>(a));
    else
        hipLaunchKernelGGL((obca_vjp_kernel<true, true>), dim3(a.B), dim3(kT), bytes, stream, a);
    return hipGetLastError();
}

}  // namespace ttmpc
