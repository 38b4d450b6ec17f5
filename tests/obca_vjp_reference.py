"""Test helper (numpy only): reference algebra for the adjoint of an MPC+OBCA solve (tt_obca_vjp*, tt_obca_vjp.hip).

For a scalar loss L(X, U) with upstream gradient g = (gX, gU) the gradient with respect to x_init, xref and uref is

    K lam = (g, 0),   dL/dx_init = lam_y,0,   dL/dxref_k = 2 Q lam_x,k,   dL/duref_k = 2 R lam_u,k,

with K the Newton matrix of the barrier problem at the exported primal-dual iterate (include/ttmpc.h
tt_obca_iterate_len; oracle/c/tt_obca.c pack_iterate), the bound multipliers eliminated into Sigma.  Two routes:

* ``dense_obca_vjp``: the un-condensed matrix over (x, u, w, s | y_c, y_d), built from the oracle's block hook
  ``tto_obca_block_lin`` and ``ttmpc_oracle.jac_f`` / ``hess_f_contract``, and ``numpy.linalg.solve``.
* ``model_obca_vjp``: the kernel's route.  Every block's 16 unknowns (w 8, s 4, y_d 4) are eliminated onto the 4 pose
  coordinates of its stage by an LU elimination with partial pivoting and a back-substitution (one row per lane in
  the kernel), the stage's addends are summed in block order, the stage recursion is track_vjp_kernel's with the dense
  4x4 addend, and REFINE_STEPS refinement steps on the un-condensed system follow.

Both return dict(x0 (6,), xref (N+1,6), uref (N,2)); the model also ``ok``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from oracle import c_oracle as co
from oracle import ttmpc_oracle as to

KEYS = ("x0", "xref", "uref")
RELAX = 1e-8


def problem(N, params, Q, R, bounds, obstacles, **kw):
    """The oracle's MPC+OBCA problem (track mode)."""
    return co.make_obca_problem(N, params, Q, R, *bounds, obstacles, mode=co.OBCA_TRACK, **kw)


def case_a(cx=10.5, y0=0.1):
    """Case A: N = 6, M = 1, a straight reference at v = 4 past one obstacle whose d_min row is active at stage 6.
    Returns (N, params, Q, R, bounds, obstacles, x_init (6,), xref (N+1,6), uref (N,2))."""
    from ttmpc import scenarios as sc
    N = 6
    xref = np.zeros((N + 1, 6))
    xref[:, 0] = 0.4 * np.arange(N + 1)
    xref[:, 5] = 4.0
    x0 = np.array([0.0, y0, 0.02, 0.0, 0.0, 4.0])
    obs = np.array([[cx, 1.0, 2.0, 3.0]])
    bounds = (sc.OBCA_XLB, sc.OBCA_XUB, sc.OBCA_ULB, sc.OBCA_UUB)
    return N, dict(sc.OBCA_PARAMS), sc.OBCA_Q, sc.OBCA_R, bounds, obs, x0, xref, np.zeros((N, 2))


def case_b():
    """N = 8, M = 2: the truck meets the first obstacle at the last stage (its d_min row is active), the second lies
    beside the trailer (four blocks per stage), and the braking bound, tightened to -0.7, is active on the first
    stages."""
    from ttmpc import scenarios as sc
    N = 8
    xref = np.zeros((N + 1, 6))
    xref[:, 0] = 0.3 * np.arange(N + 1)
    xref[:, 5] = 3.0
    x0 = np.array([0.0, 0.1, 0.02, 0.0, 0.0, 3.0])
    obs = np.array([[10.5, 1.0, 2.0, 3.0], [-6.0, -2.8, 2.0, 2.0]])
    ulb = sc.OBCA_ULB.copy()
    ulb[0] = -0.7
    bounds = (sc.OBCA_XLB, sc.OBCA_XUB, ulb, sc.OBCA_UUB)
    return N, dict(sc.OBCA_PARAMS), sc.OBCA_Q, sc.OBCA_R, bounds, obs, x0, xref, np.zeros((N, 2))


def upstream(N, seed=3):
    """gX (N+1,6), gU (N,2) ~ U(-1, 1)."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, (N + 1, 6)), rng.uniform(-1.0, 1.0, (N, 2))


def unpack(it, N, M):
    """The exported iterate as a dict of arrays (stage fields (N+1, .), block fields (N+1, 2M, .))."""
    it = np.asarray(it, dtype=np.float64)
    st = it[:30 * (N + 1)].reshape(N + 1, 30)
    bl = it[30 * (N + 1):30 * (N + 1) + 64 * M * (N + 1)].reshape(N + 1, 2 * M, 32)
    return {"x": st[:, :6], "u": st[:N, 6:8], "zLx": st[:, 8:14], "zUx": st[:, 14:20], "zLu": st[:N, 20:22],
            "zUu": st[:N, 22:24], "yc": st[:, 24:30], "w": bl[..., :8], "zw": bl[..., 8:16], "s": bl[..., 16:20],
            "vL": bl[..., 20:24], "vU": bl[..., 24:28], "yd": bl[..., 28:32]}


def _block_lin(P):
    L = co._obca_lib()
    dp = C.POINTER(C.c_double)
    L.tto_obca_block_lin.argtypes = [C.POINTER(co.TTOObcaProblem), dp, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp]
    L.tto_obca_block_lin.restype = None
    p = lambda a: a.ctypes.data_as(dp)  # noqa: E731

    def lin(x, j, w, y):
        x, w, y = (np.ascontiguousarray(v, dtype=np.float64) for v in (x, w, y))
        out = [np.zeros(n) for n in (4, 16, 32, 16, 32, 16)]
        L.tto_obca_block_lin(C.byref(P), p(x), j, p(w), p(y), *[p(o) for o in out])
        _, Jx, Jw, Hxx, Hxw, Hww = out
        Hw = np.zeros((8, 8))
        Hw[4:, 4:] = Hww.reshape(4, 4)
        return Jx.reshape(4, 4), Jw.reshape(4, 8), Hxx.reshape(4, 4), Hxw.reshape(4, 8), Hw
    return lin


def _sigma(val, zl, zu, lb, ub):
    """z_L / (v - lb_rel) + z_U / (ub_rel - v) with IPOPT's relaxed bounds; 0 where a bound is free."""
    s = np.zeros_like(val)
    for i in range(val.shape[-1]):
        if np.isfinite(lb[i]) and abs(lb[i]) < 1e19:
            s[..., i] += zl[..., i] / (val[..., i] - (lb[i] - RELAX * max(1.0, abs(lb[i]))))
        if np.isfinite(ub[i]) and abs(ub[i]) < 1e19:
            s[..., i] += zu[..., i] / ((ub[i] + RELAX * max(1.0, abs(ub[i]))) - val[..., i])
    return s


def linearise(P, it):
    """Everything both routes read: A_k, the stage Hessians without the blocks, the Sigmas and the block pieces."""
    N, M = P.N, P.M
    params = {"dt": P.dt, "L1": P.L1, "L2": P.L2, "M": P.Mh}
    v = unpack(it, N, M)
    Q = np.array(P.Q).reshape(6, 6)
    R = np.array(P.R).reshape(2, 2)
    Q, R = 0.5 * (Q + Q.T), 0.5 * (R + R.T)
    xlb, xub, ulb, uub = (np.array(a) for a in (P.xlb, P.xub, P.ulb, P.uub))
    sx = _sigma(v["x"], v["zLx"], v["zUx"], xlb, xub)
    su = _sigma(v["u"], v["zLu"], v["zUu"], ulb, uub)
    sw = v["zw"] / (v["w"] + RELAX)
    e = P.eq_tol + RELAX
    ss = np.empty_like(v["s"])
    ss[..., 0] = v["vU"][..., 0] / (RELAX - v["s"][..., 0])
    ss[..., 3] = v["vU"][..., 3] / (RELAX - v["s"][..., 3])
    for r in (1, 2):
        ss[..., r] = v["vL"][..., r] / (v["s"][..., r] + e) + v["vU"][..., r] / (e - v["s"][..., r])
    A = [np.eye(6) + P.dt * to.jac_f(v["x"][k], params) for k in range(N)]
    H = []
    for k in range(N + 1):
        h = 2.0 * Q + np.diag(sx[k])
        if k < N:
            h = h - P.dt * to.hess_f_contract(v["x"][k], v["yc"][k + 1], params)
        H.append(h)
    lin = _block_lin(P)
    blocks = [[lin(v["x"][k], j, v["w"][k, j], v["yd"][k, j]) for j in range(2 * M)] for k in range(N + 1)]
    return {"N": N, "M": M, "Q": Q, "R": R, "A": A, "B": P.dt * to.B_F, "H": H, "su": su, "sw": sw, "ss": ss,
            "blocks": blocks}


def dense_obca_vjp(P, it, gX, gU, cond=False, sparse=False):
    """The un-condensed Newton matrix, variables stage by stage (x 6, u 2 (k < N), then per block w 8, s 4), rows y_c
    then y_d.  sparse: the same matrix through scipy.sparse and SuperLU (the drivers' shape has 19,000 unknowns)."""
    ln = linearise(P, it)
    N, nb = ln["N"], 2 * ln["M"]
    per = [6 + (2 if k < N else 0) + 12 * nb for k in range(N + 1)]
    off = np.concatenate([[0], np.cumsum(per)])
    n = int(off[-1])
    mc, md = 6 * (N + 1), 4 * nb * (N + 1)
    nt = n + mc + md
    K, trip = (None, ([], [], [])) if sparse else (np.zeros((nt, nt)), None)
    rhs = np.zeros(nt)

    def add(r0, c0, M):
        """K[r0:, c0:] += M, and for a constraint row (r0 >= n) its transpose too."""
        M = np.asarray(M, dtype=np.float64)
        if sparse:
            rr, cc = np.indices(M.shape)
            for ri, ci in ((rr + r0, cc + c0),) + (((cc + c0, rr + r0),) if r0 >= n else ()):
                trip[0].append(ri.ravel())
                trip[1].append(ci.ravel())
                trip[2].append(M.ravel())
        else:
            K[r0:r0 + M.shape[0], c0:c0 + M.shape[1]] += M
            if r0 >= n:
                K[c0:c0 + M.shape[1], r0:r0 + M.shape[0]] += M.T
    ox = lambda k: int(off[k])  # noqa: E731
    ou = lambda k: int(off[k]) + 6  # noqa: E731
    ow = lambda k, j: int(off[k]) + 6 + (2 if k < N else 0) + 12 * j  # noqa: E731
    for k in range(N + 1):
        add(ox(k), ox(k), ln["H"][k])
        rhs[ox(k):ox(k) + 6] = gX[k]
        rc = n + 6 * k
        add(rc, ox(k), np.eye(6))  # x_0 - x_init;  x_k - (x_{k-1} + dt f)
        if k < N:
            add(ou(k), ou(k), 2.0 * ln["R"] + np.diag(ln["su"][k]))
            rhs[ou(k):ou(k) + 2] = gU[k]
            add(rc + 6, ox(k), -ln["A"][k])
            add(rc + 6, ou(k), -ln["B"])
        for j in range(nb):
            Jx, Jw, Hxx, Hxw, Hw = ln["blocks"][k][j]
            w0, s0, rd = ow(k, j), ow(k, j) + 8, n + mc + 4 * (k * nb + j)
            add(ox(k), ox(k), Hxx)
            add(ox(k), w0, Hxw)
            add(w0, ox(k), Hxw.T)
            add(w0, w0, Hw + np.diag(ln["sw"][k, j]))
            add(s0, s0, np.diag(ln["ss"][k, j]))
            add(rd, ox(k), Jx)
            add(rd, w0, Jw)
            add(rd, s0, -np.eye(4))
    if sparse:  # SuperLU, then two refinement steps with the residual in extended precision
        import scipy.sparse as sp
        import scipy.sparse.linalg as spl
        Kc = sp.coo_matrix((np.concatenate(trip[2]), (np.concatenate(trip[0]), np.concatenate(trip[1]))),
                           shape=(nt, nt)).tocsc()
        lu_ = spl.splu(Kc)
        lam = lu_.solve(rhs)
        Ko = Kc.tocoo()
        for _ in range(2):
            prod = np.zeros(rhs.size, dtype=np.longdouble)
            np.add.at(prod, Ko.row, Ko.data.astype(np.longdouble) * lam[Ko.col].astype(np.longdouble))
            lam = lam + lu_.solve(np.asarray(rhs.astype(np.longdouble) - prod, dtype=np.float64))
    else:
        lam = np.linalg.solve(K, rhs)
    lx = np.array([lam[ox(k):ox(k) + 6] for k in range(N + 1)])
    lu = np.array([lam[ou(k):ou(k) + 2] for k in range(N)])
    out = {"x0": lam[n:n + 6].copy(), "xref": 2.0 * lx @ ln["Q"], "uref": 2.0 * lu @ ln["R"]}
    if cond and not sparse:
        out["cond"] = float(np.linalg.cond(K))
    return out


def eliminate_block(Jx, Jw, Hxx, Hxw, Hw, sw, ss):
    """The kernel's block elimination: partially pivoted LU and back-substitution on [K_b | C],
    K_b = [[D, 0, Jw'], [0, Sigma_s, -I], [Jw, -I, 0]], C = [Hxw'; 0; Jx]; returns (Hxx - C' K_b^-1 C symmetrised from its upper triangle, ok)."""
    Kb = np.zeros((16, 20))
    Kb[:8, :8] = Hw + np.diag(sw)
    Kb[:8, 12:16] = Jw.T
    Kb[8:12, 8:12] = np.diag(ss)
    Kb[8:12, 12:16] = -np.eye(4)
    Kb[12:16, :8] = Jw
    Kb[12:16, 8:12] = -np.eye(4)
    Kb[:8, 16:] = Hxw.T
    Kb[12:16, 16:] = Jx
    Cm = Kb[:, 16:].copy()
    used = np.zeros(16, dtype=bool)
    row_of = np.full(16, -1)  # the row (lane) that pivots on column c
    for c in range(16):
        mag = np.where(used, -1.0, np.abs(Kb[:, c]))
        p = int(np.argmax(mag))  # (the first of equal magnitudes: the lowest lane)
        piv = Kb[p, c]
        if not (np.isfinite(piv) and piv != 0.0):
            return np.zeros((4, 4)), False
        used[p] = True
        row_of[c] = p
        prow = Kb[p].copy()
        for r in range(16):
            if not used[r]:
                f = Kb[r, c] / piv
                Kb[r] = Kb[r] - f * prow
    X = np.zeros((16, 4))  # row = unknown
    done = np.zeros(16, dtype=bool)
    for c in range(15, -1, -1):
        p = row_of[c]
        X[c] = Kb[p, 16:] / Kb[p, c]
        done[p] = True
        for r in range(16):
            if not done[r]:
                Kb[r, 16:] = Kb[r, 16:] - Kb[r, c] * X[c]
    add = np.zeros((4, 4))
    for a in range(4):
        for b in range(a, 4):
            add[a, b] = add[b, a] = Hxx[a, b] - float(Cm[:, a] @ X[:, b])
    return add, bool(np.all(np.isfinite(add)))


def solve2(G, H):
    """The kernel's 2x2 solve with G_k: elimination on the larger diagonal (the determinant form cancels when the
    eliminated blocks make B' P B close to rank one).  H (2,) or (2, n)."""
    sw = G[1, 1] > G[0, 0]
    d0, d1 = (G[1, 1], G[0, 0]) if sw else (G[0, 0], G[1, 1])
    b0, b1 = (H[1], H[0]) if sw else (H[0], H[1])
    m = G[0, 1] / d0
    sc = d1 - m * G[0, 1]
    x1 = (b1 - m * b0) / sc
    x0 = (b0 - G[0, 1] * x1) / d0
    return np.array([x1, x0]) if sw else np.array([x0, x1])


def block_matrix(Jx, Jw, Hxx, Hxw, Hw, sw, ss):
    """K_b (16,16) and C (16,4) of a block, rows and unknowns in the order w 8, s 4, y_d 4."""
    Kb = np.zeros((16, 16))
    Kb[:8, :8] = Hw + np.diag(sw)
    Kb[:8, 12:16] = Jw.T
    Kb[8:12, 8:12] = np.diag(ss)
    Kb[8:12, 12:16] = -np.eye(4)
    Kb[12:16, :8] = Jw
    Kb[12:16, 8:12] = -np.eye(4)
    C = np.zeros((16, 4))
    C[:8] = Hxw.T
    C[12:] = Jx
    return Kb, C


def factor_block(Kb):
    """The refinement pass's factorisation: the same pivoting as eliminate_block on K_b alone, the multipliers kept in
    place of the eliminated entries.  Returns (LU rows, row_of, col_of) or None."""
    F = Kb.copy()
    used = np.zeros(16, dtype=bool)
    row_of, col_of = np.full(16, -1), np.full(16, -1)
    for c in range(16):
        p = int(np.argmax(np.where(used, -1.0, np.abs(F[:, c]))))
        piv = F[p, c]
        if not (np.isfinite(piv) and piv != 0.0):
            return None
        used[p] = True
        row_of[c], col_of[p] = p, c
        for r in range(16):
            if not used[r]:
                f = F[r, c] / piv
                F[r, c] = f
                F[r, c + 1:] = F[r, c + 1:] - f * F[p, c + 1:]
    return F, row_of, col_of


def solve_block(fac, rhs):
    """One right-hand side through factor_block's factors (equation r in entry r); the solution by unknown."""
    F, row_of, col_of = fac
    y = np.array(rhs, dtype=np.float64)
    for c in range(16):
        p = row_of[c]
        for r in range(16):
            if col_of[r] > c:
                y[r] = y[r] - F[r, c] * y[p]
    x = np.zeros(16)
    for c in range(15, -1, -1):
        p = row_of[c]
        x[c] = y[p] / F[p, c]
        for r in range(16):
            if col_of[r] < c:
                y[r] = y[r] - F[r, c] * x[c]
    return x


def _sweeps(ln, H, gX, gU):
    """One backward and one forward sweep over the stage system with the Hessians H: (lx, lu, p_0) or None."""
    N, A, Bm = ln["N"], ln["A"], ln["B"]
    Pm = H[N]
    p = np.array(gX[N], dtype=np.float64)
    Ks, kap = [None] * N, [None] * N
    for k in range(N - 1, -1, -1):
        Mm = Pm @ A[k]
        G = 2.0 * ln["R"] + np.diag(ln["su"][k]) + Bm.T @ Pm @ Bm
        d0 = max(G[0, 0], G[1, 1])
        sc = min(G[0, 0], G[1, 1]) - G[0, 1] / d0 * G[0, 1]
        if not (d0 > 0.0 and sc > 0.0 and np.isfinite(d0) and np.isfinite(sc)):
            return None
        Hm = Bm.T @ Mm
        Ks[k] = solve2(G, Hm)
        kap[k] = solve2(G, gU[k] + Bm.T @ p)
        p = gX[k] + A[k].T @ (p - Pm @ (Bm @ kap[k]))
        if k > 0:
            Pm = H[k] + (A[k].T @ Mm - Hm.T @ Ks[k])
    lx = np.zeros((N + 1, 6))
    lu = np.zeros((N, 2))
    for k in range(N):
        lu[k] = -Ks[k] @ lx[k] + kap[k]
        lx[k + 1] = A[k] @ lx[k] + Bm @ lu[k]
    return lx, lu, p


REFINE_STEPS = 3  # obca_vjp_kernel's kRefine


def model_obca_vjp(P, it, gX, gU, steps=REFINE_STEPS):
    """The kernel's route: block elimination, addends in block order, one backward and one forward sweep; then `steps`
    refinement steps on the un-condensed system.  Per step and block v = -K_b^-1 C lx_pose, the block rows' residual
    r_b = -(C lx_pose + K_b v) and t = K_b^-1 r_b through the kept factors; lam_y from the x-rows,
    ly_k = gX_k - H0_k lx_k - sum_b (Hxx lx_pose + C' v) + A_k' ly_{k+1}, so that only the input rows
    (ru_k = gU_k - R_k lu_k + B' ly_{k+1}) and the folded block rows (-C' t on the pose) carry a residual; the same
    sweeps on that right-hand side give the correction, and dL/dx_init = ly_0 + its p_0."""
    ln = linearise(P, it)
    N, nb, A, Bm = ln["N"], 2 * ln["M"], ln["A"], ln["B"]
    out = {"x0": np.zeros(6), "xref": np.zeros((N + 1, 6)), "uref": np.zeros((N, 2)), "ok": False}
    H, facs = [], {}
    for k in range(N + 1):
        h = ln["H"][k].copy()
        if k > 0:  # (x_0 is pinned: its blocks do not enter)
            for j in range(nb):
                add, ok = eliminate_block(*ln["blocks"][k][j], ln["sw"][k, j], ln["ss"][k, j])
                if not ok:
                    return out
                h[:4, :4] += add
        H.append(h)
    first = _sweeps(ln, H, gX, gU)
    if first is None:
        return out
    lx, lu, x0 = first
    for _ in range(steps):
        w = np.zeros((N + 1, 4))     # sum_b (Hxx lx_pose + C' v)
        fold = np.zeros((N + 1, 6))  # -sum_b C' t on the pose
        for k in range(1, N + 1):
            for j in range(nb):
                blk = ln["blocks"][k][j]
                if (k, j) not in facs:  # (the kernel factors again in every step: the same factors)
                    Kb, C = block_matrix(*blk, ln["sw"][k, j], ln["ss"][k, j])
                    facs[k, j] = (Kb, C, factor_block(Kb))
                Kb, C, fac = facs[k, j]
                if fac is None:
                    return out
                b0 = -(C @ lx[k, :4])
                v = solve_block(fac, b0)
                t = solve_block(fac, b0 - Kb @ v)
                w[k] += blk[2] @ lx[k, :4] + C.T @ v
                fold[k, :4] -= C.T @ t
        ly = np.zeros((N + 2, 6))
        for k in range(N, -1, -1):
            ly[k] = gX[k] - ln["H"][k] @ lx[k]
            ly[k, :4] -= w[k]
            if k < N:
                ly[k] += A[k].T @ ly[k + 1]
        ru = np.array([gU[k] - (2.0 * ln["R"] + np.diag(ln["su"][k])) @ lu[k] + Bm.T @ ly[k + 1] for k in range(N)])
        second = _sweeps(ln, H, fold, ru)
        if second is None:
            return out
        lx, lu, x0 = lx + second[0], lu + second[1], ly[0] + second[2]
    out.update(x0=x0, xref=2.0 * lx @ ln["Q"], uref=2.0 * lu @ ln["R"])
    out["ok"] = bool(all(np.all(np.isfinite(out[k])) for k in KEYS))
    return out


def group_err(a, b, keys=KEYS):
    """Largest absolute difference per group."""
    return {k: float(np.max(np.abs(np.asarray(a[k]) - np.asarray(b[k])))) for k in keys}


def group_max(a):
    return {k: float(np.max(np.abs(np.asarray(a[k])))) for k in KEYS}


def oracle_fd_vjp(P, x0, xr, ur, gX, gU, h=1e-4):
    """Central differences of L = sum(gX * X) + sum(gU * U) over the oracle's solve in x_init, xref and uref, every
    direction in one batch.  Returns (iterate of the centre solve, its status, dict(x0, xref, uref))."""
    N, M = P.N, P.M
    sizes = (6, 6 * (N + 1), 2 * N)
    o = np.cumsum((0,) + sizes)
    theta = np.concatenate([x0.reshape(-1), xr.reshape(-1), ur.reshape(-1)])
    npar = theta.size
    ts = np.repeat(theta[None], 2 * npar + 1, axis=0)
    for c in range(npar):
        ts[1 + 2 * c, c] += h
        ts[2 + 2 * c, c] -= h
    z, st, _, _, I = co.obca_solve_batch(P, ts[:, o[0]:o[1]], xref=ts[:, o[1]:o[2]].reshape(-1, N + 1, 6),
                                         uref=ts[:, o[2]:o[3]].reshape(-1, N, 2), iterate=True)
    assert np.all(st == 0), np.unique(st)
    X, U, _, _ = co.obca_split(z, N, M)
    Lv = (X * gX).sum(axis=(1, 2)) + (U * gU).sum(axis=(1, 2))
    d = (Lv[1::2] - Lv[2::2]) / (2.0 * h)
    return I[0], int(st[0]), {"x0": d[o[0]:o[1]], "xref": d[o[1]:o[2]].reshape(N + 1, 6),
                              "uref": d[o[2]:o[3]].reshape(N, 2)}
