"""Test helper (numpy only): reference algebra for the scene and weight gradients of an MPC+OBCA solve
(tt_obca_vjp_params*, the params instantiation of obca_vjp_kernel).

The definition is obca_vjp_reference's: K lam = (g, 0) with the Newton matrix of the barrier problem at the exported
iterate, dL/dtheta = -lam' dF/dtheta.  With v the 16 entries of lam of one block (w = mu 4 | lam 4, s 4, y_d 4), y_d1
and lam the block's own iterate values and b = (cx + w/2, cy + h/2, -cx + w/2, -cy + h/2) the obstacle's offsets:

    g_b[i]  = -sum over stages k >= 1 and both bodies of (y_d1 v_lam[i] + lam[i] v_yd1)
    g_dmin  = -sum over all blocks (k >= 1) of v_yd1
    g_cx = g_b0 - g_b2, g_cy = g_b1 - g_b3, g_w = (g_b0 + g_b2) / 2, g_h = (g_b1 + g_b3) / 2
    g_Q[a][b] = -sum_k (lam_x,k[a] e_k[b] + lam_x,k[b] e_k[a]),  e_k = x_k - xref_k
    g_R[a][b] = -sum_k (lam_u,k[a] d_k[b] + lam_u,k[b] d_k[a]),  d_k = u_k - uref_k

Routes (all return dict(x0, xref, uref, obs (M,4), dmin, Q (6,6), R (2,2))):

* ``dense_scene_vjp``: the un-condensed matrix and numpy.linalg.solve (sparse=True: SuperLU and two refinement steps
  on an extended-precision residual); ``refined=True`` refines the dense solve the same way.
* ``model_scene_vjp``: the kernel's route.  The block unknowns v are CARRIED across the refinement steps: a block pass
  first applies the previous step's correction, v += K_b^-1 (r_b - C dlx_pose) (the record carries u = v + t with
  t = K_b^-1 r_b, so this is v = u - K_b^-1 C dlx_pose: the correction enters through dlx_pose, never through the
  rounded sum lx_pose + dlx_pose), then takes r_b = -(C lx_pose + K_b v) against the carried v, t = K_b^-1 r_b,
  fold = -C' t and w = H_xx lx_pose + C' v for the stage part.  STEPS refinement steps and one closing block pass.
* ``recomputed_scene_vjp``: v = -K_b^-1 C lx_pose from obca_vjp_kernel's final pose adjoint (optionally plus the
  block's own residual step t), for the record: it misses the cap by three to four orders where a row is active,
  because v_yd1 ~ 4e13 (n' lx_pose) and the sweep leaves n' lx_pose ~ 1e-12 with an absolute error of 1e-16.
"""
from __future__ import annotations

import numpy as np

import obca_vjp_reference as orf
from oracle import c_oracle as co

KEYS = ("x0", "xref", "uref", "obs", "dmin", "Q", "R")
STEPS = 3  # the params instantiation's kRefine (the closing block pass comes on top)


def _scene_terms(P, it, vblk):
    """vblk (N+1, 2M, 16) -> (obs (M,4), dmin).  Flat block order, stage 0 left out (x_0 is pinned)."""
    N, M = P.N, P.M
    u = orf.unpack(it, N, M)
    gb = np.zeros((M, 4))
    gd = 0.0
    for k in range(1, N + 1):
        for j in range(2 * M):
            v = vblk[k, j]
            yd1, lam = u["yd"][k, j, 0], u["w"][k, j, 4:8]
            gb[j >> 1] += -(yd1 * v[4:8] + lam * v[12])
            gd += -v[12]
    obs = np.stack([gb[:, 0] - gb[:, 2], gb[:, 1] - gb[:, 3], 0.5 * (gb[:, 0] + gb[:, 2]),
                    0.5 * (gb[:, 1] + gb[:, 3])], axis=1)
    return obs, gd


def _weight_terms(P, it, lx, lu, xref, uref):
    u = orf.unpack(it, P.N, P.M)
    e, d = u["x"] - xref, u["u"] - uref
    gQ, gR = np.zeros((6, 6)), np.zeros((2, 2))
    for k in range(P.N + 1):
        gQ -= np.outer(lx[k], e[k]) + np.outer(e[k], lx[k])
    for k in range(P.N):
        gR -= np.outer(lu[k], d[k]) + np.outer(d[k], lu[k])
    return gQ, gR


def _assemble(P, it, gX, gU):
    """The un-condensed matrix as COO triplets, its right-hand side and the index maps (obca_vjp_reference's
    ordering: per stage x 6, u 2, per block w 8, s 4; then the rows y_c, y_d)."""
    ln = orf.linearise(P, it)
    N, nb = ln["N"], 2 * ln["M"]
    per = [6 + (2 if k < N else 0) + 12 * nb for k in range(N + 1)]
    off = np.concatenate([[0], np.cumsum(per)])
    n = int(off[-1])
    mc = 6 * (N + 1)
    nt = n + mc + 4 * nb * (N + 1)
    R_, C_, V_ = [], [], []
    rhs = np.zeros(nt)

    def add(r0, c0, Mx):
        Mx = np.asarray(Mx, dtype=np.float64)
        rr, cc = np.indices(Mx.shape)
        for ri, ci in ((rr + r0, cc + c0),) + (((cc + c0, rr + r0),) if r0 >= n else ()):
            R_.append(ri.ravel())
            C_.append(ci.ravel())
            V_.append(Mx.ravel())
    ox = lambda k: int(off[k])  # noqa: E731
    ou = lambda k: int(off[k]) + 6  # noqa: E731
    ow = lambda k, j: int(off[k]) + 6 + (2 if k < N else 0) + 12 * j  # noqa: E731
    rd = lambda k, j: n + mc + 4 * (k * nb + j)  # noqa: E731
    for k in range(N + 1):
        add(ox(k), ox(k), ln["H"][k])
        rhs[ox(k):ox(k) + 6] = gX[k]
        rc = n + 6 * k
        add(rc, ox(k), np.eye(6))
        if k < N:
            add(ou(k), ou(k), 2.0 * ln["R"] + np.diag(ln["su"][k]))
            rhs[ou(k):ou(k) + 2] = gU[k]
            add(rc + 6, ox(k), -ln["A"][k])
            add(rc + 6, ou(k), -ln["B"])
        for j in range(nb):
            Jx, Jw, Hxx, Hxw, Hw = ln["blocks"][k][j]
            w0 = ow(k, j)
            add(ox(k), ox(k), Hxx)
            add(ox(k), w0, Hxw)
            add(w0, ox(k), Hxw.T)
            add(w0, w0, Hw + np.diag(ln["sw"][k, j]))
            add(w0 + 8, w0 + 8, np.diag(ln["ss"][k, j]))
            add(rd(k, j), ox(k), Jx)
            add(rd(k, j), w0, Jw)
            add(rd(k, j), w0 + 8, -np.eye(4))
    trip = (np.concatenate(R_), np.concatenate(C_), np.concatenate(V_))
    return ln, trip, rhs, nt, n, (ox, ou, ow, rd)


def _residual_ld(trip, rhs, lam):
    prod = np.zeros(rhs.size, dtype=np.longdouble)
    np.add.at(prod, trip[0], trip[2].astype(np.longdouble) * lam[trip[1]].astype(np.longdouble))
    return np.asarray(rhs.astype(np.longdouble) - prod, dtype=np.float64)


def split_lam(P, lam, n, maps):
    """lam -> (lx (N+1,6), lu (N,2), ly (N+1,6), vblk (N+1,2M,16))."""
    N, nb = P.N, 2 * P.M
    ox, ou, ow, rd = maps
    lx = np.array([lam[ox(k):ox(k) + 6] for k in range(N + 1)])
    lu = np.array([lam[ou(k):ou(k) + 2] for k in range(N)])
    ly = lam[n:n + 6 * (N + 1)].reshape(N + 1, 6).copy()
    vblk = np.zeros((N + 1, nb, 16))
    for k in range(N + 1):
        for j in range(nb):
            vblk[k, j, :12] = lam[ow(k, j):ow(k, j) + 12]
            vblk[k, j, 12:] = lam[rd(k, j):rd(k, j) + 4]
    return lx, lu, ly, vblk


def _from_lam(P, it, ln, lam, n, maps, xref, uref):
    lx, lu, _, vblk = split_lam(P, lam, n, maps)
    out = {"x0": lam[n:n + 6].copy(), "xref": 2.0 * lx @ ln["Q"], "uref": 2.0 * lu @ ln["R"]}
    out["obs"], out["dmin"] = _scene_terms(P, it, vblk)
    out["Q"], out["R"] = _weight_terms(P, it, lx, lu, xref, uref)
    return out


def dense_lam(P, it, gX, gU, sparse=False, refined=False):
    """The un-condensed solve -> (ln, lam, n, maps)."""
    ln, trip, rhs, nt, n, maps = _assemble(P, it, gX, gU)
    if sparse:
        import scipy.sparse as sp
        import scipy.sparse.linalg as spl
        lu_ = spl.splu(sp.coo_matrix((trip[2], (trip[0], trip[1])), shape=(nt, nt)).tocsc())
        lam = lu_.solve(rhs)
        for _ in range(2):
            lam = lam + lu_.solve(_residual_ld(trip, rhs, lam))
    else:
        K = np.zeros((nt, nt))
        np.add.at(K, (trip[0], trip[1]), trip[2])
        lam = np.linalg.solve(K, rhs)
        if refined:
            for _ in range(3):
                lam = lam + np.linalg.solve(K, _residual_ld(trip, rhs, lam))
    return ln, lam, n, maps


def dense_scene_vjp(P, it, gX, gU, xref, uref, sparse=False, refined=False):
    ln, lam, n, maps = dense_lam(P, it, gX, gU, sparse, refined)
    return _from_lam(P, it, ln, lam, n, maps, xref, uref)


def _condensed(ln):
    """Stage Hessians with the eliminated blocks' addends (stages k >= 1), or None."""
    N, nb = ln["N"], 2 * ln["M"]
    H = []
    for k in range(N + 1):
        h = ln["H"][k].copy()
        if k > 0:
            for j in range(nb):
                add, ok = orf.eliminate_block(*ln["blocks"][k][j], ln["sw"][k, j], ln["ss"][k, j])
                if not ok:
                    return None
                h[:4, :4] += add
        H.append(h)
    return H


def _zeros(P):
    N, M = P.N, P.M
    return {"x0": np.zeros(6), "xref": np.zeros((N + 1, 6)), "uref": np.zeros((N, 2)), "obs": np.zeros((M, 4)),
            "dmin": 0.0, "Q": np.zeros((6, 6)), "R": np.zeros((2, 2)), "ok": False}


def _finish(P, it, ln, out, lx, lu, x0, vblk, xref, uref):
    out.update(x0=x0, xref=2.0 * lx @ ln["Q"], uref=2.0 * lu @ ln["R"])
    out["obs"], out["dmin"] = _scene_terms(P, it, vblk)
    out["Q"], out["R"] = _weight_terms(P, it, lx, lu, xref, uref)
    out["ok"] = bool(all(np.all(np.isfinite(out[k])) for k in KEYS))
    return out


def _stage_step(ln, H, gX, gU, lx, lu, w, fold):
    """The stage part of a refinement step: lam_y from the x-rows with the blocks' w, the input rows' residual ru and
    the sweeps on (fold, ru) -> (ly (N+2,6), the correction (dlx, dlu, p_0) or None)."""
    N, A, Bm = ln["N"], ln["A"], ln["B"]
    ly = np.zeros((N + 2, 6))
    for k in range(N, -1, -1):
        ly[k] = gX[k] - ln["H"][k] @ lx[k]
        ly[k, :4] -= w[k]
        if k < N:
            ly[k] += A[k].T @ ly[k + 1]
    ru = np.array([gU[k] - (2.0 * ln["R"] + np.diag(ln["su"][k])) @ lu[k] + Bm.T @ ly[k + 1] for k in range(N)])
    return ly, orf._sweeps(ln, H, fold, ru)


def _carried(P, it, gX, gU, steps, each=None):
    """The params kernel's passes (module docstring): the first solve, `steps` refinement steps on the carried block
    unknowns and the closing block pass -> (ln, lx, lu, x0, ly of the last step (N+1,6), closed v, the blocks'
    (K_b, C, factors)) or None.  each(ln, lx, lu, x0, closed v) is called after every step, at the cost of one extra
    pass per step."""
    ln = orf.linearise(P, it)
    N, nb = ln["N"], 2 * ln["M"]
    H = _condensed(ln)
    first = None if H is None else orf._sweeps(ln, H, gX, gU)
    if first is None:
        return None
    lx, lu, x0 = first
    facs = {}
    for k in range(1, N + 1):
        for j in range(nb):
            Kb, C = orf.block_matrix(*ln["blocks"][k][j], ln["sw"][k, j], ln["ss"][k, j])
            fac = orf.factor_block(Kb)
            if fac is None:
                return None
            facs[k, j] = (Kb, C, fac)
    ublk = np.zeros((N + 1, nb, 16))  # the carried record u = v + t (zero before the first pass)
    dlx = lx                          # the last correction (the first solve itself before the first pass)

    def close(ub, dlx_):
        """v = u - K_b^-1 C dlx_pose on every block."""
        vb = ub.copy()
        for (k, j), (Kb, C, fac) in facs.items():
            vb[k, j] = ub[k, j] + orf.solve_block(fac, -(C @ dlx_[k, :4]))
        return vb
    ly = np.zeros((N + 2, 6))
    for _ in range(steps):
        vblk = close(ublk, dlx)
        w = np.zeros((N + 1, 4))
        fold = np.zeros((N + 1, 6))
        for (k, j), (Kb, C, fac) in facs.items():
            v = vblk[k, j]
            t = orf.solve_block(fac, -(C @ lx[k, :4]) - Kb @ v)
            w[k] += ln["blocks"][k][j][2] @ lx[k, :4] + C.T @ v
            fold[k, :4] -= C.T @ t
            ublk[k, j] = v + t
        ly, second = _stage_step(ln, H, gX, gU, lx, lu, w, fold)
        if second is None:
            return None
        dlx = second[0]
        lx, lu, x0 = lx + second[0], lu + second[1], ly[0] + second[2]
        if each is not None:
            each(ln, lx, lu, x0, close(ublk, dlx))
    return ln, lx, lu, x0, ly[:N + 1], close(ublk, dlx), facs


def model_scene_vjp(P, it, gX, gU, xref, uref, steps=STEPS, trace=None):
    """The params kernel's route (module docstring).  trace: a list that receives the result after every step's
    closing pass (the step-by-step record of DESIGN.md), at the cost of one extra pass per step."""
    each = None
    if trace is not None:
        each = lambda ln, lx, lu, x0, v: trace.append(_finish(P, it, ln, _zeros(P), lx, lu, x0, v, xref, uref))  # noqa: E731
    got = _carried(P, it, gX, gU, steps, each)
    if got is None:
        return _zeros(P)
    ln, lx, lu, x0, _, vblk, _ = got
    return _finish(P, it, ln, _zeros(P), lx, lu, x0, vblk, xref, uref)


def recomputed_scene_vjp(P, it, gX, gU, xref, uref, with_t=False, steps=orf.REFINE_STEPS):
    """obca_vjp_kernel's own route to the pose adjoint, then v = -K_b^-1 C lx_pose (+ t = K_b^-1 (b0 - K_b v))."""
    ln = orf.linearise(P, it)
    N, nb = ln["N"], 2 * ln["M"]
    out = _zeros(P)
    H = _condensed(ln)
    first = None if H is None else orf._sweeps(ln, H, gX, gU)
    if first is None:
        return out
    lx, lu, x0 = first
    facs = {}
    for k in range(1, N + 1):
        for j in range(nb):
            Kb, C = orf.block_matrix(*ln["blocks"][k][j], ln["sw"][k, j], ln["ss"][k, j])
            facs[k, j] = (Kb, C, orf.factor_block(Kb))

    def blocks(lx_):
        vb, tb = np.zeros((N + 1, nb, 16)), np.zeros((N + 1, nb, 16))
        for (k, j), (Kb, C, fac) in facs.items():
            b0 = -(C @ lx_[k, :4])
            vb[k, j] = orf.solve_block(fac, b0)
            tb[k, j] = orf.solve_block(fac, b0 - Kb @ vb[k, j])
        return vb, tb
    for _ in range(steps):
        vb, tb = blocks(lx)
        w = np.zeros((N + 1, 4))
        fold = np.zeros((N + 1, 6))
        for (k, j), (Kb, C, fac) in facs.items():
            w[k] += ln["blocks"][k][j][2] @ lx[k, :4] + C.T @ vb[k, j]
            fold[k, :4] -= C.T @ tb[k, j]
        ly, second = _stage_step(ln, H, gX, gU, lx, lu, w, fold)
        if second is None:
            return out
        lx, lu, x0 = lx + second[0], lu + second[1], ly[0] + second[2]
    vb, tb = blocks(lx)
    return _finish(P, it, ln, out, lx, lu, x0, vb + tb if with_t else vb, xref, uref)


def scales(ref):
    """The unit each group is measured in: obs and dmin share one with the position entries of g_x0 (and an inactive
    scene's 1e-11 entries need a floor), so max(max|ref| of the group, max|g_x0|); every other group its own max|ref|."""
    mx = {k: float(np.max(np.abs(np.asarray(ref[k])))) for k in KEYS}
    for k in ("obs", "dmin"):
        mx[k] = max(mx[k], mx["x0"])
    return mx


def group_err(a, b):
    return orf.group_err(a, b, KEYS)


def oracle_fd_scene(P, x0, xr, ur, gX, gU, h=1e-4, hw=1e-3):
    """Central differences of L = sum(gX * X) + sum(gU * U) over the oracle's solve in the obstacles and d_min (step
    h) and in the diagonals of Q and R (step hw).  P is restored.  Returns dict(obs (M,4), dmin, Qd (6,), Rd (2,))."""
    N, M = P.N, P.M

    def loss():
        z, st, _, _ = co.obca_solve_batch(P, x0[None], xref=xr[None], uref=ur[None])
        assert st[0] == 0, st
        X, U, _, _ = co.obca_split(z, N, M)
        return float((X[0] * gX).sum() + (U[0] * gU).sum())

    def diff(get, put, step):
        keep = get()
        put(keep + step)
        up = loss()
        put(keep - step)
        dn = loss()
        put(keep)
        return (up - dn) / (2.0 * step)

    def at(arr, i):
        return (lambda: arr[i]), (lambda v: arr.__setitem__(i, v))
    obs = np.array([diff(*at(P.obs, i), h) for i in range(4 * M)]).reshape(M, 4)
    dmin = diff(lambda: P.dmin, lambda v: setattr(P, "dmin", v), h)
    Qd = np.array([diff(*at(P.Q, 7 * i), hw) for i in range(6)])
    Rd = np.array([diff(*at(P.R, 3 * i), hw) for i in range(2)])
    return {"obs": obs, "dmin": dmin, "Qd": Qd, "Rd": Rd}
