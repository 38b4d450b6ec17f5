"""Test helper (numpy only): reference algebra for the gradient of a tracking solve and of the closed loop with respect
to the box (xlb, xub, ulb, uub).

With the notation of ``vjp_reference`` (K (lam_z, lam_y) = (g, 0), dL/dtheta = -lam' dF/dtheta,
F = (grad f + J' y - z_L + z_U, c)) the bounds enter F only through z_L = mu / (v - l_rel) and z_U = mu / (u_rel - v),
l_rel = l - 1e-8 max(1, |l|) and u_rel = u + 1e-8 max(1, |u|) the relaxed bounds, so

    dL/dl_v = rho_l sum_k Sigma_L,k,v lam_k,v,      dL/du_v = rho_u sum_k Sigma_U,k,v lam_k,v,

Sigma_L = z_L / (v - l_rel), Sigma_U = z_U / (u_rel - v), rho = d(relaxed bound)/d(bound): 1 -+ 1e-8 sign(bound) beyond
|bound| > 1, else 1.  The states of stage 0 are left out (x_0 is pinned to x_init: lam_x,0 = 0, whatever Sigma is there).
The gradient is ordered as the kernel's g_bounds: lower bounds of (x 6, u 2), then the upper bounds of the same.

* ``dense_bounds_vjp``: the dense Newton matrix and ``numpy.linalg.solve``, then the formula.
* ``riccati_bounds_vjp``: the stage loop track_vjp_kernel's bounds instantiation runs (tt_vjp.hip), on the lam_x | lam_u
  of the Riccati sweeps of ``vjp_reference.riccati_vjp``.
* ``oracle_dual``: multipliers at an optimum of the CPU oracle (which returns none), y by least squares and z = mu / slack
  with mu read off the active bounds.
* ``oracle_fd_bounds``: central differences of ``c_oracle.solve_batch`` on problems built with a perturbed bound.
* ``weakly_active``: the instances the comparison with those differences may leave out.
* ``chain``: the closed-loop chain, ``loop_vjp_reference.sweep`` with the sum of the solves' bound terms beside it;
  ``numpy_step_vjp`` feeds it from the numpy algebra.
"""
from __future__ import annotations

import numpy as np

import loop_vjp_reference as lv
import sens_reference as sr
from oracle import ttmpc_oracle as to

RELAX = sr.RELAX
FREE = 1e19   # a bound beyond it is no bound (track_kernel's bound_mask)


def box(nlp):
    """The box of an NLP in the order of g_bounds: (lower (8,), upper (8,)) over (x 6, u 2)."""
    return np.concatenate([nlp.xlb, nlp.ulb]).astype(np.float64), np.concatenate([nlp.xub, nlp.uub]).astype(np.float64)


def with_box(nlp, lo, up):
    """A TrackingNLP like nlp with the box (lower (8,), upper (8,))."""
    return to.TrackingNLP(nlp.N, params=nlp.params, Q=nlp.Q, R=nlp.R, xlb=np.array(lo[:6]), xub=np.array(up[:6]),
                          ulb=np.array(lo[6:]), uub=np.array(up[6:]))


def finite(lo, up):
    """Which bounds the solver takes as finite."""
    return np.isfinite(lo) & (lo > -FREE), np.isfinite(up) & (up < FREE)


def relaxation_derivative(lo, up):
    """(rho_l, rho_u): d l_rel / d l and d u_rel / d u of IPOPT's bound relaxation."""
    with np.errstate(invalid="ignore"):
        rl = np.where(np.abs(lo) > 1.0, 1.0 - RELAX * np.sign(lo), 1.0)
        ru = np.where(np.abs(up) > 1.0, 1.0 + RELAX * np.sign(up), 1.0)
    return rl, ru


def _stage_sums(nlp, z, dual, lx, lu):
    """The formula on lam_x (N+1,6), lam_u (N,2): the stage loop of the kernel, one stage after the other."""
    N = nlp.N
    X, U = nlp.unpack(z)
    d = np.asarray(dual, dtype=np.float64).reshape(N + 1, 22)
    lo, up = box(nlp)
    fl, fu = finite(lo, up)
    rl, ru = relaxation_derivative(lo, up)
    g = np.zeros(16)
    for k in range(N + 1):
        for v in range(8):
            if (k == 0) if v < 6 else (k == N):
                continue
            val = X[k, v] if v < 6 else U[k, v - 6]
            lam = lx[k, v] if v < 6 else lu[k, v - 6]
            if fl[v]:
                g[v] += d[k, 6 + v] / (val - (lo[v] - RELAX * max(1.0, abs(lo[v])))) * lam * rl[v]
            if fu[v]:
                g[8 + v] += d[k, 14 + v] / ((up[v] + RELAX * max(1.0, abs(up[v]))) - val) * lam * ru[v]
    return g


def dense_bounds_vjp(nlp, z, dual, gX, gU, wq=None, wr=None, cond=True):
    """dict(bounds (16,), x0 (6,) = lam_y of the x_0 rows, lx (N+1,6), lu (N,2), cond)."""
    n, m = nlp.n, nlp.m
    y, _, _ = sr.dual_in_z_order(dual, nlp.N)
    H = sr.lagrangian_hessian(nlp, z, y, wq, wr) + np.diag(sr.sigma(nlp, z, dual))
    J = nlp.jacobian(z)
    K = np.block([[H, J.T], [J, np.zeros((m, m))]])
    lam = np.linalg.solve(K, np.concatenate([nlp.pack(gX, gU), np.zeros(m)]))
    lx, lu = nlp.unpack(lam[:n])
    return {"bounds": _stage_sums(nlp, z, dual, lx, lu), "x0": lam[n:n + 6].copy(), "lx": lx, "lu": lu,
            "cond": float(np.linalg.cond(K)) if cond else None}


def riccati_lambda(nlp, z, dual, gX, gU, wq=None, wr=None):
    """lam_x (N+1,6), lam_u (N,2) and p_0 of the backward and forward sweeps of ``vjp_reference.riccati_vjp`` (the
    same recursion, which does not return them), or None where a G_k is not positive definite."""
    N, dt = nlp.N, nlp.params["dt"]
    X, _ = nlp.unpack(z)
    y, _, _ = sr.dual_in_z_order(dual, N)
    sg = sr.sigma(nlp, z, dual)
    Qw, Rw = nlp.weights(wq, wr)
    Bm = dt * to.B_F
    A = [np.eye(6) + dt * to.jac_f(X[k], nlp.params) for k in range(N)]
    Pm = 2.0 * Qw + np.diag(sg[8 * N:8 * N + 6])
    p = np.array(gX[N], dtype=np.float64)
    Ks, kap = [None] * N, [None] * N
    for k in range(N - 1, -1, -1):
        M = Pm @ A[k]
        G = 2.0 * Rw + np.diag(sg[8 * k + 6:8 * k + 8]) + Bm.T @ Pm @ Bm
        det = G[0, 0] * G[1, 1] - G[0, 1] * G[0, 1]
        if not (G[0, 0] > 0.0 and det > 0.0 and np.isfinite(det)):
            return None
        Hm = Bm.T @ M
        Ks[k] = np.linalg.solve(G, Hm)
        kap[k] = np.linalg.solve(G, gU[k] + Bm.T @ p)
        p = gX[k] + A[k].T @ (p - Pm @ (Bm @ kap[k]))
        if k > 0:
            Wk = 2.0 * Qw - dt * to.hess_f_contract(X[k], y[k + 1], nlp.params)
            Pm = Wk + np.diag(sg[8 * k:8 * k + 6]) + (A[k].T @ M - Hm.T @ Ks[k])
    lx, lu = np.zeros((N + 1, 6)), np.zeros((N, 2))
    for k in range(N):
        lu[k] = -Ks[k] @ lx[k] + kap[k]
        lx[k + 1] = A[k] @ lx[k] + Bm @ lu[k]
    return lx, lu, p


def riccati_bounds_vjp(nlp, z, dual, gX, gU, wq=None, wr=None):
    """The kernel's recursion and stage loop.  dict(bounds (16,), x0 (6,) = p_0, ok)."""
    r = riccati_lambda(nlp, z, dual, gX, gU, wq, wr)
    if r is None:
        return {"bounds": np.zeros(16), "x0": np.zeros(6), "ok": False}
    g = _stage_sums(nlp, z, dual, r[0], r[1])
    return {"bounds": g, "x0": r[2], "ok": bool(np.all(np.isfinite(g)))}


# ---- the CPU oracle ---------------------------------------------------------------------------------------------
def slacks(nlp, z):
    """The relaxed slacks (z - l_rel, u_rel - z) per variable of the decision vector, inf where the bound is infinite."""
    lbr, ubr = sr.relaxed_bounds(nlp)
    return z - lbr, ubr - z


def oracle_dual(nlp, z, x0, xr, ur, wq=None, wr=None):
    """Multipliers at an optimum z of the CPU oracle, in the export layout (N+1, 22), and the barrier parameter they were
    rebuilt with.  y comes from ``kkt_residual``'s least squares; on an active bound the stationarity row then gives the
    bound multiplier, z_L - z_U = grad f + J' y, and mu is the median of multiplier x relaxed slack over the active
    bounds with a multiplier above 1e-3 (1e-9 where there is none).  Every multiplier is then mu / slack."""
    N = nlp.N
    y = nlp.kkt_residual(z, x0, xr.T, ur.T, wq, wr)["y"]
    r = nlp.grad(z, xr.T, ur.T, wq, wr) + nlp.jacobian(z).T @ y
    sl, su = slacks(nlp, z)
    assert np.all(sl > 0.0) and np.all(su > 0.0)
    al, au = (r > 1e-3) & (sl < 1e-6), (r < -1e-3) & (su < 1e-6)
    prod = np.concatenate([r[al] * sl[al], -r[au] * su[au]])
    mu = float(np.median(prod)) if prod.size else 1e-9
    with np.errstate(divide="ignore"):
        zl = np.where(np.isfinite(sl), mu / sl, 0.0)
        zu = np.where(np.isfinite(su), mu / su, 0.0)
    dual = np.zeros((N + 1, 22))
    dual[:, :6] = y.reshape(N + 1, 6)
    dual[:N, 6:14], dual[N, 6:12] = zl[:8 * N].reshape(N, 8), zl[8 * N:]
    dual[:N, 14:22], dual[N, 14:20] = zu[:8 * N].reshape(N, 8), zu[8 * N:]
    return dual, mu


def oracle_fd_bounds(nlp, x0, xr, ur, gX, gU, w=None, h=1e-4, tol=1e-8):
    """Central differences of L = sum(gX * X) + sum(gU * U) over c_oracle.solve_batch in the sixteen bounds: one problem
    per perturbed bound, all solved to ``tol``; the entry of an infinite bound is 0.  Returns (z (B,n), status (B,),
    d (B,16)); z is the unperturbed optimum."""
    from oracle import c_oracle as co
    B = x0.shape[0]
    kw = dict(wq=None if w is None else w[:, :6], wr=None if w is None else w[:, 6:])
    z, st, _, _ = co.solve_batch(sr.oracle_problem(nlp, tol=tol), x0, xr, ur, **kw)
    gz = np.stack([nlp.pack(gX[b], gU[b]) for b in range(B)])
    lo, up = box(nlp)
    fl, fu = finite(lo, up)
    d = np.zeros((B, 16))
    for i in range(16):
        if not (fl[i] if i < 8 else fu[i - 8]):
            continue
        L = []
        for sgn in (1.0, -1.0):
            a, b = lo.copy(), up.copy()
            (a if i < 8 else b)[i % 8] += sgn * h
            zs, sts, _, _ = co.solve_batch(sr.oracle_problem(with_box(nlp, a, b), tol=tol), x0, xr, ur, **kw)
            assert np.all(sts == 0), (i, sts)
            L.append(np.sum(zs * gz, axis=1))
        d[:, i] = (L[0] - L[1]) / (2.0 * h)
    return z, st, d


def weakly_active(nlp, z, lo=1e-7, hi=1e-3):
    """The smallest relaxed slack of z in (lo, hi), or None: a bound that is neither decided active (its Sigma
    dominates the Hessian beside it) nor inactive (its Sigma is nothing).  There the barrier solution curves on the
    scale of a difference step and the gradient depends on the final mu to first order."""
    s = np.concatenate(slacks(nlp, z))
    s = s[(s > lo) & (s < hi)]
    return float(s.min()) if s.size else None


# ---- closed loop --------------------------------------------------------------------------------------------------
def numpy_step_vjp(nlp, fn_inputs, fn_bounds, tp, c):
    """step_vjp for ``chain`` from numpy algebra on a tape dict: fn_inputs = vjp_reference.dense_vjp or riccati_vjp,
    fn_bounds = dense_bounds_vjp or riccati_bounds_vjp, per instance at the tape's (X, U, dual) of the step; failed
    solves give zeros, as the kernel does."""
    N = nlp.N
    W = tp["W"] if "W" in tp else c["w"]

    def step(t, Xr, Ur, gU):
        B = gU.shape[0]
        out = {"x0": np.zeros((B, 6)), "xref": np.zeros((B, N + 1, 6)), "uref": np.zeros((B, N, 2)), "w": np.zeros((B, 8)),
               "bounds": np.zeros((B, 16))}
        wt = W if W is None or W.ndim == 2 else W[t]
        for b in range(B):
            if tp["status"][t, b] > 1:
                continue
            wq, wr = (None, None) if wt is None else (wt[b, :6], wt[b, 6:])
            z, gX = nlp.pack(tp["X"][t, b], tp["U"][t, b]), np.zeros((N + 1, 6))
            r = fn_inputs(nlp, z, tp["dual"][t, b], Xr.T, Ur.T, gX, gU[b], wq, wr)
            for key in ("x0", "xref", "uref", "w"):
                out[key][b] = r[key]
            out["bounds"][b] = fn_bounds(nlp, z, tp["dual"][t, b], gX, gU[b], wq, wr)["bounds"]
        return out
    return step


def chain(c, step_vjp, tp, policy="track", in_plant=False):
    """``loop_vjp_reference.sweep`` on a tape dict of the case with step_vjp(t, Xr (6,N+1), Ur (2,N), gU (B,N,2)) ->
    dict(x0, xref, uref, w, bounds (B,16)) as every step's solve adjoint (gU carries dL/dU_t[0] in row 0: the chain's
    upstream gradient of the step).  The bounds enter the loop only through the solves (the plant does not clip), so
    the loop's gradient is the sum of the steps' terms: ``bounds`` (B,16) in the returned dict, beside sweep's groups."""
    N, B = c["N"], c["B"]
    acc = np.zeros((B, 16))

    def cb(t, g_u0):
        Xr, Ur = to.reference_window(c["plan_x"], c["plan_u"], c["ks"][t], N)
        gU = np.zeros((B, N, 2))
        gU[:, 0] = g_u0
        g = step_vjp(t, Xr, Ur, gU)
        acc[:] = acc + g["bounds"]
        return g

    out = lv.sweep(cb, policy, c["ks"], c["Np"], tp["S"], tp["status"], tp["active"],
                   tp["count"] if "count" in tp else tp["consec"], c["GS"], c["GU"], lv.P, lv.DIST, in_plant)
    out["bounds"] = acc
    return out
