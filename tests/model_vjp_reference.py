"""Test helper (numpy only): reference algebra for the gradient of a tracking solve, of the plant and of the closed
loop with respect to the model geometry theta = (L1, L2, M).

With the notation of ``vjp_reference`` (K (lam_z, lam_y) = (g, 0), dL/dtheta = -lam' dF/dtheta) only the dynamics rows
c_{k+1} = x_{k+1} - x_k - dt f(x_k, u_k) and the -A_k' y_{k+1} part of the stationarity rows depend on theta, so

    dL/dtheta = dt sum_{k<N} [ lam_x,k' (dJ_f(x_k)/dtheta)' y_{k+1} + lam_y,k+1' df(x_k, u_k)/dtheta ].

* ``model_derivatives``: df/dtheta (3,6) and dJ_f/dtheta (3,6,6) of ``to.f`` / ``to.jac_f``, closed forms.
* ``dense_model_vjp``: the dense Newton matrix and ``numpy.linalg.solve``, lam_y straight from the solve.
* ``riccati_model_vjp``: the stage recursion track_vjp_kernel's model instantiation runs (tt_vjp.hip): the Riccati
  sweep and the forward sweep of ``vjp_reference.riccati_vjp``, then r_k = gX_k - H_k lam_x,k, the serial sweep
  lam_y,k = r_k + A_k' lam_y,k+1 and the stage sums.
* ``oracle_fd_model``: central differences of ``c_oracle.solve_batch`` on problems built with a perturbed parameter.
* ``plant_model_vjp``: a' dS+/dtheta of ``to.plant_update``, as policy_plant_vjp_kernel's model instantiation forms it.
* ``chain``: the closed-loop chain, ``loop_vjp_reference.sweep`` with the solver's and the plant's geometry terms.
"""
from __future__ import annotations

import numpy as np

import loop_vjp_reference as lv
import sens_reference as sr
from oracle import ttmpc_oracle as to

THETA = ("L1", "L2", "M")


def model_derivatives(q, p):
    """(df/dtheta (3,6), dJ_f/dtheta (3,6,6)) at the state q; f is linear in u and B_F does not depend on theta."""
    L1, L2, M = p["L1"], p["L2"], p["M"]
    ps, ph, v = q[3], q[4], q[5]
    t, c2 = np.tan(ph), 1.0 / np.cos(ph) ** 2
    sps, cps = np.sin(ps), np.cos(ps)
    kk = 1.0 + M / L2 * cps
    df, dJ = np.zeros((3, 6)), np.zeros((3, 6, 6))
    # L1
    df[0, 2] = -v * t / L1 ** 2
    df[0, 3] = v * t * kk / L1 ** 2
    dJ[0, 2, 4] = -v * c2 / L1 ** 2
    dJ[0, 2, 5] = -t / L1 ** 2
    dJ[0, 3, 3] = -v * t * M * sps / (L1 ** 2 * L2)
    dJ[0, 3, 4] = v * c2 * kk / L1 ** 2
    dJ[0, 3, 5] = t * kk / L1 ** 2
    # L2
    df[1, 3] = v * t * M * cps / (L1 * L2 ** 2) + v * sps / L2 ** 2
    dJ[1, 3, 3] = -v * t * M * sps / (L1 * L2 ** 2) + v * cps / L2 ** 2
    dJ[1, 3, 4] = v * c2 * M * cps / (L1 * L2 ** 2)
    dJ[1, 3, 5] = t * M * cps / (L1 * L2 ** 2) + sps / L2 ** 2
    # M
    df[2, 3] = -v * t * cps / (L1 * L2)
    dJ[2, 3, 3] = v * t * sps / (L1 * L2)
    dJ[2, 3, 4] = -v * c2 * cps / (L1 * L2)
    dJ[2, 3, 5] = -t * cps / (L1 * L2)
    return df, dJ


def _stage_sum(nlp, X, y, lx, ly):
    N, dt = nlp.N, nlp.params["dt"]
    g = np.zeros(3)
    for k in range(N):
        df, dJ = model_derivatives(X[k], nlp.params)
        for i in range(3):
            g[i] += lx[k] @ (dJ[i].T @ y[k + 1]) + ly[k + 1] @ df[i]
    return dt * g


def dense_model_vjp(nlp, z, dual, gX, gU, wq=None, wr=None, cond=True):
    """dict(model (3,), x0 (6,) = lam_y of the x_0 rows, ly (N+1,6), cond)."""
    N, n, m = nlp.N, nlp.n, nlp.m
    y, _, _ = sr.dual_in_z_order(dual, N)
    H = sr.lagrangian_hessian(nlp, z, y, wq, wr) + np.diag(sr.sigma(nlp, z, dual))
    J = nlp.jacobian(z)
    K = np.block([[H, J.T], [J, np.zeros((m, m))]])
    lam = np.linalg.solve(K, np.concatenate([nlp.pack(gX, gU), np.zeros(m)]))
    lx, _ = nlp.unpack(lam[:n])
    ly = lam[n:].reshape(N + 1, 6)
    X, _ = nlp.unpack(z)
    return {"model": _stage_sum(nlp, X, y, lx, ly), "x0": ly[0].copy(), "ly": ly,
            "cond": float(np.linalg.cond(K)) if cond else None}


def riccati_model_vjp(nlp, z, dual, gX, gU, wq=None, wr=None):
    """The kernel's recursion.  dict(model (3,), x0 (6,) = p_0, ly0 (6,) = lam_y,0 of the sweep, ly (N+1,6), ok)."""
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
    out = {"model": np.zeros(3), "x0": np.zeros(6), "ly0": np.zeros(6), "ly": np.zeros((N + 1, 6)), "ok": False}
    for k in range(N - 1, -1, -1):
        M = Pm @ A[k]
        G = 2.0 * Rw + np.diag(sg[8 * k + 6:8 * k + 8]) + Bm.T @ Pm @ Bm
        det = G[0, 0] * G[1, 1] - G[0, 1] * G[0, 1]
        if not (G[0, 0] > 0.0 and det > 0.0 and np.isfinite(det)):
            return out
        Hm = Bm.T @ M
        Ks[k] = np.linalg.solve(G, Hm)
        kap[k] = np.linalg.solve(G, gU[k] + Bm.T @ p)
        p = gX[k] + A[k].T @ (p - Pm @ (Bm @ kap[k]))
        if k > 0:
            Wk = 2.0 * Qw - dt * to.hess_f_contract(X[k], y[k + 1], nlp.params)
            Pm = Wk + np.diag(sg[8 * k:8 * k + 6]) + (A[k].T @ M - Hm.T @ Ks[k])
    lx = np.zeros((N + 1, 6))
    for k in range(N):
        lu = -Ks[k] @ lx[k] + kap[k]
        lx[k + 1] = A[k] @ lx[k] + Bm @ lu
    # r_k = gX_k - H_k lam_x,k over gX_k, then lam_y,k = r_k + A_k' lam_y,k+1 from k = N - 1 down
    ly = np.zeros((N + 1, 6))
    for k in range(N + 1):
        Hk = 2.0 * Qw + np.diag(sg[8 * k:8 * k + 6])
        if k < N:
            Hk = Hk - dt * to.hess_f_contract(X[k], y[k + 1], nlp.params)
        ly[k] = gX[k] - Hk @ lx[k]
    for k in range(N - 1, -1, -1):
        ly[k] = ly[k] + A[k].T @ ly[k + 1]
    g = _stage_sum(nlp, X, y, lx, ly)
    out.update(model=g, x0=p, ly0=ly[0].copy(), ly=ly)
    out["ok"] = bool(np.all(np.isfinite(g)) and np.all(np.isfinite(ly)))
    return out


# ---- finite differences of the CPU oracle -------------------------------------------------------------------------
def with_geometry(nlp, theta):
    """A TrackingNLP like nlp with (L1, L2, M) = theta."""
    p = dict(nlp.params, L1=float(theta[0]), L2=float(theta[1]), M=float(theta[2]))
    return to.TrackingNLP(nlp.N, params=p, Q=nlp.Q, R=nlp.R, xlb=nlp.xlb, xub=nlp.xub, ulb=nlp.ulb, uub=nlp.uub)


def geometry(p):
    return np.array([p["L1"], p["L2"], p["M"]], dtype=np.float64)


# The oracle's tolerance for these differences.  At its default 1e-8 the barrier parameter stops near 1e-9, and a bound
# whose multiplier is small is then not yet decided: in the weighted ``case_active``, instance 5, the steering-rate
# input of stage 4 ends 1.5e-6 inside its bound with Sigma = z / slack of the order of the Hessian entry beside it, and
# the derivative of that end point is neither the free nor the pinned one (dL/dL1 off by 2e-5 .. 1e-4 whatever the
# multiplier guess).  Solved further the bound is active: slack 5.8e-8 at 1e-9, 1.9e-8 at 1e-10, 4.4e-10 at 1e-11,
# 6.3e-11 at 1e-12, and the difference quotient settles (error 7.6e-6, 6.0e-6, 2.5e-8, 5.2e-9).  Every case uses it.
ORACLE_FD_TOL = 1e-12


def oracle_fd_model(nlp, x0, xr, ur, gX, gU, w=None, h=1e-4, tol=ORACLE_FD_TOL):
    """Central differences of L = sum(gX * X) + sum(gU * U) over c_oracle.solve_batch in L1, L2 and M: one problem per
    perturbed parameter, all solved to ``tol``.  Returns (z (B,n), status (B,), d (B,3)); z is the unperturbed optimum."""
    from oracle import c_oracle as co
    B = x0.shape[0]
    kw = dict(wq=None if w is None else w[:, :6], wr=None if w is None else w[:, 6:])
    z, st, _, _ = co.solve_batch(sr.oracle_problem(nlp, tol=tol), x0, xr, ur, **kw)
    gz = np.stack([nlp.pack(gX[b], gU[b]) for b in range(B)])
    th = geometry(nlp.params)
    d = np.zeros((B, 3))
    for i in range(3):
        L = []
        for sgn in (1.0, -1.0):
            t = th.copy()
            t[i] += sgn * h
            zs, sts, _, _ = co.solve_batch(sr.oracle_problem(with_geometry(nlp, t), tol=tol), x0, xr, ur, **kw)
            assert np.all(sts == 0), sts
            L.append(np.sum(zs * gz, axis=1))
        d[:, i] = (L[0] - L[1]) / (2.0 * h)
    return z, st, d


# ---- plant ------------------------------------------------------------------------------------------------------
def plant_model_vjp(q, a, p, dist=None):
    """a' dS+/dtheta (...,3) of S+ = to.plant_update(q, u, p, dist): dt slip (a_2 df_2/dtheta + a_3 df_3/dtheta); the
    lateral-slip and friction terms do not depend on theta."""
    q, a = np.asarray(q, dtype=np.float64), np.asarray(a, dtype=np.float64)
    t = lv._plant_terms(q, p, dist)
    L1, L2, M = p["L1"], p["L2"], p["M"]
    ps, ph, v = q[..., 3], q[..., 4], q[..., 5]
    tph, cps, sps = np.tan(ph), np.cos(ps), np.sin(ps)
    hk = 1 + M / L2 * cps
    f2 = np.stack([-(v * tph / L1) / L1, np.zeros_like(v), np.zeros_like(v)], axis=-1)
    f3 = np.stack([v * tph / L1 * hk / L1, v * tph / L1 * (M / L2 * cps) / L2 + v * sps / L2 / L2,
                   -(v * tph / L1) * (cps / L2)], axis=-1)
    return p["dt"] * t["slip"][..., None] * (a[..., 2:3] * f2 + a[..., 3:4] * f3)


# ---- closed loop --------------------------------------------------------------------------------------------------
def chain(c, fn, tp, policy="track", in_plant=False):
    """``lv.chain`` with fn = dense_model_vjp or riccati_model_vjp, carrying the two geometry gradients: model_solver
    (B,3), the solves' terms (fn behind the signature the tape callback calls: the window is no input of theirs), and
    model_plant (B,3), ``plant_model_vjp`` of every step."""
    return lv.chain(c, lambda nlp, z, dual, Xr, Ur, gX, gU, wq, wr: fn(nlp, z, dual, gX, gU, wq, wr), tp, policy,
                    in_plant, keys=("x0", "model"), plant_model_vjp=plant_model_vjp)


def oracle_loop(c, p_solver, p_plant, in_plant=False, tape=None, dist=lv.DIST):
    """``to.closed_loop`` (policy "track") of the case with the solver's and the plant's parameter dicts apart.
    -> (S (K+1,B,6), Ua (K,B,2), status (K,B))."""
    nlp = to.TrackingNLP(c["N"], params=dict(p_solver, horizon=c["N"]))
    return to.closed_loop(lv.oracle_solver(nlp, c["w"], tape), c["x_init"], c["plan_x"], c["plan_u"], c["N"], c["T"],
                          p_plant, dist, None if in_plant else c["noise"],
                          plant_noise=c["noise"] if in_plant else None)[:3]


def oracle_loop_fd(c, in_plant=False, h=1e-4):
    """Central differences of L = sum(GS * S) + sum(GU * Ua) per instance in the solver's and in the plant's geometry.
    -> (g_model_solver (B,3), g_model_plant (B,3), every status 0)."""
    params = lambda th: dict(lv.P, **dict(zip(THETA, (float(v) for v in th))))  # noqa: E731
    fd, ok = lv.central_differences(
        c, lambda i, owners: oracle_loop(c, params(i["model_solver"]), params(i["model_plant"]), in_plant), (),
        {"model_solver": geometry(lv.P), "model_plant": geometry(lv.P)}, h, plan_entries=())
    return fd["model_solver"], fd["model_plant"], ok
