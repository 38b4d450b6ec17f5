"""Test helper (numpy only): reference algebra for the multiplier export and the x_init sensitivities.

Two independent routes to d(solution)/d(x_init) at a primal-dual point of the tracking NLP:

* ``dense_sensitivity``: the dense Newton matrix [[W + Sigma, J'], [J, 0]] from the oracle's ``TrackingNLP`` pieces
  (``jacobian``, ``weights``, ``hess_f_contract``), right-hand side I in the x_0 - x_init rows, ``numpy.linalg.solve``.
  With ``pinned`` it is the active-set form instead: those variables are held by extra rows and carry no Sigma.
* ``riccati_sensitivity``: a float64 stage-wise Riccati pass, the CPU model of track_sens_kernel (tt_sens.hip): the
  same recursion the kernel runs, written with dense 6x6 numpy products.

``dual`` is the export layout of include/ttmpc.h: (N+1, 22) = y 6 | z_L 8 | z_U 8 per stage, IPOPT's signs
(grad f + J' y - z_L + z_U = 0, z >= 0).  The two input sets of the tests are built here as well.
"""
from __future__ import annotations

import numpy as np

from oracle import ttmpc_oracle as to

P = {"M": 0.15, "L1": 7.05, "L2": 12.45, "W1": 3.05, "W2": 2.95, "dt": 0.05}
RELAX = 1e-8  # IPOPT bound_relax_factor, as track_kernel applies it


# ---- the two input sets -----------------------------------------------------------------------------------------
def case_free(pattern="mpc_diag"):
    """N = 8, B = 8, default box: no variable near a bound at the optimum.  pattern: a weight form / bound pattern of
    tests/track_patterns.py (the inputs are the same under each)."""
    from track_patterns import nlp_of
    from ttmpc.scenarios import synthetic_batch
    x0, xr, ur = synthetic_batch(8, 8, seed=3, psi_range=0.3)
    return nlp_of(pattern, 8, P), x0, xr, ur


def case_active(pattern="mpc_diag"):
    """N = 10, B = 6, inputs boxed to -+(0.3, 0.02) (the finiteness pattern of the default box) and x_init moved away
    from the reference: 13 to 18 active input bounds per instance."""
    from ttmpc.scenarios import synthetic_batch
    x0, xr, ur = synthetic_batch(6, 10, seed=3, psi_range=0.3)
    for b in range(6):
        x0[b, 0] += 2.0 * b
        x0[b, 1] += 3.0 * b
        x0[b, 5] += 1.5 * b
    from track_patterns import nlp_of
    return nlp_of(pattern, 10, P, ulb=np.array([-0.3, -0.02]), uub=np.array([0.3, 0.02])), x0, xr, ur


def case(name, pattern="mpc_diag"):
    return case_free(pattern) if name == "free" else case_active(pattern)


# ---- pieces -----------------------------------------------------------------------------------------------------
def relaxed_bounds(nlp):
    lb, ub = nlp.bounds()
    with np.errstate(invalid="ignore"):
        return lb - RELAX * np.maximum(1.0, np.abs(lb)), ub + RELAX * np.maximum(1.0, np.abs(ub))


def dual_in_z_order(dual, N):
    """(N+1,22) -> y (N+1,6), z_L (8N+6), z_U (8N+6) in the order of the decision vector."""
    d = np.asarray(dual, dtype=np.float64).reshape(N + 1, 22)
    zl = np.concatenate([d[:N, 6:14].reshape(-1), d[N, 6:12]])
    zu = np.concatenate([d[:N, 14:22].reshape(-1), d[N, 14:20]])
    return d[:, :6].copy(), zl, zu


def sigma(nlp, z, dual):
    """Sigma = z_L / (v - lb_rel) + z_U / (ub_rel - v) per variable, 0 where the bound is infinite."""
    _, zl, zu = dual_in_z_order(dual, nlp.N)
    lbr, ubr = relaxed_bounds(nlp)
    s = np.zeros(nlp.n)
    fl, fu = np.isfinite(lbr), np.isfinite(ubr)
    s[fl] += zl[fl] / (z[fl] - lbr[fl])
    s[fu] += zu[fu] / (ubr[fu] - z[fu])
    return s


def lagrangian_hessian(nlp, z, y, wq=None, wr=None):
    """W: 2 Q_w - dt sum_i y_{k+1,i} d2f_i/dx2 (x_k) on the state blocks (2 Q_w at k = N), 2 R_w on the input blocks."""
    X, _ = nlp.unpack(z)
    N, dt = nlp.N, nlp.params["dt"]
    Qw, Rw = nlp.weights(wq, wr)
    y = np.asarray(y, dtype=np.float64).reshape(N + 1, 6)
    H = np.zeros((nlp.n, nlp.n))
    for k in range(N + 1):
        o = 8 * k
        H[o:o + 6, o:o + 6] = 2.0 * Qw
        if k < N:
            H[o:o + 6, o:o + 6] -= dt * to.hess_f_contract(X[k], y[k + 1], nlp.params)
            H[o + 6:o + 8, o + 6:o + 8] = 2.0 * Rw
    return H


def stationarity(nlp, z, xref, uref, dual, wq=None, wr=None):
    """grad f + J' y - z_L + z_U at the exported multipliers (xref (N+1,6), uref (N,2))."""
    y, zl, zu = dual_in_z_order(dual, nlp.N)
    g = nlp.grad(z, np.asarray(xref).T, np.asarray(uref).T, wq, wr)
    return g + nlp.jacobian(z).T @ y.reshape(-1) - zl + zu


# ---- the multiplier export ----------------------------------------------------------------------------------------
def check_multipliers(nlp, tol, x0, xr, ur, r, w=None, label=""):
    """Signs, zeros and IPOPT's own stopping test at the exported multipliers of up to eight converged instances of a
    ``solve_ex`` result r, in the export's layout and in CasADi's."""
    from ttmpc import layout
    N, B = nlp.N, x0.shape[0]
    lb, ub = nlp.bounds()
    lbr, ubr = relaxed_bounds(nlp)
    fl, fu = np.isfinite(lb), np.isfinite(ub)
    nb = int(fl.sum() + fu.sum())
    m = 6 * (N + 1) + nb
    ok = np.flatnonzero(r.status == 0)
    assert ok.size > 0
    pick = ok[:: max(1, ok.size // 8)][:8]
    zz = layout.pack(r.X, r.U)
    for b in pick:
        y, zl, zu = dual_in_z_order(r.dual[b], N)
        assert np.all(zl >= 0.0) and np.all(zu >= 0.0)
        assert np.all(zl[~fl] == 0.0) and np.all(zu[~fu] == 0.0)
        assert np.all(r.dual[b, N, 12:14] == 0.0) and np.all(r.dual[b, N, 20:22] == 0.0)
        wq, wr = (None, None) if w is None else (w[b, :6], w[b, 6:])
        res = stationarity(nlp, zz[b], xr[b], ur[b], r.dual[b], wq, wr)
        sz = float(np.sum(zl) + np.sum(zu))
        s_d = max(100.0, (float(np.sum(np.abs(y))) + sz) / m) / 100.0
        s_c = max(100.0, sz / nb) / 100.0
        dinf = float(np.max(np.abs(res)))
        compl = max(float(np.max(zl[fl] * (zz[b][fl] - lbr[fl]))), float(np.max(zu[fu] * (ubr[fu] - zz[b][fu]))))
        print(f"{label} N={N} instance {b}: dual inf {dinf:.3e} (bound {2 * tol * s_d:.3e}), "
              f"compl {compl:.3e} (bound {2 * tol * s_c:.3e})")
        assert dinf <= 2.0 * tol * s_d
        assert compl <= 2.0 * tol * s_c
        # CasADi's view of the same numbers
        lam_g, lam_x = layout.casadi_multipliers(r.dual[b], N)
        g = nlp.grad(zz[b], xr[b].T, ur[b].T, wq, wr)
        assert np.max(np.abs(g + nlp.jacobian(zz[b]).T @ lam_g + lam_x)) <= 2.0 * tol * s_d


def optimality_error(nlp, z, x0, xref, uref, dual, wq=None, wr=None):
    """IPOPT's scaled optimality error E0 (s_max = 100) at a primal-dual point, as track_kernel's loop forms it from a
    linearisation: xref (N+1,6), uref (N,2), dual in the export layout, bounds relaxed as the kernel relaxes them.

        dinf = max |grad f + J' y - z_L + z_U|        pinf = max |c| (dynamics rows, x_0 - x_init among them)
        c0   = max |z s| over the finite bounds       s_d  = max(100, (sum|y| + sum z) / m) / 100,  m = 6 (N+1) + nb
        E0   = max(dinf / s_d, pinf, c0 / s_c)        s_c  = max(100, sum z / nb) / 100

    ``scale`` is what rounding is measured against: the largest sum of the absolute values of the terms of any single
    row of each piece (the products 2 Q_ij dx_j, y, J_ji y_j, z of a gradient row; x_{k+1}, x_k, dt f of a dynamics
    row; z |v|, z |bound| of a complementarity product), each piece divided by the scale E0 divides it by.
    Returns dict(E0, dinf, pinf, c0, s_d, s_c, scale)."""
    N, dt = nlp.N, nlp.params["dt"]
    z = np.asarray(z, dtype=np.float64)
    X, U = nlp.unpack(z)
    xref, uref = np.asarray(xref, dtype=np.float64), np.asarray(uref, dtype=np.float64)
    y, zl, zu = dual_in_z_order(dual, N)
    lb, ub = nlp.bounds()
    lbr, ubr = relaxed_bounds(nlp)
    fl, fu = np.isfinite(lb), np.isfinite(ub)
    nb = int(fl.sum() + fu.sum())
    m = 6 * (N + 1) + nb
    # stationarity
    res = stationarity(nlp, z, xref, uref, dual, wq, wr)
    Qw, Rw = nlp.weights(wq, wr)
    ax = 2.0 * np.abs(X - xref) @ np.abs(Qw) + np.abs(y)
    au = 2.0 * np.abs(U - uref) @ np.abs(Rw)
    for k in range(N):
        ax[k] += np.abs(y[k + 1]) + dt * np.abs(to.jac_f(X[k], nlp.params)).T @ np.abs(y[k + 1])
        au[k] += dt * np.abs(to.B_F).T @ np.abs(y[k + 1])
    scale_d = float(np.max(nlp.pack(ax, au) + zl + zu))
    # dynamics
    c = nlp.constraints(z, x0).reshape(N + 1, 6)
    ac = np.abs(X)
    ac[0] += np.abs(np.asarray(x0, dtype=np.float64))
    af = np.abs(to.f(X[:-1], U, nlp.params))
    p, v, tphi = nlp.params, np.abs(X[:-1, 5]), np.abs(np.tan(X[:-1, 4]))
    af[:, 3] = v * tphi / p["L1"] * (1.0 + p["M"] / p["L2"] * np.abs(np.cos(X[:-1, 3]))) \
        + v * np.abs(np.sin(X[:-1, 3])) / p["L2"]          # the one row of f that is a sum: its terms, not their sum
    ac[1:] += np.abs(X[:-1]) + dt * af
    # complementarity
    zs = np.concatenate([zl[fl] * (z[fl] - lbr[fl]), zu[fu] * (ubr[fu] - z[fu])])
    azs = np.concatenate([zl[fl] * (np.abs(z[fl]) + np.abs(lbr[fl])), zu[fu] * (np.abs(ubr[fu]) + np.abs(z[fu]))])
    sz = float(np.sum(zl[fl]) + np.sum(zu[fu]))
    s_d = max(100.0, (float(np.sum(np.abs(y))) + sz) / m) / 100.0
    s_c = max(100.0, sz / nb) / 100.0 if nb else 1.0
    dinf, pinf = float(np.max(np.abs(res))), float(np.max(np.abs(c)))
    c0 = float(np.max(np.abs(zs))) if nb else 0.0
    scale = max(scale_d / s_d, float(np.max(ac)), float(np.max(azs)) / s_c if nb else 0.0)
    return {"E0": max(dinf / s_d, pinf, c0 / s_c), "dinf": dinf, "pinf": pinf, "c0": c0, "s_d": s_d, "s_c": s_c,
            "scale": scale}


def _split(nlp, dz):
    N = nlp.N
    dX = np.empty((N + 1, 6, 6))
    dU = np.empty((N, 2, 6))
    for c in range(6):
        Xc, Uc = nlp.unpack(dz[:, c])
        dX[:, :, c], dU[:, :, c] = Xc, Uc
    return {"gain": dU[0].copy(), "dXdx0": dX, "dUdx0": dU}


def dense_sensitivity(nlp, z, y, sig=None, pinned=None, wq=None, wr=None, cond=True):
    """d z / d x_init from the dense Newton matrix.  sig: the barrier diagonal (``sigma``) or None; pinned: indices of
    variables held fixed (active-set form).  Returns dict(gain (2,6), dXdx0 (N+1,6,6), dUdx0 (N,2,6), cond); cond(K) is
    an SVD (skip it at long horizons: cond=False leaves None)."""
    n, m = nlp.n, nlp.m
    H = lagrangian_hessian(nlp, z, y, wq, wr)
    if sig is not None:
        H = H + np.diag(sig)
    J = nlp.jacobian(z)
    if pinned is not None and len(pinned):
        E = np.zeros((len(pinned), n))
        E[np.arange(len(pinned)), np.asarray(pinned)] = 1.0
        J = np.vstack([J, E])
    mm = J.shape[0]
    K = np.block([[H, J.T], [J, np.zeros((mm, mm))]])
    rhs = np.zeros((n + mm, 6))
    rhs[n:n + 6] = np.eye(6)  # c_0 = x_0 - x_init: J dz = -dc/dx_init = +I in the first six rows
    sol = np.linalg.solve(K, rhs)
    out = _split(nlp, sol[:n])
    out["cond"] = float(np.linalg.cond(K)) if cond else None
    return out


def active_set(nlp, z, act_tol=1e-6):
    lb, ub = nlp.bounds()
    with np.errstate(invalid="ignore"):
        a = (np.isfinite(lb) & (z - lb <= act_tol * np.maximum(1.0, np.abs(lb)))) | \
            (np.isfinite(ub) & (ub - z <= act_tol * np.maximum(1.0, np.abs(ub))))
    return np.flatnonzero(a)


def riccati_sensitivity(nlp, z, dual, wq=None, wr=None):
    """The kernel's recursion in float64 numpy.  Returns dict(gain, dXdx0, dUdx0, ok)."""
    N, dt = nlp.N, nlp.params["dt"]
    X, _ = nlp.unpack(z)
    y, _, _ = dual_in_z_order(dual, N)
    sg = sigma(nlp, z, dual)
    Qw, Rw = nlp.weights(wq, wr)
    Bm = dt * to.B_F
    A = [np.eye(6) + dt * to.jac_f(X[k], nlp.params) for k in range(N)]
    Pm = 2.0 * Qw + np.diag(sg[8 * N:8 * N + 6])
    Ks = [None] * N
    ok = True
    for k in range(N - 1, -1, -1):
        M = Pm @ A[k]
        G = 2.0 * Rw + np.diag(sg[8 * k + 6:8 * k + 8]) + Bm.T @ Pm @ Bm
        det = G[0, 0] * G[1, 1] - G[0, 1] * G[0, 1]
        if not (G[0, 0] > 0.0 and det > 0.0 and np.isfinite(det)):
            ok = False
            break
        Hm = Bm.T @ M
        Ks[k] = np.linalg.solve(G, Hm)
        if k > 0:
            Wk = 2.0 * Qw - dt * to.hess_f_contract(X[k], y[k + 1], nlp.params)
            Pm = Wk + np.diag(sg[8 * k:8 * k + 6]) + (A[k].T @ M - Hm.T @ Ks[k])
    dX = np.zeros((N + 1, 6, 6))
    dU = np.zeros((N, 2, 6))
    if ok:
        dX[0] = np.eye(6)
        for k in range(N):
            dU[k] = -Ks[k] @ dX[k]
            dX[k + 1] = A[k] @ dX[k] + Bm @ dU[k]
        ok = bool(np.all(np.isfinite(dX)) and np.all(np.isfinite(dU)))
    return {"gain": dU[0].copy(), "dXdx0": dX, "dUdx0": dU, "ok": ok}


def max_err(a, b):
    return max(float(np.max(np.abs(a[k] - b[k]))) for k in ("gain", "dXdx0", "dUdx0"))


def max_abs(a):
    return max(float(np.max(np.abs(a[k]))) for k in ("gain", "dXdx0", "dUdx0"))


# ---- finite differences of the CPU oracle -------------------------------------------------------------------------
def oracle_problem(nlp, **kw):
    from oracle import c_oracle as co
    return co.make_problem(nlp.N, nlp.params, nlp.Q, nlp.R, nlp.xlb, nlp.xub, nlp.ulb, nlp.uub, **kw)


def oracle_fd(nlp, x0, xr, ur, h=1e-4, wq=None, wr=None):
    """Central differences of c_oracle.solve_batch in x_init, all instances and directions in one batch.
    Returns (z (B,n), status (B,), dz (B,n,6))."""
    from oracle import c_oracle as co
    Pp = oracle_problem(nlp)
    B = x0.shape[0]
    z, st, _, _ = co.solve_batch(Pp, x0, xr, ur, wq=wq, wr=wr)
    xs = np.repeat(x0, 12, axis=0)
    for b in range(B):
        for c in range(6):
            xs[12 * b + 2 * c, c] += h
            xs[12 * b + 2 * c + 1, c] -= h
    rep = lambda a: None if a is None else np.repeat(a, 12, axis=0)  # noqa: E731
    zs, sts, _, _ = co.solve_batch(Pp, xs, rep(xr), rep(ur), wq=rep(wq), wr=rep(wr))
    assert np.all(sts == 0), sts
    zs = zs.reshape(B, 6, 2, -1)
    dz = ((zs[:, :, 0] - zs[:, :, 1]) / (2.0 * h)).transpose(0, 2, 1)
    return z, st, dz
