"""Test helper (numpy only): reference algebra for the adjoint (vector-Jacobian product) of a tracking solve.

For a scalar loss L(X, U) with upstream gradient g = dL/dz (gX (N+1,6), gU (N,2)) the gradient with respect to the
parameters theta = (x_init, xref, uref, weights) of the solve is, as sIPOPT defines the sensitivity,

    K (lam_z, lam_y) = (g, 0),   K = [[W + Sigma, J'], [J, 0]],   dL/dtheta = -lam' dF/dtheta,

with F = (grad f + J' y - z_L + z_U, c).  Two routes to it, as in ``sens_reference``:

* ``dense_vjp``: the dense Newton matrix and ``numpy.linalg.solve``.  The x_init term is lam_y of the x_0 - x_init rows,
  the reference terms are 2 Q_w lam_x, 2 R_w lam_u, and the weight term is -lam_z' d(grad f)/dw taken from ``nlp.grad``
  itself (grad f is quadratic in the weights, so a central difference of it is exact).
* ``riccati_vjp``: the stage recursion track_vjp_kernel (tt_vjp.hip) runs, in float64 numpy.

With wq = wr = None the weights are ones and the weight gradient is the gradient with respect to a diagonal scaling.
Both return dict(x0 (6,), xref (N+1,6), uref (N,2), w (8,)).
"""
from __future__ import annotations

import numpy as np

import sens_reference as sr
from oracle import ttmpc_oracle as to

KEYS = ("x0", "xref", "uref", "w")


def dense_vjp(nlp, z, dual, xref, uref, gX, gU, wq=None, wr=None, cond=True):
    """xref (N+1,6), uref (N,2), gX (N+1,6), gU (N,2).  Also returns cond(K) (an SVD: skip it at long horizons)."""
    N, n, m = nlp.N, nlp.n, nlp.m
    y, _, _ = sr.dual_in_z_order(dual, N)
    H = sr.lagrangian_hessian(nlp, z, y, wq, wr) + np.diag(sr.sigma(nlp, z, dual))
    J = nlp.jacobian(z)
    K = np.block([[H, J.T], [J, np.zeros((m, m))]])
    rhs = np.concatenate([nlp.pack(gX, gU), np.zeros(m)])
    lam = np.linalg.solve(K, rhs)
    lz, ly = lam[:n], lam[n:]
    lx, lu = nlp.unpack(lz)
    Qw, Rw = nlp.weights(wq, wr)
    w0 = np.concatenate([np.ones(6) if wq is None else np.asarray(wq, float),
                         np.ones(2) if wr is None else np.asarray(wr, float)])
    gw = np.empty(8)
    for i in range(8):  # grad f is quadratic in w: the central difference with h = 1 is its derivative
        wp, wm = w0.copy(), w0.copy()
        wp[i] += 1.0
        wm[i] -= 1.0
        d = 0.5 * (nlp.grad(z, xref.T, uref.T, wp[:6], wp[6:]) - nlp.grad(z, xref.T, uref.T, wm[:6], wm[6:]))
        gw[i] = -float(lz @ d)
    return {"x0": ly[:6].copy(), "xref": 2.0 * lx @ Qw, "uref": 2.0 * lu @ Rw, "w": gw,
            "cond": float(np.linalg.cond(K)) if cond else None}


def riccati_vjp(nlp, z, dual, xref, uref, gX, gU, wq=None, wr=None):
    """The kernel's recursion.  Also returns ok (every G_k positive definite, every value finite)."""
    N, dt = nlp.N, nlp.params["dt"]
    X, U = nlp.unpack(z)
    y, _, _ = sr.dual_in_z_order(dual, N)
    sg = sr.sigma(nlp, z, dual)
    Qw, Rw = nlp.weights(wq, wr)
    Bm = dt * to.B_F
    A = [np.eye(6) + dt * to.jac_f(X[k], nlp.params) for k in range(N)]
    Pm = 2.0 * Qw + np.diag(sg[8 * N:8 * N + 6])
    p = np.array(gX[N], dtype=np.float64)
    Ks, kap = [None] * N, [None] * N
    out = {"x0": np.zeros(6), "xref": np.zeros((N + 1, 6)), "uref": np.zeros((N, 2)), "w": np.zeros(8), "ok": False}
    for k in range(N - 1, -1, -1):
        M = Pm @ A[k]
        G = 2.0 * Rw + np.diag(sg[8 * k + 6:8 * k + 8]) + Bm.T @ Pm @ Bm
        det = G[0, 0] * G[1, 1] - G[0, 1] * G[0, 1]
        if not (G[0, 0] > 0.0 and det > 0.0 and np.isfinite(det)):
            return out
        Hm = Bm.T @ M
        Ks[k] = np.linalg.solve(G, Hm)
        kap[k] = np.linalg.solve(G, gU[k] + Bm.T @ p)
        p = gX[k] + A[k].T @ (p - Pm @ (Bm @ kap[k]))  # (P_{k+1}: before the update below)
        if k > 0:
            Wk = 2.0 * Qw - dt * to.hess_f_contract(X[k], y[k + 1], nlp.params)
            Pm = Wk + np.diag(sg[8 * k:8 * k + 6]) + (A[k].T @ M - Hm.T @ Ks[k])
    lx = np.zeros((N + 1, 6))
    lu = np.zeros((N, 2))
    for k in range(N):
        lu[k] = -Ks[k] @ lx[k] + kap[k]
        lx[k + 1] = A[k] @ lx[k] + Bm @ lu[k]
    Qs, Rs = nlp.weights(None, None)
    dq = np.ones(6) if wq is None else np.asarray(wq, float)
    dr = np.ones(2) if wr is None else np.asarray(wr, float)
    e, f = X - xref, U - uref
    gw = np.zeros(8)
    for k in range(N + 1):
        gw[:6] += lx[k] * (Qs @ (dq * e[k])) + (Qs @ (dq * lx[k])) * e[k]
        if k < N:
            gw[6:] += lu[k] * (Rs @ (dr * f[k])) + (Rs @ (dr * lu[k])) * f[k]
    out.update(x0=p, xref=2.0 * lx @ Qw, uref=2.0 * lu @ Rw, w=-2.0 * gw)
    out["ok"] = bool(all(np.all(np.isfinite(out[k])) for k in KEYS))
    return out


def max_err(a, b):
    return max(float(np.max(np.abs(np.asarray(a[k]) - np.asarray(b[k])))) for k in KEYS)


def max_abs(a):
    return max(float(np.max(np.abs(a[k]))) for k in KEYS)


def random_upstream(B, N, seed=11):
    """A fixed random upstream gradient: gX (B,N+1,6), gU (B,N,2), entries in [-1, 1]."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, (B, N + 1, 6)), rng.uniform(-1.0, 1.0, (B, N, 2))


def random_weights(B, seed=7):
    """wq_wr (B,8) drawn from U(0.7, 1.4)."""
    return np.random.default_rng(seed).uniform(0.7, 1.4, (B, 8))


# ---- finite differences of the CPU oracle -------------------------------------------------------------------------
def oracle_fd_vjp(nlp, x0, xr, ur, gX, gU, w=None, h=1e-4):
    """Central differences of L = sum(gX * X) + sum(gU * U) over c_oracle.solve_batch in x_init, xref, uref and the
    weights (around ones when w is None), every instance and direction in one batch.
    Returns (z (B,n), status (B,), list of dict(x0, xref, uref, w))."""
    from oracle import c_oracle as co
    Pp = sr.oracle_problem(nlp)
    B, N = x0.shape[0], nlp.N
    w0 = np.ones((B, 8)) if w is None else np.asarray(w, dtype=np.float64)
    z, st, _, _ = co.solve_batch(Pp, x0, xr, ur, wq=None if w is None else w0[:, :6], wr=None if w is None else w0[:, 6:])
    sizes = (6, 6 * (N + 1), 2 * N, 8)
    npar = sum(sizes)
    theta = np.concatenate([x0.reshape(B, -1), xr.reshape(B, -1), ur.reshape(B, -1), w0], axis=1)  # (B, npar)
    ts = np.repeat(theta, 2 * npar, axis=0).reshape(B, npar, 2, npar)
    for c in range(npar):
        ts[:, c, 0, c] += h
        ts[:, c, 1, c] -= h
    ts = ts.reshape(-1, npar)
    o = np.cumsum((0,) + sizes)
    zs, sts, _, _ = co.solve_batch(Pp, ts[:, o[0]:o[1]], ts[:, o[1]:o[2]].reshape(-1, N + 1, 6),
                                   ts[:, o[2]:o[3]].reshape(-1, N, 2), wq=ts[:, o[3]:o[3] + 6], wr=ts[:, o[3] + 6:])
    assert np.all(sts == 0), np.unique(sts)
    zs = zs.reshape(B, npar, 2, -1)
    out = []
    for b in range(B):
        gz = nlp.pack(gX[b], gU[b])
        d = (zs[b, :, 0] - zs[b, :, 1]) @ gz / (2.0 * h)
        out.append({"x0": d[o[0]:o[1]], "xref": d[o[1]:o[2]].reshape(N + 1, 6), "uref": d[o[2]:o[3]].reshape(N, 2),
                    "w": d[o[3]:]})
    return z, st, out
