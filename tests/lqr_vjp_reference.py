"""Test helper (numpy only): reference algebra for the adjoint of the LQR terminal score (lqr_vjp_kernel).

Forward (csrc/tt_lqr.hip, LQR_cost.py:7-41): A = I + dt df/dx(x_goal), B = dt [e5 e4], P = DARE(A, B, Q, R) symmetrised,
score = dx' P dx with dx = x_cur - x_goal.  With K = (R + B'PB)^-1 B'PA and Ac = A - BK the DARE differentiates to

    dP = Ac' dP Ac + M,    M = dQ + K' dR K + dA' P Ac + Ac' P dA,

so for upstream gradients gs = dL/dscore and GP = dL/dP, with G = gs dx dx' + (GP + GP')/2 and S = Ac S Ac' + G:

    dL/dx_cur = 2 gs P dx,  dL/dQ = S,  dL/dR = K S K',  dL/dA = 2 P Ac S,
    dL/dx_goal[m] = -2 gs (P dx)[m] + dt sum_ij (dL/dA)_ij d2f_i/dq_j dq_m.

The pieces here:

* ``doubling_dare``: a float64 restatement of the forward's structure-preserving doubling, batched over instances.  The
  finite differences of the tests run on it: scipy's Schur solution carries a residual ~1e-11 at near-stationary goals
  (P ~ 1e7), which swamps a difference quotient.
* ``doubling_dare_dd``: the same iteration on the same inputs carried in double-double (``DD``: pairs of float64, float64
  operations only), for the central differences that must resolve 1e-6 of a gradient ~10 in a score ~1e5.
* ``dense_lqr_vjp``: the formulas above with the Lyapunov equation solved densely, (I - Ac (x) Ac) vec(S) = vec(G).
* ``dense_tangent``: dP for a given M from (I - Ac' (x) Ac') vec(dP) = vec(M).
"""
from __future__ import annotations

import numpy as np

from oracle import ttmpc_oracle as to

P6 = {"M": 0.15, "L1": 7.05, "L2": 12.45, "W1": 3.05, "W2": 2.95, "dt": 0.05}
Q_TEST = np.eye(6) + 0.1 * np.diag(np.arange(6.0))
R_TEST = np.array([[10.0, 1.0], [1.0, 8.0]])
NEAR_STATIONARY = tuple(range(8)) + (95,)     # |v| <= 0.05 and the plan's own final state
SYM_Q = tuple((i, j) for i in range(6) for j in range(i, 6))
SYM_R = ((0, 0), (0, 1), (1, 1))


def lqr_case(golden_ref):
    """The goals of tests/test_gpu_lqr.py (seed 9, B = 96): -> (x_cur, x_goal), both (96,6)."""
    rng = np.random.default_rng(9)
    B = 96
    xg = golden_ref["interp_states"].T[rng.integers(0, 400, B)].copy()
    xg[:, 5] = rng.uniform(-3, 3, B)
    xg[:8, 5] = rng.uniform(-0.05, 0.05, 8)
    xg[-1] = golden_ref["interp_states"][:, -1]
    xc = xg + rng.normal(scale=0.2, size=(B, 6))
    return xc, xg


def linearise(xg, p):
    """A = I + dt df/dx(x_goal) (6,6), B = dt [e5 e4] (6,2)."""
    return np.eye(6) + p["dt"] * to.jac_f(np.asarray(xg, dtype=np.float64), p), p["dt"] * to.B_F


def doubling_dare(A, Bm, Q, R, max_doublings=64):
    """Batched SDA (Chu, Fan & Lin 2005) as lqr_kernel runs it: A, Q (n,6,6), R (n,2,2) or single matrices, Bm (6,2).
    An instance stops at its own !(max|dH| > 1e-14 max|H|), as in the kernel.  -> (P (n,6,6) symmetrised, doublings)."""
    A = np.array(np.broadcast_to(A, np.broadcast_shapes(np.shape(A), np.shape(Q))), dtype=np.float64)
    single = A.ndim == 2
    A = A.reshape(-1, 6, 6)
    n = A.shape[0]
    H = np.array(np.broadcast_to(Q, (n, 6, 6)), dtype=np.float64)
    R = np.broadcast_to(np.asarray(R, dtype=np.float64), (n, 2, 2))
    G = Bm @ np.linalg.inv(R) @ Bm.T
    I = np.eye(6)
    live = np.ones(n, dtype=bool)
    its = np.zeros(n, dtype=np.int64)
    for _ in range(max_doublings):
        if not live.any():
            break
        a, g, h = A[live], G[live], H[live]
        W = I + g @ h
        V1, V2 = np.linalg.solve(W, a), np.linalg.solve(W, g)
        At = np.swapaxes(a, 1, 2)
        hn = h + At @ h @ V1
        A[live], G[live], H[live] = a @ V1, g + a @ V2 @ At, hn
        its[live] += 1
        dH, nH = np.abs(hn - h).max(axis=(1, 2)), np.abs(hn).max(axis=(1, 2))
        idx = np.flatnonzero(live)
        live[idx[~(dH > 1e-14 * nH) | ~np.isfinite(nH)]] = False
    its[live] = -1
    P = 0.5 * (H + np.swapaxes(H, 1, 2))
    return (P[0], int(its[0])) if single else (P, its)


# ---- the same iteration carried in double-double ----------------------------------------------------------------
def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _quick_two_sum(a, b):
    s = a + b
    return s, b - (s - a)


def _two_prod(a, b):
    """a b = p + e exactly (Dekker's split: numpy has no fused multiply-add)."""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


class DD:
    """Double-double arrays (Dekker 1971, Knuth): value = hi + lo with |lo| <= ulp(hi)/2, about 32 significant digits
    from float64 operations alone.  +, -, *, /, @ over the last two axes, indexing and assignment as for arrays."""
    __slots__ = ("hi", "lo")

    def __init__(self, hi, lo=None):
        self.hi = np.asarray(hi, dtype=np.float64)
        self.lo = np.zeros_like(self.hi) if lo is None else np.asarray(lo, dtype=np.float64)

    @staticmethod
    def of(x):
        return x if isinstance(x, DD) else DD(x)

    def __getitem__(self, k):
        return DD(self.hi[k], self.lo[k])

    def __setitem__(self, k, v):
        v = DD.of(v)
        self.hi[k], self.lo[k] = v.hi, v.lo

    def copy(self):
        return DD(self.hi.copy(), self.lo.copy())

    def __neg__(self):
        return DD(-self.hi, -self.lo)

    def __add__(self, o):
        o = DD.of(o)
        s1, s2 = _two_sum(self.hi, o.hi)
        t1, t2 = _two_sum(self.lo, o.lo)
        s1, s2 = _quick_two_sum(s1, s2 + t1)
        return DD(*_quick_two_sum(s1, s2 + t2))

    def __sub__(self, o):
        return self + (-DD.of(o))

    def __mul__(self, o):
        o = DD.of(o)
        p, e = _two_prod(self.hi, o.hi)
        return DD(*_quick_two_sum(p, e + (self.hi * o.lo + self.lo * o.hi)))

    def __truediv__(self, o):
        o = DD.of(o)
        q1 = self.hi / o.hi
        r = self - o * q1
        q2 = r.hi / o.hi
        r = r - o * q2
        return DD(*_quick_two_sum(q1, q2)) + DD(r.hi / o.hi)

    def T(self):
        return DD(np.swapaxes(self.hi, -1, -2), np.swapaxes(self.lo, -1, -2))

    def __matmul__(self, o):
        o = DD.of(o)
        acc = self[..., :, 0, None] * o[..., None, 0, :]
        for k in range(1, self.hi.shape[-1]):
            acc = acc + self[..., :, k, None] * o[..., None, k, :]
        return acc

    def value(self):
        return self.hi + self.lo


def _dd_concat(a, b, axis):
    return DD(np.concatenate([a.hi, b.hi], axis=axis), np.concatenate([a.lo, b.lo], axis=axis))


def _dd_solve(W, Rhs):
    """W^-1 Rhs, batched Gauss-Jordan with partial pivoting (as the kernel's 6x18 sweep)."""
    M = _dd_concat(W, Rhs, 2)
    ar = np.arange(M.hi.shape[0])
    for c in range(6):
        r = c + np.abs(M.hi[:, c:, c]).argmax(axis=1)
        row = M[ar, c].copy()
        M[ar, c] = M[ar, r]
        M[ar, r] = row
        M[:, c] = M[:, c] / M[:, c, c][:, None]
        f = M[:, :, c].copy()
        f[:, c] = 0.0
        M = M - f[:, :, None] * M[:, c][:, None, :]
    return M[:, :, 6:]


def doubling_dare_dd(A, Bm, Q, R, max_doublings=64):
    """``doubling_dare`` carried in double-double: the same iteration on the same float64 inputs, every operation a
    ``DD`` one.  The float64 iteration returns P to about 1e-16 cond(DARE), 1e-10 relative at a near-stationary goal;
    a central difference of a score ~1e5 with h = 1e-4 then cannot resolve a gradient ~10 (the R group), and goals that
    close to standstill also occur among the draws from U(-3, 3).  An instance stops at !(max|dH| > 1e-20 max|H|): the
    iteration is quadratic, so the step after that is exact to working precision.  A, Q (n,6,6), R (n,2,2) or single
    matrices, Bm (6,2).  -> (P as a DD (n,6,6), symmetrised; doublings)."""
    A = np.array(np.broadcast_to(A, np.broadcast_shapes(np.shape(A), np.shape(Q))), dtype=np.float64).reshape(-1, 6, 6)
    n = A.shape[0]
    A = DD(A)
    H = DD(np.array(np.broadcast_to(Q, (n, 6, 6)), dtype=np.float64))
    R = DD(np.array(np.broadcast_to(R, (n, 2, 2)), dtype=np.float64))
    det = R[:, 0, 0] * R[:, 1, 1] - R[:, 0, 1] * R[:, 1, 0]
    Ri = DD(np.zeros((n, 2, 2)))
    Ri[:, 0, 0], Ri[:, 0, 1] = R[:, 1, 1] / det, -R[:, 0, 1] / det
    Ri[:, 1, 0], Ri[:, 1, 1] = -R[:, 1, 0] / det, R[:, 0, 0] / det
    Bd = DD(np.array(np.broadcast_to(Bm, (n, 6, 2)), dtype=np.float64))
    G = Bd @ Ri @ Bd.T()
    I = DD(np.eye(6)[None])
    live = np.ones(n, dtype=bool)
    its = np.zeros(n, dtype=np.int64)
    for _ in range(max_doublings):
        if not live.any():
            break
        a, g, h = A[live], G[live], H[live]
        V = _dd_solve(g @ h + I, _dd_concat(a, g, 2))
        V1, V2, At = V[:, :, :6], V[:, :, 6:], a.T()
        d = At @ (h @ V1)
        hn = h + d
        A[live], G[live], H[live] = a @ V1, g + a @ (V2 @ At), hn
        its[live] += 1
        dH, nH = np.abs(d.hi).max(axis=(1, 2)), np.abs(hn.hi).max(axis=(1, 2))
        idx = np.flatnonzero(live)
        live[idx[~(dH > 1e-20 * nH) | ~np.isfinite(nH)]] = False
    its[live] = -1
    return (H + H.T()) * 0.5, its


def gain(A, Bm, P, R):
    """K = (R + B'PB)^-1 B'PA (2,6) and Ac = A - BK."""
    K = np.linalg.solve(R + Bm.T @ P @ Bm, Bm.T @ P @ A)
    return K, A - Bm @ K


def lyapunov_matrix(Ac):
    """I - Ac (x) Ac on row-major vec: (I - Ac (x) Ac) vec(S) = vec(S - Ac S Ac')."""
    return np.eye(36) - np.kron(Ac, Ac)


def goal_hessian_term(xg, gA, p):
    """dt sum_ij gA_ij d2f_i/dq_j dq_m, m = 0..5, through the oracle's hess_f_contract (w = gA[:, j], row j)."""
    out = np.zeros(6)
    for j in range(6):
        out += to.hess_f_contract(xg, gA[:, j], p)[j]
    return p["dt"] * out


def goal_tangent(xg, dxg, p):
    """dA = dt sum_m d(df/dx)/dq_m dxg_m (6,6): row i is (d2f_i/dq2) dxg."""
    return p["dt"] * np.array([to.hess_f_contract(xg, np.eye(6)[i], p) @ dxg for i in range(6)])


def dense_lqr_vjp(xc, xg, P, R, gs, GP, params):
    """The adjoint of one instance at a given P (6,6).  gs: float, GP: (6,6) or None.
    -> dict(g_x_cur, g_x_goal (6,), g_Q, g_A (6,6), g_R (2,2), K, Ac, S, G, cond = cond(I - Ac (x) Ac))."""
    xc, xg, P, R = (np.asarray(a, dtype=np.float64) for a in (xc, xg, P, R))
    A, Bm = linearise(xg, params)
    K, Ac = gain(A, Bm, P, R)
    dx = xc - xg
    G = gs * np.outer(dx, dx)
    if GP is not None:
        G = G + 0.5 * (GP + GP.T)
    Lm = lyapunov_matrix(Ac)
    S = np.linalg.solve(Lm, G.reshape(36)).reshape(6, 6)
    S = 0.5 * (S + S.T)
    gA = 2.0 * P @ Ac @ S
    Pdx = P @ dx
    return dict(g_x_cur=2.0 * gs * Pdx, g_x_goal=-2.0 * gs * Pdx + goal_hessian_term(xg, gA, params), g_Q=S,
                g_R=K @ S @ K.T, g_A=gA, K=K, Ac=Ac, S=S, G=G, cond=float(np.linalg.cond(Lm)))


def dense_tangent(Ac, M):
    """dP of dP = Ac' dP Ac + M, densely."""
    return np.linalg.solve(np.eye(36) - np.kron(Ac.T, Ac.T), np.asarray(M, dtype=np.float64).reshape(36)).reshape(6, 6)


def tangent_rhs(P, K, Ac, dQ=None, dR=None, dA=None):
    """M = dQ + K' dR K + dA' P Ac + Ac' P dA."""
    M = np.zeros((6, 6))
    if dQ is not None:
        M = M + dQ
    if dR is not None:
        M = M + K.T @ dR @ K
    if dA is not None:
        M = M + dA.T @ P @ Ac + Ac.T @ P @ dA
    return M


def sym_direction(n, i, j):
    d = np.zeros((n, n))
    d[i, j] = d[j, i] = 1.0
    return d
