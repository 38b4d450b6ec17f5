"""Test helper (numpy only): reference algebra for the gradient of an MPC+OBCA solve in the geometry
theta = (L1, L2, Mh, W1, W2) (tt_obca_vjp_geometry*, the geometry instantiation of obca_vjp_kernel).

The definition is obca_vjp_reference's: K lam = (g, 0) with the Newton matrix of the barrier problem at the exported
iterate, dL/dtheta = -lam' dF/dtheta.  Two parts of F depend on theta.

Dynamics share (L1, L2, Mh): the dynamics rows and the -A_k' y_{k+1} part of the x-stationarity rows,

    dt sum_{k<N} [ lam_x,k' (dJ_f(x_k)/dtheta)' y_{k+1} + lam_y,k+1' df(x_k, u_k)/dtheta ]

(model_vjp_reference.model_derivatives has the closed forms), with the OBCA solve's lam and the iterate's y_c.

Block share: of a block (stage k >= 1, obstacle m, body) only the d_min row
d_0 = g' mu - (a, c) . (p - centre) + offsets' lam + d_min - s_0, (a, c) = (lam_0 - lam_2, lam_1 - lam_3), depends on
theta: through g = (hl, hw, hl, hw) and through the body centre p,

    truck    p = (X, Y) + (L1/2)(cos th, sin th),                                       hl = L1/2, hw = W1/2
    trailer  p = (X, Y) - M (cos th, sin th) - (L2/2)(cos(th+psi), sin(th+psi)),        hl = L2/2, hw = W2/2.

With l_b = y_d0 d_0, v = (v_mu 4, v_lam 4, v_s 4, v_yd 4) the block's 16 entries of lam, (va, vc) = (v_lam0 - v_lam2,
v_lam1 - v_lam3), lp the pose adjoint of the stage and, per parameter, dg = dg/dtheta, dp = dp/dtheta,
dpt = d2p/dth dtheta, dpp = d2p/dpsi dtheta, the block's share is

    -[ y_d0 ( dg' v_mu - dp . (va, vc) - ((a, c) . dpt) lp_th - ((a, c) . dpp) lp_psi ) + v_yd0 ( dg' mu - (a, c) . dp ) ].

Truck blocks feed L1 and W1, trailer blocks L2, Mh and W2.  v_yd0 is about 4e13 times a 1e-12 component of the pose
adjoint on an active row, so the kernel's route reads the CARRIED v of obca_scene_reference.model_scene_vjp.

Routes (all return obca_scene_reference's dict plus geom (5,) = block + dyn, geom_block (5,), geom_dyn (5,), in the
order L1, L2, Mh, W1, W2):

* ``dense_geometry_vjp``: the un-condensed solve of obca_scene_reference.
* ``model_geometry_vjp``: the kernel's route: model_scene_vjp's carried passes, the block terms summed in flat block
  order, the dynamics share from the final lam_x and the lam_y of the last refinement step (the kernel's sY field:
  it is not corrected again, only lam_y,0 is, and the cap holds with it).
* ``recomputed_geometry_vjp``: the block terms from v = -K_b^-1 C lx_pose of the final pose adjoint, for the record.
* ``oracle_fd_geometry``: central differences of L over the CPU oracle's solve.
* ``residual_fd_geometry``: the central difference in theta of lam' F(theta) at the fixed iterate: the closed forms
  alone, without a solve.
"""
from __future__ import annotations

import numpy as np

import model_vjp_reference as mvr
import obca_scene_reference as osr
import obca_vjp_reference as orf
from oracle import c_oracle as co
from oracle import ttmpc_oracle as to

THETA = ("L1", "L2", "Mh", "W1", "W2")
KEYS = osr.KEYS + ("geom",)
STEPS = osr.STEPS


def _case(v, obstacle):
    from ttmpc import scenarios as sc
    N, th = 6, 0.5
    xref = np.zeros((N + 1, 6))
    k = np.arange(N + 1)
    xref[:, 0] = 0.1 * v * k * np.cos(th)
    xref[:, 1] = 0.1 * v * k * np.sin(th)
    xref[:, 2] = th
    xref[:, 5] = v
    bounds = (sc.OBCA_XLB, sc.OBCA_XUB, sc.OBCA_ULB, sc.OBCA_UUB)
    return (N, dict(sc.OBCA_PARAMS), sc.OBCA_Q, sc.OBCA_R, bounds, np.array([obstacle], dtype=np.float64),
            xref[0].copy(), xref, np.zeros((N, 2)))


def case_f(obstacle=(10.07, 3.5, 2.0, 3.0)):
    """Case F: N = 6, M = 1, forward at v = 4 along the heading 0.5: the truck's front corner meets the obstacle's -x
    face (L1 and W1 get a block share).  Returns obca_vjp_reference.case_a's tuple."""
    return _case(4.0, obstacle)


def case_r(obstacle=(-14.82, -6.0, 2.0, 3.0)):
    """Case R: the same reversing at v = -4: the trailer's rear corner meets the +x face (L2, Mh and W2)."""
    return _case(-4.0, obstacle)


def params_of(P):
    return {"dt": P.dt, "L1": P.L1, "L2": P.L2, "M": P.Mh}


def get_theta(P):
    return np.array([getattr(P, n) for n in THETA])


def set_theta(P, th):
    for n, v in zip(THETA, th):
        setattr(P, n, float(v))


# ---- the closed forms ---------------------------------------------------------------------------------------------
def block_share(xk, j, wv, yd0, lp, v):
    """The share of one block (module docstring) -> (5,)."""
    th, ps = xk[2], xk[3]
    mu, lam = wv[:4], wv[4:8]
    a, c = lam[0] - lam[2], lam[1] - lam[3]
    va, vc = v[4] - v[6], v[5] - v[7]
    ve, vo = v[0] + v[2], v[1] + v[3]
    me, mo = mu[0] + mu[2], mu[1] + mu[3]
    v12 = v[12]
    st, ct = np.sin(th), np.cos(th)
    out = np.zeros(5)

    def length(dp0, dp1, dt0, dt1, ang):
        """hl's parameter: dg = (1/2, 0, 1/2, 0); dpp = dpt for the trailer's L2 (ang = 1), else 0."""
        rot = a * dt0 + c * dt1
        return -(yd0 * (0.5 * ve - (dp0 * va + dp1 * vc) - rot * lp[2] - ang * rot * lp[3])
                 + v12 * (0.5 * me - (a * dp0 + c * dp1)))
    width = -(yd0 * (0.5 * vo) + v12 * (0.5 * mo))
    if (j & 1) == 0:
        out[0] = length(0.5 * ct, 0.5 * st, -0.5 * st, 0.5 * ct, 0.0)
        out[3] = width
    else:
        sa, ca = np.sin(th + ps), np.cos(th + ps)
        out[1] = length(-0.5 * ca, -0.5 * sa, 0.5 * sa, -0.5 * ca, 1.0)
        out[4] = width
        rot = a * st + c * -ct  # Mh: dg = 0, dp = -(ct, st), dpt = (st, -ct), dpp = 0
        out[2] = -(yd0 * (-(-ct * va + -st * vc) - rot * lp[2]) + v12 * (-(a * -ct + c * -st)))
    return out


def block_terms(P, it, lx, vblk):
    """Sum of the block shares in flat block order, stage 0 left out (x_0 is pinned: its v is zero)."""
    N, M = P.N, P.M
    u = orf.unpack(it, N, M)
    g = np.zeros(5)
    for k in range(1, N + 1):
        for j in range(2 * M):
            g = g + block_share(u["x"][k], j, u["w"][k, j], u["yd"][k, j, 0], lx[k, :4], vblk[k, j])
    return g


def dynamics_terms(P, it, lx, ly):
    """dt sum_k [ lx_k' (dJ_f/dtheta)' y_{k+1} + ly_{k+1}' df/dtheta ] -> (5,) (zeros for W1, W2)."""
    N = P.N
    u = orf.unpack(it, N, P.M)
    p = params_of(P)
    g = np.zeros(3)
    for k in range(N):
        df, dJ = mvr.model_derivatives(u["x"][k], p)
        g = g + np.array([lx[k] @ (dJ[i].T @ u["yc"][k + 1]) + ly[k + 1] @ df[i] for i in range(3)])
    return np.concatenate([P.dt * g, np.zeros(2)])


def _with_geometry(out, P, it, lx, ly, vblk):
    out["geom_block"] = block_terms(P, it, lx, vblk)
    out["geom_dyn"] = dynamics_terms(P, it, lx, ly)
    out["geom"] = out["geom_block"] + out["geom_dyn"]
    return out


# ---- routes -------------------------------------------------------------------------------------------------------
def dense_geometry_vjp(P, it, gX, gU, xref, uref, sparse=False, refined=False, parts=False):
    ln, lam, n, maps = osr.dense_lam(P, it, gX, gU, sparse, refined)
    out = osr._from_lam(P, it, ln, lam, n, maps, xref, uref)
    lx, lu, ly, vblk = osr.split_lam(P, lam, n, maps)
    _with_geometry(out, P, it, lx, ly, vblk)
    if parts:
        out["parts"] = (lx, lu, ly, vblk)
    return out


def _zeros(P):
    out = osr._zeros(P)
    out.update(geom=np.zeros(5), geom_block=np.zeros(5), geom_dyn=np.zeros(5))
    return out


def model_geometry_vjp(P, it, gX, gU, xref, uref, steps=STEPS):
    """The geometry kernel's route (module docstring)."""
    out = _zeros(P)
    got = osr._carried(P, it, gX, gU, steps)
    if got is None:
        return out
    ln, lx, lu, x0, ly, vblk, _ = got
    osr._finish(P, it, ln, out, lx, lu, x0, vblk, xref, uref)
    _with_geometry(out, P, it, lx, ly, vblk)
    out["ok"] = bool(out["ok"] and np.all(np.isfinite(out["geom"])))
    return out


def recomputed_geometry_vjp(P, it, gX, gU, xref, uref, steps=STEPS):
    """The carried route's lam_x and lam_y, but v = -K_b^-1 C lx_pose recomputed from the final pose adjoint."""
    out = _zeros(P)
    got = osr._carried(P, it, gX, gU, steps)
    if got is None:
        return out
    ln, lx, lu, x0, ly, _, facs = got
    vblk = np.zeros((P.N + 1, 2 * P.M, 16))
    for (k, j), (Kb, C, fac) in facs.items():
        vblk[k, j] = orf.solve_block(fac, -(C @ lx[k, :4]))
    osr._finish(P, it, ln, out, lx, lu, x0, vblk, xref, uref)
    return _with_geometry(out, P, it, lx, ly, vblk)


def scales(ref):
    """obca_scene_reference.scales, and the geometry group with the obs group's rule: it shares its unit with the
    position entries of g_x0."""
    mx = osr.scales(ref)
    mx["geom"] = max(float(np.max(np.abs(ref["geom"]))), float(np.max(np.abs(ref["x0"]))))
    return mx


def group_err(a, b):
    return orf.group_err(a, b, KEYS)


# ---- differences --------------------------------------------------------------------------------------------------
def oracle_fd_geometry(P, x0, xr, ur, gX, gU, h=1e-4):
    """Central differences of L = sum(gX * X) + sum(gU * U) over the oracle's solve in (L1, L2, Mh, W1, W2) and, for
    the record, in d_min.  P is restored.  Returns (geom (5,), dmin)."""
    N, M = P.N, P.M

    def loss():
        z, st, _, _ = co.obca_solve_batch(P, x0[None], xref=xr[None], uref=ur[None])
        assert st[0] == 0, st
        X, U, _, _ = co.obca_split(z, N, M)
        return float((X[0] * gX).sum() + (U[0] * gU).sum())

    def diff(name):
        keep = getattr(P, name)
        setattr(P, name, keep + h)
        up = loss()
        setattr(P, name, keep - h)
        dn = loss()
        setattr(P, name, keep)
        return (up - dn) / (2.0 * h)
    return np.array([diff(n) for n in THETA]), diff("dmin")


def residual_fd_geometry(P, it, lx, ly, vblk, h=1e-6):
    """The central difference in theta of Phi = lam' F(theta) at the fixed iterate, negated.  Of F only the terms that
    can depend on theta are formed: per stage k < N the -dt J_f(x_k)' y_{k+1} part of the x-rows and the dynamics row
    -dt f(x_k, u_k); per block the pose rows' J_x' y_d, the dual rows' J_w' y_d and the block rows d themselves, from
    tto_obca_block_lin at the perturbed parameters.  P is restored.  -> (5,)."""
    N, M = P.N, P.M
    u = orf.unpack(it, N, M)
    keep = get_theta(P)

    def phi():
        p = params_of(P)
        lin = orf._block_lin(P)
        s = 0.0
        for k in range(N):
            s += lx[k] @ (-P.dt * to.jac_f(u["x"][k], p).T @ u["yc"][k + 1])
            s += ly[k + 1] @ (-P.dt * to.f(u["x"][k], u["u"][k], p))
        L = co._obca_lib()
        for k in range(N + 1):
            for j in range(2 * M):
                d = _block_rows(L, P, u["x"][k], j, u["w"][k, j])
                Jx, Jw = lin(u["x"][k], j, u["w"][k, j], u["yd"][k, j])[:2]
                yd, v = u["yd"][k, j], vblk[k, j]
                s += lx[k, :4] @ (Jx.T @ yd) + v[:8] @ (Jw.T @ yd) + v[12:] @ d
        return s
    out = np.zeros(5)
    for i in range(5):
        t = keep.copy()
        t[i] += h
        set_theta(P, t)
        up = phi()
        t[i] -= 2.0 * h
        set_theta(P, t)
        dn = phi()
        out[i] = -(up - dn) / (2.0 * h)
    set_theta(P, keep)
    return out


def _block_rows(L, P, xk, j, wv):
    """The four row values d(pose, w) of a block (tto_obca_block_lin's first output)."""
    import ctypes as C
    dp = C.POINTER(C.c_double)
    p = lambda a: a.ctypes.data_as(dp)  # noqa: E731
    xk, wv = (np.ascontiguousarray(a, dtype=np.float64) for a in (xk, wv))
    y = np.zeros(4)
    out = [np.zeros(n) for n in (4, 16, 32, 16, 32, 16)]
    L.tto_obca_block_lin(C.byref(P), p(xk), j, p(wv), p(y), *[p(o) for o in out])
    return out[0]
