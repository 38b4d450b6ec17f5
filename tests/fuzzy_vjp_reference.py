"""Test helper (numpy only): the fuzzy weight rule as data (tt_fuzzy_rule, include/ttmpc.h), its adjoint, and the
backward sweep of tests/loop_vjp_reference.py extended by it.

One step of a rule loop:  w_t = rule(x_meas_t, xref_t[0]; theta);  X_t, U_t = solve(x_meas_t, xref_t, uref_t, w_t); an
instance whose solve fails is re-solved once with unit weights (mpc_control_fuzzy.py:145-159), and then w_t = 1 does not
depend on anything.  The solve adjoint's g_w therefore flows through the rule into dL/dx_meas_t[3] and dL/dtheta, except
where the retry was taken.

* ``rule_weights`` / ``rule_vjp``: the rule and its adjoint table, vectorised over leading axes.
* ``rule_kink_distance``: how far a point is from every kink and switch of the rule.
* ``sweep``: lr.sweep with the rule adjoint between the solve adjoint and the state accumulation.
* ``fuzzy_case`` and the oracle helpers: the issue's loop (``to.closed_loop(policy="fuzzy", fuzzy=True)`` with the rule
  patched into ``oracle.ttmpc_oracle.fuzzy_weights``), its tape, its central differences, forced first-attempt failures.
"""
from __future__ import annotations

import contextlib

import numpy as np

import loop_vjp_reference as lr
from oracle import ttmpc_oracle as to

P, DIST = lr.P, lr.DIST
DEFAULT_THETA = (0.35, 2.0, 1.2, 1.5, 1.1, 1.1, 1.2)   # psi_full | gains hitch, steer, rate | reversing factors
SETTINGS = (1.0, 3.5, -0.1)                            # w_min, w_max, v_rev
THETA = (0.9, 2.6, 1.2, 1.5, 1.1, 1.1, 1.2)            # the loop case's rule
GROUPS = ("x_init", "w", "noise", "plan_x", "plan_u", "theta")


# ---- the rule ---------------------------------------------------------------------------------------------------
def _terms(theta, psi, v, ref_v, settings):
    theta = np.asarray(theta, dtype=np.float64)
    psi, v, ref_v = (np.asarray(t, dtype=np.float64) for t in np.broadcast_arrays(psi, v, ref_v))
    w_min, w_max, v_rev = settings
    s = np.abs(psi) / theta[0]
    h = np.minimum(s, 1.0)
    rev = (ref_v < v_rev) | (v < v_rev)
    f = np.where(rev[..., None], theta[4:7], 1.0)          # channels: hitch, steer, rate
    lin = 1.0 + theta[1:4] * h[..., None]
    raw = lin * f
    m = np.maximum(1.0, raw)
    w = np.minimum(np.maximum(m, w_min), w_max)
    return dict(psi=psi, s=s, h=h, rev=rev, f=f, lin=lin, raw=raw, m=m, w=w,
                passes=(raw > 1.0) & (w_min < m) & (m < w_max))


def rule_weights(theta, psi, v, ref_v, settings=SETTINGS):
    """(..., 8) = (1, 1, w_steer, w_hitch, w_steer, 1, 1, w_rate)."""
    t = _terms(theta, psi, v, ref_v, settings)
    out = np.ones(t["psi"].shape + (8,))
    out[..., 2] = out[..., 4] = t["w"][..., 1]
    out[..., 3] = t["w"][..., 0]
    out[..., 7] = t["w"][..., 2]
    return out


def rule_vjp(theta, psi, v, ref_v, g_w, settings=SETTINGS):
    """For g_w (..., 8): (g_psi (...), g_theta (..., 7)); v and ref_v only switch, their gradient is zero."""
    theta = np.asarray(theta, dtype=np.float64)
    t = _terms(theta, psi, v, ref_v, settings)
    g_w = np.asarray(g_w, dtype=np.float64)
    G = np.stack([g_w[..., 3], g_w[..., 2] + g_w[..., 4], g_w[..., 7]], axis=-1)
    Gp = np.where(t["passes"], G, 0.0)
    inside = t["s"] < 1.0
    acc = np.zeros(t["psi"].shape)
    for c in range(3):
        acc = acc + Gp[..., c] * theta[1 + c] * t["f"][..., c]
    g_psi = np.where(inside, acc * lr.sign0(t["psi"]) / theta[0], 0.0)
    g_th = np.zeros(t["psi"].shape + (7,))
    g_th[..., 0] = np.where(inside, -(acc * np.abs(t["psi"]) / (theta[0] * theta[0])), 0.0)
    g_th[..., 1:4] = Gp * t["h"][..., None] * t["f"]
    g_th[..., 4:7] = np.where(t["rev"][..., None], Gp * t["lin"], 0.0)
    return g_psi, g_th


def rule_kink_distance(theta, psi, v, ref_v, settings=SETTINGS):
    """The smallest distance of each point to a kink or switch of the rule: |psi| at 0 and at psi_full, v and ref_v at
    v_rev, each channel's raw at 1 and its max(1, raw) at the clip bounds."""
    t = _terms(theta, psi, v, ref_v, settings)
    w_min, w_max, v_rev = settings
    d = np.minimum(np.abs(t["psi"]), np.abs(np.abs(t["psi"]) - np.asarray(theta)[0]))
    d = np.minimum(d, np.minimum(np.abs(np.asarray(v) - v_rev), np.abs(np.asarray(ref_v) - v_rev)))
    for arr in (np.abs(t["raw"] - 1.0), np.abs(t["m"] - w_max), np.where(t["m"] > w_min, np.abs(t["m"] - w_min), np.inf)):
        d = np.minimum(d, arr.min(axis=-1))
    return d


# ---- the sweep --------------------------------------------------------------------------------------------------
def sweep(solve_vjp, policy, ks, Np, S, status, active, count, GS, GU, p, dist=None, in_plant=False, theta=None,
          x_meas=None, ref_v=None, retried=None, settings=SETTINGS):
    """lr.sweep for a rule loop: x_meas (K,B,6), ref_v (K,B) = xref_t[0][5], retried (K,B).  After the solve adjoint of
    step t, g["w"] goes through ``rule_vjp`` (nothing where retried): g_x0[3] += g_psi before the state accumulation
    (so the measurement-noise gradient carries it too), theta (B,7) += g_theta.  out["w"] is sum_t dL/dW_t.  With
    theta None this is lr.sweep plus a zero theta group."""
    K, B = status.shape
    a, abar = np.array(GS[K], dtype=np.float64), np.zeros((B, 2))
    out = {"w": np.zeros((B, 8)), "noise": np.zeros((K, B, 6)), "plan_x": np.zeros((B, Np + 1, 6)),
           "plan_u": np.zeros((B, Np, 2)), "theta": np.zeros((B, 7)), "rule_terms": np.zeros((K, B, 7))}
    for t in range(K - 1, -1, -1):
        a, abar, g_u0, gn = lr.policy_plant_vjp(policy, S[t], status[t], None if t == 0 else active[t - 1], active[t],
                                                count[t], GU[t], a, abar, p, dist, in_plant)
        g = solve_vjp(t, g_u0)
        gx0 = np.array(g["x0"], dtype=np.float64)
        if theta is not None:
            g_psi, g_th = rule_vjp(theta, x_meas[t][:, 3], x_meas[t][:, 5], ref_v[t], g["w"], settings)
            live = np.asarray(retried[t]) == 0
            gx0[:, 3] = np.where(live, gx0[:, 3] + g_psi, gx0[:, 3])
            out["rule_terms"][t] = np.where(live[:, None], g_th, 0.0)
            out["theta"] += out["rule_terms"][t]
        a = (a + gx0) + GS[t]
        out["w"] += g["w"]
        out["noise"][t] = gn if in_plant else gx0
        lr.window_vjp(g["xref"], g["uref"], ks[t], Np, out["plan_x"], out["plan_u"])
    out["x_init"] = a
    return out


def solve_vjp_from_tape(nlp, fn, X, U, dual, status, ks, plan_x, plan_u, W):
    """lr.solve_vjp_from_tape with each step's own weights W (K,B,8)."""
    N = nlp.N

    def cb(t, g_u0):
        B = g_u0.shape[0]
        Xr, Ur = to.reference_window(plan_x, plan_u, ks[t], N)
        out = {"x0": np.zeros((B, 6)), "xref": np.zeros((B, N + 1, 6)), "uref": np.zeros((B, N, 2)), "w": np.zeros((B, 8))}
        for b in range(B):
            if status[t, b] > 1:
                continue
            gU = np.zeros((N, 2))
            gU[0] = g_u0[b]
            r = fn(nlp, nlp.pack(X[t, b], U[t, b]), dual[t, b], Xr.T, Ur.T, np.zeros((N + 1, 6)), gU, W[t, b, :6],
                   W[t, b, 6:])
            for key in out:
                out[key][b] = r[key]
        return out
    return cb


def window_ref_v(plan_x, ks, Np, B):
    """ref_v (K,B) of a shared plan (6,Np+1): the speed of the window's first row."""
    return np.array([[plan_x[5, min(k, Np)]] * B for k in ks])


def chain(c, fn, tp, in_plant=True, policy="fuzzy", theta=None):
    """The numpy sweep on a tape dict (S, status, active, consec|count, X, U, dual, W, retried) of the case."""
    theta = c["theta"] if theta is None else theta
    K, B = tp["status"].shape
    cb = solve_vjp_from_tape(c["nlp"], fn, tp["X"], tp["U"], tp["dual"], tp["status"], c["ks"], c["plan_x"], c["plan_u"],
                             tp["W"])
    x_meas = tp["S"][:K] if in_plant else tp["S"][:K] + c["noise"]
    count = tp["count"] if "count" in tp else tp["consec"]
    return sweep(cb, policy, c["ks"], c["Np"], tp["S"], tp["status"], tp["active"], count, c["GS"], c["GU"], P, DIST,
                 in_plant, theta, x_meas, window_ref_v(c["plan_x"], c["ks"], c["Np"], B), tp["retried"])


# ---- the issue's loop on the CPU oracle ---------------------------------------------------------------------------
def fuzzy_case(golden_ref):
    """lr.loop_case with the hitch angles of x_init shifted by (0, -0.25, +0.2) and the rule THETA; its noise is the
    plant's process noise (the fuzzy driver measures the exact state)."""
    c = dict(lr.loop_case(golden_ref))
    x = c["x_init"].copy()
    x[:, 3] += (0.0, -0.25, 0.2)
    c["x_init"], c["theta"] = x, THETA
    return c


@contextlib.contextmanager
def patched_rule(theta, settings=SETTINGS):
    """``to.fuzzy_weights`` replaced by the rule at theta (``to.closed_loop`` looks it up at call time)."""
    def fuzzy_weights(current_state, reference_states):
        rs = np.asarray(reference_states)
        w = rule_weights(theta, float(current_state[3]), float(current_state[5]),
                         float(rs[5, 0]) if rs.size > 0 else 0.0, settings)
        return w[:6], w[6:]
    old = to.fuzzy_weights
    to.fuzzy_weights = fuzzy_weights
    try:
        yield
    finally:
        to.fuzzy_weights = old


def oracle_solver(nlp, tape=None, force=None):
    """solve(x, Xr, Ur, w) for ``to.closed_loop(fuzzy=True)`` on the C oracle.  force {t: bool mask over the loop's
    instances}: those first attempts of step t report status 2 whatever the solve did, which sends them to the
    unit-weight retry; the forcing looks at the step and the instance only, never at the numbers.  tape: a list that
    gets one dict per step with the accepted x_meas, X, U, status, W and retried."""
    import sens_reference as sr
    from oracle import c_oracle as co
    from ttmpc import layout
    Pp = sr.oracle_problem(nlp)
    state = {"t": 0, "bad": None}

    def solve(x, Xr, Ur, w):
        z, st, _, _ = co.solve_batch(Pp, x, Xr, Ur, wq=w[:, :6], wr=w[:, 6:])
        X, Uo = layout.unpack(z, nlp.N)
        st = np.array(st)
        if state["bad"] is not None:                       # the retry of the step's failed instances
            bad, state["bad"] = state["bad"], None
            if tape is not None:
                r = tape[-1]
                r["X"][bad], r["U"][bad], r["status"][bad], r["W"][bad], r["retried"][bad] = X, Uo, st, 1.0, 1
            return X, Uo, st
        t, state["t"] = state["t"], state["t"] + 1
        if force is not None and t in force:
            st[np.asarray(force[t], dtype=bool)] = 2
        if np.any(st > 1):
            state["bad"] = np.where(st > 1)[0]
        if tape is not None:
            tape.append(dict(x_meas=np.array(x), X=X.copy(), U=Uo.copy(), status=st.copy(), W=np.array(w),
                             retried=np.zeros(len(st), dtype=np.int32)))
        return X, Uo, st
    return solve


def oracle_loop(c, x_init, noise, theta=None, plan_x=None, plan_u=None, tape=None, force=None):
    """The case's loop (policy "fuzzy", fuzzy weights from the rule, DIST, in-plant noise) for any number of instances.
    -> (S (K+1,B,6), Ua (K,B,2), status (K,B))."""
    with patched_rule(c["theta"] if theta is None else theta):
        return to.closed_loop(oracle_solver(c["nlp"], tape, force), x_init,
                              c["plan_x"] if plan_x is None else plan_x, c["plan_u"] if plan_u is None else plan_u,
                              c["N"], c["T"], P, DIST, None, policy="fuzzy", fuzzy=True, plant_noise=noise)[:3]


def oracle_tape(c, force=None):
    """The oracle's own run with each step's accepted solution, weights and interior multipliers: what ``chain`` needs."""
    from test_vjp_reference import _interior_dual
    nlp, N, B, K = c["nlp"], c["N"], c["B"], c["K"]
    rec = []
    S, Ua, st = oracle_loop(c, c["x_init"], c["noise"], tape=rec, force=force)
    X, U, W = (np.array([r[k] for r in rec]) for k in ("X", "U", "W"))
    retried = np.array([r["retried"] for r in rec])
    dual = np.zeros((K, B, N + 1, 22))
    for t in range(K):
        Xr, Ur = to.reference_window(c["plan_x"], c["plan_u"], c["ks"][t], N)
        for b in range(B):
            z = nlp.pack(X[t, b], U[t, b])
            y = nlp.kkt_residual(z, rec[t]["x_meas"][b], Xr, Ur, W[t, b, :6], W[t, b, 6:])["y"].reshape(N + 1, 6)
            dual[t, b] = _interior_dual(nlp, z, y)
    return dict(S=S, Ua=Ua, status=st, active=np.ones((K, B), dtype=np.int32), count=np.zeros((K, B), dtype=np.int32),
                X=X, U=U, dual=dual, W=W, retried=retried, x_meas=np.array([r["x_meas"] for r in rec]))


def oracle_fd(c, h=1e-4, force=None, plan_entries=None):
    """Central differences of L = sum(GS * S) + sum(GU * Ua) over ``oracle_loop``.  x_init and noise: one loop whose
    instances are the perturbed copies of the instance each entry belongs to (a forced failure follows its owner).
    theta: two loops per entry, differentiated per instance (L is a sum over the instances).  The shared plan: two
    loops per entry, summed over B.  force: {t: instance b}.
    -> (dict(x_init (B,6), noise (K,B,6), theta (B,7), plan_x {(r, i): v}, plan_u {(r, i): v}), every final status 0)."""
    B, K, GS, GU = c["B"], c["K"], c["GS"], c["GU"]
    force = force or {}
    owners, xs, ns = [], [], []
    for name, arr in (("x_init", c["x_init"]), ("noise", c["noise"])):
        for idx in np.ndindex(arr.shape):
            b = idx[0] if name == "x_init" else idx[1]
            for sgn in (1.0, -1.0):
                x, n = c["x_init"][b].copy(), c["noise"][:, b].copy()
                if name == "x_init":
                    x[idx[1]] += sgn * h
                else:
                    n[idx[0], idx[2]] += sgn * h
                owners.append((name, idx, b))
                xs.append(x), ns.append(n)
    own_b = np.array([o[2] for o in owners])
    S, Ua, st = oracle_loop(c, np.array(xs), np.array(ns).transpose(1, 0, 2),
                            force={t: own_b == b for t, b in force.items()})
    ok = bool(np.all(st == 0))
    out = {"x_init": np.zeros((B, 6)), "noise": np.zeros((K, B, 6)), "theta": np.zeros((B, 7)), "plan_x": {}, "plan_u": {}}
    for m in range(0, len(owners), 2):
        name, idx, b = owners[m]
        L = [float(np.sum(GS[:, b] * S[:, m + d]) + np.sum(GU[:, b] * Ua[:, m + d])) for d in (0, 1)]
        out[name][idx] = (L[0] - L[1]) / (2.0 * h)
    small = {t: np.arange(B) == b for t, b in force.items()}
    for i in range(7):
        L = []
        for sgn in (1.0, -1.0):
            th = np.array(c["theta"], dtype=np.float64)
            th[i] += sgn * h
            S, Ua, st = oracle_loop(c, c["x_init"], c["noise"], theta=th, force=small)
            ok = ok and bool(np.all(st == 0))
            L.append(np.sum(GS * S, axis=(0, 2)) + np.sum(GU * Ua, axis=(0, 2)))
        out["theta"][:, i] = (L[0] - L[1]) / (2.0 * h)
    Np = c["Np"]
    if plan_entries is None:
        plan_entries = [("plan_x", r, i) for r in range(Np + 1) for i in range(6)] + \
                       [("plan_u", r, i) for r in range(Np) for i in range(2)]
    for name, r, i in plan_entries:
        L = []
        for sgn in (1.0, -1.0):
            px, pu = c["plan_x"].copy(), c["plan_u"].copy()
            (px if name == "plan_x" else pu)[i, r] += sgn * h
            S, Ua, st = oracle_loop(c, c["x_init"], c["noise"], plan_x=px, plan_u=pu, force=small)
            ok = ok and bool(np.all(st == 0))
            L.append(float(np.sum(GS * S) + np.sum(GU * Ua)))
        out[name][(r, i)] = (L[0] - L[1]) / (2.0 * h)
    return out, ok


def fd_errors(g, fd):
    """Largest absolute differences, per group, between a sweep's gradients (plan per instance: summed here; or already
    (1, ., .)) and ``oracle_fd``'s."""
    gpx, gpu_ = np.asarray(g["plan_x"]).sum(axis=0), np.asarray(g["plan_u"]).sum(axis=0)
    return {"x_init": float(np.max(np.abs(g["x_init"] - fd["x_init"]))),
            "noise": float(np.max(np.abs(g["noise"] - fd["noise"]))),
            "plan_x": max(abs(gpx[r, i] - v) for (r, i), v in fd["plan_x"].items()),
            "plan_u": max(abs(gpu_[r, i] - v) for (r, i), v in fd["plan_u"].items()),
            "theta": float(np.max(np.abs(g["theta"] - fd["theta"])))}


def group_err(a, b):
    return {g: float(np.max(np.abs(np.asarray(a[g]) - np.asarray(b[g])))) for g in GROUPS}


def group_max(a):
    return {g: float(np.max(np.abs(np.asarray(a[g])))) for g in GROUPS}
