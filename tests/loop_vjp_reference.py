"""Test helper (numpy only): reference algebra for the adjoint of the closed loop (ClosedLoop.run_tape / backward).

One closed-loop step t (ttmpc.simulation.ClosedLoop.step, oracle.ttmpc_oracle.closed_loop):

    xref_t, uref_t = window(plan, k_t);  x_meas_t = S_t + n_t;  X_t, U_t = solve(x_meas_t, xref_t, uref_t, w)
    u_t = policy(U_t[0], status_t, u_last, consec);  S_{t+1} = plant(S_t, u_t)      (stopped: S_{t+1} = S_t)

For a scalar loss L(S, Ua) with GS = dL/dS (K+1,B,6), GU = dL/dUa (K,B,2) the sweep carries a = dL/dS_{t+1} and
abar = the adjoint of u_last.  The pieces here:

* ``plant_jacobians`` / ``plant_vjp``: J_q, J_u of ``to.plant_update`` and the products J_q' a, J_u' a in the order
  policy_plant_vjp_kernel (tt_sim_vjp.hip) forms them.  Kinks: d|x|/dx = sign(x) (0 at 0), d min(s, 0.3)/ds = [s < 0.3].
* ``policy_plant_vjp``: the kernel's branch table on logged status / active / count arrays.
* ``window_vjp``: the window's scatter into a per-instance plan gradient with the forward's end padding.
* ``policy_plant``: a numpy restatement of policy_plant_kernel (tt_sim.hip), for brute-force differentiation.
* ``sweep``: the whole backward pass with the solve adjoint as a callback (dense_vjp, riccati_vjp or a stand-in).
"""
from __future__ import annotations

import numpy as np

from oracle import ttmpc_oracle as to

POLICIES = {"track": 0, "nmpc": 1, "fuzzy": 2}
GROUPS = ("x_init", "w", "noise", "plan_x", "plan_u")


def sign0(x):
    return np.sign(x)


# ---- plant ------------------------------------------------------------------------------------------------------
def _plant_terms(q, p, dist):
    q = np.asarray(q, dtype=np.float64)
    th, ps, ph, v = q[..., 2], q[..., 3], q[..., 4], q[..., 5]
    L1, L2, Mh = p["L1"], p["L2"], p["M"]
    en = dist is not None
    d = dist or {}
    fc, sc = (d.get("friction_coeff", 1.0), d.get("slippage_coeff", 1.0)) if en else (1.0, 1.0)
    sam, gain = d.get("slip_angle_max", 0.0), d.get("lateral_slip_gain", 0.0)
    cth, sth, cps, sps, tph = np.cos(th), np.sin(th), np.cos(ps), np.sin(ps), np.tan(ph)
    sec2 = 1.0 + tph * tph
    hk = 1 + Mh / L2 * cps
    t = dict(fc=fc, sc=sc, cth=cth, sth=sth, v=v, ph=ph, gain=gain if en else 0.0, en=en)
    t["f2"] = v * tph / L1
    t["f3"] = -v * tph / L1 * hk - v * sps / L2
    t["f2_ph"], t["f2_v"] = v * sec2 / L1, tph / L1
    t["f3_ps"] = v * tph / L1 * (Mh / L2 * sps) - v * cps / L2
    t["f3_ph"] = -v * sec2 / L1 * hk
    t["f3_v"] = -tph / L1 * hk - sps / L2
    one, zero = np.ones_like(v), np.zeros_like(v)
    if en:
        s = np.abs(ph) * np.abs(v) * sam
        live = s < 0.3
        t["slip"] = 1.0 - np.minimum(s, 0.3)
        t["slip_ph"] = np.where(live, -(sign0(ph) * np.abs(v) * sam), 0.0)
        t["slip_v"] = np.where(live, -(np.abs(ph) * sign0(v) * sam), 0.0)
        t["cl"], t["sl"] = np.cos(th + np.pi / 2), np.sin(th + np.pi / 2)
    else:
        t["slip"], t["slip_ph"], t["slip_v"], t["cl"], t["sl"] = one, zero, zero, zero, zero
    return t


def plant_vjp(q, a, p, dist=None):
    """(J_q' a (...,6), J_u' a (...,2)) of S+ = to.plant_update(q, u, p, dist) at q, in the kernel's order of operations."""
    t = _plant_terms(q, p, dist)
    a = np.asarray(a, dtype=np.float64)
    dt = p["dt"]
    cu = np.stack([a[..., 5] * dt * t["fc"], a[..., 4] * dt * t["sc"]], axis=-1)
    v, ph, slip = t["v"], t["ph"], t["slip"]
    g_th = a[..., 0] * (-v * t["sth"]) + a[..., 1] * (v * t["cth"])
    g_ps = a[..., 3] * (slip * t["f3_ps"])
    g_ph = a[..., 2] * (slip * t["f2_ph"] + t["f2"] * t["slip_ph"]) + a[..., 3] * (slip * t["f3_ph"] + t["f3"] * t["slip_ph"])
    g_v = (a[..., 0] * t["cth"] + a[..., 1] * t["sth"] + a[..., 2] * (slip * t["f2_v"] + t["f2"] * t["slip_v"])
           + a[..., 3] * (slip * t["f3_v"] + t["f3"] * t["slip_v"]))
    if t["en"]:
        mag = t["gain"] * np.abs(v) * np.abs(ph)
        along = a[..., 0] * t["cl"] + a[..., 1] * t["sl"]
        g_th = g_th + mag * (a[..., 1] * t["cl"] - a[..., 0] * t["sl"])
        g_ph = g_ph + t["gain"] * np.abs(v) * sign0(ph) * along
        g_v = g_v + t["gain"] * sign0(v) * np.abs(ph) * along
    out = np.array(a, dtype=np.float64)
    out[..., 2] = a[..., 2] + g_th * dt
    out[..., 3] = a[..., 3] + g_ps * dt
    out[..., 4] = a[..., 4] + g_ph * dt
    out[..., 5] = a[..., 5] + g_v * dt
    return out, cu


def plant_jacobians(q, p, dist=None):
    """J_q (6,6) = dS+/dq and J_u (6,2) = dS+/du of one state, from ``plant_vjp`` on the unit vectors."""
    q = np.asarray(q, dtype=np.float64).reshape(6)
    Jq, Ju = np.empty((6, 6)), np.empty((6, 2))
    for i in range(6):
        Jq[i], Ju[i] = plant_vjp(q, np.eye(6)[i], p, dist)
    return Jq, Ju


def kink_distance(q, dist=None):
    """How far each state is from a kink of the disturbed plant: min(|phi|, |v|) and |phi v slip_angle_max - 0.3|."""
    q = np.asarray(q, dtype=np.float64)
    sam = (dist or {}).get("slip_angle_max", 0.0)
    return np.minimum(np.abs(q[..., 4]), np.abs(q[..., 5])), np.abs(np.abs(q[..., 4] * q[..., 5]) * sam - 0.3)


# ---- policy + plant ---------------------------------------------------------------------------------------------
def policy_plant(policy, x, u0, status, u_last, consec, active, p, dist=None, plant_noise=None):
    """policy_plant_kernel (tt_sim.hip) on copies: -> (x_next, u_applied, u_last, consec, active)."""
    x, u_last = np.array(x, dtype=np.float64), np.array(u_last, dtype=np.float64)
    consec, active = np.array(consec), np.array(active, dtype=bool)
    B = x.shape[0]
    ua = np.zeros((B, 2))
    for b in range(B):
        if not active[b]:
            continue
        if status[b] <= 1:
            ua[b] = u0[b]
            u_last[b] = ua[b]
            consec[b] = 0
        else:
            consec[b] += 1
            if policy == "nmpc":
                u_last[b] = 0.0
                if consec[b] > 20:
                    active[b] = False
            elif policy == "fuzzy":
                ua[b] = u_last[b]
                if consec[b] > 15:
                    ua[b] = 0.0
                if consec[b] > 30:
                    active[b] = False
            else:
                ua[b] = u0[b]
        if not active[b]:
            ua[b] = 0.0
    xn = to.plant_update(x, ua, p, dist, plant_noise)
    return np.where(active[:, None], xn, x), ua, u_last, consec, active


def policy_plant_vjp(policy, S_t, status, act_before, act_after, count, GU_t, a, abar, p, dist=None, in_plant=False):
    """The branch table of tt_policy_plant_vjp_device.  -> (a (B,6), abar (B,2), g_u0 (B,2), g_noise (B,6) or None)."""
    B = S_t.shape[0]
    a, abar = np.array(a, dtype=np.float64), np.array(abar, dtype=np.float64)
    before = np.ones(B, dtype=bool) if act_before is None else np.asarray(act_before) != 0
    moved = before & (np.asarray(act_after) != 0)
    aq, c = plant_vjp(S_t, a, p, dist)
    if GU_t is not None:
        c = c + GU_t
    g_u0 = np.zeros((B, 2))
    g_noise = np.where(moved[:, None], p["dt"] * a, 0.0) if in_plant else None
    for b in range(B):
        if not moved[b]:
            if before[b] and policy == "nmpc":
                abar[b] = 0.0
            continue
        if status[b] <= 1:
            g_u0[b] = c[b] + abar[b]
            abar[b] = 0.0
        elif policy == "nmpc":
            abar[b] = 0.0
        elif policy == "fuzzy":
            if count[b] <= 15:
                abar[b] = abar[b] + c[b]
        else:
            g_u0[b] = c[b]
        a[b] = aq[b]
    return a, abar, g_u0, g_noise


# ---- window -----------------------------------------------------------------------------------------------------
def window_vjp(g_xref, g_uref, k, Np, acc_x, acc_u):
    """acc_x (B,Np+1,6) += scatter(g_xref (B,N+1,6)), acc_u (B,Np,2) += scatter(g_uref (B,N,2)), in place: state row j
    to plan row min(k+j, Np), input row j to min(k+j, Np-1) while k < Np.  A padded row gets the ascending-j sum."""
    N = g_uref.shape[1]
    for r in range(min(k, Np), min(k + N, Np) + 1):
        rows = [j for j in range(N + 1) if min(k + j, Np) == r]
        s = g_xref[:, rows[0]].copy() if len(rows) == 1 else None
        if s is None:
            s = np.zeros_like(g_xref[:, 0])
            for j in rows:
                s = s + g_xref[:, j]
        acc_x[:, r] += s
    if k < Np:
        for r in range(k, min(k + N - 1, Np - 1) + 1):
            rows = [j for j in range(N) if min(k + j, Np - 1) == r]
            s = g_uref[:, rows[0]].copy() if len(rows) == 1 else None
            if s is None:
                s = np.zeros_like(g_uref[:, 0])
                for j in rows:
                    s = s + g_uref[:, j]
            acc_u[:, r] += s
    return acc_x, acc_u


# ---- the sweep --------------------------------------------------------------------------------------------------
def sweep(solve_vjp, policy, ks, Np, S, status, active, count, GS, GU, p, dist=None, in_plant=False, rule_vjp=None,
          plant_model_vjp=None):
    """The backward pass over logged S (K+1,B,6), status / active / count (K,B) (active, count: after the step).
    solve_vjp(t, g_u0 (B,2)) -> dict(x0 (B,6), xref (B,N+1,6), uref (B,N,2), w (B,8)): the solve adjoint of step t for
    the upstream gradient dL/dU_t[0] = g_u0 (zeros for an instance whose status is above 1).
    Returns dict(x_init (B,6), w (B,8), noise (K,B,6), plan_x (B,Np+1,6), plan_u (B,Np,2)): the noise gradient is the
    measurement noise's (g_x0 of each step), or with in_plant the plant noise's.

    Three optional terms ride along, each through a callable so that this module needs neither of the two that own them:
    * rule_vjp(t, g_w (B,8)) -> (g_psi (B,), g_theta (B,7), live (B,) bool), a rule loop's weights w_t = rule(x_meas_t,
      xref_t[0]): where live, g_x0[3] += g_psi before the state accumulation (so the measurement-noise gradient carries
      it too) and theta (B,7) += g_theta, kept per step in rule_terms (K,B,7).  w is then sum_t dL/dW_t.
    * plant_model_vjp(S_t, a, p, dist) -> a' dS_{t+1}/d(L1, L2, M) (B,3), with a = dL/dS_{t+1} before the J_q product:
      model_plant (B,3); stopped and inactive instances add nothing.
    * a solve adjoint that also returns model (B,3): model_solver (B,3) is their sum over the steps."""
    K, B = status.shape
    a, abar = np.array(GS[K], dtype=np.float64), np.zeros((B, 2))
    out = {"w": np.zeros((B, 8)), "noise": np.zeros((K, B, 6)), "plan_x": np.zeros((B, Np + 1, 6)),
           "plan_u": np.zeros((B, Np, 2))}
    if rule_vjp is not None:
        out.update(theta=np.zeros((B, 7)), rule_terms=np.zeros((K, B, 7)))
    if plant_model_vjp is not None:
        out.update(model_solver=np.zeros((B, 3)), model_plant=np.zeros((B, 3)))
    for t in range(K - 1, -1, -1):
        if plant_model_vjp is not None:
            before = np.ones(B, dtype=bool) if t == 0 else np.asarray(active[t - 1]) != 0
            moved = before & (np.asarray(active[t]) != 0)
            out["model_plant"] += np.where(moved[:, None], plant_model_vjp(S[t], a, p, dist), 0.0)
        a, abar, g_u0, gn = policy_plant_vjp(policy, S[t], status[t], None if t == 0 else active[t - 1], active[t],
                                             count[t], GU[t], a, abar, p, dist, in_plant)
        g = solve_vjp(t, g_u0)
        gx0 = np.array(g["x0"], dtype=np.float64)
        if rule_vjp is not None:
            g_psi, g_th, live = rule_vjp(t, g["w"])
            gx0[:, 3] = np.where(live, gx0[:, 3] + g_psi, gx0[:, 3])
            out["rule_terms"][t] = np.where(live[:, None], g_th, 0.0)
            out["theta"] += out["rule_terms"][t]
        a = (a + gx0) + GS[t]
        out["w"] += g["w"]
        out["noise"][t] = gn if in_plant else gx0
        window_vjp(g["xref"], g["uref"], ks[t], Np, out["plan_x"], out["plan_u"])
        if "model" in g:
            out["model_solver"] += g["model"]
    out["x_init"] = a
    return out


def solve_vjp_from_tape(nlp, fn, X, U, dual, status, ks, plan_x, plan_u, w=None, keys=("x0", "xref", "uref", "w")):
    """The callback for ``sweep`` from a taped run: fn = vjp_reference.dense_vjp or riccati_vjp on step t's (X, U, dual)
    (K,B,...) and the window of the shared plan (6,Np+1), (2,Np); failed solves give zeros, as the kernel does.
    w: the weights of the run (B,8), of each step (K,B,8), or None.  keys: what is taken from fn's result; the others
    stay zeros, and "model" (B,3) is one more (model_vjp_reference.chain)."""
    N = nlp.N

    def cb(t, g_u0):
        B = g_u0.shape[0]
        Xr, Ur = to.reference_window(plan_x, plan_u, ks[t], N)
        out = {"x0": np.zeros((B, 6)), "xref": np.zeros((B, N + 1, 6)), "uref": np.zeros((B, N, 2)), "w": np.zeros((B, 8))}
        if "model" in keys:
            out["model"] = np.zeros((B, 3))
        wt = w if w is None or w.ndim == 2 else w[t]
        for b in range(B):
            if status[t, b] > 1:
                continue
            gU = np.zeros((N, 2))
            gU[0] = g_u0[b]
            wq, wr = (None, None) if wt is None else (wt[b, :6], wt[b, 6:])
            r = fn(nlp, nlp.pack(X[t, b], U[t, b]), dual[t, b], Xr.T, Ur.T, np.zeros((N + 1, 6)), gU, wq, wr)
            for key in keys:
                out[key][b] = r[key]
        return out
    return cb


def chain(c, fn, tp, policy="track", in_plant=False, keys=("x0", "xref", "uref", "w"), **terms):
    """``sweep`` on a tape dict of the case (S, status, active, consec|count, X, U, dual[, W]: a GPU tape as numpy, or
    ``oracle_tape``'s) with fn per step, at the tape's per-step weights W if it has them, else at the case's."""
    cb = solve_vjp_from_tape(c["nlp"], fn, tp["X"], tp["U"], tp["dual"], tp["status"], c["ks"], c["plan_x"], c["plan_u"],
                             tp["W"] if "W" in tp else c["w"], keys)
    return sweep(cb, policy, c["ks"], c["Np"], tp["S"], tp["status"], tp["active"],
                 tp["count"] if "count" in tp else tp["consec"], c["GS"], c["GU"], P, DIST, in_plant, **terms)


def group_max(a, groups=GROUPS):
    return {g: float(np.max(np.abs(np.asarray(a[g])))) for g in groups}


# ---- the issue's inputs -------------------------------------------------------------------------------------------
P = {"M": 0.15, "L1": 7.05, "L2": 12.45, "W1": 3.05, "W2": 2.95, "dt": 0.05}
DIST = dict(to.DISTURBANCE_PARAMS, slip_angle_max=0.5)


def loop_case(golden_ref):
    """N = 6, B = 3, T_sim = 0.25 (K = 6, k = 0..5); the plan is columns 150..158 of the interpolated golden plan (Np = 8:
    end padding from k = 3); weights U(0.7, 1.4); measurement noise N(0, 0.002); GS, GU uniform in [-1, 1]."""
    N, B, T = 6, 3, 0.25
    S, U = to.do_interpolation(golden_ref["state_traj"], golden_ref["input_traj"], 0.1, 0.05)
    plan_x, plan_u = S[:, 150:159].copy(), U[:, 150:158].copy()
    rng = np.random.default_rng(5)
    x_init = plan_x[:, 0][None] + rng.normal(scale=[0.1, 0.1, 0.01, 0.01, 0.0, 0.0], size=(B, 6))
    ks = to.step_indices(T, P["dt"])
    K = len(ks)
    w = rng.uniform(0.7, 1.4, (B, 8))
    noise = rng.normal(scale=0.002, size=(K, B, 6))
    GS, GU = rng.uniform(-1.0, 1.0, (K + 1, B, 6)), rng.uniform(-1.0, 1.0, (K, B, 2))
    nlp = to.TrackingNLP(N, params=dict(P, horizon=N))
    return dict(N=N, B=B, T=T, K=K, ks=ks, Np=8, nlp=nlp, plan_x=plan_x, plan_u=plan_u, x_init=x_init, w=w, noise=noise,
                GS=GS, GU=GU)


def oracle_solver(nlp, w, tape=None):
    """solve(x, Xr, Ur) for ``to.closed_loop`` on the C oracle with per-instance weights w (B,8); every call appends
    dict(x_meas, X, U, status) to ``tape`` when one is given."""
    import sens_reference as sr
    from oracle import c_oracle as co
    from ttmpc import layout
    Pp = sr.oracle_problem(nlp)

    def solve(x, Xr, Ur):
        z, st, _, _ = co.solve_batch(Pp, x, Xr, Ur, wq=w[:, :6], wr=w[:, 6:])
        X, Uo = layout.unpack(z, nlp.N)
        if tape is not None:
            tape.append(dict(x_meas=np.array(x), X=X, U=Uo, status=np.array(st)))
        return X, Uo, st
    return solve


def oracle_loop(c, x_init, w, noise, plan_x=None, plan_u=None, in_plant=False, tape=None):
    """``to.closed_loop`` (policy "track", DIST) for any number of instances on the case's plan or another.
    -> (S (K+1,B,6), Ua (K,B,2), status (K,B))."""
    return to.closed_loop(oracle_solver(c["nlp"], w, tape), x_init, c["plan_x"] if plan_x is None else plan_x,
                          c["plan_u"] if plan_u is None else plan_u, c["N"], c["T"], P, DIST,
                          None if in_plant else noise, plant_noise=noise if in_plant else None)[:3]


def central_differences(c, run, groups, shared=None, h=1e-4, plan_entries=None):
    """Central differences of L = sum(GS * S) + sum(GU * Ua) over run(inputs, owners) -> (S, Ua, status): an oracle loop
    of the case on ``inputs``, a dict with every differentiated input of the case, some replaced; owners (n,): the
    instance of the case each of the loop's n instances is (a copy of).
    * groups: per-instance inputs (c[name] with the instances on axis 0, "noise" on axis 1).  L is a sum over the
      instances, so every entry of all of them is differentiated in ONE loop whose instances are the perturbed copies of
      the instance the entry belongs to.
    * shared {name: vector}: inputs all instances share, differentiated per instance: two loops per entry, -> (B, n).
    * the shared plan: each of its entries (plan_entries: (name, column, row) with the oracle's (6,Np+1) / (2,Np)
      orientation, default all) takes two loops and gives the gradient summed over B, -> {(r, i): v}.
    -> (dict of them all, every status 0)."""
    B, GS, GU = c["B"], c["GS"], c["GU"]
    shared = shared or {}
    base = dict({k: c[k] for k in (*groups, "plan_x", "plan_u")}, **shared)
    axis = lambda name: 1 if name == "noise" else 0  # noqa: E731
    out, ok = {"plan_x": {}, "plan_u": {}}, True
    owners, rows = [], {g: [] for g in groups}
    for name in groups:
        out[name] = np.zeros(c[name].shape)
        for idx in np.ndindex(c[name].shape):
            b = idx[axis(name)]
            for sgn in (1.0, -1.0):
                row = {g: np.take(c[g], b, axis=axis(g)).copy() for g in groups}
                row[name][idx[:axis(name)] + idx[axis(name) + 1:]] += sgn * h
                owners.append((name, idx, b))
                for g in groups:
                    rows[g].append(row[g])
    if owners:
        S, Ua, st = run(dict(base, **{g: np.moveaxis(np.array(rows[g]), 0, axis(g)) for g in groups}),
                        np.array([o[2] for o in owners]))
        ok = bool(np.all(st == 0))
        for m in range(0, len(owners), 2):
            name, idx, b = owners[m]
            L = [float(np.sum(GS[:, b] * S[:, m + d]) + np.sum(GU[:, b] * Ua[:, m + d])) for d in (0, 1)]
            out[name][idx] = (L[0] - L[1]) / (2.0 * h)

    def two_loops(name, changed, total):
        nonlocal ok
        L = []
        for sgn in (1.0, -1.0):
            S, Ua, st = run(dict(base, **{name: changed(sgn * h)}), np.arange(B))
            ok = ok and bool(np.all(st == 0))
            L.append(total(GS * S) + total(GU * Ua))
        return (L[0] - L[1]) / (2.0 * h)

    def bumped(v, at):
        def changed(d):
            w = np.array(v, dtype=np.float64)
            w[at] += d
            return w
        return changed

    for name, v in shared.items():
        out[name] = np.zeros((B, len(v)))
        for i in range(len(v)):
            out[name][:, i] = two_loops(name, bumped(v, i), lambda x: np.sum(x, axis=(0, 2)))
    Np = c["Np"]
    if plan_entries is None:
        plan_entries = [("plan_x", r, i) for r in range(Np + 1) for i in range(6)] + \
                       [("plan_u", r, i) for r in range(Np) for i in range(2)]
    for name, r, i in plan_entries:
        out[name][(r, i)] = two_loops(name, bumped(c[name], (i, r)), lambda x: float(np.sum(x)))
    return out, ok


def oracle_fd(c, h=1e-4, in_plant=False, plan_entries=None):
    """``central_differences`` of ``oracle_loop``.
    -> (dict(x_init (B,6), w (B,8), noise (K,B,6), plan_x {(r, i): v}, plan_u {(r, i): v}), every status 0)."""
    return central_differences(c, lambda i, owners: oracle_loop(c, i["x_init"], i["w"], i["noise"], i["plan_x"],
                                                                i["plan_u"], in_plant=in_plant),
                               ("x_init", "w", "noise"), None, h, plan_entries)


def oracle_tape(c, in_plant=False, run=None):
    """The oracle's own run of the case with each step's solution and interior multipliers (mu / slack on every finite
    relaxed bound, y from the stationarity least squares): what ``sweep`` needs.  run(rec) -> (S, Ua, status): another
    loop of the case that appends one dict(x_meas, X, U[, W, retried]) per step to rec, W (B,8) being the weights the
    accepted solves used (default: ``oracle_loop``, whose weights are the case's).
    -> dict(S, Ua, status, active, count, X (K,B,N+1,6), U (K,B,N,2), dual (K,B,N+1,22)[, W, retried, x_meas])."""
    from test_vjp_reference import _interior_dual
    nlp, N, B, K = c["nlp"], c["N"], c["B"], c["K"]
    rec = []
    S, Ua, st = run(rec) if run else oracle_loop(c, c["x_init"], c["w"], c["noise"], in_plant=in_plant, tape=rec)
    X, U = np.array([r["X"] for r in rec]), np.array([r["U"] for r in rec])
    W = np.array([r["W"] for r in rec]) if run else np.broadcast_to(c["w"], (K, B, 8))
    dual = np.zeros((K, B, N + 1, 22))
    for t in range(K):
        Xr, Ur = to.reference_window(c["plan_x"], c["plan_u"], c["ks"][t], N)
        for b in range(B):
            z = nlp.pack(X[t, b], U[t, b])
            y = nlp.kkt_residual(z, rec[t]["x_meas"][b], Xr, Ur, W[t, b, :6], W[t, b, 6:])["y"].reshape(N + 1, 6)
            dual[t, b] = _interior_dual(nlp, z, y)
    out = dict(S=S, Ua=Ua, status=st, active=np.ones((K, B), dtype=np.int32), count=np.zeros((K, B), dtype=np.int32),
               X=X, U=U, dual=dual)
    if run:
        out.update(W=W, retried=np.array([r["retried"] for r in rec]), x_meas=np.array([r["x_meas"] for r in rec]))
    return out
