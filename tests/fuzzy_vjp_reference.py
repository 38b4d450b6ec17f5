"""Test helper (numpy only): the fuzzy weight rule as data (tt_fuzzy_rule, include/ttmpc.h), its adjoint, and the
backward sweep of tests/loop_vjp_reference.py extended by it.

One step of a rule loop:  w_t = rule(x_meas_t, xref_t[0]; theta);  X_t, U_t = solve(x_meas_t, xref_t, uref_t, w_t); an
instance whose solve fails is re-solved once with unit weights (mpc_control_fuzzy.py:145-159), and then w_t = 1 does not
depend on anything.  The solve adjoint's g_w therefore flows through the rule into dL/dx_meas_t[3] and dL/dtheta, except
where the retry was taken.

* ``rule_weights`` / ``rule_vjp``: the rule and its adjoint table, vectorised over leading axes.
* ``rule_kink_distance``: how far a point is from every kink and switch of the rule.
* ``chain``: lr.sweep on a tape, with the rule adjoint between the solve adjoint and the state accumulation.
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
def window_ref_v(plan_x, ks, Np, B):
    """ref_v (K,B) of a shared plan (6,Np+1): the speed of the window's first row."""
    return np.array([[plan_x[5, min(k, Np)]] * B for k in ks])


def chain(c, fn, tp, in_plant=True, policy="fuzzy", theta=None, settings=SETTINGS):
    """``lr.chain`` on a tape dict that also has W and retried: the sweep at each step's own weights, with ``rule_vjp``
    (nothing where retried) as its rule term."""
    theta = c["theta"] if theta is None else theta
    K, B = tp["status"].shape
    x_meas = tp["S"][:K] if in_plant else tp["S"][:K] + c["noise"]
    ref_v = window_ref_v(c["plan_x"], c["ks"], c["Np"], B)

    def rule(t, g_w):
        return (*rule_vjp(theta, x_meas[t][:, 3], x_meas[t][:, 5], ref_v[t], g_w, settings),
                np.asarray(tp["retried"][t]) == 0)
    return lr.chain(c, fn, tp, policy, in_plant, rule_vjp=rule)


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
    return lr.oracle_tape(c, run=lambda rec: oracle_loop(c, c["x_init"], c["noise"], tape=rec, force=force))


def oracle_fd(c, h=1e-4, force=None, plan_entries=None):
    """``lr.central_differences`` of ``oracle_loop``: x_init and noise in one loop of perturbed copies (a forced failure
    follows its owner), theta per instance, the shared plan summed over B.  force: {t: instance b}.
    -> (dict(x_init (B,6), noise (K,B,6), theta (B,7), plan_x {(r, i): v}, plan_u {(r, i): v}), every final status 0)."""
    force = force or {}
    return lr.central_differences(
        c, lambda i, owners: oracle_loop(c, i["x_init"], i["noise"], i["theta"], i["plan_x"], i["plan_u"],
                                         force={t: owners == b for t, b in force.items()}),
        ("x_init", "noise"), {"theta": c["theta"]}, h, plan_entries)


def fd_errors(g, fd):
    """Largest absolute differences, per group, between a sweep's gradients (plan per instance: summed here; or already
    (1, ., .)) and ``oracle_fd``'s."""
    gpx, gpu_ = np.asarray(g["plan_x"]).sum(axis=0), np.asarray(g["plan_u"]).sum(axis=0)
    return {"x_init": float(np.max(np.abs(g["x_init"] - fd["x_init"]))),
            "noise": float(np.max(np.abs(g["noise"] - fd["noise"]))),
            "plan_x": max(abs(gpx[r, i] - v) for (r, i), v in fd["plan_x"].items()),
            "plan_u": max(abs(gpu_[r, i] - v) for (r, i), v in fd["plan_u"].items()),
            "theta": float(np.max(np.abs(g["theta"] - fd["theta"])))}


def group_max(a):
    return lr.group_max(a, GROUPS)
