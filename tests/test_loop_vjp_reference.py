"""CPU suite: the closed-loop adjoint references of tests/loop_vjp_reference.py pinned against the CPU oracle, no GPU.

1. The analytic plant Jacobians against central differences (h = 1e-6) of ``to.plant_update`` on the golden states, with
   and without disturbances, away from the kinks: <= 1e-7 (rounding is about eps |q| / h = 1e-8 for |q| = 40).
2. The numpy chain (``dense_vjp`` per step at the oracle's interior multipliers, plant and window adjoints between the
   steps) against central differences (h = 1e-4) of ``to.closed_loop``: all five gradient groups to <= 1e-6 absolute.
3. The branch table on synthetic logs: hand-built status sequences take every row of the table for the three policies;
   the sweep agrees with a brute-force differentiation of a numpy restatement of policy_plant_kernel around a linear
   stand-in for the solve.
"""
import numpy as np
import pytest

import loop_vjp_reference as lr
import vjp_reference as vr
from oracle import ttmpc_oracle as to

P = lr.P


# ---- 1 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("disturbed", [False, True])
def test_plant_jacobians_against_central_differences(golden_ref, disturbed):
    dist = lr.DIST if disturbed else None
    q, u = golden_ref["q"], golden_ref["u"]
    d0, d1 = lr.kink_distance(q, dist)
    keep = np.flatnonzero((d0 > 1e-3) & (d1 > 1e-3)) if disturbed else np.arange(q.shape[0])
    print(f"disturbed={disturbed}: {keep.size} of {q.shape[0]} points away from the kinks, max|q| {np.max(np.abs(q)):.1f}")
    assert 2 * keep.size >= q.shape[0]
    h, worst = 1e-6, 0.0
    for n in keep:
        Jq, Ju = lr.plant_jacobians(q[n], P, dist)
        for i in range(8):
            dq, du = np.zeros(6), np.zeros(2)
            (dq if i < 6 else du)[i % 6] = h
            fd = (to.plant_update(q[n] + dq, u[n] + du, P, dist) - to.plant_update(q[n] - dq, u[n] - du, P, dist)) / (2 * h)
            worst = max(worst, float(np.max(np.abs(fd - (Jq[:, i] if i < 6 else Ju[:, i - 6])))))
    print(f"disturbed={disturbed}: analytic vs central differences {worst:.3e}")
    assert worst <= 1e-7


# ---- 2 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_plant", [False, True])
def test_chain_against_oracle_loop_finite_differences(golden_ref, in_plant):
    c = lr.loop_case(golden_ref)
    tape = lr.oracle_tape(c, in_plant)
    assert np.all(tape["status"] == 0)
    umax = np.max(np.abs(tape["Ua"]), axis=(0, 1))
    print(f"in_plant={in_plant}: largest applied |u| {umax} against bounds (5, pi/2)")
    g = lr.chain(c, vr.dense_vjp, tape, "track", in_plant)
    fd, ok = lr.oracle_fd(c, h=1e-4, in_plant=in_plant)
    assert ok
    gpx, gpu_ = g["plan_x"].sum(axis=0), g["plan_u"].sum(axis=0)   # the oracle's plan is shared
    err = {"x_init": np.max(np.abs(g["x_init"] - fd["x_init"])), "w": np.max(np.abs(g["w"] - fd["w"])),
           "noise": np.max(np.abs(g["noise"] - fd["noise"])),
           "plan_x": max(abs(gpx[r, i] - v) for (r, i), v in fd["plan_x"].items()),
           "plan_u": max(abs(gpu_[r, i] - v) for (r, i), v in fd["plan_u"].items())}
    big = {"x_init": np.max(np.abs(g["x_init"])), "w": np.max(np.abs(g["w"])), "noise": np.max(np.abs(g["noise"])),
           "plan_x": np.max(np.abs(gpx)), "plan_u": np.max(np.abs(gpu_))}
    for k in lr.GROUPS:
        print(f"in_plant={in_plant} {k:7s}: chain vs oracle FD {err[k]:.3e}, largest entry {big[k]:.3e}")
    # a padded plan row (Np) and unpadded ones are both among the entries, and both carry a gradient
    assert (c["Np"], 0) in fd["plan_x"] and (1, 0) in fd["plan_x"]
    assert np.max(np.abs(gpx[c["Np"]])) > 0.0 and np.max(np.abs(gpx[1])) > 0.0
    assert max(err.values()) <= 1e-6
    for k in ("x_init", "w", "noise", "plan_u"):
        assert big[k] > 1e-3, k
    assert big["plan_x"] > 1e-3 * big["x_init"]


# ---- 3 ----------------------------------------------------------------------------------------------------------
def _standin_loop(policy, status, x_init, G, hvec, ufail, GS, GU, dist, plant_noise=None, log=None):
    """K steps of policy_plant with the solve replaced by U0_t = G S_t + h_t (a failed one returns the constant
    ufail_t: it has nothing to differentiate) and the statuses given.  -> L = sum(GS * S) + sum(GU * Ua)."""
    K, B = status.shape
    x = np.array(x_init, dtype=np.float64)
    u_last, consec, active = np.zeros((B, 2)), np.zeros(B, dtype=np.int64), np.ones(B, dtype=bool)
    L = float(np.sum(GS[0] * x))
    for t in range(K):
        u0 = np.where((status[t] <= 1)[:, None], x @ G.T + hvec[t], ufail[t])
        s_t = x
        x, ua, u_last, consec, active = lr.policy_plant(policy, x, u0, status[t], u_last, consec, active, P, dist,
                                                        None if plant_noise is None else plant_noise[t])
        if log is not None:
            log.append((s_t, consec.copy(), active.copy()))
        L += float(np.sum(GS[t + 1] * x) + np.sum(GU[t] * ua))
    return L


@pytest.mark.parametrize("in_plant", [False, True])
@pytest.mark.parametrize("policy", ["track", "nmpc", "fuzzy"])
def test_branch_table_on_synthetic_logs(policy, in_plant):
    """Instances: all success | isolated failures between successes | 17 failures in a row then success (fuzzy: past the
    zero-control threshold) | failures to the end (nmpc stops after 20, fuzzy after 30) | failure at t = 0."""
    K, B = 36, 5
    status = np.zeros((K, B), dtype=np.int32)
    status[[2, 5, 6], 1] = 3
    status[3:20, 2] = 3
    status[4:, 3] = 2
    status[0, 4] = 3
    rng = np.random.default_rng(3)
    # states that stay clear of the kinks for all K steps; instance 2 sits on the saturated side of min(s, 0.3)
    x_init = np.array([[1.0, 2.0, 0.3, 0.1, 0.15, 1.5], [-2.0, 1.0, -0.5, -0.2, -0.2, 2.0], [0.5, -1.0, 1.0, 0.05, 0.4, 3.0],
                       [3.0, 3.0, 2.0, 0.3, -0.12, -1.2], [0.0, 0.0, 0.0, 0.0, 0.2, -1.5]])
    G = rng.uniform(-0.005, 0.005, (2, 6))
    hvec, ufail = rng.uniform(-0.03, 0.03, (K, B, 2)), rng.uniform(-0.03, 0.03, (K, B, 2))
    GS, GU = rng.uniform(-1, 1, (K + 1, B, 6)), rng.uniform(-1, 1, (K, B, 2))
    pn = rng.normal(scale=0.02, size=(K, B, 6)) if in_plant else None

    def loss(x=x_init, hv=hvec, n=pn, log=None):
        return _standin_loop(policy, status, x, G, hv, ufail, GS, GU, lr.DIST, n, log)

    log = []
    L0 = loss(log=log)
    S = np.array([r[0] for r in log] + [log[-1][0]])           # S[K] is not read by the sweep
    count, active = np.array([r[1] for r in log]), np.array([r[2] for r in log]).astype(np.int32)
    d0, d1 = lr.kink_distance(S, lr.DIST)
    assert d0.min() > 1e-3 and d1.min() > 1e-3
    if policy == "nmpc":
        assert active[:, 3].tolist() == [1] * 24 + [0] * 12      # stopped by the 21st consecutive failure
    elif policy == "fuzzy":
        assert active[:, 3].tolist() == [1] * 34 + [0] * 2 and count[:, 2].max() == 17
    else:
        assert active.all()
    seeds = np.zeros((K, B, 2))

    def standin_vjp(t, g_u0):
        g = np.where((status[t] <= 1)[:, None], g_u0, 0.0)   # what tt_track_vjp_device does with a failed solve
        seeds[t] = g
        return {"x0": g @ G, "xref": np.zeros((B, 3, 6)), "uref": np.zeros((B, 2, 2)), "w": np.zeros((B, 8))}

    g = lr.sweep(standin_vjp, policy, [0] * K, 4, S, status, active, count, GS, GU, P, lr.DIST, in_plant)
    h, worst, big = 1e-6, 0.0, 0.0

    def central(name, arr, idx):
        out = []
        for sgn in (h, -h):
            v = arr.copy()
            v[idx] += sgn
            out.append(loss(**{name: v}))
        return (out[0] - out[1]) / (2 * h)

    for b in range(B):
        for i in range(6):
            d = central("x", x_init, (b, i))
            worst, big = max(worst, abs(d - g["x_init"][b, i])), max(big, abs(d))
    # the seeds are the gradient with respect to the stand-in's offsets h_t: steps around every change of branch
    for t in (0, 1, 2, 3, 5, 6, 7, 18, 19, 20, 23, 24, 33, 34, 35):
        for b in range(B):
            for i in range(2):
                d = central("hv", hvec, (t, b, i))
                worst, big = max(worst, abs(d - seeds[t, b, i])), max(big, abs(d))
    if in_plant:
        for t in (0, 5, 23, 24, 34, 35):
            for b in range(B):
                worst = max(worst, abs(central("n", pn, (t, b, 1)) - g["noise"][t, b, 1]))
    print(f"{policy} in_plant={in_plant}: |L| {abs(L0):.1f}, sweep vs brute force {worst:.3e}, largest derivative {big:.3e}")
    # central differences with h = 1e-6: the loss adds about 1e3 in absolute terms (37 x 5 x 6 state entries of size
    # up to 5), so rounding is at most eps 1e3 / h = 2e-7; truncation (h^2 x third derivatives) is far below it
    assert worst <= 2e-7
    assert big > 1e-1
    # the table's zero rows are exact zeros
    assert not seeds[status > 1].any()
    assert not seeds[:, 3][active[:, 3] == 0].any()
