"""CPU suite: the reference algebra of tests/lqr_vjp_reference.py (what tests/test_gpu_lqr_vjp.py measures
lqr_vjp_kernel against) pinned by central differences of the score and by the tangent identity.

Inputs: the goals of tests/test_gpu_lqr.py (seed 9, B = 96), Q = I + 0.1 diag(0..5), R = [[10, 1], [1, 8]].  P comes from
``doubling_dare`` (a float64 restatement of lqr_kernel's iteration): scipy's Schur DARE leaves a residual ~1e-11 at the
near-stationary goals (|v| ~ 0.01, P ~ 1e7) and that swamps a difference quotient.

Central differences take, per instance and group (x_cur, x_goal, the symmetric entries of Q, of R), the best error over
h in {1e-4, 1e-5, 1e-6} relative to the group's largest entry.  Bounds: 1e-6 on the 88 goals with v drawn from +-3
(measured 3e-11 .. 4e-8 on three of them, v = 1.34, -2.55, -2.76, when the bound was set; eight of the 88 turn out to be
near standstill, so that test runs the same iteration in double-double, ``doubling_dare_dd``: its docstring has the
figures), 1e-4 on the nine near-stationary ones for x_goal and Q (measured 3.0e-6 and 7.1e-6).  R on the
near-stationary goals is not differenced (a score ~1e6 cannot resolve a gradient ~10): it is checked by the tangent
identity <G, dP> = <g, dtheta> with dP from the dense tangent solve, to 1e-9 relative, on all 96 instances, as are Q
and A along a random dx_goal (measured 1.0e-11, 1.4e-12, 3.8e-13; upstream on P alone 2.8e-13)."""
import functools

import numpy as np

import lqr_vjp_reference as lv

P6, Q, R = lv.P6, lv.Q_TEST, lv.R_TEST
HS = (1e-4, 1e-5, 1e-6)
GROUPS = ("x_cur", "x_goal", "Q", "R")


@functools.lru_cache(maxsize=None)
def _case():
    from conftest import GOLDEN
    xc, xg = lv.lqr_case(dict(np.load(GOLDEN / "reference_numpy.npz")))
    A = np.array([lv.linearise(x, P6)[0] for x in xg])
    P, its = lv.doubling_dare(A, lv.linearise(xg[0], P6)[1], Q, R)
    assert np.all(its > 0)
    return xc, xg, P


def _directions():
    """(group, dxc, dxg, dQ, dR) of every differenced entry."""
    z6, zQ, zR = np.zeros(6), np.zeros((6, 6)), np.zeros((2, 2))
    out = [("x_cur", np.eye(6)[m], z6, zQ, zR) for m in range(6)]
    out += [("x_goal", z6, np.eye(6)[m], zQ, zR) for m in range(6)]
    out += [("Q", z6, z6, lv.sym_direction(6, i, j), zR) for i, j in lv.SYM_Q]
    out += [("R", z6, z6, zQ, lv.sym_direction(2, i, j)) for i, j in lv.SYM_R]
    return out


@functools.lru_cache(maxsize=None)
def _case_dd():
    """The same P from the double-double iteration (a DD, (96,6,6))."""
    xc, xg, _ = _case()
    A = np.array([lv.linearise(x, P6)[0] for x in xg])
    P, its = lv.doubling_dare_dd(A, lv.linearise(xg[0], P6)[1], Q, R)
    assert np.all(its > 0)
    return P


def _fd_errors(instances, groups, dd=False):
    """-> {group: (len(instances),) best-over-h error relative to the group's largest entry}; one batched DARE, in
    float64 or (dd) in double-double, where the scores and their differences are double-double too and the formulas
    are evaluated at that P rounded to float64.  An x_cur entry moves no input of the DARE and takes the unperturbed P."""
    xc, xg, P = _case()
    Pd = _case_dd() if dd else None
    dirs = [d for d in _directions() if d[0] in groups]
    Bm = lv.linearise(xg[0], P6)[1]
    As, Qs, Rs, dxs, owner, moved = [], [], [], [], [], []
    for b in instances:
        for grp, dxc, dxg, dQ, dR in dirs:
            for h in HS:
                for sgn in (1.0, -1.0):
                    g = xg[b] + sgn * h * dxg
                    As.append(lv.linearise(g, P6)[0])
                    Qs.append(Q + sgn * h * dQ)
                    Rs.append(R + sgn * h * dR)
                    dxs.append(xc[b] + sgn * h * dxc - g)
                    owner.append(b)
                    moved.append(grp != "x_cur")
    As, Qs, Rs, dxs, owner, moved = (np.array(a) for a in (As, Qs, Rs, dxs, owner, moved))
    shape = (len(instances), len(dirs), len(HS), 2)
    if dd:
        Pp, its = lv.doubling_dare_dd(As[moved], Bm, Qs[moved], Rs[moved])
        Pall = lv.DD(np.zeros((len(owner), 6, 6)))
        Pall[moved], Pall[~moved] = Pp, Pd[owner[~moved]]
        dx = lv.DD(dxs)
        s = dx[:, None, :] @ (Pall @ dx[:, :, None])
        s = lv.DD(s.hi.reshape(shape), s.lo.reshape(shape))
        fd = (s[..., 0] - s[..., 1]).value() / (2.0 * np.array(HS))
        P = Pd.hi
    else:
        Pp, its = lv.doubling_dare(As[moved], Bm, Qs[moved], Rs[moved])
        Pall = np.zeros((len(owner), 6, 6))
        Pall[moved], Pall[~moved] = Pp, P[owner[~moved]]
        score = np.einsum("ni,nij,nj->n", dxs, Pall, dxs).reshape(shape)
        fd = (score[..., 0] - score[..., 1]) / (2.0 * np.array(HS))       # (instances, dirs, h)
    assert np.all(its > 0)
    err = {g: np.zeros(len(instances)) for g in groups}
    for n, b in enumerate(instances):
        r = lv.dense_lqr_vjp(xc[b], xg[b], P[b], R, 1.0, None, P6)
        an = np.array([r["g_x_cur"] @ dxc + r["g_x_goal"] @ dxg + np.sum(r["g_Q"] * dQ) + np.sum(r["g_R"] * dR)
                       for _, dxc, dxg, dQ, dR in dirs])
        for g in groups:
            sel = np.array([d[0] == g for d in dirs])
            e = np.abs(fd[n, sel] - an[sel, None]).max(axis=0) / np.abs(an[sel]).max()
            err[g][n] = e.min()
    return err


def test_central_differences_on_the_well_conditioned_goals():
    """All 88 instances, all four groups, 1e-6.  The doubling DARE is carried in double-double here.  Eight of the 88
    are not well conditioned: seven draws from U(-3, 3) landed near zero (instances 37, 46, 62, 68, 72, 73, 86:
    v = -0.091, -0.0072, 0.0024, -0.057, 0.0055, -0.100, -0.147) and instance 95 is the plan's final state (v = -0.01).
    There P ~ 1e5 .. 2e7, the float64 iteration returns it to ~1e-10, and the difference of two such scores cannot
    resolve the R gradient: differenced in float64 the eight give R errors 1.1e-6 .. 1.3e-2 and instance 46 a Q error
    1.29e-6 (the other 80: x_goal <= 3.9e-9, Q <= 7.2e-9, R <= 3.5e-7), and 80-bit arithmetic still leaves 4.4e-6 in R on
    instance 46.  In double-double the worst best-over-h errors are x_cur 9.6e-12, x_goal 1.7e-7 (instance 62, at
    h = 1e-6: the truncation term, which falls as h^2), Q 3.6e-11, R 3.7e-11."""
    inst = list(range(8, 96))                                              # the 88 goals with v drawn from +-3
    err = _fd_errors(inst, GROUPS, dd=True)
    for g in GROUPS:
        print(f"{g:7s}: worst best-over-h error {err[g].max():.3e} (instance {inst[int(err[g].argmax())]})")
    assert len(inst) == 88
    assert max(e.max() for e in err.values()) <= 1e-6


def test_near_stationary_goals_and_the_tangent_identity():
    xc, xg, P = _case()
    inst = list(lv.NEAR_STATIONARY)
    err = _fd_errors(inst, ("x_goal", "Q"))
    for g in ("x_goal", "Q"):
        print(f"{g:7s}: worst best-over-h error {err[g].max():.3e} (instance {inst[int(err[g].argmax())]})")
    assert len(inst) == 9 and max(e.max() for e in err.values()) <= 1e-4
    # tangent identity on every instance: R, Q, and A along a random dx_goal
    rng = np.random.default_rng(31)
    worst, done = {"R": 0.0, "Q": 0.0, "x_goal": 0.0}, 0
    for b in range(96):
        r = lv.dense_lqr_vjp(xc[b], xg[b], P[b], R, 1.0, None, P6)
        dR, dQ = rng.uniform(-1, 1, (2, 2)), rng.uniform(-1, 1, (6, 6))
        dR, dQ, dxg = dR + dR.T, dQ + dQ.T, rng.uniform(-1, 1, 6)
        dA = lv.goal_tangent(xg[b], dxg, P6)
        for key, M, rhs in (("R", lv.tangent_rhs(P[b], r["K"], r["Ac"], dR=dR), np.sum(r["g_R"] * dR)),
                            ("Q", lv.tangent_rhs(P[b], r["K"], r["Ac"], dQ=dQ), np.sum(r["g_Q"] * dQ)),
                            ("x_goal", lv.tangent_rhs(P[b], r["K"], r["Ac"], dA=dA),
                             (r["g_x_goal"] + r["g_x_cur"]) @ dxg)):     # (g_x_goal + 2 gs P dx: the part through A)
            lhs = np.sum(r["G"] * lv.dense_tangent(r["Ac"], M))
            worst[key] = max(worst[key], abs(lhs - rhs) / max(abs(lhs), abs(rhs)))
        done += 1
    print("tangent identity, worst relative mismatch: " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert done == 96
    assert max(worst.values()) <= 1e-9


def test_upstream_on_P_alone():
    xc, xg, P = _case()
    rng = np.random.default_rng(32)
    worst = 0.0
    for b in range(96):
        GP = rng.uniform(-1, 1, (6, 6))
        r = lv.dense_lqr_vjp(xc[b], xg[b], P[b], R, 0.0, GP, P6)
        assert not r["g_x_cur"].any() and np.array_equal(r["G"], 0.5 * (GP + GP.T))
        dR, dQ = rng.uniform(-1, 1, (2, 2)), rng.uniform(-1, 1, (6, 6))
        dR, dQ, dxg = dR + dR.T, dQ + dQ.T, rng.uniform(-1, 1, 6)
        M = lv.tangent_rhs(P[b], r["K"], r["Ac"], dQ=dQ, dR=dR, dA=lv.goal_tangent(xg[b], dxg, P6))
        dP = lv.dense_tangent(r["Ac"], M)
        lhs = np.sum(GP * 0.5 * (dP + dP.T))                               # the forward symmetrises P
        rhs = np.sum(r["g_Q"] * dQ) + np.sum(r["g_R"] * dR) + r["g_x_goal"] @ dxg
        worst = max(worst, abs(lhs - rhs) / max(abs(lhs), abs(rhs)))
    print(f"upstream on P alone, worst relative mismatch: {worst:.3e}")
    assert worst <= 1e-9
