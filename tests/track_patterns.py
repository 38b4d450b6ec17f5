"""Test helper (numpy only): the weight forms and bound patterns that select track_kernel's generic builds, one table
for every suite that runs more than the default problem.

Each entry is (Q, R, xlb, xub, ulb, uub).  The MPC pattern with diagonal and with non-diagonal weights, the OBCA pattern
with both, and a pattern that is neither, which takes the build that reads its bounds at run time.  The off-diagonal
weights are dyadic, so that the kernels' symmetrisation 0.5 (Q_ij + Q_ji) is exact: ``mpc_asym`` is an asymmetric Q, R
whose symmetric part is bitwise ``mpc_full``.
"""
import numpy as np


def patterns():
    from oracle import ttmpc_oracle as to
    q_full = np.array(to.DEFAULT_Q, dtype=float)
    q_full[0, 1] = q_full[1, 0] = 0.25   # symmetric, diagonally dominant: still positive definite
    q_full[2, 3] = q_full[3, 2] = -0.125
    r_full = np.array(to.DEFAULT_R, dtype=float)
    r_full[0, 1] = r_full[1, 0] = 0.5
    q_asym, r_asym = q_full.copy(), r_full.copy()
    q_asym[0, 1], q_asym[1, 0] = 0.375, 0.125
    q_asym[2, 3], q_asym[3, 2] = -0.1875, -0.0625
    r_asym[0, 1], r_asym[1, 0] = 0.75, 0.25
    mpc = (to.MPC_XLB, to.MPC_XUB, to.MPC_ULB, to.MPC_UUB)
    obca = (to.OBCA_XLB, to.OBCA_XUB, to.MPC_ULB, to.MPC_UUB)
    one_sided = np.array(to.MPC_XUB, dtype=float)
    one_sided[2] = np.inf                # heading bounded below only: neither the MPC nor the OBCA pattern
    return {
        "mpc_diag": (to.DEFAULT_Q, to.DEFAULT_R) + mpc,
        "mpc_full": (q_full, r_full) + mpc,
        "mpc_asym": (q_asym, r_asym) + mpc,
        "obca": (to.DEFAULT_Q, to.DEFAULT_R) + obca,
        "obca_full": (q_full, r_full) + obca,
        "run_time": (to.DEFAULT_Q, to.DEFAULT_R, to.MPC_XLB, one_sided, to.MPC_ULB, to.MPC_UUB),
    }


# (input set, pattern, weighted) of the derivative suites: ``case_free`` under every pattern, ``case_active`` under the two
# MPC weight forms; the default problem unweighted is each suite's own first case
DERIVATIVE_CASES = [c for c in
                    [("free", p, w) for p in ("mpc_diag", "mpc_full", "obca", "run_time") for w in (False, True)]
                    + [("active", p, w) for p in ("mpc_diag", "mpc_full") for w in (False, True)]
                    if c[1:] != ("mpc_diag", False)]


def nlp_of(pattern, N, params, ulb=None, uub=None):
    """The oracle's TrackingNLP of a pattern at horizon N (ulb / uub: another input box, as ``case_active`` has)."""
    from oracle import ttmpc_oracle as to
    Q, R, xlb, xub, pl, pu = patterns()[pattern]
    f = lambda a: np.array(a, dtype=float)  # noqa: E731
    return to.TrackingNLP(N, params=dict(params, horizon=N), Q=f(Q), R=f(R), xlb=f(xlb), xub=f(xub),
                          ulb=f(pl if ulb is None else ulb), uub=f(pu if uub is None else uub))
