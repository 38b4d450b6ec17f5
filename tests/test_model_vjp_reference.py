"""CPU suite: the model-geometry references of tests/model_vjp_reference.py pinned against the CPU oracle, no GPU.

1. ``dense_model_vjp`` against central differences (h = 1e-4) of ``c_oracle.solve_batch`` (solved to 1e-12) over L1, L2,
   M, on both input sets with and without weights: <= 1e-7 absolute, every parameter's largest entry above 1e-3.
2. ``riccati_model_vjp`` (the CPU model of track_vjp_kernel's model instantiation, r_k / lam_y sweep included) against
   the dense form to 10 eps cond(K) max|ref|; lam_y,0 equals the x_init gradient to the same bound.
3. The plant term against central differences (h = 1e-6) of ``to.plant_update`` in L1, L2, M on the golden states,
   nominal and disturbed, away from the kinks: <= 1e-7.
4. The closed-loop chain against central differences of ``to.closed_loop`` with the solver's and the plant's geometry
   perturbed apart, both noise modes: <= 1e-6.

Every case prints its figures before it asserts (DESIGN.md "Adjoint in the model geometry" records them).
"""
import numpy as np
import pytest

import loop_vjp_reference as lv
import model_vjp_reference as mr
import sens_reference as sr
import vjp_reference as vr
from oracle import ttmpc_oracle as to
from test_vjp_reference import _interior_dual


def _case(name):
    return sr.case_free() if name == "free" else sr.case_active()


def _dual(nlp, z, x0, xr, ur, wq, wr):
    y = nlp.kkt_residual(z, x0, xr.T, ur.T, wq, wr)["y"].reshape(nlp.N + 1, 6)
    return _interior_dual(nlp, z, y)


# ---- 1 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("case", ["free", "active"])
def test_dense_model_vjp_matches_oracle_finite_differences(case, weighted):
    """The oracle is solved to ``model_vjp_reference.ORACLE_FD_TOL`` in every case (the comment there says why: at its
    default tolerance one weakly active bound of [active-True] is undecided and the difference quotient is off by 2e-5)."""
    nlp, x0, xr, ur = _case(case)
    B, N = x0.shape[0], nlp.N
    w = vr.random_weights(B) if weighted else None
    gX, gU = vr.random_upstream(B, N)
    z, st, fd = mr.oracle_fd_model(nlp, x0, xr, ur, gX, gU, w=w, h=1e-4)
    assert np.all(st == 0)
    ref = np.zeros((B, 3))
    for b in range(B):
        wq, wr = (None, None) if w is None else (w[b, :6], w[b, 6:])
        ref[b] = mr.dense_model_vjp(nlp, z[b], _dual(nlp, z[b], x0[b], xr[b], ur[b], wq, wr), gX[b], gU[b], wq, wr,
                                    cond=False)["model"]
    worst, big = np.max(np.abs(fd - ref), axis=0), np.max(np.abs(ref), axis=0)
    print(f"{case} weighted={weighted}: FD vs dense (L1, L2, M) {worst}, largest entries {big}")
    assert np.max(worst) <= 1e-7
    assert np.min(big) > 1e-3


# ---- 2 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("case", ["free", "active"])
def test_riccati_model_vjp_is_the_dense_solve(case, weighted):
    from oracle import c_oracle as co
    nlp, x0, xr, ur = _case(case)
    B, N = x0.shape[0], nlp.N
    w = vr.random_weights(B) if weighted else None
    gX, gU = vr.random_upstream(B, N)
    z, st, _, _ = co.solve_batch(sr.oracle_problem(nlp), x0, xr, ur, wq=None if w is None else w[:, :6],
                                 wr=None if w is None else w[:, 6:])
    for b in range(0, B, 2):
        wq, wr = (None, None) if w is None else (w[b, :6], w[b, 6:])
        dual = _dual(nlp, z[b], x0[b], xr[b], ur[b], wq, wr)
        dense = mr.dense_model_vjp(nlp, z[b], dual, gX[b], gU[b], wq, wr)
        model = mr.riccati_model_vjp(nlp, z[b], dual, gX[b], gU[b], wq, wr)
        assert model["ok"]
        eps_cond = 10.0 * np.finfo(float).eps * dense["cond"]
        err, tol = float(np.max(np.abs(model["model"] - dense["model"]))), eps_cond * float(np.max(np.abs(dense["model"])))
        err_y, tol_y = float(np.max(np.abs(model["ly"] - dense["ly"]))), eps_cond * float(np.max(np.abs(dense["ly"])))
        err_0 = float(np.max(np.abs(model["ly0"] - model["x0"])))
        print(f"{case} weighted={weighted} instance {b}: model gradient {err:.3e} (bound {tol:.3e}), lam_y {err_y:.3e} "
              f"(bound {tol_y:.3e}, max {np.max(np.abs(dense['ly'])):.2f}), lam_y,0 vs p_0 {err_0:.3e}, "
              f"cond {dense['cond']:.2e}")
        assert err <= tol
        assert err_y <= tol_y
        assert err_0 <= tol_y


def test_full_weights_dense_and_riccati_against_the_oracle():
    """Cases 1 and 2 under the non-diagonal ``mpc_full`` weights of tests/track_patterns.py, weighted, free inputs."""
    from oracle import c_oracle as co
    nlp, x0, xr, ur = sr.case_free("mpc_full")
    B, N = x0.shape[0], nlp.N
    w = vr.random_weights(B)
    gX, gU = vr.random_upstream(B, N)
    z, st, fd = mr.oracle_fd_model(nlp, x0, xr, ur, gX, gU, w=w, h=1e-4)
    assert np.all(st == 0)
    ref = np.zeros((B, 3))
    for b in range(B):
        wq, wr = w[b, :6], w[b, 6:]
        dual = _dual(nlp, z[b], x0[b], xr[b], ur[b], wq, wr)
        dense = mr.dense_model_vjp(nlp, z[b], dual, gX[b], gU[b], wq, wr)
        model = mr.riccati_model_vjp(nlp, z[b], dual, gX[b], gU[b], wq, wr)
        assert model["ok"]
        ref[b] = dense["model"]
        err = float(np.max(np.abs(model["model"] - dense["model"])))
        tol = 10.0 * np.finfo(float).eps * dense["cond"] * float(np.max(np.abs(dense["model"])))
        print(f"mpc_full weighted instance {b}: Riccati vs dense {err:.3e} (bound {tol:.3e})")
        assert err <= tol
    worst, big = np.max(np.abs(fd - ref), axis=0), np.max(np.abs(ref), axis=0)
    print(f"mpc_full weighted: FD vs dense (L1, L2, M) {worst}, largest entries {big}")
    assert np.max(worst) <= 1e-7
    assert np.min(big) > 1e-3


# ---- 3 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("disturbed", [False, True])
def test_plant_term_against_central_differences(golden_ref, disturbed):
    dist = lv.DIST if disturbed else None
    q, u = golden_ref["q"], golden_ref["u"]
    d0, d1 = lv.kink_distance(q, dist)
    keep = np.flatnonzero((d0 > 1e-3) & (d1 > 1e-3)) if disturbed else np.arange(q.shape[0])
    assert 2 * keep.size >= q.shape[0]
    q, u = q[keep], u[keep]
    h, worst, big = 1e-6, 0.0, 0.0
    for i in range(6):   # a = e_i: row i of dS+/dtheta
        a = np.zeros_like(q)
        a[:, i] = 1.0
        g = mr.plant_model_vjp(q, a, lv.P, dist)
        for j, name in enumerate(mr.THETA):
            pp, pm = dict(lv.P), dict(lv.P)
            pp[name] += h
            pm[name] -= h
            fd = (to.plant_update(q, u, pp, dist) - to.plant_update(q, u, pm, dist))[:, i] / (2 * h)
            worst, big = max(worst, float(np.max(np.abs(fd - g[:, j])))), max(big, float(np.max(np.abs(g[:, j]))))
    print(f"disturbed={disturbed}: {keep.size} points, plant term vs central differences {worst:.3e}, largest {big:.3e}")
    assert worst <= 1e-7
    assert big > 1e-6


# ---- 4 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_plant", [False, True])
def test_chain_against_oracle_loop_finite_differences(golden_ref, in_plant):
    c = lv.loop_case(golden_ref)
    tape = lv.oracle_tape(c, in_plant)
    assert np.all(tape["status"] == 0)
    g = mr.chain(c, mr.dense_model_vjp, tape, "track", in_plant)
    gs, gp = g["model_solver"], g["model_plant"]
    fs, fp, ok = mr.oracle_loop_fd(c, in_plant, h=1e-4)
    assert ok
    es, ep = np.max(np.abs(gs - fs), axis=0), np.max(np.abs(gp - fp), axis=0)
    bs, bp = np.max(np.abs(gs), axis=0), np.max(np.abs(gp), axis=0)
    print(f"in_plant={in_plant} solver geometry: chain vs oracle FD {es}, largest entries {bs}")
    print(f"in_plant={in_plant} plant  geometry: chain vs oracle FD {ep}, largest entries {bp}")
    assert max(np.max(es), np.max(ep)) <= 1e-6
    # the comparison is not between zeros: each geometry's largest entry is at least a hundred times the bound (the
    # loop applies only U[0] of six short solves, so the solver's share is much smaller than that of a loss on a whole
    # solve: 1.2e-4 in L1, 9e-6 in L2)
    assert np.max(bs) > 1e-4 and np.max(bp) > 1e-4
