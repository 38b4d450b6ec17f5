"""CPU suite: the sensitivity references of tests/sens_reference.py pinned against the CPU oracle, no GPU.

* The dense d(solution)/d(x_init) (multipliers from ``kkt_residual()["y"]``, variables within 1e-6 of a bound treated as
  active rows) agrees with central finite differences (h = 1e-4) of ``c_oracle.solve_batch`` to <= 1e-5 absolute on
  both input sets.
* The numpy Riccati (the CPU model of track_sens_kernel) and the dense barrier form are the same linear algebra: on a
  synthetic interior primal-dual point they agree to the accuracy a backward-stable dense solve has,
  10 eps cond(KKT) max|S|.
* ``layout.casadi_multipliers`` orders and signs the export as CasADi's lam_g / lam_x.
* The same two pins under non-diagonal weights (``mpc_full`` of tests/track_patterns.py) scaled by ``random_weights``,
  where the GPU suites lean on the references' off-diagonal terms.
* ``optimality_error`` (the E0 of track_kernel's loop, restated) on interior points of the oracle's optima: its
  complementarity is the mu the point was built with, its dual infeasibility is ``kkt_residual``'s stationarity.
"""
import numpy as np
import pytest

import sens_reference as sr


@pytest.fixture(scope="module", params=["free", "active"])
def fd_case(request):
    nlp, x0, xr, ur = sr.case_free() if request.param == "free" else sr.case_active()
    z, st, dz = sr.oracle_fd(nlp, x0, xr, ur, h=1e-4)
    return request.param, nlp, x0, xr, ur, z, st, dz


def test_dense_reference_matches_oracle_finite_differences(fd_case):
    name, nlp, x0, xr, ur, z, st, dz = fd_case
    assert np.all(st == 0)
    worst = 0.0
    for b in range(x0.shape[0]):
        k = nlp.kkt_residual(z[b], x0[b], xr[b].T, ur[b].T)
        act = sr.active_set(nlp, z[b])
        # x_0 is held by its own equality rows; a pinned x_0 entry would duplicate one
        act = act[act >= 6]
        if name == "free":
            assert act.size == 0
        else:
            assert 13 <= act.size <= 18, act.size
        ref = sr.dense_sensitivity(nlp, z[b], k["y"].reshape(nlp.N + 1, 6), pinned=act)
        fd = sr._split(nlp, dz[b])
        err_gain, err = float(np.max(np.abs(fd["gain"] - ref["gain"]))), sr.max_err(fd, ref)
        # A bound that is active to 1e-6 but whose slack exceeds IPOPT's relaxation (1e-8) is only weakly active: the
        # barrier solution the oracle returns keeps a finite Sigma = z / s there, so the variable still moves a little
        # and the active-row form is not its derivative (instance 0 of the active set: omega_5, slack 1.7e-7,
        # dU_5/dx0 = -1.3e-5 by finite differences at h, 2h and h/2).  The gain is checked everywhere; the whole
        # trajectory sensitivity where no bound is weakly active.
        lb, ub = nlp.bounds()
        with np.errstate(invalid="ignore"):
            slack = np.minimum(z[b] - lb, ub - z[b])[act]
            weak = bool(np.any(slack > sr.RELAX * np.maximum(1.0, np.abs(np.where(z[b] - lb < ub - z[b], lb, ub)[act]))))
        print(f"{name} instance {b}: active {act.size}, weakly active {weak}, max|K| {np.max(np.abs(ref['gain'])):.4f}, "
              f"FD vs dense: gain {err_gain:.3e}, all {err:.3e}")
        worst = max(worst, err_gain if weak else err)
    assert worst <= 1e-5, worst
    if name == "active":  # instance 2: a_0 free (a live row of the gain), omega_0 on its bound (a dead row)
        K = sr._split(nlp, dz[2])["gain"]
        assert np.max(np.abs(K[0])) > 0.01
        assert np.max(np.abs(K[1])) <= 1e-5


@pytest.mark.parametrize("case", ["free", "active"])
def test_riccati_model_is_the_dense_barrier_form(case):
    from oracle import c_oracle as co
    nlp, x0, xr, ur = sr.case_free() if case == "free" else sr.case_active()
    z, st, _, _ = co.solve_batch(sr.oracle_problem(nlp), x0, xr, ur)
    N = nlp.N
    lbr, ubr = sr.relaxed_bounds(nlp)
    for b in range(0, x0.shape[0], 2):
        # an interior primal-dual point: y of the optimum, z = mu / slack on every finite bound (mu = 1e-9)
        y = nlp.kkt_residual(z[b], x0[b], xr[b].T, ur[b].T)["y"].reshape(N + 1, 6)
        with np.errstate(divide="ignore"):
            zl = np.where(np.isfinite(lbr), 1e-9 / (z[b] - lbr), 0.0)
            zu = np.where(np.isfinite(ubr), 1e-9 / (ubr - z[b]), 0.0)
        assert np.all(z[b] > lbr) and np.all(z[b] < ubr)
        dual = np.zeros((N + 1, 22))
        dual[:, :6] = y
        dual[:N, 6:14], dual[N, 6:12] = zl[:8 * N].reshape(N, 8), zl[8 * N:]
        dual[:N, 14:22], dual[N, 14:20] = zu[:8 * N].reshape(N, 8), zu[8 * N:]
        dense = sr.dense_sensitivity(nlp, z[b], y, sig=sr.sigma(nlp, z[b], dual))
        model = sr.riccati_sensitivity(nlp, z[b], dual)
        assert model["ok"]
        err, tol = sr.max_err(model, dense), 10.0 * np.finfo(float).eps * dense["cond"] * sr.max_abs(dense)
        print(f"{case} instance {b}: Riccati vs dense {err:.3e} (bound {tol:.3e}, cond {dense['cond']:.2e})")
        assert err <= tol


def test_full_weights_dense_and_riccati_against_the_oracle():
    """``mpc_full`` weighted, free inputs: dense vs oracle FD <= 1e-5, Riccati vs dense <= 10 eps cond max|S|."""
    import vjp_reference as vr
    from test_vjp_reference import _interior_dual
    nlp, x0, xr, ur = sr.case_free("mpc_full")
    assert nlp.Q[0, 1] == 0.25 and nlp.R[0, 1] == 0.5
    w = vr.random_weights(x0.shape[0])
    z, st, dz = sr.oracle_fd(nlp, x0, xr, ur, h=1e-4, wq=w[:, :6], wr=w[:, 6:])
    assert np.all(st == 0)
    for b in range(x0.shape[0]):
        wq, wr = w[b, :6], w[b, 6:]
        y = nlp.kkt_residual(z[b], x0[b], xr[b].T, ur[b].T, wq, wr)["y"].reshape(nlp.N + 1, 6)
        assert sr.active_set(nlp, z[b]).size == 0
        ref = sr.dense_sensitivity(nlp, z[b], y, wq=wq, wr=wr)
        err = sr.max_err(sr._split(nlp, dz[b]), ref)
        dual = _interior_dual(nlp, z[b], y)
        dense = sr.dense_sensitivity(nlp, z[b], y, sig=sr.sigma(nlp, z[b], dual), wq=wq, wr=wr)
        model = sr.riccati_sensitivity(nlp, z[b], dual, wq, wr)
        assert model["ok"]
        e2, tol = sr.max_err(model, dense), 10.0 * np.finfo(float).eps * dense["cond"] * sr.max_abs(dense)
        plain = sr.riccati_sensitivity(nlp, z[b], dual)
        print(f"mpc_full weighted instance {b}: FD vs dense {err:.3e}, Riccati vs dense {e2:.3e} (bound {tol:.3e}), "
              f"weights move the gain by {np.max(np.abs(plain['gain'] - model['gain'])):.3e}")
        assert err <= 1e-5
        assert e2 <= tol
        assert np.max(np.abs(plain["gain"] - model["gain"])) > 1e-4   # a reference that ignored the weights would differ


@pytest.mark.parametrize("pattern,weighted", [("mpc_diag", False), ("mpc_full", True), ("obca", False)])
def test_optimality_error_on_interior_points(pattern, weighted):
    import vjp_reference as vr
    from oracle import c_oracle as co
    from test_vjp_reference import _interior_dual
    nlp, x0, xr, ur = sr.case_free(pattern)
    w = vr.random_weights(x0.shape[0]) if weighted else None
    z, st, _, _ = co.solve_batch(sr.oracle_problem(nlp), x0, xr, ur, wq=None if w is None else w[:, :6],
                                 wr=None if w is None else w[:, 6:])
    assert np.all(st == 0)
    eps, mu = np.finfo(float).eps, 1e-9
    for b in range(x0.shape[0]):
        wq, wr = (None, None) if w is None else (w[b, :6], w[b, 6:])
        k = nlp.kkt_residual(z[b], x0[b], xr[b].T, ur[b].T, wq, wr)
        dual = _interior_dual(nlp, z[b], k["y"].reshape(nlp.N + 1, 6), mu=mu)
        e = sr.optimality_error(nlp, z[b], x0[b], xr[b], ur[b], dual, wq, wr)
        _, zl, zu = sr.dual_in_z_order(dual, nlp.N)
        print(f"{pattern} weighted={weighted} instance {b}: E0 {e['E0']:.3e} dinf {e['dinf']:.3e} (stat {k['stat']:.3e}) "
              f"pinf {e['pinf']:.3e} (prim {k['prim']:.3e}) c0 {e['c0']:.3e} s_d {e['s_d']} s_c {e['s_c']} "
              f"scale {e['scale']:.3e}")
        assert abs(e["c0"] - mu) <= 4.0 * eps * mu                    # z s = (mu / s) s: one division, one product
        assert e["pinf"] == k["prim"]
        # no bound is active on this input set, so kkt_residual's residual is grad f + J' y: ours adds -z_L + z_U
        assert sr.active_set(nlp, z[b]).size == 0
        assert abs(e["dinf"] - k["stat"]) <= float(np.max(zl + zu)) + 64.0 * eps * e["scale"]
        assert e["s_d"] == 1.0 and e["s_c"] == 1.0
        assert e["E0"] == max(e["dinf"], e["pinf"], e["c0"])
        assert 1.0 < e["scale"] < 1e3


def test_casadi_multipliers_order_and_sign():
    from ttmpc import layout
    N = 3
    rng = np.random.default_rng(0)
    dual = rng.uniform(0.0, 1.0, (2, N + 1, 22))
    dual[:, N, 12:14] = 0.0
    dual[:, N, 20:22] = 0.0
    lam_g, lam_x = layout.casadi_multipliers(dual, N)
    assert lam_g.shape == (2, 6 * (N + 1)) and lam_x.shape == (2, 8 * N + 6)
    for k in range(N + 1):
        assert np.array_equal(lam_g[0, 6 * k:6 * k + 6], dual[0, k, :6])
        nv = 8 if k < N else 6
        assert np.array_equal(lam_x[1, 8 * k:8 * k + nv], dual[1, k, 14:14 + nv] - dual[1, k, 6:6 + nv])
    g1, x1 = layout.casadi_multipliers(dual[0], N)
    assert np.array_equal(g1, lam_g[0]) and np.array_equal(x1, lam_x[0])
