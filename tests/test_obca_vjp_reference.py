"""CPU checks of the reference algebra for the MPC+OBCA adjoint (tests/obca_vjp_reference.py): the dense un-condensed
solve against central differences of the CPU oracle, and the numpy model of obca_vjp_kernel against the dense solve.

Measured on the CPU oracle (largest absolute difference per group x0 / xref / uref):

  case                      dense vs differences (h = 1e-4)     model vs dense             largest entry (x0)
  A                         7.6e-7 / 2.0e-6 / 2.0e-6            6.5e-12 / 1e-14 / 3e-13    11.5
  A, obstacle at cx = 13    1.4e-9 / 8e-12 / 6e-12              3e-15 / 1e-15 / 1e-16      3.0
  A, x_init[1] = -0.1       3.2e-6 / 5.7e-6 / 3.1e-6            1.2e-11 / 2e-14 / 6e-13    11.1
  B (N = 8, M = 2)          2.1e-6 / 2.2e-6 / 2.2e-6            3.3e-13 / 1e-15 / 2e-14    2.9

The dense solve itself is exact to 6e-12 (x0) against 50-digit arithmetic on case A, which is where the model stands
with its refinement steps.  Without them (``steps=0``) the model misses the cap wherever an obstacle row is active
(4.2e-7, 4.7e-6 and 1.7e-5 on x0 for A, x_init[1] = -0.1 and B): the eliminated active block puts entries of 1e13 on
the pose block, the float64 Riccati pass over them loses seven digits, and the float64 addend cannot hold the
block's curvature beside them ("Adjoint of an MPC+OBCA solve").
"""
import functools

import numpy as np
import pytest

import obca_vjp_reference as orf

FD_BOUND = 1e-5      # absolute per group: the bound of the tracking adjoint's difference tests
MODEL_CAP = 1e-9     # err_model <= MODEL_CAP * max|ref| per group

CASES = {"A": lambda: orf.case_a(), "A_inactive": lambda: orf.case_a(cx=13.0), "A_left": lambda: orf.case_a(y0=-0.1),
         "B": orf.case_b}


@functools.lru_cache(maxsize=None)
def solved(name):
    """(P, iterate, upstream, central differences, dense, model) of a case, computed once."""
    N, p, Q, R, bnd, obs, x0, xr, ur = CASES[name]()
    P = orf.problem(N, p, Q, R, bnd, obs)
    gX, gU = orf.upstream(N)
    I, st, fd = orf.oracle_fd_vjp(P, x0, xr, ur, gX, gU)
    assert st == 0
    return P, I, (gX, gU), fd, orf.dense_obca_vjp(P, I, gX, gU), orf.model_obca_vjp(P, I, gX, gU)


def test_case_a_is_active_and_bent():
    P, I, _, _, _, _ = solved("A")
    v = orf.unpack(I, P.N, P.M)
    assert v["yd"][P.N, 0, 0] > 1.0            # the truck's d_min row at the last stage carries a multiplier
    assert np.all(np.abs(v["yd"][:P.N, :, 0]) < 1e-6)
    assert abs(v["u"][0, 0] + 1.36) < 0.01 and abs(v["u"][0, 1] + 0.35) < 0.01
    Pi, Ii, _, _, _, _ = solved("A_inactive")
    assert np.all(np.abs(orf.unpack(Ii, Pi.N, Pi.M)["yd"][..., 0]) < 1e-6)


def test_case_b_is_what_it_claims():
    """Several blocks per stage, an active obstacle row and an active input bound."""
    P, I, _, _, _, _ = solved("B")
    v = orf.unpack(I, P.N, P.M)
    assert P.M == 2 and v["w"].shape[1] == 4
    assert np.abs(v["yd"][..., 0]).max() > 1.0
    assert max(v["zLu"].max(), v["zUu"].max(), v["zLx"].max(), v["zUx"].max()) > 1e-3


@pytest.mark.parametrize("name", list(CASES))
def test_dense_matches_central_differences(name):
    _, _, _, fd, dense, _ = solved(name)
    err = orf.group_err(dense, fd)
    print(name, "dense vs central differences", err, "largest", orf.group_max(dense))
    for k in orf.KEYS:
        assert err[k] <= FD_BOUND, (k, err[k])


def test_inactive_case_is_the_plain_tracking_adjoint():
    """Without an active obstacle row the OBCA solve is the plain tracking NLP's, within the two solvers' tolerance:
    measured 8.0e-11 (x0), 2.0e-12 (xref), 1.05e-10 (uref); the bound is ten times that."""
    import sens_reference as sr
    import vjp_reference as vr
    from oracle import c_oracle as co
    from oracle import ttmpc_oracle as to
    N, p, Q, R, bnd, obs, x0, xr, ur = CASES["A_inactive"]()
    _, _, (gX, gU), _, dense, _ = solved("A_inactive")
    nlp = to.TrackingNLP(N, p, Q, R, *bnd)
    z, st, _, _ = co.solve_batch(sr.oracle_problem(nlp), x0[None], xr[None], ur[None])
    assert st[0] == 0
    dual = _tracking_duals(nlp, z[0], xr, ur)
    ref = vr.dense_vjp(nlp, z[0], dual, xr, ur, gX, gU, cond=False)
    err = orf.group_err(dense, ref)
    print("OBCA dense vs tracking dense", err)
    assert err["x0"] <= 8.0e-10 and err["xref"] <= 2.0e-11 and err["uref"] <= 1.05e-9, err


def _tracking_duals(nlp, z, xr, ur):
    """Multipliers of the tracking optimum in the export layout (N+1, 22): y from the stationarity rows by least
    squares, no bound active (the case's optimum is interior)."""
    g = nlp.grad(z, xr.T, ur.T)
    J = nlp.jacobian(z)
    y = np.linalg.lstsq(J.T, -g, rcond=None)[0]
    dual = np.zeros((nlp.N + 1, 22))
    dual[:, :6] = y.reshape(nlp.N + 1, 6)
    return dual


@pytest.mark.parametrize("name", list(CASES))
def test_model_matches_dense(name):
    """err_model <= 1e-9 max|ref| per group (measured: module docstring)."""
    _, _, _, _, dense, model = solved(name)
    assert model["ok"]
    err, mx = orf.group_err(model, dense), orf.group_max(dense)
    print(name, "model vs dense", err, "largest", mx)
    for k in orf.KEYS:
        assert err[k] <= MODEL_CAP * mx[k], (k, err[k], MODEL_CAP * mx[k])


def test_refinement_is_what_meets_the_cap():
    """Without the refinement steps the model is the condensed solve alone and misses the cap on case A by more than
    ten times: the steps are not decoration."""
    P, I, (gX, gU), _, dense, _ = solved("A")
    plain = orf.model_obca_vjp(P, I, gX, gU, steps=0)
    assert plain["ok"]
    assert orf.group_err(plain, dense)["x0"] > 10.0 * MODEL_CAP * orf.group_max(dense)["x0"]
