"""CPU checks of the reference algebra for the scene and weight gradients of an MPC+OBCA solve
(tests/obca_scene_reference.py): the dense un-condensed solve against central differences of the CPU oracle in the
obstacles, d_min and the diagonals of Q and R, against its own extended-precision refinement, and the numpy model of
the params kernel (block unknowns carried) against it.

Measured on the CPU oracle, largest absolute difference over scale (obca_scene_reference.scales):

  case                 dense vs refined (obs | Q | R)   carried, 3 steps (obs | Q | R)   recomputed v (obs) | with t
  A                    5.6e-13 | 3.9e-12 | 3.0e-10      <1e-16 | 3.9e-16 | 4.2e-14       6.2e-16 | 1.5e-16
  A, cx = 13           1e-24   | 3.5e-14 | 4.5e-16      1e-27  | 1.5e-16 | 0             2e-27   | 2e-27
  A, x_init[1] = -0.1  1.1e-12 | 4.9e-12 | 1.0e-11      1e-17  | 2.7e-16 | 1.2e-15       4.9e-6  | 5.8e-9
  B (N = 8, M = 2)     9.9e-14 | 5.8e-14 | 9.8e-14      7.6e-17 | 3.9e-17 | 0            3.2e-6  | 1.1e-7
  golden window 10     (sparse reference)               6.6e-15 | 1.6e-12 | 1.7e-12      -       | 5.9e-7

(N = 50, M = 11 for the window; with two steps it stands at 5.6e-12 | 1.4e-9 | 1.6e-9, which misses the cap on Q and
R, so the kernel takes three.)  Dense against the oracle's differences: A obs 1.9e-8, d_min 9e-9, Q 6.7e-9, R 8e-10;
B obs 2.2e-6, d_min 7.9e-8, Q 2.1e-7, R 4.6e-9.
"""
import functools

import numpy as np
import pytest

import obca_scene_reference as osr
import obca_vjp_reference as orf
from oracle import c_oracle as co

FD_BOUND = 1e-5      # absolute: the bound of the existing difference tests
MODEL_CAP = 1e-9     # err <= MODEL_CAP * scale per group

CASES = {"A": lambda: orf.case_a(), "A_inactive": lambda: orf.case_a(cx=13.0), "A_left": lambda: orf.case_a(y0=-0.1),
         "B": orf.case_b}


@functools.lru_cache(maxsize=None)
def solved(name):
    """(case, P, iterate, upstream, dense, refined dense) of a case, computed once."""
    case = CASES[name]()
    N, p, Q, R, bnd, obs, x0, xr, ur = case
    P = orf.problem(N, p, Q, R, bnd, obs)
    gX, gU = orf.upstream(N)
    z, st, _, _, I = co.obca_solve_batch(P, x0[None], xref=xr[None], uref=ur[None], iterate=True)
    assert st[0] == 0
    return (case, P, I[0], (gX, gU), osr.dense_scene_vjp(P, I[0], gX, gU, xr, ur),
            osr.dense_scene_vjp(P, I[0], gX, gU, xr, ur, refined=True))


@pytest.mark.parametrize("name", ["A", "B"])
def test_dense_matches_central_differences(name):
    case, P, I, (gX, gU), dense, _ = solved(name)
    x0, xr, ur = case[6:]
    fd = osr.oracle_fd_scene(P, x0, xr, ur, gX, gU)
    err = {"obs": np.abs(fd["obs"] - dense["obs"]).max(), "dmin": abs(fd["dmin"] - dense["dmin"]),
           "Q": np.abs(fd["Qd"] - np.diag(dense["Q"])).max(), "R": np.abs(fd["Rd"] - np.diag(dense["R"])).max()}
    print(name, "dense vs central differences", err, "obs", dense["obs"], "dmin", dense["dmin"])
    for k, e in err.items():
        assert e <= FD_BOUND, (k, e)
    assert np.array_equal(np.array(P.obs[:4 * P.M]).reshape(-1, 4), case[5]) and P.dmin == 0.2  # (P is restored)
    assert abs(dense["dmin"]) > 1.0  # the case is active


def test_face_contact_identity():
    """Case A touches the obstacle's -x face: g_cx = -g_dmin and g_w = g_dmin / 2 (the other entries are ~0)."""
    _, _, _, _, dense, _ = solved("A")
    g = dense["obs"][0]
    assert abs(g[0] + dense["dmin"]) <= 1e-7 * abs(dense["dmin"])
    assert abs(g[2] - 0.5 * dense["dmin"]) <= 1e-7 * abs(dense["dmin"])


@pytest.mark.parametrize("name", list(CASES))
def test_dense_matches_its_refinement(name):
    _, _, _, _, dense, ref = solved(name)
    err, sc = osr.group_err(dense, ref), osr.scales(ref)
    print(name, "dense vs refined", err, "scales", sc)
    for k in osr.KEYS:
        assert err[k] <= MODEL_CAP * sc[k], (k, err[k], sc[k])


@pytest.mark.parametrize("name", ["A", "A_left", "B"])
def test_carried_route_meets_the_cap(name):
    case, P, I, (gX, gU), _, ref = solved(name)
    xr, ur = case[7:]
    model = osr.model_scene_vjp(P, I, gX, gU, xr, ur)
    assert model["ok"]
    err, sc = osr.group_err(model, ref), osr.scales(ref)
    print(name, "carried vs refined dense", err, "scales", sc)
    for k in osr.KEYS:
        assert err[k] <= MODEL_CAP * sc[k], (k, err[k], sc[k])


def test_recomputed_route_misses_the_cap():
    """v = -K_b^-1 C lx_pose from the final pose adjoint misses the cap on the scene groups by more than 100 times on
    A with x_init[1] = -0.1 (measured: about 5e3 times), while its x0 group is fine: carrying v is not decoration."""
    case, P, I, (gX, gU), _, ref = solved("A_left")
    xr, ur = case[7:]
    rec = osr.recomputed_scene_vjp(P, I, gX, gU, xr, ur)
    err, sc = osr.group_err(rec, ref), osr.scales(ref)
    print("recomputed vs refined dense", err, "scales", sc)
    assert err["obs"] > 100.0 * MODEL_CAP * sc["obs"] and err["dmin"] > 100.0 * MODEL_CAP * sc["dmin"]
    assert err["x0"] <= MODEL_CAP * sc["x0"]


def test_inactive_scene_has_no_gradient():
    _, _, _, _, dense, _ = solved("A_inactive")
    top = np.abs(dense["x0"]).max()
    assert np.abs(dense["obs"]).max() <= 1e-9 * top and abs(dense["dmin"]) <= 1e-9 * top
