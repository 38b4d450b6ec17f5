"""CPU checks of the reference algebra for the geometry gradient of an MPC+OBCA solve
(tests/obca_geometry_reference.py): the dense un-condensed solve's closed forms against the central difference of
lam' F(theta) at the fixed iterate and against central differences of the CPU oracle's solve, and the numpy model of
the geometry kernel (block unknowns carried) against the refined dense solve.

Measured on the CPU oracle (order L1, L2, Mh, W1, W2):

  case  dense closed forms                                               vs residual difference   vs oracle difference
  F     -2.16377178  1.18168e-5  -2.48600e-3  -0.70992458  -5.3e-14      1.9e-9                   1.0e-6 (d_min 9.2e-7)
  R     6.65885e-3   10.9172981  10.9177672   8.1e-14      2.96308147    5.5e-9                   1.4e-7 (d_min 6.8e-7)
  B     -1.53815791  -2.28623e-5 1.23140e-4   1.5151e-8    -6.3e-10      8.7e-10                  -

F: block share -2.05107451 (L1), -0.70992458 (W1), dynamics share -0.11269727 (L1).  R: block share 10.9333295 (L2),
10.8676013 (Mh), 2.96308147 (W2), dynamics share 6.65885e-3, -1.60314e-2, 5.01660e-2.  A with cx = 13: every block
share <= 1.8e-11 on max|g_x0| = 2.98, the gradient is the dynamics share (3.98e-5, -5.2e-9, 2.36e-6).

Carried route (3 steps and the closing pass, lam_y of the last step) against the refined dense solve, geometry group,
largest absolute difference | scale: A 3e-29 | 11.5; A, x_init[1] = -0.1 4e-19 | 11.1; B 2.2e-16 | 2.90; F 7e-21 | 10.6;
R 1.8e-15 | 69.6 (the other groups are bitwise model_scene_vjp's).  v recomputed from the final pose adjoint on A,
x_init[1] = -0.1: 5.5e-5 on the scale 11.1, 5e3 times the cap.
"""
import functools

import numpy as np
import pytest

import obca_geometry_reference as ogr
import obca_scene_reference as osr
import obca_vjp_reference as orf
from oracle import c_oracle as co

FD_BOUND = 1e-5      # absolute: the bound of the existing difference tests
MODEL_CAP = 1e-9     # err <= MODEL_CAP * scale per group

CASES = {"A": lambda: orf.case_a(), "A_inactive": lambda: orf.case_a(cx=13.0), "A_left": lambda: orf.case_a(y0=-0.1),
         "B": orf.case_b, "F": ogr.case_f, "R": ogr.case_r}


@functools.lru_cache(maxsize=None)
def solved(name):
    """(case, P, iterate, upstream, dense with its parts, refined dense) of a case, computed once."""
    case = CASES[name]()
    N, p, Q, R, bnd, obs, x0, xr, ur = case
    P = orf.problem(N, p, Q, R, bnd, obs)
    gX, gU = orf.upstream(N)
    z, st, _, _, I = co.obca_solve_batch(P, x0[None], xref=xr[None], uref=ur[None], iterate=True)
    assert st[0] == 0
    return (case, P, I[0], (gX, gU), ogr.dense_geometry_vjp(P, I[0], gX, gU, xr, ur, parts=True),
            ogr.dense_geometry_vjp(P, I[0], gX, gU, xr, ur, refined=True))


@pytest.mark.parametrize("name", ["F", "R", "B"])
def test_closed_forms_match_the_residual_difference(name):
    """-d(lam' F)/dtheta at the fixed iterate, by central differences of the oracle's block linearisation and of
    ttmpc_oracle.f / jac_f, against the closed forms with the same lam."""
    case, P, I, _, dense, _ = solved(name)
    lx, lu, ly, vblk = dense["parts"]
    keep = ogr.get_theta(P)
    fd = ogr.residual_fd_geometry(P, I, lx, ly, vblk)
    assert np.array_equal(ogr.get_theta(P), keep)  # (P is restored)
    err = np.abs(fd - dense["geom"])
    print(name, "closed forms", dense["geom"], "residual differences", fd, "err", err)
    assert err.max() <= FD_BOUND, err


@pytest.mark.parametrize("name", ["F", "R"])
def test_dense_matches_central_differences(name):
    case, P, I, (gX, gU), dense, _ = solved(name)
    x0, xr, ur = case[6:]
    keep = ogr.get_theta(P)
    fd, fd_dmin = ogr.oracle_fd_geometry(P, x0, xr, ur, gX, gU, h=1e-4)
    assert np.array_equal(ogr.get_theta(P), keep) and P.dmin == 0.2
    err = np.abs(fd - dense["geom"])
    print(name, "dense", dense["geom"], "block", dense["geom_block"], "dyn", dense["geom_dyn"], "\n  oracle differences",
          fd, "err", err, "d_min", dense["dmin"], fd_dmin)
    assert err.max() <= FD_BOUND, err
    assert abs(fd_dmin - dense["dmin"]) <= FD_BOUND
    g = dict(zip(ogr.THETA, dense["geom"]))
    if name == "F":  # the case is active in the truck's length and width
        assert abs(g["L1"]) > 1.0 and abs(g["W1"]) > 0.1
    else:            # and in the trailer's length, hitch offset and width
        assert abs(g["L2"]) > 1.0 and abs(g["Mh"]) > 1.0 and abs(g["W2"]) > 1.0


def test_inactive_scene_leaves_the_dynamics_share():
    _, _, _, _, dense, _ = solved("A_inactive")
    top = np.abs(dense["x0"]).max()
    print("inactive: block", dense["geom_block"], "dyn", dense["geom_dyn"], "max|g_x0|", top)
    assert np.abs(dense["geom_block"]).max() <= 1e-9 * top
    assert np.array_equal(dense["geom_dyn"][3:], np.zeros(2))


@pytest.mark.parametrize("name", ["A", "A_left", "B", "F", "R"])
def test_carried_route_meets_the_cap(name):
    case, P, I, (gX, gU), _, ref = solved(name)
    xr, ur = case[7:]
    model = ogr.model_geometry_vjp(P, I, gX, gU, xr, ur)
    assert model["ok"]
    scene = osr.model_scene_vjp(P, I, gX, gU, xr, ur)
    for k in osr.KEYS:  # the shared groups are the params route's, bit for bit
        assert np.array_equal(np.asarray(model[k]), np.asarray(scene[k])), k
    err, sc = ogr.group_err(model, ref), ogr.scales(ref)
    print(name, "carried vs refined dense", err, "scales", sc, "geom", ref["geom"])
    for k in ogr.KEYS:
        assert err[k] <= MODEL_CAP * sc[k], (k, err[k], sc[k])


def test_recomputed_route_misses_the_cap():
    """v = -K_b^-1 C lx_pose from the final pose adjoint misses the cap on the geometry group by more than 100 times on
    A with x_init[1] = -0.1, as it does on the scene groups: the block terms need the carried v."""
    case, P, I, (gX, gU), _, ref = solved("A_left")
    xr, ur = case[7:]
    rec = ogr.recomputed_geometry_vjp(P, I, gX, gU, xr, ur)
    err, sc = ogr.group_err(rec, ref), ogr.scales(ref)
    print("recomputed vs refined dense", err["geom"], "scale", sc["geom"])
    assert err["geom"] > 100.0 * MODEL_CAP * sc["geom"]
    assert err["x0"] <= MODEL_CAP * sc["x0"]
