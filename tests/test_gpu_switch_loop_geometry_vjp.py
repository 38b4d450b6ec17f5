"""GPU suite: the geometry gradients of the switch closed loop (ClosedLoop.backward(..., geometry=True)).

The loop is tests/test_gpu_switch_loop_vjp.py's: case A's scene, N = 6, B = 3, K = 4 steps on a shared straight plan
towards the obstacle at cx = 10.5; instances 0 and 1 are switched to the MPC+OBCA solve when their previous prediction
touches it, instance 2 never is.

1. backward(geometry=True): g_geometry_switch against the numpy chain (loop_vjp_reference.sweep) on the GPU's own
   tape, with the dense geometry adjoint (obca_geometry_reference.dense_geometry_vjp) on the switched instance-steps;
   the model chain uses the numpy model of the geometry kernel.  The harness's rule: err_gpu <= 10 err_model + 1e-12
   scale with err_model <= 1e-9 scale, the geometry group measured against max(its own max|ref|, max|g_x_init|).
2. A directional central difference of the GPU loop through loop.switch.set_geometry (the geometry is shared by the
   batch: the direction is the sum of g_geometry_switch over B), 1e-3 relative as the loop's directional tests, with
   the collision flags and the statuses the same at both points.  The step is 1e-5, the step the d_min loop test
   needed (instance 0 has an obstacle row that changes sides within 1e-4 of d_min = 0.2, and the body sizes move
   that row as d_min does).  Measured on an MI355X: finite difference 7.039523 against g . d 7.039540, 2.5e-6 relative.
3. The same directional difference for g_model_solver and g_model_plant through loop.set_model.  g_model_solver is
   also checked against the numpy chain of test 1 (the dense model adjoint of model_vjp_reference on the instance-steps
   that were not switched): measured difference 7e-18 on a largest entry of 2.1e-4.
   The steps.  These two gradients are small (g . d = 2.08e-4 and 5.41e-4) on a loss of order ten, and the loss of a
   perturbed run is not smooth at that level: a switched MPC+OBCA solve (84 .. 128 iterations) ends one iteration
   sooner or later at some perturbed points, which moves L by 2e-10 typically and by up to 3.5e-8.  The tracking and
   plant models enter smoothly (no obstacle row depends on them; the never-switched instance 2 agrees to 2e-6 relative
   at the step 1e-2 and to 2e-8 at 1e-3), so the step is the largest that keeps the truncation negligible instead of
   the 1e-5 of test 2: 1e-2 for the solver's geometry (the bound, 2.1e-7 absolute, needs noise / (2 step) below it)
   and 1e-3 for the plant's, the step of the model loop's directional test (tests/test_gpu_model_vjp.py; the plant's
   geometry also feeds the collision check, so it is kept smaller).  Measured on an MI355X, solver direction, finite
   difference against g . d = 2.081258e-4 per step: 1e-2 2.081379e-4; 3e-3 2.081589e-4; 1e-3 2.255253e-4 (instance 0
   alone is off by 1.7e-5: one of its switched solves changes its iteration count between the two points); 3e-4
   2.079374e-4; 1e-4 2.079006e-4; 3e-5 2.060816e-4; 1e-5 2.174918e-4; instance 2's share is 2.120364e-4 at every
   step.  Plant direction at 1e-3: 5.405744e-4 against 5.406960e-4 (2.2e-4 relative); at 1e-5 5.414438e-4.
4. geometry=True raises on a loop without switch_adjoint; model=True on the switch loop still raises.
"""
import functools

import numpy as np
import pytest

import loop_vjp_reference as lr
import model_vjp_reference as mvr
import obca_geometry_reference as ogr
import vjp_harness as h
import vjp_reference as vr

pytestmark = pytest.mark.gpu

_t, _n, _grads = h.t, h.n, h.grads
GROUPS = ("x_init", "w", "plan_x", "plan_u")


def _base():
    import test_gpu_switch_loop_vjp as base
    return base


@functools.lru_cache(maxsize=None)
def _run():
    b = _base()
    c = b._case()
    loop = b._loop(switch_adjoint=True)
    out = loop.run_tape(c["x_init"], c["T"])
    g = loop.backward(out["tape"], _t(c["GS"]), _t(c["GU"]), geometry=True)
    got = _grads(g)
    for k in ("g_geometry_switch", "g_model_solver", "g_model_plant"):
        got[k] = _n(g[k])
    plain = _grads(loop.backward(out["tape"], _t(c["GS"]), _t(c["GU"])))
    return loop, out, got, plain


def _chain(obca_fn, track_fn, model_fn):
    """loop_vjp_reference.sweep on the GPU's tape: obca_fn (a geometry route) on the switched instance-steps, track_fn
    on the others; the geometry rows are summed over the switched steps of each instance, and model_fn's (L1, L2, M)
    rows (model_vjp_reference) over the others."""
    from oracle import ttmpc_oracle as to
    b = _base()
    c = b._case()
    _, out, _, _ = _run()
    tp, rec = h.tape_np(out["tape"]), b._switched(out["tape"])
    N, nlp = c["N"], c["nlp"]
    geom, model_solver = np.zeros((c["B"], 5)), np.zeros((c["B"], 3))

    def cb(t, g_u0):
        B = g_u0.shape[0]
        Xr, Ur = to.reference_window(c["plan_x"], c["plan_u"], c["ks"][t], N)
        o = {"x0": np.zeros((B, 6)), "xref": np.zeros((B, N + 1, 6)), "uref": np.zeros((B, N, 2)),
             "w": np.zeros((B, 8))}
        for i in range(B):
            gU = np.zeros((N, 2))
            gU[0] = g_u0[i]
            if (t, i) in rec:
                I, st = rec[t, i]
                if st <= 1:
                    r = obca_fn(c["P_obca"], I, np.zeros((N + 1, 6)), gU, Xr.T, Ur.T)
                    for k in ("x0", "xref", "uref"):
                        o[k][i] = r[k]
                    geom[i] += r["geom"]
            elif tp["status"][t, i] <= 1:
                z = nlp.pack(tp["X"][t, i], tp["U"][t, i])
                r = track_fn(nlp, z, tp["dual"][t, i], Xr.T, Ur.T, np.zeros((N + 1, 6)), gU, None, None)
                for k in ("x0", "xref", "uref", "w"):
                    o[k][i] = r[k]
                model_solver[i] += model_fn(nlp, z, tp["dual"][t, i], np.zeros((N + 1, 6)), gU)["model"]
        return o
    g = lr.sweep(cb, "track", c["ks"], c["Np"], tp["S"], tp["status"], tp["active"], tp["consec"], c["GS"], c["GU"],
                 c["params"], None, False)
    return dict(h.shared_plan(g), geom=geom, model_solver=model_solver)


def test_backward_geometry_matches_the_numpy_chain_on_its_own_tape():
    _, out, got, plain = _run()
    dense = _chain(ogr.dense_geometry_vjp, vr.dense_vjp, mvr.dense_model_vjp)
    model = _chain(ogr.model_geometry_vjp, vr.riccati_vjp, mvr.riccati_model_vjp)
    big = h.compare_with_chain("switch loop, geometry", got, dense, model, GROUPS, per_group=False)
    unit = max(np.abs(dense["geom"]).max(), big["x_init"])
    e_gpu = np.abs(got["g_geometry_switch"] - dense["geom"]).max()
    e_model = np.abs(model["geom"] - dense["geom"]).max()
    print(f"switch loop, geometry: err_gpu {e_gpu:.3e}, err_model {e_model:.3e}, scale {unit:.3e}\n"
          f"   dense {dense['geom']}\n   gpu {got['g_geometry_switch']}")
    assert e_model <= 1e-9 * unit
    assert e_gpu <= 10.0 * e_model + 1e-12 * unit
    e_gpu = np.abs(got["g_model_solver"] - dense["model_solver"]).max()
    e_model = np.abs(model["model_solver"] - dense["model_solver"]).max()
    print(f"switch loop, g_model_solver: err_gpu {e_gpu:.3e}, err_model {e_model:.3e}, "
          f"max|ref| {np.abs(dense['model_solver']).max():.3e}")
    assert e_model <= 1e-9 * unit
    assert e_gpu <= 10.0 * e_model + 1e-12 * unit
    assert np.abs(dense["geom"]).max() > 1e-3                 # a switched step whose d_min row is active
    assert np.all(got["g_geometry_switch"][2] == 0.0)         # the instance that is never switched
    # the other groups of the same backward agree with the plain backward (each meets the 1e-9 cap)
    for k in GROUPS:
        assert np.abs(got[k] - plain[k]).max() <= 2e-9 * max(1.0, np.abs(plain[k]).max()), k


def _directional(set_point, base, g, eps):
    """Central difference of the GPU loop along d = g / |g| from base; set_point(loop, values)."""
    b = _base()
    c = b._case()
    _, out, _, _ = _run()
    d = g / np.linalg.norm(g)
    L, flags, stats = [], [], []
    plain = b._loop()
    for sgn in (1.0, -1.0):
        set_point(plain, np.asarray(base) + sgn * eps * d)
        r = plain.run(c["x_init"], c["T"])
        flags.append(r["collide"])
        stats.append(r["status"])
        assert np.all(r["status"] <= 1)
        L.append(float(np.sum(c["GS"] * r["states"]) + np.sum(c["GU"] * r["controls"])))
    assert np.array_equal(flags[0], flags[1]) and np.array_equal(flags[0], out["collide"])   # no switch straddled
    assert np.array_equal(stats[0], stats[1]) and np.array_equal(stats[0], out["status"])
    return (L[0] - L[1]) / (2 * eps), float(np.sum(g * d))


def test_central_difference_of_the_gpu_loop_in_the_switch_geometry():
    loop, out, got, _ = _run()
    g = got["g_geometry_switch"].sum(axis=0)
    names = ("L1", "L2", "M", "W1", "W2")
    fd, an = _directional(lambda lp, v: lp.switch.set_geometry(**dict(zip(names, v))), loop.switch.geometry(), g, 1e-5)
    print(f"switch geometry, direction {g / np.linalg.norm(g)}: finite difference {fd:.6e}, g . d {an:.6e}, relative "
          f"{abs(fd - an) / abs(an):.3e}")
    assert abs(fd - an) <= 1e-3 * abs(an)


@pytest.mark.parametrize("which", ["solver", "plant"])
def test_central_difference_of_the_gpu_loop_in_the_model(which):
    loop, out, got, _ = _run()
    g = got["g_model_" + which].sum(axis=0)
    base = loop.solver.model() if which == "solver" else loop.plant_model()
    fd, an = _directional(lambda lp, v: lp.set_model(**{which: v}), base, g, {"solver": 1e-2, "plant": 1e-3}[which])
    print(f"model_{which}, direction {g / np.linalg.norm(g)}: finite difference {fd:.6e}, g . d {an:.6e}, relative "
          f"{abs(fd - an) / abs(an):.3e}")
    assert abs(fd - an) <= 1e-3 * abs(an)


def test_what_raises():
    b = _base()
    c = b._case()
    loop, out, _, _ = _run()
    GS, GU = _t(c["GS"]), _t(c["GU"])
    with pytest.raises(ValueError, match="switch_adjoint"):
        b._loop().backward(out["tape"], GS, GU, geometry=True)
    with pytest.raises(ValueError, match="model=True"):
        loop.backward(out["tape"], GS, GU, model=True)
    keep = loop.switch.geometry()
    loop.switch.set_geometry(L1=keep[0] + 0.1)
    with pytest.raises(ValueError, match="geometry changed"):
        loop.backward(out["tape"], GS, GU, geometry=True)
    loop.switch.set_geometry(L1=keep[0])
    loop.backward(out["tape"], GS, GU, geometry=True)
