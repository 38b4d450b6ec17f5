"""GPU suite: the scene gradients of the switch closed loop (ClosedLoop.backward(..., scene=True)).

The loop is tests/test_gpu_switch_loop_vjp.py's: case A's scene, N = 6, B = 3, K = 4 steps on a shared straight plan
towards the obstacle at cx = 10.5; instances 0 and 1 are switched to the MPC+OBCA solve when their previous prediction
touches it, instance 2 never is.

1. backward(scene=True) against the numpy chain (loop_vjp_reference.sweep) on the GPU's own tape, with the dense scene
   adjoint (obca_scene_reference.dense_scene_vjp) on the switched instance-steps; the model chain uses the numpy model
   of the params kernel.  The harness's rule: err_gpu <= 10 err_model + 1e-12 scale, the scene groups measured against
   max(their own max|ref|, max|g_x_init|) (they share a unit with the position entries of g_x_init).
2. A central difference of the GPU loop in the switch solver's d_min (shared by the batch: the sum of g_dmin), 1e-3
   relative as the loop's directional test, with the collision flags the same at both points.  The step is 1e-5: the
   gradient is first order with the active set fixed, and instance 0 (switched at steps 1 and 3) has an obstacle row
   that changes sides within 1e-4 of d_min = 0.2.  Measured per instance (gradient 1.25587144 | 5.7544084 | 0):
   step 1e-3 0.2213 | 5.75440808; 3e-4 0.4546 | 5.75440837; 1e-4 1.1183 | 5.75440757; 3e-5 1.25623567 | 5.75440564;
   1e-5 1.25586321 | 5.75440938.  Instance 1, whose active set does not move, agrees at every step.
3. scene=True raises on a loop without switch_adjoint or without a switch solver.
"""
import functools

import numpy as np
import pytest

import loop_vjp_reference as lr
import obca_scene_reference as osr
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
    g = loop.backward(out["tape"], _t(c["GS"]), _t(c["GU"]), scene=True)
    got = _grads(g)
    got["obs"], got["dmin"] = _n(g["g_obstacles"]), _n(g["g_dmin"])
    plain = _grads(loop.backward(out["tape"], _t(c["GS"]), _t(c["GU"])))
    return loop, out, got, plain


def _chain(obca_fn, track_fn):
    """loop_vjp_reference.sweep on the GPU's tape: obca_fn (a scene route) on the switched instance-steps, track_fn on
    the others; the scene rows are summed over the switched steps of each instance."""
    from oracle import ttmpc_oracle as to
    b = _base()
    c = b._case()
    _, out, _, _ = _run()
    tp, rec = h.tape_np(out["tape"]), b._switched(out["tape"])
    N, nlp, M = c["N"], c["nlp"], c["obs"].shape[0]
    scene = {"obs": np.zeros((c["B"], M, 4)), "dmin": np.zeros(c["B"])}

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
                    scene["obs"][i] += r["obs"]
                    scene["dmin"][i] += r["dmin"]
            elif tp["status"][t, i] <= 1:
                r = track_fn(nlp, nlp.pack(tp["X"][t, i], tp["U"][t, i]), tp["dual"][t, i], Xr.T, Ur.T,
                             np.zeros((N + 1, 6)), gU, None, None)
                for k in ("x0", "xref", "uref", "w"):
                    o[k][i] = r[k]
        return o
    g = lr.sweep(cb, "track", c["ks"], c["Np"], tp["S"], tp["status"], tp["active"], tp["consec"], c["GS"], c["GU"],
                 c["params"], None, False)
    return dict(h.shared_plan(g), **scene)


def test_backward_scene_matches_the_numpy_chain_on_its_own_tape():
    _, out, got, plain = _run()
    dense = _chain(osr.dense_scene_vjp, vr.dense_vjp)
    model = _chain(osr.model_scene_vjp, vr.riccati_vjp)
    big = h.compare_with_chain("switch loop, scene", got, dense, model, GROUPS, per_group=False)
    unit = max(np.abs(dense["obs"]).max(), np.abs(dense["dmin"]).max(), big["x_init"])
    for k in ("obs", "dmin"):
        e_gpu, e_model = np.abs(got[k] - dense[k]).max(), np.abs(model[k] - dense[k]).max()
        print(f"switch loop, scene {k}: err_gpu {e_gpu:.3e}, err_model {e_model:.3e}, scale {unit:.3e}, "
              f"max|ref| {np.abs(dense[k]).max():.3e}")
        assert e_model <= 1e-9 * unit, k
        assert e_gpu <= 10.0 * e_model + 1e-12 * unit, k
    assert np.abs(dense["dmin"]).max() > 1e-3          # a switched step whose d_min row is active
    assert np.all(got["obs"][2] == 0.0) and got["dmin"][2] == 0.0   # the instance that is never switched
    # the other groups of the same backward agree with the plain backward (each meets the 1e-9 cap)
    for k in GROUPS:
        assert np.abs(got[k] - plain[k]).max() <= 2e-9 * max(1.0, np.abs(plain[k]).max()), k


def test_central_difference_of_the_gpu_loop_in_d_min():
    b = _base()
    c = b._case()
    loop, out, got, _ = _run()
    an = float(got["dmin"].sum())
    eps, L, flags = 1e-5, [], []
    plain = b._loop()
    for sgn in (1.0, -1.0):
        plain.switch.set_scene(d_min=0.2 + sgn * eps)
        r = plain.run(c["x_init"], c["T"])
        flags.append(r["collide"])
        assert np.all(r["status"] <= 1)
        L.append(float(np.sum(c["GS"] * r["states"]) + np.sum(c["GU"] * r["controls"])))
    assert np.array_equal(flags[0], flags[1]) and np.array_equal(flags[0], out["collide"])   # no switch straddled
    fd = (L[0] - L[1]) / (2 * eps)
    print(f"dL/dd_min of the loop: finite difference {fd:.6e}, sum of g_dmin {an:.6e}, relative "
          f"{abs(fd - an) / abs(an):.3e}")
    assert abs(fd - an) <= 1e-3 * abs(an)


def test_scene_needs_the_switch_adjoint():
    from ttmpc import simulation as sim
    b = _base()
    c = b._case()
    loop, out, _, _ = _run()
    GS, GU = _t(c["GS"]), _t(c["GU"])
    with pytest.raises(ValueError, match="switch_adjoint"):
        b._loop().backward(out["tape"], GS, GU, scene=True)
    track = sim.ClosedLoop(h.solver(c["nlp"], c["params"]), c["plan_x"], c["plan_u"], c["params"], None)
    tape = track.run_tape(c["x_init"], c["T"])["tape"]
    with pytest.raises(ValueError, match="scene=True"):
        track.backward(tape, GS, GU, scene=True)
