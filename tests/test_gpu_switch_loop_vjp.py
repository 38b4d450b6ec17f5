"""GPU suite: the adjoint of the switch closed loop (ClosedLoop(..., switch_solver=obca, switch_adjoint=True)).

The loop is case A's scene (tests/obca_vjp_reference.py): N = 6, dt = 0.1, B = 3, K = 4 steps on a shared straight plan
at v = 1.5 from X = 1.5 towards the obstacle at cx = 10.5 (slow enough that the MPC+OBCA solve can still stop the truck
when the check, which looks at the previous prediction, first fires).  A step switches an instance to the MPC+OBCA
solve when its previous prediction touches the obstacle.  Instances 0 and 1 drive along the plan (0 a little ahead of it); instance 2 drives
3 m beside it, clear of the obstacle, and is never switched.

1. run_tape is run(), bitwise, and the tape keeps the switch record.
2. The backward sweep against the numpy chain (loop_vjp_reference.sweep) on the GPU's own tape, with the dense OBCA
   adjoint on the switched instance-steps and the dense tracking adjoint on the others; the model chain uses the two
   numpy models.  The harness's rule: err_gpu <= 10 err_model + 1e-12 max|ref|.
3. A directional central difference of the GPU loop in x_init, 1e-3 relative, with the collision flags the same at both
   perturbed points.
4. The default loop still raises; model=True, rule=True and run_graph raise.
"""
import functools

import numpy as np
import pytest

import loop_vjp_reference as lr
import obca_vjp_reference as orf
import vjp_harness as h
import vjp_reference as vr

pytestmark = pytest.mark.gpu

_t, _n, _grads = h.t, h.n, h.grads
GROUPS = ("x_init", "w", "plan_x", "plan_u")   # (the run has no noise)


@functools.lru_cache(maxsize=None)
def _case():
    from oracle import ttmpc_oracle as to
    N, p, Q, R, bnd, obs, x0, xr, ur = orf.case_a()
    B, T = 3, 0.35
    ks = to.step_indices(T, p["dt"])
    Np = 10
    plan_x = np.zeros((6, Np + 1))
    plan_x[0] = 1.5 + 0.15 * np.arange(Np + 1)
    plan_x[5] = 1.5
    plan_u = np.zeros((2, Np))
    x_init = np.array([[1.6, 0.1, 0.02, 0.0, 0.0, 1.5], [1.5, 0.1, 0.02, 0.0, 0.0, 1.5],
                       [1.5, -3.0, 0.0, 0.0, 0.0, 1.5]])
    rng = np.random.default_rng(9)
    K = len(ks)
    GS, GU = rng.uniform(-1.0, 1.0, (K + 1, B, 6)), rng.uniform(-1.0, 1.0, (K, B, 2))
    nlp = to.TrackingNLP(N, dict(p, horizon=N), Q, R, *bnd)
    return dict(N=N, B=B, T=T, K=K, ks=ks, Np=Np, nlp=nlp, params=p, obs=obs, plan_x=plan_x, plan_u=plan_u,
                x_init=x_init, GS=GS, GU=GU, P_obca=orf.problem(N, p, Q, R, bnd, obs), Q=Q, R=R, bnd=bnd)


def _loop(**kw):
    import ttmpc
    from ttmpc import simulation as sim
    c = _case()
    obca = ttmpc.ObcaSolver(c["N"], c["params"], c["Q"], c["R"], *c["bnd"], c["obs"],
                            variant=ttmpc.TT_VARIANT_TRACK_OBCA)
    return sim.ClosedLoop(h.solver(c["nlp"], c["params"]), c["plan_x"], c["plan_u"], c["params"], None,
                          obstacles=c["obs"], switch_solver=obca, **kw)


@functools.lru_cache(maxsize=None)
def _run():
    c = _case()
    loop = _loop(switch_adjoint=True)
    out = loop.run_tape(c["x_init"], c["T"])
    g = loop.backward(out["tape"], _t(c["GS"]), _t(c["GU"]))
    return loop, out, _grads(g)


def _switched(tape):
    """{(t, b): (iterate, status)} of the tape's switch record."""
    rec = {}
    for t, r in enumerate(tape.switched):
        if r is not None:
            idx, I, st = (_n(v) for v in r)
            for i, b in enumerate(idx):
                rec[t, int(b)] = (I[i], int(st[i]))
    return rec


def test_the_run_switches_and_run_tape_is_run():
    c = _case()
    loop, out, _ = _run()
    plain = _loop().run(c["x_init"], c["T"])
    for k in ("states", "controls", "status", "iters", "collide"):
        assert np.array_equal(out[k], plain[k]), k
    rec = _switched(out["tape"])
    print("collide\n", out["collide"].astype(int), "\nstatus\n", out["status"], "\nswitched", sorted(rec))
    assert len(out["tape"].switched) == c["K"]
    assert set(rec) == {(t, b) for t in range(c["K"]) for b in range(c["B"]) if out["collide"][t, b]}
    assert any(st <= 1 for _, st in rec.values())           # a switched instance-step that solved
    assert not out["collide"][:, 2].any()                    # an instance that is never switched
    for (t, b), (_, st) in rec.items():
        assert st == out["status"][t, b]


def _chain(obca_fn, track_fn):
    """loop_vjp_reference.sweep on the GPU's tape: obca_fn on the switched instance-steps, track_fn on the others."""
    from oracle import ttmpc_oracle as to
    c = _case()
    _, out, _ = _run()
    tp, rec = h.tape_np(out["tape"]), _switched(out["tape"])
    N, nlp = c["N"], c["nlp"]

    def cb(t, g_u0):
        B = g_u0.shape[0]
        Xr, Ur = to.reference_window(c["plan_x"], c["plan_u"], c["ks"][t], N)
        o = {"x0": np.zeros((B, 6)), "xref": np.zeros((B, N + 1, 6)), "uref": np.zeros((B, N, 2)),
             "w": np.zeros((B, 8))}
        for b in range(B):
            gU = np.zeros((N, 2))
            gU[0] = g_u0[b]
            if (t, b) in rec:
                I, st = rec[t, b]
                if st <= 1:
                    r = obca_fn(c["P_obca"], I, np.zeros((N + 1, 6)), gU)
                    for k in ("x0", "xref", "uref"):
                        o[k][b] = r[k]
            elif tp["status"][t, b] <= 1:
                r = track_fn(nlp, nlp.pack(tp["X"][t, b], tp["U"][t, b]), tp["dual"][t, b], Xr.T, Ur.T,
                             np.zeros((N + 1, 6)), gU, None, None)
                for k in ("x0", "xref", "uref", "w"):
                    o[k][b] = r[k]
        return o
    g = lr.sweep(cb, "track", c["ks"], c["Np"], tp["S"], tp["status"], tp["active"], tp["consec"], c["GS"], c["GU"],
                 c["params"], None, False)
    return h.shared_plan(g)


def test_backward_matches_the_numpy_chain_on_its_own_tape():
    _, out, got = _run()
    dense = _chain(orf.dense_obca_vjp, vr.dense_vjp)
    model = _chain(orf.model_obca_vjp, vr.riccati_vjp)
    big = h.compare_with_chain("switch loop", got, dense, model, GROUPS, per_group=False)
    assert big["x_init"] > 1e-3
    # switched instance-steps add nothing to g_wq_wr: the chain has zeros there too, and the comparison above holds


def test_directional_central_difference_of_the_gpu_loop():
    c = _case()
    loop, out, got = _run()
    g = got["x_init"]
    d = g / np.linalg.norm(g)
    eps, L, flags = 1e-4, [], []
    plain = _loop()
    for sgn in (1.0, -1.0):
        r = plain.run(c["x_init"] + sgn * eps * d, c["T"])
        flags.append(r["collide"])
        assert np.all(r["status"] <= 1)
        L.append(float(np.sum(c["GS"] * r["states"]) + np.sum(c["GU"] * r["controls"])))
    assert np.array_equal(flags[0], flags[1]) and np.array_equal(flags[0], out["collide"])   # no switch straddled
    fd, an = (L[0] - L[1]) / (2 * eps), float(np.sum(g * d))
    print(f"directional derivative along g_x_init: finite difference {fd:.6e}, g . d {an:.6e}, relative "
          f"{abs(fd - an) / abs(an):.3e}")
    assert abs(fd - an) <= 1e-3 * abs(an)


def test_what_still_raises_and_the_autograd_layer():
    import torch
    from ttmpc import simulation as sim
    from ttmpc.diff import DifferentiableClosedLoop
    c = _case()
    default = _loop()
    with pytest.raises(ValueError, match="OBCA.*switch_adjoint|switch_adjoint.*OBCA"):
        default.run_tape(c["x_init"], c["T"])
    with pytest.raises(ValueError, match="switch_adjoint"):
        DifferentiableClosedLoop(default)
    loop, out, got = _run()
    GS, GU = _t(c["GS"]), _t(c["GU"])
    with pytest.raises(ValueError, match="model=True"):
        loop.backward(out["tape"], GS, GU, model=True)
    with pytest.raises(ValueError, match="rule"):
        loop.backward(out["tape"], GS, GU, rule=True)
    with pytest.raises(ValueError, match="run_graph"):
        loop.run_graph(c["x_init"], c["T"])
    with pytest.raises(ValueError, match="fuzzy_rule"):
        _loop(switch_adjoint=True, fuzzy_rule=sim.FuzzyRule()).run_tape(c["x_init"], c["T"])
    layer = DifferentiableClosedLoop(loop)
    x = _t(c["x_init"]).requires_grad_(True)
    S, Ua, st = layer(x, c["T"])
    ((GS * S).sum() + (GU * Ua).sum()).backward()
    assert np.array_equal(_n(x.grad), got["x_init"])
    assert isinstance(x.grad, torch.Tensor)
