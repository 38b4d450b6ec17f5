"""GPU suite: the adjoint of the LQR terminal score (lqr_vjp_kernel, tt_lqr_score_vjp_device, lqr.lqr_scores_vjp) and
the autograd layer on it (ttmpc.diff.DifferentiableLqrScore).

1. The kernel against lqr_vjp_reference.dense_lqr_vjp at the GPU forward's own P (the DARE's conditioning stays out).
2. Grid edges, optional outputs, optional upstream gradients, determinism.
3. Status: a skipped instance, a NaN upstream gradient; the neighbours are untouched.
4. Rejected calls.
5. Autograd: the layer is the vjp call.
6. Composition with the differentiable closed loop: a directional check on the device.

Inputs of 1 to 5: the goals of test_gpu_lqr.py (seed 9, B = 96), Q = I + 0.1 diag(0..5), R = [[10, 1], [1, 8]].
Tolerance of 1, per instance and group, relative to the group's largest reference entry: max(1e-12, eps cond(I - Ac (x)
Ac)), the forward-error bound of the Lyapunov solve both sides perform (eps = 2.2e-16).  Every case prints its figures
before it asserts (DESIGN.md "Adjoint of the LQR score" records them).
"""
import ctypes as C
import errno
import functools
import itertools

import numpy as np
import pytest

import loop_vjp_reference as lr
import lqr_vjp_reference as lv
import vjp_harness as h

pytestmark = pytest.mark.gpu

P6, Q, R = lv.P6, lv.Q_TEST, lv.R_TEST
EPS = 2.2e-16
B = 96
OUTS = ("g_x_cur", "g_x_goal", "g_Q", "g_R", "vjp_status", "doublings")
GRADS = OUTS[:4]


_t, _n, _golden = h.t, h.n, h.golden


@functools.lru_cache(maxsize=None)
def _fwd():
    """The forward once: host inputs, device inputs, and the forward's device outputs (score, P, doublings)."""
    from ttmpc import lqr
    xc, xg = lv.lqr_case(_golden())
    txc, txg = _t(xc), _t(xg)
    s, Pm, it = lqr.lqr_scores(txc, txg, P6, Q, R)
    assert np.all(_n(it) > 0)
    rng = np.random.default_rng(41)
    gs, GP = rng.uniform(-1, 1, B), rng.uniform(-1, 1, (B, 6, 6))      # GP is not symmetric
    return dict(xc=xc, xg=xg, txc=txc, txg=txg, P=Pm, it=it, gs=gs, GP=GP, tgs=_t(gs), tGP=_t(GP))


@functools.lru_cache(maxsize=None)
def _run(upstream):
    """The B = 96 vjp for upstream in ("score", "score+P", "P"), as numpy arrays."""
    from ttmpc import lqr
    f = _fwd()
    g = lqr.lqr_scores_vjp(f["txc"], f["txg"], P6, R, f["P"], grad_score=f["tgs"] if "score" in upstream else None,
                           grad_P=f["tGP"] if "P" in upstream else None, fwd_iters=f["it"])
    return {k: _n(v) for k, v in g.items()}


def _raw(nb, f, R_=R, gs=True, GP=True, it=True, want=OUTS, fill=7.0):
    """tt_lqr_score_vjp_device through ctypes on the first nb instances with any subset of outputs; the output tensors
    are pre-filled.  -> (return code, dict of numpy outputs)."""
    import torch
    import ttmpc
    from ttmpc._lib import TTLqrVjpOut
    from ttmpc.simulation import plant
    shapes = {"g_x_cur": (max(nb, 0), 6), "g_x_goal": (max(nb, 0), 6), "g_Q": (max(nb, 0), 6, 6),
              "g_R": (max(nb, 0), 2, 2), "vjp_status": (max(nb, 0),), "doublings": (max(nb, 0),)}
    outs = {k: torch.full(shapes[k], fill, dtype=torch.int32 if k in OUTS[4:] else torch.float64, device="cuda")
            for k in want}
    o = TTLqrVjpOut(*[outs[k].data_ptr() if k in outs else None for k in OUTS])
    p = plant(P6)
    r = np.ascontiguousarray(np.asarray(R_, dtype=np.float64).reshape(4))
    rc = ttmpc.lib().tt_lqr_score_vjp_device(nb, C.byref(p), r.ctypes.data_as(C.POINTER(C.c_double)),
                                             f["txc"].data_ptr(), f["txg"].data_ptr(), f["P"].data_ptr(),
                                             f["it"].data_ptr() if it else None, f["tgs"].data_ptr() if gs else None,
                                             f["tGP"].data_ptr() if GP else None, C.byref(o), None)
    torch.cuda.synchronize()
    return rc, {k: _n(v) for k, v in outs.items()}


# ---- 1 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("upstream", ["score", "score+P", "P"])
def test_kernel_against_dense_reference_at_the_forward_P(upstream):
    f, g = _fwd(), _run(upstream)
    Pm = _n(f["P"])
    assert np.all(g["vjp_status"] == 0) and np.all(g["doublings"] > 0)
    worst, where, worst_abs, conds = 0.0, None, {k: 0.0 for k in GRADS}, []
    for b in range(B):
        r = lv.dense_lqr_vjp(f["xc"][b], f["xg"][b], Pm[b], R, f["gs"][b] if "score" in upstream else 0.0,
                             f["GP"][b] if "P" in upstream else None, P6)
        tol = max(1e-12, EPS * r["cond"])
        conds.append(r["cond"])
        for k in GRADS:
            big = np.abs(r[k]).max()
            if big == 0.0:                       # x_cur gets nothing from an upstream on P alone: exact zeros
                assert not g[k][b].any(), (b, k)
                continue
            e = np.abs(g[k][b] - r[k]).max() / big
            if e / tol > worst:
                worst, where = e / tol, (b, k, f"cond {r['cond']:.1e}", f"v {f['xg'][b, 5]:.4f}")
            worst_abs[k] = max(worst_abs[k], e)
            assert e <= tol, (b, k, e, tol)
    print(f"{upstream}: worst error / bound {worst:.3e} at {where}; worst relative error per group "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst_abs.items())
          + f"; cond {min(conds):.1e} .. {max(conds):.1e}; doublings {g['doublings'].min()} .. {g['doublings'].max()}")
    assert np.array_equal(g["g_Q"], np.swapaxes(g["g_Q"], 1, 2))      # S is symmetrised: exactly symmetric


# ---- 2 ----------------------------------------------------------------------------------------------------------
def test_grid_edges_optional_pointers_and_determinism():
    f, full = _fwd(), _run("score+P")
    rc, again = _raw(B, f)
    assert rc == 0
    for k in OUTS:
        assert np.array_equal(again[k], full[k]), k                   # two launches: the same bits
    for nb in (1, 3):
        rc, g = _raw(nb, f)
        assert rc == 0
        for k in OUTS:
            assert np.array_equal(g[k], full[k][:nb]), (nb, k)
    # every subset of outputs leaves the others bitwise unchanged (B = 3 keeps the 64 launches small)
    for m in range(len(OUTS) + 1):
        for want in itertools.combinations(OUTS, m):
            rc, g = _raw(3, f, want=want)
            assert rc == 0 and set(g) == set(want)
            for k in want:
                assert np.array_equal(g[k], full[k][:3]), (want, k)
    # either upstream gradient alone
    for gs, GP, name in ((True, False, "score"), (False, True, "P")):
        rc, g = _raw(B, f, gs=gs, GP=GP)
        assert rc == 0
        for k in OUTS:
            assert np.array_equal(g[k], _run(name)[k]), (name, k)
    assert np.max(np.abs(_run("P")["g_Q"])) > 0.0 and not _run("P")["g_x_cur"].any()


# ---- 3 ----------------------------------------------------------------------------------------------------------
def test_status_skipped_and_undefined():
    import torch
    from ttmpc import lqr
    f, full = _fwd(), _run("score+P")
    it = f["it"].clone()
    it[5] = -1
    gs = f["tgs"].clone()
    gs[40] = float("nan")
    GP = f["tGP"].clone()
    GP[70, 2, 3] = float("inf")
    g = {k: _n(v) for k, v in lqr.lqr_scores_vjp(f["txc"], f["txg"], P6, R, f["P"], grad_score=gs, grad_P=GP,
                                                 fwd_iters=it).items()}
    torch.cuda.synchronize()
    expect = np.zeros(B, dtype=np.int32)
    expect[5], expect[40], expect[70] = 2, 1, 1
    assert np.array_equal(g["vjp_status"], expect)
    keep = expect == 0
    for k in GRADS:
        assert not g[k][~keep].any(), k
        assert np.array_equal(g[k][keep], full[k][keep]), k           # the neighbours: bitwise the undisturbed run
    assert g["doublings"][5] == 0 and np.array_equal(g["doublings"][keep], full["doublings"][keep])
    # without fwd_iters every instance is differentiated
    g2 = lqr.lqr_scores_vjp(f["txc"], f["txg"], P6, R, f["P"], grad_score=f["tgs"], grad_P=f["tGP"])
    for k in OUTS:
        assert np.array_equal(_n(g2[k]), full[k]), k


# ---- 4 ----------------------------------------------------------------------------------------------------------
def test_rejected_calls():
    import torch
    from ttmpc import TTError, lqr
    f = _fwd()
    bad = [_raw(3, f, R_=[[1.0, 2.0], [2.0, 4.0]]), _raw(3, f, gs=False, GP=False), _raw(-1, f)]
    for rc, g in bad:
        assert rc == -errno.EINVAL
        for k, v in g.items():
            assert np.all(v == 7), k                                   # nothing was launched
    rc, _ = _raw(0, f)
    assert rc == 0
    xc, xg, Pm, gs = f["txc"], f["txg"], f["P"], f["tgs"]
    with pytest.raises(TypeError):
        lqr.lqr_scores_vjp(xc.float(), xg, P6, R, Pm, grad_score=gs)
    with pytest.raises(TypeError):
        lqr.lqr_scores_vjp(xc, xg.cpu(), P6, R, Pm, grad_score=gs)
    with pytest.raises(TypeError):
        lqr.lqr_scores_vjp(xc, xg, P6, R, Pm, grad_score=gs, fwd_iters=f["it"].long())
    with pytest.raises(ValueError):
        lqr.lqr_scores_vjp(xc, xg[:5], P6, R, Pm, grad_score=gs)
    with pytest.raises(ValueError):
        lqr.lqr_scores_vjp(xc, xg, P6, R, Pm.reshape(B, 36), grad_score=gs)
    with pytest.raises(ValueError):
        lqr.lqr_scores_vjp(xc, xg, P6, R, Pm, grad_score=gs.reshape(B, 1))
    with pytest.raises(ValueError):
        lqr.lqr_scores_vjp(xc, xg, P6, R, Pm)
    with pytest.raises(ValueError):
        lqr.lqr_scores_vjp(xc, xg, P6, np.eye(3), Pm, grad_score=gs)
    with pytest.raises(TTError):
        lqr.lqr_scores_vjp(xc, xg, P6, [[1.0, 2.0], [2.0, 4.0]], Pm, grad_score=gs)
    empty = lqr.lqr_scores_vjp(xc[:0], xg[:0], P6, R, Pm[:0], grad_score=gs[:0])
    assert tuple(empty["g_Q"].shape) == (0, 6, 6)
    torch.cuda.synchronize()


# ---- 5 ----------------------------------------------------------------------------------------------------------
def test_autograd_is_the_vjp_call():
    import torch
    from ttmpc.diff import DifferentiableLqrScore
    f, full = _fwd(), _run("score+P")
    layer = DifferentiableLqrScore(P6)
    xc, xg = f["txc"].clone().requires_grad_(True), f["txg"].clone().requires_grad_(True)
    tQ, tR = _t(Q).requires_grad_(True), _t(R).requires_grad_(True)
    score, Pm, it = layer(xc, xg, tQ, tR)
    assert not it.requires_grad and it.dtype == torch.int32
    assert torch.equal(Pm, f["P"]) and torch.equal(it, f["it"])       # the forward is lqr_scores
    ((f["tgs"] * score).sum() + (f["tGP"] * Pm).sum()).backward()
    assert np.array_equal(_n(xc.grad), full["g_x_cur"]) and np.array_equal(_n(xg.grad), full["g_x_goal"])
    assert np.array_equal(_n(tQ.grad), _n(_t(full["g_Q"]).sum(dim=0)))
    assert np.array_equal(_n(tR.grad), _n(_t(full["g_R"]).sum(dim=0)))
    assert tQ.grad.is_cuda and tQ.grad.dtype == torch.float64
    # the score alone, a host Q and a float32 device R (its entries are exact in float32): gradients only where asked,
    # on the device and in the dtype of the tensor given
    hQ = torch.as_tensor(Q, dtype=torch.float64).requires_grad_(True)
    R32 = _t(R, torch.float32).requires_grad_(True)
    xc2, xg2 = f["txc"].clone().requires_grad_(True), f["txg"].clone()
    score, _, _ = layer(xc2, xg2, hQ, R32)
    (f["tgs"] * score).sum().backward()
    one = _run("score")
    assert np.array_equal(_n(xc2.grad), one["g_x_cur"]) and xg2.grad is None
    assert not hQ.grad.is_cuda and hQ.grad.dtype == torch.float64
    assert np.array_equal(_n(hQ.grad), _n(_t(one["g_Q"]).sum(dim=0)))
    assert R32.grad.is_cuda and R32.grad.dtype == torch.float32
    assert np.array_equal(_n(R32.grad), _n(_t(one["g_R"]).sum(dim=0).float()))


# ---- 6 ----------------------------------------------------------------------------------------------------------
def _loop_inputs(N, nb):
    """(6, 3): loop_vjp_reference.loop_case, the case of test_gpu_loop_vjp.py.  Otherwise the same recipe at horizon N
    with nb instances: the plan is columns 150 .. 150 + N + 2 of the interpolated golden plan (Np = N + 2, end padding
    from k = 3), T_sim = 0.25 (K = 6 steps), weights U(0.7, 1.4)."""
    from oracle import ttmpc_oracle as to
    g = _golden()
    if (N, nb) == (6, 3):
        c = lr.loop_case(g)
        return c["nlp"], c["plan_x"], c["plan_u"], c["x_init"], c["w"], c["T"]
    S, U = to.do_interpolation(g["state_traj"], g["input_traj"], 0.1, 0.05)
    plan_x, plan_u = S[:, 150:150 + N + 3].copy(), U[:, 150:150 + N + 2].copy()
    rng = np.random.default_rng(5)
    x_init = plan_x[:, 0][None] + rng.normal(scale=[0.1, 0.1, 0.01, 0.01, 0.0, 0.0], size=(nb, 6))
    w = rng.uniform(0.7, 1.4, (nb, 8))
    return to.TrackingNLP(N, params=dict(lr.P, horizon=N)), plan_x, plan_u, x_init, w, 0.25


@pytest.mark.parametrize("N,nb", [(6, 3), (20, 4)])
def test_composition_with_the_closed_loop(N, nb):
    """L = sum_b score_b of S[-1] against the plan's last row, TT_VARIANT_TRACK, no noise.  dL/dwq_wr along one random
    direction against a central difference of the rerun loop, with the step and the tolerance of the directional check
    of test_gpu_loop_vjp.py (eps = 1e-3, 1e-3 relative).  (6, 3) is that file's own case; (20, 4) its recipe at N = 20
    with B = 4."""
    import torch
    import ttmpc
    from ttmpc import simulation as sim
    from ttmpc.diff import DifferentiableClosedLoop, DifferentiableLqrScore
    nlp, plan_x, plan_u, x_init, w, T = _loop_inputs(N, nb)
    loop = sim.ClosedLoop(h.solver(nlp), plan_x, plan_u, lr.P, lr.DIST, measurement_noise=False, policy="track")
    layer, score_layer = DifferentiableClosedLoop(loop), DifferentiableLqrScore(lr.P)
    px0, pu0 = _t(plan_x.T[None]), _t(plan_u.T[None])

    def loss(tw, px, pu, tx, detach_goal=False):
        S, Ua, st = layer(tx, T, wq_wr=tw, plan_x=px, plan_u=pu)
        assert torch.all(st == 0)
        goal = px[:, -1].expand(nb, 6)
        score, _, it = score_layer(S[-1], goal.detach() if detach_goal else goal, Q, R)
        assert torch.all(it > 0)
        return score.sum()

    grads = []
    for detach in (False, True):
        tw, tx = _t(w).requires_grad_(True), _t(x_init).requires_grad_(True)
        px, pu = px0.clone().requires_grad_(True), pu0.clone().requires_grad_(True)
        L0 = loss(tw, px, pu, tx, detach)
        L0.backward()
        grads.append({k: _n(v.grad) for k, v in (("w", tw), ("x_init", tx), ("plan_x", px), ("plan_u", pu))})
        L0 = float(L0.detach())
    g, gd = grads
    for k, v in g.items():
        assert np.all(np.isfinite(v)) and np.max(np.abs(v)) > 0.0, k
    d = np.random.default_rng(43).normal(size=w.shape)
    d /= np.linalg.norm(d)
    eps, Ls = 1e-3, []
    with torch.no_grad():
        for sgn in (1.0, -1.0):
            Ls.append(float(loss(_t(w + sgn * eps * d), px0, pu0, _t(x_init))))
    fd, an = (Ls[0] - Ls[1]) / (2 * eps), float(np.sum(g["w"] * d))
    direct = g["plan_x"][0, -1] - gd["plan_x"][0, -1]
    print(f"N={N} B={nb}: L {L0:.6e}; dL/dw along d: finite difference {fd:.6e}, g_w . d {an:.6e}, relative "
          f"{abs(fd - an) / abs(an):.3e}; |g_w| {np.linalg.norm(g['w']):.3e}; direct x_goal term in g_plan_x[-1] "
          f"{direct}, with the goal detached {gd['plan_x'][0, -1]}")
    assert abs(fd - an) <= 1e-3 * abs(an)
    assert np.max(np.abs(direct)) > 0.0                               # the direct x_goal term reached the plan's last row
    assert np.array_equal(g["w"], gd["w"]) and np.array_equal(g["x_init"], gd["x_init"])
