"""GPU suite: the adjoint of the tracking solve (tt_track_vjp*, track_vjp_kernel) and the autograd layer on it.

1. The kernel against dense algebra on the GPU's own duals, with the numpy recursion as the yardstick: the default
   problem, then every weight form and bound pattern of tests/track_patterns.py, group by group; an asymmetric Q, R
   against its symmetric part, bit for bit.
2. The horizons at which the kernel takes another path, and grid indexing.
3. dL/dx_init against the forward sensitivities of track_sens_kernel.
4. All four gradients against central finite differences of the CPU oracle.
5. Status plumbing: failed instances, a NaN upstream gradient, NULL gradients, OBCA handles.
6. ttmpc.diff: autograd through the solve, streams, gradient descent on the weights.

Every case prints its figures before it asserts (DESIGN.md "Adjoint of a tracking solve" records them).
"""
import functools

import numpy as np
import pytest

import sens_reference as sr
import vjp_harness as h
import vjp_reference as vr
from track_patterns import DERIVATIVE_CASES

pytestmark = pytest.mark.gpu

P = sr.P
_solver, _w = h.solver, h.w_of


def _gpu(v, b):
    return {"x0": v.g_x0[b], "xref": v.g_xref[b], "uref": v.g_uref[b], "w": v.g_wq_wr[b]}


@functools.lru_cache(maxsize=None)
def _case_run(name, weighted, pattern="mpc_diag"):
    """solve_ex with every output and one adjoint call on one of the two checked input sets, shared by cases 1, 3, 4."""
    nlp, x0, xr, ur = sr.case(name, pattern)
    B = x0.shape[0]
    w = vr.random_weights(B) if weighted else None
    s = _solver(nlp)
    r = s.solve_ex(x0, xr, ur, wq_wr=w, duals=True, gain=True, trajectory_sens=True)
    gX, gU = vr.random_upstream(B, nlp.N)
    v = s.vjp(r.X, r.U, r.dual, xr, ur, r.status, gX, gU, wq_wr=w)
    return nlp, x0, xr, ur, w, s, r, gX, gU, v


@functools.lru_cache(maxsize=None)
def _references(name, weighted):
    """dense_vjp and riccati_vjp of every instance of a case at the GPU's own primal-dual point."""
    from ttmpc import layout
    nlp, x0, xr, ur, w, s, r, gX, gU, v = _case_run(name, weighted)
    zz = layout.pack(r.X, r.U)
    dense, model = [], []
    for b in range(x0.shape[0]):
        dense.append(vr.dense_vjp(nlp, zz[b], r.dual[b], xr[b], ur[b], gX[b], gU[b], *_w(w, b)))
        model.append(vr.riccati_vjp(nlp, zz[b], r.dual[b], xr[b], ur[b], gX[b], gU[b], *_w(w, b)))
    return zz, dense, model


# ---- 1 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", ["free", "active"])
def test_kernel_against_dense_algebra(name, weighted):
    nlp, x0, xr, ur, w, s, r, gX, gU, v = _case_run(name, weighted)
    zz, dense, model = _references(name, weighted)
    assert np.all(r.status == 0) and np.all(v.vjp_status == 0)
    err_gpu = err_model = smax = 0.0
    nact = []
    for b in range(x0.shape[0]):
        assert model[b]["ok"]
        err_gpu = max(err_gpu, vr.max_err(_gpu(v, b), dense[b]))
        err_model = max(err_model, vr.max_err(model[b], dense[b]))
        smax = max(smax, vr.max_abs(dense[b]))
        act = sr.active_set(nlp, zz[b])
        nact.append(int(act[act >= 6].size))
        assert not v.g_xref[b, 0].any()  # x_0 is pinned
    print(f"{name} weighted={weighted}: err_gpu {err_gpu:.3e}, err_model {err_model:.3e}, max|grad_dense| {smax:.3e}, "
          f"active {nact}")
    if name == "free":
        assert max(nact) == 0
    else:
        assert min(nact) >= 13
    assert err_gpu <= 10.0 * err_model + 1e-12 * smax


@pytest.mark.parametrize("name,pattern,weighted", DERIVATIVE_CASES)
def test_kernel_against_dense_algebra_patterns(name, pattern, weighted):
    """Group by group, so that the weight gradient's cross terms (non-diagonal Q, R) cannot hide behind a larger group."""
    from ttmpc import layout
    nlp, x0, xr, ur, w, s, r, gX, gU, v = _case_run(name, weighted, pattern)
    assert np.all(r.status == 0) and np.all(v.vjp_status == 0)
    zz = layout.pack(r.X, r.U)
    e_gpu, e_model, big = ({k: 0.0 for k in vr.KEYS} for _ in range(3))
    nact = []
    for b in range(x0.shape[0]):
        dense = vr.dense_vjp(nlp, zz[b], r.dual[b], xr[b], ur[b], gX[b], gU[b], *_w(w, b), cond=False)
        model = vr.riccati_vjp(nlp, zz[b], r.dual[b], xr[b], ur[b], gX[b], gU[b], *_w(w, b))
        assert model["ok"]
        g = _gpu(v, b)
        for k in vr.KEYS:
            e_gpu[k] = max(e_gpu[k], float(np.max(np.abs(g[k] - dense[k]))))
            e_model[k] = max(e_model[k], float(np.max(np.abs(model[k] - dense[k]))))
            big[k] = max(big[k], float(np.max(np.abs(dense[k]))))
        act = sr.active_set(nlp, zz[b])
        nact.append(int(act[act >= 6].size))
        assert not v.g_xref[b, 0].any()  # x_0 is pinned
    for k in vr.KEYS:
        print(f"{name} {pattern} weighted={weighted} {k:5s}: err_gpu {e_gpu[k]:.3e}, err_model {e_model[k]:.3e}, "
              f"max|ref| {big[k]:.3e}")
    print(f"{name} {pattern} weighted={weighted}: active {nact}")
    assert (max(nact) == 0) if name == "free" else (min(nact) >= 13)
    for k in vr.KEYS:
        assert big[k] > 1e-3, k
        assert e_gpu[k] <= 10.0 * e_model[k] + 1e-12 * big[k], k


@pytest.mark.parametrize("name", ["free", "active"])
def test_asymmetric_weights_are_their_symmetric_part(name):
    """``mpc_asym`` has dyadic off-diagonals whose mean is ``mpc_full`` exactly: every kernel symmetrises on its own, so
    a handle built with either returns the same bits from the solve, the export, the sensitivities and the adjoints."""
    runs = []
    for pattern in ("mpc_full", "mpc_asym"):
        nlp, x0, xr, ur = sr.case(name, pattern)
        B = x0.shape[0]
        w = vr.random_weights(B)
        s = _solver(nlp)
        r = s.solve_ex(x0, xr, ur, wq_wr=w, duals=True, gain=True, trajectory_sens=True)
        gX, gU = vr.random_upstream(B, nlp.N)
        v = s.vjp(r.X, r.U, r.dual, xr, ur, r.status, gX, gU, wq_wr=w, model=True)
        assert np.all(r.status == 0) and np.all(r.sens_status == 0) and np.all(v.vjp_status == 0)
        runs.append((nlp, r, v))
    (nf, rf, vf), (na, ra, va) = runs
    assert not np.array_equal(nf.Q, na.Q) and np.array_equal(nf.Q, 0.5 * (na.Q + na.Q.T))
    assert not np.array_equal(nf.R, na.R) and np.array_equal(nf.R, 0.5 * (na.R + na.R.T))
    for k in ("X", "U", "status", "iters", "kkt", "dual", "gain", "dXdx0", "dUdx0", "sens_status"):
        assert np.array_equal(getattr(rf, k), getattr(ra, k)), k
    for k in ("g_x0", "g_xref", "g_uref", "g_wq_wr", "g_model", "vjp_status"):
        assert np.array_equal(getattr(vf, k), getattr(va, k)), k
    assert np.max(np.abs(vf.g_wq_wr)) > 1e-3 and np.max(np.abs(vf.g_model)) > 1e-3


# ---- 2 ----------------------------------------------------------------------------------------------------------
def _max_horizon():
    import ttmpc
    return int(ttmpc.lib().tt_max_horizon())


@functools.lru_cache(maxsize=None)
def _horizon_run(N):
    from oracle import ttmpc_oracle as to
    from ttmpc.scenarios import synthetic_batch
    nlp = to.TrackingNLP(N, params=dict(P, horizon=N))
    x0, xr, ur = synthetic_batch(4, N, seed=4000 + N, psi_range=0.3)
    s = _solver(nlp, tol=1e-8)
    r = s.solve_ex(x0, xr, ur, duals=True, gain=False)
    gX, gU = vr.random_upstream(4, N, seed=N)
    v = s.vjp(r.X, r.U, r.dual, xr, ur, r.status, gX, gU)
    return nlp, x0, xr, ur, s, r, gX, gU, v


@pytest.mark.parametrize("N", [1, 2, 20, 63, 64, "max"])
def test_horizons(N):
    from ttmpc import layout
    N = _max_horizon() if N == "max" else N
    nlp, x0, xr, ur, s, r, gX, gU, v = _horizon_run(N)
    zz = layout.pack(r.X, r.U)
    ok = np.flatnonzero(r.status <= 1)
    print(f"N={N}: status {r.status.tolist()}, vjp_status {v.vjp_status.tolist()}")
    assert ok.size >= 3
    err_gpu = err_model = smax = 0.0
    for b in range(4):
        if r.status[b] > 1:
            assert v.vjp_status[b] == 2 and not any(a.any() for a in _gpu(v, b).values())
            continue
        assert v.vjp_status[b] == 0
        dense = vr.dense_vjp(nlp, zz[b], r.dual[b], xr[b], ur[b], gX[b], gU[b], cond=False)
        model = vr.riccati_vjp(nlp, zz[b], r.dual[b], xr[b], ur[b], gX[b], gU[b])
        assert model["ok"]
        err_gpu = max(err_gpu, vr.max_err(_gpu(v, b), model))
        err_model = max(err_model, vr.max_err(model, dense))
        smax = max(smax, vr.max_abs(model))
        assert not v.g_xref[b, 0].any()
    print(f"N={N}: gpu vs riccati_vjp {err_gpu:.3e}, riccati_vjp vs dense {err_model:.3e}, max|grad| {smax:.3e}")
    assert smax > 1e-3
    assert err_gpu <= 10.0 * err_model + 1e-12 * smax


def test_grid_indexing():
    """One B = 2304 launch on 576 copies of the N = 20 batch: every block finds its own instance."""
    nlp, x0, xr, ur, s, r, gX, gU, v = _horizon_run(20)
    rep = lambda a: np.tile(a, (576,) + (1,) * (a.ndim - 1))  # noqa: E731
    big = s.vjp(rep(r.X), rep(r.U), rep(r.dual), rep(xr), rep(ur), rep(r.status), rep(gX), rep(gU))
    for k in ("g_x0", "g_xref", "g_uref", "g_wq_wr", "vjp_status"):
        got, ref = getattr(big, k), getattr(v, k)
        assert got.shape[0] == 2304
        assert np.array_equal(got[:4], ref), k
        assert np.array_equal(got, rep(ref)), k


# ---- 3 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["free", "active"])
def test_x0_gradient_against_forward_sensitivities(name):
    nlp, x0, xr, ur, w, s, r, gX, gU, v = _case_run(name, False)
    zz, dense, model = _references(name, False)
    assert np.all(r.sens_status == 0) and np.all(v.vjp_status == 0)
    err = err_model = smax = 0.0
    for b in range(x0.shape[0]):
        fwd = np.einsum("kij,ki->j", r.dXdx0[b], gX[b]) + np.einsum("kij,ki->j", r.dUdx0[b], gU[b])
        ms = sr.riccati_sensitivity(nlp, zz[b], r.dual[b])
        fwd_model = np.einsum("kij,ki->j", ms["dXdx0"], gX[b]) + np.einsum("kij,ki->j", ms["dUdx0"], gU[b])
        ref = dense[b]["x0"]
        err = max(err, float(np.max(np.abs(v.g_x0[b] - fwd))))
        err_model = max(err_model, float(np.max(np.abs(model[b]["x0"] - ref))), float(np.max(np.abs(fwd_model - ref))))
        smax = max(smax, float(np.max(np.abs(ref))))
    print(f"{name}: adjoint vs forward dL/dx_init {err:.3e}, err_model {err_model:.3e}, max|ref| {smax:.3e}")
    assert smax > 1e-3
    assert err <= 10.0 * err_model + 1e-12 * smax


# ---- 4 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_against_oracle_finite_differences(weighted):
    nlp, x0, xr, ur, w, s, r, gX, gU, v = _case_run("free", weighted)
    z, st, fd = vr.oracle_fd_vjp(nlp, x0, xr, ur, gX, gU, w=w, h=1e-4)
    assert np.all(st == 0) and np.all(r.status == 0) and np.all(v.vjp_status == 0)
    worst = {k: 0.0 for k in vr.KEYS}
    big = {k: 0.0 for k in vr.KEYS}
    for b in range(x0.shape[0]):
        g = _gpu(v, b)
        for k in vr.KEYS:
            worst[k] = max(worst[k], float(np.max(np.abs(g[k] - fd[b][k]))))
            big[k] = max(big[k], float(np.max(np.abs(g[k]))))
    print(f"weighted={weighted}: gpu vs oracle FD {worst}, largest entries {big}")
    assert max(worst.values()) <= 1e-5
    assert min(big.values()) > 1e-3


def test_against_oracle_finite_differences_full_weights():
    """The non-diagonal ``mpc_full`` weights, weighted, at the bound of the cases above (the CPU references reach
    2.4e-9 there, tests/test_vjp_reference.py)."""
    nlp, x0, xr, ur, w, s, r, gX, gU, v = _case_run("free", True, "mpc_full")
    z, st, fd = vr.oracle_fd_vjp(nlp, x0, xr, ur, gX, gU, w=w, h=1e-4)
    assert np.all(st == 0) and np.all(r.status == 0) and np.all(v.vjp_status == 0)
    worst = {k: 0.0 for k in vr.KEYS}
    big = {k: 0.0 for k in vr.KEYS}
    for b in range(x0.shape[0]):
        g = _gpu(v, b)
        for k in vr.KEYS:
            worst[k] = max(worst[k], float(np.max(np.abs(g[k] - fd[b][k]))))
            big[k] = max(big[k], float(np.max(np.abs(g[k]))))
    print(f"mpc_full weighted: gpu vs oracle FD {worst}, largest entries {big}")
    assert max(worst.values()) <= 1e-5
    assert min(big.values()) > 1e-3


# ---- 5 ----------------------------------------------------------------------------------------------------------
def test_status_plumbing():
    from oracle import ttmpc_oracle as to
    from ttmpc.scenarios import synthetic_batch
    N = 12
    nlp = to.TrackingNLP(N, params=dict(P, horizon=N))
    x0, xr, ur = synthetic_batch(5, N, seed=8)
    s = _solver(nlp)
    gX, gU = vr.random_upstream(5, N)
    keys = ("g_x0", "g_xref", "g_uref", "g_wq_wr")
    good = s.solve_ex(x0, xr, ur, gain=False)
    vg = s.vjp(good.X, good.U, good.dual, xr, ur, good.status, gX, gU)
    assert list(good.status) == [0] * 5 and list(vg.vjp_status) == [0] * 5
    x0b = x0.copy()
    x0b[1, 3] = 1.3            # hitch angle beyond pi/3
    x0b[3, 2] = 4.0            # heading beyond pi
    r = s.solve_ex(x0b, xr, ur, gain=False)
    v = s.vjp(r.X, r.U, r.dual, xr, ur, r.status, gX, gU)
    assert list(r.status) == [0, 3, 0, 3, 0]
    assert list(v.vjp_status) == [0, 2, 0, 2, 0]
    for b in (1, 3):
        assert not any(getattr(v, k)[b].any() for k in keys)
    for b in (0, 2, 4):  # the neighbours are what they were in the all-feasible batch
        for k in keys:
            assert np.array_equal(getattr(v, k)[b], getattr(vg, k)[b]), (b, k)
        assert np.max(np.abs(v.g_x0[b])) > 0.0
    # a NaN in one instance's upstream gradient: that instance alone is undefined
    gXn = gX.copy()
    gXn[2, 5, 1] = np.nan
    vn = s.vjp(good.X, good.U, good.dual, xr, ur, good.status, gXn, gU)
    assert list(vn.vjp_status) == [0, 0, 1, 0, 0]
    assert not any(getattr(vn, k)[2].any() for k in keys)
    for b in (0, 1, 3, 4):
        for k in keys:
            assert np.array_equal(getattr(vn, k)[b], getattr(vg, k)[b]), (b, k)
    # NULL grad_u is an array of zeros
    v0 = s.vjp(good.X, good.U, good.dual, xr, ur, good.status, gX, np.zeros_like(gU))
    vnull = s.vjp(good.X, good.U, good.dual, xr, ur, good.status, gX, None)
    for k in keys + ("vjp_status",):
        assert np.array_equal(getattr(v0, k), getattr(vnull, k)), k
    assert np.max(np.abs(vnull.g_x0)) > 0.0


def test_bad_calls_are_rejected():
    import ctypes as C
    import errno

    import ttmpc
    from oracle import ttmpc_oracle as to
    from ttmpc._lib import TTError, TTTrackVjpOut
    N = 10
    out = TTTrackVjpOut(None, None, None, None, None)
    o = ttmpc.ObcaSolver(N, P, to.DEFAULT_Q, to.DEFAULT_R, to.OBCA_XLB, to.OBCA_XUB, to.MPC_ULB, to.MPC_UUB,
                         np.array([[30.0, 30.0, 4.0, 4.0]]), variant=ttmpc.TT_VARIANT_TRACK_OBCA)
    assert o._L.tt_track_vjp_device(o._h, 1, None, None, None, None, None, None, None, None, None, C.byref(out),
                                    None) == -errno.EINVAL
    assert o._L.tt_track_vjp(o._h, 1, None, None, None, None, None, None, None, None, None,
                             C.byref(out)) == -errno.EINVAL
    nlp = to.TrackingNLP(N, params=dict(P, horizon=N))
    s = _solver(nlp)
    z = np.zeros
    with pytest.raises(TTError, match="both NULL"):
        s.vjp(z((1, N + 1, 6)), z((1, N, 2)), z((1, N + 1, 22)), z((1, N + 1, 6)), z((1, N, 2)), z(1, dtype=np.int32),
              None, None)
    assert s._L.tt_track_vjp_device(s._h, 1, 8, 8, 8, 8, 8, None, 8, None, None, C.byref(out), None) == -errno.EINVAL


# ---- 6 ----------------------------------------------------------------------------------------------------------
def _layer_inputs(requires=(True, True, True, True)):
    import torch
    nlp, x0, xr, ur = sr.case_free()
    w = vr.random_weights(x0.shape[0])
    dev = torch.device("cuda")
    ts = [torch.from_numpy(np.ascontiguousarray(a)).to(dev).requires_grad_(q) for a, q in zip((x0, xr, ur, w), requires)]
    return nlp, (x0, xr, ur, w), ts


def test_autograd_is_the_adjoint_call():
    import torch
    from ttmpc.diff import DifferentiableTracking
    nlp, (x0, xr, ur, w), ts = _layer_inputs()
    B, N = x0.shape[0], nlp.N
    s = _solver(nlp)
    layer = DifferentiableTracking(s)
    dev = ts[0].device
    gX, gU = (torch.from_numpy(a).to(dev) for a in vr.random_upstream(B, N))

    def grads(inputs):
        X, U, st = layer(*inputs)
        assert not st.requires_grad and st.dtype == torch.int32
        saved = [t.clone() for t in X.grad_fn.saved_tensors]
        loss = (gX * X).sum() + (gU * U).sum()
        return torch.autograd.grad(loss, inputs), saved, st

    g, saved, st = grads(ts)
    Xs, Us, dual, status, xrs, urs, ws = saved
    assert torch.all(st == 0)
    outs = [torch.full(s_, np.nan, dtype=torch.float64, device=dev) for s_ in ((B, 6), (B, N + 1, 6), (B, N, 2), (B, 8))]
    vst = torch.full((B,), -1, dtype=torch.int32, device=dev)
    s.vjp_device(B, Xs.data_ptr(), Us.data_ptr(), dual.data_ptr(), xrs.data_ptr(), urs.data_ptr(), status.data_ptr(),
                 grad_x=gX.data_ptr(), grad_u=gU.data_ptr(), g_x0=outs[0].data_ptr(), g_xref=outs[1].data_ptr(),
                 g_uref=outs[2].data_ptr(), g_wq_wr=outs[3].data_ptr(), vjp_status=vst.data_ptr(),
                 wq_wr=ws.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.all(vst == 0)
    for a, b in zip(g, outs):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
        assert float(a.abs().max()) > 1e-3
    # forward and backward on another stream: the same bits
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g2, _, _ = grads(_layer_inputs()[2])
    side.synchronize()
    for a, b in zip(g, g2):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    # inputs that do not ask for a gradient get none
    _, _, ts2 = _layer_inputs(requires=(True, False, False, True))
    X, U, _ = layer(*ts2)
    ((gX * X).sum() + (gU * U).sum()).backward()
    assert ts2[1].grad is None and ts2[2].grad is None
    assert np.array_equal(ts2[0].grad.cpu().numpy(), g[0].cpu().numpy())
    assert np.array_equal(ts2[3].grad.cpu().numpy(), g[3].cpu().numpy())


def test_first_input_loss_gives_the_gain():
    import torch
    from ttmpc import layout
    from ttmpc.diff import DifferentiableTracking
    nlp, (x0, xr, ur, w), ts = _layer_inputs(requires=(True, False, False, False))
    B, N = x0.shape[0], nlp.N
    s = _solver(nlp)
    r = s.solve_ex(x0, xr, ur, wq_wr=w, duals=True, gain=True)
    c = np.random.default_rng(5).uniform(-1.0, 1.0, (B, 2))
    X, U, st = DifferentiableTracking(s)(*ts)
    (torch.from_numpy(c).to(U.device) * U[:, 0]).sum().backward()
    g = ts[0].grad.cpu().numpy()
    assert np.array_equal(U.detach().cpu().numpy(), r.U)
    zz = layout.pack(r.X, r.U)
    gU = np.zeros((B, N, 2))
    gU[:, 0] = c
    err = err_model = smax = 0.0
    for b in range(B):
        args = (nlp, zz[b], r.dual[b], xr[b], ur[b], np.zeros((N + 1, 6)), gU[b], w[b, :6], w[b, 6:])
        dense, model = vr.dense_vjp(*args), vr.riccati_vjp(*args)
        err = max(err, float(np.max(np.abs(g[b] - r.gain[b].T @ c[b]))))
        err_model = max(err_model, float(np.max(np.abs(model["x0"] - dense["x0"]))))
        smax = max(smax, float(np.max(np.abs(dense["x0"]))))
    print(f"dL/dx0 vs gain' c: {err:.3e}, err_model {err_model:.3e}, max|ref| {smax:.3e}")
    assert smax > 1e-3
    assert err <= 10.0 * err_model + 1e-12 * smax


def _descend(target_w, lr, steps=10):
    """Gradient descent on wq_wr from ones towards the trajectories of target_w; the loss before every step and after
    the last."""
    import torch
    from ttmpc.diff import DifferentiableTracking
    nlp, (x0, xr, ur, _), ts = _layer_inputs(requires=(False, False, False, False))
    B = x0.shape[0]
    layer = DifferentiableTracking(_solver(nlp))
    dev = ts[0].device
    with torch.no_grad():
        Xt, _, st = layer(ts[0], ts[1], ts[2], torch.from_numpy(target_w).to(dev))
    assert torch.all(st == 0)
    w = torch.ones((B, 8), dtype=torch.float64, device=dev, requires_grad=True)
    seq = []
    for _ in range(steps + 1):
        X, _, st = layer(ts[0], ts[1], ts[2], w)
        assert torch.all(st == 0)
        loss = ((X - Xt) ** 2).mean()
        seq.append(float(loss.detach()))
        (g,) = torch.autograd.grad(loss, [w])
        with torch.no_grad():
            w -= lr * g
    return seq


def test_gradient_descent_on_the_weights():
    """Ten steps from ones towards the trajectories of wq = 1.2, wr = 1 (B = 8, N = 8), fixed step 1e5 (the loss is a
    mean over 432 entries, so its gradient is small; the CPU oracle's descent is monotone up to 3e5 and not at 1e6)."""
    tw = np.concatenate([1.2 * np.ones((8, 6)), np.ones((8, 2))], axis=1)
    seq = _descend(tw, 1e5)
    print("loss sequence (target wq 1.2, wr 1):", " ".join(f"{v:.4e}" for v in seq))
    assert all(b < a for a, b in zip(seq, seq[1:]))
    assert seq[-1] < 0.5 * seq[0]


def test_gradient_descent_towards_uniformly_scaled_weights():
    """The same with the target solved at 1.2 * ones in all eight weights.  Scaling every weight by one factor scales
    the whole objective and leaves the optimum where it is, so the target trajectories are those of the start up to the
    solver's tolerance: the loss starts at 5.2e-25 (MI355X and CPU oracle alike) and the descent has only that residue
    to work on (5.1975e-25 -> 5.1568e-25 in ten steps on an MI355X).  The test above is the one with a distance to
    cover."""
    seq = _descend(1.2 * np.ones((8, 8)), 1e5)
    print("loss sequence (target 1.2 * ones):", " ".join(f"{v:.4e}" for v in seq))
    assert all(b < a for a, b in zip(seq, seq[1:]))
