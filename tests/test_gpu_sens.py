"""GPU suite: multiplier export and x_init sensitivities of the tracking solve (tt_solve_batch_ex, track_sens_kernel).

1. solve_ex returns bitwise the plain outputs of solve, for every build of track_kernel.
2. The exported duals are the multipliers: signs, zeros, and IPOPT's own stopping test re-evaluated in numpy.
3. The sensitivity kernel against dense algebra on the same duals, with the numpy Riccati as the yardstick: the two
   checked input sets under every weight form and bound pattern of tests/track_patterns.py, weighted and not; the
   horizons at which the pre-pass wraps its lanes and the longest one; grid indexing; the device calls with weights.
4. The gain against central finite differences of the CPU oracle.
5. Status plumbing: failed instances, undefined sensitivities (sens_status 1), OBCA handles.
6. MPCTrackingControl.solve_with_gain.

Every case prints its figures before it asserts (DESIGN.md "Multiplier export and x_init sensitivities" records them).
"""
import functools

import numpy as np
import pytest

import sens_reference as sr
import vjp_reference as vr
from track_patterns import DERIVATIVE_CASES

pytestmark = pytest.mark.gpu

P = sr.P
SHAPES = [(8, 64), (20, 256), (20, 2304), (40, 128), (50, 832), (63, 64), (64, 64)]


def _solver(nlp, **kw):
    import ttmpc
    return ttmpc.BatchSolver(nlp.N, P, nlp.Q, nlp.R, nlp.xlb, nlp.xub, nlp.ulb, nlp.uub, **kw)


@functools.lru_cache(maxsize=None)
def _shape_run(N, B):
    """One plain and one extended solve of a synthetic batch, shared by cases 1 and 2."""
    from oracle import ttmpc_oracle as to
    from ttmpc.scenarios import synthetic_batch
    nlp = to.TrackingNLP(N, params=dict(P, horizon=N))
    x0, xr, ur = synthetic_batch(B, N, seed=4000 + N, psi_range=0.3)
    s = _solver(nlp, tol=1e-8)
    plain = s.solve(x0, xr, ur)
    ex = s.solve_ex(x0, xr, ur, duals=True, gain=True, trajectory_sens=False)
    return nlp, x0, xr, ur, plain, ex


def _case_run(name, pattern="mpc_diag", weighted=False):
    """solve_ex with every output on one of the two checked input sets, shared by cases 3 and 4; with a pattern of
    tests/track_patterns.py and ``random_weights`` the weights come seventh."""
    out = _pattern_run(name, pattern, weighted)
    return out if weighted or pattern != "mpc_diag" else out[:6]


@functools.lru_cache(maxsize=None)
def _pattern_run(name, pattern, weighted):
    nlp, x0, xr, ur = sr.case(name, pattern)
    w = vr.random_weights(x0.shape[0]) if weighted else None
    s = _solver(nlp)
    r = s.solve_ex(x0, xr, ur, wq_wr=w, duals=True, gain=True, trajectory_sens=True)
    return nlp, x0, xr, ur, s, r, w


# ---- 1 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B", SHAPES)
def test_plain_results_unchanged(N, B):
    _, _, _, _, plain, ex = _shape_run(N, B)
    for a, b in zip(plain, (ex.X, ex.U, ex.status, ex.iters, ex.kkt)):
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
    assert ex.dual.shape == (B, N + 1, 22) and ex.gain.shape == (B, 2, 6) and ex.sens_status.shape == (B,)
    assert ex.dXdx0 is None and ex.dUdx0 is None


# ---- 2 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B", SHAPES)
def test_duals_are_the_multipliers(N, B):
    nlp, x0, xr, ur, _, ex = _shape_run(N, B)
    sr.check_multipliers(nlp, 1e-8, x0, xr, ur, ex, label="track")


def test_duals_are_the_multipliers_fuzzy():
    import ttmpc
    from oracle import ttmpc_oracle as to
    from ttmpc.scenarios import synthetic_batch
    N, B = 30, 64
    nlp = to.TrackingNLP(N, params=dict(P, horizon=N))
    x0, xr, ur = synthetic_batch(B, N, seed=5, psi_range=0.6)
    w = np.empty((B, 8))
    for b in range(B):
        w[b, :6], w[b, 6:] = to.fuzzy_weights(x0[b], xr[b].T)
    s = _solver(nlp, variant=ttmpc.TT_VARIANT_FUZZY, tol=1e-3, acc_tol=1e-2, max_iter=2000, acc_iter=5)
    plain = s.solve(x0, xr, ur, wq_wr=w)
    r = s.solve_ex(x0, xr, ur, wq_wr=w)
    for a, b in zip(plain, (r.X, r.U, r.status, r.iters, r.kkt)):
        assert np.array_equal(a, b)
    sr.check_multipliers(nlp, 1e-3, x0, xr, ur, r, w=w, label="fuzzy")


# ---- 3 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["free", "active"])
def test_kernel_against_dense_algebra(name):
    from ttmpc import layout
    nlp, x0, xr, ur, s, r = _case_run(name)
    assert np.all(r.status == 0) and np.all(r.sens_status == 0)
    zz = layout.pack(r.X, r.U)
    err_gpu = err_model = smax = 0.0
    nact = []
    for b in range(x0.shape[0]):
        y, _, _ = sr.dual_in_z_order(r.dual[b], nlp.N)
        dense = sr.dense_sensitivity(nlp, zz[b], y, sig=sr.sigma(nlp, zz[b], r.dual[b]))
        model = sr.riccati_sensitivity(nlp, zz[b], r.dual[b])
        assert model["ok"]
        gpu = {"gain": r.gain[b], "dXdx0": r.dXdx0[b], "dUdx0": r.dUdx0[b]}
        assert np.array_equal(r.dUdx0[b, 0], r.gain[b]) and np.array_equal(r.dXdx0[b, 0], np.eye(6))
        err_gpu = max(err_gpu, sr.max_err(gpu, dense))
        err_model = max(err_model, sr.max_err(model, dense))
        smax = max(smax, sr.max_abs(dense))
        act = sr.active_set(nlp, zz[b])
        nact.append(int(act[act >= 6].size))
    print(f"{name}: err_gpu {err_gpu:.3e}, err_model {err_model:.3e}, max|S_dense| {smax:.3e}, active {nact}")
    if name == "free":
        assert max(nact) == 0
    else:
        assert min(nact) >= 13
    assert err_gpu <= 10.0 * err_model + 1e-12 * smax


def _against_dense(tag, nlp, r, w, rows, cond=True):
    """err_gpu <= 10 err_model + 1e-12 max|ref| of the instances ``rows`` against dense algebra at the GPU's own
    primal-dual point, with the numpy recursion as the yardstick; -> (err_gpu, err_model, max|ref|, active counts)."""
    from ttmpc import layout
    zz = layout.pack(r.X, r.U)
    err_gpu = err_model = smax = 0.0
    nact = []
    for b in rows:
        wq, wr = (None, None) if w is None else (w[b, :6], w[b, 6:])
        y, _, _ = sr.dual_in_z_order(r.dual[b], nlp.N)
        dense = sr.dense_sensitivity(nlp, zz[b], y, sig=sr.sigma(nlp, zz[b], r.dual[b]), wq=wq, wr=wr, cond=cond)
        model = sr.riccati_sensitivity(nlp, zz[b], r.dual[b], wq, wr)
        assert model["ok"]
        gpu = {"gain": r.gain[b], "dXdx0": r.dXdx0[b], "dUdx0": r.dUdx0[b]}
        assert np.array_equal(r.dUdx0[b, 0], r.gain[b]) and np.array_equal(r.dXdx0[b, 0], np.eye(6))
        err_gpu = max(err_gpu, sr.max_err(gpu, dense))
        err_model = max(err_model, sr.max_err(model, dense))
        smax = max(smax, sr.max_abs(dense))
        act = sr.active_set(nlp, zz[b])
        nact.append(int(act[act >= 6].size))
    print(f"{tag}: err_gpu {err_gpu:.3e}, err_model {err_model:.3e}, max|S_dense| {smax:.3e}, active {nact}")
    assert err_gpu <= 10.0 * err_model + 1e-12 * smax
    return err_gpu, err_model, smax, nact


@pytest.mark.parametrize("name,pattern,weighted", DERIVATIVE_CASES)
def test_kernel_against_dense_algebra_patterns(name, pattern, weighted):
    nlp, x0, xr, ur, s, r, w = _pattern_run(name, pattern, weighted)
    assert np.all(r.status == 0) and np.all(r.sens_status == 0)
    _, _, _, nact = _against_dense(f"{name} {pattern} weighted={weighted}", nlp, r, w, range(x0.shape[0]))
    if name == "free":
        assert max(nact) == 0
    else:
        assert min(nact) >= 13
    if weighted:   # the weights reach the kernel: the same points without them have other gains
        from ttmpc import layout
        zz = layout.pack(r.X, r.U)
        plain = np.stack([sr.riccati_sensitivity(nlp, zz[b], r.dual[b])["gain"] for b in range(x0.shape[0])])
        assert np.max(np.abs(plain - r.gain)) > 1e-4


def _max_horizon():
    import ttmpc
    return int(ttmpc.lib().tt_max_horizon())


@functools.lru_cache(maxsize=None)
def _horizon_run(N, weighted):
    from oracle import ttmpc_oracle as to
    from ttmpc.scenarios import synthetic_batch
    nlp = to.TrackingNLP(N, params=dict(P, horizon=N))
    x0, xr, ur = synthetic_batch(4, N, seed=4000 + N, psi_range=0.3)
    w = vr.random_weights(4) if weighted else None
    s = _solver(nlp, tol=1e-8)
    r = s.solve_ex(x0, xr, ur, wq_wr=w, duals=True, gain=True, trajectory_sens=True)
    return nlp, x0, xr, ur, w, s, r


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("N", [1, 2, 20, 63, 64, 65, "max"])
def test_horizons(N, weighted):
    """The pre-pass gives lane k the stages k, k + 64, ...: one trip up to N = 63, a second from N = 64 on, a third at
    the longest horizon, whose launch is also the largest dynamic LDS request (sens_lds_doubles)."""
    N = _max_horizon() if N == "max" else N
    nlp, x0, xr, ur, w, s, r = _horizon_run(N, weighted)
    print(f"N={N} weighted={weighted}: status {r.status.tolist()}, sens_status {r.sens_status.tolist()}")
    ok = np.flatnonzero(r.status <= 1)
    assert ok.size >= 3
    for b in np.flatnonzero(r.status > 1):
        assert r.sens_status[b] == 2 and not r.gain[b].any() and not r.dXdx0[b].any() and not r.dUdx0[b].any()
    assert np.all(r.sens_status[ok] == 0)
    _, _, smax, _ = _against_dense(f"N={N} weighted={weighted}", nlp, r, w, ok, cond=False)
    assert np.max(np.abs(r.gain[ok])) > 1e-3 and smax >= 1.0


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sens_device(s, N, X, U, D, st, w=None, gain=True, traj=True):
    """tt_track_sens_device on host arrays staged by torch -> (gain, dXdx0, dUdx0, sens_status), NaN / -1 prefilled."""
    import torch
    B = X.shape[0]
    dev = torch.device("cuda")
    tX, tU, tD, tst = _dev(X), _dev(U), _dev(D), _dev(np.asarray(st, dtype=np.int32))
    tw = None if w is None else _dev(w)
    g = torch.full((B, 2, 6), np.nan, dtype=torch.float64, device=dev)
    dX = torch.full((B, N + 1, 6, 6), np.nan, dtype=torch.float64, device=dev)
    dU = torch.full((B, N, 2, 6), np.nan, dtype=torch.float64, device=dev)
    ss = torch.full((B,), -1, dtype=torch.int32, device=dev)
    s.sens_device(B, tX.data_ptr(), tU.data_ptr(), tD.data_ptr(), tst.data_ptr(), gain=g.data_ptr() if gain else 0,
                  dxdx0=dX.data_ptr() if traj else 0, dudx0=dU.data_ptr() if traj else 0, sens_status=ss.data_ptr(),
                  wq_wr=0 if tw is None else tw.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return g.cpu().numpy(), dX.cpu().numpy(), dU.cpu().numpy(), ss.cpu().numpy()


def test_grid_indexing():
    """One B = 2304 launch on 576 copies of the N = 20 batch: every block finds its own instance."""
    nlp, x0, xr, ur, w, s, r = _horizon_run(20, True)
    rep = lambda a: np.tile(a, (576,) + (1,) * (a.ndim - 1))  # noqa: E731
    g, dX, dU, ss = _sens_device(s, 20, rep(r.X), rep(r.U), rep(r.dual), rep(r.status), w=rep(w))
    for got, ref in ((g, r.gain), (dX, r.dXdx0), (dU, r.dUdx0), (ss, r.sens_status)):
        assert got.shape[0] == 2304
        assert np.array_equal(got[:4], ref)
        assert np.array_equal(got, rep(ref))


def test_weighted_sens_device_is_bitwise_the_fused_call():
    """tt_track_sens_device with wq_wr on the outputs of a weighted solve, and the gain alone."""
    nlp, x0, xr, ur, s, r, w = _pattern_run("active", "mpc_full", True)
    assert np.all(r.sens_status == 0)
    g, dX, dU, ss = _sens_device(s, nlp.N, r.X, r.U, r.dual, r.status, w=w)
    assert np.array_equal(g, r.gain) and np.array_equal(dX, r.dXdx0) and np.array_equal(dU, r.dUdx0)
    assert np.array_equal(ss, r.sens_status)
    g1, dX1, dU1, ss1 = _sens_device(s, nlp.N, r.X, r.U, r.dual, r.status, w=w, traj=False)
    assert np.array_equal(g1, r.gain) and np.array_equal(ss1, r.sens_status)
    assert np.isnan(dX1).all() and np.isnan(dU1).all()            # outputs not asked for are not written
    g0, _, _, _ = _sens_device(s, nlp.N, r.X, r.U, r.dual, r.status)   # without the weights: another gain
    assert np.max(np.abs(g0 - r.gain)) > 1e-4
    one = s.solve_ex(x0, xr, ur, wq_wr=w, duals=False, gain=True, trajectory_sens=False)
    assert np.array_equal(one.gain, r.gain) and np.array_equal(one.sens_status, r.sens_status)


def test_sens_device_is_bitwise_the_fused_call():
    import torch
    nlp, x0, xr, ur, s, r = _case_run("active")
    B, N = x0.shape[0], nlp.N
    dev = torch.device("cuda")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    X, U, D, st = t(r.X), t(r.U), t(r.dual), t(r.status)
    gain = torch.full((B, 2, 6), np.nan, dtype=torch.float64, device=dev)
    dX = torch.full((B, N + 1, 6, 6), np.nan, dtype=torch.float64, device=dev)
    dU = torch.full((B, N, 2, 6), np.nan, dtype=torch.float64, device=dev)
    ss = torch.full((B,), -1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    s.sens_device(B, X.data_ptr(), U.data_ptr(), D.data_ptr(), st.data_ptr(), gain=gain.data_ptr(),
                  dxdx0=dX.data_ptr(), dudx0=dU.data_ptr(), sens_status=ss.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(gain.cpu().numpy(), r.gain)
    assert np.array_equal(dX.cpu().numpy(), r.dXdx0)
    assert np.array_equal(dU.cpu().numpy(), r.dUdx0)
    assert np.array_equal(ss.cpu().numpy(), r.sens_status)
    # the fused device call, with the handle-owned dual buffer (no `dual` output): the same numbers again
    xo = torch.empty((B, N + 1, 6), dtype=torch.float64, device=dev)
    uo = torch.empty((B, N, 2), dtype=torch.float64, device=dev)
    st2 = torch.empty((B,), dtype=torch.int32, device=dev)
    gain2 = torch.full((B, 2, 6), np.nan, dtype=torch.float64, device=dev)
    ss2 = torch.full((B,), -1, dtype=torch.int32, device=dev)
    a0, ar, au = t(x0), t(xr), t(ur)
    s.solve_ex_device(B, a0.data_ptr(), ar.data_ptr(), au.data_ptr(), xo.data_ptr(), uo.data_ptr(), st2.data_ptr(),
                      gain=gain2.data_ptr(), sens_status=ss2.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert np.array_equal(xo.cpu().numpy(), r.X) and np.array_equal(gain2.cpu().numpy(), r.gain)
    assert np.array_equal(ss2.cpu().numpy(), r.sens_status)


# ---- 4 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["free", "active"])
def test_gain_against_oracle_finite_differences(name):
    nlp, x0, xr, ur, s, r = _case_run(name)
    z, st, dz = sr.oracle_fd(nlp, x0, xr, ur, h=1e-4)
    assert np.all(st == 0) and np.all(r.status == 0) and np.all(r.sens_status == 0)
    Kfd = np.stack([sr._split(nlp, dz[b])["gain"] for b in range(x0.shape[0])])
    err = np.max(np.abs(r.gain - Kfd), axis=(1, 2))
    print(f"{name}: gain vs oracle FD per instance {err}, max|K| per instance {np.max(np.abs(r.gain), axis=(1, 2))}")
    assert np.max(err) <= 1e-5
    if name == "free":
        assert np.max(np.abs(r.gain)) > 0.01
    else:
        assert np.max(np.abs(r.gain[2, 0])) > 0.01      # a_0 free
        assert np.max(np.abs(r.gain[2, 1])) <= 1e-5     # omega_0 on its bound
        for b in range(x0.shape[0]):
            u0 = z[b, 6:8]
            on = np.minimum(u0 - nlp.ulb, nlp.uub - u0) <= 1e-6
            if on.all():
                assert np.max(np.abs(r.gain[b])) <= 1e-5, b


# ---- 5 ----------------------------------------------------------------------------------------------------------
def test_status_plumbing():
    import ttmpc
    from oracle import ttmpc_oracle as to
    from ttmpc.scenarios import synthetic_batch
    N = 12
    nlp = to.TrackingNLP(N, params=dict(P, horizon=N))
    x0, xr, ur = synthetic_batch(5, N, seed=8)
    s = _solver(nlp)
    good = s.solve_ex(x0, xr, ur, trajectory_sens=True)
    assert list(good.status) == [0] * 5 and list(good.sens_status) == [0] * 5
    x0b = x0.copy()
    x0b[1, 3] = 1.3            # hitch angle beyond pi/3
    x0b[3, 2] = 4.0            # heading beyond pi
    r = s.solve_ex(x0b, xr, ur, trajectory_sens=True)
    assert list(r.status) == [0, 3, 0, 3, 0]
    assert list(r.sens_status) == [0, 2, 0, 2, 0]
    for b in (1, 3):
        assert not r.gain[b].any() and not r.dXdx0[b].any() and not r.dUdx0[b].any() and not r.dual[b].any()
    for b in (0, 2, 4):  # the neighbours are what they were in the all-feasible batch
        for k in ("X", "U", "dual", "gain", "dXdx0", "dUdx0"):
            assert np.array_equal(getattr(r, k)[b], getattr(good, k)[b]), (b, k)
        assert np.max(np.abs(r.gain[b])) > 0.0
    # all-NULL extra is the plain call
    plain = s.solve(x0, xr, ur)
    none = s.solve_ex(x0, xr, ur, duals=False, gain=False)
    assert np.array_equal(plain[0], none.X) and none.dual is None and none.sens_status is None
    assert s._L.tt_track_dual_len(N) == 22 * (N + 1)


def test_undefined_sensitivity_reports_status_1():
    """The kernel's handled path: a point at which the sweep has no positive definite G_k, or is not finite, reports
    sens_status 1 with zeroed outputs and leaves its neighbours alone."""
    from oracle import ttmpc_oracle as to
    from ttmpc import layout
    from ttmpc.scenarios import synthetic_batch
    N = 12
    nlp = to.TrackingNLP(N, params=dict(P, horizon=N))
    x0, xr, ur = synthetic_batch(5, N, seed=8)
    s = _solver(nlp)
    good = s.solve_ex(x0, xr, ur, trajectory_sens=True)
    assert list(good.status) == [0] * 5 and list(good.sens_status) == [0] * 5
    dual = good.dual.copy()
    dual[1, 4, 2] = np.nan          # a multiplier of the dynamics: the curvature it scales is not a number
    dual[3, N - 1, 14 + 6] = -1e9   # z_U of a_{N-1}: Sigma = z_U / (ub - a) takes G_00 = 2 R_00 + Sigma + ... below 0
    zz = layout.pack(good.X, good.U)
    assert not sr.riccati_sensitivity(nlp, zz[3], dual[3])["ok"] and sr.riccati_sensitivity(nlp, zz[2], dual[2])["ok"]
    for traj in (True, False):
        g, dX, dU, ss = _sens_device(s, N, good.X, good.U, dual, good.status, traj=traj)
        assert list(ss) == [0, 1, 0, 1, 0]
        for b in (1, 3):
            assert not g[b].any()
            assert not traj or (not dX[b].any() and not dU[b].any())
        for b in (0, 2, 4):
            assert np.array_equal(g[b], good.gain[b])
            assert not traj or (np.array_equal(dX[b], good.dXdx0[b]) and np.array_equal(dU[b], good.dUdx0[b]))


def test_obca_handle_is_rejected():
    import ctypes as C
    import errno

    import ttmpc
    from oracle import ttmpc_oracle as to
    N = 10
    o = ttmpc.ObcaSolver(N, P, to.DEFAULT_Q, to.DEFAULT_R, to.OBCA_XLB, to.OBCA_XUB, to.MPC_ULB, to.MPC_UUB,
                         np.array([[30.0, 30.0, 4.0, 4.0]]), variant=ttmpc.TT_VARIANT_TRACK_OBCA)
    from ttmpc._lib import TTTrackExtra, _ip, _ptr
    x0, xr, ur = np.zeros((1, 6)), np.zeros((1, N + 1, 6)), np.zeros((1, N, 2))
    X, U, st = np.empty((1, N + 1, 6)), np.empty((1, N, 2)), np.empty(1, dtype=np.int32)
    gain = np.empty((1, 2, 6))
    ex = TTTrackExtra(None, gain.ctypes.data, None, None, None)
    rc = o._L.tt_solve_batch_ex(o._h, 1, _ptr(x0), _ptr(xr), _ptr(ur), None, None, _ptr(X), _ptr(U),
                                st.ctypes.data_as(_ip), None, None, C.byref(ex))
    assert rc == -errno.EINVAL
    assert o._L.tt_solve_batch_ex_device(o._h, 1, None, None, None, None, None, None, None, None, None, None,
                                         C.byref(ex), None) == -errno.EINVAL
    assert o._L.tt_track_sens_device(o._h, 1, None, None, None, None, None, None, None, None, None,
                                     None) == -errno.EINVAL


# ---- 6 ----------------------------------------------------------------------------------------------------------
def test_solve_with_gain_matches_solve_ex():
    import ttmpc
    from oracle import ttmpc_oracle as to
    nlp, x0, xr, ur, s, r = _case_run("free")
    N = nlp.N
    ctl = ttmpc.MPCTrackingControl(ttmpc.TruckTrailerModel(dict(P, horizon=N)), dict(P, horizon=N), to.DEFAULT_Q,
                                   to.DEFAULT_R, {"lb": to.MPC_XLB, "ub": to.MPC_XUB},
                                   {"lb": to.MPC_ULB, "ub": to.MPC_UUB})
    one = s.solve_ex(x0[:1], xr[:1], ur[:1])
    states, inputs, K = ctl.solve_with_gain(x0[0], xr[0].T, ur[0].T)
    assert K.shape == (2, 6) and np.array_equal(K, one.gain[0])
    assert np.array_equal(states, one.X[0].T) and np.array_equal(inputs, one.U[0].T)
    s2, i2 = ctl.solve(x0[0], xr[0].T, ur[0].T)
    assert np.array_equal(s2, states) and np.array_equal(i2, inputs)
    assert np.array_equal(one.gain[0], r.gain[0])  # B = 1 and B = 8 give the same instance the same gain
