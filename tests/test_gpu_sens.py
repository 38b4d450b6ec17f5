"""GPU suite: multiplier export and x_init sensitivities of the tracking solve (tt_solve_batch_ex, track_sens_kernel).

1. solve_ex returns bitwise the plain outputs of solve, for every build of track_kernel.
2. The exported duals are the multipliers: signs, zeros, and IPOPT's own stopping test re-evaluated in numpy.
3. The sensitivity kernel against dense algebra on the same duals, with the numpy Riccati as the yardstick.
4. The gain against central finite differences of the CPU oracle.
5. Status plumbing: failed instances, OBCA handles.
6. MPCTrackingControl.solve_with_gain.

Every case prints its figures before it asserts (DESIGN.md "Multiplier export and x_init sensitivities" records them).
"""
import functools

import numpy as np
import pytest

import sens_reference as sr

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


@functools.lru_cache(maxsize=None)
def _case_run(name):
    """solve_ex with every output on one of the two checked input sets, shared by cases 3 and 4."""
    nlp, x0, xr, ur = sr.case_free() if name == "free" else sr.case_active()
    s = _solver(nlp)
    r = s.solve_ex(x0, xr, ur, duals=True, gain=True, trajectory_sens=True)
    return nlp, x0, xr, ur, s, r


# ---- 1 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,B", SHAPES)
def test_plain_results_unchanged(N, B):
    _, _, _, _, plain, ex = _shape_run(N, B)
    for a, b in zip(plain, (ex.X, ex.U, ex.status, ex.iters, ex.kkt)):
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
    assert ex.dual.shape == (B, N + 1, 22) and ex.gain.shape == (B, 2, 6) and ex.sens_status.shape == (B,)
    assert ex.dXdx0 is None and ex.dUdx0 is None


# ---- 2 ----------------------------------------------------------------------------------------------------------
def _check_multipliers(nlp, tol, x0, xr, ur, r, w=None, label=""):
    from ttmpc import layout
    N, B = nlp.N, x0.shape[0]
    lb, ub = nlp.bounds()
    lbr, ubr = sr.relaxed_bounds(nlp)
    fl, fu = np.isfinite(lb), np.isfinite(ub)
    nb = int(fl.sum() + fu.sum())
    m = 6 * (N + 1) + nb
    ok = np.flatnonzero(r.status == 0)
    assert ok.size > 0
    pick = ok[:: max(1, ok.size // 8)][:8]
    zz = layout.pack(r.X, r.U)
    for b in pick:
        y, zl, zu = sr.dual_in_z_order(r.dual[b], N)
        assert np.all(zl >= 0.0) and np.all(zu >= 0.0)
        assert np.all(zl[~fl] == 0.0) and np.all(zu[~fu] == 0.0)
        assert np.all(r.dual[b, N, 12:14] == 0.0) and np.all(r.dual[b, N, 20:22] == 0.0)
        wq, wr = (None, None) if w is None else (w[b, :6], w[b, 6:])
        res = sr.stationarity(nlp, zz[b], xr[b], ur[b], r.dual[b], wq, wr)
        sz = float(np.sum(zl) + np.sum(zu))
        s_d = max(100.0, (float(np.sum(np.abs(y))) + sz) / m) / 100.0
        s_c = max(100.0, sz / nb) / 100.0
        dinf = float(np.max(np.abs(res)))
        compl = max(float(np.max(zl[fl] * (zz[b][fl] - lbr[fl]))), float(np.max(zu[fu] * (ubr[fu] - zz[b][fu]))))
        print(f"{label} N={N} instance {b}: dual inf {dinf:.3e} (bound {2 * tol * s_d:.3e}), "
              f"compl {compl:.3e} (bound {2 * tol * s_c:.3e})")
        assert dinf <= 2.0 * tol * s_d
        assert compl <= 2.0 * tol * s_c
        # CasADi's view of the same numbers
        lam_g, lam_x = layout.casadi_multipliers(r.dual[b], N)
        g = nlp.grad(zz[b], xr[b].T, ur[b].T, wq, wr)
        assert np.max(np.abs(g + nlp.jacobian(zz[b]).T @ lam_g + lam_x)) <= 2.0 * tol * s_d


@pytest.mark.parametrize("N,B", SHAPES)
def test_duals_are_the_multipliers(N, B):
    nlp, x0, xr, ur, _, ex = _shape_run(N, B)
    _check_multipliers(nlp, 1e-8, x0, xr, ur, ex, label="track")


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
    _check_multipliers(nlp, 1e-3, x0, xr, ur, r, w=w, label="fuzzy")


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
