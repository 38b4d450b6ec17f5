"""GPU suite: gradients in the box (xlb, xub, ulb, uub): track_vjp_kernel's bounds instantiations behind
tt_track_vjp_bounds*, tt_set_bounds / tt_get_bounds, ClosedLoop.backward(bounds=True) and the ``bounds`` tensor of
ttmpc.diff.

1. The kernel against dense algebra on the GPU's own duals (the numpy recursion as the yardstick), the lower and the
   upper bounds each on their own: both input sets, the run-time and the OBCA bound pattern, a state-bound case.
2. Horizons, grid indexing.
3. Neutrality: the other outputs with g_bounds, the NULL g_bounds call, the host call.
4. accumulate, failed solves, a NaN upstream gradient.
5. tt_set_bounds against fresh handles, bit for bit, across the builds of the tracking kernel; bad calls.
6. Against central differences of the CPU oracle in the bounds.
7. The closed loop's sweep against the numpy chain and against the per-step calls; neutrality; raises.
8. Autograd: the layers are the calls; the unit gradient of a saturated input.

Every case prints its figures before it asserts (DESIGN.md "Adjoint in the bounds" records them).
"""
import ctypes as C
import errno
import functools

import numpy as np
import pytest

import bounds_vjp_reference as br
import loop_vjp_reference as lv
import sens_reference as sr
import vjp_harness as h
import vjp_reference as vr

pytestmark = pytest.mark.gpu

P = sr.P
OUTS = ("g_x0", "g_xref", "g_uref", "g_wq_wr", "vjp_status")
HALVES = ("lower", "upper")
TIGHT = dict(ulb=np.array([-0.3, -0.02]), uub=np.array([0.3, 0.02]))   # case_active's input box

_t, _n, _solver, _w = h.t, h.n, h.solver, h.w_of


def _halves(g):
    g = np.asarray(g)
    return {"lower": g[..., :8], "upper": g[..., 8:]}


def _tensor16(nlp):
    """The box of an NLP as the (16,) vector of the autograd layers: xlb 6, ulb 2, xub 6, uub 2."""
    return np.concatenate(br.box(nlp))


def _references(nlp, r, gX, gU, w=None, cond=False):
    """dense and model (B,16) on the GPU's own primal-dual point."""
    from ttmpc import layout
    zz = layout.pack(r.X, r.U)
    dense, model = np.zeros((zz.shape[0], 16)), np.zeros((zz.shape[0], 16))
    for b in range(zz.shape[0]):
        dense[b] = br.dense_bounds_vjp(nlp, zz[b], r.dual[b], gX[b], gU[b], *_w(w, b), cond=cond)["bounds"]
        m = br.riccati_bounds_vjp(nlp, zz[b], r.dual[b], gX[b], gU[b], *_w(w, b))
        assert m["ok"]
        model[b] = m["bounds"]
    return dense, model


def _infinite(nlp):
    fl, fu = br.finite(*br.box(nlp))
    return np.concatenate([~fl, ~fu])


def _exact_zeros(g, mask):
    z = np.asarray(g)[..., mask]
    return bool(np.all(z == 0.0) and not np.any(np.signbit(z)))


@functools.lru_cache(maxsize=None)
def _case_run(name, weighted, pattern="mpc_diag"):
    nlp, x0, xr, ur = sr.case(name, pattern)
    B = x0.shape[0]
    w = vr.random_weights(B) if weighted else None
    s = _solver(nlp)
    r = s.solve_ex(x0, xr, ur, wq_wr=w, duals=True, gain=False)
    gX, gU = vr.random_upstream(B, nlp.N)
    v = s.vjp(r.X, r.U, r.dual, xr, ur, r.status, gX, gU, wq_wr=w, bounds=True)
    return nlp, x0, xr, ur, w, s, r, gX, gU, v


# ---- 1 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,weighted,pattern", [("free", False, "mpc_diag"), ("active", False, "mpc_diag"),
                                                   ("active", True, "mpc_diag"), ("free", False, "run_time"),
                                                   ("free", False, "obca")])
def test_kernel_against_dense_algebra(name, weighted, pattern):
    nlp, x0, xr, ur, w, s, r, gX, gU, v = _case_run(name, weighted, pattern)
    B = x0.shape[0]
    assert np.all(r.status == 0) and np.all(v.vjp_status == 0)
    assert v["bounds"].shape == (B, 16) and v["bounds"] is v.g_bounds
    for part, lo, hi in (("g_xlb", 0, 6), ("g_ulb", 6, 8), ("g_xub", 8, 14), ("g_uub", 14, 16)):
        assert np.shares_memory(getattr(v, part), v.g_bounds) and np.array_equal(getattr(v, part), v.g_bounds[:, lo:hi])
    dense, model = _references(nlp, r, gX, gU, w)
    h.compare_with_chain(f"{name} {pattern} weighted={weighted}", _halves(v.g_bounds), _halves(dense), _halves(model),
                         HALVES, per_group=True)
    inf = _infinite(nlp)
    print(f"{name} {pattern}: infinite bounds at {np.flatnonzero(inf).tolist()}")
    assert inf.any() and _exact_zeros(v.g_bounds, inf)
    if pattern == "run_time":
        assert inf[8 + 2] and not inf[2]          # the heading: bounded below only
    if pattern == "obca":
        assert inf[2] and inf[8 + 2]              # the heading: free
    if name == "active":
        assert np.max(np.abs(dense)) > 0.1        # the loss on saturated inputs arrives here
    plain = s.vjp(r.X, r.U, r.dual, xr, ur, r.status, gX, gU, wq_wr=w)
    assert plain.g_bounds is None and plain.g_xlb is None
    for k in OUTS:
        assert np.array_equal(getattr(v, k), getattr(plain, k)), k


def test_state_bound_case():
    """case_active with the steering angle bounded below at -0.2405 (found with the CPU oracle: instance 4 starts at
    -0.2383, every other instance above it, and its optimum then sits on the bound at two stages with multipliers near
    5; every instance converges)."""
    nlp0, x0, xr, ur = sr.case_active()
    lo, up = br.box(nlp0)
    lo[4] = -0.2405
    nlp = br.with_box(nlp0, lo, up)
    assert np.all(x0[:, :6] > lo[:6] + 1e-3) and np.all(x0[:, :6] < up[:6] - 1e-3)          # every x_init feasible
    B, N = x0.shape[0], nlp.N
    s = _solver(nlp)
    r = s.solve_ex(x0, xr, ur, duals=True, gain=False)
    assert np.all(r.status == 0)
    zx = np.concatenate([r.dual[:, 1:, 6:12], r.dual[:, 1:, 14:20]], axis=2)                # state bounds, stages >= 1
    print(f"state-bound multipliers above 1e-3 at stages k >= 1: {zx[zx > 1e-3].tolist()}")
    assert int((zx > 1e-3).sum()) >= 2
    gX, gU = vr.random_upstream(B, N)
    v = s.vjp(r.X, r.U, r.dual, xr, ur, r.status, gX, gU, bounds=True)
    assert np.all(v.vjp_status == 0)
    dense, model = _references(nlp, r, gX, gU)
    h.compare_with_chain("state bound", _halves(v.g_bounds), _halves(dense), _halves(model), HALVES, per_group=True)
    print(f"dL/dxlb[4] per instance {v.g_xlb[:, 4]}")
    assert np.max(np.abs(v.g_xlb[:, 4])) > 1e-2


# ---- 2 ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _horizon_run(N):
    """B = 4 in case_active's input box: bounds are active at every horizon (the CPU oracle converges on all four)."""
    from oracle import ttmpc_oracle as to
    from ttmpc.scenarios import synthetic_batch
    nlp = to.TrackingNLP(N, params=dict(P, horizon=N), **TIGHT)
    x0, xr, ur = synthetic_batch(4, N, seed=4000 + N, psi_range=0.3)
    s = _solver(nlp)
    r = s.solve_ex(x0, xr, ur, duals=True, gain=False)
    gX, gU = vr.random_upstream(4, N, seed=N)
    v = s.vjp(r.X, r.U, r.dual, xr, ur, r.status, gX, gU, bounds=True)
    return nlp, x0, xr, ur, s, r, gX, gU, v


@pytest.mark.parametrize("N", [1, 2, 64, 170])
def test_horizons(N):
    """N = 64 is the first horizon where lanes take a second stage, N = 170 the LDS limit."""
    nlp, x0, xr, ur, s, r, gX, gU, v = _horizon_run(N)
    print(f"N={N}: status {r.status.tolist()}, vjp_status {v.vjp_status.tolist()}")
    assert not r.status.any() and not v.vjp_status.any()
    dense, model = _references(nlp, r, gX, gU)
    e_gpu = {k: float(np.max(np.abs(_halves(v.g_bounds)[k] - _halves(model)[k]))) for k in HALVES}
    e_model = {k: float(np.max(np.abs(_halves(model)[k] - _halves(dense)[k]))) for k in HALVES}
    big = {k: float(np.max(np.abs(_halves(model)[k]))) for k in HALVES}
    for k in HALVES:
        print(f"N={N} {k}: gpu vs numpy recursion {e_gpu[k]:.3e}, recursion vs dense {e_model[k]:.3e}, "
              f"max|g_bounds| {big[k]:.3e}")
    assert max(big.values()) > 0.1
    for k in HALVES:
        assert e_gpu[k] <= 10.0 * e_model[k] + 1e-12 * big[k], k
    assert _exact_zeros(v.g_bounds, _infinite(nlp))


@functools.lru_cache(maxsize=None)
def _n20_run():
    from oracle import ttmpc_oracle as to
    from ttmpc.scenarios import synthetic_batch
    N = 20
    nlp = to.TrackingNLP(N, params=dict(P, horizon=N), **TIGHT)
    x0, xr, ur = synthetic_batch(4, N, seed=4020, psi_range=0.3)
    s = _solver(nlp)
    r = s.solve_ex(x0, xr, ur, duals=True, gain=False)
    gX, gU = vr.random_upstream(4, N, seed=N)
    return nlp, x0, xr, ur, s, r, gX, gU


def test_batch_independence():
    """One B = 2304 launch on 576 copies of an N = 20, B = 4 batch returns the B = 4 rows, bit for bit."""
    nlp, x0, xr, ur, s, r, gX, gU = _n20_run()
    assert not r.status.any()
    v = s.vjp(r.X, r.U, r.dual, xr, ur, r.status, gX, gU, bounds=True, model=True)
    rep = lambda a: np.tile(a, (576,) + (1,) * (a.ndim - 1))  # noqa: E731
    big = s.vjp(rep(r.X), rep(r.U), rep(r.dual), rep(xr), rep(ur), rep(r.status), rep(gX), rep(gU), bounds=True,
                model=True)
    for k in OUTS + ("g_model", "g_bounds"):
        got, ref = getattr(big, k), getattr(v, k)
        assert got.shape[0] == 2304
        assert np.array_equal(got, rep(ref)), k
    assert not v.vjp_status.any() and np.max(np.abs(v.g_bounds)) > 0.1


# ---- 3, 4 -------------------------------------------------------------------------------------------------------
def _device_vjp(s, r, xr, ur, gX, gU, w=None, mode="bounds", g_bounds=None, g_model=None, accumulate=False):
    """One device call on fresh buffers: mode "plain" (tt_track_vjp_device), "model" (tt_track_vjp_model_device),
    "bounds" (tt_track_vjp_bounds_device with g_bounds, and g_model if given) or "null" (that entry with
    g_bounds == NULL).  -> dict of numpy outputs."""
    import torch
    from ttmpc._lib import TTTrackVjpBoundsOut
    B, N = r.X.shape[0], s.N
    ins = [_t(a) for a in (r.X, r.U, r.dual, xr, ur)]
    st, tgx, tgu = _t(r.status, torch.int32), _t(gX), _t(gU)
    tw = None if w is None else _t(w)
    outs = [torch.full(sh, np.nan, dtype=torch.float64, device="cuda") for sh in ((B, 6), (B, N + 1, 6), (B, N, 2), (B, 8))]
    vst = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    gb = None if g_bounds is None else _t(g_bounds)
    gm = None if g_model is None else _t(g_model)
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    if mode == "null":
        bo = TTTrackVjpBoundsOut(*[o.data_ptr() for o in outs], ptr(gm) or None, None, vst.data_ptr())
        rc = s._L.tt_track_vjp_bounds_device(s._h, B, *[t.data_ptr() for t in ins], ptr(tw) or None, st.data_ptr(),
                                             tgx.data_ptr(), tgu.data_ptr(), C.byref(bo), int(accumulate), None)
        assert rc == 0
    else:
        s.vjp_device(B, *[t.data_ptr() for t in ins[:3]], ins[3].data_ptr(), ins[4].data_ptr(), st.data_ptr(),
                     grad_x=tgx.data_ptr(), grad_u=tgu.data_ptr(), g_x0=outs[0].data_ptr(), g_xref=outs[1].data_ptr(),
                     g_uref=outs[2].data_ptr(), g_wq_wr=outs[3].data_ptr(), vjp_status=vst.data_ptr(), wq_wr=ptr(tw),
                     g_model=ptr(gm) if mode in ("model", "bounds") else 0, accumulate=accumulate,
                     g_bounds=ptr(gb) if mode == "bounds" else 0)
    torch.cuda.synchronize()
    d = {k: _n(o) for k, o in zip(OUTS, outs + [vst])}
    d["g_bounds"] = None if gb is None else _n(gb)
    d["g_model"] = None if gm is None else _n(gm)
    return d


@pytest.mark.parametrize("weighted", [False, True])
def test_neutrality(weighted):
    nlp, x0, xr, ur, w, s, r, gX, gU, v = _case_run("active", weighted)
    B = x0.shape[0]
    nan16, nan3 = np.full((B, 16), np.nan), np.full((B, 3), np.nan)
    plain = _device_vjp(s, r, xr, ur, gX, gU, w, "plain")
    model = _device_vjp(s, r, xr, ur, gX, gU, w, "model", g_model=nan3)
    only = _device_vjp(s, r, xr, ur, gX, gU, w, "bounds", nan16)
    both = _device_vjp(s, r, xr, ur, gX, gU, w, "bounds", nan16, nan3)
    null = _device_vjp(s, r, xr, ur, gX, gU, w, "null")
    null_m = _device_vjp(s, r, xr, ur, gX, gU, w, "null", g_model=nan3)
    for k in OUTS:
        assert np.array_equal(only[k], plain[k]), k            # with g_bounds: the other outputs are the plain call's
        assert np.array_equal(both[k], plain[k]), k
        assert np.array_equal(null[k], plain[k]), k            # g_bounds == NULL: tt_track_vjp_model_device
        assert np.array_equal(null_m[k], plain[k]), k
        assert np.array_equal(getattr(v, k), plain[k]), k      # the host call: the device call
    assert np.array_equal(both["g_model"], model["g_model"]) and np.array_equal(null_m["g_model"], model["g_model"])
    assert np.array_equal(both["g_bounds"], only["g_bounds"]) and np.array_equal(v.g_bounds, only["g_bounds"])
    assert not plain["vjp_status"].any() and np.max(np.abs(only["g_bounds"])) > 0.1
    hb = s.vjp(r.X, r.U, r.dual, xr, ur, r.status, gX, gU, wq_wr=w, bounds=True, model=True)
    assert np.array_equal(hb.g_bounds, only["g_bounds"]) and np.array_equal(hb.g_model, model["g_model"])


def test_accumulate_and_failures():
    from oracle import ttmpc_oracle as to
    from ttmpc.scenarios import synthetic_batch
    N, B = 12, 5
    nlp = to.TrackingNLP(N, params=dict(P, horizon=N), **TIGHT)
    x0, xr, ur = synthetic_batch(B, N, seed=8)
    s = _solver(nlp)
    gX, gU = vr.random_upstream(B, N)
    good = s.solve_ex(x0, xr, ur, gain=False)
    assert list(good.status) == [0] * B
    rng = np.random.default_rng(2)
    pre, pre_m = rng.uniform(-1.0, 1.0, (B, 16)), rng.uniform(-1.0, 1.0, (B, 3))
    once = _device_vjp(s, good, xr, ur, gX, gU, None, "bounds", np.full((B, 16), np.nan), np.full((B, 3), np.nan))
    val, val_m = once["g_bounds"], once["g_model"]
    assert not once["vjp_status"].any() and np.max(np.abs(val)) > 1e-2
    acc1 = _device_vjp(s, good, xr, ur, gX, gU, None, "bounds", pre, pre_m, accumulate=True)
    acc2 = _device_vjp(s, good, xr, ur, gX, gU, None, "bounds", acc1["g_bounds"], acc1["g_model"], accumulate=True)
    assert np.array_equal(acc1["g_bounds"], pre + val) and np.array_equal(acc2["g_bounds"], (pre + val) + val)
    assert np.array_equal(acc1["g_model"], pre_m + val_m) and np.array_equal(acc2["g_model"], (pre_m + val_m) + val_m)
    for k in OUTS:                                                  # accumulate concerns g_model and g_bounds only
        assert np.array_equal(acc1[k], once[k]), k
    # a failed solve (x_init outside the box): status 3 -> vjp_status 2
    x0b = x0.copy()
    x0b[1, 3] = 1.3            # hitch angle beyond pi/3
    x0b[3, 2] = 4.0            # heading beyond pi
    r = s.solve_ex(x0b, xr, ur, gain=False)
    assert list(r.status) == [0, 3, 0, 3, 0]
    wr = _device_vjp(s, r, xr, ur, gX, gU, None, "bounds", np.full((B, 16), np.nan))
    ac = _device_vjp(s, r, xr, ur, gX, gU, None, "bounds", pre, accumulate=True)
    assert list(wr["vjp_status"]) == [0, 2, 0, 2, 0] and list(ac["vjp_status"]) == [0, 2, 0, 2, 0]
    for b in (1, 3):
        assert not wr["g_bounds"][b].any()                         # zeros for accumulate = 0
        assert np.array_equal(ac["g_bounds"][b], pre[b])           # an untouched accumulator for accumulate = 1
    for b in (0, 2, 4):
        assert np.array_equal(wr["g_bounds"][b], val[b])
        assert np.array_equal(ac["g_bounds"][b], pre[b] + val[b])
    # a NaN in one instance's upstream gradient: that instance alone is undefined
    gXn = gX.copy()
    gXn[2, 5, 1] = np.nan
    nw = _device_vjp(s, good, xr, ur, gXn, gU, None, "bounds", np.full((B, 16), np.nan))
    na = _device_vjp(s, good, xr, ur, gXn, gU, None, "bounds", pre, accumulate=True)
    assert list(nw["vjp_status"]) == [0, 0, 1, 0, 0] and list(na["vjp_status"]) == [0, 0, 1, 0, 0]
    assert not nw["g_bounds"][2].any() and np.array_equal(na["g_bounds"][2], pre[2])
    for b in (0, 1, 3, 4):
        assert np.array_equal(nw["g_bounds"][b], val[b])
        for k in OUTS[:4]:
            assert np.array_equal(nw[k][b], once[k][b]), (b, k)


# ---- 5 ----------------------------------------------------------------------------------------------------------
def _device_solve(s, x0, xr, ur):
    """solve_ex_device on fresh buffers -> [X, U, status, iters, kkt, dual]."""
    import torch
    B, N = x0.shape[0], s.N
    ins = [_t(a) for a in (x0, xr, ur)]
    X, U, dual = (torch.full(sh, np.nan, dtype=torch.float64, device="cuda")
                  for sh in ((B, N + 1, 6), (B, N, 2), (B, N + 1, 22)))
    kkt = torch.full((B,), np.nan, dtype=torch.float64, device="cuda")
    st, it = (torch.full((B,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    s.solve_ex_device(B, *[t.data_ptr() for t in ins], X.data_ptr(), U.data_ptr(), st.data_ptr(), iters=it.data_ptr(),
                      kkt=kkt.data_ptr(), dual=dual.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [_n(a) for a in (X, U, st, it, kkt, dual)]


def _all_solves(s, x0, xr, ur):
    """The host entry (B = 4: the zero-copy path), the exporting host entry and the device entry of one solver."""
    r = s.solve_ex(x0, xr, ur, duals=True, gain=False)
    return list(s.solve(x0, xr, ur)) + [r.X, r.U, r.status, r.iters, r.kkt, r.dual] + _device_solve(s, x0, xr, ur)


def test_set_bounds_is_a_fresh_handle():
    """MPC box -> run-time pattern -> MPC box with a tighter input box, at N = 20 (a stage-unrolled build for the MPC
    pattern, the generic one for the other): every solve is that of a fresh handle created with those bounds."""
    from track_patterns import nlp_of
    from ttmpc.scenarios import synthetic_batch
    N = 20
    x0, xr, ur = synthetic_batch(4, N, seed=97, psi_range=0.3)
    mpc, run_time = nlp_of("mpc_diag", N, P), nlp_of("run_time", N, P)
    tight = nlp_of("mpc_diag", N, P, **TIGHT)
    s = _solver(mpc)
    for a, b in zip(s.get_bounds(), (mpc.xlb, mpc.xub, mpc.ulb, mpc.uub)):
        assert np.array_equal(a, b)                                  # round trip, +-inf included
    assert np.isinf(s.get_bounds()[0][0]) and np.isinf(s.get_bounds()[1][0])
    first = _all_solves(s, x0, xr, ur)                               # (the cached small-call marshalling is now in use)
    results = {}
    for name, nlp in (("run_time", run_time), ("tight", tight), ("mpc", mpc)):
        s.set_bounds(nlp.xlb, nlp.xub, nlp.ulb, nlp.uub)
        for a, b, c in zip(s.get_bounds(), s.bounds, (nlp.xlb, nlp.xub, nlp.ulb, nlp.uub)):
            assert np.array_equal(a, c) and np.array_equal(b, c)
        results[name] = _all_solves(s, x0, xr, ur)
        fresh = _all_solves(_solver(nlp), x0, xr, ur)
        for i, (a, b) in enumerate(zip(results[name], fresh)):
            assert np.array_equal(a, b), (name, i)
        assert not results[name][2].any()
    for i, (a, b) in enumerate(zip(results["mpc"], first)):
        assert np.array_equal(a, b), i
    assert not np.array_equal(results["tight"][1], first[1])         # the input box does move the solution
    s.set_bounds(uub=[0.4, 0.03])                                    # a vector left out keeps its values
    got = s.get_bounds()
    assert np.array_equal(got[3], [0.4, 0.03]) and np.array_equal(got[2], mpc.ulb) and np.array_equal(got[0], mpc.xlb)


def test_set_bounds_bad_calls():
    import ttmpc
    from oracle import ttmpc_oracle as to
    from ttmpc._lib import TTError
    nlp = to.TrackingNLP(10, params=dict(P, horizon=10))
    s = _solver(nlp)
    before = s.get_bounds()
    with pytest.raises(TTError, match="lb > ub"):
        s.set_bounds(ulb=[0.5, -1.0], uub=[0.4, 1.0])                # lb > ub
    with pytest.raises(TTError, match="lb > ub"):
        s.set_bounds(xub=[np.inf, np.inf, 3.0, np.nan, 0.7, 10.0])   # a NaN
    with pytest.raises(ValueError):
        s.set_bounds(xlb=[0.0] * 5)                                  # a wrong length
    for a, b, c in zip(s.get_bounds(), before, s.bounds):            # a refused call changes nothing
        assert np.array_equal(a, b) and np.array_equal(c, b)
    dp = C.POINTER(C.c_double)
    four = [np.zeros(6), np.ones(6), np.zeros(2), np.ones(2)]
    ptrs = [a.ctypes.data_as(dp) for a in four]
    assert s._L.tt_set_bounds(None, *ptrs) == -errno.EINVAL and s._L.tt_get_bounds(None, *ptrs) == -errno.EINVAL
    assert s._L.tt_set_bounds(s._h, None, *ptrs[1:]) == -errno.EINVAL
    o = ttmpc.ObcaSolver(10, P, to.DEFAULT_Q, to.DEFAULT_R, to.OBCA_XLB, to.OBCA_XUB, to.MPC_ULB, to.MPC_UUB,
                         np.array([[30.0, 30.0, 4.0, 4.0]]), variant=ttmpc.TT_VARIANT_TRACK_OBCA)
    assert o._L.tt_set_bounds(o._h, *ptrs) == -errno.EINVAL
    assert b"OBCA" in o._L.tt_last_error(o._h)
    assert o._L.tt_get_bounds(o._h, *ptrs) == -errno.EINVAL
    from ttmpc._lib import TTTrackVjpBoundsOut
    bo = TTTrackVjpBoundsOut()
    assert o._L.tt_track_vjp_bounds_device(o._h, 1, *[None] * 9, C.byref(bo), 0, None) == -errno.EINVAL
    assert not hasattr(o, "set_bounds")


# ---- 6 ----------------------------------------------------------------------------------------------------------
def test_kernel_against_oracle_finite_differences():
    """case_active, unweighted, h = 1e-4, bound 1e-5 per entry.  An instance may be left out only if one of its finite
    bounds is weakly active (a relaxed slack in (1e-7, 1e-3) at the oracle's optimum), at most one of the six: on the
    CPU that is instance 0 (slack 1.76e-7, error 2.4e-4 for the dense algebra at the oracle's own optimum)."""
    nlp, x0, xr, ur, w, s, r, gX, gU, v = _case_run("active", False)
    B = x0.shape[0]
    z, st, fd = br.oracle_fd_bounds(nlp, x0, xr, ur, gX, gU, h=1e-4)
    assert np.all(st == 0) and np.all(r.status == 0) and np.all(v.vjp_status == 0)
    left_out, worst, big = [], 0.0, 0.0
    for b in range(B):
        err, weak = np.abs(v.g_bounds[b] - fd[b]), br.weakly_active(nlp, z[b])
        print(f"instance {b}: gpu vs oracle FD per entry max {err.max():.3e}, largest entry {np.abs(fd[b]).max():.3f}, "
              f"weakly active slack {weak}")
        if weak is not None and err.max() > 1e-5:
            left_out.append(b)
            continue
        assert np.all(err <= 1e-5), (b, err)
        worst, big = max(worst, float(err.max())), max(big, float(np.abs(fd[b]).max()))
    print(f"left out {left_out}; worst of the others {worst:.3e}, largest entry {big:.3f}")
    assert len(left_out) <= 1
    assert big > 0.1


# ---- 7 ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _loop_case():
    """loop_vjp_reference.loop_case (B = 3, K = 6, N = 6) with the acceleration capped at 1.25 and the steering rate
    bounded below at -0.16.  In the default box the applied inputs are 1.20 .. 1.32 and -0.169 .. -0.155 (CPU oracle
    loop), so the acceleration saturates from step 2 on and the steering rate up to step 3."""
    c = lv.loop_case(h.golden())
    lo, up = br.box(c["nlp"])
    up[6], lo[7] = 1.25, -0.16
    return dict(c, nlp=br.with_box(c["nlp"], lo, up))


def _loop(*a, **kw):
    return h.loop(_loop_case(), *a, **kw)


GROUPS = ("g_x_init", "g_wq_wr", "g_noise", "g_plan_x", "g_plan_u")


@functools.lru_cache(maxsize=None)
def _loop_run(policy="track", rule=False):
    from ttmpc import simulation as sim
    c = _loop_case()
    loop = _loop(policy, rule=sim.FuzzyRule() if rule else None)
    out = loop.run_tape(c["x_init"], c["T"], noise=c["noise"], wq_wr=None if rule else c["w"])
    g = {k: _n(v) for k, v in loop.backward(out["tape"], _t(c["GS"]), _t(c["GU"]), bounds=True).items()}
    return loop, out, g


def test_loop_sweep_against_chain_and_per_step_calls():
    c = _loop_case()
    loop, out, g = _loop_run()
    tp = h.tape_np(out["tape"])
    assert np.all(out["status"] == 0) and g["g_bounds"].shape == (c["B"], 16)
    z0 = np.concatenate([tp["dual"][:, :, 0, 12:14], tp["dual"][:, :, 0, 20:22]], axis=2)   # the applied inputs' bounds
    cap, rate = z0[..., 2] > 1e-3, z0[..., 1] > 1e-3          # (K,B): the acceleration's cap, the steering rate's floor
    print("steps x instances on the acceleration cap:\n", cap.astype(int), "\non the steering-rate floor:\n",
          rate.astype(int))
    assert cap.any() and not cap.all() and rate.any() and not rate.all()
    nlp = c["nlp"]
    dense = br.chain(c, br.numpy_step_vjp(nlp, vr.dense_vjp, br.dense_bounds_vjp, tp, c), tp)
    model = br.chain(c, br.numpy_step_vjp(nlp, vr.riccati_vjp, br.riccati_bounds_vjp, tp, c), tp)

    def gpu_step(t, Xr, Ur, gU):
        B = gU.shape[0]
        v = loop.solver.vjp(tp["X"][t], tp["U"][t], tp["dual"][t], np.tile(Xr.T, (B, 1, 1)), np.tile(Ur.T, (B, 1, 1)),
                            tp["status"][t], None, gU, wq_wr=c["w"], bounds=True)
        return {"x0": v.g_x0, "xref": v.g_xref, "uref": v.g_uref, "w": v.g_wq_wr, "bounds": v.g_bounds}

    steps = br.chain(c, gpu_step, tp)
    h.compare_with_chain("loop backward", _halves(g["g_bounds"]), _halves(dense["bounds"]), _halves(model["bounds"]),
                         HALVES, per_group=True)
    h.compare_with_chain("per-step calls", _halves(steps["bounds"]), _halves(dense["bounds"]), _halves(model["bounds"]),
                         HALVES, per_group=True)
    print(f"backward vs the sum of the per-step calls: {np.max(np.abs(g['g_bounds'] - steps['bounds'])):.3e}, largest "
          f"entry {np.max(np.abs(g['g_bounds'])):.3e}")
    assert np.max(np.abs(g["g_bounds"])) > 0.1
    assert _exact_zeros(g["g_bounds"], _infinite(nlp))
    plain = loop.backward(out["tape"], _t(c["GS"]), _t(c["GU"]))
    assert sorted(plain) == sorted(GROUPS)
    for k in GROUPS:                                                # the five existing groups: bitwise
        assert np.array_equal(_n(plain[k]), g[k]), k
    both = loop.backward(out["tape"], _t(c["GS"]), _t(c["GU"]), bounds=True, model=True)
    mdl = loop.backward(out["tape"], _t(c["GS"]), _t(c["GU"]), model=True)
    assert np.array_equal(_n(both["g_bounds"]), g["g_bounds"])
    for k in ("g_model_solver", "g_model_plant") + GROUPS:
        assert np.array_equal(_n(both[k]), _n(mdl[k])), k


@pytest.mark.parametrize("policy", ["nmpc", "fuzzy"])
def test_loop_other_policies(policy):
    c = _loop_case()
    loop, out, g = _loop_run(policy)
    tp = h.tape_np(out["tape"])
    assert np.all(out["status"] == 0)
    dense = br.chain(c, br.numpy_step_vjp(c["nlp"], vr.dense_vjp, br.dense_bounds_vjp, tp, c), tp, policy)
    model = br.chain(c, br.numpy_step_vjp(c["nlp"], vr.riccati_vjp, br.riccati_bounds_vjp, tp, c), tp, policy)
    h.compare_with_chain(policy, _halves(g["g_bounds"]), _halves(dense["bounds"]), _halves(model["bounds"]), HALVES,
                         per_group=True)
    assert np.max(np.abs(g["g_bounds"])) > 0.1
    plain = loop.backward(out["tape"], _t(c["GS"]), _t(c["GU"]))
    for k in GROUPS:
        assert np.array_equal(_n(plain[k]), g[k]), k


def test_rule_loop():
    """A loop with a FuzzyRule: bounds=True rides on the same step as rule=True, and neither moves the other's bits."""
    c = _loop_case()
    loop, out, g = _loop_run("track", True)
    assert np.all(out["status"] == 0) and np.max(np.abs(g["g_bounds"])) > 0.1
    GS, GU = _t(c["GS"]), _t(c["GU"])
    plain = loop.backward(out["tape"], GS, GU, rule=True)
    both = loop.backward(out["tape"], GS, GU, rule=True, bounds=True)
    assert np.array_equal(_n(both["g_bounds"]), g["g_bounds"])
    for k in GROUPS + ("g_fuzzy_rule",):
        assert np.array_equal(_n(both[k]), _n(plain[k])), k
    for k in GROUPS:
        assert np.array_equal(_n(plain[k]), g[k]), k


def test_loop_raises():
    import ttmpc
    from oracle import ttmpc_oracle as to
    from ttmpc import simulation as sim
    c = _loop_case()
    loop = _loop()
    out = loop.run_tape(c["x_init"], c["T"], noise=c["noise"], wq_wr=c["w"])
    for a, b in zip(out["tape"].bounds, loop.solver.get_bounds()):
        assert np.array_equal(a, b)
    loop.set_bounds(uub=[1.3, np.pi / 2])
    for kw in ({"bounds": True}, {}):
        with pytest.raises(ValueError, match="bounds changed"):
            loop.backward(out["tape"], _t(c["GS"]), _t(c["GU"]), **kw)
    loop.set_bounds(uub=c["nlp"].uub)
    loop.backward(out["tape"], _t(c["GS"]), _t(c["GU"]), bounds=True)
    obca = ttmpc.ObcaSolver(c["N"], P, to.DEFAULT_Q, to.DEFAULT_R, to.OBCA_XLB, to.OBCA_XUB, to.MPC_ULB, to.MPC_UUB,
                            np.array([[30.0, 30.0, 4.0, 4.0]]), variant=ttmpc.TT_VARIANT_TRACK_OBCA)
    switch = sim.ClosedLoop(h.solver(c["nlp"]), c["plan_x"], c["plan_u"], P, None, obstacles=np.array([[30.0, 30.0, 4.0, 4.0]]),
                            switch_solver=obca, switch_adjoint=True)
    with pytest.raises(ValueError, match="bounds=True"):
        switch.backward(None, None, None, bounds=True)


# ---- 8 ----------------------------------------------------------------------------------------------------------
def test_tracking_layer_with_bounds_tensor():
    import torch
    from ttmpc.diff import DifferentiableTracking, TrackingSolveFunction
    nlp, x0, xr, ur, w, s0, r, gX, gU, v = _case_run("active", True)
    layer = DifferentiableTracking(_solver(nlp))
    tgx, tgu = _t(gX), _t(gU)
    ins = lambda: [_t(a).requires_grad_(True) for a in (x0, xr, ur, w)]  # noqa: E731

    def loss(X, U):
        return (tgx * X).sum() + (tgu * U).sum()

    for dev in ("cpu", "cuda"):
        tb = torch.tensor(_tensor16(nlp), dtype=torch.float64, device=dev, requires_grad=True)
        ts = ins()
        X, U, st = layer(*ts, bounds=tb)
        assert torch.all(st == 0) and np.array_equal(_n(X), r.X)
        loss(X, U).backward()
        assert tb.grad.device == tb.device and tuple(tb.grad.shape) == (16,)
        assert np.array_equal(_n(tb.grad), _n(_t(v.g_bounds).sum(dim=0)))         # the sum over B of the kernel's rows
        for t, k in zip(ts, OUTS[:4]):
            assert np.array_equal(_n(t.grad), getattr(v, k)), k
    # the shorter call forms stand
    ts, tp = ins(), ins()
    X, U, _ = layer(*ts)
    loss(X, U).backward()
    Xp, Up, _ = TrackingSolveFunction.apply(layer.solver, *tp, None)
    loss(Xp, Up).backward()
    for t, u, k in zip(ts, tp, OUTS[:4]):
        assert np.array_equal(_n(t.grad), getattr(v, k)) and np.array_equal(_n(u.grad), getattr(v, k)), k
    # another box is applied to the handle and stays applied; a change before the backward raises
    wide = _tensor16(nlp)
    wide[6:8], wide[14:16] = [-0.5, -0.05], [0.5, 0.05]
    tb = torch.tensor(wide, dtype=torch.float64, requires_grad=True)
    X, U, st = layer(*[_t(a) for a in (x0, xr, ur, w)], bounds=tb)
    assert np.array_equal(layer.solver.get_bounds()[3], [0.5, 0.05]) and not np.array_equal(_n(U), r.U)
    layer.solver.set_bounds(uub=[0.6, 0.05])
    with pytest.raises(RuntimeError, match="bounds changed"):
        loss(X, U).backward()
    with pytest.raises(TypeError, match="float64"):
        layer(*[_t(a) for a in (x0, xr, ur, w)], bounds=torch.tensor(wide, dtype=torch.float32))


def test_saturated_input_has_unit_gradient_in_its_bound():
    """The loss that had no gradient before: L = U[b, k, i] with that input on its bound.  dL/d(bound) = 1 - H / Sigma
    with Sigma = z / slack = z^2 / mu and H the reduced Hessian entry beside it (tens): the entry with the largest
    multiplier of the batch (z above 10 on the CPU oracle, mu = 2.5e-9: 1 - dL/dbound ~ 1e-10) is the one taken."""
    import torch
    from ttmpc.diff import DifferentiableTracking
    nlp, x0, xr, ur, w, s0, r, gX, gU, v = _case_run("active", False)
    zin = np.stack([r.dual[:, :-1, 12:14], r.dual[:, :-1, 20:22]], axis=-1)        # (B, N, i, lower | upper)
    b, k, i, side = np.unravel_index(np.argmax(zin), zin.shape)
    entry = (6 if side == 0 else 14) + i
    layer = DifferentiableTracking(_solver(nlp))
    tb = torch.tensor(_tensor16(nlp), dtype=torch.float64, device="cuda", requires_grad=True)
    tx = _t(x0).requires_grad_(True)
    X, U, st = layer(tx, _t(xr), _t(ur), bounds=tb)
    (g, gx) = torch.autograd.grad(U[b, k, i], [tb, tx])
    g = _n(g)
    print(f"U[{b},{k},{i}] = {float(U[b, k, i].detach()):.6f} on bound entry {entry} = {float(tb[entry].detach()):.6f}, multiplier "
          f"{zin[b, k, i, side]:.3e}: dL/dbounds[{entry}] = 1 - {1.0 - g[entry]:.3e}, largest other entry "
          f"{np.max(np.abs(np.delete(g, entry))):.3e}, largest dL/dx_init {np.max(np.abs(_n(gx))):.3e}")
    assert zin[b, k, i, side] > 1.0 and abs(float(U[b, k, i].detach()) - float(tb[entry].detach())) < 1e-6
    assert abs(g[entry] - 1.0) <= 1e-6
    assert np.max(np.abs(np.delete(g, entry))) <= 1e-6


def test_closed_loop_layer_with_bounds_tensor():
    import torch
    from ttmpc.diff import DifferentiableClosedLoop
    c = _loop_case()
    loop, out, g = _loop_run()
    gb = _n(_t(g["g_bounds"]).sum(dim=0))
    layer = DifferentiableClosedLoop(_loop())
    GS, GU = _t(c["GS"]), _t(c["GU"])
    for dev in ("cpu", "cuda"):
        tb = torch.tensor(_tensor16(c["nlp"]), dtype=torch.float64, device=dev, requires_grad=True)
        x, w = _t(c["x_init"]).requires_grad_(True), _t(c["w"]).requires_grad_(True)
        S, Ua, st = layer(x, c["T"], wq_wr=w, noise=_t(c["noise"]), bounds=tb)
        assert torch.all(st == 0) and np.array_equal(_n(S), out["states"])
        ((GS * S).sum() + (GU * Ua).sum()).backward()
        assert tb.grad.device == tb.device and np.array_equal(_n(tb.grad), gb)
        assert np.array_equal(_n(x.grad), g["g_x_init"]) and np.array_equal(_n(w.grad), g["g_wq_wr"])
    # the old call form: the gradients of before
    x, w = _t(c["x_init"]).requires_grad_(True), _t(c["w"]).requires_grad_(True)
    S, Ua, st = layer(x, c["T"], wq_wr=w, noise=_t(c["noise"]))
    ((GS * S).sum() + (GU * Ua).sum()).backward()
    assert np.array_equal(_n(x.grad), g["g_x_init"]) and np.array_equal(_n(w.grad), g["g_wq_wr"])
