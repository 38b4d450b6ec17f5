"""GPU suite: gradients in the model geometry (L1, L2, M): track_vjp_kernel's model instantiation behind
tt_track_vjp_model*, tt_set_model / tt_get_model, tt_policy_plant_vjp_model_device, ClosedLoop.backward(model=True) and
the ``model`` / ``plant_model`` tensors of ttmpc.diff.

1. The kernel against dense algebra on the GPU's own duals (the numpy recursion as the yardstick) and against central
   differences of the CPU oracle; against dense algebra under every weight form and bound pattern of
   tests/track_patterns.py, its other four outputs bitwise those of the plain instantiation.
2. Horizons, grid indexing, determinism.
3. Neutrality: the other outputs with g_model, the NULL g_model call, the host call.
4. accumulate, failed solves, a NaN upstream gradient.
5. tt_set_model against fresh handles, bit for bit; bad calls.
6. The plant adjoint's model term against the numpy model.
7. The closed loop's sweep against the numpy chain; neutrality, grid, determinism, failure branches.
8. Autograd: the layers are the calls; shared geometry; a directional check through set_model; a short descent.

Every case prints its figures before it asserts (DESIGN.md "Adjoint in the model geometry" records them).
"""
import ctypes as C
import errno
import functools

import numpy as np
import pytest

import loop_vjp_reference as lv
import model_vjp_reference as mr
import sens_reference as sr
import vjp_harness as h
import vjp_reference as vr
from track_patterns import DERIVATIVE_CASES

pytestmark = pytest.mark.gpu

P = sr.P
NEW = (7.3, 12.0, 0.25)
OUTS = ("g_x0", "g_xref", "g_uref", "g_wq_wr", "vjp_status")
# what tests/test_model_vjp_reference.py measured for dense_model_vjp against the oracle's central differences (the
# largest of L1, L2, M; the oracle solved to model_vjp_reference.ORACLE_FD_TOL)
CPU_FD_ERR = {("free", False): 3.3e-10, ("free", True): 4.3e-10, ("active", False): 4.6e-10, ("active", True): 5.2e-9}


_t, _n, _solver, _w, _golden = h.t, h.n, h.solver, h.w_of, h.golden


@functools.lru_cache(maxsize=None)
def _case_run(name, weighted):
    nlp, x0, xr, ur = sr.case_free() if name == "free" else sr.case_active()
    B = x0.shape[0]
    w = vr.random_weights(B) if weighted else None
    s = _solver(nlp, tol=mr.ORACLE_FD_TOL)   # the optimum the oracle's differences are taken at (the comment there)
    r = s.solve_ex(x0, xr, ur, wq_wr=w, duals=True, gain=False)
    gX, gU = vr.random_upstream(B, nlp.N)
    v = s.vjp(r.X, r.U, r.dual, xr, ur, r.status, gX, gU, wq_wr=w, model=True)
    return nlp, x0, xr, ur, w, s, r, gX, gU, v


# ---- 1 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name", ["free", "active"])
def test_kernel_against_dense_algebra_and_oracle(name, weighted):
    """Both sides are solved to ``model_vjp_reference.ORACLE_FD_TOL``.  At the default 1e-8 one weakly active bound of
    [active-True] is undecided on both (an input 1.5e-6 inside its bound), and the two end points' derivatives differ by
    1.4e-4 in dL/dL1 although the kernel agrees with dense algebra on its own duals to 4e-16; with the GPU at 1e-10,
    1e-11, 1e-12 against the oracle at 1e-12 the difference is 9.9e-7, 1.8e-8, 1.9e-9."""
    from ttmpc import layout
    nlp, x0, xr, ur, w, s, r, gX, gU, v = _case_run(name, weighted)
    assert np.all(r.status == 0) and np.all(v.vjp_status == 0)
    assert v["model"].shape == (x0.shape[0], 3)
    zz = layout.pack(r.X, r.U)
    err_gpu = err_model = smax = err_y0 = 0.0
    for b in range(x0.shape[0]):
        dense = mr.dense_model_vjp(nlp, zz[b], r.dual[b], gX[b], gU[b], *_w(w, b), cond=False)
        model = mr.riccati_model_vjp(nlp, zz[b], r.dual[b], gX[b], gU[b], *_w(w, b))
        assert model["ok"]
        err_gpu = max(err_gpu, float(np.max(np.abs(v.g_model[b] - dense["model"]))))
        err_model = max(err_model, float(np.max(np.abs(model["model"] - dense["model"]))))
        err_y0 = max(err_y0, float(np.max(np.abs(model["ly0"] - v.g_x0[b]))))
        smax = max(smax, float(np.max(np.abs(dense["model"]))))
    print(f"{name} weighted={weighted}: err_gpu {err_gpu:.3e}, err_model {err_model:.3e}, max|ref| {smax:.3e}; "
          f"numpy lam_y,0 vs the kernel's g_x0 {err_y0:.3e}")
    assert smax > 1e-3
    assert err_gpu <= 10.0 * err_model + 1e-12 * smax
    z, st, fd = mr.oracle_fd_model(nlp, x0, xr, ur, gX, gU, w=w, h=1e-4)
    assert np.all(st == 0)
    worst, bound = np.max(np.abs(fd - v.g_model), axis=0), min(10.0 * CPU_FD_ERR[(name, weighted)], 1e-5)
    print(f"{name} weighted={weighted}: gpu vs oracle FD (L1, L2, M) {worst} (bound {bound:.1e}), largest entries "
          f"{np.max(np.abs(v.g_model), axis=0)}")
    assert np.max(worst) <= bound


@pytest.mark.parametrize("name,pattern,weighted", DERIVATIVE_CASES)
def test_kernel_against_dense_algebra_patterns(name, pattern, weighted):
    from ttmpc import layout
    nlp, x0, xr, ur = sr.case(name, pattern)
    B = x0.shape[0]
    w = vr.random_weights(B) if weighted else None
    s = _solver(nlp)
    r = s.solve_ex(x0, xr, ur, wq_wr=w, duals=True, gain=False)
    gX, gU = vr.random_upstream(B, nlp.N)
    v = s.vjp(r.X, r.U, r.dual, xr, ur, r.status, gX, gU, wq_wr=w, model=True)
    plain = s.vjp(r.X, r.U, r.dual, xr, ur, r.status, gX, gU, wq_wr=w)
    assert np.all(r.status == 0) and np.all(v.vjp_status == 0)
    for k in OUTS:
        assert np.array_equal(getattr(v, k), getattr(plain, k)), k
    zz = layout.pack(r.X, r.U)
    err_gpu = err_model = smax = 0.0
    for b in range(B):
        dense = mr.dense_model_vjp(nlp, zz[b], r.dual[b], gX[b], gU[b], *_w(w, b), cond=False)
        model = mr.riccati_model_vjp(nlp, zz[b], r.dual[b], gX[b], gU[b], *_w(w, b))
        assert model["ok"]
        err_gpu = max(err_gpu, float(np.max(np.abs(v.g_model[b] - dense["model"]))))
        err_model = max(err_model, float(np.max(np.abs(model["model"] - dense["model"]))))
        smax = max(smax, float(np.max(np.abs(dense["model"]))))
    print(f"{name} {pattern} weighted={weighted}: err_gpu {err_gpu:.3e}, err_model {err_model:.3e}, max|ref| {smax:.3e}")
    assert smax > 1e-3
    assert err_gpu <= 10.0 * err_model + 1e-12 * smax


# ---- 2 ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _horizon_run(N):
    from oracle import ttmpc_oracle as to
    from ttmpc.scenarios import synthetic_batch
    nlp = to.TrackingNLP(N, params=dict(P, horizon=N))
    x0, xr, ur = synthetic_batch(4, N, seed=4000 + N, psi_range=0.3)
    s = _solver(nlp, tol=1e-8)
    r = s.solve_ex(x0, xr, ur, duals=True, gain=False)
    gX, gU = vr.random_upstream(4, N, seed=N)
    v = s.vjp(r.X, r.U, r.dual, xr, ur, r.status, gX, gU, model=True)
    return nlp, x0, xr, ur, s, r, gX, gU, v


@pytest.mark.parametrize("N", [1, 2, 20, 63, 64, 170])
def test_horizons(N):
    from ttmpc import layout
    nlp, x0, xr, ur, s, r, gX, gU, v = _horizon_run(N)
    zz = layout.pack(r.X, r.U)
    print(f"N={N}: status {r.status.tolist()}, vjp_status {v.vjp_status.tolist()}")
    assert not r.status.any() and not v.vjp_status.any()
    err_gpu = err_model = smax = 0.0
    for b in range(4):
        dense = mr.dense_model_vjp(nlp, zz[b], r.dual[b], gX[b], gU[b], cond=False)
        model = mr.riccati_model_vjp(nlp, zz[b], r.dual[b], gX[b], gU[b])
        assert model["ok"]
        err_gpu = max(err_gpu, float(np.max(np.abs(v.g_model[b] - model["model"]))))
        err_model = max(err_model, float(np.max(np.abs(model["model"] - dense["model"]))))
        smax = max(smax, float(np.max(np.abs(model["model"]))))
    print(f"N={N}: gpu vs numpy recursion {err_gpu:.3e}, recursion vs dense {err_model:.3e}, max|g_model| {smax:.3e}")
    assert smax > 1e-4
    assert err_gpu <= 10.0 * err_model + 1e-12 * smax


def test_grid_indexing_and_determinism():
    """One B = 2304 launch on 576 copies of the N = 20 batch; two launches on one input."""
    nlp, x0, xr, ur, s, r, gX, gU, v = _horizon_run(20)
    rep = lambda a: np.tile(a, (576,) + (1,) * (a.ndim - 1))  # noqa: E731
    big = s.vjp(rep(r.X), rep(r.U), rep(r.dual), rep(xr), rep(ur), rep(r.status), rep(gX), rep(gU), model=True)
    again = s.vjp(r.X, r.U, r.dual, xr, ur, r.status, gX, gU, model=True)
    for k in OUTS + ("g_model",):
        got, ref = getattr(big, k), getattr(v, k)
        assert got.shape[0] == 2304
        assert np.array_equal(got[:4], ref), k
        assert np.array_equal(got, rep(ref)), k
        assert np.array_equal(getattr(again, k), ref), k
    assert np.max(np.abs(v.g_model)) > 0.0


# ---- 3, 4 -------------------------------------------------------------------------------------------------------
def _device_vjp(s, r, xr, ur, gX, gU, w=None, mode="plain", g_model=None, accumulate=False):
    """One device call on fresh buffers: mode "plain" (tt_track_vjp_device), "model" (g_model given) or "null"
    (tt_track_vjp_model_device with g_model == NULL).  -> dict of numpy outputs."""
    import torch
    from ttmpc._lib import TTTrackVjpModelOut
    B, N = r.X.shape[0], s.N
    ins = [_t(a) for a in (r.X, r.U, r.dual, xr, ur)]
    st, tgx, tgu = _t(r.status, torch.int32), _t(gX), _t(gU)
    tw = None if w is None else _t(w)
    outs = [torch.full(sh, np.nan, dtype=torch.float64, device="cuda") for sh in ((B, 6), (B, N + 1, 6), (B, N, 2), (B, 8))]
    vst = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    gm = None if g_model is None else _t(g_model)
    ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    if mode == "null":
        mo = TTTrackVjpModelOut(*[o.data_ptr() for o in outs], None, vst.data_ptr())
        rc = s._L.tt_track_vjp_model_device(s._h, B, *[t.data_ptr() for t in ins], ptr(tw) or None, st.data_ptr(),
                                            tgx.data_ptr(), tgu.data_ptr(), C.byref(mo), 1, None)
        assert rc == 0
    else:
        s.vjp_device(B, *[t.data_ptr() for t in ins[:3]], ins[3].data_ptr(), ins[4].data_ptr(), st.data_ptr(),
                     grad_x=tgx.data_ptr(), grad_u=tgu.data_ptr(), g_x0=outs[0].data_ptr(), g_xref=outs[1].data_ptr(),
                     g_uref=outs[2].data_ptr(), g_wq_wr=outs[3].data_ptr(), vjp_status=vst.data_ptr(), wq_wr=ptr(tw),
                     g_model=ptr(gm) if mode == "model" else 0, accumulate=accumulate)
    torch.cuda.synchronize()
    d = {k: _n(o) for k, o in zip(OUTS, outs + [vst])}
    d["g_model"] = None if gm is None else _n(gm)
    return d


@pytest.mark.parametrize("weighted", [False, True])
def test_neutrality(weighted):
    nlp, x0, xr, ur, w, s, r, gX, gU, v = _case_run("active", weighted)
    B = x0.shape[0]
    plain = _device_vjp(s, r, xr, ur, gX, gU, w)
    model = _device_vjp(s, r, xr, ur, gX, gU, w, "model", np.full((B, 3), np.nan))
    null = _device_vjp(s, r, xr, ur, gX, gU, w, "null")
    for k in OUTS:
        assert np.array_equal(model[k], plain[k]), k        # the other four outputs and vjp_status: the plain call's
        assert np.array_equal(null[k], plain[k]), k         # g_model == NULL: the plain call
        assert np.array_equal(getattr(v, k), plain[k]), k   # the host call: the device call
    assert np.array_equal(v.g_model, model["g_model"])
    assert not plain["vjp_status"].any() and np.max(np.abs(model["g_model"])) > 1e-3
    old = s.vjp(r.X, r.U, r.dual, xr, ur, r.status, gX, gU, wq_wr=w)
    assert type(old).__name__ == "TrackVjpResult" and old.g_model is None           # the old call asks for no g_model
    for k in OUTS:
        assert np.array_equal(getattr(old, k), plain[k]), k


def test_accumulate_and_failures():
    from oracle import ttmpc_oracle as to
    from ttmpc.scenarios import synthetic_batch
    N, B = 12, 5
    nlp = to.TrackingNLP(N, params=dict(P, horizon=N))
    x0, xr, ur = synthetic_batch(B, N, seed=8)
    s = _solver(nlp)
    gX, gU = vr.random_upstream(B, N)
    good = s.solve_ex(x0, xr, ur, gain=False)
    assert list(good.status) == [0] * B
    pre = np.random.default_rng(2).uniform(-1.0, 1.0, (B, 3))
    once = _device_vjp(s, good, xr, ur, gX, gU, None, "model", np.full((B, 3), np.nan))
    val = once["g_model"]
    assert not once["vjp_status"].any() and np.max(np.abs(val)) > 1e-4
    acc1 = _device_vjp(s, good, xr, ur, gX, gU, None, "model", pre, accumulate=True)["g_model"]
    acc2 = _device_vjp(s, good, xr, ur, gX, gU, None, "model", acc1, accumulate=True)["g_model"]
    assert np.array_equal(acc1, pre + val) and np.array_equal(acc2, (pre + val) + val)
    # a failed solve (x_init outside the box): status 3 -> vjp_status 2
    x0b = x0.copy()
    x0b[1, 3] = 1.3            # hitch angle beyond pi/3
    x0b[3, 2] = 4.0            # heading beyond pi
    r = s.solve_ex(x0b, xr, ur, gain=False)
    assert list(r.status) == [0, 3, 0, 3, 0]
    wr = _device_vjp(s, r, xr, ur, gX, gU, None, "model", np.full((B, 3), np.nan))
    ac = _device_vjp(s, r, xr, ur, gX, gU, None, "model", pre, accumulate=True)
    assert list(wr["vjp_status"]) == [0, 2, 0, 2, 0] and list(ac["vjp_status"]) == [0, 2, 0, 2, 0]
    for b in (1, 3):
        assert not wr["g_model"][b].any()                          # zeros for accumulate = 0
        assert np.array_equal(ac["g_model"][b], pre[b])            # an untouched accumulator for accumulate = 1
    for b in (0, 2, 4):
        assert np.array_equal(wr["g_model"][b], val[b])
        assert np.array_equal(ac["g_model"][b], pre[b] + val[b])
    # a NaN in one instance's upstream gradient: that instance alone is undefined
    gXn = gX.copy()
    gXn[2, 5, 1] = np.nan
    nw = _device_vjp(s, good, xr, ur, gXn, gU, None, "model", np.full((B, 3), np.nan))
    na = _device_vjp(s, good, xr, ur, gXn, gU, None, "model", pre, accumulate=True)
    assert list(nw["vjp_status"]) == [0, 0, 1, 0, 0]
    assert not nw["g_model"][2].any() and np.array_equal(na["g_model"][2], pre[2])
    for b in (0, 1, 3, 4):
        assert np.array_equal(nw["g_model"][b], val[b])
        for k in OUTS[:4]:
            assert np.array_equal(nw[k][b], once[k][b]), (b, k)


# ---- 5 ----------------------------------------------------------------------------------------------------------
def _all_calls(s, x0, xr, ur, gX, gU):
    """solve, solve_ex (duals and gain) and vjp (with the model gradient) of one solver: a flat list of arrays."""
    out = list(s.solve(x0, xr, ur))
    r = s.solve_ex(x0, xr, ur, duals=True, gain=True)
    out += [r.X, r.U, r.status, r.iters, r.kkt, r.dual, r.gain, r.sens_status]
    v = s.vjp(r.X, r.U, r.dual, xr, ur, r.status, gX, gU, model=True)
    return out + [getattr(v, k) for k in OUTS + ("g_model",)]


@pytest.mark.parametrize("N", [20, 8])
def test_set_model_is_a_fresh_handle(N):
    """N = 20 is a stage-unrolled build, N = 8 the generic one; B = 4 host calls take the zero-copy path, which is
    called once before the change so that its cached marshalling is exercised."""
    from oracle import ttmpc_oracle as to
    from ttmpc.scenarios import synthetic_batch
    nlp = to.TrackingNLP(N, params=dict(P, horizon=N))
    x0, xr, ur = synthetic_batch(4, N, seed=77 + N, psi_range=0.3)
    gX, gU = vr.random_upstream(4, N)
    s = _solver(nlp)
    assert s.model() == (P["L1"], P["L2"], P["M"])
    first = _all_calls(s, x0, xr, ur, gX, gU)
    s.set_model(*NEW)
    assert s.model() == NEW
    changed = _all_calls(s, x0, xr, ur, gX, gU)
    fresh = _all_calls(_solver(nlp, dict(P, L1=NEW[0], L2=NEW[1], M=NEW[2])), x0, xr, ur, gX, gU)
    for i, (a, b) in enumerate(zip(changed, fresh)):
        assert np.array_equal(a, b), i
    assert not np.array_equal(changed[0], first[0])                 # the geometry does move the solution
    assert not changed[2].any()
    s.set_model(L1=P["L1"], L2=P["L2"], M=P["M"])
    back = _all_calls(s, x0, xr, ur, gX, gU)
    for i, (a, b) in enumerate(zip(back, first)):
        assert np.array_equal(a, b), i
    s.set_model(L2=NEW[1])                                          # a value left out keeps its current one
    assert s.model() == (P["L1"], NEW[1], P["M"])


def test_set_model_bad_calls():
    import ttmpc
    from oracle import ttmpc_oracle as to
    from ttmpc._lib import TTError
    nlp = to.TrackingNLP(10, params=dict(P, horizon=10))
    s = _solver(nlp)
    for bad in ((0.0, 12.0, 0.1), (7.0, -1.0, 0.1), (7.0, 12.0, np.nan), (np.inf, 12.0, 0.1)):
        assert s._L.tt_set_model(s._h, *bad) == -errno.EINVAL
    with pytest.raises(TTError, match="L1, L2"):
        s.set_model(L1=0.0)
    assert s.model() == (P["L1"], P["L2"], P["M"])                  # a refused call changes nothing
    assert s._L.tt_set_model(None, *NEW) == -errno.EINVAL and s._L.tt_get_model(None, None, None, None) == -errno.EINVAL
    o = ttmpc.ObcaSolver(10, P, to.DEFAULT_Q, to.DEFAULT_R, to.OBCA_XLB, to.OBCA_XUB, to.MPC_ULB, to.MPC_UUB,
                         np.array([[30.0, 30.0, 4.0, 4.0]]), variant=ttmpc.TT_VARIANT_TRACK_OBCA)
    assert o._L.tt_set_model(o._h, *NEW) == -errno.EINVAL
    assert b"OBCA" in o._L.tt_last_error(o._h)


# ---- 6 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("disturbed", [False, True])
@pytest.mark.parametrize("policy", ["track", "nmpc", "fuzzy"])
def test_plant_model_term_against_numpy_model(policy, disturbed):
    """B = 300 (two 256-thread blocks), the states, statuses and flags of test_gpu_loop_vjp's plant test."""
    import torch
    from ttmpc import simulation as sim
    B, N = 300, 5
    rng = np.random.default_rng(17)
    q = np.tile(_golden()["q"], (5, 1))[:B]
    a, abar, GU = rng.uniform(-1, 1, (B, 6)), rng.uniform(-1, 1, (B, 2)), rng.uniform(-1, 1, (B, 2))
    status = rng.choice([0, 1, 2, 3], size=B).astype(np.int32)
    before = (rng.uniform(size=B) > 0.15).astype(np.int32)
    after = (before & (rng.uniform(size=B) > 0.15)).astype(np.int32)
    count = rng.integers(0, 36, size=B).astype(np.int32)
    acc0 = rng.uniform(-1, 1, (B, 3))
    dist = lv.DIST if disturbed else None
    moved = (before != 0) & (after != 0)
    term = np.where(moved[:, None], mr.plant_model_vjp(q, a, P, dist), 0.0)

    def call(g_model):
        ta, tabar = _t(a), _t(abar)
        gu = torch.full((B, N, 2), 7.0, dtype=torch.float64, device="cuda")
        gn = torch.full((B, 6), 7.0, dtype=torch.float64, device="cuda")
        sim.policy_plant_vjp(_t(q), _t(status, torch.int32), _t(after, torch.int32), _t(count, torch.int32), ta, tabar,
                             gu, P, dist, policy=policy, active_before=_t(before, torch.int32), grad_u_applied=_t(GU),
                             g_state_noise=gn, g_model=g_model)
        torch.cuda.synchronize()
        return [_n(t) for t in (ta, tabar, gu, gn)]

    gm = _t(acc0)
    with_model, plain = call(gm), call(None)
    got = _n(gm)
    err = float(np.max(np.abs(got - (acc0 + term))))
    print(f"{policy} disturbed={disturbed}: model term {err:.3e}, largest {np.max(np.abs(term)):.3e}; moved "
          f"{int(moved.sum())}, stopped {int((~moved).sum())}")
    assert err <= 1e-13
    assert np.max(np.abs(term)) > 1e-4
    assert np.array_equal(got[~moved], acc0[~moved])                # stopped and inactive instances add exactly 0
    for x, y in zip(with_model, plain):                             # the existing outputs: the existing call's bits
        assert np.array_equal(x, y)


# ---- 7 ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case():
    return lv.loop_case(_golden())


def _loop(*a, **kw):
    return h.loop(_case(), *a, **kw)


GROUPS = ("g_x_init", "g_wq_wr", "g_noise", "g_plan_x", "g_plan_u")


@functools.lru_cache(maxsize=None)
def _run(policy="track", in_plant=False, fail=False):
    c = _case()
    noise = c["noise"].copy()
    if fail:
        noise[2, 0, 5] += 100.0
        noise[0, 1, 5] += 100.0
    loop = _loop(policy, in_plant)
    out = loop.run_tape(c["x_init"], c["T"], noise=noise, wq_wr=c["w"])
    g = {k: _n(v) for k, v in loop.backward(out["tape"], _t(c["GS"]), _t(c["GU"]), model=True).items()}
    return loop, out, g


def _compare_with_chain(tag, policy, in_plant, out, g):
    c, tp = _case(), h.tape_np(out["tape"])
    dense, model = ({k: v[f"model_{k}"] for k in ("solver", "plant")} for v in
                    (mr.chain(c, fn, tp, policy, in_plant) for fn in (mr.dense_model_vjp, mr.riccati_model_vjp)))
    got = {k: g[f"g_model_{k}"] for k in ("solver", "plant")}
    return max(h.compare_with_chain(tag, got, dense, model, ("solver", "plant"), per_group=True).values())


@pytest.mark.parametrize("in_plant", [False, True])
def test_sweep_against_numpy_chain(in_plant):
    c = _case()
    loop, out, g = _run("track", in_plant)
    assert np.all(out["status"] == 0)
    assert g["g_model_solver"].shape == (c["B"], 3) and g["g_model_plant"].shape == (c["B"], 3)
    assert _compare_with_chain(f"in_plant={in_plant}", "track", in_plant, out, g) > 1e-3
    assert np.max(np.abs(g["g_model_solver"])) > 1e-5
    plain = loop.backward(out["tape"], _t(c["GS"]), _t(c["GU"]))
    assert sorted(plain) == sorted(GROUPS)
    for k in GROUPS:                                                # the five existing groups: bitwise
        assert np.array_equal(_n(plain[k]), g[k]), k


@pytest.mark.parametrize("policy", ["track", "nmpc", "fuzzy"])
def test_failure_branches(policy):
    loop, out, g = _run(policy, False, fail=True)
    st = out["status"]
    assert st[2, 0] == 3 and st[0, 1] == 3 and int((st > 1).sum()) == 2
    _compare_with_chain(policy, policy, False, out, g)


def test_grid_and_determinism():
    c = _case()
    R = 100
    rep = lambda a, ax=0: np.concatenate([a] * R, axis=ax)  # noqa: E731
    small = _loop(per_instance=3)
    o3 = small.run_tape(c["x_init"], c["T"], noise=c["noise"], wq_wr=c["w"])
    g3 = small.backward(o3["tape"], _t(c["GS"]), _t(c["GU"]), model=True)
    big = _loop(per_instance=3 * R)
    o = big.run_tape(rep(c["x_init"]), c["T"], noise=rep(c["noise"], 1), wq_wr=rep(c["w"]))
    GS, GU = _t(rep(c["GS"], 1)), _t(rep(c["GU"], 1))
    g = big.backward(o["tape"], GS, GU, model=True)
    again = big.backward(o["tape"], GS, GU, model=True)
    shared = _run("track", False)[2]
    for k in ("g_model_solver", "g_model_plant"):
        assert _n(g[k]).shape == (3 * R, 3)
        assert np.array_equal(_n(g[k]), rep(_n(g3[k]))), k
        assert np.array_equal(_n(g[k]), _n(again[k])), k
        assert np.array_equal(_n(g3[k]), shared[k]), k             # a shared plan changes nothing per instance
        assert np.max(np.abs(_n(g3[k]))) > 0.0


def test_backward_raises_after_a_change():
    c = _case()
    loop = _loop()
    out = loop.run_tape(c["x_init"], c["T"], noise=c["noise"], wq_wr=c["w"])
    assert out["tape"].model_solver == (P["L1"], P["L2"], P["M"]) and out["tape"].model_plant == out["tape"].model_solver
    loop.set_model(solver=NEW)
    with pytest.raises(ValueError, match="geometry changed"):
        loop.backward(out["tape"], _t(c["GS"]), _t(c["GU"]), model=True)
    loop.set_model(solver=(P["L1"], P["L2"], P["M"]), plant=NEW)
    with pytest.raises(ValueError, match="geometry changed"):
        loop.backward(out["tape"], _t(c["GS"]), _t(c["GU"]))
    with pytest.raises(ValueError, match="L1, L2"):
        loop.set_model(plant=(0.0, 1.0, 0.0))
    loop.set_model(plant=(P["L1"], P["L2"], P["M"]))
    loop.backward(out["tape"], _t(c["GS"]), _t(c["GU"]), model=True)
    # a loop whose plant differs from the controller's model runs the plant with its own geometry
    other = _loop(params=dict(P, L2=P["L2"] + 0.5))
    o2 = other.run_tape(c["x_init"], c["T"], noise=c["noise"], wq_wr=c["w"])
    loop.set_model(plant=(P["L1"], P["L2"] + 0.5, P["M"]))
    o3 = loop.run_tape(c["x_init"], c["T"], noise=c["noise"], wq_wr=c["w"])
    assert np.array_equal(o2["states"], o3["states"]) and not np.array_equal(o2["states"], out["states"])


# ---- 8 ----------------------------------------------------------------------------------------------------------
def test_tracking_layer_with_model_tensor():
    import torch
    from ttmpc.diff import DifferentiableTracking, TrackingSolveFunction
    nlp, x0, xr, ur, w, s0, r, gX, gU, v = _case_run("free", True)
    B, N = x0.shape[0], nlp.N
    s = _solver(nlp, tol=mr.ORACLE_FD_TOL)      # as the shared run, whose bits the layer must return
    layer = DifferentiableTracking(s)
    tgx, tgu = _t(gX), _t(gU)
    ins = lambda: [_t(a).requires_grad_(True) for a in (x0, xr, ur, w)]  # noqa: E731

    def loss(X, U):
        return (tgx * X).sum() + (tgu * U).sum()

    for dev in ("cpu", "cuda"):
        th = torch.tensor([P["L1"], P["L2"], P["M"]], dtype=torch.float64, device=dev, requires_grad=True)
        ts = ins()
        X, U, st = layer(*ts, model=th)
        assert torch.all(st == 0) and np.array_equal(_n(X), r.X)
        loss(X, U).backward()
        assert th.grad.device == th.device and tuple(th.grad.shape) == (3,)
        assert np.array_equal(_n(th.grad), _n(_t(v.g_model).sum(dim=0)))          # the sum over B of the kernel's
        for t, k in zip(ts, OUTS[:4]):
            assert np.array_equal(_n(t.grad), getattr(v, k)), k
    # the old call forms return what they return: no model argument, and the positional apply
    ts = ins()
    X, U, st = layer(*ts)
    loss(X, U).backward()
    tp = ins()
    Xp, Up, _ = TrackingSolveFunction.apply(s, *tp, None)
    loss(Xp, Up).backward()
    for t, u, k in zip(ts, tp, OUTS[:4]):
        assert np.array_equal(_n(t.grad), getattr(v, k)) and np.array_equal(_n(u.grad), getattr(v, k)), k
    # another geometry is applied to the handle and stays applied
    th = torch.tensor(NEW, dtype=torch.float64, requires_grad=True)
    X, U, st = layer(*[_t(a) for a in (x0, xr, ur, w)], model=th)
    assert s.model() == NEW and not np.array_equal(_n(X), r.X)
    s.set_model(L1=7.0)
    with pytest.raises(RuntimeError, match="geometry changed"):
        loss(X, U).backward()
    with pytest.raises(TypeError, match="float64"):
        layer(*[_t(a) for a in (x0, xr, ur, w)], model=torch.tensor(NEW, dtype=torch.float32))


def _layer_loss(layer, c, model=None, plant_model=None, grad=True):
    import torch
    GS, GU = _t(c["GS"]), _t(c["GU"])
    with torch.enable_grad() if grad else torch.no_grad():
        S, Ua, st = layer(_t(c["x_init"]), c["T"], wq_wr=_t(c["w"]), noise=_t(c["noise"]), model=model,
                          plant_model=plant_model)
        assert torch.all(st == 0)
        return (GS * S).sum() + (GU * Ua).sum(), S


def test_closed_loop_layer_with_model_tensors():
    import torch
    from ttmpc.diff import DifferentiableClosedLoop
    c = _case()
    loop, out, g = _run("track", False)
    gs, gp = _t(g["g_model_solver"]).sum(dim=0), _t(g["g_model_plant"]).sum(dim=0)
    layer = DifferentiableClosedLoop(_loop())
    th = lambda dev="cpu": torch.tensor([P["L1"], P["L2"], P["M"]], dtype=torch.float64, device=dev,  # noqa: E731
                                        requires_grad=True)
    ts, tp = th(), th("cuda")
    L, S = _layer_loss(layer, c, ts, tp)
    assert np.array_equal(_n(S), out["states"])
    L.backward()
    assert ts.grad.device.type == "cpu" and tp.grad.device.type == "cuda"
    assert np.array_equal(_n(ts.grad), _n(gs)) and np.array_equal(_n(tp.grad), _n(gp))
    only = th()
    _layer_loss(layer, c, None, only)[0].backward()                 # one of the two alone
    assert np.array_equal(_n(only.grad), _n(gp))
    both = th("cuda")
    _layer_loss(layer, c, both, both)[0].backward()                 # a geometry controller and plant share
    assert np.array_equal(_n(both.grad), _n(gs + gp))
    # the old call form: the five gradients of before, bit for bit
    x, w = _t(c["x_init"]).requires_grad_(True), _t(c["w"]).requires_grad_(True)
    S, Ua, st = layer(x, c["T"], wq_wr=w, noise=_t(c["noise"]))
    ((_t(c["GS"]) * S).sum() + (_t(c["GU"]) * Ua).sum()).backward()
    assert np.array_equal(_n(x.grad), g["g_x_init"]) and np.array_equal(_n(w.grad), g["g_wq_wr"])
    # directional check, the GPU loop against itself through set_model: along -g / |g| of the solver's geometry
    gv = _n(gs)
    d = -gv / np.linalg.norm(gv)
    eps, Ls = 1e-3, []
    base = np.array([P["L1"], P["L2"], P["M"]])
    for sgn in (1.0, -1.0):
        Ls.append(float(_layer_loss(layer, c, torch.tensor(base + sgn * eps * d), None, grad=False)[0]))
    fd, an = (Ls[0] - Ls[1]) / (2 * eps), float(np.sum(gv * d))
    print(f"directional derivative along -g_model: finite difference {fd:.6e}, g . d {an:.6e}, relative "
          f"{abs(fd - an) / abs(an):.3e}")
    assert fd < 0.0 and abs(fd - an) <= 1e-3 * abs(an)


# The loss below is a mean over 7 x 3 x 6 squared distances of a tracking loop that hardly notices the mismatch: 2.5e-14
# at the start, its gradient 1.4e-12 in L1.  The CPU oracle loop's own descent (central differences of the same loss) is
# monotone over five steps at 1e9, 1e10 and 3e10 and diverges at 1e11.
DESCENT_STEP = 1e10


def test_gradient_descent_on_the_model():
    """The plant keeps its geometry; the controller's L2 starts 0.5 off.  Loss: the mean squared distance of S to the
    run with matched geometry.  Five fixed steps of DESCENT_STEP on (L1, L2, M) of the controller; only the first step's
    decrease is asserted.  (The CPU oracle loop goes 2.54e-14 -> 9.6e-15 -> 4.8e-15 -> 3.3e-15 -> 2.8e-15 -> 2.6e-15,
    mostly along L1: the loss cannot tell a longer trailer from a shorter wheelbase over six steps.)"""
    import torch
    from ttmpc.diff import DifferentiableClosedLoop
    c = _case()
    layer = DifferentiableClosedLoop(_loop())
    args = lambda: (_t(c["x_init"]), c["T"])  # noqa: E731
    kw = lambda: dict(wq_wr=_t(c["w"]), noise=_t(c["noise"]))  # noqa: E731
    base = torch.tensor([P["L1"], P["L2"], P["M"]], dtype=torch.float64)
    with torch.no_grad():
        St, _, st = layer(*args(), **kw(), model=base)
    assert torch.all(st == 0)
    th = (base + torch.tensor([0.0, 0.5, 0.0], dtype=torch.float64)).requires_grad_(True)
    seq, path = [], []
    for _ in range(6):
        S, _, st = layer(*args(), **kw(), model=th)
        assert torch.all(st == 0)
        loss = ((S - St) ** 2).mean()
        seq.append(float(loss.detach()))
        path.append(th.detach().tolist())
        (gth,) = torch.autograd.grad(loss, [th])
        with torch.no_grad():
            th -= DESCENT_STEP * gth
    print("loss sequence:", " ".join(f"{v:.4e}" for v in seq))
    print("geometry path:", " | ".join(" ".join(f"{v:.4f}" for v in p) for p in path))
    assert seq[1] < seq[0]
