"""GPU suite: the adjoint of the closed loop (tt_policy_plant_vjp_device, tt_sim_window_vjp_device, ClosedLoop.run_tape /
backward) and the autograd layer on it (ttmpc.diff.DifferentiableClosedLoop).

1. policy_plant_vjp alone against the numpy model, every policy and branch.
2. window_vjp alone against the numpy scatter: padding, long windows, determinism, accumulation.
3. run_tape is run(), bitwise.
4. The sweep against the numpy chain on the GPU's own tape, with measurement and with in-plant noise.
5. The sweep against central differences of the CPU oracle's loop.
6. Failure branches forced by an infeasible measurement, for the three policies; a hand-stopped instance.
7. Grid indexing and determinism.
8. Autograd: the layer is the backward call; a directional check on the device; unsupported loops.
9. Bad calls.

Every case prints its figures before it asserts (DESIGN.md "Adjoint of the closed loop" records them).  The inputs are
loop_vjp_reference.loop_case: N = 6, B = 3, K = 6 steps on a plan of Np = 8 inputs, so the end padding is live.
"""
import functools

import numpy as np
import pytest

import loop_vjp_reference as lr
import vjp_harness as h
import vjp_reference as vr

pytestmark = pytest.mark.gpu

P, EPS = lr.P, h.EPS
_t, _n, _golden, _solver, _grads = h.t, h.n, h.golden, h.solver, h.grads


@functools.lru_cache(maxsize=None)
def _case():
    return lr.loop_case(_golden())


def _loop(*a, **kw):
    return h.loop(_case(), *a, **kw)


@functools.lru_cache(maxsize=None)
def _run(policy="track", in_plant=False, fail=False):
    """One taped run and one backward sweep on the case (fail: the measurement of instance 0 at t = 2 and of instance 1
    at t = 0 is pushed out of the state box).  Shared by cases 4 to 8."""
    c = _case()
    noise = c["noise"].copy()
    if fail:
        noise[2, 0, 5] += 100.0
        noise[0, 1, 5] += 100.0
    loop = _loop(policy, in_plant)
    out = loop.run_tape(c["x_init"], c["T"], noise=noise, wq_wr=c["w"])
    g = loop.backward(out["tape"], _t(c["GS"]), _t(c["GU"]))
    return loop, out, _grads(g), noise


def _compare_with_chain(tag, policy, in_plant, out, got):
    """Against the numpy sweep on the GPU's own tape, fn = dense_vjp and riccati_vjp per step; the plan is shared."""
    c, tp = _case(), h.tape_np(out["tape"])
    dense, model = (h.shared_plan(lr.chain(c, fn, tp, policy, in_plant)) for fn in (vr.dense_vjp, vr.riccati_vjp))
    h.compare_with_chain(tag, got, dense, model, lr.GROUPS, per_group=False)
    return dense


# ---- 1 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_plant", [False, True])
@pytest.mark.parametrize("disturbed", [False, True])
@pytest.mark.parametrize("policy", ["track", "nmpc", "fuzzy"])
def test_policy_plant_vjp_against_numpy_model(policy, disturbed, in_plant):
    """B = 300 (two 256-thread blocks): states tiled from the golden q; status, active and count arrays run through
    every row of the branch table."""
    import torch
    from ttmpc import simulation as sim
    B, N = 300, 5
    g = _golden()
    rng = np.random.default_rng(17)
    q = np.tile(g["q"], (5, 1))[:B]
    a, abar, GU = rng.uniform(-1, 1, (B, 6)), rng.uniform(-1, 1, (B, 2)), rng.uniform(-1, 1, (B, 2))
    status = rng.choice([0, 1, 2, 3], size=B).astype(np.int32)
    before = (rng.uniform(size=B) > 0.15).astype(np.int32)
    after = (before & (rng.uniform(size=B) > 0.15)).astype(np.int32)
    count = rng.integers(0, 36, size=B).astype(np.int32)
    count[:4] = (15, 16, 15, 16)
    status[:4], before[:4], after[:4] = 3, 1, 1             # both sides of the fuzzy zero-control threshold
    dist = lr.DIST if disturbed else None
    ra, rabar, rg, rn = lr.policy_plant_vjp(policy, q, status, before, after, count, GU, a, abar, P, dist, in_plant)
    ta, tabar = _t(a), _t(abar)
    gu = torch.full((B, N, 2), 7.0, dtype=torch.float64, device="cuda")
    gn = torch.full((B, 6), 7.0, dtype=torch.float64, device="cuda") if in_plant else None
    sim.policy_plant_vjp(_t(q), _t(status, torch.int32), _t(after, torch.int32), _t(count, torch.int32), ta, tabar, gu, P,
                         dist, policy=policy, active_before=_t(before, torch.int32), grad_u_applied=_t(GU),
                         g_state_noise=gn)
    torch.cuda.synchronize()
    errs = {"a": np.max(np.abs(_n(ta) - ra)), "abar": np.max(np.abs(_n(tabar) - rabar)),
            "g_u0": np.max(np.abs(_n(gu)[:, 0] - rg))}
    if in_plant:
        errs["g_noise"] = np.max(np.abs(_n(gn) - rn))
    moved = (before != 0) & (after != 0)
    print(f"{policy} disturbed={disturbed} in_plant={in_plant}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items())
          + f"; moved {int(moved.sum())}, stopped {int((~moved).sum())}, failed {int((status[moved] > 1).sum())}, "
          f"max|a| {np.max(np.abs(ra)):.2f}")
    assert max(errs.values()) <= 1e-13
    assert np.all(_n(gu)[:, 1:] == 7.0)                      # only row 0 of the grad_u buffer is written
    assert np.array_equal(_n(ta)[~moved], a[~moved])         # a stopped instance keeps a, bit for bit
    assert not _n(gu)[~moved, 0].any()
    # first step: no `active before` array means all active
    ta2, tabar2, gu2 = _t(a), _t(abar), torch.zeros((B, N, 2), dtype=torch.float64, device="cuda")
    sim.policy_plant_vjp(_t(q), _t(status, torch.int32), _t(after, torch.int32), _t(count, torch.int32), ta2, tabar2, gu2,
                         P, dist, policy=policy)
    r2 = lr.policy_plant_vjp(policy, q, status, None, after, count, None, a, abar, P, dist, False)
    e2 = max(np.max(np.abs(_n(ta2) - r2[0])), np.max(np.abs(_n(tabar2) - r2[1])), np.max(np.abs(_n(gu2)[:, 0] - r2[2])))
    print(f"  without active_before and GU: {e2:.3e}")
    assert e2 <= 1e-13


# ---- 2 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("N,Np,k", [(6, 8, 0), (6, 8, 5), (6, 8, 9), (70, 100, 40), (70, 100, 95)])
def test_window_vjp_against_numpy_scatter(N, Np, k, shared):
    import torch
    from ttmpc import simulation as sim
    B = 3
    rng = np.random.default_rng(100 * N + k)
    gxr, gur = rng.uniform(-1, 1, (B, N + 1, 6)), rng.uniform(-1, 1, (B, N, 2))
    ax0, au0 = rng.uniform(-1, 1, (B, Np + 1, 6)), rng.uniform(-1, 1, (B, Np, 2))   # pre-filled accumulators
    rx, ru = lr.window_vjp(gxr, gur, k, Np, ax0.copy(), au0.copy())
    ax, au = _t(ax0), _t(au0)
    sim.window_vjp(_t(gxr), _t(gur), k, Np, ax, au)
    ax2, au2 = _t(ax0), _t(au0)
    sim.window_vjp(_t(gxr), _t(gur), k, Np, ax2, au2)
    torch.cuda.synchronize()
    gx, gu = _n(ax), _n(au)
    assert np.array_equal(gx, _n(ax2)) and np.array_equal(gu, _n(au2))            # two runs: the same bits
    # unpadded rows exactly; the padded row holds acc + (ascending-j sum): <= 4 eps sum|terms|
    tail_x = np.abs(ax0[:, Np]) + np.abs(gxr[:, max(Np - k, 0):]).sum(axis=1)
    ex = np.abs(gx - rx)
    print(f"N={N} Np={Np} k={k}: padded state row error {ex[:, Np].max():.3e} (bound {4 * EPS * tail_x.max():.3e}), "
          f"rows folded onto it {max(N + 1 - max(Np - k, 0), 0)}")
    assert np.array_equal(gx[:, :Np], rx[:, :Np])
    assert np.all(ex[:, Np] <= 4 * EPS * tail_x)
    if k < Np:
        tail_u = np.abs(au0[:, Np - 1]) + np.abs(gur[:, max(Np - 1 - k, 0):]).sum(axis=1)
        eu = np.abs(gu - ru)
        print(f"  padded input row error {eu[:, Np - 1].max():.3e} (bound {4 * EPS * tail_u.max():.3e})")
        assert np.array_equal(gu[:, :Np - 1], ru[:, :Np - 1])
        assert np.all(eu[:, Np - 1] <= 4 * EPS * tail_u)
    else:
        assert np.array_equal(gu, au0)                                            # k >= Np: nothing reaches plan_u
    assert np.array_equal(gx[:, :min(k, Np)], ax0[:, :min(k, Np)])                # rows before the window: untouched
    if shared:   # one plan for all instances: the wrapper's sum over B of fresh per-instance gradients
        sx, su = sim.window_vjp(_t(gxr), _t(gur), k, Np, shared=True)
        fx, fu = lr.window_vjp(gxr, gur, k, Np, np.zeros((B, Np + 1, 6)), np.zeros((B, Np, 2)))
        assert tuple(sx.shape) == (1, Np + 1, 6) and tuple(su.shape) == (1, Np, 2)
        bx = 4 * EPS * (np.abs(fx).sum(axis=0) + np.abs(gxr).sum(axis=(0, 1)))
        bu = 4 * EPS * (np.abs(fu).sum(axis=0) + np.abs(gur).sum(axis=(0, 1)))
        assert np.all(np.abs(_n(sx)[0] - fx.sum(axis=0)) <= bx) and np.all(np.abs(_n(su)[0] - fu.sum(axis=0)) <= bu)


# ---- 3 ----------------------------------------------------------------------------------------------------------
def test_run_tape_is_run():
    c = _case()
    obs = _golden()["obstacles"]
    plain = _loop(obstacles=obs).run(c["x_init"], c["T"], noise=c["noise"])
    taped = _loop(obstacles=obs).run_tape(c["x_init"], c["T"], noise=c["noise"])
    for k in ("states", "controls", "status", "iters", "collide"):
        assert np.array_equal(plain[k], taped[k]), k
    tape = taped["tape"]
    assert np.array_equal(_n(tape.S), plain["states"]) and np.array_equal(_n(tape.Ua), plain["controls"])
    assert np.array_equal(_n(tape.U)[:, :, 0], plain["controls"])                 # every solve succeeded and was applied
    per = tape.nbytes() / (c["K"] * c["B"])
    print(f"tape: {tape.nbytes()} bytes, {per:.0f} per instance and step ((30 (N+1) - 2) * 8 = {(30 * 7 - 2) * 8} in X, U, dual)")
    assert np.all(plain["status"] == 0)


# ---- 4 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_plant", [False, True])
def test_sweep_against_numpy_chain(in_plant):
    loop, out, got, _ = _run("track", in_plant)
    assert np.all(out["status"] == 0)
    dense = _compare_with_chain(f"in_plant={in_plant}", "track", in_plant, out, got)
    big = lr.group_max(dense)
    assert min(big[k] for k in ("x_init", "w", "noise", "plan_u")) > 1e-3 and big["plan_x"] > 1e-3 * big["x_init"]


# ---- 5 ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_fd():
    return lr.oracle_fd(_case(), h=1e-4)


def test_sweep_against_oracle_loop_finite_differences():
    loop, out, got, _ = _run("track", False)
    fd, ok = _oracle_fd()
    assert ok and np.all(out["status"] == 0)
    err = {"x_init": np.max(np.abs(got["x_init"] - fd["x_init"])), "w": np.max(np.abs(got["w"] - fd["w"])),
           "noise": np.max(np.abs(got["noise"] - fd["noise"])),
           "plan_x": max(abs(got["plan_x"][0, r, i] - v) for (r, i), v in fd["plan_x"].items()),
           "plan_u": max(abs(got["plan_u"][0, r, i] - v) for (r, i), v in fd["plan_u"].items())}
    big = lr.group_max(got)
    for k in lr.GROUPS:
        print(f"{k:7s}: gpu vs oracle FD {err[k]:.3e}, largest entry {big[k]:.3e}")
    assert max(err.values()) <= 1e-5
    assert min(big[k] for k in ("x_init", "w", "noise", "plan_u")) > 1e-3 and big["plan_x"] > 1e-3 * big["x_init"]


# ---- 6 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["track", "nmpc", "fuzzy"])
def test_failure_branches(policy):
    """+100 on the measured speed of instance 0 at t = 2 and of instance 1 at t = 0: x_meas leaves the state box, that
    solve alone is TT_INFEASIBLE.  Instance 0 is a failure between successes (fuzzy: u_last re-applied, abar live)."""
    import torch
    from ttmpc.simulation import LoopTape
    c = _case()
    loop, out, got, noise = _run(policy, False, fail=True)
    assert loop.noise_in_plant is False and loop.measurement_noise
    st = out["status"]
    print(f"{policy}: status by step {st.tolist()}, applied controls at the failures {out['controls'][2, 0]}, "
          f"{out['controls'][0, 1]}")
    failed = np.zeros_like(st, dtype=bool)
    failed[2, 0] = failed[0, 1] = True
    assert np.all(st[failed] == 3) and np.all(st[~failed] <= 1)
    assert out["active"].all()
    if policy == "fuzzy":
        assert np.array_equal(out["controls"][2, 0], out["controls"][1, 0])       # the last successful control again
    if policy != "track":
        assert not out["controls"][0, 1].any()
    _compare_with_chain(policy, policy, False, out, got)
    assert not got["noise"][2, 0].any() and not got["noise"][0, 1].any()          # dL/dn_t at a failed step: exactly 0
    assert np.max(np.abs(got["noise"][1, 0])) > 0.0
    # a hand-stopped instance: nothing of its run reaches x_init but the loss on its (constant) states
    tape = out["tape"]
    stopped = LoopTape(**{k: getattr(tape, k) for k in LoopTape.__slots__})
    stopped.active = tape.active.clone()
    stopped.active[:, 2] = 0
    g2 = _grads(loop.backward(stopped, _t(c["GS"]), _t(c["GU"])))
    acc = c["GS"][c["K"], 2].copy()
    for t in range(c["K"] - 1, -1, -1):
        acc = acc + c["GS"][t, 2]
    assert np.array_equal(g2["x_init"][2], acc)
    assert not g2["w"][2].any() and not g2["noise"][:, 2].any()
    assert np.array_equal(g2["x_init"][:2], got["x_init"][:2])                    # the neighbours are what they were
    torch.cuda.synchronize()


# ---- 7 ----------------------------------------------------------------------------------------------------------
def test_grid_and_determinism():
    """B = 300 as 100 copies of the three instances, every instance with its own plan: each copy's gradients are those
    of the B = 3 run, bit for bit; two sweeps over one tape are bitwise equal."""
    c = _case()
    R = 100
    rep = lambda a, ax=0: np.concatenate([a] * R, axis=ax)  # noqa: E731
    small = _loop(per_instance=3)
    o3 = small.run_tape(c["x_init"], c["T"], noise=c["noise"], wq_wr=c["w"])
    g3 = _grads(small.backward(o3["tape"], _t(c["GS"]), _t(c["GU"])))
    big = _loop(per_instance=3 * R)
    o = big.run_tape(rep(c["x_init"]), c["T"], noise=rep(c["noise"], 1), wq_wr=rep(c["w"]))
    GS, GU = _t(rep(c["GS"], 1)), _t(rep(c["GU"], 1))
    g = _grads(big.backward(o["tape"], GS, GU))
    again = _grads(big.backward(o["tape"], GS, GU))
    assert np.array_equal(o["states"], rep(o3["states"], 1)) and np.all(o["status"] == 0)
    for k in lr.GROUPS:
        ax = 1 if k == "noise" else 0
        assert g[k].shape[ax] == 3 * R
        assert np.array_equal(g[k], rep(g3[k], ax)), k
        assert np.array_equal(g[k], again[k]), k
        assert np.max(np.abs(g3[k])) > 0.0
    # the shared-plan run's gradient is the per-instance one summed over B
    shared = _run("track", False)[2]
    bx = 4 * EPS * np.abs(g3["plan_x"]).sum(axis=0)
    assert np.all(np.abs(shared["plan_x"][0] - g3["plan_x"].sum(axis=0)) <= bx)
    assert np.array_equal(shared["x_init"], g3["x_init"])


# ---- 8 ----------------------------------------------------------------------------------------------------------
def test_autograd_is_the_backward_call():
    import torch
    from ttmpc.diff import DifferentiableClosedLoop
    c = _case()
    loop, out, got, _ = _run("track", False)
    layer = DifferentiableClosedLoop(_loop())
    GS, GU = _t(c["GS"]), _t(c["GU"])
    px, pu = _t(c["plan_x"].T[None]), _t(c["plan_u"].T[None])

    def inputs(req):
        ts = [_t(c["x_init"]), _t(c["w"]), px.clone(), pu.clone(), _t(c["noise"])]
        return [t.requires_grad_(r) for t, r in zip(ts, req)]

    x, w, tx, tu, nz = inputs([True] * 5)
    S, Ua, st = layer(x, c["T"], wq_wr=w, plan_x=tx, plan_u=tu, noise=nz)
    assert not st.requires_grad and st.dtype == torch.int32 and torch.all(st == 0)
    assert np.array_equal(_n(S), out["states"]) and np.array_equal(_n(Ua), out["controls"])
    ((GS * S).sum() + (GU * Ua).sum()).backward()
    for t, k in zip((x, w, nz, tx, tu), lr.GROUPS):
        assert np.array_equal(_n(t.grad), got[k]), k
    # inputs that do not ask for a gradient get none
    x, w, tx, tu, nz = inputs([False, True, False, False, False])
    S, Ua, _ = layer(x, c["T"], wq_wr=w, plan_x=tx, plan_u=tu, noise=nz)
    ((GS * S).sum() + (GU * Ua).sum()).backward()
    assert x.grad is None and tx.grad is None and tu.grad is None and nz.grad is None
    assert np.array_equal(_n(w.grad), got["w"])
    # a directional check on the device itself: step against the weight gradient
    gw = got["w"]
    d = -gw / np.linalg.norm(gw)
    eps, L = 1e-3, []
    with torch.no_grad():
        for sgn in (1.0, -1.0):
            S, Ua, st = layer(_t(c["x_init"]), c["T"], wq_wr=_t(c["w"] + sgn * eps * d), plan_x=px, plan_u=pu,
                              noise=_t(c["noise"]))
            assert torch.all(st == 0)
            L.append(float((GS * S).sum() + (GU * Ua).sum()))
    fd, an = (L[0] - L[1]) / (2 * eps), float(np.sum(gw * d))
    print(f"directional derivative along -g_w: finite difference {fd:.6e}, g_w . d {an:.6e}, relative "
          f"{abs(fd - an) / abs(an):.3e}")
    assert fd < 0.0 and abs(fd - an) <= 1e-3 * abs(an)


def test_unsupported_loops_raise():
    import ttmpc
    from oracle import ttmpc_oracle as to
    from ttmpc import simulation as sim
    from ttmpc.diff import DifferentiableClosedLoop
    c = _case()
    nlp = c["nlp"]
    fuzzy = sim.ClosedLoop(_solver(nlp, variant=ttmpc.TT_VARIANT_FUZZY), c["plan_x"], c["plan_u"], P, lr.DIST)
    obs = _golden()["obstacles"]
    obca = ttmpc.ObcaSolver(nlp.N, P, to.DEFAULT_Q, to.DEFAULT_R, to.MPC_XLB, to.MPC_XUB, to.MPC_ULB, to.MPC_UUB, obs,
                            variant=ttmpc.TT_VARIANT_TRACK_OBCA)
    switch = sim.ClosedLoop(_solver(nlp), c["plan_x"], c["plan_u"], P, lr.DIST, obstacles=obs, switch_solver=obca)
    for loop, why in ((fuzzy, "FUZZY"), (switch, "OBCA")):
        with pytest.raises(ValueError, match=why):
            DifferentiableClosedLoop(loop)
        with pytest.raises(ValueError, match=why):
            loop.run_tape(c["x_init"], c["T"], noise=c["noise"])
    nmpc = sim.ClosedLoop(_solver(nlp, variant=ttmpc.TT_VARIANT_NMPC), c["plan_x"], c["plan_u"], P, lr.DIST,
                          warm_start=True, policy="nmpc")
    out = nmpc.run_tape(c["x_init"], c["T"], noise=c["noise"])      # the NMPC variant with its warm start is supported
    g = _grads(nmpc.backward(out["tape"], _t(c["GS"]), _t(c["GU"])))
    assert nmpc.noise_in_plant and np.all(out["status"] <= 1)
    assert np.max(np.abs(g["x_init"])) > 1e-3 and np.max(np.abs(g["noise"])) > 0.0 and np.max(np.abs(g["w"])) > 0.0


# ---- 9 ----------------------------------------------------------------------------------------------------------
def test_bad_calls_are_rejected():
    import ctypes as C
    import errno

    import torch
    import ttmpc
    from ttmpc import simulation as sim
    L = ttmpc.lib()
    B, N = 4, 6
    p = sim.plant(P, lr.DIST)
    f = lambda *s: torch.full(s, 5.0, dtype=torch.float64, device="cuda")  # noqa: E731
    i = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")  # noqa: E731
    S, a, ab, gu = f(B, 6), f(B, 6), f(B, 2), f(B, N, 2)
    st, act, cnt = i(B), i(B) + 1, i(B)

    def call(B_=B, N_=N, pol=0, state=S):
        return L.tt_policy_plant_vjp_device(B_, N_, C.byref(p), pol, None if state is None else state.data_ptr(),
                                            st.data_ptr(), None, act.data_ptr(), cnt.data_ptr(), None, a.data_ptr(),
                                            ab.data_ptr(), gu.data_ptr(), None, None)
    bad = [call(state=None), call(B_=0), call(B_=-1), call(N_=0), call(N_=L.tt_max_horizon() + 1), call(pol=3),
           call(pol=-1)]
    gx, gr, px, pu = f(B, N + 1, 6), f(B, N, 2), f(B, 9, 6), f(B, 8, 2)

    def wcall(B_=B, N_=N, k=0, Np=8):
        return L.tt_sim_window_vjp_device(B_, N_, k, Np, gx.data_ptr(), gr.data_ptr(), px.data_ptr(), pu.data_ptr(),
                                          None, None, None, None, None, None, None)
    bad += [wcall(B_=0), wcall(N_=0), wcall(N_=L.tt_max_horizon() + 1), wcall(k=-1), wcall(Np=0)]
    torch.cuda.synchronize()
    assert bad == [-errno.EINVAL] * len(bad), bad
    for t in (a, ab, gu, px, pu):     # nothing was launched
        assert torch.all(t == 5.0)
    assert call() == 0 and wcall() == 0
    torch.cuda.synchronize()
    assert not torch.all(gu == 5.0) and not torch.all(px == 5.0)
