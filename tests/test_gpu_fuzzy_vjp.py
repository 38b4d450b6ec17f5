"""GPU suite: the fuzzy weight rule as data, its adjoint, the taped retry and the differentiable fuzzy closed loop
(tt_fuzzy_weights_rule_device, tt_fuzzy_weights_vjp_device, tt_sim_window_vjp_fuzzy_device, ClosedLoop(fuzzy_rule=...),
ttmpc.diff).

4. Rule forward: the defaults are tt_fuzzy_weights_device bit for bit; another rule against numpy.
5. Rule adjoint against numpy: retried mask, accumulation, determinism.
6. The fused window adjoint: without a rule it is tt_sim_window_vjp_device, with one it is "stand-alone adjoint, then
   tt_sim_window_vjp_device", bit for bit.
7. The loop: run_tape is run(); the sweep against the numpy chain on the GPU's own tape and against the oracle's central
   differences; grid indexing; a TT_VARIANT_FUZZY solver with an explicit rule.
8. The retry on the device, forced through the status word.
9. Autograd, the stand-alone node, unsupported and bad calls.

Every case prints its figures before it asserts (DESIGN.md "Adjoint of the fuzzy closed loop" records them).  The loop
is fuzzy_vjp_reference.fuzzy_case: N = 6, B = 3, K = 6, in-plant noise, policy "fuzzy", theta = fr.THETA.
"""
import ctypes as C
import errno
import functools

import numpy as np
import pytest

import fuzzy_vjp_reference as fr
import vjp_harness as h
import vjp_reference as vr

pytestmark = pytest.mark.gpu

P, DIST, EPS = fr.P, fr.DIST, h.EPS
SHAPES = [(1, 3, 0), (6, 8, 5), (6, 8, 9), (70, 100, 95)]
_t, _n, _grads, _tape_np = h.t, h.n, h.grads, h.tape_np


@functools.lru_cache(maxsize=None)
def _case():
    return fr.fuzzy_case(h.golden())


def _rule(theta=fr.THETA):
    from ttmpc.simulation import FuzzyRule
    return FuzzyRule(*theta)


def _loop(variant=None, tol=1e-8, per_instance=0, rule="case"):
    import ttmpc
    return h.loop(_case(), "fuzzy", True, per_instance, _rule() if rule == "case" else rule,
                  solver_kw=dict(tol=tol, variant=ttmpc.TT_VARIANT_TRACK if variant is None else variant))


def _states(n, rng):
    """n measured states and window heads on both sides of every switch of the default and the case's rule."""
    x = rng.uniform(-1.0, 1.0, (n, 6))
    x[:, 3] = rng.uniform(-1.2, 1.2, n) * rng.choice([0.25, 1.0], n)
    x[:, 5] = np.where(rng.uniform(size=n) < 0.5, rng.uniform(-2.0, -0.1, n), rng.uniform(-0.1, 2.0, n))
    xref = rng.uniform(-1.0, 1.0, (n, 6, 6))
    xref[:, 0, 5] = np.where(rng.uniform(size=n) < 0.5, rng.uniform(-2.0, -0.1, n), rng.uniform(-0.1, 2.0, n))
    x[:4, 3] = (0.0, 0.35, -0.35, 0.9)                      # on the kinks themselves
    x[4:6, 5], xref[6:8, 0, 5] = -0.1, -0.1
    return x, xref


# ---- 4 ----------------------------------------------------------------------------------------------------------
def test_rule_forward():
    import torch
    import ttmpc
    from ttmpc import simulation as sim
    B, N = 300, 5
    x, xref = _states(B, np.random.default_rng(21))
    tx, tr = _t(x), _t(xref)
    old = torch.full((B, 8), 7.0, dtype=torch.float64, device="cuda")
    assert ttmpc.lib().tt_fuzzy_weights_device(B, N, tx.data_ptr(), tr.data_ptr(), old.data_ptr(), None) == 0
    w_null, w_def = sim.fuzzy_weights_rule(tx, tr, None), sim.fuzzy_weights_rule(tx, tr, sim.FuzzyRule())
    torch.cuda.synchronize()
    ref = fr.rule_weights(fr.DEFAULT_THETA, x[:, 3], x[:, 5], xref[:, 0, 5])
    rev = (x[:, 5] < -0.1) | (xref[:, 0, 5] < -0.1)
    print(f"defaults: reversing {rev.sum()} of {B}, saturated {(np.abs(x[:, 3]) >= 0.35).sum()}, against numpy "
          f"{np.max(np.abs(_n(old) - ref)):.3e}")
    assert np.array_equal(_n(w_null), _n(old)) and np.array_equal(_n(w_def), _n(old))
    assert 50 < rev.sum() < 250 and np.max(np.abs(_n(old) - ref)) <= 4 * EPS * 3.5
    for theta in (fr.THETA, (0.2, 3.0, 2.6, 2.9, 1.2, 1.3, 1.1)):
        w = _n(sim.fuzzy_weights_rule(tx, tr, _rule(theta)))
        ref = fr.rule_weights(theta, x[:, 3], x[:, 5], xref[:, 0, 5])
        rel = np.max(np.abs(w - ref) / np.abs(ref))
        print(f"theta {theta}: relative to numpy {rel:.3e} ({rel / EPS:.2f} eps), clipped entries {(ref == 3.5).sum()}")
        assert rel <= 4 * EPS


# ---- 5 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta", [fr.DEFAULT_THETA, fr.THETA, (0.2, 3.0, 2.6, 2.9, 1.2, 1.3, 1.1)])
def test_rule_adjoint_against_numpy(theta):
    import torch
    from ttmpc import simulation as sim
    B = 300
    rng = np.random.default_rng(22)
    x, xref = _states(B, rng)
    g_w = rng.uniform(-1.0, 1.0, (B, 8))
    retried = (rng.uniform(size=B) < 0.2).astype(np.int32)
    retried[:3], retried[-1] = (1, 0, 1), 1
    gx0, acc0 = rng.uniform(-1.0, 1.0, (B, 6)), rng.uniform(-1.0, 1.0, (B, 7))
    g_psi, g_th = fr.rule_vjp(theta, x[:, 3], x[:, 5], xref[:, 0, 5], g_w)
    live = retried == 0
    rx, racc = gx0.copy(), acc0 + np.where(live[:, None], g_th, 0.0)
    rx[:, 3] += np.where(live, g_psi, 0.0)
    tx, tr, tg, rt = _t(x), _t(xref), _t(g_w), _t(retried, torch.int32)
    outs = []
    for _ in range(2):
        gx, acc = _t(gx0), _t(acc0)
        sim.fuzzy_weights_vjp(tx, tr, tg, _rule(theta), rt, gx, acc)
        outs.append((_n(gx), _n(acc)))
    ex, ea = np.max(np.abs(outs[0][0] - rx)), np.max(np.abs(outs[0][1] - racc))
    print(f"theta {theta}: g_x {ex:.3e}, g_rule_acc {ea:.3e}; retried {int(retried.sum())}, largest |g_psi| "
          f"{np.max(np.abs(g_psi)):.2f}, |g_theta| {np.max(np.abs(g_th)):.2f}")
    assert max(ex, ea) <= 1e-13
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(outs[0][0][~live], gx0[~live]) and np.array_equal(outs[0][1][~live], acc0[~live])
    assert np.array_equal(np.delete(outs[0][0], 3, axis=1), np.delete(gx0, 3, axis=1))      # only the hitch angle
    # no mask and fresh accumulators: the wrapper's zeros
    gx, acc = sim.fuzzy_weights_vjp(tx, tr, tg, _rule(theta))
    assert np.max(np.abs(_n(gx)[:, 3] - g_psi)) <= 1e-13 and np.max(np.abs(_n(acc) - g_th)) <= 1e-13


# ---- 6 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Np,k", SHAPES)
def test_fused_window_adjoint(N, Np, k):
    import torch
    import ttmpc
    from ttmpc import simulation as sim
    L, B = ttmpc.lib(), 7
    rng = np.random.default_rng(100 * N + k)
    x, xr6 = _states(B, rng)
    x[:, 3] = (-0.62, -0.4, -0.11, 0.07, 0.3, 0.55, 0.83)   # inside the case's linear range: every g_psi is live
    xref = rng.uniform(-1.0, 1.0, (B, N + 1, 6))
    xref[:, 0, 5] = xr6[:, 0, 5]
    host = dict(gxr=rng.uniform(-1, 1, (B, N + 1, 6)), gur=rng.uniform(-1, 1, (B, N, 2)),
                px=rng.uniform(-1, 1, (B, Np + 1, 6)), pu=rng.uniform(-1, 1, (B, Np, 2)), gx0=rng.uniform(-1, 1, (B, 6)),
                gs=rng.uniform(-1, 1, (B, 6)), adj=rng.uniform(-1, 1, (B, 6)), gw=rng.uniform(-1, 1, (B, 8)),
                wacc=rng.uniform(-1, 1, (B, 8)), gn=np.full((B, 6), 7.0), racc=rng.uniform(-1, 1, (B, 7)))
    retried = _t(np.array([0, 1, 0, 0, 1, 0, 0]), torch.int32)
    tx, tr = _t(x), _t(xref)
    rule = _rule()

    def run(mode):
        d = {key: _t(v) for key, v in host.items()}
        args = (B, N, k, Np, d["gxr"].data_ptr(), d["gur"].data_ptr(), d["px"].data_ptr(), d["pu"].data_ptr(),
                d["gx0"].data_ptr(), d["gs"].data_ptr(), d["adj"].data_ptr(), d["gw"].data_ptr(), d["wacc"].data_ptr(),
                d["gn"].data_ptr())
        if mode == "plain":
            rc = L.tt_sim_window_vjp_device(*args, None)
        elif mode == "null":
            rc = L.tt_sim_window_vjp_fuzzy_device(*args, None, tx.data_ptr(), tr.data_ptr(), retried.data_ptr(),
                                                  d["racc"].data_ptr(), None)
        elif mode == "fused":
            rc = L.tt_sim_window_vjp_fuzzy_device(*args, C.byref(rule.as_struct()), tx.data_ptr(), tr.data_ptr(),
                                                  retried.data_ptr(), d["racc"].data_ptr(), None)
        else:   # the stand-alone adjoint on g_x0, then the plain window adjoint
            sim.fuzzy_weights_vjp(tx, tr, d["gw"], rule, retried, d["gx0"], d["racc"])
            rc = L.tt_sim_window_vjp_device(*args, None)
        assert rc == 0
        torch.cuda.synchronize()
        return {key: _n(v) for key, v in d.items()}

    plain, null, fused, two = run("plain"), run("null"), run("fused"), run("two")
    for key in host:
        assert np.array_equal(plain[key], null[key]), key                 # no rule: the plain entry, bit for bit
        if key != "gx0":                                                  # (the fused entry leaves the g_x0 buffer alone)
            assert np.array_equal(fused[key], two[key]), key
    assert np.array_equal(fused["gx0"], host["gx0"])
    moved = np.abs(fused["adj"][:, 3] - plain["adj"][:, 3])
    print(f"N={N} Np={Np} k={k}: the rule's term in adj[:, 3] {moved}, in the rule accumulator "
          f"{np.max(np.abs(fused['racc'] - host['racc'])):.3f}")
    assert not moved[[1, 4]].any() and np.all(moved[[0, 2, 3, 5, 6]] > 0.0)
    assert np.array_equal(fused["racc"][[1, 4]], host["racc"][[1, 4]]) and np.array_equal(plain["racc"], host["racc"])
    assert np.array_equal(fused["gn"], two["gx0"])                        # the noise gradient carries the rule's term
    assert np.array_equal(np.delete(fused["adj"], 3, axis=1), np.delete(plain["adj"], 3, axis=1))


# ---- 7 ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _run(variant=None, tol=1e-8):
    c = _case()
    loop = _loop(variant, tol)
    out = loop.run_tape(c["x_init"], c["T"], noise=c["noise"])
    g = loop.backward(out["tape"], _t(c["GS"]), _t(c["GU"]), rule=True)
    return loop, out, _grads(g)


@functools.lru_cache(maxsize=None)
def _oracle_fd(force=()):
    return fr.oracle_fd(_case(), h=1e-4, force=dict(force))


def _compare_with_chain(tag, out, got):
    c, tp = _case(), _tape_np(out["tape"])
    dense, model = (h.shared_plan(fr.chain(c, fn, tp)) for fn in (vr.dense_vjp, vr.riccati_vjp))
    h.compare_with_chain(tag, got, dense, model, fr.GROUPS, per_group=True)
    return dense


def _fd_errors(got, fd):
    e = fr.fd_errors(got, fd)
    for k, v in e.items():
        print(f"  {k:7s}: gpu vs oracle FD {v:.3e}")
    return e


def test_loop_run_tape_is_run():
    c = _case()
    loop, out, _ = _run()
    plain = _loop().run(c["x_init"], c["T"], noise=c["noise"])
    for k in ("states", "controls", "status"):
        assert np.array_equal(plain[k], out[k]), k
    tape = out["tape"]
    assert np.all(out["status"] == 0) and not _n(tape.retried).any()
    x = _n(tape.S)[:-1]
    ref = fr.rule_weights(fr.THETA, x[..., 3], x[..., 5], fr.window_ref_v(c["plan_x"], c["ks"], c["Np"], c["B"]))
    print(f"taped weights against numpy {np.max(np.abs(_n(tape.W) - ref)):.3e}; hitch weights {_n(tape.W)[..., 3].tolist()}")
    assert np.max(np.abs(_n(tape.W) - ref)) <= 4 * EPS * 3.5
    per = (tape.W.numel() * 8 + tape.retried.numel() * 4) / (c["K"] * c["B"])
    assert per == 68


def test_loop_sweep_against_chain_and_oracle_differences():
    loop, out, got = _run()
    assert np.all(out["status"] == 0)
    dense = _compare_with_chain("track variant, tol 1e-8", out, got)
    big = fr.group_max(dense)
    assert min(big[k] for k in ("x_init", "w", "noise", "plan_u")) > 1e-3 and big["theta"] > 1e-3
    fd, ok = _oracle_fd()
    assert ok
    assert max(_fd_errors(got, fd).values()) <= 1e-5


def test_loop_grid_and_determinism():
    c = _case()
    R = 100
    rep = lambda a, ax=0: np.concatenate([a] * R, axis=ax)  # noqa: E731
    small = _loop(per_instance=3)
    o3 = small.run_tape(c["x_init"], c["T"], noise=c["noise"])
    g3 = _grads(small.backward(o3["tape"], _t(c["GS"]), _t(c["GU"]), rule=True))
    big = _loop(per_instance=3 * R)
    o = big.run_tape(rep(c["x_init"]), c["T"], noise=rep(c["noise"], 1))
    GS, GU = _t(rep(c["GS"], 1)), _t(rep(c["GU"], 1))
    g = _grads(big.backward(o["tape"], GS, GU, rule=True))
    again = _grads(big.backward(o["tape"], GS, GU, rule=True))
    assert np.array_equal(o["states"], rep(o3["states"], 1)) and np.all(o["status"] == 0)
    for k in fr.GROUPS:
        ax = 1 if k == "noise" else 0
        assert g[k].shape[ax] == 3 * R
        assert np.array_equal(g[k], rep(g3[k], ax)), k
        assert np.array_equal(g[k], again[k]), k
        assert np.max(np.abs(g3[k])) > 0.0
    assert np.array_equal(_run()[2]["theta"], g3["theta"])                # the shared-plan run: the same per instance


def test_loop_fuzzy_variant_with_explicit_rule():
    import ttmpc
    loop, out, got = _run(ttmpc.TT_VARIANT_FUZZY, 1e-3)
    assert loop.policy == "fuzzy" and loop.noise_in_plant and np.all(out["status"] <= 1)
    _compare_with_chain("fuzzy variant, tol 1e-3", out, got)
    fd, _ = _oracle_fd()
    print("fuzzy variant, tol 1e-3, against the tight oracle's differences (not asserted: the point is only converged "
          "to that tolerance):")
    _fd_errors(got, fd)


# ---- 8 ----------------------------------------------------------------------------------------------------------
def test_retry_on_the_device():
    """After the full-batch solves of steps 0 and 3 the status word of instance 1 is overwritten with TT_MAX_ITER on the
    loop's stream, as if that first attempt had failed: the loop must retry it with unit weights and tape the retry."""
    import torch
    from ttmpc.simulation import LoopTape
    c = _case()
    B, K = c["B"], c["K"]
    loop = _loop()
    plain, calls = loop.solver.solve_ex_device, []

    def forced(n, *a, **kw):
        plain(n, *a, **kw)
        if n == B:
            calls.append(n)
            if len(calls) - 1 in (0, 3):
                with torch.cuda.stream(loop.stream):
                    loop.st[1] = 2
    loop.solver.solve_ex_device = forced
    out = loop.run_tape(c["x_init"], c["T"], noise=c["noise"])
    loop.solver.solve_ex_device = plain
    tape = out["tape"]
    want = np.zeros((K, B), dtype=np.int32)
    want[0, 1] = want[3, 1] = 1
    W = _n(tape.W)
    assert len(calls) == K and np.array_equal(_n(tape.retried), want)
    assert np.all(W[want == 1] == 1.0) and np.all(W[want == 0][:, 3] > 1.0)
    assert np.all(out["status"] == 0)
    S = _n(tape.S)
    for t in (0, 3):
        Xr, Ur = fr.to.reference_window(c["plan_x"], c["plan_u"], c["ks"][t], c["N"])
        r = loop.solver.solve_ex(S[t, 1][None], Xr.T[None], Ur.T[None], wq_wr=np.ones((1, 8)), gain=False)
        assert r.status[0] == 0
        assert np.array_equal(_n(tape.dual)[t, 1], r.dual[0]) and np.array_equal(_n(tape.X)[t, 1], r.X[0])
        assert np.array_equal(out["controls"][t, 1], r.U[0, 0])
    got = _grads(loop.backward(tape, _t(c["GS"]), _t(c["GU"]), rule=True))
    dense = _compare_with_chain("forced retries", out, got)
    assert not dense["rule_terms"][want == 1].any()
    fd, ok = _oracle_fd(((0, 1), (3, 1)))
    assert ok and max(_fd_errors(got, fd).values()) <= 1e-5
    # mark instance 1's other steps as retried too: what is left of its theta gradient is the forced steps' share,
    # and that is exactly zero
    rest = LoopTape(**{k: getattr(tape, k) for k in LoopTape.__slots__})
    rest.retried = tape.retried.clone()
    rest.retried[:, 1] = 1
    g2 = _grads(loop.backward(rest, _t(c["GS"]), _t(c["GU"]), rule=True))
    assert not g2["theta"][1].any() and np.array_equal(g2["theta"][[0, 2]], got["theta"][[0, 2]])
    assert np.max(np.abs(got["theta"][1])) > 0.0


# ---- 9 ----------------------------------------------------------------------------------------------------------
def test_autograd_is_the_backward_call():
    import torch
    from ttmpc.diff import DifferentiableClosedLoop
    c = _case()
    loop, out, got = _run()
    layer = DifferentiableClosedLoop(_loop(rule=_rule(fr.DEFAULT_THETA)))   # the forward applies the tensor's values
    GS, GU = _t(c["GS"]), _t(c["GU"])
    px, pu = _t(c["plan_x"].T[None]), _t(c["plan_u"].T[None])
    x, nz = _t(c["x_init"]).requires_grad_(True), _t(c["noise"]).requires_grad_(True)
    tx, tu = px.clone().requires_grad_(True), pu.clone().requires_grad_(True)
    theta = torch.tensor(fr.THETA, dtype=torch.float64, requires_grad=True)          # a host tensor
    S, Ua, st = layer(x, c["T"], plan_x=tx, plan_u=tu, noise=nz, fuzzy_rule=theta)
    assert layer.loop.rule.theta() == fr.THETA and torch.all(st == 0)
    assert np.array_equal(_n(S), out["states"]) and np.array_equal(_n(Ua), out["controls"])
    ((GS * S).sum() + (GU * Ua).sum()).backward()
    for t, k in zip((x, nz, tx, tu), ("x_init", "noise", "plan_x", "plan_u")):
        assert np.array_equal(_n(t.grad), got[k]), k
    assert theta.grad.device.type == "cpu"
    assert np.array_equal(theta.grad.numpy(), _n(_t(got["theta"]).sum(dim=0)))
    # a directional check on the device itself: step against the theta gradient
    gth = theta.grad.numpy()
    d = -gth / np.linalg.norm(gth)
    eps, L = 1e-3, []
    with torch.no_grad():
        for sgn in (1.0, -1.0):
            S, Ua, st = layer(_t(c["x_init"]), c["T"], plan_x=px, plan_u=pu, noise=_t(c["noise"]),
                              fuzzy_rule=_t(np.asarray(fr.THETA) + sgn * eps * d))
            assert torch.all(st == 0)
            L.append(float((GS * S).sum() + (GU * Ua).sum()))
    fd, an = (L[0] - L[1]) / (2 * eps), float(np.sum(gth * d))
    print(f"directional derivative along -g_theta: finite difference {fd:.6e}, g_theta . d {an:.6e}, relative "
          f"{abs(fd - an) / abs(an):.3e}")
    assert fd < 0.0 and abs(fd - an) <= 1e-3 * abs(an)
    # the rule of the tape is remembered
    loop.set_fuzzy_rule(_rule(fr.DEFAULT_THETA))
    with pytest.raises(ValueError, match="rule changed"):
        loop.backward(out["tape"], GS, GU)
    loop.set_fuzzy_rule(_rule())
    assert np.array_equal(_n(loop.backward(out["tape"], GS, GU)["g_x_init"]), got["x_init"])


def test_fuzzy_weights_node_feeds_the_tracking_layer():
    import torch
    from ttmpc import simulation as sim
    from ttmpc.diff import DifferentiableTracking, fuzzy_weights
    c = _case()
    loop, out, _ = _run()
    tape, N, B = out["tape"], c["N"], c["B"]
    _, xref, uref = sim.window(loop.plan_x, loop.plan_u, c["ks"][1], N, tape.S[1])
    rng = np.random.default_rng(9)
    gX, gU = _t(rng.uniform(-1, 1, (B, N + 1, 6))), _t(rng.uniform(-1, 1, (B, N, 2)))
    layer = DifferentiableTracking(loop.solver)
    x0 = tape.S[1].clone().requires_grad_(True)
    theta = _t(np.asarray(fr.THETA)).requires_grad_(True)
    w = fuzzy_weights(x0, xref, theta)
    X, U, st = layer(x0, xref, uref, wq_wr=w)
    ((gX * X).sum() + (gU * U).sum()).backward()
    assert torch.all(st == 0) and np.array_equal(_n(w), _n(tape.W[1]))
    # by hand: the solve's gradients for (x0, w) as leaves, then the stand-alone rule adjoint
    x0b, wb = tape.S[1].clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    X, U, _ = layer(x0b, xref, uref, wq_wr=wb)
    ((gX * X).sum() + (gU * U).sum()).backward()
    g_x, g_rule = sim.fuzzy_weights_vjp(tape.S[1], xref, wb.grad, _rule())
    print(f"dL/dx0[3]: through the solve {_n(x0b.grad)[:, 3]}, through the rule {_n(g_x)[:, 3]}")
    assert np.array_equal(_n(x0.grad), _n(x0b.grad + g_x)) and np.all(_n(g_x)[:, 3] != 0.0)
    assert np.array_equal(_n(theta.grad), _n(g_rule.sum(dim=0))) and theta.grad.is_cuda


def test_unsupported_and_bad_calls():
    import torch
    import ttmpc
    from ttmpc import simulation as sim
    from ttmpc.diff import DifferentiableClosedLoop
    c = _case()
    builtin = _loop(ttmpc.TT_VARIANT_FUZZY, 1e-3, rule=None)           # a fuzzy solver on the built-in rule
    with pytest.raises(ValueError, match="FUZZY"):
        DifferentiableClosedLoop(builtin)
    with pytest.raises(ValueError, match="fuzzy_rule="):
        builtin.run_tape(c["x_init"], c["T"], noise=c["noise"])
    with pytest.raises(ValueError, match="wq_wr"):
        _loop().run_tape(c["x_init"], c["T"], noise=c["noise"], wq_wr=np.ones((c["B"], 8)))
    plain = _loop(rule=None)
    tape = plain.run_tape(c["x_init"], c["T"], noise=c["noise"])["tape"]
    with pytest.raises(ValueError, match="rule=True"):
        plain.backward(tape, _t(c["GS"]), _t(c["GU"]), rule=True)
    for bad in (dict(psi_full=0.0), dict(psi_full=-1.0), dict(gain_rate=float("nan")), dict(w_min=4.0),
                dict(v_rev=float("inf"))):
        with pytest.raises(ValueError):
            sim.FuzzyRule(**bad)
    L = ttmpc.lib()
    B, N = 4, 6
    f = lambda *s: torch.full(s, 5.0, dtype=torch.float64, device="cuda")  # noqa: E731
    x, xref, w, gx, acc = f(B, 6), f(B, N + 1, 6), f(B, 8), f(B, 6), f(B, 7)
    good = sim.FuzzyRule().as_struct()

    def struct(**kw):
        r = sim.FuzzyRule().as_struct()
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    def fwd(B_=B, N_=N, r=good):
        return L.tt_fuzzy_weights_rule_device(B_, N_, C.byref(r), x.data_ptr(), xref.data_ptr(), w.data_ptr(), None)

    def vjp(B_=B, N_=N, r=good):
        return L.tt_fuzzy_weights_vjp_device(B_, N_, C.byref(r), x.data_ptr(), xref.data_ptr(), None, w.data_ptr(),
                                             gx.data_ptr(), acc.data_ptr(), None)

    def fused(B_=B, N_=N, r=good):
        return L.tt_sim_window_vjp_fuzzy_device(B_, N_, 0, 8, None, None, None, None, gx.data_ptr(), None, None,
                                                w.data_ptr(), None, None, C.byref(r), x.data_ptr(), xref.data_ptr(),
                                                None, acc.data_ptr(), None)
    rules = [struct(psi_full=0.0), struct(psi_full=-0.35), struct(rev_steer=float("nan")), struct(w_max=float("inf")),
             struct(w_min=3.6)]
    bad = []
    for call in (fwd, vjp, fused):
        bad += [call(B_=0), call(B_=-1), call(N_=0), call(N_=L.tt_max_horizon() + 1)] + [call(r=r) for r in rules]
    torch.cuda.synchronize()
    assert bad == [-errno.EINVAL] * len(bad), bad
    for t in (w, gx, acc):        # nothing was launched
        assert torch.all(t == 5.0)
    assert fwd() == 0 and vjp() == 0 and fused() == 0
    torch.cuda.synchronize()
    assert not torch.all(w == 5.0)
