"""GPU tests of per-instance obstacle scenes in OBCA solves and their adjoints (tt_obca_solve_batch_scenes*,
tt_obca_vjp_scenes*; obca_kernel's per-instance scene load, the helper workgroups' scene reload and obca_vjp_kernel's
per-instance obstacle rows).

The main criterion is bitwise and has no tolerance: row b of a batch with scenes is what a B = 1 call returns on a
fresh handle whose ``set_scene`` got row b.  The scene family is made from a case's own scene: the scene itself, the
whole scene moved 2.5 m back (the inactive variant), one obstacle widened by 0.3, and d_min beside the default 0.2.

Family of case A (N = 6, M = 1): obstacle 0 widened, d_min 0.1 and 0.35; the CPU oracle converges on all six rows.
Family of case B (N = 8, M = 2): the contact with obstacle 0 sits at the tightened braking bound, so the oracle ends
TT_INFEASIBLE with obstacle 0 widened by 0.3 and with d_min 0.25, 0.3 and 0.35 (chosen on the CPU, as are all rows
here); the widened obstacle is therefore obstacle 1 (beside the trailer) and the larger margin is 0.22, on which the
oracle returns status 0 for every row.

Measured on an MI355X: every bitwise comparison holds; case B's rows against the oracle max|X - X_oracle| 5e-20 to
3.1e-10 with equal statuses; the two plan scenes 2.1e-10 and 1.3e-7; the adjoint rows against the dense solve 9.2e-12
(the scene itself) and 1.7e-12 (obstacle widened), the numpy model of the kernel at the same figures.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import obca_scene_reference as osr
import obca_vjp_harness as hx
import obca_vjp_reference as orf
from conftest import GOLDEN
from test_obca_oracle import P6, toy_plan

pytestmark = pytest.mark.gpu

OUT8, OUT4 = hx.OUT8, hx.OUT4


def family(obs, widen=0, big=0.35):
    """The B = 6 scene family of a case: (obstacles (6,M,4), d_min (6,))."""
    moved, wide = obs.copy(), obs.copy()
    moved[:, 0] += 2.5
    wide[widen, 2] += 0.3
    return np.array([obs, moved, wide, obs, obs, wide]), np.array([0.2, 0.2, 0.2, 0.1, big, 0.1])


def _case(name):
    if name == "a":
        case = orf.case_a()
        return case, family(case[5])
    case = orf.case_b()
    return case, family(case[5], widen=1, big=0.22)


_solver = hx.solver


@functools.lru_cache(maxsize=None)
def batch(name):
    """The family in one launch: the solve with its iterate, the params adjoint and the plain adjoint."""
    case, (S, D) = _case(name)
    N, p, Q, R, bnd, obs, x0, xr, ur = case
    B = len(D)
    tile = lambda a: np.tile(a, (B,) + (1,) * a.ndim)  # noqa: E731
    x0b, xrb, urb = tile(x0), tile(xr), tile(ur)
    gX, gU = orf.upstream(N)
    gXb, gUb = tile(gX), tile(gU)
    s = _solver(case)
    out = s.solve(x0b, xref=xrb, uref=urb, iterate=True, obstacles=S, d_min=D)
    st, I = out[3], out[6]
    rp = s.vjp(I, st, gXb, gUb, xref=xrb, uref=urb, params=True, obstacles=S, d_min=D)
    r = s.vjp(I, st, gXb, gUb, obstacles=S, d_min=D)
    return case, (S, D), (x0b, xrb, urb, gXb, gUb), out, rp, r


# ---- 1. bitwise against one handle per scene ----
@pytest.mark.parametrize("name", ["a", "b"])
def test_rows_equal_one_handle_per_scene(name):
    case, (S, D), (x0b, xrb, urb, gXb, gUb), out, rp, r = batch(name)
    st = out[3]
    print(f"case {name}: status {st.tolist()} iters {out[4].tolist()}")
    assert np.all(st <= 1), st
    for b in range(len(D)):
        h = _solver(case)
        h.set_scene(S[b], D[b])
        one = h.solve(x0b[b:b + 1], xref=xrb[b:b + 1], uref=urb[b:b + 1], iterate=True)
        for k, (u, v) in enumerate(zip(out, one)):
            assert np.array_equal(u[b], v[0]), (name, b, k)
        p1 = h.vjp(one[6], one[3], gXb[b:b + 1], gUb[b:b + 1], xref=xrb[b:b + 1], uref=urb[b:b + 1], params=True)
        for k in OUT8:
            assert np.array_equal(getattr(rp, k)[b], getattr(p1, k)[0]), (name, b, k)
        q1 = h.vjp(one[6], one[3], gXb[b:b + 1], gUb[b:b + 1])
        for k in OUT4:
            assert np.array_equal(getattr(r, k)[b], getattr(q1, k)[0]), (name, b, k)
    assert np.all(rp.vjp_status == 0) and np.all(r.vjp_status == 0)
    # the rows are not one scene's: the moved row and the d_min rows differ from row 0
    for b in (1, 3, 4):
        assert not np.array_equal(out[0][b], out[0][0]), b


# ---- 2. a shared scene is the plain call ----
def test_shared_scene_and_null_struct_are_the_plain_call():
    import ttmpc
    case, (S, D), (x0b, xrb, urb, gXb, gUb), _, _, _ = batch("b")
    N, M = case[0], case[5].shape[0]
    B = len(D)
    s = _solver(case)
    ob, dm = s.scene()
    plain = s.solve(x0b, xref=xrb, uref=urb, iterate=True)
    tiled = s.solve(x0b, xref=xrb, uref=urb, iterate=True, obstacles=np.tile(ob, (B, 1, 1)), d_min=np.full(B, dm))
    only_obs = s.solve(x0b, xref=xrb, uref=urb, iterate=True, obstacles=np.tile(ob, (B, 1, 1)))
    only_dm = s.solve(x0b, xref=xrb, uref=urb, iterate=True, d_min=dm)
    for other in (tiled, only_obs, only_dm):
        for u, v in zip(plain, other):
            assert np.array_equal(u, v)
    # a NULL struct and a struct of two NULLs through the raw ABI
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    P = lambda a: a.ctypes.data_as(dp)  # noqa: E731
    I_ = lambda a: a.ctypes.data_as(ip)  # noqa: E731
    st, I = plain[3], plain[6]
    pp = s.vjp(I, st, gXb, gUb, xref=xrb, uref=urb, params=True)
    pq = s.vjp(I, st, gXb, gUb)
    for sc_arg in (None, C.byref(ttmpc._lib.TTObcaScenes(None, None))):
        X, U, Z = np.empty((B, N + 1, 6)), np.empty((B, N, 2)), np.empty((B, s.n))
        st2, it2, kk2 = np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B)
        I2 = np.empty((B, s.iterate_len()))
        rc = s._L.tt_obca_solve_batch_scenes(s._h, B, P(x0b), None, P(xrb), P(urb), None, P(X), P(U), P(Z), I_(st2),
                                             I_(it2), P(kk2), P(I2), sc_arg)
        assert rc == 0
        for u, v in zip(plain, (X, U, Z, st2, it2, kk2, I2)):
            assert np.array_equal(u, v)
        # both adjoints: eight outputs -> the params instantiation, four -> the plain one
        g = {"g_x0": np.empty((B, 6)), "g_xref": np.empty((B, N + 1, 6)), "g_uref": np.empty((B, N, 2)),
             "g_obstacles": np.empty((B, M, 4)), "g_dmin": np.empty(B), "g_Q": np.empty((B, 6, 6)),
             "g_R": np.empty((B, 2, 2)), "vjp_status": np.empty(B, np.int32)}
        o8 = ttmpc._lib.TTObcaVjpParamsOut(*[g[k].ctypes.data for k in ("g_x0", "g_xref", "g_uref", "vjp_status",
                                                                         "g_obstacles", "g_dmin", "g_Q", "g_R")])
        rc = s._L.tt_obca_vjp_scenes(s._h, B, P(I), I_(st), P(xrb), P(urb), P(gXb), P(gUb), C.byref(o8), sc_arg)
        assert rc == 0
        for k in OUT8:
            assert np.array_equal(g[k], getattr(pp, k)), k
        o4 = ttmpc._lib.TTObcaVjpParamsOut(g["g_x0"].ctypes.data, g["g_xref"].ctypes.data, g["g_uref"].ctypes.data,
                                           g["vjp_status"].ctypes.data, None, None, None, None)
        rc = s._L.tt_obca_vjp_scenes(s._h, B, P(I), I_(st), None, None, P(gXb), P(gUb), C.byref(o4), sc_arg)
        assert rc == 0
        for k in OUT4:
            assert np.array_equal(g[k], getattr(pq, k)), k
    # the adjoints with the tiled scene
    tp = s.vjp(I, st, gXb, gUb, xref=xrb, uref=urb, params=True, obstacles=np.tile(ob, (B, 1, 1)), d_min=dm)
    tq = s.vjp(I, st, gXb, gUb, obstacles=np.tile(ob, (B, 1, 1)), d_min=dm)
    for k in OUT8:
        assert np.array_equal(getattr(tp, k), getattr(pp, k)), k
    for k in OUT4:
        assert np.array_equal(getattr(tq, k), getattr(pq, k)), k


# ---- 3. helpers serve instances of different scenes ----
def _windows():
    from ttmpc import scenarios as sc
    g = np.load(GOLDEN / "reference_numpy.npz")
    x0, xr, ur = sc.mpc_obs_batch(g["state_traj"], g["input_traj"], 16, 50, seed=0)
    obs = g["obstacles"]
    b = np.arange(16.0)
    S = np.tile(obs, (16, 1, 1))
    S[:, :, 0] += (0.02 * b)[:, None]   # 0 .. 0.30 m in x
    S[:, :, 1] -= (0.01 * b)[:, None]   # 0 .. 0.15 m in y
    D = 0.1 + 0.2 * b / 15.0            # 0.1 .. 0.3
    return obs, x0, xr, ur, S, D


def _window_solver(obs, max_iter):
    import ttmpc
    from ttmpc import scenarios as sc
    return ttmpc.ObcaSolver(50, dict(P6, dt=0.05), sc.OBCA_Q, sc.OBCA_R, sc.XLB, sc.XUB, sc.ULB, sc.UUB, obs,
                            variant=ttmpc.TT_VARIANT_TRACK_OBCA, max_iter=max_iter)


def test_helpers_serve_instances_of_different_scenes():
    """The 16 MPC+OBCA windows (N = 50, M = 11), each with its own shifted obstacles and its own d_min, stopped at
    max_iter 60 (every iteration runs block passes, so every instance that iterates has run them): with helpers and
    without agree bitwise, and three instances equal a B = 1 solve on a handle with their scene."""
    obs, x0, xr, ur, S, D = _windows()
    runs = []
    for nh in (-1, 0):
        s = _window_solver(obs, 60)
        s.set_helpers(nh)
        runs.append(s.solve(x0, xref=xr, uref=ur, iterate=True, obstacles=S, d_min=D))
    print("status", runs[0][3].tolist(), "iters", runs[0][4].tolist())
    assert np.any(runs[0][4] > 0)  # block passes ran
    for u, v in zip(*runs):
        assert np.array_equal(u, v)
    for b in (0, 8, 15):
        h = _window_solver(obs, 60)
        h.set_scene(S[b], D[b])
        one = h.solve(x0[b:b + 1], xref=xr[b:b + 1], uref=ur[b:b + 1], iterate=True)
        for k, (u, v) in enumerate(zip(runs[0], one)):
            assert np.array_equal(u[b], v[0]), (b, k)


# ---- 4. plan variant ----
def test_plan_variant_with_two_scenes():
    import ttmpc
    from oracle import c_oracle as co
    from oracle.obca_nlp import ObcaNLP
    from ttmpc import scenarios as sc
    N, M, obs, x0, xg, zg = toy_plan()
    S = np.array([obs, obs + np.array([0.4, 0.1, 0.3, 0.0])])
    D = np.array([0.2, 0.3])
    bnd = (sc.OBCA_XLB, sc.OBCA_XUB, sc.OBCA_ULB, sc.OBCA_UUB)
    mk = lambda: ttmpc.ObcaSolver(N, P6, sc.OBCA_Q, sc.OBCA_R, *bnd, obs)  # noqa: E731
    out = mk().solve(x0, xg, z_guess=zg, iterate=True, obstacles=S, d_min=D)
    assert np.all(out[3] == 0), out[3]
    for b in range(2):
        h = mk()
        h.set_scene(S[b], D[b])
        one = h.solve(x0[b:b + 1], xg[b:b + 1], z_guess=zg[b:b + 1], iterate=True)
        for k, (u, v) in enumerate(zip(out, one)):
            assert np.array_equal(u[b], v[0]), (b, k)
        P = co.make_obca_problem(N, P6, sc.OBCA_Q, sc.OBCA_R, *bnd, S[b])
        P.dmin = D[b]
        zc, stc, itc, kkc = co.obca_solve_batch(P, x0[b:b + 1], xg[b:b + 1], z_guess=zg[b:b + 1])
        assert stc[0] == 0
        nlp = ObcaNLP(N, M, P6, sc.OBCA_Q, sc.OBCA_R, *bnd, S[b])
        (Xg, Ug, _, _), (Xo, Uo, _, _) = nlp.split(out[2][b]), nlp.split(zc[0])
        err = max(np.max(np.abs(Xg - Xo)), np.max(np.abs(Ug - Uo)))
        print(f"plan scene {b}: max|GPU - oracle| {err:.2e}")
        assert err <= 1e-6


def test_reference_classes_take_obstacle_lists():
    """MPCTrackingControlObs.solve_batch and TrajectoryOptimization.plan_batch with one obstacle list per instance (the
    reference's format) are the solver calls with those scenes; a wrong B or a wrong M raises."""
    import ttmpc
    from ttmpc import scenarios as sc
    case, (S, D), (x0b, xrb, urb, gXb, gUb), out, _, _ = batch("b")
    N, p, Q, R, bnd, obs = case[:6]
    lists = [[{"center": (o[0], o[1]), "width": o[2], "height": o[3]} for o in Sb] for Sb in S]
    box = ({"lb": bnd[0], "ub": bnd[1]}, {"lb": bnd[2], "ub": bnd[3]})
    pp = dict(p, horizon=N)
    ctrl = ttmpc.MPCTrackingControlObs(ttmpc.TruckTrailerModel(pp), pp, Q, R, *box, obstacle_list=lists[0])
    X, U, st = ctrl.solve_batch(x0b, xrb.transpose(0, 2, 1), urb.transpose(0, 2, 1), obstacle_lists=lists)
    ref = _solver(case).solve(x0b, xref=xrb, uref=urb, obstacles=S)   # (d_min stays the handle's 0.2)
    assert np.array_equal(X.transpose(0, 2, 1), ref[0]) and np.array_equal(U.transpose(0, 2, 1), ref[1])
    assert np.array_equal(st, ref[3])
    assert not np.array_equal(ref[0][0], ref[0][1])
    with pytest.raises(ValueError):
        ctrl.solve_batch(x0b, xrb.transpose(0, 2, 1), urb.transpose(0, 2, 1), obstacle_lists=lists[:3])
    with pytest.raises(ValueError):
        ctrl.solve_batch(x0b, xrb.transpose(0, 2, 1), urb.transpose(0, 2, 1), obstacle_lists=[l[:1] for l in lists])
    Np, M, obs_p, x0, xg, zg = toy_plan()
    Sp = np.array([obs_p, obs_p + np.array([0.4, 0.1, 0.3, 0.0])])
    pl = [[{"center": (o[0], o[1]), "width": o[2], "height": o[3]} for o in Sb] for Sb in Sp]
    pbox = ({"lb": sc.OBCA_XLB, "ub": sc.OBCA_XUB}, {"lb": sc.OBCA_ULB, "ub": sc.OBCA_UUB})
    pp = dict(P6, horizon=Np)
    planner = ttmpc.TrajectoryOptimization(ttmpc.TruckTrailerModel(pp), pp, sc.OBCA_Q, sc.OBCA_R, *pbox, pl[0])
    Xp, Up, Zp = planner.plan_batch(x0, xg, zg, obstacle_lists=pl)
    refp = ttmpc.ObcaSolver(Np, P6, sc.OBCA_Q, sc.OBCA_R, sc.OBCA_XLB, sc.OBCA_XUB, sc.OBCA_ULB, sc.OBCA_UUB,
                            obs_p).solve(x0, xg, z_guess=zg, obstacles=Sp)
    assert np.array_equal(Xp.transpose(0, 2, 1), refp[0]) and np.array_equal(Zp, refp[2])
    with pytest.raises(ValueError):
        planner.plan_batch(x0, xg, zg, obstacle_lists=pl[:1])


# ---- 5. oracle parity of the MPC+OBCA path ----
def test_mpc_obca_rows_match_oracle():
    from oracle import c_oracle as co
    case, (S, D), (x0b, xrb, urb, gXb, gUb), out, _, _ = batch("b")
    N, p, Q, R, bnd, obs, x0, xr, ur = case
    X, st = out[0], out[3]
    for b in range(len(D)):
        P = orf.problem(N, p, Q, R, bnd, S[b])
        P.dmin = D[b]
        zc, stc, itc, kkc = co.obca_solve_batch(P, x0[None], xref=xr[None], uref=ur[None])
        Xc = co.obca_split(zc, N, S.shape[1])[0]
        err = np.max(np.abs(X[b] - Xc[0]))
        print(f"row {b}: status gpu {st[b]} oracle {stc[0]}  max|X - X_oracle| {err:.2e}")
        assert stc[0] == 0  # (chosen so on the CPU)
        assert st[b] == stc[0]
        assert err <= 1e-8


# ---- 6. adjoint against the dense reference ----
@pytest.mark.parametrize("b,label", [(0, "the scene itself (active)"), (2, "obstacle 0 widened")])
def test_adjoint_matches_dense_in_the_rows_scene(b, label):
    case, (S, D), (x0b, xrb, urb, gXb, gUb), out, rp, _ = batch("a")
    N, p, Q, R, bnd = case[:5]
    I = out[6]
    P = orf.problem(N, p, Q, R, bnd, S[b])
    P.dmin = D[b]
    dense = hx.check_against_dense(osr, osr.dense_scene_vjp, osr.model_scene_vjp, osr.scales, osr.KEYS,
                                   (P, I[b], gXb[b], gUb[b], xrb[b], urb[b]), hx.row(rp, b, hx.got_map(7)),
                                   rp.vjp_status[b], label)
    assert abs(dense["dmin"]) > 1.0  # the row's d_min constraint is active


# ---- device entries ----
def _device_run(s, x0b, xrb, urb, gXb, gUb, S, D):
    """solve_device and vjp_device (params) with per-instance scenes on torch tensors -> dict of host arrays."""
    import torch
    N, M, B = s.N, s.M, len(x0b)
    dev = torch.device("cuda", s.device)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
    dx0, dxr, dur, dgx, dgu, dS, dD = (t(a) for a in (x0b, xrb, urb, gXb, gUb, S, D))
    f = lambda *shape: torch.full(shape, 7.0, dtype=torch.float64, device=dev)  # noqa: E731
    o = {"X": f(B, N + 1, 6), "U": f(B, N, 2), "Z": f(B, s.n), "kkt": f(B), "I": f(B, s.iterate_len()),
         "g_x0": f(B, 6), "g_xref": f(B, N + 1, 6), "g_uref": f(B, N, 2), "g_obstacles": f(B, M, 4), "g_dmin": f(B)}
    o["status"] = torch.full((B,), 7, dtype=torch.int32, device=dev)
    o["iters"] = torch.full((B,), 7, dtype=torch.int32, device=dev)
    o["vjp_status"] = torch.full((B,), 7, dtype=torch.int32, device=dev)
    wk = torch.empty((B * s.vjp_params_work_bytes() // 8,), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    p = {k: v.data_ptr() for k, v in o.items()}
    s.solve_device(B, dx0.data_ptr(), 0, dxr.data_ptr(), dur.data_ptr(), 0, p["X"], p["U"], p["Z"], p["status"],
                   iters=p["iters"], kkt=p["kkt"], stream=stream, iterate=p["I"], obstacles=dS.data_ptr(),
                   d_min=dD.data_ptr())
    s.vjp_device(B, p["I"], p["status"], grad_x=dgx.data_ptr(), grad_u=dgu.data_ptr(), g_x0=p["g_x0"],
                 g_xref=p["g_xref"], g_uref=p["g_uref"], vjp_status=p["vjp_status"], stream=stream,
                 g_obstacles=p["g_obstacles"], g_dmin=p["g_dmin"], work=wk.data_ptr(), obstacles=dS.data_ptr(),
                 d_min=dD.data_ptr())
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in o.items()}


def test_device_entries_are_the_host_entries():
    case, (S, D), (x0b, xrb, urb, gXb, gUb), out, rp, _ = batch("a")
    d = _device_run(_solver(case), x0b, xrb, urb, gXb, gUb, S, D)
    for k, v in zip(("X", "U", "Z", "status", "iters", "kkt", "I"), out):
        assert np.array_equal(d[k], v), k
    for k in ("g_x0", "g_xref", "g_uref", "g_obstacles", "g_dmin", "vjp_status"):
        assert np.array_equal(d[k], getattr(rp, k)), k


# ---- 7. autograd ----
def test_autograd_per_instance_scene_inputs():
    import torch
    from ttmpc.diff import DifferentiableObcaTracking
    case, (S, D), (x0b, xrb, urb, gXb, gUb), out, rp, _ = batch("a")
    s = _solver(case)
    dev = torch.device("cuda", s.device)
    layer = DifferentiableObcaTracking(s)
    t = lambda a: torch.as_tensor(a, device=dev)  # noqa: E731
    x0, xr, ur = (t(a).clone().requires_grad_(True) for a in (x0b, xrb, urb))
    obs = t(S).clone().requires_grad_(True)
    dmin = t(D).clone().requires_grad_(True)
    Xo, Uo, sto = layer(x0, xr, ur, obstacles=obs, d_min=dmin)
    assert np.array_equal(Xo.detach().cpu().numpy(), out[0])
    ((Xo * t(gXb)).sum() + (Uo * t(gUb)).sum()).backward()
    d = _device_run(_solver(case), x0b, xrb, urb, gXb, gUb, S, D)
    assert tuple(obs.grad.shape) == S.shape and tuple(dmin.grad.shape) == D.shape
    assert np.array_equal(obs.grad.cpu().numpy(), d["g_obstacles"])
    assert np.array_equal(dmin.grad.cpu().numpy(), d["g_dmin"])
    assert np.array_equal(x0.grad.cpu().numpy(), d["g_x0"])
    go, gd = obs.grad.cpu().numpy(), dmin.grad.cpu().numpy()
    unit = np.abs(d["g_x0"][1]).max()
    assert np.abs(go[1]).max() <= 1e-9 * unit and abs(gd[1]) <= 1e-9 * unit   # the inactive row: rounding level
    assert np.abs(go[0]).max() > 1.0 and abs(gd[0]) > 1.0                     # the active row
    assert not np.array_equal(go[0], go[2]) and not np.array_equal(gd[0], gd[3])
    # the handle's scene is untouched by the per-instance path
    ob1, dm1 = s.scene()
    assert np.array_equal(ob1, case[5]) and dm1 == 0.2


# ---- 10. refusals and isolation ----
def test_refused_calls_write_nothing():
    import ttmpc
    case, (S, D), (x0b, xrb, urb, gXb, gUb), out, _, _ = batch("a")
    N, p, Q, R, bnd, obs = case[:6]
    B = len(D)
    s = _solver(case)
    kw = dict(xref=xrb, uref=urb)
    for bad in (S[:5], S[:, 0], np.tile(S, (1, 2, 1)), S[..., :3]):  # wrong B, no M axis, wrong M, wrong width
        with pytest.raises(ValueError):
            s.solve(x0b, obstacles=bad, **kw)
        with pytest.raises(ValueError):
            s.vjp(out[6], out[3], gXb, gUb, obstacles=bad)
    with pytest.raises(ValueError):
        s.solve(x0b, d_min=D[:5], **kw)
    with pytest.raises(ValueError):
        s.vjp(out[6], out[3], gXb, gUb, params=True, d_min=np.tile(D, (2, 1)))
    # values tt_set_scene refuses: -EINVAL from the host entry, no output written
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    P = lambda a: a.ctypes.data_as(dp)  # noqa: E731
    nan, flat, neg = S.copy(), S.copy(), D.copy()
    nan[4, 0, 1] = np.nan
    flat[2, 0, 2] = 0.0
    neg[5] = -0.01
    for So, Do in ((nan, D), (flat, D), (S, neg)):
        X, U = np.full((B, N + 1, 6), 7.0), np.full((B, N, 2), 7.0)
        st = np.full(B, 7, np.int32)
        sc_arg = ttmpc._lib.TTObcaScenes(So.ctypes.data, Do.ctypes.data)
        rc = s._L.tt_obca_solve_batch_scenes(s._h, B, P(x0b), None, P(xrb), P(urb), None, P(X), P(U), None,
                                             st.ctypes.data_as(ip), None, None, None, C.byref(sc_arg))
        assert rc == -22
        assert np.all(X == 7.0) and np.all(U == 7.0) and np.all(st == 7)
        with pytest.raises(ttmpc.TTError, match="-22"):
            s.solve(x0b, obstacles=So, d_min=Do, **kw)
        with pytest.raises(ttmpc.TTError, match="-22"):
            s.vjp(out[6], out[3], gXb, gUb, obstacles=So, d_min=Do)
    # a tracking handle
    track = ttmpc.BatchSolver(N, p, Q, R, *bnd)
    X, U = np.full((B, N + 1, 6), 7.0), np.full((B, N, 2), 7.0)
    st = np.full(B, 7, np.int32)
    sc_arg = ttmpc._lib.TTObcaScenes(S.ctypes.data, D.ctypes.data)
    rc = track._L.tt_obca_solve_batch_scenes(track._h, B, P(x0b), None, P(xrb), P(urb), None, P(X), P(U), None,
                                             st.ctypes.data_as(ip), None, None, None, C.byref(sc_arg))
    assert rc == -22 and np.all(st == 7)
    o4 = ttmpc._lib.TTObcaVjpParamsOut(*[None] * 8)
    rc = track._L.tt_obca_vjp_scenes(track._h, B, P(out[6]), out[3].ctypes.data_as(ip), None, None, P(gXb), P(gUb),
                                     C.byref(o4), C.byref(sc_arg))
    assert rc == -22


@pytest.mark.parametrize("kind", ["nan", "w <= 0", "d_min < 0"])
def test_invalid_scene_on_the_device_path_is_isolated(kind):
    """The device entry cannot read the scenes on the host: the instance checks its own row, ends TT_NONFINITE with 0
    iterations and the initial guess, its adjoint row is skipped with zeros, and the other rows are bitwise the
    family's."""
    import ttmpc
    case, (S, D), (x0b, xrb, urb, gXb, gUb), out, rp, _ = batch("a")
    So, Do, bad = S.copy(), D.copy(), 1
    if kind == "nan":
        So[bad, 0, 0] = np.nan
    elif kind == "w <= 0":
        So[bad, 0, 2] = -1.0
    else:
        Do[bad] = -0.05
    d = _device_run(_solver(case), x0b, xrb, urb, gXb, gUb, So, Do)
    assert d["status"][bad] == ttmpc.TT_NONFINITE and d["iters"][bad] == 0
    assert np.array_equal(d["X"][bad], xrb[bad]) and np.array_equal(d["U"][bad], urb[bad])  # the initial guess
    assert d["vjp_status"][bad] in (1, 2)
    for k in ("g_x0", "g_xref", "g_uref", "g_obstacles", "g_dmin"):
        assert np.all(d[k][bad] == 0.0), k
    keep = np.arange(len(D)) != bad
    for k, v in zip(("X", "U", "Z", "status", "iters", "kkt", "I"), out):
        assert np.array_equal(d[k][keep], v[keep]), k
    for k in ("g_x0", "g_xref", "g_uref", "g_obstacles", "g_dmin", "vjp_status"):
        assert np.array_equal(d[k][keep], getattr(rp, k)[keep]), k
