"""Test helper for the GPU suites of the MPC+OBCA adjoint (test_gpu_obca_vjp, _scene_vjp, _geometry_vjp, _scenes): the
solver builder, the solved batches the suites share, the golden window at the drivers' shape, a result row under the
references' keys, the comparison with the dense solve, the device call and the tiling check.  torch and ttmpc are imported
inside the functions, so that collecting the suites needs neither."""
import functools

import numpy as np

import obca_vjp_reference as orf

MODEL_CAP = 1e-9
# reference key -> member of the result (the scene suites use the first seven, the plain suite the first three)
GOT = {"x0": "g_x0", "xref": "g_xref", "uref": "g_uref", "obs": "g_obstacles", "dmin": "g_dmin", "Q": "g_Q", "R": "g_R",
       "geom": "g_geometry"}
OUT4 = ("g_x0", "g_xref", "g_uref", "vjp_status")
OUT8 = ("g_x0", "g_xref", "g_uref", "g_obstacles", "g_dmin", "g_Q", "g_R", "vjp_status")
OUT9 = OUT8[:7] + ("g_geometry", "vjp_status")


def got_map(n):
    """The first n entries of GOT."""
    return dict(list(GOT.items())[:n])


def solver(case, **kw):
    import ttmpc
    N, p, Q, R, bnd, obs = case[:6]
    return ttmpc.ObcaSolver(N, p, Q, R, *bnd, obs, variant=ttmpc.TT_VARIANT_TRACK_OBCA, **kw)


@functools.lru_cache(maxsize=None)
def solved_a():
    """B = 4 on case A's handle: case A; the inactive variant (the whole scene moved 2.5 m back, which is the obstacle
    at cx = 13); x_init[1] = -0.1; x_init outside the box (v above its bound), which cannot be solved.
    -> (case, solver, (x0b, xrb, urb), (X, U, st, I), (gXb, gUb))"""
    case = orf.case_a()
    N, p, Q, R, bnd, obs, x0, xr, ur = case
    xs, rs = [x0], [xr]
    a, b = x0.copy(), xr.copy()
    a[0] -= 2.5
    b[:, 0] -= 2.5
    xs.append(a)
    rs.append(b)
    c = x0.copy()
    c[1] = -0.1
    xs.append(c)
    rs.append(xr)
    d = x0.copy()
    d[5] = 11.0
    xs.append(d)
    rs.append(xr)
    x0b, xrb, urb = np.array(xs), np.array(rs), np.tile(ur, (4, 1, 1))
    s = solver(case)
    X, U, Z, st, it, kk, I = s.solve(x0b, xref=xrb, uref=urb, iterate=True)
    gX, gU = orf.upstream(N)
    return case, s, (x0b, xrb, urb), (X, U, st, I), (np.tile(gX, (4, 1, 1)), np.tile(gU, (4, 1, 1)))


@functools.lru_cache(maxsize=None)
def solved_b():
    """Case B (N = 8, M = 2), B = 1 -> (case, solver, (X, U, st, I), (gX, gU))."""
    case = orf.case_b()
    N, p, Q, R, bnd, obs, x0, xr, ur = case
    s = solver(case)
    X, U, Z, st, it, kk, I = s.solve(x0[None], xref=xr[None], uref=ur[None], iterate=True)
    return case, s, (X, U, st, I), orf.upstream(N)


def golden_windows(pick):
    """The picked golden MPC+OBCA windows at the drivers' shape N = 50, M = 11 (1122 blocks: 70 full rounds and a tail
    of 2), solved in one launch -> (solver, the oracle's problem, st, I, (gX, gU), xref[pick], uref[pick])."""
    import ttmpc
    from conftest import GOLDEN
    from ttmpc import scenarios as sc
    g = np.load(GOLDEN / "reference_numpy.npz")
    obs = g["obstacles"]
    x0, xr, ur = sc.mpc_obs_batch(g["state_traj"], g["input_traj"], 16, 50, seed=0)
    p = dict(sc.OBCA_PARAMS, dt=0.05)
    bnd = (sc.XLB, sc.XUB, sc.ULB, sc.UUB)
    s = ttmpc.ObcaSolver(50, p, sc.OBCA_Q, sc.OBCA_R, *bnd, obs, variant=ttmpc.TT_VARIANT_TRACK_OBCA)
    X, U, Z, st, it, kk, I = s.solve(x0[pick], xref=xr[pick], uref=ur[pick], iterate=True)
    assert np.all(st <= 1), st
    return s, orf.problem(50, p, sc.OBCA_Q, sc.OBCA_R, bnd, obs), st, I, orf.upstream(50), xr[pick], ur[pick]


def row(r, b, got):
    """Instance b of a result under the reference's keys (got: reference key -> member)."""
    return {k: (float(getattr(r, a)[b]) if k == "dmin" else getattr(r, a)[b]) for k, a in got.items()}


def check_against_dense(ref, dense_fn, model_fn, scales_fn, keys, args, got, vjp_status, label, sparse=False,
                        word="scales"):
    """The house rule on one instance: err_gpu <= 10 err_model + 1e-12 scale per group with the cap
    err_model <= 1e-9 scale, both against dense_fn(*args) on the kernel's own iterate; model_fn(*args) is the numpy
    model of the kernel, scales_fn(dense) the unit of each group and ref.group_err the distance.  Prints every figure
    before it asserts.  -> dense."""
    dense = dense_fn(*args, sparse=sparse)
    model = model_fn(*args)
    sc, em, eg = scales_fn(dense), ref.group_err(model, dense), ref.group_err(got, dense)
    text = f"{label}: {word} {sc}\n   model vs dense {em}\n   gpu   vs dense {eg}"
    if "geom" in keys:
        text += f"\n   geometry dense {dense['geom']}\n   geometry gpu   {got['geom']}"
    print(text)
    assert model["ok"] and vjp_status == 0
    for k in keys:
        assert eg[k] <= 10.0 * em[k] + 1e-12 * sc[k], (label, k, eg[k], em[k])
    for k in keys:
        assert em[k] <= MODEL_CAP * sc[k], (label, k, em[k], MODEL_CAP * sc[k])
    return dense


def device_call(s, B, I, st, gX, gU, xr=None, ur=None, ob=None, keys=OUT4, want=None, work=False):
    """ObcaSolver.vjp_device on torch tensors -> dict of host arrays over ``keys``.  Every output starts as 7 and only
    those in ``want`` (default: all of keys) are handed to the call; xr, ur, ob (per-instance obstacles) and the work
    buffer are handed over where given."""
    import torch
    N, M = s.N, s.M
    dev = torch.device("cuda", s.device)
    t = lambda a: None if a is None else torch.as_tensor(a, device=dev).contiguous()  # noqa: E731
    p = lambda a: 0 if a is None else a.data_ptr()  # noqa: E731
    dI, dgx, dgu, dxr, dur, dob = t(I), t(gX), t(gU), t(xr), t(ur), t(ob)
    dst = torch.as_tensor(st.astype(np.int32), device=dev)
    shapes = {"g_x0": (B, 6), "g_xref": (B, N + 1, 6), "g_uref": (B, N, 2), "g_obstacles": (B, M, 4), "g_dmin": (B,),
              "g_Q": (B, 6, 6), "g_R": (B, 2, 2), "g_geometry": (B, 5)}
    out = {k: torch.full(shapes[k], 7.0, dtype=torch.float64, device=dev) for k in keys if k != "vjp_status"}
    out["vjp_status"] = torch.full((B,), 7, dtype=torch.int32, device=dev)
    wk = torch.empty((B * s.vjp_params_work_bytes() // 8,), dtype=torch.float64, device=dev) if work else None
    s.vjp_device(B, dI.data_ptr(), dst.data_ptr(), grad_x=p(dgx), grad_u=p(dgu), xref=p(dxr), uref=p(dur), work=p(wk),
                 obstacles=p(dob), **{k: (v.data_ptr() if want is None or k in want else 0) for k, v in out.items()},
                 stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_tiling(call, d4, T, *arrays):
    """T tiles of a batch return its rows d4 bitwise and two launches agree bitwise; call(*tiled arrays) -> dict."""
    args = [np.tile(a, (T,) + (1,) * (a.ndim - 1)) for a in arrays]
    big, again = call(*args), call(*args)
    for k in d4:
        assert np.array_equal(big[k], again[k]), k
        assert np.array_equal(big[k].reshape((T,) + d4[k].shape), np.broadcast_to(d4[k], (T,) + d4[k].shape)), k
