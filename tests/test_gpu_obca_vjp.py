"""GPU tests of the MPC+OBCA adjoint (tt_obca_vjp*, obca_vjp_kernel): against the dense un-condensed solve on the
kernel's own iterate, against central differences of the CPU oracle, determinism, NULL handling, the refused handles
and the host entry.  The accuracy rule is err_gpu <= 10 err_model + 1e-12 max|ref| per group with the cap
err_model <= 1e-9 max|ref| (tests/test_obca_vjp_reference.py states what the model measures against that cap).

Measured on an MI355X (x0 group, kernel vs dense | model vs dense on the kernel's iterate): case A 9.3e-12 | 9.3e-12;
inactive 4.4e-15 | 4.4e-15; x_init[1] = -0.1 1.2e-11 | 1.2e-11; N = 8, M = 2 7.2e-13 | 7.2e-13; golden window 10 at
N = 50, M = 11 2.2e-12 | 2.3e-13 on a largest entry of 331 ("Adjoint of an MPC+OBCA solve").
"""
import ctypes as C
import functools

import numpy as np
import pytest

import obca_vjp_reference as orf

pytestmark = pytest.mark.gpu

MODEL_CAP = 1e-9


def _solver(case, **kw):
    import ttmpc
    N, p, Q, R, bnd, obs = case[:6]
    return ttmpc.ObcaSolver(N, p, Q, R, *bnd, obs, variant=ttmpc.TT_VARIANT_TRACK_OBCA, **kw)


def _shift(x0, xr, dx):
    x0, xr = x0.copy(), xr.copy()
    x0[0] += dx
    xr[:, 0] += dx
    return x0, xr


@functools.lru_cache(maxsize=None)
def batch_a():
    """B = 4 on case A's handle: case A; the inactive variant (the whole scene moved 2.5 m back, which is the obstacle
    at cx = 13); x_init[1] = -0.1; x_init outside the box (v above its bound), which cannot be solved."""
    case = orf.case_a()
    N, p, Q, R, bnd, obs, x0, xr, ur = case
    xs, rs = [x0], [xr]
    a, b = _shift(x0, xr, -2.5)
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
    s = _solver(case)
    X, U, Z, st, it, kk, I = s.solve(x0b, xref=xrb, uref=urb, iterate=True)
    gX, gU = orf.upstream(N)
    gXb, gUb = np.tile(gX, (4, 1, 1)), np.tile(gU, (4, 1, 1))
    r = s.vjp(I, st, gXb, gUb)
    return case, s, (x0b, xrb, urb), (X, U, st, I), (gXb, gUb), r


@functools.lru_cache(maxsize=None)
def batch_b():
    case = orf.case_b()
    N, p, Q, R, bnd, obs, x0, xr, ur = case
    s = _solver(case)
    X, U, Z, st, it, kk, I = s.solve(x0[None], xref=xr[None], uref=ur[None], iterate=True)
    gX, gU = orf.upstream(N)
    return case, s, (X, U, st, I), (gX, gU), s.vjp(I, st, gX[None], gU[None])


def _check_against_dense(P, I, gX, gU, r, b, label, sparse=False):
    dense = orf.dense_obca_vjp(P, I, gX, gU, sparse=sparse)
    model = orf.model_obca_vjp(P, I, gX, gU)
    got = {"x0": r.g_x0[b], "xref": r.g_xref[b], "uref": r.g_uref[b]}
    mx, em, eg = orf.group_max(dense), orf.group_err(model, dense), orf.group_err(got, dense)
    print(f"{label}: largest {mx}\n   model vs dense {em}\n   gpu   vs dense {eg}")
    assert model["ok"] and r.vjp_status[b] == 0
    for k in orf.KEYS:
        assert eg[k] <= 10.0 * em[k] + 1e-12 * mx[k], (label, k, eg[k], em[k])
    for k in orf.KEYS:
        assert em[k] <= MODEL_CAP * mx[k], (label, k, em[k], MODEL_CAP * mx[k])


@pytest.mark.parametrize("b,label", [(0, "case A"), (1, "inactive"), (2, "x_init[1] = -0.1")])
def test_kernel_matches_dense_on_its_own_iterate(b, label):
    """Measured on the GPU: module docstring."""
    case, s, _, (X, U, st, I), (gXb, gUb), r = batch_a()
    assert st[b] <= 1
    P = orf.problem(*case[:6])
    _check_against_dense(P, I[b], gXb[b], gUb[b], r, b, label)
    assert np.all(r.g_xref[b, 0] == 0.0)


def test_unsolved_instance_is_skipped():
    _, _, _, (X, U, st, I), _, r = batch_a()
    assert st[3] > 1, st
    assert r.vjp_status[3] == 2
    assert np.all(r.g_x0[3] == 0.0) and np.all(r.g_xref[3] == 0.0) and np.all(r.g_uref[3] == 0.0)


def test_kernel_matches_dense_with_several_blocks():
    case, s, (X, U, st, I), (gX, gU), r = batch_b()
    assert st[0] <= 1
    v = orf.unpack(I[0], case[0], 2)
    assert np.abs(v["yd"][..., 0]).max() > 1.0 and v["zLu"].max() > 1e-3
    _check_against_dense(orf.problem(*case[:6]), I[0], gX, gU, r, 0, "N = 8, M = 2")


def test_kernel_matches_central_differences_of_the_oracle():
    case, s, _, (X, U, st, I), (gXb, gUb), r = batch_a()
    N, p, Q, R, bnd, obs, x0, xr, ur = case
    _, sto, fd = orf.oracle_fd_vjp(orf.problem(*case[:6]), x0, xr, ur, gXb[0], gUb[0])
    got = {"x0": r.g_x0[0], "xref": r.g_xref[0], "uref": r.g_uref[0]}
    err = orf.group_err(got, fd)
    print("gpu vs central differences of the oracle", err)
    for k in orf.KEYS:
        assert err[k] <= 1e-5, (k, err[k])


def test_full_size_windows():
    """B = 2 at the drivers' shape N = 50, M = 11 (1122 blocks: 70 full rounds and a tail of 2): window 0 (open road)
    and window 10 (obstacle rows active) of the golden MPC+OBCA windows, both against the sparse un-condensed solve
    (SuperLU, refined on an extended-precision residual) by the module's rule."""
    import ttmpc
    from conftest import GOLDEN
    from ttmpc import scenarios as sc
    g = np.load(GOLDEN / "reference_numpy.npz")
    obs = g["obstacles"]
    x0, xr, ur = sc.mpc_obs_batch(g["state_traj"], g["input_traj"], 16, 50, seed=0)
    pick = [0, 10]
    p = dict(sc.OBCA_PARAMS, dt=0.05)
    bnd = (sc.XLB, sc.XUB, sc.ULB, sc.UUB)
    s = ttmpc.ObcaSolver(50, p, sc.OBCA_Q, sc.OBCA_R, *bnd, obs, variant=ttmpc.TT_VARIANT_TRACK_OBCA)
    X, U, Z, st, it, kk, I = s.solve(x0[pick], xref=xr[pick], uref=ur[pick], iterate=True)
    assert np.all(st <= 1), st
    gX, gU = orf.upstream(50)
    r = s.vjp(I, st, np.tile(gX, (2, 1, 1)), np.tile(gU, (2, 1, 1)))
    assert np.all(r.vjp_status == 0), r.vjp_status
    P = orf.problem(50, p, sc.OBCA_Q, sc.OBCA_R, bnd, obs)
    _check_against_dense(P, I[0], gX, gU, r, 0, "window 0", sparse=True)
    assert np.abs(orf.unpack(I[1], 50, 11)["yd"][..., 0]).max() > 1.0
    _check_against_dense(P, I[1], gX, gU, r, 1, "window 10", sparse=True)


def _device_call(s, B, I, st, gX, gU, want=("g_x0", "g_xref", "g_uref", "vjp_status")):
    import torch
    N = s.N
    dev = torch.device("cuda", s.device)
    dI = torch.as_tensor(I, device=dev).contiguous()
    dst = torch.as_tensor(st.astype(np.int32), device=dev)
    dgx = None if gX is None else torch.as_tensor(gX, device=dev).contiguous()
    dgu = None if gU is None else torch.as_tensor(gU, device=dev).contiguous()
    out = {"g_x0": torch.full((B, 6), 7.0, dtype=torch.float64, device=dev),
           "g_xref": torch.full((B, N + 1, 6), 7.0, dtype=torch.float64, device=dev),
           "g_uref": torch.full((B, N, 2), 7.0, dtype=torch.float64, device=dev),
           "vjp_status": torch.full((B,), 7, dtype=torch.int32, device=dev)}
    s.vjp_device(B, dI.data_ptr(), dst.data_ptr(), grad_x=0 if dgx is None else dgx.data_ptr(),
                 grad_u=0 if dgu is None else dgu.data_ptr(),
                 **{k: (v.data_ptr() if k in want else 0) for k, v in out.items()},
                 stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_determinism_tiling_and_host_entry():
    """300 tiles of the B = 4 batch return the B = 4 results bitwise, two launches agree bitwise, and the host entry is
    the device entry."""
    _, s, _, (X, U, st, I), (gXb, gUb), r = batch_a()
    d4 = _device_call(s, 4, I, st, gXb, gUb)
    for k, ref in (("g_x0", r.g_x0), ("g_xref", r.g_xref), ("g_uref", r.g_uref), ("vjp_status", r.vjp_status)):
        assert np.array_equal(d4[k], ref), k
    T = 300
    big = _device_call(s, 4 * T, np.tile(I, (T, 1)), np.tile(st, T), np.tile(gXb, (T, 1, 1)), np.tile(gUb, (T, 1, 1)))
    again = _device_call(s, 4 * T, np.tile(I, (T, 1)), np.tile(st, T), np.tile(gXb, (T, 1, 1)), np.tile(gUb, (T, 1, 1)))
    for k in d4:
        assert np.array_equal(big[k], again[k]), k
        assert np.array_equal(big[k].reshape((T,) + d4[k].shape), np.broadcast_to(d4[k], (T,) + d4[k].shape)), k


def test_null_members_and_null_gradient():
    _, s, _, (X, U, st, I), (gXb, gUb), r = batch_a()
    part = _device_call(s, 4, I, st, gXb, gUb, want=("g_uref",))
    assert np.array_equal(part["g_uref"], r.g_uref)
    assert np.all(part["g_x0"] == 7.0) and np.all(part["g_xref"] == 7.0) and np.all(part["vjp_status"] == 7)
    nul = _device_call(s, 4, I, st, None, gUb)
    zer = _device_call(s, 4, I, st, np.zeros_like(gXb), gUb)
    for k in nul:
        assert np.array_equal(nul[k], zer[k]), k
    rh = s.vjp(I, st, None, gUb)
    assert np.array_equal(rh.g_x0, zer["g_x0"])


def test_refused_calls():
    import ttmpc
    from ttmpc import scenarios as sc
    case, s, _, (X, U, st, I), (gXb, gUb), _ = batch_a()
    with pytest.raises(ttmpc.TTError, match="-22"):
        s.vjp(I, st, None, None)
    N, p, Q, R, bnd, obs = case[:6]
    plan = ttmpc.ObcaSolver(N, p, Q, R, *bnd, obs, variant=ttmpc.TT_VARIANT_OBCA_PLAN)
    with pytest.raises(ttmpc.TTError, match="-22"):
        plan.vjp(I, st, gXb, gUb)
    track = ttmpc.BatchSolver(N, p, Q, R, *bnd)
    out = ttmpc._lib.TTObcaVjpOut(None, None, None, None)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rc = track._L.tt_obca_vjp(track._h, 4, I.ctypes.data_as(dp), st.astype(np.int32).ctypes.data_as(ip),
                              gXb.ctypes.data_as(dp), gUb.ctypes.data_as(dp), C.byref(out))
    assert rc == -22


def test_autograd_layer_is_the_device_call_and_passes_a_directional_check():
    """DifferentiableObcaTracking's backward is tt_obca_vjp_device, bitwise; a directional central difference of the GPU
    solve along a fixed random direction in (x0, xref, uref) agrees with the gradient to 1e-5 relative to the largest
    of the two (h = 1e-4: the oracle's differences of case A agree with the dense adjoint to 2e-6)."""
    import torch
    from ttmpc.diff import DifferentiableObcaTracking
    case, s, (x0b, xrb, urb), (X, U, st, I), (gXb, gUb), r = batch_a()
    dev = torch.device("cuda", s.device)
    layer = DifferentiableObcaTracking(s)
    t = lambda a: torch.as_tensor(a, device=dev)  # noqa: E731
    x0, xr, ur = (t(a[:3]).clone().requires_grad_(True) for a in (x0b, xrb, urb))
    gX, gU = t(gXb[:3]), t(gUb[:3])
    Xo, Uo, sto = layer(x0, xr, ur)
    loss = (Xo * gX).sum() + (Uo * gU).sum()
    loss.backward()
    assert np.array_equal(x0.grad.cpu().numpy(), r.g_x0[:3])
    assert np.array_equal(xr.grad.cpu().numpy(), r.g_xref[:3])
    assert np.array_equal(ur.grad.cpu().numpy(), r.g_uref[:3])
    rng = np.random.default_rng(5)
    d0, dr, du = (t(rng.uniform(-1.0, 1.0, a.shape)) for a in (x0b[:3], xrb[:3], urb[:3]))
    dr[:, 0] = 0.0  # (xref_0 does not enter: x_0 is pinned)
    h = 1e-4
    with torch.no_grad():
        vals = []
        for sg in (1.0, -1.0):
            Xp, Up, stp = layer(x0 + sg * h * d0, xr + sg * h * dr, ur + sg * h * du)
            assert torch.all(stp <= 1)
            vals.append(((Xp * gX).sum(dim=(1, 2)) + (Up * gU).sum(dim=(1, 2))).cpu().numpy())
    fd = (vals[0] - vals[1]) / (2.0 * h)
    an = ((x0.grad * d0).sum(dim=1) + (xr.grad * dr).sum(dim=(1, 2)) + (ur.grad * du).sum(dim=(1, 2))).cpu().numpy()
    print("directional: differences", fd, "gradient", an)
    assert np.all(np.abs(fd - an) <= 1e-5 * np.maximum(1.0, np.maximum(np.abs(fd), np.abs(an))))
