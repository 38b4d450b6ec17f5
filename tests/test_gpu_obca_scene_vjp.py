"""GPU tests of the scene and weight gradients of an MPC+OBCA solve (tt_obca_vjp_params*, tt_set_scene, the params
instantiation of obca_vjp_kernel): against the dense un-condensed solve on the kernel's own iterate, end to end against
central differences of the GPU solve through tt_set_scene, determinism, NULL handling, the refused calls, the host entry
and the autograd layer.

The accuracy rule is the house rule, err_gpu <= 10 err_model + 1e-12 scale per group with the cap
err_model <= 1e-9 scale (tests/obca_scene_reference.py ``scales``: obs and d_min are measured against
max(their own max|ref|, max|g_x0|), every other group against its own max|ref|).

Measured on an MI355X (obs group, kernel vs dense | model vs dense on the kernel's iterate): case A 9.2e-12 | 9.2e-12;
inactive 1.3e-24 | 1.3e-24; x_init[1] = -0.1 1.2e-11 | 1.2e-11; N = 8, M = 2 5.3e-13 | 5.3e-13; golden window 10 at
N = 50, M = 11 2.3e-13 | 2.5e-14 on a scale of 331 (Q 6.9e-15 | 1.1e-15 on 0.26).  End to end through tt_set_scene:
cx 11.05360764 (differences) against 11.05360760, w -5.52680371 against -5.52680369, d_min -11.05360750 against
-11.05360749 ("Scene and weight gradients of an MPC+OBCA solve").
"""
import ctypes as C
import functools

import numpy as np
import pytest

import obca_scene_reference as osr
import obca_vjp_harness as hx
import obca_vjp_reference as orf

pytestmark = pytest.mark.gpu

GOT = hx.got_map(7)
_solver = hx.solver


@functools.lru_cache(maxsize=None)
def batch_a():
    """obca_vjp_harness.solved_a and its params adjoint."""
    case, s, (x0b, xrb, urb), (X, U, st, I), (gXb, gUb) = hx.solved_a()
    r = s.vjp(I, st, gXb, gUb, xref=xrb, uref=urb, params=True)
    return case, s, (x0b, xrb, urb), (X, U, st, I), (gXb, gUb), r


@functools.lru_cache(maxsize=None)
def batch_b():
    case, s, (X, U, st, I), (gX, gU) = hx.solved_b()
    xr, ur = case[7], case[8]
    return case, s, (X, U, st, I), (gX, gU), s.vjp(I, st, gX[None], gU[None], xref=xr[None], uref=ur[None], params=True)


def _check_against_dense(P, I, gX, gU, xr, ur, r, b, label, sparse=False):
    return hx.check_against_dense(osr, osr.dense_scene_vjp, osr.model_scene_vjp, osr.scales, osr.KEYS,
                                  (P, I, gX, gU, xr, ur), hx.row(r, b, GOT), r.vjp_status[b], label, sparse)


@pytest.mark.parametrize("b,label", [(0, "case A"), (1, "inactive"), (2, "x_init[1] = -0.1")])
def test_kernel_matches_dense_on_its_own_iterate(b, label):
    case, s, (x0b, xrb, urb), (X, U, st, I), (gXb, gUb), r = batch_a()
    assert st[b] <= 1
    P = orf.problem(*case[:6])
    dense = _check_against_dense(P, I[b], gXb[b], gUb[b], xrb[b], urb[b], r, b, label)
    if b == 0:  # a face contact: moving the face and widening the margin are one motion (the dense reference on the CPU
        # oracle's iterate holds both identities to 1e-8 relative: the contact normal is the x axis to 1e-9)
        assert abs(dense["dmin"]) > 1.0
        assert abs(r.g_obstacles[0, 0, 0] + r.g_dmin[0]) <= 1e-6 * abs(r.g_dmin[0])
        assert abs(r.g_obstacles[0, 0, 2] - 0.5 * r.g_dmin[0]) <= 1e-6 * abs(r.g_dmin[0])
    if b == 1:
        assert np.abs(r.g_obstacles[1]).max() <= 1e-9 * np.abs(r.g_x0[1]).max()
        assert abs(r.g_dmin[1]) <= 1e-9 * np.abs(r.g_x0[1]).max()


def test_unsolved_instance_is_skipped():
    _, _, _, (X, U, st, I), _, r = batch_a()
    assert st[3] > 1, st
    assert r.vjp_status[3] == 2
    for a in GOT.values():
        assert np.all(getattr(r, a)[3] == 0.0), a


def test_kernel_matches_dense_with_several_blocks():
    case, s, (X, U, st, I), (gX, gU), r = batch_b()
    N, p, Q, R, bnd, obs, x0, xr, ur = case
    assert st[0] <= 1
    dense = _check_against_dense(orf.problem(*case[:6]), I[0], gX, gU, xr, ur, r, 0, "N = 8, M = 2")
    assert np.abs(dense["obs"][0]).max() > 0.1  # the first obstacle is the one in contact


def test_full_size_window():
    """One instance at the drivers' shape N = 50, M = 11 (1122 blocks: 70 full rounds and a tail of 2): window 10
    (obstacle rows active) of the golden MPC+OBCA windows against the sparse un-condensed solve."""
    s, P, st, I, (gX, gU), xr, ur = hx.golden_windows([10])
    r = s.vjp(I, st, gX[None], gU[None], xref=xr, uref=ur, params=True)
    assert np.all(r.vjp_status == 0), r.vjp_status
    assert np.abs(orf.unpack(I[0], 50, 11)["yd"][..., 0]).max() > 1.0
    dense = _check_against_dense(P, I[0], gX, gU, xr[0], ur[0], r, 0, "window 10", sparse=True)
    assert abs(dense["dmin"]) > 1.0


def test_end_to_end_through_set_scene():
    """Central differences of the GPU solve itself in obstacle 0's cx and w and in d_min on case A (h = 1e-4) agree
    with the gradient to 1e-5 relative to max(1, both values); restoring the scene gives the first solve bitwise."""
    case, s0, (x0b, xrb, urb), (X0, U0, st0, I0), (gXb, gUb), r = batch_a()
    N, p, Q, R, bnd, obs, x0, xr, ur = case
    s = _solver(case)
    ob0, dm0 = s.scene()
    assert np.array_equal(ob0, obs) and dm0 == 0.2
    h = 1e-4

    def loss():
        X, U, Z, st, it, kk = s.solve(x0[None], xref=xr[None], uref=ur[None])
        assert st[0] <= 1
        return float((X[0] * gXb[0]).sum() + (U[0] * gUb[0]).sum()), X, U

    base, Xb, Ub = loss()
    assert np.array_equal(Xb[0], X0[0]) and np.array_equal(Ub[0], U0[0])
    for label, col, an in (("cx", 0, r.g_obstacles[0, 0, 0]), ("w", 2, r.g_obstacles[0, 0, 2]),
                           ("d_min", None, r.g_dmin[0])):
        vals = []
        for sg in (1.0, -1.0):
            if col is None:
                s.set_scene(d_min=0.2 + sg * h)
            else:
                ob = obs.copy()
                ob[0, col] += sg * h
                s.set_scene(obstacles=ob)
            vals.append(loss()[0])
            s.set_scene(obstacles=obs, d_min=0.2)
        fd = (vals[0] - vals[1]) / (2.0 * h)
        print(f"{label}: differences {fd} gradient {an}")
        assert abs(fd - an) <= 1e-5 * max(1.0, abs(fd), abs(an)), (label, fd, an)
    ob1, dm1 = s.scene()
    assert np.array_equal(ob1, obs) and dm1 == 0.2
    again, Xa, Ua = loss()
    assert np.array_equal(Xa, Xb) and np.array_equal(Ua, Ub)


def _device_call(s, B, I, st, gX, gU, xr, ur, want=None, work=True):
    return hx.device_call(s, B, I, st, gX, gU, xr, ur, keys=hx.OUT8, want=want, work=work)


def test_determinism_tiling_and_host_entry():
    """300 tiles of the B = 4 batch return the B = 4 results bitwise, two launches agree bitwise, and the host entry is
    the device entry."""
    _, s, (x0b, xrb, urb), (X, U, st, I), (gXb, gUb), r = batch_a()
    d4 = _device_call(s, 4, I, st, gXb, gUb, xrb, urb)
    for k in d4:
        assert np.array_equal(d4[k], getattr(r, k)), k
    T = 300
    hx.check_tiling(lambda *a: _device_call(s, 4 * T, *a), d4, T, I, st, gXb, gUb, xrb, urb)


def test_null_members_stay_untouched():
    _, s, (x0b, xrb, urb), (X, U, st, I), (gXb, gUb), r = batch_a()
    part = _device_call(s, 4, I, st, gXb, gUb, None, None, want=("g_dmin", "g_uref"))
    assert np.array_equal(part["g_dmin"], r.g_dmin) and np.array_equal(part["g_uref"], r.g_uref)
    for k in ("g_x0", "g_xref", "g_obstacles", "g_Q", "g_R", "vjp_status"):
        assert np.all(part[k] == 7), k


def test_refused_calls():
    import ttmpc
    case, s, (x0b, xrb, urb), (X, U, st, I), (gXb, gUb), _ = batch_a()
    N, p, Q, R, bnd, obs = case[:6]
    with pytest.raises(ttmpc.TTError, match="-22"):  # NULL work
        _device_call(s, 4, I, st, gXb, gUb, xrb, urb, work=False)
    with pytest.raises(ttmpc.TTError, match="-22"):  # g_Q without xref
        _device_call(s, 4, I, st, gXb, gUb, None, urb, want=("g_Q",))
    with pytest.raises(ttmpc.TTError, match="-22"):  # g_R without uref
        _device_call(s, 4, I, st, gXb, gUb, xrb, None, want=("g_R",))
    with pytest.raises(ttmpc.TTError, match="-22"):
        s.vjp(I, st, None, None, params=True)
    plan = ttmpc.ObcaSolver(N, p, Q, R, *bnd, obs, variant=ttmpc.TT_VARIANT_OBCA_PLAN)
    with pytest.raises(ttmpc.TTError, match="-22"):
        plan.vjp(I, st, gXb, gUb, params=True)
    plan.set_scene(d_min=0.3)  # (both OBCA variants have a scene)
    assert plan.scene()[1] == 0.3
    track = ttmpc.BatchSolver(N, p, Q, R, *bnd)
    out = ttmpc._lib.TTObcaVjpParamsOut(*[None] * 8)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    rc = track._L.tt_obca_vjp_params(track._h, 4, I.ctypes.data_as(dp), st.astype(np.int32).ctypes.data_as(ip), None,
                                     None, gXb.ctypes.data_as(dp), gUb.ctypes.data_as(dp), C.byref(out))
    assert rc == -22
    dm = np.array([0.3])
    assert track._L.tt_set_scene(track._h, None, dm.ctypes.data_as(dp)) == -22
    fresh = _solver(case)
    for bad_obs, bad_dm in ((np.array([[10.5, 1.0, 0.0, 3.0]]), None), (np.array([[10.5, np.nan, 2.0, 3.0]]), None),
                            (np.array([[10.5, 1.0, 2.0, -1.0]]), None), (None, -0.1), (None, np.inf)):
        with pytest.raises(ttmpc.TTError, match="-22"):
            fresh.set_scene(bad_obs, bad_dm)
    ob, dm = fresh.scene()
    assert np.array_equal(ob, obs) and dm == 0.2


def test_autograd_scene_inputs_are_the_device_call():
    """obstacles.grad and d_min.grad are bitwise the batch sums of the device call's rows, from a CPU tensor and from a
    device tensor; a scene changed between the forward and the backward raises."""
    import torch
    from ttmpc.diff import DifferentiableObcaTracking, _batch_sum
    case, s0, (x0b, xrb, urb), (X, U, st, I), (gXb, gUb), r = batch_a()
    s = _solver(case)
    dev = torch.device("cuda", s.device)
    layer = DifferentiableObcaTracking(s)
    t = lambda a: torch.as_tensor(a, device=dev)  # noqa: E731
    x0, xr, ur = (t(a[:3]).clone().requires_grad_(True) for a in (x0b, xrb, urb))
    gX, gU = t(gXb[:3]), t(gUb[:3])
    obs = torch.tensor(case[5], dtype=torch.float64, requires_grad=True)               # CPU
    dmin = torch.tensor(0.2, dtype=torch.float64, device=dev, requires_grad=True)      # device
    Xo, Uo, sto = layer(x0, xr, ur, obstacles=obs, d_min=dmin)
    assert np.array_equal(Xo.detach().cpu().numpy(), X[:3])
    ((Xo * gX).sum() + (Uo * gU).sum()).backward()
    d3 = _device_call(s0, 3, I[:3], st[:3], gXb[:3], gUb[:3], None, None,
                      want=("g_x0", "g_xref", "g_uref", "g_obstacles", "g_dmin"))
    assert obs.grad.device.type == "cpu" and dmin.grad.device == dev
    assert np.array_equal(obs.grad.numpy(), _batch_sum(t(d3["g_obstacles"]), "cpu").numpy())
    assert np.array_equal(dmin.grad.cpu().numpy(), _batch_sum(t(d3["g_dmin"]), "cpu").numpy())
    assert np.array_equal(x0.grad.cpu().numpy(), d3["g_x0"])
    assert np.array_equal(xr.grad.cpu().numpy(), d3["g_xref"])
    assert np.array_equal(ur.grad.cpu().numpy(), d3["g_uref"])
    # a new margin is applied by the forward and stays applied
    d2 = torch.tensor(0.25, dtype=torch.float64, requires_grad=True)
    Xo, Uo, sto = layer(x0, xr, ur, d_min=d2)
    assert s.scene()[1] == 0.25
    s.set_scene(d_min=0.2)
    with pytest.raises(RuntimeError, match="scene changed"):
        ((Xo * gX).sum() + (Uo * gU).sum()).backward()
