"""GPU tests of the geometry gradient of an MPC+OBCA solve (tt_obca_vjp_geometry*, tt_set_geometry, the geometry
instantiation of obca_vjp_kernel): against the dense un-condensed solve on the kernel's own iterate, end to end against
central differences of the GPU solve through tt_set_geometry, bitwise against the params call, determinism, the host
entry, the setter and the autograd layer.

The accuracy rule is the house rule, err_gpu <= 10 err_model + 1e-12 scale per group with the cap
err_model <= 1e-9 scale (tests/obca_geometry_reference.py ``scales``: the geometry group is measured against
max(its own max|ref|, max|g_x0|), as the obs group is).

Measured on an MI355X (geometry group, kernel vs dense | model vs dense on the kernel's iterate | scale): F 1.403e-12 |
1.404e-12 | 10.6; R 2.162e-12 | 2.155e-12 | 69.6; F with the obstacle 3 m away 3.5e-24 | 3.5e-24 | 2.95; N = 8, M = 2
5.32e-13 | 5.33e-13 | 2.90; golden window 10 at N = 50, M = 11 1.55e-13 | 5.84e-13 | 331 (dL/d(L1, L2, Mh, W1, W2) =
-0.0578, -3.692, -3.748, -1.2e-9, -10.736).  End to end through tt_set_geometry (h = 1e-4): F L1 -2.16377267 (differences)
against -2.16377178, W1 -0.70992451 against -0.70992458; R L2 10.91729824 against 10.91729812, M 10.91776712 against
10.91776724, W2 2.96308132 against 2.96308147 ("Geometry gradients of an MPC+OBCA solve").
"""
import ctypes as C
import functools

import numpy as np
import pytest

import obca_geometry_reference as ogr
import obca_vjp_harness as hx
import obca_vjp_reference as orf

pytestmark = pytest.mark.gpu

GOT = hx.GOT
SHARED = ("g_x0", "g_xref", "g_uref", "vjp_status", "g_obstacles", "g_dmin", "g_Q", "g_R")
NEW = dict(L1=7.3, L2=12.0, M=0.3, W1=2.9, W2=3.1)


_solver = hx.solver


@functools.lru_cache(maxsize=None)
def batch_f():
    """B = 4 on case F's handle with per-instance scenes: F; R; F with the obstacle moved 3 m away (no block is
    active); F with x_init outside the box (v = 11 above its bound), which cannot be solved."""
    f, r = ogr.case_f(), ogr.case_r()
    N = f[0]
    far = f[5].copy()
    far[0, 0] += 3.0
    bad = f[6].copy()
    bad[5] = 11.0
    x0b = np.array([f[6], r[6], f[6], bad])
    xrb = np.array([f[7], r[7], f[7], f[7]])
    urb = np.zeros((4, N, 2))
    obb = np.array([f[5], r[5], far, f[5]])
    s = _solver(f)
    X, U, Z, st, it, kk, I = s.solve(x0b, xref=xrb, uref=urb, iterate=True, obstacles=obb)
    gX, gU = orf.upstream(N)
    gXb, gUb = np.tile(gX, (4, 1, 1)), np.tile(gU, (4, 1, 1))
    res = s.vjp(I, st, gXb, gUb, xref=xrb, uref=urb, obstacles=obb, geometry=True)
    return f, s, (x0b, xrb, urb, obb), (X, U, st, I), (gXb, gUb), res


def _check_against_dense(P, I, gX, gU, xr, ur, r, b, label, sparse=False):
    return hx.check_against_dense(ogr, ogr.dense_geometry_vjp, ogr.model_geometry_vjp, ogr.scales, ogr.KEYS,
                                  (P, I, gX, gU, xr, ur), hx.row(r, b, GOT), r.vjp_status[b], label, sparse)


@pytest.mark.parametrize("b,label", [(0, "F"), (1, "R"), (2, "F, obstacle 3 m away")])
def test_kernel_matches_dense_on_its_own_iterate(b, label):
    case, s, (x0b, xrb, urb, obb), (X, U, st, I), (gXb, gUb), r = batch_f()
    assert st[b] <= 1
    P = orf.problem(*case[:5], obb[b])
    dense = _check_against_dense(P, I[b], gXb[b], gUb[b], xrb[b], urb[b], r, b, label)
    g = dict(zip(ogr.THETA, r.g_geometry[b]))
    if b == 0:
        assert abs(g["L1"]) > 1.0 and abs(g["W1"]) > 0.1
    if b == 1:
        assert abs(g["L2"]) > 1.0 and abs(g["Mh"]) > 1.0 and abs(g["W2"]) > 1.0
    if b == 2:  # no block share: the gradient is its dynamics share
        assert np.abs(dense["geom_block"]).max() <= 1e-9 * np.abs(dense["x0"]).max()
        assert np.all(r.g_geometry[b, 3:] == 0.0) or np.abs(r.g_geometry[b, 3:]).max() <= 1e-9 * np.abs(r.g_x0[b]).max()


def test_unsolved_instance_is_skipped():
    _, _, _, (X, U, st, I), _, r = batch_f()
    assert st[3] > 1, st
    assert r.vjp_status[3] == 2
    for a in GOT.values():
        assert np.all(getattr(r, a)[3] == 0.0), a


def test_kernel_matches_dense_with_several_blocks():
    case, s, (X, U, st, I), (gX, gU) = hx.solved_b()
    xr, ur = case[7], case[8]
    assert st[0] <= 1
    r = s.vjp(I, st, gX[None], gU[None], xref=xr[None], uref=ur[None], geometry=True)
    dense = _check_against_dense(orf.problem(*case[:6]), I[0], gX, gU, xr, ur, r, 0, "N = 8, M = 2")
    assert abs(dense["geom"][0]) > 1.0  # the truck's front face is in contact


def test_full_size_window():
    """One instance at the drivers' shape N = 50, M = 11 (1122 blocks: 70 full rounds and a tail of 2): window 10
    (obstacle rows active) of the golden MPC+OBCA windows against the sparse un-condensed solve."""
    s, P, st, I, (gX, gU), xr, ur = hx.golden_windows([10])
    r = s.vjp(I, st, gX[None], gU[None], xref=xr, uref=ur, geometry=True)
    assert np.all(r.vjp_status == 0), r.vjp_status
    dense = _check_against_dense(P, I[0], gX, gU, xr[0], ur[0], r, 0, "window 10", sparse=True)
    assert np.abs(dense["geom_block"]).max() > 1.0


@pytest.mark.parametrize("name,b,which", [("F", 0, ("L1", "W1")), ("R", 1, ("L2", "M", "W2"))])
def test_end_to_end_through_set_geometry(name, b, which):
    """Central differences of the GPU solve itself (h = 1e-4) through tt_set_geometry agree with the gradient to 1e-5
    relative to max(1, both values); restoring the geometry gives the first solve bitwise."""
    _, s0, (x0b, xrb, urb, obb), (X0, U0, st0, I0), (gXb, gUb), r = batch_f()
    case = ogr.case_f() if name == "F" else ogr.case_r()
    N, p, Q, R, bnd, obs, x0, xr, ur = case
    s = _solver(case)
    base = s.geometry()
    assert base == (p["L1"], p["L2"], p["M"], p["W1"], p["W2"])
    h = 1e-4

    def loss():
        X, U, Z, st, it, kk = s.solve(x0[None], xref=xr[None], uref=ur[None])
        assert st[0] <= 1
        return float((X[0] * gXb[b]).sum() + (U[0] * gUb[b]).sum()), X, U

    _, Xb, Ub = loss()
    assert np.array_equal(Xb[0], X0[b]) and np.array_equal(Ub[0], U0[b])  # (row b of the scenes batch is this solve)
    names = ("L1", "L2", "M", "W1", "W2")
    for key in which:
        i = names.index(key)
        an = r.g_geometry[b, i]
        vals = []
        for sg in (1.0, -1.0):
            s.set_geometry(**{key: base[i] + sg * h})
            vals.append(loss()[0])
            s.set_geometry(**{key: base[i]})
        fd = (vals[0] - vals[1]) / (2.0 * h)
        print(f"{name} {key}: differences {fd} gradient {an}")
        assert abs(fd - an) <= 1e-5 * max(1.0, abs(fd), abs(an)), (key, fd, an)
    assert s.geometry() == base
    _, Xa, Ua = loss()
    assert np.array_equal(Xa, Xb) and np.array_equal(Ua, Ub)


def test_shared_outputs_are_the_params_call_bitwise():
    """With g_geometry set the eight shared outputs are bitwise those of vjp(params=True, obstacles=...); with it NULL
    the entry is tt_obca_vjp_scenes: every output bitwise."""
    import ttmpc
    from ttmpc._lib import TTObcaScenes, TTObcaVjpGeometryOut
    _, s, (x0b, xrb, urb, obb), (X, U, st, I), (gXb, gUb), r = batch_f()
    ref = s.vjp(I, st, gXb, gUb, xref=xrb, uref=urb, params=True, obstacles=obb)
    for k in SHARED:
        assert np.array_equal(getattr(r, k), getattr(ref, k)), k
    N, M, B = s.N, s.M, 4
    out = {"g_x0": np.full((B, 6), 7.0), "g_xref": np.full((B, N + 1, 6), 7.0), "g_uref": np.full((B, N, 2), 7.0),
           "vjp_status": np.full(B, 7, dtype=np.int32), "g_obstacles": np.full((B, M, 4), 7.0), "g_dmin": np.full(B, 7.0),
           "g_Q": np.full((B, 6, 6), 7.0), "g_R": np.full((B, 2, 2), 7.0)}
    gout = TTObcaVjpGeometryOut(*[out[k].ctypes.data for k in SHARED], None)
    sc = TTObcaScenes(obb.ctypes.data, None)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(dp)  # noqa: E731
    rc = s._L.tt_obca_vjp_geometry(s._h, B, p(I), st.astype(np.int32).ctypes.data_as(ip), p(xrb), p(urb), p(gXb), p(gUb),
                                   C.byref(gout), C.byref(sc))
    assert rc == 0
    for k in SHARED:
        assert np.array_equal(out[k], getattr(ref, k)), k
    plan = ttmpc.ObcaSolver(N, ogr.case_f()[1], *ogr.case_f()[2:4], *ogr.case_f()[4], ogr.case_f()[5],
                            variant=ttmpc.TT_VARIANT_OBCA_PLAN)
    with pytest.raises(ttmpc.TTError, match="-22"):  # only TT_VARIANT_TRACK_OBCA, as its siblings
        plan.vjp(I, st, gXb, gUb, geometry=True)


def _device_call(s, B, I, st, gX, gU, xr, ur, ob, work=True):
    return hx.device_call(s, B, I, st, gX, gU, xr, ur, ob, keys=hx.OUT9, work=work)


def test_determinism_tiling_and_host_entry():
    """75 tiles of the B = 4 batch (B = 300) return the B = 4 rows bitwise, two launches agree bitwise, and the host
    entry is the device entry; a NULL work buffer is refused."""
    import ttmpc
    _, s, (x0b, xrb, urb, obb), (X, U, st, I), (gXb, gUb), r = batch_f()
    d4 = _device_call(s, 4, I, st, gXb, gUb, xrb, urb, obb)
    for k in d4:
        assert np.array_equal(d4[k], getattr(r, k)), k
    T = 75
    hx.check_tiling(lambda *a: _device_call(s, 4 * T, *a), d4, T, I, st, gXb, gUb, xrb, urb, obb)
    with pytest.raises(ttmpc.TTError, match="-22"):
        _device_call(s, 4, I, st, gXb, gUb, xrb, urb, obb, work=False)


def test_set_geometry_is_a_fresh_handle():
    """A solve after set_geometry(NEW) is bitwise a fresh handle's, on a TRACK_OBCA handle (case F) and on a plan
    handle (the toy plan, N = 60: the smallest horizon of the plan tests); setting it back restores the first bits; bad
    values and a tracking handle are refused with -EINVAL and the values are kept."""
    import ttmpc
    from test_obca_oracle import toy_plan
    case = ogr.case_f()
    N, p, Q, R, bnd, obs, x0, xr, ur = case
    pn = dict(p, **NEW)
    new = (NEW["L1"], NEW["L2"], NEW["M"], NEW["W1"], NEW["W2"])
    s = _solver(case)
    first = s.solve(x0[None], xref=xr[None], uref=ur[None], iterate=True)
    s.set_geometry(**NEW)
    assert s.geometry() == new
    moved = s.solve(x0[None], xref=xr[None], uref=ur[None], iterate=True)
    fresh_s = _solver((N, pn) + case[2:])
    fresh = fresh_s.solve(x0[None], xref=xr[None], uref=ur[None], iterate=True)
    assert not np.array_equal(moved[0], first[0])
    for a, b in zip(moved, fresh):
        assert np.array_equal(a, b)
    gX, gU = orf.upstream(N)
    ra = s.vjp(moved[6], moved[3], gX[None], gU[None], xref=xr[None], uref=ur[None], geometry=True)
    rb = fresh_s.vjp(fresh[6], fresh[3], gX[None], gU[None], xref=xr[None], uref=ur[None], geometry=True)
    for k in GOT.values():
        assert np.array_equal(getattr(ra, k), getattr(rb, k)), k
    s.set_geometry(L1=p["L1"], L2=p["L2"], M=p["M"], W1=p["W1"], W2=p["W2"])
    back = s.solve(x0[None], xref=xr[None], uref=ur[None], iterate=True)
    for a, b in zip(back, first):
        assert np.array_equal(a, b)
    # the plan variant
    from ttmpc import scenarios as sc
    Np, M, obs_p, x0p, xg, zg = toy_plan()
    pb = (sc.OBCA_XLB, sc.OBCA_XUB, sc.OBCA_ULB, sc.OBCA_UUB)
    mk = lambda prm: ttmpc.ObcaSolver(Np, prm, sc.OBCA_Q, sc.OBCA_R, *pb, obs_p,  # noqa: E731
                                      variant=ttmpc.TT_VARIANT_OBCA_PLAN)
    plan = mk(dict(sc.OBCA_PARAMS))
    p_first = plan.solve(x0p, xg, z_guess=zg)
    plan.set_geometry(**NEW)
    p_moved = plan.solve(x0p, xg, z_guess=zg)
    p_fresh = mk(dict(sc.OBCA_PARAMS, **NEW)).solve(x0p, xg, z_guess=zg)
    assert not np.array_equal(p_moved[0], p_first[0])
    for a, b in zip(p_moved, p_fresh):
        assert np.array_equal(a, b)
    q = sc.OBCA_PARAMS
    plan.set_geometry(L1=q["L1"], L2=q["L2"], M=q["M"], W1=q["W1"], W2=q["W2"])
    for a, b in zip(plan.solve(x0p, xg, z_guess=zg), p_first):
        assert np.array_equal(a, b)
    # refused values change nothing
    keep = s.geometry()
    for bad in (dict(L1=0.0), dict(L2=-1.0), dict(W1=0.0), dict(W2=np.inf), dict(M=np.nan), dict(L1=np.nan)):
        with pytest.raises(ttmpc.TTError, match="-22"):
            s.set_geometry(**bad)
        assert s.geometry() == keep
    track = ttmpc.BatchSolver(N, p, Q, R, *bnd)
    assert track._L.tt_set_geometry(track._h, 7.0, 12.0, 0.2, 3.0, 3.0) == -22
    assert track.model() == (p["L1"], p["L2"], p["M"])
    assert s._L.tt_set_model(s._h, 7.0, 12.0, 0.2) == -22  # tt_set_model keeps refusing OBCA handles
    assert s.geometry() == keep


def test_autograd_geometry_input_is_the_device_call():
    """geometry.grad is bitwise the batch sum of the device call's rows, from a CPU tensor; a geometry changed between
    the forward and the backward raises."""
    import torch
    from ttmpc.diff import DifferentiableObcaTracking, _batch_sum
    case, s0, (x0b, xrb, urb, obb), (X, U, st, I), (gXb, gUb), r = batch_f()
    s = _solver(case)
    dev = torch.device("cuda", s.device)
    layer = DifferentiableObcaTracking(s)
    t = lambda a: torch.as_tensor(a, device=dev)  # noqa: E731
    x0, xr, ur = (t(a[:3]).clone().requires_grad_(True) for a in (x0b, xrb, urb))
    ob = t(obb[:3].copy())
    gX, gU = t(gXb[:3]), t(gUb[:3])
    geom = torch.tensor(s.geometry(), dtype=torch.float64, requires_grad=True)  # CPU
    Xo, Uo, sto = layer(x0, xr, ur, obstacles=ob, geometry=geom)
    assert np.array_equal(Xo.detach().cpu().numpy(), X[:3])
    ((Xo * gX).sum() + (Uo * gU).sum()).backward()
    assert geom.grad.device.type == "cpu"
    assert np.array_equal(geom.grad.numpy(), _batch_sum(t(r.g_geometry[:3]), "cpu").numpy())
    assert np.array_equal(x0.grad.cpu().numpy(), r.g_x0[:3])
    assert np.array_equal(xr.grad.cpu().numpy(), r.g_xref[:3])
    # a new geometry is applied by the forward and stays applied
    g2 = torch.tensor([7.3, 12.0, 0.3, 2.9, 3.1], dtype=torch.float64, device=dev, requires_grad=True)
    Xo, Uo, sto = layer(x0, xr, ur, obstacles=ob, geometry=g2)
    assert s.geometry() == (7.3, 12.0, 0.3, 2.9, 3.1)
    s.set_geometry(L1=7.05)
    with pytest.raises(RuntimeError, match="geometry changed"):
        ((Xo * gX).sum() + (Uo * gU).sum()).backward()
