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

import obca_vjp_harness as hx
import obca_vjp_reference as orf

pytestmark = pytest.mark.gpu

GOT = hx.got_map(3)


@functools.lru_cache(maxsize=None)
def batch_a():
    """obca_vjp_harness.solved_a and its plain adjoint."""
    case, s, inputs, (X, U, st, I), (gXb, gUb) = hx.solved_a()
    return case, s, inputs, (X, U, st, I), (gXb, gUb), s.vjp(I, st, gXb, gUb)


@functools.lru_cache(maxsize=None)
def batch_b():
    case, s, (X, U, st, I), (gX, gU) = hx.solved_b()
    return case, s, (X, U, st, I), (gX, gU), s.vjp(I, st, gX[None], gU[None])


def _check_against_dense(P, I, gX, gU, r, b, label, sparse=False):
    hx.check_against_dense(orf, orf.dense_obca_vjp, orf.model_obca_vjp, orf.group_max, orf.KEYS, (P, I, gX, gU),
                           hx.row(r, b, GOT), r.vjp_status[b], label, sparse, word="largest")


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
    err = orf.group_err(hx.row(r, 0, GOT), fd)
    print("gpu vs central differences of the oracle", err)
    for k in orf.KEYS:
        assert err[k] <= 1e-5, (k, err[k])


def test_full_size_windows():
    """B = 2 at the drivers' shape N = 50, M = 11 (1122 blocks: 70 full rounds and a tail of 2): window 0 (open road)
    and window 10 (obstacle rows active) of the golden MPC+OBCA windows, both against the sparse un-condensed solve
    (SuperLU, refined on an extended-precision residual) by the module's rule."""
    s, P, st, I, (gX, gU), _, _ = hx.golden_windows([0, 10])
    r = s.vjp(I, st, np.tile(gX, (2, 1, 1)), np.tile(gU, (2, 1, 1)))
    assert np.all(r.vjp_status == 0), r.vjp_status
    _check_against_dense(P, I[0], gX, gU, r, 0, "window 0", sparse=True)
    assert np.abs(orf.unpack(I[1], 50, 11)["yd"][..., 0]).max() > 1.0
    _check_against_dense(P, I[1], gX, gU, r, 1, "window 10", sparse=True)


_device_call = hx.device_call


def test_determinism_tiling_and_host_entry():
    """300 tiles of the B = 4 batch return the B = 4 results bitwise, two launches agree bitwise, and the host entry is
    the device entry."""
    _, s, _, (X, U, st, I), (gXb, gUb), r = batch_a()
    d4 = _device_call(s, 4, I, st, gXb, gUb)
    for k, ref in (("g_x0", r.g_x0), ("g_xref", r.g_xref), ("g_uref", r.g_uref), ("vjp_status", r.vjp_status)):
        assert np.array_equal(d4[k], ref), k
    T = 300
    hx.check_tiling(lambda *a: _device_call(s, 4 * T, *a), d4, T, I, st, gXb, gUb)


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
