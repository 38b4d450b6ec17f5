"""LQR terminal score on the GPU -- python-files/LQR_cost.py:7-41, batched.

lqr_riccati(params, dynamics, Q, R, x_goal, u_goal) -> P          LQR_cost.py:7-34
lqr_distance(x_current, x_goal, params, dynamics, Q, R, u_goal)   LQR_cost.py:37-41
lqr_scores(x_cur, x_goal, params, Q, R) -> (scores, P, doublings) batched, device tensors or arrays
lqr_scores_vjp(x_cur, x_goal, params, R, P, grad_score, grad_P)   its vector-Jacobian product, device tensors

The DARE is solved per instance by the doubling algorithm in csrc/tt_lqr.hip (the reference calls
scipy.linalg.solve_discrete_are; tests/test_gpu_lqr.py compares the two).  The adjoint (csrc/tt_lqr_vjp.hip) solves
one discrete Lyapunov equation per instance at the forward's P; ttmpc.diff.DifferentiableLqrScore is the autograd
layer over the pair.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._lib import TTLqrVjpOut, lib
from .simulation import _check, _ptr, _stream, plant


def lqr_scores(x_cur, x_goal, params, Q, R, u_goal=None, stream=None):
    """Batched lqr_distance: x_cur, x_goal (B,6) -> score (B,), P (B,6,6), doublings (B,) as torch tensors
    on the GPU (inputs may be numpy or device tensors)."""
    dev = x_goal.device if torch.is_tensor(x_goal) and x_goal.is_cuda else torch.device("cuda", torch.cuda.current_device())
    t = lambda a: (a if torch.is_tensor(a) else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
                   ).to(dev, torch.float64).reshape(-1, 6).contiguous()
    xc, xg = t(x_cur), t(x_goal)
    B = xg.shape[0]
    P = torch.empty((B, 6, 6), dtype=torch.float64, device=dev)
    score = torch.empty(B, dtype=torch.float64, device=dev)
    it = torch.empty(B, dtype=torch.int32, device=dev)
    q = np.ascontiguousarray(np.asarray(Q, dtype=np.float64).reshape(36))
    r = np.ascontiguousarray(np.asarray(R, dtype=np.float64).reshape(4))
    dp = C.POINTER(C.c_double)
    p = plant(params)
    _check(lib().tt_lqr_score_device(B, C.byref(p), q.ctypes.data_as(dp), r.ctypes.data_as(dp), xc.data_ptr(),
                                     xg.data_ptr(), None, P.data_ptr(), score.data_ptr(), it.data_ptr(),
                                     _stream(stream, dev)), "tt_lqr_score_device")
    return score, P, it


def _dev64(name, t, shape, dev=None):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float64:
        raise TypeError(f"{name} must be a float64 CUDA tensor, got "
                        + (f"{t.dtype} on {t.device}" if torch.is_tensor(t) else type(t).__name__))
    if tuple(t.shape) != shape:
        raise ValueError(f"{name} must have shape {shape}, got {tuple(t.shape)}")
    if dev is not None and t.device != dev:
        raise ValueError(f"{name} is on {t.device}, x_cur on {dev}")
    return t.detach().contiguous()


def lqr_scores_vjp(x_cur, x_goal, params, R, P, grad_score=None, grad_P=None, fwd_iters=None, stream=None):
    """The vector-Jacobian product of ``lqr_scores`` (tt_lqr_score_vjp_device, csrc/tt_lqr_vjp.hip) at its P.

    x_cur, x_goal (B,6), P (B,6,6) as ``lqr_scores`` took and returned them, grad_score (B,) = dL/dscore and grad_P
    (B,6,6) = dL/dP (either may be None for zeros, not both): float64 CUDA tensors on one device.  fwd_iters (B,) int32
    is the forward's ``doublings`` (None: every instance is differentiated; an instance with a negative entry is
    skipped).  R is a host 2x2 (array or CPU tensor; a CUDA tensor is copied to the host, which synchronises).
    Returns a dict of device tensors: g_x_cur, g_x_goal (B,6), g_Q (B,6,6), g_R (B,2,2), per instance (sum g_Q and g_R
    over B for a Q and R shared by the batch; both are symmetric: the gradients for symmetric Q and R), vjp_status (B,)
    int32 (0 ok, 1 undefined, 2 skipped; the gradients of such an instance are zeros) and doublings (B,) int32, the
    Lyapunov doublings run.  Asynchronous on ``stream`` (default: the current stream of the inputs' device)."""
    if not torch.is_tensor(x_cur) or x_cur.dim() != 2:
        raise ValueError("x_cur must be a (B,6) tensor")
    if grad_score is None and grad_P is None:
        raise ValueError("give grad_score or grad_P")
    B, dev = x_cur.shape[0], x_cur.device
    xc = _dev64("x_cur", x_cur, (B, 6))
    xg = _dev64("x_goal", x_goal, (B, 6), dev)
    Pm = _dev64("P", P, (B, 6, 6), dev)
    gs = None if grad_score is None else _dev64("grad_score", grad_score, (B,), dev)
    gP = None if grad_P is None else _dev64("grad_P", grad_P, (B, 6, 6), dev)
    if fwd_iters is not None:
        if not torch.is_tensor(fwd_iters) or fwd_iters.dtype != torch.int32 or fwd_iters.device != dev:
            raise TypeError("fwd_iters must be an int32 tensor on the device of x_cur")
        if tuple(fwd_iters.shape) != (B,):
            raise ValueError(f"fwd_iters must have shape {(B,)}, got {tuple(fwd_iters.shape)}")
        fwd_iters = fwd_iters.contiguous()
    r = np.ascontiguousarray(np.asarray(R.detach().cpu() if torch.is_tensor(R) else R, dtype=np.float64))
    if r.size != 4:
        raise ValueError(f"R must be 2x2, got shape {r.shape}")
    r = r.reshape(4)
    new = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)  # noqa: E731
    out = {"g_x_cur": new(B, 6), "g_x_goal": new(B, 6), "g_Q": new(B, 6, 6), "g_R": new(B, 2, 2),
           "vjp_status": torch.empty(B, dtype=torch.int32, device=dev),
           "doublings": torch.empty(B, dtype=torch.int32, device=dev)}
    o = TTLqrVjpOut(*[out[k].data_ptr() or None for k in ("g_x_cur", "g_x_goal", "g_Q", "g_R", "vjp_status",
                                                         "doublings")])
    p = plant(params)
    _check(lib().tt_lqr_score_vjp_device(B, C.byref(p), r.ctypes.data_as(C.POINTER(C.c_double)), xc.data_ptr(),
                                         xg.data_ptr(), Pm.data_ptr(), _ptr(fwd_iters), _ptr(gs), _ptr(gP), C.byref(o),
                                         _stream(stream, dev)), "tt_lqr_score_vjp_device")
    return out


def lqr_riccati(params, dynamics, Q, R, x_goal, u_goal):
    """LQR_cost.py:7-34 (dynamics is accepted for signature parity; the model is the built-in one)."""
    _, P, _ = lqr_scores(np.asarray(x_goal, dtype=np.float64), np.asarray(x_goal, dtype=np.float64), params, Q, R)
    return P.cpu().numpy()[0]


def lqr_distance(x_current, x_goal, params, dynamics, Q, R, u_goal):
    """LQR_cost.py:37-41."""
    s, _, _ = lqr_scores(np.asarray(x_current, dtype=np.float64), np.asarray(x_goal, dtype=np.float64), params, Q, R)
    return float(s.cpu()[0])
