"""Differentiable tracking solve and differentiable closed loop for PyTorch: autograd nodes over the batched MPC solve.

``DifferentiableTracking(solver)`` wraps a ``BatchSolver`` of a tracking variant.  Forward is one
``solve_ex_device`` (the solve with its multipliers), backward one ``vjp_device`` (track_vjp_kernel): for a scalar loss
L(X, U) it returns dL/d(x0, xref, uref, wq_wr) as sIPOPT defines the sensitivity of the solution, from one Riccati pass
at the returned primal-dual point (include/ttmpc.h, "Reverse mode").  First order: the active set is taken as fixed.
Both run on ``torch.cuda.current_stream()`` without any host synchronisation.

``DifferentiableObcaTracking(solver)`` is the same layer over an ``ObcaSolver`` of TT_VARIANT_TRACK_OBCA: forward one
``solve_device(..., iterate=ptr)``, backward one ``ObcaSolver.vjp_device`` (obca_vjp_kernel), differentiable with
respect to x0, xref and uref.

``DifferentiableClosedLoop(loop)`` wraps a ``ttmpc.simulation.ClosedLoop``: forward is ``run_tape`` (K closed-loop steps
with every solve taped on the device), backward is ``ClosedLoop.backward`` (the plant, policy and window adjoints around
one ``vjp_device`` per step).  For a scalar loss on the visited states S and the applied controls Ua it returns
dL/d(x_init, wq_wr, plan_x, plan_u, noise).

Both layers also take the model geometry as a tensor: ``model`` = (L1, L2, M) of the controller's model (applied to the
handle with ``set_model``) and, for the closed loop, ``plant_model`` = the plant's.  Their gradients come from the model
instantiations of the adjoint kernels (include/ttmpc.h, tt_track_vjp_model_device, tt_policy_plant_vjp_model_device),
summed over the batch.

Both layers also take the solver's box as a tensor: ``bounds`` = (xlb 6, ulb 2, xub 6, uub 2), applied to the handle with
``set_bounds``; its gradient comes from the bounds instantiations of the adjoint kernel (tt_track_vjp_bounds_device),
summed over the batch.  It is where the loss on a saturated variable goes.

A closed loop built with a ``ttmpc.simulation.FuzzyRule`` takes the rule's seven parameters as a tensor too
(``fuzzy_rule=``), and ``fuzzy_weights(x, xref, theta)`` is the rule alone as an autograd
node (tt_fuzzy_weights_rule_device / tt_fuzzy_weights_vjp_device) whose output feeds ``DifferentiableTracking``'s wq_wr.

``DifferentiableLqrScore(params)`` is the LQR terminal score the drivers report at the end of a run
(``ttmpc.lqr.lqr_scores``): forward one lqr_kernel launch, backward one lqr_vjp_kernel launch
(``ttmpc.lqr.lqr_scores_vjp``), differentiable with respect to x_cur, x_goal, Q and R.  Fed with the last state of a
``DifferentiableClosedLoop`` and the plan's last row it closes the chain from the reference's own metric back to the
weights, the plan, x_init and the noise.
"""
from __future__ import annotations

import numpy as np
import torch

from . import simulation as sim

__all__ = ["TrackingSolveFunction", "TrackingSolveModelFunction", "DifferentiableTracking", "ObcaTrackingSolveFunction",
           "DifferentiableObcaTracking", "ClosedLoopFunction",
           "ClosedLoopModelFunction", "ClosedLoopRuleFunction", "DifferentiableClosedLoop", "FuzzyWeightsFunction",
           "fuzzy_weights", "LqrScoreFunction", "DifferentiableLqrScore"]


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def _check(name, t, shape):
    sim.check_tensor(name, t, shape)
    return t.detach().contiguous()


_GEOMETRY = "(L1, L2, M)"
_OBCA_GEOMETRY = "(L1, L2, M, W1, W2)"
_THETA = "(psi_full, gain_hitch, gain_steer, gain_rate, rev_hitch, rev_steer, rev_rate)"


def _host_vector(name, t, what):
    """A geometry (_GEOMETRY, _OBCA_GEOMETRY) or rule-parameter (_THETA) tensor as host floats: float64, shape (3,),
    (5,) or (7,), on the CPU or on a device (one host read)."""
    n = what.count(",") + 1
    if not (torch.is_tensor(t) and t.dtype == torch.float64 and tuple(t.shape) == (n,)):
        raise TypeError(f"{name} must be a float64 tensor of shape ({n},) = {what}")
    return tuple(float(v) for v in t.detach().cpu().tolist())


def _host_bounds(t):
    """A bounds tensor, float64 (16,) = (xlb 6, ulb 2, xub 6, uub 2) on the CPU or on a device (one host read; +-inf
    allowed), as the (xlb, xub, ulb, uub) of ``BatchSolver.set_bounds``."""
    if not (torch.is_tensor(t) and t.dtype == torch.float64 and tuple(t.shape) == (16,)):
        raise TypeError("bounds must be a float64 tensor of shape (16,) = (xlb 6, ulb 2, xub 6, uub 2)")
    v = t.detach().cpu().numpy()
    return v[0:6].copy(), v[8:14].copy(), v[6:8].copy(), v[14:16].copy()


def _same_bounds(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _batch_sum(g, device):
    """The per-instance gradients (B,n) summed over the batch, on the input tensor's device."""
    return g.sum(dim=0).to(device)


class TrackingSolveFunction(torch.autograd.Function):
    """``X, U, status = TrackingSolveFunction.apply(solver, x0, xref, uref, wq_wr, z_guess[, model[, bounds]])``.

    x0 (B,6), xref (B,N+1,6), uref (B,N,2), wq_wr (B,8) or None, z_guess (B,8N+6) or None: float64 CUDA tensors on the
    solver's device.  X (B,N+1,6) and U (B,N,2) are differentiable with respect to x0, xref, uref and wq_wr; status
    (B,) int32 is not, and z_guess gets no gradient (it does not move a converged solution).  An instance whose solve
    status is above TT_ACCEPTABLE, or whose adjoint is undefined, contributes a zero gradient.

    model, if given, makes the solver's geometry an input: float64 (3,) = (L1, L2, M), on the CPU or on a device (then
    the forward reads it to the host once).  The forward applies it with ``solver.set_model`` when it differs from the
    handle's values, and it stays applied; the backward runs the adjoint kernel's model instantiation and returns the
    per-instance gradients summed over B on the tensor's device.  It raises if the handle's geometry was changed
    between the forward and the backward.  Left out or None: the geometry as it is, no gradient for it.

    bounds, if given, makes the solver's box an input in the same way: float64 (16,) = (xlb 6, ulb 2, xub 6, uub 2), the
    order of g_bounds, on the CPU or on a device; +-inf is a free bound.  The forward applies it with
    ``solver.set_bounds`` when it differs from the handle's box, and it stays applied; the backward runs the adjoint
    kernel's bounds instantiation and returns the per-instance gradients summed over B on the tensor's device.  It
    raises if the handle's box was changed between the forward and the backward."""

    @staticmethod
    def forward(ctx, solver, x0, xref, uref, wq_wr, z_guess, model=None, bounds=None):
        ctx.box = None
        if bounds is not None:
            ctx.box, ctx.box_like = _host_bounds(bounds), bounds.device
            if not _same_bounds(ctx.box, solver.get_bounds()):
                solver.set_bounds(*ctx.box)
        ctx.geometry = None
        if model is not None:
            ctx.geometry, ctx.like = _host_vector("model", model, _GEOMETRY), model.device
            if ctx.geometry != solver.model():
                solver.set_model(*ctx.geometry)
        N, B = solver.N, x0.shape[0]
        x0 = _check("x0", x0, (B, 6))
        xref = _check("xref", xref, (B, N + 1, 6))
        uref = _check("uref", uref, (B, N, 2))
        wq_wr = None if wq_wr is None else _check("wq_wr", wq_wr, (B, 8))
        z_guess = None if z_guess is None else _check("z_guess", z_guess, (B, 8 * N + 6))
        dev = x0.device
        X = torch.empty((B, N + 1, 6), dtype=torch.float64, device=dev)
        U = torch.empty((B, N, 2), dtype=torch.float64, device=dev)
        dual = torch.empty((B, N + 1, 22), dtype=torch.float64, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        solver.solve_ex_device(B, x0.data_ptr(), xref.data_ptr(), uref.data_ptr(), X.data_ptr(), U.data_ptr(),
                               status.data_ptr(), wq_wr=_ptr(wq_wr), z_guess=_ptr(z_guess), dual=dual.data_ptr(),
                               stream=torch.cuda.current_stream(dev).cuda_stream)
        ctx.solver = solver
        ctx.has_w = wq_wr is not None
        ctx.save_for_backward(X, U, dual, status, xref, uref, *(() if wq_wr is None else (wq_wr,)))
        ctx.mark_non_differentiable(status)
        return X, U, status

    @staticmethod
    def backward(ctx, grad_X, grad_U, _grad_status):
        # (solver, x0, xref, uref, wq_wr, z_guess[, model[, bounds]]): one gradient per input given
        need = ctx.needs_input_grad
        if ctx.geometry is not None and ctx.geometry != ctx.solver.model():
            raise RuntimeError(f"the solver's geometry changed since the forward: {ctx.geometry} -> "
                               f"{ctx.solver.model()}")
        if ctx.box is not None and not _same_bounds(ctx.box, ctx.solver.get_bounds()):
            raise RuntimeError("the solver's bounds changed since the forward")
        if grad_X is None and grad_U is None:
            return (None,) * len(need)
        X, U, dual, status, xref, uref = ctx.saved_tensors[:6]
        wq_wr = ctx.saved_tensors[6] if ctx.has_w else None
        B, N, dev = X.shape[0], ctx.solver.N, X.device
        gX = None if grad_X is None else grad_X.to(torch.float64).contiguous()
        gU = None if grad_U is None else grad_U.to(torch.float64).contiguous()
        new = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)  # noqa: E731
        g_x0 = new(B, 6) if need[1] else None
        g_xref = new(B, N + 1, 6) if need[2] else None
        g_uref = new(B, N, 2) if need[3] else None
        g_w = new(B, 8) if need[4] else None
        g_m = new(B, 3) if len(need) > 6 and need[6] else None
        g_b = new(B, 16) if len(need) > 7 and need[7] else None
        ctx.solver.vjp_device(B, X.data_ptr(), U.data_ptr(), dual.data_ptr(), xref.data_ptr(), uref.data_ptr(),
                              status.data_ptr(), grad_x=_ptr(gX), grad_u=_ptr(gU), g_x0=_ptr(g_x0), g_xref=_ptr(g_xref),
                              g_uref=_ptr(g_uref), g_wq_wr=_ptr(g_w), wq_wr=_ptr(wq_wr),
                              stream=torch.cuda.current_stream(dev).cuda_stream, g_model=_ptr(g_m),
                              g_bounds=_ptr(g_b))
        return (None, g_x0, g_xref, g_uref, g_w, None, None if g_m is None else _batch_sum(g_m, ctx.like),
                None if g_b is None else _batch_sum(g_b, ctx.box_like))[:len(need)]


TrackingSolveModelFunction = TrackingSolveFunction


class DifferentiableTracking:
    """``X, U, status = layer(x0, xref, uref, wq_wr=None, z_guess=None, model=None, bounds=None)`` with float64 CUDA
    tensors.

    A thin callable over ``TrackingSolveFunction`` for one ``BatchSolver`` (TT_VARIANT_TRACK, _NMPC or _FUZZY; the
    fuzzy variant needs wq_wr).  One handle serialises its solves on one stream: the forward uses workspaces of the
    handle, so every forward of one layer must be enqueued on the same stream (and a second layer wants its own
    solver).  The backward uses no buffer of the handle and may run on any stream that is ordered behind the forward,
    as autograd's stream bookkeeping arranges.  Look at ``status`` (and at ``solver.vjp_device(..., vjp_status=...)``
    when in doubt) to see which instances gave a gradient: failed ones give zeros.  With ``model`` (a float64 (3,)
    tensor (L1, L2, M), CPU or device) the solver's geometry is an input too, and with ``bounds`` (a float64 (16,)
    tensor (xlb 6, ulb 2, xub 6, uub 2), CPU or device) its box: a loss on a saturated variable, which has no gradient
    in the other inputs, arrives at the bound it sits on."""

    def __init__(self, solver):
        self.solver = solver

    def __call__(self, x0, xref, uref, wq_wr=None, z_guess=None, model=None, bounds=None):
        """model: float64 (3,) tensor (L1, L2, M) or None (the solver's geometry as it is, no gradient for it).
        bounds: float64 (16,) tensor (xlb 6, ulb 2, xub 6, uub 2) or None (the solver's box as it is, no gradient)."""
        if bounds is None:   # (the call form of before)
            return TrackingSolveFunction.apply(self.solver, x0, xref, uref, wq_wr, z_guess, model)
        return TrackingSolveFunction.apply(self.solver, x0, xref, uref, wq_wr, z_guess, model, bounds)


class ObcaTrackingSolveFunction(torch.autograd.Function):
    """``X, U, status = ObcaTrackingSolveFunction.apply(solver, x0, xref, uref)`` for an ``ObcaSolver`` of
    TT_VARIANT_TRACK_OBCA: x0 (B,6), xref (B,N+1,6), uref (B,N,2) float64 CUDA tensors on the solver's device.  X and U
    are differentiable with respect to all three (tt_obca_vjp_device: first order, the active set fixed); an instance
    whose solve status is above TT_ACCEPTABLE, or whose adjoint is undefined, contributes a zero gradient.

    obstacles (float64 (M,4) of (cx, cy, w, h)) and d_min (float64 ()), if given, make the handle's scene an input, on
    the CPU or on a device (then the forward reads them to the host once).  The forward applies them with
    ``solver.set_scene`` when they differ from the handle's, and they stay applied; the backward then runs the adjoint
    kernel's params instantiation (tt_obca_vjp_params_device) and returns the per-instance rows summed over B on each
    tensor's device.  It raises if the handle's scene was changed between the forward and the backward.

    obstacles of shape (B,M,4) and / or d_min of shape (B,) select the per-instance path instead: every instance solves
    against its own row (tt_obca_solve_batch_scenes_device; one left None is the handle's for every instance), the
    handle's scene is left alone, and the backward (tt_obca_vjp_scenes_device) returns the rows as they are, (B,M,4)
    and (B,), each instance's gradient in its own scene.  The two forms do not mix in one call.

    geometry (float64 (5,) = (L1, L2, M, W1, W2), CPU or device), if given, makes the handle's geometry an input, the
    pattern of ``TrackingSolveFunction``'s ``model``: the forward applies it with ``solver.set_geometry`` when it
    differs from the handle's, and it stays applied; the backward runs the adjoint kernel's geometry instantiation
    (tt_obca_vjp_geometry_device) and returns the per-instance rows summed over B on the tensor's device.  It raises if
    the handle's geometry was changed between the forward and the backward."""

    @staticmethod
    def forward(ctx, solver, x0, xref, uref, obstacles=None, d_min=None, geometry=None):
        ctx.geom = None
        if geometry is not None:
            vals = _host_vector("geometry", geometry, _OBCA_GEOMETRY)
            if vals != solver.geometry():
                solver.set_geometry(*vals)
            ctx.geom, ctx.geom_like = solver.geometry(), geometry.device
        ctx.scene = None
        ctx.like = (None, None)
        ctx.rows = (torch.is_tensor(obstacles) and obstacles.dim() == 3) or (torch.is_tensor(d_min) and d_min.dim() == 1)
        if ctx.rows:
            B, dev = x0.shape[0], x0.device
            for name, t, shape in (("obstacles", obstacles, (B, solver.M, 4)), ("d_min", d_min, (B,))):
                if t is not None and not (torch.is_tensor(t) and t.dtype == torch.float64 and tuple(t.shape) == shape):
                    raise TypeError(f"per-instance {name} must be a float64 tensor of shape {shape}")
            ctx.scene = solver.scene()  # (a member left None is the handle's)
            ctx.like = (None if obstacles is None else obstacles.device, None if d_min is None else d_min.device)
            scenes = tuple(None if t is None else t.detach().to(dev).contiguous() for t in (obstacles, d_min))
        elif obstacles is not None or d_min is not None:
            ob, dm = solver.scene()
            for name, t, shape in (("obstacles", obstacles, (solver.M, 4)), ("d_min", d_min, ())):
                if t is not None and not (torch.is_tensor(t) and t.dtype == torch.float64 and tuple(t.shape) == shape):
                    raise TypeError(f"{name} must be a float64 tensor of shape {shape}")
            new_ob = None if obstacles is None else obstacles.detach().cpu().numpy()
            new_dm = None if d_min is None else float(d_min.detach().cpu())
            if (new_ob is not None and not (new_ob == ob).all()) or (new_dm is not None and new_dm != dm):
                solver.set_scene(new_ob, new_dm)
            ctx.scene = solver.scene()
            ctx.like = (None if obstacles is None else obstacles.device, None if d_min is None else d_min.device)
        N, B = solver.N, x0.shape[0]
        x0 = _check("x0", x0, (B, 6))
        xref = _check("xref", xref, (B, N + 1, 6))
        uref = _check("uref", uref, (B, N, 2))
        dev = x0.device
        X = torch.empty((B, N + 1, 6), dtype=torch.float64, device=dev)
        U = torch.empty((B, N, 2), dtype=torch.float64, device=dev)
        iterate = torch.empty((B, solver.iterate_len()), dtype=torch.float64, device=dev)
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        if ctx.rows:
            solver.solve_device(B, x0.data_ptr(), 0, xref.data_ptr(), uref.data_ptr(), 0, X.data_ptr(), U.data_ptr(), 0,
                                status.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream,
                                iterate=iterate.data_ptr(), obstacles=_ptr(scenes[0]), d_min=_ptr(scenes[1]))
            ctx.scenes = scenes
        else:
            solver.solve_device(B, x0.data_ptr(), 0, xref.data_ptr(), uref.data_ptr(), 0, X.data_ptr(), U.data_ptr(), 0,
                                status.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream,
                                iterate=iterate.data_ptr())
        ctx.solver = solver
        ctx.save_for_backward(iterate, status)
        ctx.mark_non_differentiable(status)
        return X, U, status

    @staticmethod
    def backward(ctx, grad_X, grad_U, _grad_status):
        need = ctx.needs_input_grad  # (solver, x0, xref, uref[, obstacles, d_min[, geometry]])
        if ctx.geom is not None and ctx.solver.geometry() != ctx.geom:
            raise RuntimeError("the solver's geometry changed since the forward")
        if ctx.scene is not None:
            ob, dm = ctx.solver.scene()
            if not (ob == ctx.scene[0]).all() or dm != ctx.scene[1]:
                raise RuntimeError("the solver's scene changed since the forward")
        if grad_X is None and grad_U is None:
            return (None,) * len(need)
        iterate, status = ctx.saved_tensors
        B, N, dev = status.shape[0], ctx.solver.N, status.device
        gX = None if grad_X is None else grad_X.to(torch.float64).contiguous()
        gU = None if grad_U is None else grad_U.to(torch.float64).contiguous()
        new = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)  # noqa: E731
        g_x0 = new(B, 6) if need[1] else None
        g_xref = new(B, N + 1, 6) if need[2] else None
        g_uref = new(B, N, 2) if need[3] else None
        if ctx.scene is not None or ctx.geom is not None:
            g_ob = new(B, ctx.solver.M, 4) if len(need) > 4 and need[4] else None
            g_dm = new(B) if len(need) > 5 and need[5] else None
            g_ge = new(B, 5) if len(need) > 6 and need[6] else None
            work = torch.empty((B * ctx.solver.vjp_params_work_bytes() // 8,), dtype=torch.float64, device=dev)
            rows = dict(obstacles=_ptr(ctx.scenes[0]), d_min=_ptr(ctx.scenes[1])) if ctx.rows else {}
            ctx.solver.vjp_device(B, iterate.data_ptr(), status.data_ptr(), grad_x=_ptr(gX), grad_u=_ptr(gU),
                                  g_x0=_ptr(g_x0), g_xref=_ptr(g_xref), g_uref=_ptr(g_uref), g_obstacles=_ptr(g_ob),
                                  g_dmin=_ptr(g_dm), work=work.data_ptr(), g_geometry=_ptr(g_ge),
                                  stream=torch.cuda.current_stream(dev).cuda_stream, **rows)
            g_ge = None if g_ge is None else _batch_sum(g_ge, ctx.geom_like)  # (one geometry for the batch)
            if ctx.rows:  # each instance's gradient in its own scene: nothing to sum
                return (None, g_x0, g_xref, g_uref, None if g_ob is None else g_ob.to(ctx.like[0]),
                        None if g_dm is None else g_dm.to(ctx.like[1]), g_ge)[:len(need)]
            return (None, g_x0, g_xref, g_uref, None if g_ob is None else _batch_sum(g_ob, ctx.like[0]),
                    None if g_dm is None else _batch_sum(g_dm, ctx.like[1]), g_ge)[:len(need)]
        ctx.solver.vjp_device(B, iterate.data_ptr(), status.data_ptr(), grad_x=_ptr(gX), grad_u=_ptr(gU),
                              g_x0=_ptr(g_x0), g_xref=_ptr(g_xref), g_uref=_ptr(g_uref),
                              stream=torch.cuda.current_stream(dev).cuda_stream)
        return (None, g_x0, g_xref, g_uref, None, None, None)[:len(need)]


class DifferentiableObcaTracking:
    """``X, U, status = layer(x0, xref, uref, obstacles=None, d_min=None, geometry=None)`` with float64 CUDA tensors: a thin callable
    over ``ObcaTrackingSolveFunction`` for one ``ObcaSolver`` of TT_VARIANT_TRACK_OBCA.  The forward uses the handle's
    solver workspace (one stream per handle); the backward uses no buffer of the handle.  Failed instances give zeros.
    With ``obstacles`` (float64 (M,4)) and / or ``d_min`` (float64 ()), CPU or device, the handle's scene is an input
    too: ``obstacles.grad`` and ``d_min.grad`` are the batch sums of tt_obca_vjp_params_device's rows.  With
    ``obstacles`` of shape (B,M,4) and / or ``d_min`` of shape (B,) every instance has its own scene and ``.grad`` has
    those shapes: row b is instance b's gradient in its own scene (tt_obca_vjp_scenes_device).  Q and R are not
    inputs (there is no setter for them); ``ObcaSolver.vjp(..., params=True)`` returns their gradients.  With
    ``geometry`` (float64 (5,) = (L1, L2, M, W1, W2), CPU or device) the handle's geometry is an input:
    ``geometry.grad`` is the batch sum of tt_obca_vjp_geometry_device's rows."""

    def __init__(self, solver):
        from ._lib import TT_VARIANT_TRACK_OBCA
        if getattr(solver, "variant", None) != TT_VARIANT_TRACK_OBCA or not hasattr(solver, "iterate_len"):
            raise TypeError("DifferentiableObcaTracking needs an ObcaSolver of TT_VARIANT_TRACK_OBCA")
        self.solver = solver

    def __call__(self, x0, xref, uref, obstacles=None, d_min=None, geometry=None):
        return ObcaTrackingSolveFunction.apply(self.solver, x0, xref, uref, obstacles, d_min, geometry)


class ClosedLoopFunction(torch.autograd.Function):
    """``S, Ua, status = ClosedLoopFunction.apply(loop, T_sim, x_init, wq_wr, plan_x, plan_u, noise[, model,
    plant_model[, fuzzy_rule[, bounds]]])``.

    x_init (B,6), wq_wr (B,8) or None, plan_x (P,Np+1,6) and plan_u (P,Np,2) with P = 1 (shared) or B, or None for the
    loop's own plan, noise (K,B,6) or None: float64 CUDA tensors on the loop's device.  S (K+1,B,6) and Ua (K,B,2) are
    differentiable with respect to all five; status (K,B) int32 is not.

    model, plant_model: the two geometries as inputs, each a float64 (3,) tensor (L1, L2, M) on the CPU or on a device
    (one host read each), or None.  model is the geometry the controller believes, plant_model the plant's; the forward
    applies them with ``loop.set_model`` when they differ from the current values, and they stay applied.  The backward
    returns their gradients summed over B on each tensor's device; the same tensor given as both receives the sum of
    the two, the gradient for a geometry controller and plant share.

    fuzzy_rule, for a loop built with a ``FuzzyRule``: the rule's parameters as an input, a float64 (7,) tensor theta on
    the CPU or on a device (one host read), or None.  The forward applies it with ``loop.set_fuzzy_rule`` (the rule's
    settings w_min, w_max, v_rev stay the loop's) when it differs from the current values, and it stays applied; the
    backward returns dL/dtheta summed over B on the tensor's device.  wq_wr must then be None: the weights come from
    the rule.

    bounds: the solver's box as an input, a float64 (16,) tensor (xlb 6, ulb 2, xub 6, uub 2) on the CPU or on a device
    (one host read; +-inf is a free bound), or None.  The forward applies it with ``loop.set_bounds`` when it differs
    from the handle's box, and it stays applied; the backward returns dL/dbounds summed over B on the tensor's device
    (the bounds enter the loop only through the solves: the plant does not clip)."""

    EXTRA = ("g_model_solver", "g_model_plant", "g_fuzzy_rule", "g_bounds")   # ClosedLoop.backward's keys of inputs 7 .. 10

    @staticmethod
    def forward(ctx, loop, T_sim, x_init, wq_wr, plan_x, plan_u, noise, model=None, plant_model=None, fuzzy_rule=None,
                bounds=None):
        if bounds is not None:
            box = _host_bounds(bounds)
            if not _same_bounds(box, loop.solver.get_bounds()):
                loop.set_bounds(*box)
        if fuzzy_rule is not None:
            if loop.rule is None:
                raise ValueError("fuzzy_rule= needs a loop built with ClosedLoop(..., fuzzy_rule=FuzzyRule(...))")
            vals = _host_vector("fuzzy_rule", fuzzy_rule, _THETA)
            if vals != loop.rule.theta():
                loop.set_fuzzy_rule(loop.rule.with_theta(vals))
        vs = None if model is None else _host_vector("model", model, _GEOMETRY)
        vp = None if plant_model is None else _host_vector("plant_model", plant_model, _GEOMETRY)
        loop.set_model(solver=None if vs is None or vs == loop.solver.model() else vs,
                       plant=None if vp is None or vp == loop.plant_model() else vp)
        ctx.like = tuple(None if t is None else t.device for t in (model, plant_model, fuzzy_rule, bounds))
        if (plan_x is None) != (plan_u is None):
            raise ValueError("give plan_x and plan_u together")
        B = x_init.shape[0]
        x_init = _check("x_init", x_init, (B, 6))
        if plan_x is not None:
            Np = plan_u.shape[-2]
            P = plan_x.shape[0]
            if plan_x.dim() != 3 or P not in (1, B):
                raise ValueError("plan_x must be (1, Np+1, 6) for a shared plan or (B, Np+1, 6)")
            loop.plan_x, loop.plan_u = _check("plan_x", plan_x, (P, Np + 1, 6)), _check("plan_u", plan_u, (P, Np, 2))
        out = loop.run_tape(x_init, T_sim, noise=noise, wq_wr=wq_wr)
        tape = out["tape"]
        ctx.loop, ctx.tape = loop, tape
        status = tape.status.clone()   # (copies: the node keeps the tape, the outputs must not keep the node)
        ctx.mark_non_differentiable(status)
        return tape.S.clone(), tape.Ua.clone(), status

    @staticmethod
    def backward(ctx, grad_S, grad_Ua, _grad_status):
        # (loop, T_sim, x_init, wq_wr, plan_x, plan_u, noise[, model, plant_model[, fuzzy_rule[, bounds]]]): one
        # gradient per input given
        need = ctx.needs_input_grad + (False,) * (11 - len(ctx.needs_input_grad))
        tape = ctx.tape
        if grad_S is None and grad_Ua is None:
            return (None,) * len(ctx.needs_input_grad)
        GS = torch.zeros_like(tape.S) if grad_S is None else grad_S.to(torch.float64).contiguous()
        GU = torch.zeros_like(tape.Ua) if grad_Ua is None else grad_Ua.to(torch.float64).contiguous()
        g = ctx.loop.backward(tape, GS, GU, **(dict(model=True) if need[7] or need[8] else {}),
                              **(dict(rule=True) if need[9] else {}), **(dict(bounds=True) if need[10] else {}))
        pick = lambda i, k: g[k] if need[i] else None  # noqa: E731
        extra = [_batch_sum(g[k], ctx.like[i]) if need[7 + i] else None for i, k in enumerate(ClosedLoopFunction.EXTRA)]
        return (None, None, pick(2, "g_x_init"), pick(3, "g_wq_wr"), pick(4, "g_plan_x"), pick(5, "g_plan_u"),
                pick(6, "g_noise"), *extra)[:len(ctx.needs_input_grad)]


ClosedLoopModelFunction = ClosedLoopRuleFunction = ClosedLoopFunction


class FuzzyWeightsFunction(torch.autograd.Function):
    """``wq_wr = FuzzyWeightsFunction.apply(x, xref, theta, rule)``: the fuzzy weight rule alone, for the one-solve
    case.  x (B,6) the measured states, xref (B,N+1,6) the windows: float64 CUDA tensors; theta: float64 (7,), CPU or
    device; rule: a ``FuzzyRule`` whose settings (w_min, w_max, v_rev) are used, or None for the reference's.  wq_wr
    (B,8) is differentiable with respect to x (only the hitch angle x[:, 3] carries a gradient) and theta (summed over
    B, on theta's device); xref only switches and gets none.  Forward tt_fuzzy_weights_rule_device, backward
    tt_fuzzy_weights_vjp_device, both on the current stream."""

    @staticmethod
    def forward(ctx, x, xref, theta, rule):
        B = x.shape[0]
        x = _check("x", x, (B, 6))
        if xref.dim() != 3:
            raise ValueError("xref must be (B, N+1, 6)")
        xref = _check("xref", xref, (B, xref.shape[1], 6))
        ctx.rule = (rule or sim.FuzzyRule()).with_theta(_host_vector("fuzzy_rule", theta, _THETA))
        ctx.like = theta.device
        ctx.save_for_backward(x, xref)
        return sim.fuzzy_weights_rule(x, xref, ctx.rule)

    @staticmethod
    def backward(ctx, grad_w):
        x, xref = ctx.saved_tensors
        g_x, g_rule = sim.fuzzy_weights_vjp(x, xref, grad_w.to(torch.float64).contiguous(), ctx.rule)
        need = ctx.needs_input_grad
        return g_x if need[0] else None, None, _batch_sum(g_rule, ctx.like) if need[2] else None, None


def fuzzy_weights(x, xref, theta, rule=None):
    """``FuzzyWeightsFunction.apply``: the weights (B,8) of a ``DifferentiableTracking`` solve from the measured state,
    the window and the rule parameters theta (7,)."""
    return FuzzyWeightsFunction.apply(x, xref, theta, rule)


class DifferentiableClosedLoop:
    """``S, Ua, status = layer(x_init, T_sim, wq_wr=None, plan_x=None, plan_u=None, noise=None, model=None,
    plant_model=None, fuzzy_rule=None, bounds=None)``.

    A thin callable over ``ClosedLoopFunction`` for one ``ClosedLoop`` whose solver is TT_VARIANT_TRACK or
    TT_VARIANT_NMPC (any of the three failure policies, warm start on or off, measurement or in-plant noise, shared or
    per-instance plan), or any tracking variant with a ``FuzzyRule`` (ClosedLoop(..., fuzzy_rule=...)).  A
    TT_VARIANT_FUZZY solver on the built-in rule raises ValueError, and so does a switch solver unless the loop was
    built with ``switch_adjoint=True`` (then x_init, the plan and the noise get gradients through the MPC+OBCA solves too;
    model, plant_model and fuzzy_rule are not available on such a loop).  A plan given here replaces
    the loop's.  The forward synchronises once at its end, as ``run`` does; the backward does not.  Zero gradient comes
    from: failed solves (whatever the policy then applies), stopped instances, variables sitting on a bound, and the
    warm start (z_guess does not move a converged solution).  With ``model`` and / or ``plant_model`` (float64 (3,)
    tensors (L1, L2, M), CPU or device) the controller's and the plant's geometry are inputs too.  With ``fuzzy_rule``
    (a float64 (7,) tensor theta, CPU or device) the parameters of the loop's fuzzy rule are an input as well.  With
    ``bounds`` (a float64 (16,) tensor (xlb 6, ulb 2, xub 6, uub 2), CPU or device; not on a switch loop) the solver's box
    is an input: the loss on the saturated inputs of every step arrives at the bounds they sit on."""

    def __init__(self, loop):
        loop._check_differentiable()
        self.loop = loop

    def __call__(self, x_init, T_sim, wq_wr=None, plan_x=None, plan_u=None, noise=None, model=None, plant_model=None,
                 fuzzy_rule=None, bounds=None):
        """model, plant_model: float64 (3,) tensors (L1, L2, M) of the controller's and of the plant's geometry, or
        None (as they are, no gradient).  fuzzy_rule: float64 (7,) tensor theta of the loop's ``FuzzyRule``, or None.
        bounds: float64 (16,) tensor (xlb 6, ulb 2, xub 6, uub 2) of the solver's box, or None."""
        if bounds is None:   # (the call form of before)
            return ClosedLoopFunction.apply(self.loop, T_sim, x_init, wq_wr, plan_x, plan_u, noise, model, plant_model,
                                            fuzzy_rule)
        return ClosedLoopFunction.apply(self.loop, T_sim, x_init, wq_wr, plan_x, plan_u, noise, model, plant_model,
                                        fuzzy_rule, bounds)


def _host(name, m, n):
    """Q or R as a host (n,n) float64 array; a device tensor is copied (one synchronisation)."""
    a = np.ascontiguousarray(np.asarray(m.detach().cpu() if torch.is_tensor(m) else m, dtype=np.float64))
    if a.shape != (n, n):
        raise ValueError(f"{name} must have shape {(n, n)}, got {a.shape}")
    return a


class LqrScoreFunction(torch.autograd.Function):
    """``score, P, doublings = LqrScoreFunction.apply(params, x_cur, x_goal, Q, R)``.

    x_cur, x_goal (B,6): float64 CUDA tensors on one device; Q (6,6) and R (2,2): tensors (any device and dtype) or
    arrays, shared by the batch.  score (B,) and P (B,6,6) are differentiable with respect to x_cur, x_goal, Q and R;
    doublings (B,) int32 (the forward's, -1 = the DARE did not converge) is not.  The Q and R gradients are the
    per-instance ones summed over B, symmetric (the gradients for symmetric Q and R).  An instance whose DARE did not
    converge, or whose adjoint is undefined, contributes a zero gradient."""

    @staticmethod
    def forward(ctx, params, x_cur, x_goal, Q, R):
        from . import lqr
        B = x_cur.shape[0]
        xc = _check("x_cur", x_cur, (B, 6))
        xg = _check("x_goal", x_goal, (B, 6))
        if xg.device != xc.device:
            raise ValueError(f"x_goal is on {xg.device}, x_cur on {xc.device}")
        q, r = _host("Q", Q, 6), _host("R", R, 2)
        score, P, it = lqr.lqr_scores(xc, xg, params, q, r)
        ctx.params, ctx.R = params, r
        ctx.like = [(m.device, m.dtype) if torch.is_tensor(m) else None for m in (Q, R)]
        ctx.save_for_backward(xc, xg, P, it)
        ctx.mark_non_differentiable(it)
        ctx.set_materialize_grads(False)
        return score, P, it

    @staticmethod
    def backward(ctx, grad_score, grad_P, _grad_doublings):
        from . import lqr
        need = ctx.needs_input_grad  # (params, x_cur, x_goal, Q, R)
        if grad_score is None and grad_P is None:
            return (None,) * 5
        xc, xg, P, it = ctx.saved_tensors
        gs = None if grad_score is None else grad_score.to(torch.float64).contiguous()
        gP = None if grad_P is None else grad_P.to(torch.float64).contiguous()
        g = lqr.lqr_scores_vjp(xc, xg, ctx.params, ctx.R, P, grad_score=gs, grad_P=gP, fwd_iters=it)
        shared = lambda k, n: g[k].sum(dim=0).to(*ctx.like[n - 3]) if need[n] else None  # noqa: E731
        return (None, g["g_x_cur"] if need[1] else None, g["g_x_goal"] if need[2] else None, shared("g_Q", 3),
                shared("g_R", 4))


class DifferentiableLqrScore:
    """``score, P, doublings = layer(x_cur, x_goal, Q, R)`` for one parameter dict (dt, L1, L2, M; no gradient).

    A thin callable over ``LqrScoreFunction``.  The C ABI takes Q and R from the host: given as device tensors, the
    forward copies them to the host once (one synchronisation; host tensors and arrays cost none); the backward reads
    the copy it kept and does not synchronise.  The Q and R gradients arrive on the device and in the dtype of the Q and
    R tensors given (for a host tensor that move is a synchronisation the caller chose).  With the last
    state of a differentiable closed loop::

        S, Ua, st = DifferentiableClosedLoop(loop)(x_init, T, wq_wr=w, plan_x=px, plan_u=pu)
        score, P, _ = DifferentiableLqrScore(params)(S[-1], px[:, -1].expand(B, 6), Q, R)
        score.sum().backward()        # w.grad, px.grad, pu.grad, x_init.grad: the derivative of the drivers' metric
    """

    def __init__(self, params):
        self.params = params

    def __call__(self, x_cur, x_goal, Q, R):
        return LqrScoreFunction.apply(self.params, x_cur, x_goal, Q, R)
