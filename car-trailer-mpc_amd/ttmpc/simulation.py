"""Batched closed-loop simulation on the GPU -- the receding-horizon loop of python-files/simulation.py
(and simulation_nmpc.py) for B Monte-Carlo instances at once, with every per-step array in HBM.

Reference loop (simulation.py:484-531), per instance, per step t = 0, dt, 2dt, ... <= T_sim:
    k = floor(t / dt)                                   (t accumulated with +=, as the reference does)
    window  = reference window at k with end padding                         486-501
    collide = check_trajectory_collision(previous prediction or window)       503-506
    x_meas  = state + N(0, process_noise_std)  (ENABLE_DISTURBANCES)          509-513
    X, U    = controller.solve(x_meas, window)                                516
    state   = update(state, U[:, 0], params, DISTURBANCE_PARAMS)              524-527
Here one step = sim_window_kernel -> collision_kernel -> [warm_kernel] -> track_kernel -> [record_kernel]
-> plant_kernel, all enqueued on one stream (libttmpc.so: tt_sim.hip + tt_track.hip).  With a switch
solver (USE_SWITCH_MPC, simulation.py:23, 433-441) the instances whose check collides are re-solved by
MPCTrackingControlObs (the OBCA kernel) and their results replace the tracking solution.

The reference draws the measurement noise with np.random.normal; pass ``noise`` (steps, B, 6) to
reproduce a given draw, else it is drawn on the device with a seeded torch generator.

Reverse mode: ``ClosedLoop.run_tape`` keeps every step's solve on the device and ``ClosedLoop.backward`` sweeps that
tape for the gradient of a loss on the visited states and applied controls with respect to x_init, the weights, the
plan and the noise (tt_sim_vjp.hip around tt_vjp.hip; ``ttmpc.diff.DifferentiableClosedLoop`` is the autograd layer).
A loop built with a ``FuzzyRule`` (the fuzzy weight rule with its constants as data, tt_fuzzy.hip) is differentiable
with respect to the rule's parameters too.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import dataclasses
import math

import numpy as np
import torch

from ._lib import TT_ACCEPTABLE, TT_MAX_ITER, TT_VARIANT_FUZZY, TTError, TTFuzzyRule, TTPlant, lib

# closed-loop failure policies (include/ttmpc.h TT_POLICY_*): what a driver does after a failed solve
POLICIES = {"track": 0, "nmpc": 1, "fuzzy": 2}

# simulation.py:26-32
DISTURBANCE_PARAMS = {"friction_coeff": 0.9, "slippage_coeff": 0.9, "process_noise_std": 0.02,
                      "lateral_slip_gain": 0.01, "slip_angle_max": 0.0}
# simulation_nmpc.py:21-27 (there ENABLE_DISTURBANCES = False)
DISTURBANCE_PARAMS_NMPC = {"friction_coeff": 1.0, "slippage_coeff": 1.0, "process_noise_std": 0.02,
                           "lateral_slip_gain": 0.0, "slip_angle_max": 0.0}


def plant(params, disturbance_params=None) -> TTPlant:
    """tt_plant from the reference's params dict (+ DISTURBANCE_PARAMS, or None = nominal update)."""
    p = TTPlant()
    p.dt, p.L1, p.L2, p.Mh = float(params["dt"]), float(params["L1"]), float(params["L2"]), float(params["M"])
    p.W1, p.W2 = float(params.get("W1", 0.0)), float(params.get("W2", 0.0))
    d = disturbance_params
    p.enable = int(d is not None)
    d = d or {}
    # apply_disturbances / apply_slippage_to_dynamics / apply_lateral_slip skip a missing key
    p.friction_coeff = float(d.get("friction_coeff", 1.0))
    p.slippage_coeff = float(d.get("slippage_coeff", 1.0))
    p.process_noise_std = float(d.get("process_noise_std", 0.0))
    p.lateral_slip_gain = float(d.get("lateral_slip_gain", 0.0))
    p.slip_angle_max = float(d.get("slip_angle_max", 0.0))
    return p


def _stream(stream, dev):
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    return C.c_void_p(s.cuda_stream)


def _check(rc, what):
    if rc != 0:
        raise TTError(f"{what} failed ({rc})")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _dev(a, dev, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a) if not torch.is_tensor(a) else a, dtype=dtype).to(dev).contiguous()


def check_tensor(name, t, shape, dev=None, got=False):
    """Raise unless t is a float64 tensor of exactly ``shape`` (the kernels index it as such) on ``dev``; got: the
    message also says what came instead.  dev None, the autograd layer's inputs: on any CUDA device, a TypeError for
    the kind of tensor and a ValueError for its shape."""
    shape = tuple(shape)
    if dev is None:
        if not (t.is_cuda and t.dtype == torch.float64):
            raise TypeError(f"{name} must be a float64 CUDA tensor, got {t.dtype} on {t.device}")
        if tuple(t.shape) != shape:
            raise ValueError(f"{name} must have shape {shape}, got {tuple(t.shape)}")
    elif not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and t.device == dev and
              tuple(t.shape) == shape):
        what = (tuple(t.shape), t.dtype, t.device) if isinstance(t, torch.Tensor) else type(t)
        raise ValueError(f"{name} must be a float64 tensor of shape {shape} on {dev}" + (f", got {what}" if got else ""))


def _run_noise(noise, K, B, dev):
    """A whole run's noise draws (host or device, or None) as a (steps, B, 6) float64 tensor on the device."""
    if noise is None:
        return None
    nz = _dev(noise.detach() if isinstance(noise, torch.Tensor) else noise, dev)
    if tuple(nz.shape) != (K, B, 6):
        raise ValueError(f"noise must have shape (steps, B, 6) = {(K, B, 6)}, got {tuple(nz.shape)}")
    return nz


# ---------------------------------------------------------------- single-kernel device entry points
def window(plan_x, plan_u, k, N, state=None, noise=None, x_meas=None, xref=None, uref=None, stream=None):
    """Reference window (simulation.py:486-501) for every instance: plan_x (P,Np+1,6), plan_u (P,Np,2) device
    tensors with P = 1 (shared plan) or B; state (B,6) -> x_meas = state + noise (509-513)."""
    dev = plan_x.device
    Np = plan_u.shape[-2]
    B = state.shape[0] if state is not None else plan_x.shape[0]
    xref = torch.empty((B, N + 1, 6), dtype=torch.float64, device=dev) if xref is None else xref
    uref = torch.empty((B, N, 2), dtype=torch.float64, device=dev) if uref is None else uref
    if state is not None and x_meas is None:
        x_meas = torch.empty((B, 6), dtype=torch.float64, device=dev)
    per = int(plan_x.shape[0] != 1)
    if per and plan_x.shape[0] != B:
        raise ValueError("per-instance plans need one plan per instance")
    _check(lib().tt_sim_window_device(B, int(N), int(k), int(Np), plan_x.data_ptr(), plan_u.data_ptr(), per,
                                      _ptr(state), _ptr(noise), _ptr(x_meas), xref.data_ptr(), uref.data_ptr(),
                                      _stream(stream, dev)), "tt_sim_window_device")
    return x_meas, xref, uref


def collision_flags(poses, obstacles, params, flag=None, stream=None):
    """check_trajectory_collision (simulation.py:363-385) per instance: poses (B,K,>=4) device tensor with
    contiguous rows; obstacles (M,4) device tensor, or (B,M,4) for per-instance scenes (tt_collision_scenes_device:
    instance b against obstacles[b]).  -> int32 flag (B,)."""
    dev = poses.device
    B, K, w = poses.shape
    flag = torch.empty(B, dtype=torch.int32, device=dev) if flag is None else flag
    p = plant(params)
    if poses.stride(-1) != 1:
        raise ValueError("pose rows must be contiguous")
    sk = poses.stride(1) if K > 1 else w          # a size-1 dim may carry any stride (numpy gives 0)
    if obstacles is not None and obstacles.dim() == 3:
        if obstacles.shape[0] != B or obstacles.shape[2] != 4 or not obstacles.is_contiguous():
            raise ValueError(f"per-instance obstacles must be a contiguous (B, M, 4) = ({B}, M, 4) tensor, got "
                             f"{tuple(obstacles.shape)}")
        M = int(obstacles.shape[1])
        _check(lib().tt_collision_scenes_device(B, K, poses.data_ptr(), poses.stride(0), sk,
                                                None if M == 0 else obstacles.data_ptr(), M, C.byref(p),
                                                flag.data_ptr(), _stream(stream, dev)), "tt_collision_scenes_device")
        return flag
    M = 0 if obstacles is None else int(obstacles.shape[0])
    _check(lib().tt_collision_device(B, K, poses.data_ptr(), poses.stride(0), sk,
                                     None if M == 0 else obstacles.data_ptr(), M, C.byref(p), flag.data_ptr(),
                                     _stream(stream, dev)), "tt_collision_device")
    return flag


def plant_update(state, u, params, disturbance_params=None, status=None, zero_on_fail=False, u_applied=None,
                 stream=None, state_noise=None):
    """update(q, u, params, disturbance_params) (simulation.py:167-199) in place on state (B,6); u is
    (B,2) or a solve's U (B,N,2) (applies U[:, 0]).  state_noise (B,6): the NMPC / fuzzy drivers' update
    (simulation_nmpc.py:94-105), which adds state_noise * dt right after the Euler step."""
    dev = state.device
    p = plant(params, disturbance_params)
    stride = u.stride(0)
    if state_noise is not None and (state_noise.shape != state.shape or not state_noise.is_contiguous()):
        raise ValueError("state_noise must be a contiguous (B, 6) tensor")
    _check(lib().tt_plant_update_noise_device(state.shape[0], C.byref(p), state.data_ptr(), u.data_ptr(), stride,
                                              _ptr(status), int(bool(zero_on_fail)), _ptr(state_noise), _ptr(u_applied),
                                              _stream(stream, dev)), "tt_plant_update_noise_device")
    return state


def update(q, u, params, disturbance_params=None, device=0, state_noise=None):
    """Host convenience with the reference's signature (simulation.py:167): one state, numpy in / out.
    state_noise (6,): simulation_nmpc.py / simulation_fuzzy.py's update, with the process noise the reference
    draws inside apply_disturbances given explicitly."""
    dev = torch.device("cuda", device)
    s = _dev(np.asarray(q, dtype=np.float64).reshape(1, 6), dev)
    sn = None if state_noise is None else _dev(np.asarray(state_noise, dtype=np.float64).reshape(1, 6), dev)
    plant_update(s, _dev(np.asarray(u, dtype=np.float64).reshape(1, 2), dev), params, disturbance_params,
                 state_noise=sn)
    return s.cpu().numpy()[0]


def interpolate(state_traj, input_traj, dt_1, dt_2, stream=None):
    """do_interpolation (simulation.py:201-218) of B plans on the device: (B,Np+1,6), (B,Np,2) ->
    (B,nNp+1,6), (B,nNp,2), n = floor(dt_1/dt_2)."""
    dev = state_traj.device
    B, Np = input_traj.shape[0], input_traj.shape[1]
    n = math.floor(dt_1 / dt_2)
    so = torch.empty((B, n * Np + 1, 6), dtype=torch.float64, device=dev)
    uo = torch.empty((B, n * Np, 2), dtype=torch.float64, device=dev)
    _check(lib().tt_interpolate_device(B, Np, n, state_traj.data_ptr(), input_traj.data_ptr(), so.data_ptr(),
                                       uo.data_ptr(), _stream(stream, dev)), "tt_interpolate_device")
    return so, uo


def policy_plant_vjp(state, status, active_after, consecutive, adj_state, adj_u_last, grad_u, params,
                     disturbance_params=None, policy="track", active_before=None, grad_u_applied=None,
                     g_state_noise=None, stream=None, g_model=None):
    """Adjoint of one policy + plant step (tt_policy_plant_vjp_device; include/ttmpc.h has the branch table), device
    tensors: state (B,6) = S_t, status / active_after / consecutive (B,) int32 from the logs, active_before (B,) or None
    (the first step: all active), grad_u_applied (B,2) = dL/dUa_t or None.  In place: adj_state (B,6) = dL/dS_{t+1}
    becomes the plant's share of dL/dS_t, adj_u_last (B,2) the adjoint of u_last; grad_u (B,N,2) gets the seed
    dL/dU_t[0] in row 0; g_state_noise (B,6), if given, dL/d(in-plant noise).  g_model (B,3), if given, is an
    accumulator: += adj_state' dS_{t+1}/d(L1, L2, M) of the plant's geometry, with adj_state as it came in
    (tt_policy_plant_vjp_model_device); stopped and inactive instances add nothing."""
    dev = state.device
    if policy not in POLICIES:
        raise ValueError(f"policy must be one of {sorted(POLICIES)}")
    p = plant(params, disturbance_params)
    _check(lib().tt_policy_plant_vjp_model_device(   # (a NULL accumulator forwards to the plain entry)
        state.shape[0], grad_u.shape[1], C.byref(p), POLICIES[policy], state.data_ptr(), status.data_ptr(),
        _ptr(active_before), active_after.data_ptr(), consecutive.data_ptr(), _ptr(grad_u_applied),
        adj_state.data_ptr(), adj_u_last.data_ptr(), grad_u.data_ptr(), _ptr(g_state_noise), _ptr(g_model),
        _stream(stream, dev)), "tt_policy_plant_vjp_model_device" if g_model is not None else "tt_policy_plant_vjp_device")
    return adj_state, adj_u_last, grad_u


def window_vjp(g_xref, g_uref, k, Np, g_plan_x=None, g_plan_u=None, shared=False, g_x0=None, grad_state=None,
               adj_state=None, g_wq_wr=None, g_wq_wr_acc=None, g_meas_noise=None, stream=None):
    """Adjoint of ``window`` at step index k (tt_sim_window_vjp_device): g_xref (B,N+1,6), g_uref (B,N,2) are
    scatter-added, with the forward's end padding and without atomics, into the per-instance plan gradients g_plan_x
    (B,Np+1,6), g_plan_u (B,Np,2) (made of zeros when None).  shared=True returns their sums over B, (1,Np+1,6) and
    (1,Np,2), the gradient of one plan shared by all instances.  The step's per-instance accumulation rides along when
    asked for: adj_state += g_x0 + grad_state, g_wq_wr_acc += g_wq_wr, g_meas_noise = g_x0."""
    dev = g_xref.device
    B, N = g_uref.shape[0], g_uref.shape[1]
    z = lambda *sh: torch.zeros(sh, dtype=torch.float64, device=dev)  # noqa: E731
    g_plan_x = z(B, Np + 1, 6) if g_plan_x is None else g_plan_x
    g_plan_u = z(B, Np, 2) if g_plan_u is None else g_plan_u
    _check(lib().tt_sim_window_vjp_device(B, N, int(k), int(Np), g_xref.data_ptr(), g_uref.data_ptr(),
                                          g_plan_x.data_ptr(), g_plan_u.data_ptr(), _ptr(g_x0), _ptr(grad_state),
                                          _ptr(adj_state), _ptr(g_wq_wr), _ptr(g_wq_wr_acc), _ptr(g_meas_noise),
                                          _stream(stream, dev)), "tt_sim_window_vjp_device")
    if shared:
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            return g_plan_x.sum(dim=0, keepdim=True), g_plan_u.sum(dim=0, keepdim=True)
    return g_plan_x, g_plan_u


@dataclasses.dataclass(frozen=True)
class FuzzyRule:
    """tt_fuzzy_rule (include/ttmpc.h): the constants of the fuzzy weight rule (mpc_control_fuzzy.py:90-119), the
    reference's by default.  The first seven fields are the differentiable vector theta; w_min, w_max and v_rev are
    settings without a gradient."""
    psi_full: float = 0.35
    gain_hitch: float = 2.0
    gain_steer: float = 1.2
    gain_rate: float = 1.5
    rev_hitch: float = 1.1
    rev_steer: float = 1.1
    rev_rate: float = 1.2
    w_min: float = 1.0
    w_max: float = 3.5
    v_rev: float = -0.1

    def __post_init__(self):
        v = dataclasses.astuple(self)
        if not (all(math.isfinite(float(t)) for t in v) and self.psi_full > 0 and self.w_min <= self.w_max):
            raise ValueError(f"fuzzy rule: every value finite, psi_full > 0 and w_min <= w_max, got {self}")

    def as_struct(self) -> TTFuzzyRule:
        return TTFuzzyRule(*(float(t) for t in dataclasses.astuple(self)))

    def theta(self):
        """(psi_full, gain_hitch, gain_steer, gain_rate, rev_hitch, rev_steer, rev_rate)."""
        return tuple(float(t) for t in dataclasses.astuple(self)[:7])

    def with_theta(self, theta):
        """This rule with other values of theta (7), the settings kept."""
        theta = [float(t) for t in theta]
        if len(theta) != 7:
            raise ValueError("theta has seven entries")
        return FuzzyRule(*theta, self.w_min, self.w_max, self.v_rev)


def _rule_ref(rule):
    return None if rule is None else C.byref(rule.as_struct())


def fuzzy_weights_rule(x, xref, rule=None, wq_wr=None, stream=None):
    """The fuzzy weights (B,8) of measured states x (B,6) and windows xref (B,N+1,6), device tensors, for a
    ``FuzzyRule`` (tt_fuzzy_weights_rule_device; None: the reference's constants, bitwise tt_fuzzy_weights_device)."""
    dev = x.device
    B, N = x.shape[0], xref.shape[1] - 1
    wq_wr = torch.empty((B, 8), dtype=torch.float64, device=dev) if wq_wr is None else wq_wr
    _check(lib().tt_fuzzy_weights_rule_device(B, N, _rule_ref(rule), x.data_ptr(), xref.data_ptr(), wq_wr.data_ptr(),
                                              _stream(stream, dev)), "tt_fuzzy_weights_rule_device")
    return wq_wr


def fuzzy_weights_vjp(x, xref, g_wq_wr, rule=None, retried=None, g_x=None, g_rule=None, stream=None):
    """Adjoint of ``fuzzy_weights_rule`` (tt_fuzzy_weights_vjp_device): for the upstream g_wq_wr (B,8), g_x (B,6) gets
    g_x[:, 3] += dL/dpsi and g_rule (B,7) += dL/dtheta per instance; both are accumulators, made of zeros when None.
    retried (B,) int32 or None: instances whose accepted solve used unit weights add nothing.  -> (g_x, g_rule)."""
    dev = x.device
    B, N = x.shape[0], xref.shape[1] - 1
    g_x = torch.zeros((B, 6), dtype=torch.float64, device=dev) if g_x is None else g_x
    g_rule = torch.zeros((B, 7), dtype=torch.float64, device=dev) if g_rule is None else g_rule
    _check(lib().tt_fuzzy_weights_vjp_device(B, N, _rule_ref(rule), x.data_ptr(), xref.data_ptr(), _ptr(retried),
                                             g_wq_wr.data_ptr(), g_x.data_ptr(), g_rule.data_ptr(),
                                             _stream(stream, dev)), "tt_fuzzy_weights_vjp_device")
    return g_x, g_rule


class LoopTape:
    """The device log of an eager run.  Every recorded run has the step indices ks and the logs S (K+1,B,6), Ua
    (K,B,2), status / iters / collide / active (K,B) (active: after each step).  ``ClosedLoop.run_tape`` also keeps
    what ``ClosedLoop.backward`` needs, None in a plain ``run``: consec (K,B), the consecutive-failure count after each
    step, each step's solve X (K,B,N+1,6), U (K,B,N,2), dual (K,B,N+1,22) and the noise it used (K,B,6) or None.
    wq_wr (B,8) or None are the run's weights, plan_x / plan_u the plan it saw, model_solver / model_plant the
    (L1, L2, M) of the solver's handle and of the plant during a taped run, bounds the handle's box (xlb, xub, ulb, uub)
    during it.  The taped run of a loop with a
    ``FuzzyRule`` also keeps rule (that rule), W (K,B,8), the weights each step's accepted solve used (ones where the
    unit-weight retry was taken), and retried (K,B) int32, where it was: 68 bytes per instance and step.  The taped run
    of a switch loop (``switch_adjoint=True``) keeps switched: per step None, or (idx (n,) int64, the flagged instances;
    iterate (n, tt_obca_iterate_len), the MPC+OBCA solve's exported iterates of those instances; status (n,) int32),
    and geometry_switch, the (L1, L2, M, W1, W2) of the switch solver's handle during the run."""
    __slots__ = ("ks", "S", "Ua", "status", "iters", "collide", "active", "consec", "X", "U", "dual", "noise", "wq_wr",
                 "plan_x", "plan_u", "model_solver", "model_plant", "W", "retried", "rule", "switched",
                 "geometry_switch", "bounds")
    # (log field, the loop's buffer a step leaves it in), in the order record() copies them; the solve writes dual
    STEP = (("S", "state"), ("Ua", "u_applied"), ("status", "st"), ("iters", "it"), ("collide", "flag"),
            ("active", "active"), ("consec", "consec"), ("X", "X"), ("U", "U"), ("W", "wq"), ("retried", "retried"))

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))

    @classmethod
    def alloc(cls, loop, ks, record=True, taped=False, **kw):
        """The log of a run of ``loop`` over the steps ks: the logs if record, the backward's fields too if taped."""
        K, B, N = len(ks), loop.B, loop.N
        new = lambda *sh, dtype=torch.float64: torch.empty(sh, dtype=dtype, device=loop.dev)  # noqa: E731
        log = cls(ks=list(ks), plan_x=loop.plan_x, plan_u=loop.plan_u, **kw)
        if record:
            log.S, log.Ua = new(K + 1, B, 6), new(K, B, 2)
            log.status, log.iters, log.collide, log.active = (new(K, B, dtype=torch.int32) for _ in range(4))
        if taped:
            log.consec = new(K, B, dtype=torch.int32)
            log.X, log.U, log.dual = new(K, B, N + 1, 6), new(K, B, N, 2), new(K, B, N + 1, 22)
            log.model_solver, log.model_plant = loop.solver.model(), loop.plant_model()   # (run_tape: a BatchSolver)
            log.bounds = loop.solver.get_bounds()
            if loop.switch is not None and loop.switch_adjoint:
                log.geometry_switch = loop.switch.geometry()
            if loop.rule is not None:
                log.W, log.retried, log.rule = new(K, B, 8), new(K, B, dtype=torch.int32), loop.rule
        return log

    def record(self, j, loop):
        """Copy what step j left in the loop's buffers into every allocated field, on the current stream."""
        for name, src in self.STEP:
            dst = getattr(self, name)
            if dst is not None:
                dst[j + 1 if name == "S" else j].copy_(getattr(loop, src))

    def result(self):
        """The logs as the numpy dict ``run`` returns (after a synchronisation)."""
        st, act = self.status.cpu().numpy(), self.active.cpu().numpy()
        stop = np.where((act == 0).any(axis=0), (act == 0).argmax(axis=0), -1)
        return dict(k=np.array(self.ks), states=self.S.cpu().numpy(), controls=self.Ua.cpu().numpy(), status=st,
                    iters=self.iters.cpu().numpy(), collide=self.collide.cpu().numpy().astype(bool),
                    success=st <= TT_ACCEPTABLE, active=act.astype(bool), stop_step=stop)

    def nbytes(self):
        return sum(t.numel() * t.element_size() for t in (getattr(self, k) for k in self.__slots__)
                   if isinstance(t, torch.Tensor))


def step_indices(T_sim, dt):
    """The reference's step sequence: t = 0; while t <= T_sim: k = floor(t/dt); ...; t += dt."""
    ks, t = [], 0.0
    while t <= T_sim:
        ks.append(math.floor(t / dt))
        t += dt
    return ks


class ClosedLoop:
    """B independent closed loops driven by one tracking solver (a ttmpc.BatchSolver of horizon N).

    plan_x / plan_u: one shared plan in the reference's (6,Np+1) / (2,Np) orientation (e.g.
    do_interpolation(state_traj.txt, ...)), or (B,Np+1,6) / (B,Np,2) per-instance plans.  warm_start=True
    is TruckTrailerNMPC's shifted warm start (NMPC / fuzzy solvers).

    policy: the driver's reaction to a failed solve, on the device per instance (tt_policy_plant_device):
      "track" (simulation.py:519-527) applies the returned inputs; "nmpc" (simulation_nmpc.py:206-216)
      applies zero control and stops the instance after 20 consecutive failures; "fuzzy"
      (simulation_fuzzy.py:207-221) re-applies the last successful control, zero after 15 consecutive
      failures, stops after 30.  Default: "fuzzy" for a TT_VARIANT_FUZZY solver, "nmpc" when
      zero_on_fail=True, else "track".  A TT_VARIANT_FUZZY solver gets per-instance fuzzy weights each step
      (tt_fuzzy_weights_device, mpc_control_fuzzy.py:90-119) and its failed instances are re-solved once
      with unit weights from the same guess (145-159).

    fuzzy_rule: None, or a ``FuzzyRule``: the weight rule with its constants as data (tt_fuzzy_weights_rule_device),
      for a solver of any tracking variant (TT_VARIANT_TRACK, _NMPC, _FUZZY), with the unit-weight retry.  Such a loop
      is differentiable (``run_tape`` / ``backward``, also with respect to the rule's parameters); policy and
      noise_in_plant still default from the solver's variant.  None keeps a TT_VARIANT_FUZZY solver on the built-in
      rule, which is not differentiable.

    noise_in_plant=True is the NMPC / fuzzy drivers' disturbance model (simulation_nmpc.py:94-105,
    simulation_fuzzy.py): the solver sees the exact state and, with disturbances on, the process noise
    N(0, process_noise_std) enters the plant as q_ += noise * dt (tt_policy_plant_noise_device); the default is
    simulation.py's (noise on the measured state, simulation.py:509-513).  Default: True for the "nmpc" and
    "fuzzy" policies.

    switch_adjoint=True makes a loop with a switch_solver differentiable (``run_tape`` / ``backward``): the switch step
    then exports the MPC+OBCA solve's iterate, and the backward runs tt_obca_vjp_device on the switched instances.  The
    default keeps such a loop refusing ``run_tape``.

    obstacles of shape (B,M,4) give every loop its own scene: the collision check tests instance b against
    obstacles[b], the switch solves run with the rows of the switched instances (tt_obca_solve_batch_scenes_device; M is
    the switch solver's), and so does their adjoint in ``backward``.  d_min (a scalar or (B,)): the safety margin of the
    switch solves, per instance; None is the switch solver's own.  ``run_graph`` does not take a switch loop either
    way."""

    def __init__(self, solver, plan_x, plan_u, params, disturbance_params=None, measurement_noise=None,
                 obstacles=None, check_collision=True, switch_solver=None, warm_start=False, bug_compatible=True,
                 zero_on_fail=False, device=None, seed=0, policy=None, noise_in_plant=None, fuzzy_rule=None,
                 switch_adjoint=False, d_min=None):
        self.solver = solver
        self.N = solver.N
        self.dev = torch.device("cuda", solver.device if device is None else device)
        px, pu = np.asarray(plan_x, dtype=np.float64), np.asarray(plan_u, dtype=np.float64)
        if px.ndim == 2:   # one shared plan in the reference's orientation: (6, Np+1), (2, Np)
            px, pu = px.T[None], pu.T[None]
        self.plan_x, self.plan_u = _dev(px, self.dev), _dev(pu, self.dev)
        self.params = dict(params)
        self.dist = disturbance_params
        # simulation.py:509-513: noisy measurement iff disturbances are on
        self.measurement_noise = (disturbance_params is not None) if measurement_noise is None else measurement_noise
        ob = None if obstacles is None else np.asarray(obstacles, dtype=np.float64)
        self.per_scene = ob is not None and ob.ndim == 3   # (B,M,4): every loop has its own scene
        if self.per_scene and ob.shape[2] != 4:
            raise ValueError(f"per-instance obstacles must have shape (B, M, 4), got {ob.shape}")
        self.obstacles = None if ob is None else _dev(ob if self.per_scene else ob.reshape(-1, 4), self.dev)
        # the switch solves' safety margin: None (the switch solver's), a float for every loop, or a (B,) device tensor
        dm = None if d_min is None else np.asarray(d_min, dtype=np.float64)
        if dm is not None and dm.ndim > 1:
            raise ValueError(f"d_min must be a scalar or have shape (B,), got {dm.shape}")
        self.d_min = None if dm is None else (float(dm) if dm.ndim == 0 else _dev(dm, self.dev))
        if switch_solver is not None and self.per_scene and ob.shape[1] != switch_solver.M:
            raise ValueError(f"per-instance obstacles have M = {ob.shape[1]}, the switch solver has M = "
                             f"{switch_solver.M}")
        self.check_collision = check_collision and self.obstacles is not None
        self.switch = switch_solver
        self.switch_adjoint = bool(switch_adjoint)   # run_tape / backward through the switch solve (tt_obca_vjp_device)
        self._switched = None                         # a taped run's per-step record of the switch solves
        self.warm, self.bug_compatible, self.zero_on_fail = warm_start, bug_compatible, zero_on_fail
        self._fuzzy_variant = getattr(solver, "variant", None) == TT_VARIANT_FUZZY
        self.set_fuzzy_rule(fuzzy_rule)
        if policy is None:
            policy = "fuzzy" if self._fuzzy_variant else ("nmpc" if zero_on_fail else "track")
        if policy not in POLICIES:
            raise ValueError(f"policy must be one of {sorted(POLICIES)}")
        self.policy = policy
        self.noise_in_plant = (policy in ("nmpc", "fuzzy")) if noise_in_plant is None else bool(noise_in_plant)
        if self.noise_in_plant and measurement_noise:
            raise ValueError("noise_in_plant: the NMPC / fuzzy drivers measure the exact state")
        if self.noise_in_plant:
            self.measurement_noise = False
        self.gen = torch.Generator(device=self.dev)
        self.gen.manual_seed(int(seed))
        self.stream = torch.cuda.Stream(self.dev)

    def plant_model(self):
        """The plant's (L1, L2, M)."""
        return tuple(float(self.params[k]) for k in ("L1", "L2", "M"))

    def set_model(self, solver=None, plant=None):
        """Change the geometry (L1, L2, M) the controller believes (``solver``: through the handle, tt_set_model) and /
        or the plant's (``plant``: this loop's own copy in ``params``, which also feeds the collision check).  Host-side
        state only: later steps and runs use the new values.  ``run_graph`` captures its step anew on every call, so it
        never replays a capture made with other values.  A tape keeps the geometry of its run; ``backward`` on a tape
        made before a change raises."""
        if solver is not None:
            self.solver.set_model(*(float(v) for v in solver))
        if plant is not None:
            L1, L2, M = (float(v) for v in plant)
            if not (L1 > 0 and L2 > 0 and math.isfinite(L1) and math.isfinite(L2) and math.isfinite(M)):
                raise ValueError("plant geometry: L1, L2 must be > 0 and M finite")
            self.params.update(L1=L1, L2=L2, M=M)

    def set_bounds(self, xlb=None, xub=None, ulb=None, uub=None):
        """Change the box of the tracking solver (``BatchSolver.set_bounds``, tt_set_bounds; a vector left None keeps its
        values).  Host-side state only: later steps and runs solve in the new box; the plant does not clip, so the box
        enters the loop through the solves alone.  ``run_graph`` captures its step anew on every call.  A tape keeps the
        box of its run; ``backward`` on a tape made before a change raises."""
        self.solver.set_bounds(xlb, xub, ulb, uub)

    def set_fuzzy_rule(self, rule):
        """The ``FuzzyRule`` of the steps and runs from now on (None: the built-in rule for a TT_VARIANT_FUZZY solver,
        no rule for another).  Host-side state only.  A tape keeps the rule of its run; ``backward`` on a tape made
        with another raises."""
        if rule is not None and not isinstance(rule, FuzzyRule):
            raise TypeError("fuzzy_rule must be a ttmpc.simulation.FuzzyRule or None")
        self.rule = rule
        self.fuzzy = self._fuzzy_variant or rule is not None   # per-step weights and the unit-weight retry

    def _scene_rows(self, idx):
        """The per-instance scenes of the compacted batch idx: (obstacles (n,M,4) | None, d_min (n,) | None)."""
        ob = self.obstacles[idx].contiguous() if self.per_scene else None
        if self.d_min is None or torch.is_tensor(self.d_min):
            dm = None if self.d_min is None else self.d_min[idx].contiguous()
        else:
            dm = torch.full((int(idx.numel()),), self.d_min, dtype=torch.float64, device=self.dev)
        return ob, dm

    def _alloc(self, B):
        N, d, f = self.N, self.dev, torch.float64
        for name, t in (("obstacles", self.obstacles if self.per_scene else None), ("d_min", self.d_min)):
            if torch.is_tensor(t) and t.shape[0] != B:
                raise ValueError(f"per-instance {name} are for B = {t.shape[0]} loops, the run has B = {B}")
        self.B = B
        self.state = torch.empty((B, 6), dtype=f, device=d)
        self.x_meas = torch.empty((B, 6), dtype=f, device=d)
        self.xref = torch.empty((B, N + 1, 6), dtype=f, device=d)
        self.uref = torch.empty((B, N, 2), dtype=f, device=d)
        self.X = torch.empty((B, N + 1, 6), dtype=f, device=d)
        self.U = torch.empty((B, N, 2), dtype=f, device=d)
        self.st = torch.empty(B, dtype=torch.int32, device=d)
        self.it = torch.empty(B, dtype=torch.int32, device=d)
        self.kkt = torch.empty(B, dtype=f, device=d)
        self.flag = torch.zeros(B, dtype=torch.int32, device=d)
        self.u_applied = torch.empty((B, 2), dtype=f, device=d)
        # failure-policy state (tt_policy_plant_device)
        self.u_last = torch.zeros((B, 2), dtype=f, device=d)
        self.consec = torch.zeros(B, dtype=torch.int32, device=d)
        self.fails = torch.zeros(B, dtype=torch.int32, device=d)
        self.active = torch.ones(B, dtype=torch.int32, device=d)
        self.wq = torch.empty((B, 8), dtype=f, device=d)          # the fuzzy weights of a step
        self.retried = torch.empty(B, dtype=torch.int32, device=d)  # taped fuzzy steps: took the unit-weight retry
        if self.warm:
            self.zg = torch.empty((B, 8 * N + 6), dtype=f, device=d)
            self.last = torch.zeros((B, 8 * N + 6), dtype=f, device=d)
            self.have = torch.zeros(B, dtype=torch.int32, device=d)

    def reset(self, x_init):
        x = np.asarray(x_init, dtype=np.float64).reshape(-1, 6)
        self._alloc(x.shape[0])
        self.state.copy_(_dev(x, self.dev))
        self.first = True
        # the buffers were allocated and filled on the current stream; step() works on self.stream
        self.stream.wait_stream(torch.cuda.current_stream(self.dev))

    def _check_noise(self, noise, shape):
        check_tensor("noise", noise, shape, self.dev, got=True)

    def step(self, k, noise=None, dual=None, wq_wr=None):
        """Enqueue one closed-loop step at window index k (noise: (B,6) float64 device tensor or None: the measurement
        noise, or with noise_in_plant -- the default of the "nmpc" / "fuzzy" policies -- the plant's process noise
        before its dt factor).  dual (B,N+1,22): also export the solve's multipliers (run_tape; the solve is bitwise
        the plain one); wq_wr (B,8): per-instance weights of a solver that is not TT_VARIANT_FUZZY."""
        s, N = self.stream, self.N
        if noise is not None:
            self._check_noise(noise, (self.B, 6))
        with torch.cuda.stream(s):
            if noise is None and self._noisy:
                noise = self._draw()
            meas = noise if self.measurement_noise else None
            self._enqueue_step(lambda: window(self.plan_x, self.plan_u, k, N, self.state, meas, self.x_meas, self.xref,
                                              self.uref, stream=s),
                               self.first, noise if self.noise_in_plant else None, dual, wq_wr)
        self.first = False

    @property
    def _noisy(self):
        """Whether a run without given noise draws its own."""
        return (self.measurement_noise or self.noise_in_plant) and self.dist is not None

    def _draw(self, *steps, out=None):
        """process_noise_std * N(0, 1) of shape (*steps, B, 6) from the loop's generator, on the current stream; copied
        to ``out`` before the scaling if given."""
        nz = torch.randn((*steps, self.B, 6), generator=self.gen, dtype=torch.float64, device=self.dev)
        if out is not None:
            nz = out.copy_(nz)
        return nz.mul_(float(self.dist.get("process_noise_std", 0.0)))

    def _enqueue_step(self, enqueue_window, first, plant_noise, dual=None, wq_wr=None):
        """The one statement of a closed-loop step, enqueued on the loop's stream (the caller has made it current):
        enqueue_window() -> collision check (first: of the first window, else of the previous prediction) -> [warm
        start] -> [fuzzy weights] -> solve [-> fuzzy retry] [-> switch solve] -> [record] -> policy + plant.
        plant_noise: the plant's process noise (B,6), None, or a callable that enqueues its selection on the device
        right before the plant and returns it (the replayed step).  dual, wq_wr: as ``step`` takes them."""
        L, s, B, N = lib(), self.stream, self.B, self.N
        sp = C.c_void_p(s.cuda_stream)
        enqueue_window()
        if self.check_collision:
            collision_flags(self.xref if first else self.X, self.obstacles, self.params, self.flag, stream=s)
        zg = 0
        if self.warm:
            _check(L.tt_warm_start_device(B, N, self.last.data_ptr(), self.have.data_ptr(), self.xref.data_ptr(),
                                          self.uref.data_ptr(), int(self.bug_compatible), self.zg.data_ptr(), sp),
                   "tt_warm_start_device")
            zg = self.zg.data_ptr()
        wq = 0
        if self.rule is not None:
            _check(L.tt_fuzzy_weights_rule_device(B, N, _rule_ref(self.rule), self.x_meas.data_ptr(),
                                                  self.xref.data_ptr(), self.wq.data_ptr(), sp),
                   "tt_fuzzy_weights_rule_device")
            wq = self.wq.data_ptr()
        elif self.fuzzy:
            _check(L.tt_fuzzy_weights_device(B, N, self.x_meas.data_ptr(), self.xref.data_ptr(), self.wq.data_ptr(),
                                             sp), "tt_fuzzy_weights_device")
            wq = self.wq.data_ptr()
        elif wq_wr is not None:
            wq = wq_wr.data_ptr()
        io = [t.data_ptr() for t in (self.x_meas, self.xref, self.uref, self.X, self.U, self.st, self.it, self.kkt)]
        if dual is None:
            self.solver.solve_device(B, *io, wq_wr=wq, z_guess=zg, stream=s.cuda_stream)
        else:
            self.solver.solve_ex_device(B, *io, wq_wr=wq, z_guess=zg, dual=dual.data_ptr(), stream=s.cuda_stream)
        if self.fuzzy:
            self._fuzzy_retry(s, dual)
        if self.switch is not None and self.check_collision:
            self._switch_solve(s)
        if self.warm:
            _check(L.tt_record_solution_device(B, N, self.X.data_ptr(), self.U.data_ptr(), self.st.data_ptr(),
                                               self.last.data_ptr(), self.have.data_ptr(), sp),
                   "tt_record_solution_device")
        self._policy_plant(sp, plant_noise() if callable(plant_noise) else plant_noise)

    def _policy_plant(self, sp, state_noise=None):
        p = plant(self.params, self.dist)
        sn = None
        if state_noise is not None:
            self._check_noise(state_noise, (self.B, 6))
            state_noise = state_noise.contiguous()
            self._sn = state_noise    # keep it alive until the stream has consumed it
            sn = state_noise.data_ptr()
        _check(lib().tt_policy_plant_noise_device(self.B, C.byref(p), POLICIES[self.policy], self.state.data_ptr(),
                                                  self.U.data_ptr(), self.U.stride(0), self.st.data_ptr(),
                                                  self.u_last.data_ptr(), self.consec.data_ptr(), self.fails.data_ptr(),
                                                  self.active.data_ptr(), sn, self.u_applied.data_ptr(), sp),
               "tt_policy_plant_noise_device")

    def _fuzzy_retry(self, s, dual=None):
        """mpc_control_fuzzy.py:145-159: failed instances re-solve once with unit weights, same guess.  dual (a taped
        step): the retry exports its multipliers too, and the step leaves in ``retried`` / ``wq`` which instances took
        it and the weights every accepted solve used."""
        idx = torch.nonzero((self.st > TT_ACCEPTABLE) & (self.active != 0), as_tuple=True)[0]

        def solve(n, *io, dual=0):
            w = torch.ones((n, 8), dtype=torch.float64, device=self.dev)
            zg = self.zg[idx].contiguous() if self.warm else None
            kw = dict(wq_wr=w.data_ptr(), z_guess=0 if zg is None else zg.data_ptr(), stream=s.cuda_stream)
            if dual:
                self.solver.solve_ex_device(n, *io, dual=dual, **kw)
            else:
                self.solver.solve_device(n, *io, **kw)
        self._resolve(idx, solve, dual)
        if dual is not None:
            self.retried.zero_()
            if idx.numel():
                self.retried[idx] = 1
                self.wq[idx] = 1.0

    def _switch_solve(self, s):
        """USE_SWITCH_MPC: instances whose check collided use MPCTrackingControlObs (simulation.py:506-512).  In a taped
        run the solve also exports its iterates (the other outputs are bitwise the same), and the step's record
        (flagged indices, compacted iterates and statuses) joins the tape."""
        idx = torch.nonzero(self.flag, as_tuple=True)[0]
        rec = self._switched
        # per-instance scenes: the rows of the compacted batch (allocated on the loop's stream, which consumes them)
        ob, dm = self._scene_rows(idx) if (self.per_scene or self.d_min is not None) and idx.numel() else (None, None)
        rows = dict(obstacles=_ptr(ob) or 0, d_min=_ptr(dm) or 0) if ob is not None or dm is not None else {}
        if rec is None:
            self._resolve(idx, lambda n, x0, xr, ur, X, U, st, it, kk: self.switch.solve_device(
                n, x0, 0, xr, ur, 0, X, U, 0, st, it, kk, stream=s.cuda_stream, **rows))
            return
        kept = []

        def solve(n, x0, xr, ur, X, U, st, it, kk, dual=0):   # (dual: the tracking solve's export, not the switch's)
            I = torch.empty((n, self.switch.iterate_len()), dtype=torch.float64, device=self.dev)
            self.switch.solve_device(n, x0, 0, xr, ur, 0, X, U, 0, st, it, kk, stream=s.cuda_stream,
                                     iterate=I.data_ptr(), **rows)
            kept.append(I)
        self._resolve(idx, solve)
        rec.append((idx, kept[0], self.st[idx].contiguous()) if kept else None)

    def _resolve(self, idx, solve, dual=None):
        """Solve the instances idx again as a compacted batch and put the results in their places: gathers x_meas,
        xref, uref, calls solve(n, x0, xref, uref, X, U, status, iters, kkt) with device pointers of n-instance buffers
        (it launches on the loop's stream, which is current), scatters the five outputs back.  dual (B,N+1,22), the
        step's multipliers of a taped run: solve also gets dual=<pointer of an (n,N+1,22) buffer>, scattered likewise."""
        n = int(idx.numel())          # host sync: the compaction size decides the launch
        if n == 0:
            return
        N = self.N
        new = lambda *sh, dtype=torch.float64: torch.empty(sh, dtype=dtype, device=self.dev)  # noqa: E731
        x0, xr, ur = self.x_meas[idx].contiguous(), self.xref[idx].contiguous(), self.uref[idx].contiguous()
        X, U, st, it, kk = new(n, N + 1, 6), new(n, N, 2), new(n, dtype=torch.int32), new(n, dtype=torch.int32), new(n)
        if dual is None:
            solve(n, *(t.data_ptr() for t in (x0, xr, ur, X, U, st, it, kk)))
        else:
            D = new(n, N + 1, 22)
            solve(n, *(t.data_ptr() for t in (x0, xr, ur, X, U, st, it, kk)), dual=D.data_ptr())
            dual[idx] = D
        self.X[idx], self.U[idx], self.st[idx], self.it[idx], self.kkt[idx] = X, U, st, it, kk

    # ---------------- hipGraph replay of the closed loop ----------------
    def _graph_step(self, first, d_ks, d_step, noise_all, logs):
        """Enqueue one closed-loop step whose step index lives on the device (replayable): the step at k = d_ks[*d_step]
        with the noise noise_all[*d_step], its logs written at *d_step, then *d_step += 1."""
        L, s, B = lib(), self.stream, self.B
        sp = C.c_void_p(s.cuda_stream)
        meas_all = None if self.noise_in_plant else noise_all

        def enqueue_window():
            _check(L.tt_sim_window_indexed_device(B, self.N, d_ks.data_ptr(), d_step.data_ptr(),
                                                  int(self.plan_u.shape[-2]), self.plan_x.data_ptr(),
                                                  self.plan_u.data_ptr(), int(self.plan_x.shape[0] != 1),
                                                  self.state.data_ptr(), _ptr(meas_all), self.x_meas.data_ptr(),
                                                  self.xref.data_ptr(), self.uref.data_ptr(), sp),
                   "tt_sim_window_indexed_device")

        def select():   # this step's process noise, selected on the device
            return self._sn_buf.copy_(torch.index_select(noise_all, 0, d_step.long()).view(B, 6))
        self._enqueue_step(enqueue_window, first, select if self.noise_in_plant and noise_all is not None else None)
        S, Ua, Ss, Si, Sc = logs
        _check(L.tt_sim_log_advance_device(B, d_step.data_ptr(), self.state.data_ptr(), self.u_applied.data_ptr(),
                                           self.st.data_ptr(), self.it.data_ptr(),
                                           self.flag.data_ptr() if self.check_collision else None, S.data_ptr(),
                                           Ua.data_ptr(), Ss.data_ptr(), Si.data_ptr(), Sc.data_ptr(), sp),
               "tt_sim_log_advance_device")

    def run_graph(self, x_init, T_sim, noise=None):
        """run() with the per-step launches captured once into a hipGraph (torch.cuda.CUDAGraph on this
        loop's stream) and replayed: step 0 runs eagerly (its collision check looks at the first window,
        simulation.py:503-506), steps 1.. replay the captured step.  The step index, the reference's k
        sequence and the measurement noise of every step are device-resident.  Not available with a switch
        solver (its compaction needs the host).  Same logs as run()."""
        if self.switch is not None or self.fuzzy:
            raise ValueError("run_graph supports neither the switch solver nor the fuzzy retry (host compaction); "
                             "use run()")
        ks = step_indices(T_sim, float(self.params["dt"]))
        self.reset(x_init)
        B, K, d, s = self.B, len(ks), self.dev, self.stream
        d_ks = torch.tensor(ks, dtype=torch.int32, device=d)
        d_step = torch.zeros(1, dtype=torch.int32, device=d)
        noise_all = None
        self._sn_buf = torch.empty((B, 6), dtype=torch.float64, device=d)
        if self._noisy:   # one (K, B, 6) draw for the whole run: not the numbers of run()'s K draws of (B, 6)
            noise_all = self._draw(K) if noise is None else _run_noise(noise, K, B, d)
        logs = (torch.empty((K + 1, B, 6), dtype=torch.float64, device=d),
                torch.empty((K, B, 2), dtype=torch.float64, device=d),
                torch.zeros((K, B), dtype=torch.int32, device=d), torch.zeros((K, B), dtype=torch.int32, device=d),
                torch.zeros((K, B), dtype=torch.int32, device=d))
        logs[0][0].copy_(self.state)
        torch.cuda.synchronize(d)
        with torch.cuda.stream(s):
            self._graph_step(True, d_ks, d_step, noise_all, logs)
        if K > 1:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                self._graph_step(False, d_ks, d_step, noise_all, logs)
            with torch.cuda.stream(s):  # replay() launches on the current stream
                for _ in range(K - 1):
                    g.replay()
        torch.cuda.synchronize(d)
        self.first = False
        S, Ua, Ss, Si, Sc = (t.cpu().numpy() for t in logs)
        return dict(self._policy_logs(), k=np.array(ks), states=S, controls=Ua, status=Ss, iters=Si,
                    collide=Sc.astype(bool), success=Ss <= TT_ACCEPTABLE)

    # ---------------- eager runs: plain and taped, one log ----------------
    def _begin(self, x_init, T_sim, noise=None, wq_wr=None, record=True, taped=False):
        """reset() and the log of an eager run to T_sim: -> (log, whether the run draws its noise step by step into
        log.noise).  noise (steps, B, 6) and wq_wr (B, 8): host or device, checked and moved to the device."""
        ks = step_indices(T_sim, float(self.params["dt"]))
        if isinstance(x_init, torch.Tensor):
            x_init = x_init.detach().cpu().numpy()
        self.reset(x_init)
        B, K, d = self.B, len(ks), self.dev
        w = None if wq_wr is None else _dev(wq_wr.detach() if isinstance(wq_wr, torch.Tensor) else wq_wr, d)
        if w is not None and tuple(w.shape) != (B, 8):
            raise ValueError(f"wq_wr must have shape (B, 8) = {(B, 8)}, got {tuple(w.shape)}")
        nz = _run_noise(noise, K, B, d)
        drawn = taped and nz is None and self._noisy
        if drawn:
            nz = torch.empty((K, B, 6), dtype=torch.float64, device=d)
        log = LoopTape.alloc(self, ks, record, taped, noise=nz, wq_wr=w)
        if record:
            log.S[0].copy_(self.state)
        # noise and weights may just have been converted on the current stream; the steps read them on self.stream
        self.stream.wait_stream(torch.cuda.current_stream(d))
        return log, drawn

    def _steps(self, log, drawn=False):
        """Enqueue the steps of an eager run on the loop's stream (no host synchronisation): step(), with the multiplier
        export if the log is a tape, then the step's copies into the log."""
        for j, k in enumerate(log.ks):
            noise = None if log.noise is None else log.noise[j]
            if drawn:   # the draw step() would make, kept
                with torch.cuda.stream(self.stream):
                    self._draw(out=noise)
            self.step(k, noise, dual=None if log.dual is None else log.dual[j], wq_wr=log.wq_wr)
            if log.S is not None:
                with torch.cuda.stream(self.stream):
                    log.record(j, self)

    def run(self, x_init, T_sim, noise=None, record=True):
        """Run the reference's loop to T_sim.  noise: optional (steps, B, 6) measurement-noise draws (with
        noise_in_plant: the plant's process-noise draws).
        Returns numpy logs: states (steps+1,B,6), controls (steps,B,2) as applied, status / iters /
        collide (steps,B), and the step indices k; with record=False only the final state and the policy logs."""
        log, _ = self._begin(x_init, T_sim, noise, record=record)
        self._steps(log)
        torch.cuda.synchronize(self.dev)
        if not record:
            return dict(self._policy_logs(), k=np.array(log.ks), state=self.state.cpu().numpy())
        return dict(self._policy_logs(), **log.result())

    # ---------------- reverse mode: taped run and backward sweep ----------------
    def _check_differentiable(self):
        if self.fuzzy and self.rule is None:
            raise ValueError("the closed loop of a TT_VARIANT_FUZZY solver on the built-in weight rule is not "
                             "differentiable: give the rule as data, ClosedLoop(..., fuzzy_rule=FuzzyRule()), whose "
                             "adjoint and taped retry exist")
        if self.switch is not None and not self.switch_adjoint:
            raise ValueError("the closed loop with a switch solver is differentiable only on request: the OBCA solve's "
                             "adjoint joins the backward with ClosedLoop(..., switch_solver=..., switch_adjoint=True)")
        if self.switch is not None and self.rule is not None:
            raise ValueError("a switch (OBCA) loop with a fuzzy_rule is not differentiable: the rule's adjoint "
                             "(rule=True) is not carried through the switch solve")

    def run_tape(self, x_init, T_sim, noise=None, wq_wr=None):
        """``run`` that also keeps what ``backward`` needs: the same steps with the solve's multipliers exported
        (solve_ex_device: bitwise the plain solve) and each step's X, U, dual copied to a ``LoopTape`` on the device,
        (30 (N+1) - 2) * 8 bytes per instance and step.  wq_wr: constant per-instance weights (B,8), host or device.
        Returns run()'s dict plus "tape".  Solver variants TT_VARIANT_TRACK and TT_VARIANT_NMPC, or any tracking
        variant with a ``FuzzyRule`` (then the weights come from the rule and wq_wr must be None; the unit-weight retry
        exports its multipliers into the step's dual, and the tape keeps W and retried).  A switch solver needs
        ``switch_adjoint=True``: its step then calls the iterate-exporting MPC+OBCA solve and the tape keeps, per step,
        the flagged indices and the compacted iterates and statuses (``LoopTape.switched``)."""
        self._check_differentiable()
        if self.rule is not None and wq_wr is not None:
            raise ValueError("a loop with a fuzzy_rule takes its weights from the rule: wq_wr must be None")
        tape, drawn = self._begin(x_init, T_sim, noise, wq_wr, taped=True)
        if self.switch is not None and self.check_collision:
            self._switched = tape.switched = []
        try:
            self._steps(tape, drawn)
        finally:
            self._switched = None
        torch.cuda.synchronize(self.dev)
        return dict(self._policy_logs(), **tape.result(), tape=tape)

    def backward(self, tape, GS, GU, model=False, rule=False, scene=False, geometry=False, bounds=False):
        """The adjoint of a taped run for a scalar loss L(S, Ua): GS = dL/dS (K+1,B,6), GU = dL/dUa (K,B,2), float64
        device tensors.  Per step, backwards: tt_policy_plant_vjp_device, the step's window again,
        tt_track_vjp_device on the taped solve, tt_sim_window_vjp_device (include/ttmpc.h, "Reverse mode of the closed
        loop").  Enqueued on the loop's stream, which is ordered behind the current stream at entry and ahead of it at
        exit; no host synchronisation.  Returns device tensors dict(g_x_init (B,6), g_wq_wr (B,8), g_plan_x, g_plan_u
        (shaped as the loop's plan: summed over B for a shared one), g_noise (K,B,6): of the measurement noise, or with
        noise_in_plant of the plant's process noise; zeros where the run had no noise).  model=True adds g_model_solver
        and g_model_plant (B,3): dL/d(L1, L2, M) per instance of the geometry the controller believes and of the
        plant's; the step stays four launches (the model instantiations of the plant and solve adjoints, the solve's
        term accumulated in place).  Raises if the solver's or the plant's geometry is no longer that of the tape.
        The tape of a loop with a ``FuzzyRule``: each step's weights were w_t = rule(x_meas_t, xref_t[0]), so the window
        launch also rebuilds x_meas_t, the solve adjoint runs at tape.W[t], and the fourth launch is
        tt_sim_window_vjp_fuzzy_device, which sends the solve's dL/dw_t through the rule's adjoint into the state
        adjoint (and the measurement-noise gradient) unless the step took the unit-weight retry: still four launches.
        g_wq_wr is then the sum over the steps of dL/dW_t, the gradient for a constant offset added to every step's
        weights.  rule=True adds g_fuzzy_rule (B,7): dL/dtheta per instance.  Raises if the loop's rule is no longer the
        tape's.
        The tape of a switch loop (``switch_adjoint=True``): the step's tracking adjoint runs on a copy of the statuses
        in which the switched instances carry TT_MAX_ITER, so it writes zeros for them (and nothing into g_wq_wr);
        tt_obca_vjp_device then runs on the taped iterates of the compacted set with the gathered dL/dU, and its g_x0,
        g_xref, g_uref take those rows before the window adjoint.  The compaction sizes are the tape's: no host
        synchronisation.  model=True and rule=True raise on such a loop (it has three geometries: geometry=True below
        returns them; the rule's adjoint is not carried through the switch solve).
        scene=True (a switch loop with ``switch_adjoint=True`` only, else it raises) adds g_obstacles (B,M,4) and g_dmin
        (B,): dL/d(cx, cy, w, h) and dL/dd_min of the switch solver's scene per instance, accumulated over the switched
        instance-steps from the same compacted adjoint call, which is then tt_obca_vjp_params_device (its g_x0, g_xref,
        g_uref agree with the plain call's to rounding).  The switch solver's scene must still be the run's.  The
        collision switch itself is piecewise constant in the scene and contributes nothing: the gradient holds while no
        flag changes.  No host synchronisation is added.  With per-instance scenes (``ClosedLoop(obstacles=(B,M,4))`` and
        / or ``d_min=``) the compacted adjoint gets the rows its solve got, and g_obstacles / g_dmin are each instance's
        gradient in its own scene.
        geometry=True (a switch loop with ``switch_adjoint=True`` only, else it raises) adds g_geometry_switch (B,5):
        dL/d(L1, L2, M, W1, W2) of the switch solver's geometry per instance, accumulated over the switched
        instance-steps from the same compacted adjoint call (then tt_obca_vjp_geometry_device), and g_model_solver and
        g_model_plant (B,3) of the tracking solver's and the plant's (L1, L2, M) as model=True forms them on a loop
        without a switch; the switched instances, masked in the tracking adjoint, add nothing to g_model_solver.  The
        three geometries are separate inputs: a loop that shares one sums them.  The switch solver's geometry must still
        be the run's.  The collision switch is piecewise constant in the geometry too.  No host synchronisation is
        added.
        bounds=True adds g_bounds (B,16): dL/d(xlb 6, ulb 2, xub 6, uub 2) per instance of the tracking solver's box,
        accumulated over the steps by the step's one solve adjoint (then tt_track_vjp_bounds_device, beside g_model
        with model=True): the step stays four launches.  The box enters the loop only through the solves (the plant
        does not clip).  The same loops as model=True: all three policies and a loop with a ``FuzzyRule``; a switch
        loop raises (the MPC+OBCA solver's box is not differentiated).  Raises if the solver's box is no longer the
        tape's, with or without bounds=True."""
        if self.switch is not None and bounds:
            raise ValueError("a switch (OBCA) loop has no bounds=True gradient: the box of the MPC+OBCA solver is not "
                             "differentiated")
        self._check_differentiable()
        if scene and (self.switch is None or not self.switch_adjoint):
            raise ValueError("scene=True needs a switch loop: ClosedLoop(..., switch_solver=..., switch_adjoint=True)")
        if geometry and (self.switch is None or not self.switch_adjoint):
            raise ValueError("geometry=True needs a switch loop: ClosedLoop(..., switch_solver=..., switch_adjoint=True)")
        if self.switch is not None and (model or rule):
            raise ValueError("a switch (OBCA) loop has no model=True or rule=True gradient: the OBCA adjoint "
                             "(switch_adjoint) gives dL/d(x_init, xref, uref) only")
        if tape.bounds is not None and not all(np.array_equal(a, b) for a, b in zip(tape.bounds,
                                                                                     self.solver.get_bounds())):
            raise ValueError("the solver's bounds changed since the tape was made; run the tape again, or set the "
                             "bounds back before the backward")
        if tape.rule != self.rule:
            raise ValueError(f"the fuzzy rule changed since the tape was made: {tape.rule} -> {self.rule}; run the tape "
                             "again, or set the rule back before the backward")
        if rule and tape.rule is None:
            raise ValueError("rule=True needs the tape of a loop with a fuzzy_rule")
        if tape.model_solver is not None and (tape.model_solver != self.solver.model() or
                                              tape.model_plant != self.plant_model()):
            raise ValueError(f"the geometry changed since the tape was made: solver {tape.model_solver} -> "
                             f"{self.solver.model()}, plant {tape.model_plant} -> {self.plant_model()}; run the tape "
                             "again, or set the geometry back before the backward")
        if tape.geometry_switch is not None and tape.geometry_switch != self.switch.geometry():
            raise ValueError(f"the switch solver's geometry changed since the tape was made: {tape.geometry_switch} -> "
                             f"{self.switch.geometry()}; run the tape again, or set the geometry back before the "
                             "backward")
        mdl = model or geometry   # (the model instantiations of the plant and tracking adjoints)
        s, d, N = self.stream, self.dev, self.N
        K, B = tape.status.shape
        Np = tape.plan_u.shape[-2]
        check_tensor("GS", GS, (K + 1, B, 6), d)
        check_tensor("GU", GU, (K, B, 2), d)
        GS, GU = GS.contiguous(), GU.contiguous()
        z = lambda *sh: torch.zeros(sh, dtype=torch.float64, device=d)  # noqa: E731
        a, abar, gU = GS[K].clone(), z(B, 2), z(B, N, 2)
        g_w, g_px, g_pu, g_n = z(B, 8), z(B, Np + 1, 6), z(B, Np, 2), z(K, B, 6)
        xref, uref = z(B, N + 1, 6), z(B, N, 2)
        g_x0, g_xr, g_ur, g_ws = z(B, 6), z(B, N + 1, 6), z(B, N, 2), z(B, 8)
        g_ms, g_mp = (z(B, 3), z(B, 3)) if mdl else (None, None)
        g_bd = z(B, 16) if bounds else None
        fz = tape.rule is not None
        g_th = z(B, 7) if rule else None
        x_meas = z(B, 6) if fz else None
        g_ob, g_dm = (z(B, self.switch.M, 4), z(B)) if scene else (None, None)
        g_ge = z(B, 5) if geometry else None
        wbytes = self.switch.vjp_params_work_bytes() if scene or geometry else 0
        rs = _rule_ref(tape.rule)
        in_plant = self.noise_in_plant and tape.noise is not None
        meas = self.measurement_noise and tape.noise is not None
        # the raw entries, not the module-level wrappers: a backward step is four short launches the host only just
        # keeps ahead of, and the wrappers' per-call tt_plant and stream lookups cost it about 1 %
        L, p, sp = lib(), plant(self.params, self.dist), C.c_void_p(s.cuda_stream)
        per = int(tape.plan_x.shape[0] != 1)
        wq = 0 if tape.wq_wr is None else tape.wq_wr.data_ptr()
        # Chosen once per run: the plant adjoint and the window adjoint each come in a plain and a wider form, and a run
        # calls the form it needs (marshalling the wider argument lists costs about 1.5 us per step, which the plain
        # loop must not pay).  at(t): what a rule loop adds per step, ((state, noise) of the window launch that rebuilds
        # x_meas, the weights the solve used, the tail of the window adjoint).
        plant_vjp, plant_tail = ((L.tt_policy_plant_vjp_model_device, (g_mp.data_ptr(), sp)) if mdl else
                                 (L.tt_policy_plant_vjp_device, (sp,)))
        g_model = g_ms.data_ptr() if mdl else 0
        g_bounds = g_bd.data_ptr() if bounds else 0
        if fz:
            # the rule's four extra per-step addresses by offset: a tape slice made on the host costs it more than the
            # launch it feeds, and the host only just keeps ahead of a backward step
            if not all(t.is_contiguous() for t in (tape.S, tape.W, tape.retried) + ((tape.noise,) if meas else ())):
                raise ValueError("the tape's S, W, retried and noise must be contiguous")
            S0, W0, R0 = tape.S.data_ptr(), tape.W.data_ptr(), tape.retried.data_ptr()
            N0 = tape.noise.data_ptr() if meas else None
            win_vjp, head = L.tt_sim_window_vjp_fuzzy_device, (rs, x_meas.data_ptr(), xref.data_ptr())
            at = lambda t: ((S0 + t * B * 48, N0 + t * B * 48 if meas else None), W0 + t * B * 64,  # noqa: E731
                            (*head, R0 + t * B * 4, _ptr(g_th), sp))
        else:
            win_vjp, plain = L.tt_sim_window_vjp_device, ((None, None), wq, (sp,))
            at = lambda t: plain  # noqa: E731
        plant_name, win_name = plant_vjp.__name__, win_vjp.__name__
        s.wait_stream(torch.cuda.current_stream(d))
        sw, status = tape.switched or [None] * K, [tape.status[t] for t in range(K)]
        with torch.cuda.stream(s):
            for t in range(K):   # the tracking adjoint skips the switched instances
                if sw[t] is not None:
                    status[t] = tape.status[t].clone()
                    status[t][sw[t][0]] = TT_MAX_ITER
        for t in range(K - 1, -1, -1):
            meas_in, w_t, win_tail = at(t)
            _check(plant_vjp(B, N, C.byref(p), POLICIES[self.policy], tape.S[t].data_ptr(), tape.status[t].data_ptr(),
                             None if t == 0 else tape.active[t - 1].data_ptr(), tape.active[t].data_ptr(),
                             tape.consec[t].data_ptr(), GU[t].data_ptr(), a.data_ptr(), abar.data_ptr(), gU.data_ptr(),
                             g_n[t].data_ptr() if in_plant else None, *plant_tail), plant_name)
            _check(L.tt_sim_window_device(B, N, int(tape.ks[t]), int(Np), tape.plan_x.data_ptr(),
                                          tape.plan_u.data_ptr(), per, *meas_in, _ptr(x_meas), xref.data_ptr(),
                                          uref.data_ptr(), sp),
                   "tt_sim_window_device")
            self.solver.vjp_device(B, tape.X[t].data_ptr(), tape.U[t].data_ptr(), tape.dual[t].data_ptr(),
                                   xref.data_ptr(), uref.data_ptr(), status[t].data_ptr(), grad_u=gU.data_ptr(),
                                   g_x0=g_x0.data_ptr(), g_xref=g_xr.data_ptr(), g_uref=g_ur.data_ptr(),
                                   g_wq_wr=g_ws.data_ptr(), wq_wr=w_t, stream=s.cuda_stream, g_model=g_model,
                                   accumulate=True, g_bounds=g_bounds)
            if sw[t] is not None:
                idx, it_c, st_c = sw[t]
                n = int(idx.shape[0])
                with torch.cuda.stream(s):
                    gu_c = gU[idx].contiguous()
                    o0, oxr, our = z(n, 6), z(n, N + 1, 6), z(n, N, 2)
                    # per-instance scenes: the adjoint gets the rows the switch solve got
                    ob_c, dm_c = self._scene_rows(idx) if self.per_scene or self.d_min is not None else (None, None)
                    rows = (dict(obstacles=_ptr(ob_c) or 0, d_min=_ptr(dm_c) or 0)
                            if ob_c is not None or dm_c is not None else {})
                    if scene or geometry:  # (idx has no repeats: the indexed += is one add per row)
                        oob, odm = (z(n, self.switch.M, 4), z(n)) if scene else (None, None)
                        oge = z(n, 5) if geometry else None
                        work = torch.empty((n * wbytes // 8,), dtype=torch.float64, device=d)
                        self.switch.vjp_device(n, it_c.data_ptr(), st_c.data_ptr(), grad_u=gu_c.data_ptr(),
                                               g_x0=o0.data_ptr(), g_xref=oxr.data_ptr(), g_uref=our.data_ptr(),
                                               g_obstacles=_ptr(oob) or 0, g_dmin=_ptr(odm) or 0, work=work.data_ptr(),
                                               g_geometry=_ptr(oge) or 0, stream=s.cuda_stream, **rows)
                        if scene:
                            g_ob[idx] += oob
                            g_dm[idx] += odm
                        if geometry:
                            g_ge[idx] += oge
                    else:
                        self.switch.vjp_device(n, it_c.data_ptr(), st_c.data_ptr(), grad_u=gu_c.data_ptr(),
                                               g_x0=o0.data_ptr(), g_xref=oxr.data_ptr(), g_uref=our.data_ptr(),
                                               stream=s.cuda_stream, **rows)
                    g_x0[idx], g_xr[idx], g_ur[idx] = o0, oxr, our
            _check(win_vjp(B, N, int(tape.ks[t]), int(Np), g_xr.data_ptr(), g_ur.data_ptr(), g_px.data_ptr(),
                           g_pu.data_ptr(), g_x0.data_ptr(), GS[t].data_ptr(), a.data_ptr(), g_ws.data_ptr(),
                           g_w.data_ptr(), g_n[t].data_ptr() if meas else None, *win_tail), win_name)
        with torch.cuda.stream(s):
            if not per:
                g_px, g_pu = g_px.sum(dim=0, keepdim=True), g_pu.sum(dim=0, keepdim=True)
        torch.cuda.current_stream(d).wait_stream(s)
        out = {"g_x_init": a, "g_wq_wr": g_w, "g_plan_x": g_px, "g_plan_u": g_pu, "g_noise": g_n}
        if mdl:
            out.update(g_model_solver=g_ms, g_model_plant=g_mp)
        if geometry:
            out["g_geometry_switch"] = g_ge
        if bounds:
            out["g_bounds"] = g_bd
        if rule:
            out["g_fuzzy_rule"] = g_th
        if scene:
            out.update(g_obstacles=g_ob, g_dmin=g_dm)
        return out

    def _policy_logs(self):
        """failure_count / consecutive_failures of the reference drivers, per instance, and whether the
        instance is still running (False = stopped by the policy)."""
        return {"failures": self.fails.cpu().numpy(), "consecutive_failures": self.consec.cpu().numpy(),
                "running": self.active.cpu().numpy().astype(bool)}
