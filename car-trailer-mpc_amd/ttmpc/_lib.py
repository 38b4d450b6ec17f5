"""ctypes binding of libttmpc.so (the C ABI in include/ttmpc.h).

The product path is GPU-only: if the library is missing or no gfx950 device is usable, every
entry point raises -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import warnings
from pathlib import Path

import numpy as np

LIB_PATH = Path(__file__).resolve().parent / "libttmpc.so"
# diagnostics only (A/B timing of two builds in one GPU session): TTMPC_LIB=<path to another build>
if os.environ.get("TTMPC_LIB"):
    LIB_PATH = Path(os.environ["TTMPC_LIB"]).resolve()

TT_CONVERGED, TT_ACCEPTABLE, TT_MAX_ITER, TT_INFEASIBLE, TT_NONFINITE, TT_STEP_FAILED, TT_HANDOFF_TIMEOUT = range(7)
TT_VARIANT_TRACK, TT_VARIANT_TRACK_OBCA, TT_VARIANT_NMPC, TT_VARIANT_FUZZY, TT_VARIANT_OBCA_PLAN = range(5)
STATUS_NAMES = {0: "converged", 1: "acceptable", 2: "max_iter", 3: "infeasible", 4: "non-finite", 5: "step_failed",
                6: "handoff_timeout"}


class TTConfig(C.Structure):
    _fields_ = [("nx", C.c_int), ("nu", C.c_int), ("N", C.c_int), ("M", C.c_int),
                ("dt", C.c_double), ("L1", C.c_double), ("L2", C.c_double), ("Mh", C.c_double),
                ("W1", C.c_double), ("W2", C.c_double), ("variant", C.c_int),
                ("tol", C.c_double), ("acc_tol", C.c_double), ("max_iter", C.c_int), ("acc_iter", C.c_int),
                ("warm_shift_compat", C.c_int), ("dual_init", C.c_int)]


class TTPlant(C.Structure):
    """tt_plant (include/ttmpc.h): params + DISTURBANCE_PARAMS of simulation.py:26-32, 391-397."""
    _fields_ = [("dt", C.c_double), ("L1", C.c_double), ("L2", C.c_double), ("Mh", C.c_double),
                ("W1", C.c_double), ("W2", C.c_double), ("enable", C.c_int), ("friction_coeff", C.c_double),
                ("slippage_coeff", C.c_double), ("process_noise_std", C.c_double),
                ("lateral_slip_gain", C.c_double), ("slip_angle_max", C.c_double)]


class TTFuzzyRule(C.Structure):
    """tt_fuzzy_rule (include/ttmpc.h): the constants of mpc_control_fuzzy.py:90-119; the first seven are theta."""
    _fields_ = [(k, C.c_double) for k in ("psi_full", "gain_hitch", "gain_steer", "gain_rate", "rev_hitch", "rev_steer",
                                          "rev_rate", "w_min", "w_max", "v_rev")]


class TTTrackExtra(C.Structure):
    """tt_track_extra (include/ttmpc.h): the optional outputs of tt_solve_batch_ex*; NULL members are skipped."""
    _fields_ = [("dual", C.c_void_p), ("gain", C.c_void_p), ("dxdx0", C.c_void_p), ("dudx0", C.c_void_p),
                ("sens_status", C.c_void_p)]


class TTTrackVjpOut(C.Structure):
    """tt_track_vjp_out (include/ttmpc.h): the outputs of tt_track_vjp*; NULL members are skipped."""
    _fields_ = [("g_x0", C.c_void_p), ("g_xref", C.c_void_p), ("g_uref", C.c_void_p), ("g_wq_wr", C.c_void_p),
                ("vjp_status", C.c_void_p)]


class TTTrackVjpModelOut(C.Structure):
    """tt_track_vjp_model_out (include/ttmpc.h): tt_track_vjp_out with g_model [B][3] before vjp_status."""
    _fields_ = [("g_x0", C.c_void_p), ("g_xref", C.c_void_p), ("g_uref", C.c_void_p), ("g_wq_wr", C.c_void_p),
                ("g_model", C.c_void_p), ("vjp_status", C.c_void_p)]


class TTTrackVjpBoundsOut(C.Structure):
    """tt_track_vjp_bounds_out (include/ttmpc.h): tt_track_vjp_model_out with g_bounds [B][16] before vjp_status."""
    _fields_ = [("g_x0", C.c_void_p), ("g_xref", C.c_void_p), ("g_uref", C.c_void_p), ("g_wq_wr", C.c_void_p),
                ("g_model", C.c_void_p), ("g_bounds", C.c_void_p), ("vjp_status", C.c_void_p)]


class TTObcaVjpOut(C.Structure):
    """tt_obca_vjp_out (include/ttmpc.h): the outputs of tt_obca_vjp*; NULL members are skipped."""
    _fields_ = [("g_x0", C.c_void_p), ("g_xref", C.c_void_p), ("g_uref", C.c_void_p), ("vjp_status", C.c_void_p)]


class TTObcaVjpParamsOut(C.Structure):
    """tt_obca_vjp_params_out (include/ttmpc.h): tt_obca_vjp_out and the scene and weight gradients behind it."""
    _fields_ = TTObcaVjpOut._fields_ + [("g_obstacles", C.c_void_p), ("g_dmin", C.c_void_p), ("g_Q", C.c_void_p),
                                        ("g_R", C.c_void_p)]


class TTObcaVjpGeometryOut(C.Structure):
    """tt_obca_vjp_geometry_out (include/ttmpc.h): tt_obca_vjp_params_out and g_geometry [B][5] behind it."""
    _fields_ = TTObcaVjpParamsOut._fields_ + [("g_geometry", C.c_void_p)]


class TTObcaScenes(C.Structure):
    """tt_obca_scenes (include/ttmpc.h): per-instance obstacles [B][M][4] and d_min [B]; a NULL member = the handle's."""
    _fields_ = [("obstacles", C.c_void_p), ("d_min", C.c_void_p)]


class TTLqrVjpOut(C.Structure):
    """tt_lqr_vjp_out (include/ttmpc.h): the outputs of tt_lqr_score_vjp_device; NULL members are skipped."""
    _fields_ = [("g_x_cur", C.c_void_p), ("g_x_goal", C.c_void_p), ("g_Q", C.c_void_p), ("g_R", C.c_void_p),
                ("vjp_status", C.c_void_p), ("iters", C.c_void_p)]


class TTError(RuntimeError):
    pass


class _BoundsGradient:
    """g_bounds of a ``TrackVjpResult`` and its four views.  A slot of its own: ``TrackVjpResult.__slots__`` stays the
    list of what every ``vjp`` call fills."""
    __slots__ = ("g_bounds",)

    def _part(self, lo, hi):
        return None if self.g_bounds is None else self.g_bounds[:, lo:hi]

    g_xlb = property(lambda self: self._part(0, 6))
    g_ulb = property(lambda self: self._part(6, 8))
    g_xub = property(lambda self: self._part(8, 14))
    g_uub = property(lambda self: self._part(14, 16))


class TrackVjpResult(_BoundsGradient):
    """What ``BatchSolver.vjp`` returns: g_x0 (B,6) = dL/dx0, g_xref (B,N+1,6), g_uref (B,N,2), g_wq_wr (B,8) and
    vjp_status (B,) (0 ok, 1 undefined, 2 solve not successful; the gradients of a failed instance are zeros); with
    ``model=True`` also g_model (B,3) = dL/d(L1, L2, M) per instance, else None.  ``r["model"]``, ``r["x0"]``,
    ``r["xref"]``, ``r["uref"]``, ``r["w"]`` read the gradients by the names of the inputs.  With ``bounds=True`` also
    g_bounds (B,16) = dL/d(xlb 6, ulb 2, xub 6, uub 2) per instance (``r["bounds"]``), else None; g_xlb (B,6), g_ulb
    (B,2), g_xub (B,6) and g_uub (B,2) are views of it."""
    __slots__ = ("g_x0", "g_xref", "g_uref", "g_wq_wr", "g_model", "vjp_status")

    def __init__(self, **kw):
        for k in self.__slots__ + _BoundsGradient.__slots__:
            setattr(self, k, kw.get(k))

    def __getitem__(self, key):
        return getattr(self, {"model": "g_model", "x0": "g_x0", "xref": "g_xref", "uref": "g_uref", "w": "g_wq_wr",
                              "bounds": "g_bounds", "vjp_status": "vjp_status"}[key])


TrackVjpModelResult = TrackVjpResult


class ObcaVjpParamsResult:
    """What ``ObcaSolver.vjp(..., params=True)`` returns: g_x0, g_xref, g_uref and vjp_status as ``TrackVjpResult``,
    and g_obstacles (B,M,4) = dL/d(cx, cy, w, h), g_dmin (B,), g_Q (B,6,6) and g_R (B,2,2) (None without xref / uref),
    all per instance; the arrays of a failed instance are zeros.  With ``geometry=True`` also g_geometry (B,5) =
    dL/d(L1, L2, M, W1, W2) per instance, else None."""
    __slots__ = ("g_x0", "g_xref", "g_uref", "vjp_status", "g_obstacles", "g_dmin", "g_Q", "g_R", "g_geometry")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


class TrackExResult:
    """What ``BatchSolver.solve_ex`` returns: the plain outputs X (B,N+1,6), U (B,N,2), status, iters, kkt and, where
    asked for (else None), dual (B,N+1,22: y 6 | z_L 8 | z_U 8 per stage), gain (B,2,6) = du_0/dx_init,
    dXdx0 (B,N+1,6,6), dUdx0 (B,N,2,6) and sens_status (B,) (0 ok, 1 undefined, 2 solve not successful)."""
    __slots__ = ("X", "U", "status", "iters", "kkt", "dual", "gain", "dXdx0", "dUdx0", "sens_status")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))


_lib = None
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


def _share_torch_hip_runtime():
    """If PyTorch-ROCm is installed, pre-load ITS libamdhip64.so (SONAME libamdhip64.so.7) so that
    libttmpc.so binds to the same HIP runtime torch uses.  Two HIP runtimes in one process do not
    coexist (torch then reports no GPU), and torch tensors / streams must be valid for our kernel.
    Set TTMPC_HIP_RUNTIME=system to use /opt/rocm's runtime instead."""
    if os.environ.get("TTMPC_HIP_RUNTIME", "") == "system":
        return
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return
    hip = Path(list(spec.submodule_search_locations)[0]) / "lib" / "libamdhip64.so"
    if hip.exists():
        C.CDLL(str(hip), mode=C.RTLD_GLOBAL)


def lib():
    """Load libttmpc.so (raises if it was not built: run ``make -C car-trailer-mpc_amd``)."""
    global _lib
    if _lib is not None:
        return _lib
    _share_torch_hip_runtime()
    if not LIB_PATH.exists():
        raise TTError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
                      " (ttmpc is GPU-only; there is no CPU fallback)")
    L = C.CDLL(str(LIB_PATH))
    for name, (argtypes, restype) in _SIGNATURES.items():
        if os.environ.get("TTMPC_LIB") and not hasattr(L, name):
            continue  # A/B diagnostics against an older build (otherwise a missing name is an error)
        fn = getattr(L, name)
        fn.argtypes = argtypes
        fn.restype = restype
    _lib = L
    return L


def _signatures():
    """name -> (argtypes, restype) of every entry ``lib()`` binds: include/ttmpc.h, then the ttx_* diagnostics."""
    vp, i, ll, d, dp, ip, P = C.c_void_p, C.c_int, C.c_longlong, C.c_double, _dp, _ip, C.POINTER
    plant, rule = P(TTPlant), P(TTFuzzyRule)
    track_in = [vp, i, dp, dp, dp, dp, dp]          # handle, B, x0, xref, uref, wq_wr, z_guess
    track_vjp = [vp, i, dp, dp, dp, dp, dp, dp, ip, dp, dp]
    obca_in = [vp, i, dp, dp, dp, dp, dp]           # handle, B, x0, xgoal, xref, uref, z_guess
    obca_out = [dp, dp, dp, ip, ip, dp]             # X, U, z, status, iters, kkt
    # the out-struct of the OBCA adjoint entries goes as a plain address: tt_obca_vjp_out and tt_obca_vjp_params_out
    # are prefixes of tt_obca_vjp_geometry_out, so one TTObcaVjpGeometryOut serves all eight
    obca_vjp = [vp, i, dp, ip, dp, dp, dp, dp, vp]  # handle, B, iterate, status, xref, uref, grad_x, grad_u, out
    scenes = P(TTObcaScenes)
    ints = {  # the entries that return an int; the others follow
        "tt_create": [P(TTConfig), dp, dp, dp, dp, dp, dp, dp, i, P(vp)],
        "tt_solve_batch": track_in + [dp, dp, ip, ip, dp],
        "tt_solve_batch_device": [vp, i] + [vp] * 11,
        "tt_solve_batch_ex": track_in + [dp, dp, ip, ip, dp, P(TTTrackExtra)],
        "tt_solve_batch_ex_device": [vp, i] + [vp] * 10 + [P(TTTrackExtra), vp],
        "tt_track_sens_device": [vp, i] + [vp] * 10,
        "tt_track_vjp_device": [vp, i] + [vp] * 9 + [P(TTTrackVjpOut), vp],
        "tt_track_vjp": track_vjp + [P(TTTrackVjpOut)],
        "tt_track_vjp_model_device": [vp, i] + [vp] * 9 + [P(TTTrackVjpModelOut), i, vp],
        "tt_track_vjp_model": track_vjp + [P(TTTrackVjpModelOut), i],
        "tt_set_model": [vp, d, d, d],
        "tt_get_model": [vp, dp, dp, dp],
        "tt_track_vjp_bounds_device": [vp, i] + [vp] * 9 + [P(TTTrackVjpBoundsOut), i, vp],
        "tt_track_vjp_bounds": track_vjp + [P(TTTrackVjpBoundsOut), i],
        "tt_set_bounds": [vp, dp, dp, dp, dp],
        "tt_get_bounds": [vp, dp, dp, dp, dp],
        "tt_plan_batch": [vp, i, dp, dp, dp, dp, dp, ip, ip],
        "tt_obca_solve_batch": obca_in + obca_out,
        "tt_obca_solve_batch_device": [vp, i] + [vp] * 12,
        "tt_obca_solve_batch_iterate": obca_in + obca_out + [dp],
        "tt_obca_solve_batch_iterate_device": [vp, i] + [vp] * 13,
        "tt_obca_solve_batch_scenes": obca_in + obca_out + [dp, scenes],
        "tt_obca_solve_batch_scenes_device": [vp, i] + [vp] * 12 + [scenes, vp],
        "tt_obca_vjp": [vp, i, dp, ip, dp, dp, vp],
        "tt_obca_vjp_device": [vp, i] + [vp] * 4 + [vp, vp],
        "tt_obca_vjp_params": obca_vjp,
        "tt_obca_vjp_params_device": [vp, i] + [vp] * 6 + [vp, vp, vp],
        "tt_obca_vjp_scenes": obca_vjp + [scenes],
        "tt_obca_vjp_scenes_device": [vp, i] + [vp] * 6 + [vp, vp, scenes, vp],
        "tt_obca_vjp_geometry": obca_vjp + [scenes],
        "tt_obca_vjp_geometry_device": [vp, i] + [vp] * 6 + [vp, vp, scenes, vp],
        "tt_set_scene": [vp, dp, dp],
        "tt_get_scene": [vp, dp, dp],
        "tt_set_geometry": [vp] + [d] * 5,
        "tt_get_geometry": [vp] + [dp] * 5,
        "tt_lds_bytes": [i],
        "tt_max_horizon": [],
        "tt_sim_window_device": [i, i, i, i, vp, vp, i, vp, vp, vp, vp, vp, vp],
        "tt_collision_device": [i, i, vp, ll, i, vp, i, plant, vp, vp],
        "tt_collision_scenes_device": [i, i, vp, ll, i, vp, i, plant, vp, vp],
        "tt_plant_update_device": [i, plant, vp, vp, ll, vp, i, vp, vp],
        "tt_warm_start_device": [i, i, vp, vp, vp, vp, i, vp, vp],
        "tt_record_solution_device": [i, i, vp, vp, vp, vp, vp, vp],
        "tt_interpolate_device": [i, i, i, vp, vp, vp, vp, vp],
        "tt_lqr_score_device": [i, plant, dp, dp, vp, vp, vp, vp, vp, vp, vp],
        "tt_sim_window_indexed_device": [i, i, vp, vp, i, vp, vp, i, vp, vp, vp, vp, vp, vp],
        "tt_sim_log_advance_device": [i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "tt_policy_plant_device": [i, plant, i, vp, vp, ll, vp, vp, vp, vp, vp, vp, vp],
        "tt_plant_update_noise_device": [i, plant, vp, vp, ll, vp, i, vp, vp, vp],
        "tt_policy_plant_noise_device": [i, plant, i, vp, vp, ll, vp, vp, vp, vp, vp, vp, vp, vp],
        "tt_fuzzy_weights_device": [i, i, vp, vp, vp, vp],
        "tt_policy_plant_vjp_device": [i, i, plant, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "tt_policy_plant_vjp_model_device": [i, i, plant, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "tt_sim_window_vjp_device": [i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp],
        "tt_fuzzy_weights_rule_device": [i, i, rule, vp, vp, vp, vp],
        "tt_fuzzy_weights_vjp_device": [i, i, rule, vp, vp, vp, vp, vp, vp, vp],
        "tt_sim_window_vjp_fuzzy_device": [i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, rule, vp, vp, vp, vp, vp],
        "tt_lqr_score_vjp_device": [i, plant, dp, vp, vp, vp, vp, vp, vp, P(TTLqrVjpOut), vp],
        "ttx_obca_set_helpers": [vp, i],  # diagnostics (not in include/ttmpc.h)
        "ttx_obca_set_handoff_debug": [vp, ll, i],
    }
    sigs = {name: (args, i) for name, args in ints.items()}
    sigs.update({"tt_track_dual_len": ([i], ll), "tt_obca_iterate_len": ([i, i], ll),
                 "tt_obca_vjp_params_work_bytes": ([i, i], ll), "tt_obca_n": ([i, i], ll),
                 "tt_obca_workspace_bytes": ([i, i], ll), "tt_destroy": ([vp], None),
                 "tt_last_error": ([vp], C.c_char_p), "tt_version": ([], C.c_char_p)})
    return sigs


_SIGNATURES = _signatures()
EXPORTED_SYMBOLS = tuple(name for name in _SIGNATURES if not name.startswith("ttx_"))  # (tests/test_abi.py)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _f64(a, shape=None):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if shape is not None:
        a = a.reshape(shape)
    return a


def _bounds(v, n):
    v = _f64(v).reshape(-1)
    if v.size != n:
        raise ValueError(f"bound vector must have {n} entries, got {v.size}")
    return v


def default_device() -> int:
    for key in ("TTMPC_DEVICE", "LOCAL_RANK"):
        if key in os.environ:
            return int(os.environ[key])
    return 0


class _Solver:
    """What the two solver classes share: the library handle made from a config, its release and its error text."""

    def __init__(self, N, params, W1, W2, Q, R, xlb, xub, ulb, uub, obstacles, variant, tol, acc_tol, max_iter,
                 acc_iter, dual_init, device):
        cfg = TTConfig()
        cfg.nx, cfg.nu, cfg.N, cfg.M = 6, 2, int(N), 0 if obstacles is None else int(obstacles.shape[0])
        cfg.dt, cfg.L1, cfg.L2, cfg.Mh = float(params["dt"]), float(params["L1"]), float(params["L2"]), float(params["M"])
        cfg.W1, cfg.W2 = float(W1), float(W2)
        cfg.variant = int(variant)
        cfg.tol, cfg.acc_tol, cfg.max_iter, cfg.acc_iter = float(tol), float(acc_tol), int(max_iter), int(acc_iter)
        cfg.warm_shift_compat = 0
        cfg.dual_init = int(bool(dual_init))
        self.N = int(N)
        self.variant = int(variant)
        self.Q = _f64(Q, (6, 6))
        self.R = _f64(R, (2, 2))
        self.bounds = tuple(_bounds(b, n) for b, n in ((xlb, 6), (xub, 6), (ulb, 2), (uub, 2)))
        self.device = default_device() if device is None else int(device)
        h = C.c_void_p()
        L = lib()
        rc = L.tt_create(C.byref(cfg), _ptr(self.Q), _ptr(self.R), *[_ptr(b) for b in self.bounds], _ptr(obstacles),
                         self.device, C.byref(h))
        if rc != 0:
            raise TTError(f"tt_create failed ({rc}): {L.tt_last_error(None).decode()}")
        self._h = h
        self._L = L

    def close(self):
        if getattr(self, "_h", None):
            self._L.tt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    def _err(self, rc, what):
        raise TTError(f"{what} failed ({rc}): {self._L.tt_last_error(self._h).decode()}")


def _track_inputs(N, x0, xref, uref, wq_wr, z_guess):
    """B and the contiguous float64 inputs of a tracking host call: (B, x0, xref, uref, wq_wr|None, z_guess|None)."""
    x0 = _f64(x0)
    B = x0.shape[0] if x0.ndim == 2 else 1
    return (B, x0.reshape(B, 6), _f64(xref, (B, N + 1, 6)), _f64(uref, (B, N, 2)),
            None if wq_wr is None else _f64(wq_wr, (B, 8)), None if z_guess is None else _f64(z_guess, (B, 8 * N + 6)))


class BatchSolver(_Solver):
    """One library handle = one compiled NLP (the reference's CasADi ``nlpsol`` object) on one GPU."""

    def __init__(self, N, params, Q, R, xlb, xub, ulb, uub, variant=TT_VARIANT_TRACK, tol=0.0, acc_tol=0.0,
                 max_iter=0, acc_iter=0, device=None):
        super().__init__(N, params, params.get("W1", 0.0), params.get("W2", 0.0), Q, R, xlb, xub, ulb, uub, None,
                         variant, tol, acc_tol, max_iter, acc_iter, False, device)

    # Small host calls (the reference's one-instance-per-step controllers) reuse per-shape arrays whose ctypes pointers
    # were made once: building ten pointers per call cost more wall clock than the copies they avoid.
    _SMALL_B = 64

    def _small_call(self, B, x0, xref, uref, wq_wr, z_guess):
        N = self.N
        ins = [(x0, (B, 6), B * 6), (xref, (B, N + 1, 6), B * (N + 1) * 6), (uref, (B, N, 2), B * N * 2)]
        if wq_wr is not None:
            ins.append((wq_wr, (B, 8), B * 8))
        if z_guess is not None:
            ins.append((z_guess, (B, 8 * N + 6), B * (8 * N + 6)))
        arrs = []
        for a, _, n in ins:
            a = np.asarray(a, dtype=np.float64)
            if a.size != n:
                return None  # the general path raises the shape error
            arrs.append(a)
        key = (B, wq_wr is not None, z_guess is not None)
        cache = self.__dict__.setdefault("_small", {})
        ent = cache.get(key)
        if ent is None:
            if len(cache) >= 8:
                cache.clear()
            bufs = [np.empty(shp) for _, shp, _ in ins]
            outs = (np.empty((B, N + 1, 6)), np.empty((B, N, 2)), np.empty(B, dtype=np.int32),
                    np.empty(B, dtype=np.int32), np.empty(B))
            p = [_ptr(b) for b in bufs[:3]]
            p += [_ptr(bufs[3]) if wq_wr is not None else None]
            p += [_ptr(bufs[-1]) if z_guess is not None else None]
            p += [_ptr(outs[0]), _ptr(outs[1]), outs[2].ctypes.data_as(_ip), outs[3].ctypes.data_as(_ip), _ptr(outs[4])]
            ent = cache[key] = (bufs, outs, tuple(p))
        bufs, outs, p = ent
        for b, a in zip(bufs, arrs):
            np.copyto(b, a.reshape(b.shape))
        rc = self._L.tt_solve_batch(self._h, B, *p)
        if rc != 0:
            self._err(rc, "tt_solve_batch")
        return tuple(o.copy() for o in outs)

    def solve(self, x0, xref, uref, wq_wr=None, z_guess=None):
        """Host arrays: x0 (B,6), xref (B,N+1,6), uref (B,N,2), wq_wr (B,8)|None, z_guess (B,8N+6)|None.
        Returns (X (B,N+1,6), U (B,N,2), status (B,), iters (B,), kkt (B,))."""
        N = self.N
        x0a = np.asarray(x0)
        B = x0a.shape[0] if x0a.ndim == 2 else 1
        if 0 < B <= self._SMALL_B:
            r = self._small_call(B, x0a, xref, uref, wq_wr, z_guess)
            if r is not None:
                return r
        B, x0, xref, uref, w, zg = _track_inputs(N, x0, xref, uref, wq_wr, z_guess)
        X = np.empty((B, N + 1, 6))
        U = np.empty((B, N, 2))
        st = np.empty(B, dtype=np.int32)
        it = np.empty(B, dtype=np.int32)
        kk = np.empty(B)
        rc = self._L.tt_solve_batch(self._h, B, _ptr(x0), _ptr(xref), _ptr(uref), _ptr(w), _ptr(zg), _ptr(X), _ptr(U),
                                    st.ctypes.data_as(_ip), it.ctypes.data_as(_ip), _ptr(kk))
        if rc != 0:
            self._err(rc, "tt_solve_batch")
        return X, U, st, it, kk

    def solve_device(self, B, x0, xref, uref, x_out, u_out, status, iters=0, kkt=0, wq_wr=0, z_guess=0, stream=0):
        """Device pointers (ints, e.g. torch ``tensor.data_ptr()``), enqueued on ``stream`` (int handle)."""
        rc = self._L.tt_solve_batch_device(self._h, int(B), x0, xref, uref, wq_wr or None, z_guess or None, x_out,
                                           u_out, status, iters or None, kkt or None, stream or None)
        if rc != 0:
            self._err(rc, "tt_solve_batch_device")

    def solve_ex(self, x0, xref, uref, wq_wr=None, z_guess=None, duals=True, gain=True, trajectory_sens=False):
        """``solve`` plus the multipliers and the first-order sensitivities to x0 (include/ttmpc.h, tt_solve_batch_ex).
        duals: the (B,N+1,22) multipliers; gain: du_0/dx0 (B,2,6); trajectory_sens: dX/dx0 (B,N+1,6,6) and
        dU/dx0 (B,N,2,6).  sens_status comes with either sensitivity.  Returns a ``TrackExResult``; X, U, status, iters
        and kkt are bitwise those of ``solve``."""
        N = self.N
        B, x0, xref, uref, w, zg = _track_inputs(N, x0, xref, uref, wq_wr, z_guess)
        r = TrackExResult(X=np.empty((B, N + 1, 6)), U=np.empty((B, N, 2)), status=np.empty(B, dtype=np.int32),
                          iters=np.empty(B, dtype=np.int32), kkt=np.empty(B))
        if duals:
            r.dual = np.empty((B, N + 1, 22))
        if gain:
            r.gain = np.empty((B, 2, 6))
        if trajectory_sens:
            r.dXdx0 = np.empty((B, N + 1, 6, 6))
            r.dUdx0 = np.empty((B, N, 2, 6))
        if gain or trajectory_sens:
            r.sens_status = np.empty(B, dtype=np.int32)
        ex = TTTrackExtra(*[None if a is None else a.ctypes.data for a in (r.dual, r.gain, r.dXdx0, r.dUdx0,
                                                                             r.sens_status)])
        rc = self._L.tt_solve_batch_ex(self._h, B, _ptr(x0), _ptr(xref), _ptr(uref), _ptr(w), _ptr(zg), _ptr(r.X),
                                       _ptr(r.U), r.status.ctypes.data_as(_ip), r.iters.ctypes.data_as(_ip),
                                       _ptr(r.kkt), C.byref(ex))
        if rc != 0:
            self._err(rc, "tt_solve_batch_ex")
        return r

    def solve_ex_device(self, B, x0, xref, uref, x_out, u_out, status, iters=0, kkt=0, wq_wr=0, z_guess=0, dual=0,
                        gain=0, dxdx0=0, dudx0=0, sens_status=0, stream=0):
        """``solve_device`` with the optional device outputs of tt_solve_batch_ex_device (0 = not wanted)."""
        ex = TTTrackExtra(dual or None, gain or None, dxdx0 or None, dudx0 or None, sens_status or None)
        rc = self._L.tt_solve_batch_ex_device(self._h, int(B), x0, xref, uref, wq_wr or None, z_guess or None, x_out,
                                              u_out, status, iters or None, kkt or None, C.byref(ex), stream or None)
        if rc != 0:
            self._err(rc, "tt_solve_batch_ex_device")

    def sens_device(self, B, x, u, dual, status, gain=0, dxdx0=0, dudx0=0, sens_status=0, wq_wr=0, stream=0):
        """tt_track_sens_device: the sensitivity kernel alone on device arrays of an earlier ``solve_ex_device``."""
        rc = self._L.tt_track_sens_device(self._h, int(B), x, u, dual, wq_wr or None, status, gain or None,
                                          dxdx0 or None, dudx0 or None, sens_status or None, stream or None)
        if rc != 0:
            self._err(rc, "tt_track_sens_device")

    def set_model(self, L1=None, L2=None, M=None):
        """tt_set_model: change the handle's geometry (a value left None keeps its current one).  Host-side state only:
        every later call of this solver, host or device, runs with the new values, and a solve is bitwise that of a
        fresh solver created with them.  Work already enqueued, and a captured graph, keep the old values.  Raises
        TTError for L1 or L2 <= 0 or a non-finite value."""
        cur = self.model()
        L1, L2, M = (float(c if v is None else v) for v, c in zip((L1, L2, M), cur))
        rc = self._L.tt_set_model(self._h, L1, L2, M)
        if rc != 0:
            self._err(rc, "tt_set_model")

    def model(self):
        """tt_get_model: the handle's current (L1, L2, M)."""
        if os.environ.get("TTMPC_LIB") and not hasattr(self._L, "tt_get_model"):  # (A/B against a build without it)
            return None
        v = [C.c_double() for _ in range(3)]
        rc = self._L.tt_get_model(self._h, *[C.byref(c) for c in v])
        if rc != 0:
            self._err(rc, "tt_get_model")
        return tuple(c.value for c in v)

    def set_bounds(self, xlb=None, xub=None, ulb=None, uub=None):
        """tt_set_bounds: change the handle's box (a vector left None keeps its current values; +-inf or beyond +-1e19 is
        a free bound).  Host-side state only: every later call of this solver, host or device, runs with the new box,
        and a solve is bitwise that of a fresh solver created with it, whichever build of the tracking kernel the new
        bound pattern selects.  Work already enqueued, and a captured graph, keep the old box.  Raises TTError for a
        NaN or lb > ub (nothing is changed then).  ``self.bounds`` follows."""
        new = tuple(c if v is None else _bounds(v, n) for v, c, n in zip((xlb, xub, ulb, uub), self.get_bounds(),
                                                                          (6, 6, 2, 2)))
        rc = self._L.tt_set_bounds(self._h, *[_ptr(b) for b in new])
        if rc != 0:
            self._err(rc, "tt_set_bounds")
        self.bounds = tuple(b.copy() for b in new)

    def get_bounds(self):
        """tt_get_bounds: the handle's current (xlb (6,), xub (6,), ulb (2,), uub (2,))."""
        if os.environ.get("TTMPC_LIB") and not hasattr(self._L, "tt_get_bounds"):  # (A/B against a build without it)
            return None
        out = (np.empty(6), np.empty(6), np.empty(2), np.empty(2))
        rc = self._L.tt_get_bounds(self._h, *[_ptr(b) for b in out])
        if rc != 0:
            self._err(rc, "tt_get_bounds")
        return out

    def vjp_device(self, B, x, u, dual, xref, uref, status, grad_x=0, grad_u=0, g_x0=0, g_xref=0, g_uref=0, g_wq_wr=0,
                   vjp_status=0, wq_wr=0, stream=0, g_model=0, accumulate=False, g_bounds=0):
        """tt_track_vjp_device: the adjoint kernel on device arrays of an earlier ``solve_ex_device`` (its x, u, dual,
        status, and its inputs xref, uref, wq_wr) and the upstream gradients grad_x = dL/dX, grad_u = dL/dU (0 = zeros,
        not both).  Outputs (0 = not wanted): g_x0, g_xref, g_uref, g_wq_wr, vjp_status.  Uses no buffer of the handle:
        any stream will do, behind the solve whose outputs it reads.  g_model (B,3): also dL/d(L1, L2, M) per instance,
        added to the buffer instead of written with ``accumulate``.  One call of tt_track_vjp_model_device either way:
        without g_model it launches the plain kernel instantiation, as tt_track_vjp_device does.  g_bounds (B,16): also
        dL/d(xlb 6, ulb 2, xub 6, uub 2) per instance, written or added as g_model is, from the same launch
        (tt_track_vjp_bounds_device; without it the call and its bits are the ones above)."""
        self._vjp_call(True, (int(B), x, u, dual, xref or None, uref or None, wq_wr or None, status, grad_x or None,
                              grad_u or None),
                       [p or None for p in (g_x0, g_xref, g_uref, g_wq_wr, g_model, g_bounds, vjp_status)],
                       (int(bool(accumulate)), stream or None))

    def _vjp_call(self, device, args, outs, tail):
        """The one library call behind ``vjp`` and ``vjp_device``.  outs: the seven members of tt_track_vjp_bounds_out as
        addresses (None = not wanted).  tt_track_vjp_bounds* with g_bounds, else tt_track_vjp_model*, whose out-struct
        has no such member; an error names the narrowest entry that carries what was asked for."""
        g_model, g_bounds = outs[4], outs[5]
        out = TTTrackVjpBoundsOut(*outs) if g_bounds else TTTrackVjpModelOut(*outs[:5], outs[6])
        name = "tt_track_vjp" + ("_bounds" if g_bounds else "_model") + ("_device" if device else "")
        rc = getattr(self._L, name)(self._h, *args, C.byref(out), *tail)
        if rc != 0:
            self._err(rc, name if g_bounds or g_model else name.replace("_model", ""))

    def vjp(self, x, u, dual, xref, uref, status, grad_x, grad_u, wq_wr=None, model=False, bounds=False):
        """Host arrays: the gradient of a scalar loss L(X, U) with respect to the inputs of the solve that returned
        x (B,N+1,6), u (B,N,2), dual (B,N+1,22) and status (B,) for xref, uref and wq_wr; grad_x (B,N+1,6) = dL/dX and
        grad_u (B,N,2) = dL/dU (either may be None for zeros).  Returns a ``TrackVjpResult``; with ``model=True`` it
        also has g_model (B,3) = dL/d(L1, L2, M) per instance (``r["model"]``).  One call of tt_track_vjp_model either
        way.  With ``bounds=True`` it also has g_bounds (B,16) = dL/d(xlb 6, ulb 2, xub 6, uub 2) per instance
        (``r["bounds"]``, and the views g_xlb, g_ulb, g_xub, g_uub): the call is then tt_track_vjp_bounds, the other
        outputs bitwise the same."""
        N = self.N
        x = _f64(x)
        B = x.shape[0] if x.ndim == 3 else 1
        x = x.reshape(B, N + 1, 6)
        u = _f64(u, (B, N, 2))
        dual = _f64(dual, (B, N + 1, 22))
        xref = _f64(xref, (B, N + 1, 6))
        uref = _f64(uref, (B, N, 2))
        st = np.ascontiguousarray(np.asarray(status, dtype=np.int32)).reshape(B)
        gx = None if grad_x is None else _f64(grad_x, (B, N + 1, 6))
        gu = None if grad_u is None else _f64(grad_u, (B, N, 2))
        w = None if wq_wr is None else _f64(wq_wr, (B, 8))
        r = TrackVjpResult(g_x0=np.empty((B, 6)), g_xref=np.empty((B, N + 1, 6)), g_uref=np.empty((B, N, 2)),
                           g_wq_wr=np.empty((B, 8)), g_model=np.empty((B, 3)) if model else None,
                           g_bounds=np.empty((B, 16)) if bounds else None, vjp_status=np.empty(B, dtype=np.int32))
        self._vjp_call(False, (B, _ptr(x), _ptr(u), _ptr(dual), _ptr(xref), _ptr(uref), _ptr(w), st.ctypes.data_as(_ip),
                               _ptr(gx), _ptr(gu)),
                       [None if a is None else a.ctypes.data for a in (r.g_x0, r.g_xref, r.g_uref, r.g_wq_wr, r.g_model,
                                                                       r.g_bounds, r.vjp_status)], (0,))
        return r


def obca_n(N: int, M: int) -> int:
    """Length of the reference's OBCA decision vector (trajectory_optimization.py:55-91)."""
    return N * (8 + 16 * M) + 6 + 16 * M


def _warn_handoff(st):
    """A helper hand-off timeout is a failure of the launch, not of the NLP: plan() (which by the reference's contract
    never signals failure, trajectory_optimization.py:326-331) still returns, but not silently."""
    bad = np.flatnonzero(np.asarray(st) == TT_HANDOFF_TIMEOUT)
    if bad.size:
        warnings.warn(f"OBCA helper hand-off timed out for {bad.size} instance(s) {bad[:8].tolist()}: their outputs are "
                      "partial iterates (status TT_HANDOFF_TIMEOUT)", RuntimeWarning, stacklevel=3)


class ObcaSolver(_Solver):
    """Handle for the OBCA NLPs: TT_VARIANT_OBCA_PLAN (TrajectoryOptimization) or TT_VARIANT_TRACK_OBCA
    (MPCTrackingControlObs).  obstacles: (M,4) array of (cx, cy, w, h)."""

    def __init__(self, N, params, Q, R, xlb, xub, ulb, uub, obstacles, variant=TT_VARIANT_OBCA_PLAN, tol=0.0,
                 acc_tol=0.0, max_iter=0, acc_iter=0, dual_init=False, device=None):
        ob = _f64(obstacles).reshape(-1, 4)
        self.M = int(ob.shape[0])
        self.n = obca_n(int(N), self.M)
        self.obstacles = ob
        super().__init__(N, params, params["W1"], params["W2"], Q, R, xlb, xub, ulb, uub, ob, variant, tol, acc_tol,
                         max_iter, acc_iter, dual_init, device)

    def _scenes(self, B, obstacles, d_min):
        """The host arrays of per-instance scenes, checked: obstacles (B,M,4)|None, d_min (B,) or a scalar|None ->
        (obstacles, d_min, TTObcaScenes).  ValueError on a wrong shape or a wrong M, before any call into the library."""
        ob = dm = None
        if obstacles is not None:
            ob = _f64(obstacles)
            if ob.shape != (B, self.M, 4):
                raise ValueError(f"per-instance obstacles must have shape (B, M, 4) = {(B, self.M, 4)}, got {ob.shape}")
        if d_min is not None:
            dm = np.full(B, float(d_min)) if np.ndim(d_min) == 0 else _f64(d_min)
            if dm.shape != (B,):
                raise ValueError(f"per-instance d_min must be a scalar or have shape (B,) = {(B,)}, got {dm.shape}")
        return ob, dm, TTObcaScenes(None if ob is None else ob.ctypes.data, None if dm is None else dm.ctypes.data)

    def solve(self, x0, x_goal=None, xref=None, uref=None, z_guess=None, iterate=False, obstacles=None, d_min=None):
        """Host arrays -> (X (B,N+1,6), U (B,N,2), z (B,n), status, iters, kkt); with ``iterate=True`` also the final
        primal-dual iterate (B, tt_obca_iterate_len) of the diagnostic export (include/ttmpc.h) as a 7th element.

        obstacles (B,M,4) and d_min (B,) (or a scalar for every instance) give each instance its own scene
        (tt_obca_solve_batch_scenes); one left None is the handle's.  Row b then solves bitwise as a B = 1 call on a
        handle whose ``set_scene`` got row b.  TTError (-EINVAL, nothing launched) on a value ``set_scene`` refuses."""
        N, n = self.N, self.n
        x0 = _f64(x0)
        B = x0.shape[0] if x0.ndim == 2 else 1
        x0 = x0.reshape(B, 6)
        if obstacles is not None or d_min is not None:
            ob, dm, sc = self._scenes(B, obstacles, d_min)
        xg = None if x_goal is None else _f64(x_goal, (B, 6))
        xr = None if xref is None else _f64(xref, (B, N + 1, 6))
        ur = None if uref is None else _f64(uref, (B, N, 2))
        zg = None if z_guess is None else _f64(z_guess, (B, n))
        X = np.empty((B, N + 1, 6))
        U = np.empty((B, N, 2))
        Z = np.empty((B, n))
        st = np.empty(B, dtype=np.int32)
        it = np.empty(B, dtype=np.int32)
        kk = np.empty(B)
        if obstacles is not None or d_min is not None:
            I = np.empty((B, self.iterate_len())) if iterate else None
            rc = self._L.tt_obca_solve_batch_scenes(self._h, B, _ptr(x0), _ptr(xg), _ptr(xr), _ptr(ur), _ptr(zg),
                                                    _ptr(X), _ptr(U), _ptr(Z), st.ctypes.data_as(_ip),
                                                    it.ctypes.data_as(_ip), _ptr(kk), _ptr(I), C.byref(sc))
            if rc != 0:
                self._err(rc, "tt_obca_solve_batch_scenes")
            _warn_handoff(st)
            return (X, U, Z, st, it, kk, I) if iterate else (X, U, Z, st, it, kk)
        if iterate:
            I = np.empty((B, int(self._L.tt_obca_iterate_len(N, self.M))))
            rc = self._L.tt_obca_solve_batch_iterate(self._h, B, _ptr(x0), _ptr(xg), _ptr(xr), _ptr(ur), _ptr(zg),
                                                     _ptr(X), _ptr(U), _ptr(Z), st.ctypes.data_as(_ip),
                                                     it.ctypes.data_as(_ip), _ptr(kk), _ptr(I))
            if rc != 0:
                self._err(rc, "tt_obca_solve_batch_iterate")
            _warn_handoff(st)
            return X, U, Z, st, it, kk, I
        rc = self._L.tt_obca_solve_batch(self._h, B, _ptr(x0), _ptr(xg), _ptr(xr), _ptr(ur), _ptr(zg), _ptr(X),
                                         _ptr(U), _ptr(Z), st.ctypes.data_as(_ip), it.ctypes.data_as(_ip), _ptr(kk))
        if rc != 0:
            self._err(rc, "tt_obca_solve_batch")
        _warn_handoff(st)
        return X, U, Z, st, it, kk

    def set_helpers(self, n):
        """Diagnostics: helper workgroups of this handle's launches (0 none, -1 one per CU: the default).  The block
        passes of the instances still solving run on the idle CUs; the results are bitwise the same either way."""
        if hasattr(self._L, "ttx_obca_set_helpers"):
            self._L.ttx_obca_set_helpers(self._h, int(n))

    def set_handoff_debug(self, spin_us=0, fail_b=-1):
        """Diagnostics: the helper hand-off's spin limit in microseconds (0: the default 5 s) and one instance whose
        hand-offs never complete (-1: none); that instance then ends with TT_HANDOFF_TIMEOUT (6)."""
        rc = self._L.ttx_obca_set_handoff_debug(self._h, int(spin_us), int(fail_b))
        if rc != 0:
            self._err(rc, "ttx_obca_set_handoff_debug")

    def solve_device(self, B, x0, x_goal, xref, uref, z_guess, x_out, u_out, z_out, status, iters=0, kkt=0, stream=0,
                     iterate=0, obstacles=0, d_min=0):
        """Device pointers (ints), enqueued on ``stream``.  iterate: (B, tt_obca_iterate_len) for the final primal-dual
        iterate, the device twin of ``solve(iterate=True)`` (0 = not wanted); the other outputs are bitwise the same
        with or without it.  obstacles (B,M,4) / d_min (B,): per-instance scenes (tt_obca_solve_batch_scenes_device;
        0 = the handle's); an instance whose scene ``set_scene`` would refuse ends TT_NONFINITE with 0 iterations."""
        if obstacles or d_min:
            sc = TTObcaScenes(obstacles or None, d_min or None)
            rc = self._L.tt_obca_solve_batch_scenes_device(self._h, int(B), x0, x_goal or None, xref or None,
                                                           uref or None, z_guess or None, x_out, u_out, z_out or None,
                                                           status, iters or None, kkt or None, iterate or None,
                                                           C.byref(sc), stream or None)
            if rc != 0:
                self._err(rc, "tt_obca_solve_batch_scenes_device")
            return
        if iterate:
            rc = self._L.tt_obca_solve_batch_iterate_device(self._h, int(B), x0, x_goal or None, xref or None,
                                                            uref or None, z_guess or None, x_out, u_out, z_out or None,
                                                            status, iters or None, kkt or None, iterate, stream or None)
            if rc != 0:
                self._err(rc, "tt_obca_solve_batch_iterate_device")
            return
        rc = self._L.tt_obca_solve_batch_device(self._h, int(B), x0, x_goal or None, xref or None, uref or None,
                                                z_guess or None, x_out, u_out, z_out or None, status, iters or None,
                                                kkt or None, stream or None)
        if rc != 0:
            self._err(rc, "tt_obca_solve_batch_device")

    def iterate_len(self):
        """tt_obca_iterate_len of this handle's (N, M)."""
        return int(self._L.tt_obca_iterate_len(self.N, self.M))

    def set_scene(self, obstacles=None, d_min=None):
        """tt_set_scene: the handle's obstacles (M,4) of (cx, cy, w, h) (M is fixed) and its safety margin d_min (0.2
        unless set); a value left None keeps the current one.  Host-side state only: every later call uses it."""
        ob = None if obstacles is None else _f64(obstacles, (self.M, 4))
        dm = None if d_min is None else np.array([float(d_min)])
        rc = self._L.tt_set_scene(self._h, _ptr(ob), _ptr(dm))
        if rc != 0:
            self._err(rc, "tt_set_scene")
        if ob is not None:
            self.obstacles = ob.copy()

    def scene(self):
        """tt_get_scene -> (obstacles (M,4), d_min)."""
        ob, dm = np.empty((self.M, 4)), np.empty(1)
        rc = self._L.tt_get_scene(self._h, _ptr(ob), _ptr(dm))
        if rc != 0:
            self._err(rc, "tt_get_scene")
        return ob, float(dm[0])

    def set_geometry(self, L1=None, L2=None, M=None, W1=None, W2=None):
        """tt_set_geometry: change the handle's lengths L1, L2, hitch offset M and widths W1, W2 (a value left None keeps
        its current one).  Host-side state only: every later call of this solver runs with the new values, and a solve
        is bitwise that of a fresh solver created with them.  Work already enqueued keeps the old values.  Raises
        TTError for a length or width <= 0 or a non-finite value (nothing is changed then)."""
        cur = self.geometry()
        v = [float(c if x is None else x) for x, c in zip((L1, L2, M, W1, W2), cur)]
        rc = self._L.tt_set_geometry(self._h, *v)
        if rc != 0:
            self._err(rc, "tt_set_geometry")

    def geometry(self):
        """tt_get_geometry: the handle's current (L1, L2, M, W1, W2)."""
        v = [C.c_double() for _ in range(5)]
        rc = self._L.tt_get_geometry(self._h, *[C.byref(c) for c in v])
        if rc != 0:
            self._err(rc, "tt_get_geometry")
        return tuple(c.value for c in v)

    def vjp_params_work_bytes(self):
        """tt_obca_vjp_params_work_bytes of this handle's (N, M): bytes of ``work`` per instance."""
        return int(self._L.tt_obca_vjp_params_work_bytes(self.N, self.M))

    def vjp_device(self, B, iterate, status, grad_x=0, grad_u=0, g_x0=0, g_xref=0, g_uref=0, vjp_status=0, stream=0,
                   xref=0, uref=0, g_obstacles=0, g_dmin=0, g_Q=0, g_R=0, work=0, obstacles=0, d_min=0, g_geometry=0):
        """tt_obca_vjp_device (TT_VARIANT_TRACK_OBCA): the adjoint kernel on the device iterate and status of an earlier
        ``solve_device(..., iterate=ptr)`` and the upstream gradients grad_x = dL/dX, grad_u = dL/dU (0 = zeros, not
        both).  Outputs (0 = not wanted): g_x0, g_xref, g_uref, vjp_status.  Uses no buffer of the handle: any stream
        will do, behind the solve whose iterate it reads.

        With ``work`` (B * vjp_params_work_bytes() bytes) or one of g_obstacles (B,M,4), g_dmin (B,), g_Q (B,6,6),
        g_R (B,2,2) the call is tt_obca_vjp_params_device: the same adjoint with the block unknowns carried, plus the
        scene and weight gradients; xref / uref are the solve's (needed for g_Q / g_R only).

        obstacles (B,M,4) / d_min (B,): the per-instance scenes the solve was given (tt_obca_vjp_scenes_device, which
        picks the kernel by the same rule); g_obstacles and g_dmin are then the gradients in each instance's own scene.

        g_geometry (B,5): also dL/d(L1, L2, M, W1, W2) per instance at the handle's geometry
        (tt_obca_vjp_geometry_device; needs ``work``); the other outputs are bitwise those of the call without it."""
        self._vjp_call(True, B, iterate or None, status or None, xref or None, uref or None, grad_x or None,
                       grad_u or None, [p or None for p in (g_x0, g_xref, g_uref, vjp_status, g_obstacles, g_dmin, g_Q,
                                                             g_R, g_geometry)],
                       TTObcaScenes(obstacles or None, d_min or None), work or None, stream or None)

    def _vjp_call(self, device, B, iterate, status, xref, uref, grad_x, grad_u, outs, scenes, work=None, stream=None):
        """The one library call behind ``vjp`` and ``vjp_device``.  outs: the nine members of tt_obca_vjp_geometry_out
        as addresses (None = not wanted); the narrower out-structs are prefixes of it.  The entry is the narrowest that
        carries what was asked for: geometry with g_geometry, else scenes with a per-instance scene, else params with
        ``work`` or a parameter output, else the plain one."""
        out = TTObcaVjpGeometryOut(*outs)
        if out.g_geometry:
            name = "tt_obca_vjp_geometry"
        elif scenes.obstacles or scenes.d_min:
            name = "tt_obca_vjp_scenes"
        elif work or out.g_obstacles or out.g_dmin or out.g_Q or out.g_R:
            name = "tt_obca_vjp_params"
        else:
            name = "tt_obca_vjp"
        args = [self._h, int(B), iterate, status] + ([xref, uref] if name != "tt_obca_vjp" else [])
        args += [grad_x, grad_u, C.byref(out)] + ([work] if device and name != "tt_obca_vjp" else [])
        args += [C.byref(scenes)] if name in ("tt_obca_vjp_geometry", "tt_obca_vjp_scenes") else []
        if device:
            name += "_device"
            args.append(stream)
        rc = getattr(self._L, name)(*args)
        if rc != 0:
            self._err(rc, name)

    def vjp(self, iterate, status, grad_x, grad_u, xref=None, uref=None, params=False, obstacles=None, d_min=None,
            geometry=False):
        """Host arrays: the gradient of a scalar loss L(X, U) with respect to x_init, xref and uref of the MPC+OBCA
        solve that returned iterate (B, tt_obca_iterate_len) and status (B,); grad_x (B,N+1,6) = dL/dX and grad_u (B,N,2) =
        dL/dU (either may be None for zeros).  Returns a ``TrackVjpResult`` (g_wq_wr and g_model are None).

        ``params=True``: tt_obca_vjp_params, an ``ObcaVjpParamsResult`` with g_obstacles and g_dmin and, where the
        solve's xref (B,N+1,6) / uref (B,N,2) are given, g_Q / g_R.

        obstacles (B,M,4) / d_min (B,) or a scalar: the per-instance scenes the solve was given (tt_obca_vjp_scenes);
        g_obstacles and g_dmin are then per instance in its own scene.

        ``geometry=True`` implies ``params=True`` and adds g_geometry (B,5) = dL/d(L1, L2, M, W1, W2) per instance
        (tt_obca_vjp_geometry); the other arrays are bitwise those of the params call."""
        N, M = self.N, self.M
        params = params or geometry
        I = _f64(iterate).reshape(-1, self.iterate_len())
        B = I.shape[0]
        ob, dm, sc = self._scenes(B, obstacles, d_min)
        st = np.ascontiguousarray(np.asarray(status, dtype=np.int32)).reshape(B)
        gx = None if grad_x is None else _f64(grad_x, (B, N + 1, 6))
        gu = None if grad_u is None else _f64(grad_u, (B, N, 2))
        xr = None if xref is None or not params else _f64(xref, (B, N + 1, 6))
        ur = None if uref is None or not params else _f64(uref, (B, N, 2))
        r = (ObcaVjpParamsResult if params else TrackVjpResult)(
            g_x0=np.empty((B, 6)), g_xref=np.empty((B, N + 1, 6)), g_uref=np.empty((B, N, 2)),
            vjp_status=np.empty(B, dtype=np.int32))
        if params:
            r.g_obstacles, r.g_dmin = np.empty((B, M, 4)), np.empty(B)
            r.g_Q = None if xr is None else np.empty((B, 6, 6))
            r.g_R = None if ur is None else np.empty((B, 2, 2))
            r.g_geometry = np.empty((B, 5)) if geometry else None
        outs = [getattr(r, k, None) for k in ObcaVjpParamsResult.__slots__]
        self._vjp_call(False, B, _ptr(I), st.ctypes.data_as(_ip), _ptr(xr), _ptr(ur), _ptr(gx), _ptr(gu),
                       [None if a is None else a.ctypes.data for a in outs], sc)
        return r
