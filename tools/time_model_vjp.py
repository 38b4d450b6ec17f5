"""Launch times of track_vjp_kernel's two instantiations, and of the closed loop's backward step with and without the
model gradient.

    timeout 300 python tools/time_model_vjp.py [--parent <libttmpc.so of the parent commit>] [--launches 200]
                                               [--rounds 5] [--shapes 1024x20,256x40] [--loop 1024x20x50]

One GPU process.  Per shape: one solve with multiplier export gives the device arrays; then, per round, `--launches`
back-to-back launches of each kernel between two device events, the kernels alternating within a round, after a warm-up
of each: the plain adjoint of the parent's library (when --parent is given: a second handle made through that library's
own tt_create, in the same process), the plain adjoint of this build and the model instantiation (g_model written, and
accumulated).  Then the loop of tools/time_loop_vjp.py: ClosedLoop.backward with model=False and model=True, alternating,
in microseconds per step (the parent's backward step comes from tools/time_loop_vjp.py under TTMPC_LIB=<parent>).
Prints the median and the min..max over the rounds, and one JSON line.
"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO), str(REPO / "car-trailer-mpc_amd")]

PARAMS = {"M": 0.15, "L1": 7.05, "L2": 12.45, "W1": 3.05, "W2": 2.95, "dt": 0.05}


def parent_handle(path, s, N):
    """(library, handle) of a second build loaded beside this one: the configuration of the BatchSolver s."""
    from ttmpc._lib import TTConfig, _dp, _ptr
    L = C.CDLL(str(path))
    L.tt_create.argtypes = [C.POINTER(TTConfig), _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.c_int, C.POINTER(C.c_void_p)]
    L.tt_create.restype = C.c_int
    L.tt_track_vjp_device.argtypes = s._L.tt_track_vjp_device.argtypes
    L.tt_track_vjp_device.restype = C.c_int
    cfg = TTConfig()
    cfg.nx, cfg.nu, cfg.N, cfg.M = 6, 2, N, 0
    cfg.dt, cfg.L1, cfg.L2, cfg.Mh = PARAMS["dt"], PARAMS["L1"], PARAMS["L2"], PARAMS["M"]
    cfg.variant = s.variant
    h = C.c_void_p()
    rc = L.tt_create(C.byref(cfg), _ptr(s.Q), _ptr(s.R), *[_ptr(b) for b in s.bounds], None, s.device, C.byref(h))
    if rc != 0:
        sys.exit(f"time_model_vjp: tt_create of {path} failed ({rc})")
    return L, h


def rounds_of(kernels, launches, rounds):
    import torch
    for f in kernels.values():
        for _ in range(20):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in kernels}
    for _ in range(rounds):
        for k, f in kernels.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(1e3 * e0.elapsed_time(e1) / launches)
    return times


def report(times, width=34):
    for k, v in times.items():
        print(f"  {k:{width}s} median {statistics.median(v):8.2f}   min {min(v):8.2f}   max {max(v):8.2f}")
    return {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="1024x20,256x40")
    ap.add_argument("--loop", default="1024x20x50", help="BxNxK of the closed loop ('' skips it)")
    args = ap.parse_args()

    import numpy as np
    import torch

    import ttmpc
    from oracle import ttmpc_oracle as to
    from ttmpc._lib import TTTrackVjpOut
    from ttmpc.scenarios import synthetic_batch

    if not torch.cuda.is_available():
        sys.exit("time_model_vjp: no GPU (timings are taken on the device only)")
    dev = torch.device("cuda")
    stream = torch.cuda.current_stream().cuda_stream
    result = {}
    for shape in args.shapes.split(","):
        B, N = (int(v) for v in shape.split("x"))
        s = ttmpc.BatchSolver(N, dict(PARAMS, horizon=N), to.DEFAULT_Q, to.DEFAULT_R, to.MPC_XLB, to.MPC_XUB,
                              to.MPC_ULB, to.MPC_UUB)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        new = lambda *sh: torch.empty(sh, dtype=torch.float64, device=dev)  # noqa: E731
        x0, xr, ur = (t(a) for a in synthetic_batch(B, N, seed=0))
        X, U, dual, st = new(B, N + 1, 6), new(B, N, 2), new(B, N + 1, 22), torch.empty(B, dtype=torch.int32, device=dev)
        rng = np.random.default_rng(1)
        gX, gU = t(rng.uniform(-1, 1, (B, N + 1, 6))), t(rng.uniform(-1, 1, (B, N, 2)))
        g0, gxr, gur, gw, gm = new(B, 6), new(B, N + 1, 6), new(B, N, 2), new(B, 8), torch.zeros((B, 3), dtype=torch.float64,
                                                                                                 device=dev)
        vst = torch.empty(B, dtype=torch.int32, device=dev)
        s.solve_ex_device(B, x0.data_ptr(), xr.data_ptr(), ur.data_ptr(), X.data_ptr(), U.data_ptr(), st.data_ptr(),
                          dual=dual.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        ok = int((st <= 1).sum())

        def vjp(**kw):
            s.vjp_device(B, X.data_ptr(), U.data_ptr(), dual.data_ptr(), xr.data_ptr(), ur.data_ptr(), st.data_ptr(),
                         grad_x=gX.data_ptr(), grad_u=gU.data_ptr(), g_x0=g0.data_ptr(), g_xref=gxr.data_ptr(),
                         g_uref=gur.data_ptr(), g_wq_wr=gw.data_ptr(), vjp_status=vst.data_ptr(), stream=stream, **kw)

        kernels = {}
        if args.parent:
            PL, ph = parent_handle(args.parent, s, N)
            out = TTTrackVjpOut(g0.data_ptr(), gxr.data_ptr(), gur.data_ptr(), gw.data_ptr(), vst.data_ptr())
            kernels["plain adjoint, parent's library"] = lambda: PL.tt_track_vjp_device(
                ph, B, X.data_ptr(), U.data_ptr(), dual.data_ptr(), xr.data_ptr(), ur.data_ptr(), None, st.data_ptr(),
                gX.data_ptr(), gU.data_ptr(), C.byref(out), stream)
        kernels["plain adjoint, this build"] = vjp
        kernels["model instantiation"] = lambda: vjp(g_model=gm.data_ptr())
        kernels["model instantiation, accumulate"] = lambda: vjp(g_model=gm.data_ptr(), accumulate=True)
        times = rounds_of(kernels, args.launches, args.rounds)
        assert int((vst == 0).sum()) == ok, "adjoint failed on solved instances"
        print(f"B = {B}, N = {N} ({ok} of {B} solved), {args.launches} launches x {args.rounds} rounds, us per launch:")
        result[shape] = report(times)

    if args.loop:
        from ttmpc import scenarios as sc
        from ttmpc import simulation as sim
        B, N, K = (int(v) for v in args.loop.split("x"))
        g = np.load(REPO / "tests" / "golden" / "reference_numpy.npz")
        S, U = g["interp_states"], g["interp_inputs"]
        params = dict(sc.PARAMS, horizon=N)
        rng = np.random.default_rng(0)
        x0 = S[:, 0][None] + rng.normal(scale=[0.3, 0.3, 0.02, 0.02, 0.0, 0.0], size=(B, 6))
        T = (K - 0.5) * params["dt"]
        noise = torch.from_numpy(rng.normal(scale=0.02, size=(K, B, 6))).to(dev)
        w = torch.from_numpy(rng.uniform(0.7, 1.4, (B, 8))).to(dev)
        GS = torch.from_numpy(rng.uniform(-1, 1, (K + 1, B, 6))).to(dev)
        GU = torch.from_numpy(rng.uniform(-1, 1, (K, B, 2))).to(dev)
        solver = ttmpc.BatchSolver(N, params, sc.MPC_Q, sc.MPC_R, sc.XLB, sc.XUB, sc.ULB, sc.UUB)
        cl = sim.ClosedLoop(solver, S, U, params, sim.DISTURBANCE_PARAMS)
        tape = cl.run_tape(x0, T, noise=noise, wq_wr=w)["tape"]
        cur = torch.cuda.current_stream(dev)

        def backward(model):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(cur)
            out = cl.backward(tape, GS, GU, model=model)
            e1.record(cur)
            e1.synchronize()
            return 1e3 * e0.elapsed_time(e1) / K, out
        backward(False), backward(True)
        times = {"backward step, model=False": [], "backward step, model=True": []}
        for _ in range(args.rounds):
            times["backward step, model=False"].append(backward(False)[0])
            us, grads = backward(True)
            times["backward step, model=True"].append(us)
        assert bool(torch.isfinite(grads["g_model_solver"]).all() and torch.isfinite(grads["g_model_plant"]).all())
        print(f"closed loop B = {B}, N = {N}, K = {K}, {args.rounds} rounds, us per step:")
        result["loop " + args.loop] = report(times)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
