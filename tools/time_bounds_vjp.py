"""Launch times of track_vjp_kernel's instantiations with and without the bounds gradient, the closed loop's backward
step with and without it, and the parent's adjoint outputs against this build's, bit for bit.

    timeout 300 python tools/time_bounds_vjp.py [--parent <libttmpc.so of the parent commit>] [--launches 200]
                                                [--rounds 5] [--shapes 1024x20,256x40] [--loop 1024x20x50]

One GPU process, the method of tools/time_vjp.py and tools/time_model_vjp.py (whose helpers it uses).  Per shape: one
solve with multiplier export gives the device arrays; then, per round, `--launches` back-to-back launches of each kernel
between two device events, the kernels alternating within a round, after a warm-up of each: the plain and the model
instantiation of the parent's library (when --parent is given: a second handle made through that library's own
tt_create, in the same process), the plain and the model instantiation of this build, and the bounds instantiations
(g_bounds alone, g_bounds beside g_model, and that accumulated as the closed loop calls it).  Then the loop of
tools/time_loop_vjp.py: ClosedLoop.backward with bounds=False and bounds=True, alternating, in microseconds per step.
With --parent also the comparison of the existing adjoint outputs: tt_track_vjp_device and tt_track_vjp_model_device of
both libraries on the two checked input sets of tests/sens_reference.py (solved once, by this build), array by array.
Prints the median and the min..max over the rounds, the number of arrays compared and how many are bitwise equal, and
one JSON line.
"""
import argparse
import ctypes as C
import json
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO), str(REPO / "car-trailer-mpc_amd"), str(REPO / "tests"), str(REPO / "tools")]

from time_model_vjp import PARAMS, parent_handle, report, rounds_of  # noqa: E402


def parent_with_model(path, s, N):
    """time_model_vjp.parent_handle plus the model entry's signature."""
    L, h = parent_handle(path, s, N)
    L.tt_track_vjp_model_device.argtypes = s._L.tt_track_vjp_model_device.argtypes
    L.tt_track_vjp_model_device.restype = C.c_int
    return L, h


def compare_with_parent(path):
    """The plain and the model adjoint of both libraries on case_free and case_active -> (arrays compared, equal)."""
    import numpy as np
    import torch

    import sens_reference as sr
    import vjp_harness as h
    import vjp_reference as vr
    from ttmpc._lib import TTTrackVjpModelOut, TTTrackVjpOut
    total = same = 0
    for name in ("free", "active"):
        nlp, x0, xr, ur = sr.case(name)
        B, N = x0.shape[0], nlp.N
        s = h.solver(nlp)
        r = s.solve_ex(x0, xr, ur, duals=True, gain=False)
        gX, gU = vr.random_upstream(B, N)
        PL, ph = parent_with_model(path, s, N)
        ins = [h.t(a) for a in (r.X, r.U, r.dual, xr, ur)]
        st, tgx, tgu = h.t(r.status, torch.int32), h.t(gX), h.t(gU)
        got = {}
        for who, L, hd in (("parent", PL, ph), ("this", s._L, s._h)):
            for entry in ("plain", "model"):
                outs = [torch.full(sh, np.nan, dtype=torch.float64, device="cuda")
                        for sh in ((B, 6), (B, N + 1, 6), (B, N, 2), (B, 8))]
                vst = torch.full((B,), -1, dtype=torch.int32, device="cuda")
                gm = torch.full((B, 3), np.nan, dtype=torch.float64, device="cuda")
                head = [hd, B] + [t.data_ptr() for t in ins] + [None, st.data_ptr(), tgx.data_ptr(), tgu.data_ptr()]
                if entry == "plain":
                    o = TTTrackVjpOut(*[t.data_ptr() for t in outs], vst.data_ptr())
                    rc = L.tt_track_vjp_device(*head, C.byref(o), None)
                else:
                    o = TTTrackVjpModelOut(*[t.data_ptr() for t in outs], gm.data_ptr(), vst.data_ptr())
                    rc = L.tt_track_vjp_model_device(*head, C.byref(o), 0, None)
                assert rc == 0, (who, entry, rc)
                torch.cuda.synchronize()
                got[who, entry] = [h.n(t) for t in outs + [vst] + ([gm] if entry == "model" else [])]
        for entry in ("plain", "model"):
            for a, b in zip(got["parent", entry], got["this", entry]):
                total += 1
                same += int(np.array_equal(a, b))
        assert not got["this", "plain"][4].any()
    return total, same


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
    from ttmpc._lib import TTTrackVjpModelOut, TTTrackVjpOut
    from ttmpc.scenarios import synthetic_batch

    if not torch.cuda.is_available():
        sys.exit("time_bounds_vjp: no GPU (timings are taken on the device only)")
    dev = torch.device("cuda")
    stream = torch.cuda.current_stream().cuda_stream
    result = {}
    for shape in (args.shapes.split(",") if args.shapes else []):
        B, N = (int(v) for v in shape.split("x"))
        s = ttmpc.BatchSolver(N, dict(PARAMS, horizon=N), to.DEFAULT_Q, to.DEFAULT_R, to.MPC_XLB, to.MPC_XUB,
                              to.MPC_ULB, to.MPC_UUB)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        new = lambda *sh: torch.empty(sh, dtype=torch.float64, device=dev)  # noqa: E731
        zeros = lambda *sh: torch.zeros(sh, dtype=torch.float64, device=dev)  # noqa: E731
        x0, xr, ur = (t(a) for a in synthetic_batch(B, N, seed=0))
        X, U, dual, st = new(B, N + 1, 6), new(B, N, 2), new(B, N + 1, 22), torch.empty(B, dtype=torch.int32, device=dev)
        rng = np.random.default_rng(1)
        gX, gU = t(rng.uniform(-1, 1, (B, N + 1, 6))), t(rng.uniform(-1, 1, (B, N, 2)))
        g0, gxr, gur, gw, gm, gb = new(B, 6), new(B, N + 1, 6), new(B, N, 2), new(B, 8), zeros(B, 3), zeros(B, 16)
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
            PL, ph = parent_with_model(args.parent, s, N)
            head = (ph, B, X.data_ptr(), U.data_ptr(), dual.data_ptr(), xr.data_ptr(), ur.data_ptr(), None, st.data_ptr(),
                    gX.data_ptr(), gU.data_ptr())
            po = TTTrackVjpOut(g0.data_ptr(), gxr.data_ptr(), gur.data_ptr(), gw.data_ptr(), vst.data_ptr())
            pm = TTTrackVjpModelOut(g0.data_ptr(), gxr.data_ptr(), gur.data_ptr(), gw.data_ptr(), gm.data_ptr(),
                                    vst.data_ptr())
            kernels["plain, parent's library"] = lambda: PL.tt_track_vjp_device(*head, C.byref(po), stream)
            kernels["model, parent's library"] = lambda: PL.tt_track_vjp_model_device(*head, C.byref(pm), 0, stream)
        kernels["plain, this build"] = vjp
        kernels["model, this build"] = lambda: vjp(g_model=gm.data_ptr())
        kernels["bounds"] = lambda: vjp(g_bounds=gb.data_ptr())
        kernels["bounds and model"] = lambda: vjp(g_bounds=gb.data_ptr(), g_model=gm.data_ptr())
        kernels["bounds and model, accumulate"] = lambda: vjp(g_bounds=gb.data_ptr(), g_model=gm.data_ptr(),
                                                             accumulate=True)
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

        def backward(**kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(cur)
            out = cl.backward(tape, GS, GU, **kw)
            e1.record(cur)
            e1.synchronize()
            return 1e3 * e0.elapsed_time(e1) / K, out
        forms = {"backward step": {}, "backward step, bounds=True": dict(bounds=True),
                 "backward step, model=True": dict(model=True),
                 "backward step, bounds=True, model=True": dict(bounds=True, model=True)}
        for kw in forms.values():
            backward(**kw)
        times = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, kw in forms.items():
                us, grads = backward(**kw)
                times[k].append(us)
        assert bool(torch.isfinite(grads["g_bounds"]).all())
        print(f"closed loop B = {B}, N = {N}, K = {K}, {args.rounds} rounds, us per step:")
        result["loop " + args.loop] = report(times, 40)

    if args.parent:
        total, same = compare_with_parent(args.parent)
        print(f"parent's library against this build, tt_track_vjp_device and tt_track_vjp_model_device on the two "
              f"checked input sets: {total} arrays compared, {same} bitwise equal")
        result["parent_compare"] = {"arrays": total, "bitwise_equal": same}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
