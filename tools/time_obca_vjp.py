#!/usr/bin/env python3
"""Time the MPC+OBCA adjoint (tt_obca_vjp_device) and its params entry (tt_obca_vjp_params_device: the scene and weight
gradients, the block unknowns carried in HBM) next to the solve they differentiate, with device events.

Two shapes: the drivers' (B = 64, N = 50, M = 11: the golden windows, tiled) and B = 1024 on case A of
tests/obca_vjp_reference.py (N = 6, M = 1).  Solve, adjoint and params adjoint alternate for several rounds, as
tools/time_vjp.py does; the line per shape gives the median of each and the ratios adjoint / solve, params / adjoint
and params / solve.

    python tools/time_obca_vjp.py [--rounds 5] [--geometry]

--geometry also times the geometry entry (tt_obca_vjp_geometry_device: the params outputs plus dL/d(L1, L2, Mh, W1, W2))
in the same alternation and adds geometry_ms and geometry_over_params to the line.  A library without the entry
(TTMPC_LIB pointing at an older build) is timed without it, so the same command measures both sides of a comparison.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "car-trailer-mpc_amd"), str(ROOT), str(ROOT / "tests")]


def shapes():
    import obca_vjp_reference as orf
    from ttmpc import scenarios as sc
    g = np.load(ROOT / "tests" / "golden" / "reference_numpy.npz")
    x0, xr, ur = sc.mpc_obs_batch(g["state_traj"], g["input_traj"], 16, 50, seed=0)
    t = 4
    bnd = (sc.XLB, sc.XUB, sc.ULB, sc.UUB)
    yield ("windows B=64 N=50 M=11", 50, dict(sc.OBCA_PARAMS, dt=0.05), bnd, g["obstacles"], np.tile(x0, (t, 1)),
           np.tile(xr, (t, 1, 1)), np.tile(ur, (t, 1, 1)))
    N, p, Q, R, bnd, obs, a, b, c = orf.case_a()
    yield ("case A B=1024 N=6 M=1", N, p, bnd, obs, np.tile(a, (1024, 1)), np.tile(b, (1024, 1, 1)),
           np.tile(c, (1024, 1, 1)))


def main():
    import torch
    import ttmpc
    from ttmpc import scenarios as sc
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--geometry", action="store_true", help="also time tt_obca_vjp_geometry_device")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name, N, p, bnd, obs, x0, xr, ur in shapes():
        s = ttmpc.ObcaSolver(N, p, sc.OBCA_Q, sc.OBCA_R, *bnd, obs, variant=ttmpc.TT_VARIANT_TRACK_OBCA, device=0)
        B = x0.shape[0]
        t = lambda v: torch.as_tensor(np.ascontiguousarray(v), device=dev)  # noqa: E731
        dx0, dxr, dur = t(x0), t(xr), t(ur)
        new = lambda *sh: torch.empty(sh, dtype=torch.float64, device=dev)  # noqa: E731
        X, U, I = new(B, N + 1, 6), new(B, N, 2), new(B, s.iterate_len())
        st = torch.empty(B, dtype=torch.int32, device=dev)
        gX = torch.rand(B, N + 1, 6, dtype=torch.float64, device=dev)
        gU = torch.rand(B, N, 2, dtype=torch.float64, device=dev)
        g0, gr, gu = new(B, 6), new(B, N + 1, 6), new(B, N, 2)
        vs = torch.empty(B, dtype=torch.int32, device=dev)
        vp = torch.empty(B, dtype=torch.int32, device=dev)
        gob, gdm, gQ, gR = new(B, s.M, 4), new(B), new(B, 6, 6), new(B, 2, 2)
        work = new(B * s.vjp_params_work_bytes() // 8)
        geo = a.geometry and hasattr(s._L, "tt_obca_vjp_geometry_device")
        gge, vg = new(B, 5), torch.empty(B, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def solve():
            s.solve_device(B, dx0.data_ptr(), 0, dxr.data_ptr(), dur.data_ptr(), 0, X.data_ptr(), U.data_ptr(), 0,
                           st.data_ptr(), stream=stream, iterate=I.data_ptr())

        def adjoint():
            s.vjp_device(B, I.data_ptr(), st.data_ptr(), grad_x=gX.data_ptr(), grad_u=gU.data_ptr(), g_x0=g0.data_ptr(),
                         g_xref=gr.data_ptr(), g_uref=gu.data_ptr(), vjp_status=vs.data_ptr(), stream=stream)

        def params():
            s.vjp_device(B, I.data_ptr(), st.data_ptr(), grad_x=gX.data_ptr(), grad_u=gU.data_ptr(), g_x0=g0.data_ptr(),
                         g_xref=gr.data_ptr(), g_uref=gu.data_ptr(), vjp_status=vp.data_ptr(), stream=stream,
                         xref=dxr.data_ptr(), uref=dur.data_ptr(), g_obstacles=gob.data_ptr(), g_dmin=gdm.data_ptr(),
                         g_Q=gQ.data_ptr(), g_R=gR.data_ptr(), work=work.data_ptr())

        def geometry():
            s.vjp_device(B, I.data_ptr(), st.data_ptr(), grad_x=gX.data_ptr(), grad_u=gU.data_ptr(), g_x0=g0.data_ptr(),
                         g_xref=gr.data_ptr(), g_uref=gu.data_ptr(), vjp_status=vg.data_ptr(), stream=stream,
                         xref=dxr.data_ptr(), uref=dur.data_ptr(), g_obstacles=gob.data_ptr(), g_dmin=gdm.data_ptr(),
                         g_Q=gQ.data_ptr(), g_R=gR.data_ptr(), work=work.data_ptr(), g_geometry=gge.data_ptr())

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        solve()
        adjoint()
        params()
        if geo:
            geometry()
        torch.cuda.synchronize(dev)
        ts, ta, tp, tg = [], [], [], []
        for _ in range(a.rounds):
            ts.append(timed(solve))
            ta.append(timed(adjoint))
            tp.append(timed(params))
            if geo:
                tg.append(timed(geometry))
        ms, ma, mp = float(np.median(ts)), float(np.median(ta)), float(np.median(tp))
        extra = {}
        if geo:
            mg = float(np.median(tg))
            extra = {"geometry_ms": round(mg, 4), "geometry_over_params": round(mg / mp, 4),
                     "geometry_ok": int((vg == 0).sum().item())}
        print(json.dumps({"shape": name, "solve_ms": round(ms, 3), "adjoint_ms": round(ma, 4),
                          "adjoint_over_solve": round(ma / ms, 5), "params_ms": round(mp, 4),
                          "params_over_adjoint": round(mp / ma, 4), "params_over_solve": round(mp / ms, 5),
                          "solved": int((st <= 1).sum().item()), "adjoint_ok": int((vs == 0).sum().item()),
                          "params_ok": int((vp == 0).sum().item()), "work_mb": round(work.numel() * 8 / 2**20, 2),
                          "rounds": a.rounds, **extra}))


if __name__ == "__main__":
    main()
