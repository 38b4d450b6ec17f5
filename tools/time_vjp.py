"""Launch times of track_vjp_kernel next to track_sens_kernel (gain only) and the solve that feeds them.

    timeout 300 python tools/time_vjp.py [--launches 200] [--rounds 5] [--shapes 1024x20,256x40]

One GPU process.  Per shape: one solve with multiplier export gives the device arrays; then, per round, `--launches`
back-to-back launches of each kernel between two device events, the kernels alternating within a round, after a
warm-up of each.  Prints the median and the min..max over the rounds in microseconds per launch, and one JSON line.
TTMPC_LIB=<another build> times that build instead (a build without the adjoint skips it).
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO), str(REPO / "car-trailer-mpc_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="1024x20,256x40")
    args = ap.parse_args()

    import numpy as np
    import torch

    import ttmpc
    from oracle import ttmpc_oracle as to
    from ttmpc.scenarios import synthetic_batch

    if not torch.cuda.is_available():
        sys.exit("time_vjp: no GPU (timings are taken on the device only)")
    dev = torch.device("cuda")
    stream = torch.cuda.current_stream().cuda_stream
    params = {"M": 0.15, "L1": 7.05, "L2": 12.45, "W1": 3.05, "W2": 2.95, "dt": 0.05}
    result = {}
    for shape in args.shapes.split(","):
        B, N = (int(v) for v in shape.split("x"))
        s = ttmpc.BatchSolver(N, dict(params, horizon=N), to.DEFAULT_Q, to.DEFAULT_R, to.MPC_XLB, to.MPC_XUB,
                              to.MPC_ULB, to.MPC_UUB)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        new = lambda *sh: torch.empty(sh, dtype=torch.float64, device=dev)  # noqa: E731
        x0, xr, ur = (t(a) for a in synthetic_batch(B, N, seed=0))
        X, U, dual, st = new(B, N + 1, 6), new(B, N, 2), new(B, N + 1, 22), torch.empty(B, dtype=torch.int32, device=dev)
        rng = np.random.default_rng(1)
        gX, gU = t(rng.uniform(-1, 1, (B, N + 1, 6))), t(rng.uniform(-1, 1, (B, N, 2)))
        gain, sst = new(B, 2, 6), torch.empty(B, dtype=torch.int32, device=dev)
        g0, gxr, gur, gw = new(B, 6), new(B, N + 1, 6), new(B, N, 2), new(B, 8)
        vst = torch.empty(B, dtype=torch.int32, device=dev)

        def solve():
            s.solve_ex_device(B, x0.data_ptr(), xr.data_ptr(), ur.data_ptr(), X.data_ptr(), U.data_ptr(), st.data_ptr(),
                              dual=dual.data_ptr(), stream=stream)

        def sens():
            s.sens_device(B, X.data_ptr(), U.data_ptr(), dual.data_ptr(), st.data_ptr(), gain=gain.data_ptr(),
                          sens_status=sst.data_ptr(), stream=stream)

        def vjp():
            s.vjp_device(B, X.data_ptr(), U.data_ptr(), dual.data_ptr(), xr.data_ptr(), ur.data_ptr(), st.data_ptr(),
                         grad_x=gX.data_ptr(), grad_u=gU.data_ptr(), g_x0=g0.data_ptr(), g_xref=gxr.data_ptr(),
                         g_uref=gur.data_ptr(), g_wq_wr=gw.data_ptr(), vjp_status=vst.data_ptr(), stream=stream)

        kernels = {"solve+export": solve, "track_sens_kernel (gain)": sens}
        if hasattr(s._L, "tt_track_vjp_device"):
            kernels["track_vjp_kernel"] = vjp
        solve()
        torch.cuda.synchronize()
        ok = int((st <= 1).sum())
        for f in kernels.values():
            for _ in range(20):
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in kernels}
        for _ in range(args.rounds):
            for k, f in kernels.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    f()
                e1.record()
                e1.synchronize()
                times[k].append(1e3 * e0.elapsed_time(e1) / args.launches)
        if "track_vjp_kernel" in kernels:
            assert int((vst == 0).sum()) == ok, "adjoint failed on solved instances"
        print(f"B = {B}, N = {N} ({ok} of {B} solved), {args.launches} launches x {args.rounds} rounds, us per launch:")
        for k, v in times.items():
            print(f"  {k:26s} median {statistics.median(v):8.2f}   min {min(v):8.2f}   max {max(v):8.2f}")
        result[shape] = {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
