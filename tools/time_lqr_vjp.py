"""Launch times of the LQR score and of its adjoint on the same inputs.

    timeout 120 python tools/time_lqr_vjp.py [--batch 4096] [--launches 200] [--rounds 5]

One GPU process.  The goals are those of tests/test_gpu_lqr.py (seed 9: states of the committed plan with v drawn from
U(-3, 3), eight near-stationary ones and the plan's final state) tiled to the batch, Q = I + 0.1 diag(0..5),
R = [[10, 1], [1, 8]], both upstream gradients given.  After a warm-up of each, `--rounds` rounds alternate `--launches`
back-to-back tt_lqr_score_device calls and as many tt_lqr_score_vjp_device calls into preallocated outputs, each between
two device events, with no host synchronisation inside.  Prints the median and the min..max over the rounds in
microseconds per launch and one JSON line.
"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO), str(REPO / "car-trailer-mpc_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    import numpy as np
    import torch

    import ttmpc
    from ttmpc._lib import TTLqrVjpOut
    from ttmpc.simulation import plant

    if not torch.cuda.is_available():
        sys.exit("time_lqr_vjp: no GPU (timings are taken on the device only)")
    B = args.batch
    params = {"M": 0.15, "L1": 7.05, "L2": 12.45, "W1": 3.05, "W2": 2.95, "dt": 0.05}
    g = np.load(REPO / "tests" / "golden" / "reference_numpy.npz")
    rng = np.random.default_rng(9)
    xg = g["interp_states"].T[rng.integers(0, 400, 96)].copy()
    xg[:, 5] = rng.uniform(-3, 3, 96)
    xg[:8, 5] = rng.uniform(-0.05, 0.05, 8)
    xg[-1] = g["interp_states"][:, -1]
    xc = xg + rng.normal(scale=0.2, size=(96, 6))
    rep = B // 96 + 1
    dev = torch.device("cuda", 0)
    f64 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64).to(dev)  # noqa: E731
    txc, txg = f64(np.tile(xc, (rep, 1))[:B]), f64(np.tile(xg, (rep, 1))[:B])
    new = lambda *s, dtype=torch.float64: torch.empty(s, dtype=dtype, device=dev)  # noqa: E731
    P, score, it = new(B, 6, 6), new(B), new(B, dtype=torch.int32)
    gs, GP = f64(rng.uniform(-1, 1, B)), f64(rng.uniform(-1, 1, (B, 6, 6)))
    outs = [new(B, 6), new(B, 6), new(B, 6, 6), new(B, 2, 2), new(B, dtype=torch.int32), new(B, dtype=torch.int32)]
    o = TTLqrVjpOut(*[t.data_ptr() for t in outs])
    Q = np.ascontiguousarray((np.eye(6) + 0.1 * np.diag(np.arange(6.0))).reshape(36))
    R = np.ascontiguousarray(np.array([10.0, 1.0, 1.0, 8.0]))
    dp = C.POINTER(C.c_double)
    L, p = ttmpc.lib(), plant(params)
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def fwd():
        return L.tt_lqr_score_device(B, C.byref(p), Q.ctypes.data_as(dp), R.ctypes.data_as(dp), txc.data_ptr(),
                                     txg.data_ptr(), None, P.data_ptr(), score.data_ptr(), it.data_ptr(), s)

    def vjp():
        return L.tt_lqr_score_vjp_device(B, C.byref(p), R.ctypes.data_as(dp), txc.data_ptr(), txg.data_ptr(),
                                         P.data_ptr(), it.data_ptr(), gs.data_ptr(), GP.data_ptr(), C.byref(o), s)

    def timed(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            if fn() != 0:
                sys.exit("time_lqr_vjp: a launch failed")
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) / n * 1e3

    for fn in (fwd, vjp):
        timed(fn, 20)
    t = {"forward": [], "vjp": []}
    for _ in range(args.rounds):
        t["forward"].append(timed(fwd, args.launches))
        t["vjp"].append(timed(vjp, args.launches))
    ok = int((outs[4] == 0).sum())
    res = {"batch": B, "launches": args.launches, "rounds": args.rounds, "vjp_ok": ok,
           "forward_doublings": [int(it.min()), int(it.max())], "vjp_doublings": [int(outs[5].min()), int(outs[5].max())]}
    for k, v in t.items():
        res[k + "_us"] = {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
        print(f"{k:8s}: {statistics.median(v):8.2f} us per launch ({min(v):.2f}..{max(v):.2f})")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
