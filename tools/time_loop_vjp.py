"""Step times of the differentiable closed loop: the taped forward, the plain forward, the backward sweep.

    timeout 300 python tools/time_loop_vjp.py [--batch 1024] [--horizon 20] [--steps 50] [--rounds 5]

One GPU process.  The loop is bench.py --config sim's (the committed plan at 0.05 s, disturbed plant, noisy measurements,
B starts around the plan's start) without the collision check.  After a warm-up of each, `--rounds` rounds alternate
  * the K steps of ClosedLoop.run_tape   (step with multiplier export + the tape copies),
  * the K steps of ClosedLoop.run        (plain step + the log copies),
  * ClosedLoop.backward on the tape just made,
and the same three for a rule loop: the same solver variant, plan, noise and starts with
ClosedLoop(..., fuzzy_rule=FuzzyRule()), whose weights come from the fuzzy rule each step and whose backward step ends
in the fused window + rule adjoint (its taped forward step also has the retry's host compaction and two more copies);
each between two device events on the stream it runs on, with no host synchronisation inside the backward.  Prints the
median and the min..max over the rounds in microseconds per step, the ratio taped / plain, and one JSON line.
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
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()

    import numpy as np
    import torch

    import ttmpc
    from ttmpc import scenarios as sc
    from ttmpc import simulation as sim

    if not torch.cuda.is_available():
        sys.exit("time_loop_vjp: no GPU (timings are taken on the device only)")
    B, N, K = args.batch, args.horizon, args.steps
    dev = torch.device("cuda")
    g = np.load(REPO / "tests" / "golden" / "reference_numpy.npz")
    S, U = g["interp_states"], g["interp_inputs"]
    params = dict(sc.PARAMS, horizon=N)
    rng = np.random.default_rng(0)
    x0 = S[:, 0][None] + rng.normal(scale=[0.3, 0.3, 0.02, 0.02, 0.0, 0.0], size=(B, 6))
    T = (K - 0.5) * params["dt"]
    assert len(sim.step_indices(T, params["dt"])) == K
    noise = torch.from_numpy(rng.normal(scale=0.02, size=(K, B, 6))).to(dev)
    w = torch.from_numpy(rng.uniform(0.7, 1.4, (B, 8))).to(dev)
    GS = torch.from_numpy(rng.uniform(-1, 1, (K + 1, B, 6))).to(dev)
    GU = torch.from_numpy(rng.uniform(-1, 1, (K, B, 2))).to(dev)
    solver = ttmpc.BatchSolver(N, params, sc.MPC_Q, sc.MPC_R, sc.XLB, sc.XUB, sc.ULB, sc.UUB)
    cl = sim.ClosedLoop(solver, S, U, params, sim.DISTURBANCE_PARAMS)
    rule_solver = ttmpc.BatchSolver(N, params, sc.MPC_Q, sc.MPC_R, sc.XLB, sc.XUB, sc.ULB, sc.UUB)
    rl = sim.ClosedLoop(rule_solver, S, U, params, sim.DISTURBANCE_PARAMS, fuzzy_rule=sim.FuzzyRule())

    def timed(stream, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = fn()
        e1.record(stream)
        e1.synchronize()
        return 1e3 * e0.elapsed_time(e1) / K, out

    def forward(taped, loop=cl):
        """run_tape()'s / run()'s steps (step + the nine / six log copies; a rule loop: eleven) without the host copies
        at the end."""
        log, drawn = loop._begin(x0, T, noise, w if loop.rule is None else None, taped=taped)
        us, _ = timed(loop.stream, lambda: loop._steps(log, drawn))
        return us, log

    def backward(tape, loop=cl):
        return timed(torch.cuda.current_stream(dev), lambda: loop.backward(tape, GS, GU, rule=loop.rule is not None))

    _, tape = forward(True)
    forward(False)
    _, grads = backward(tape)
    _, rtape = forward(True, rl)
    forward(False, rl)
    _, rgrads = backward(rtape, rl)
    torch.cuda.synchronize()
    ok, rok, retried = int((tape.status <= 1).sum()), int((rtape.status <= 1).sum()), int(rtape.retried.sum())
    times = {"taped forward step": [], "plain forward step": [], "backward step": [],
             "rule loop: taped forward step": [], "rule loop: plain forward step": [], "rule loop: backward step": []}
    for _ in range(args.rounds):
        us, tape = forward(True)
        times["taped forward step"].append(us)
        times["plain forward step"].append(forward(False)[0])
        times["backward step"].append(backward(tape)[0])
        us, rtape = forward(True, rl)
        times["rule loop: taped forward step"].append(us)
        times["rule loop: plain forward step"].append(forward(False, rl)[0])
        times["rule loop: backward step"].append(backward(rtape, rl)[0])
    assert bool(torch.isfinite(grads["g_x_init"]).all()) and bool(torch.isfinite(rgrads["g_fuzzy_rule"]).all())
    print(f"B = {B}, N = {N}, K = {K} ({ok} of {K * B} solves succeeded; rule loop {rok}, {retried} retried), "
          f"{args.rounds} rounds, us per step; tape {tape.nbytes() / 2**20:.1f} MiB, rule loop "
          f"{rtape.nbytes() / 2**20:.1f} MiB:")
    for k, v in times.items():
        print(f"  {k:30s} median {statistics.median(v):8.2f}   min {min(v):8.2f}   max {max(v):8.2f}")
    ratio = statistics.median(times["taped forward step"]) / statistics.median(times["plain forward step"])
    print(f"  taped / plain {ratio:.3f}")
    result = {k: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for k, v in times.items()}
    result["taped_over_plain"] = ratio
    rratio = (statistics.median(times["rule loop: taped forward step"]) /
              statistics.median(times["rule loop: plain forward step"]))
    bratio = statistics.median(times["rule loop: backward step"]) / statistics.median(times["backward step"])
    print(f"  rule loop: taped / plain {rratio:.3f}, backward step rule / plain {bratio:.3f}")
    result["rule_taped_over_plain"], result["rule_backward_over_plain_backward"] = rratio, bratio

    # the four launches of a backward step on their own: 200 back-to-back launches each, median of the rounds
    import ctypes as C
    cur = torch.cuda.current_stream(dev)
    z = lambda *sh: torch.zeros(sh, dtype=torch.float64, device=dev)  # noqa: E731
    a, abar, gU, xref, uref = z(B, 6), z(B, 2), z(B, N, 2), z(B, N + 1, 6), z(B, N, 2)
    g0, gxr, gur, gws, gw = z(B, 6), z(B, N + 1, 6), z(B, N, 2), z(B, 8), z(B, 8)
    Np = tape.plan_u.shape[-2]
    gpx, gpu_ = z(B, Np + 1, 6), z(B, Np, 2)
    t, L = K // 2, ttmpc.lib()
    pl, sp = sim.plant(params, sim.DISTURBANCE_PARAMS), C.c_void_p(cur.cuda_stream)
    rstruct, gth = sim.FuzzyRule().as_struct(), z(B, 7)
    parts = {
        "policy_plant_vjp_kernel": lambda: L.tt_policy_plant_vjp_device(
            B, N, C.byref(pl), 0, tape.S[t].data_ptr(), tape.status[t].data_ptr(), tape.active[t - 1].data_ptr(),
            tape.active[t].data_ptr(), tape.consec[t].data_ptr(), GU[t].data_ptr(), a.data_ptr(), abar.data_ptr(),
            gU.data_ptr(), None, sp),
        "sim_window_kernel": lambda: L.tt_sim_window_device(
            B, N, tape.ks[t], Np, tape.plan_x.data_ptr(), tape.plan_u.data_ptr(), 0, None, None, None, xref.data_ptr(),
            uref.data_ptr(), sp),
        "track_vjp_kernel": lambda: solver.vjp_device(
            B, tape.X[t].data_ptr(), tape.U[t].data_ptr(), tape.dual[t].data_ptr(), xref.data_ptr(), uref.data_ptr(),
            tape.status[t].data_ptr(), grad_u=gU.data_ptr(), g_x0=g0.data_ptr(), g_xref=gxr.data_ptr(),
            g_uref=gur.data_ptr(), g_wq_wr=gws.data_ptr(), wq_wr=w.data_ptr(), stream=cur.cuda_stream),
        "sim_window_vjp_kernel": lambda: L.tt_sim_window_vjp_device(
            B, N, tape.ks[t], Np, gxr.data_ptr(), gur.data_ptr(), gpx.data_ptr(), gpu_.data_ptr(), g0.data_ptr(),
            GS[t].data_ptr(), a.data_ptr(), gws.data_ptr(), gw.data_ptr(), None, sp),
        "sim_window_vjp_fuzzy_kernel": lambda: L.tt_sim_window_vjp_fuzzy_device(
            B, N, tape.ks[t], Np, gxr.data_ptr(), gur.data_ptr(), gpx.data_ptr(), gpu_.data_ptr(), g0.data_ptr(),
            GS[t].data_ptr(), a.data_ptr(), gws.data_ptr(), gw.data_ptr(), None, C.byref(rstruct), rtape.S[t].data_ptr(),
            xref.data_ptr(), rtape.retried[t].data_ptr(), gth.data_ptr(), sp),
    }
    n = 200
    print(f"  the launches of one backward step alone ({n} back to back), us per launch:")
    for name, fn in parts.items():
        for _ in range(20):
            fn()
        v = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            e1.synchronize()
            v.append(1e3 * e0.elapsed_time(e1) / n)
        print(f"    {name:26s} median {statistics.median(v):8.2f}   min {min(v):8.2f}   max {max(v):8.2f}")
        result[name] = {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
