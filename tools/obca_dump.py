"""Dump the OBCA kernel's outputs on fixed batches (development check: bitwise A/B of two builds).

    TTMPC_LIB=<build> python tools/obca_dump.py OUT.npz [B] [max_iter]
    python tools/obca_dump.py --compare A.npz B.npz      (exit status 1 when any array differs)
Solves the seed-0 cobs windows (B) and c4 plans (B/4) of the bench workloads and the N = 230, B = 8, max_iter 25 case
batch of tests/test_gpu_obca.py::test_hbm_source_sweeps_lockstep (the sweeps' HBM sources), and saves X, U, Z, status,
iters and kk of each.  OBCA_HELPERS=n sets the helper workgroups (0: none)."""
import json
import os
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO), str(REPO / "car-trailer-mpc_amd"), str(REPO / "tools")]
import numpy as np  # noqa: E402


def dump(out, B, max_iter):
    import ttmpc
    from obca_diag import G, workload
    from ttmpc import scenarios as sc

    def solver(N, params, bnd, obs, variant, max_iter):
        s = ttmpc.ObcaSolver(N, params, sc.OBCA_Q, sc.OBCA_R, *bnd, obs, variant=variant, max_iter=max_iter)
        if os.environ.get("OBCA_HELPERS"):  # helper workgroups: -1 one per CU (default), 0 none
            s.set_helpers(int(os.environ["OBCA_HELPERS"]))
        return s

    res = {}

    def keep(name, sol):
        X, U, Z, st, it, kk = sol
        res.update({f"{name}_X": X, f"{name}_U": U, f"{name}_Z": Z, f"{name}_st": st, f"{name}_it": it, f"{name}_kk": kk})
        print(name, "status", np.bincount(st, minlength=6).tolist(), "iters mean", float(it.mean()))

    for cfg, b in (("cobs", B), ("c4", max(1, B // 4))):
        P, data = workload(cfg, B=max(b, 8))
        data = {k: v[:b] for k, v in data.items()}
        variant = ttmpc.TT_VARIANT_TRACK_OBCA if cfg == "cobs" else ttmpc.TT_VARIANT_OBCA_PLAN
        s = solver(P["N"], P["params"], P["bnd"], P["obs"], variant, max_iter)
        if cfg == "cobs":
            keep(cfg, s.solve(data["x0"], xref=data["xref"], uref=data["uref"]))
        else:
            keep(cfg, s.solve(data["x0"], data["x_goal"], z_guess=data["z_guess"]))
    # N = 230: the sweeps' stage records no longer fit the LDS, every sweep reads its operands from the HBM workspace
    obs6 = sc.obstacles_array(sc.load_obstacles(G / "obstacles.json"))[:6]
    cases = json.loads((G / "test_cases.json").read_text())["cases"]
    x0, xg, zg = sc.obca_case_batch(cases, 8, 230, 6, seed=3, obstacles=obs6)
    s = solver(230, dict(sc.OBCA_PARAMS), (sc.OBCA_XLB, sc.OBCA_XUB, sc.OBCA_ULB, sc.OBCA_UUB), obs6,
               ttmpc.TT_VARIANT_OBCA_PLAN, 25)
    keep("n230", s.solve(x0, xg, z_guess=zg))
    np.savez(out, **res)


def compare(a, b):
    A, Bz = np.load(a), np.load(b)
    differ = sorted(set(A.files) ^ set(Bz.files))
    for k in differ:
        print(f"{k:10s} in one file only")
    for k in A.files:
        if k not in Bz.files:
            continue
        # bytes, not values: NaN == NaN and -0.0 != 0.0 here
        same = A[k].shape == Bz[k].shape and A[k].dtype == Bz[k].dtype and A[k].tobytes() == Bz[k].tobytes()
        d = np.abs(A[k].astype(float) - Bz[k].astype(float)).max() if A[k].shape == Bz[k].shape else float("nan")
        print(f"{k:10s} bitwise {same}  max|diff| {d:.3e}")
        if not same:
            differ.append(k)
    print(f"{len(A.files) - len([k for k in differ if k in A.files])} of {len(A.files)} arrays bitwise equal")
    return 1 if differ else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        dump(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 64, int(sys.argv[3]) if len(sys.argv) > 3 else 400)
