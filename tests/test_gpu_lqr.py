"""GPU suite: batched LQR terminal score (csrc/tt_lqr.hip, doubling algorithm) against the reference's
algorithm (LQR_cost.py: scipy.linalg.solve_discrete_are on the Euler linearisation at the goal).
Tolerance: the GPU P satisfies the DARE to a relative residual <= 1e-12, and agrees with scipy's P (and
score) to max(1e-9, 1e6 x scipy's own relative residual): at near-stationary goals (|v| ~ 0.01, P ~ 1e7)
the DARE is ill-conditioned and scipy's Schur solution carries residuals ~1e-11 while the doubling
iteration reaches ~1e-14, so the two differ at the 1e-7 level there.

The same comparison runs with non-diagonal weights (a dense symmetric Q, an R with an off-diagonal), which the terms
R^-1_01, R^-1_10 of G = B R^-1 B' and the off-diagonal of H_0 = Q need to be seen at all.  Then the kernel's own
plumbing: NULL P_out / iters, the batch size, and the exit that reports iters = -1."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P6 = {"M": 0.15, "L1": 7.05, "L2": 12.45, "W1": 3.05, "W2": 2.95, "dt": 0.05}


def _goals(golden_ref, B=96):
    rng = np.random.default_rng(9)
    xg = golden_ref["interp_states"].T[rng.integers(0, 400, B)].copy()
    xg[:, 5] = rng.uniform(-3, 3, B)          # goals with motion (well conditioned) ...
    xg[:8, 5] = rng.uniform(-0.05, 0.05, 8)   # ... and near-stationary ones (P up to ~1e7)
    xg[-1] = golden_ref["interp_states"][:, -1]   # the plan's own final state, as simulation.py:563 scores it
    xc = xg + rng.normal(scale=0.2, size=(B, 6))
    return xc, xg


def _dense_weights():
    """Q = I + 0.1 A A' (A from a fixed seed: symmetric, positive definite, every entry non-zero), R with an
    off-diagonal."""
    M = np.random.default_rng(17).normal(size=(6, 6))
    M = M @ M.T
    return np.eye(6) + 0.05 * (M + M.T), np.array([[10.0, 1.5], [1.5, 8.0]])   # (the product, symmetric to the bit)


def test_lqr_scores_match_scipy_dare(golden_ref):
    _scores_match_scipy_dare(golden_ref, np.eye(6), 10 * np.eye(2))


def test_lqr_scores_match_scipy_dare_dense_weights(golden_ref):
    Q, R = _dense_weights()
    assert np.array_equal(Q, Q.T) and np.min(np.abs(Q - np.diag(np.diag(Q)))[~np.eye(6, dtype=bool)]) > 1e-3
    _scores_match_scipy_dare(golden_ref, Q, R)


def _scores_match_scipy_dare(golden_ref, Q, R):
    from oracle import ttmpc_oracle as to
    from ttmpc import lqr
    xc, xg = _goals(golden_ref)
    B = xg.shape[0]
    s, P, it = lqr.lqr_scores(xc, xg, P6, Q, R)
    s, P, it = s.cpu().numpy(), P.cpu().numpy(), it.cpu().numpy()
    assert np.all(it > 0)
    def resid(Pm, x):
        A = np.eye(6) + P6["dt"] * to.jac_f(x, P6)
        Bm = P6["dt"] * to.B_F
        K = np.linalg.solve(R + Bm.T @ Pm @ Bm, Bm.T @ Pm @ A)
        return np.abs(A.T @ Pm @ A - Pm - A.T @ Pm @ Bm @ K + Q).max() / np.abs(Pm).max()
    for b in range(B):
        Pr = to.lqr_riccati(P6, Q, R, xg[b])
        assert resid(P[b], xg[b]) <= 1e-12, b
        rs = resid(Pr, xg[b])
        assert resid(P[b], xg[b]) <= max(1e-13, rs), b          # at least as accurate as scipy
        tol = max(1e-9, 1e6 * rs)                                 # forward error <= cond x residual
        assert np.max(np.abs(P[b] - Pr)) <= tol * np.max(np.abs(Pr)), b
        sr = float((xc[b] - xg[b]) @ Pr @ (xc[b] - xg[b]))
        assert abs(s[b] - sr) <= tol * abs(sr), b


def test_lqr_reference_signatures():
    from oracle import ttmpc_oracle as to
    from ttmpc import lqr
    xg = np.array([10.0, 5.0, 0.3, 0.1, 0.05, 1.5])
    xc = xg + 0.1
    d = lqr.lqr_distance(xc, xg, P6, None, np.eye(6), 10 * np.eye(2), np.zeros(2))
    assert d == pytest.approx(to.lqr_distance(xc, xg, P6, np.eye(6), 10 * np.eye(2)), rel=1e-9)
    P = lqr.lqr_riccati(P6, None, np.eye(6), 10 * np.eye(2), xg, np.zeros(2))
    assert np.allclose(P, P.T) and np.all(np.linalg.eigvalsh(P) > 0)


def _raw_scores(xc, xg, Q, R, want_P=True, want_iters=True):
    """tt_lqr_score_device itself, P_out and iters optional -> (score, P | None, iters | None) as arrays."""
    import torch
    from ttmpc._lib import lib
    from ttmpc.simulation import plant
    B = xg.shape[0]
    dev = torch.device("cuda")
    txc, txg = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (xc, xg))
    score = torch.full((B,), np.nan, dtype=torch.float64, device=dev)
    P = torch.full((B, 6, 6), np.nan, dtype=torch.float64, device=dev) if want_P else None
    it = torch.full((B,), -7, dtype=torch.int32, device=dev) if want_iters else None
    dp = C.POINTER(C.c_double)
    q = np.ascontiguousarray(np.asarray(Q, dtype=np.float64).reshape(36))
    r = np.ascontiguousarray(np.asarray(R, dtype=np.float64).reshape(4))
    p = plant(P6)
    rc = lib().tt_lqr_score_device(B, C.byref(p), q.ctypes.data_as(dp), r.ctypes.data_as(dp), txc.data_ptr(),
                                   txg.data_ptr(), None, P.data_ptr() if want_P else None, score.data_ptr(),
                                   it.data_ptr() if want_iters else None, None)
    assert rc == 0
    torch.cuda.synchronize()
    return score.cpu().numpy(), None if P is None else P.cpu().numpy(), None if it is None else it.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def test_lqr_optional_outputs_and_batch_size(golden_ref):
    """P_out = NULL and iters = NULL leave the scores bit for bit; an instance's numbers do not depend on the batch it
    is launched in (B = 1, B = 97 against the rows of a B = 192 launch)."""
    Q, R = _dense_weights()
    xc, xg = _goals(golden_ref)
    xc, xg = np.tile(xc, (2, 1)), np.tile(xg, (2, 1))
    s, P, it = _raw_scores(xc, xg, Q, R)
    assert np.all(np.isfinite(s)) and np.all(np.isfinite(P)) and np.all(it > 0)
    assert _same_bits(s[:96], s[96:]) and _same_bits(P[:96], P[96:]) and np.array_equal(it[:96], it[96:])
    for want_P, want_iters in ((False, True), (True, False), (False, False)):
        s2, P2, it2 = _raw_scores(xc, xg, Q, R, want_P, want_iters)
        assert _same_bits(s2, s)
        assert P2 is None or _same_bits(P2, P)
        assert it2 is None or np.array_equal(it2, it)
    for lo, hi in ((5, 6), (95, 192)):
        s3, P3, it3 = _raw_scores(xc[lo:hi], xg[lo:hi], Q, R)
        assert s3.shape[0] in (1, 97)
        assert _same_bits(s3, s[lo:hi]) and _same_bits(P3, P[lo:hi]) and np.array_equal(it3, it[lo:hi])


def test_lqr_unfinished_doubling_reports_minus_one(golden_ref):
    """iters = -1: the doubling has not met its stopping test after 64 steps.  A goal at standstill (v = 0) is not
    stabilisable in x and y, H grows with every doubling until rounding stops it near 1e11..1e13, and whether the
    iterate then sits still to the last bit or keeps moving in its low bits differs from goal to goal: on the CPU model
    (lqr_vjp_reference.doubling_dare) 2 of the first 32 goals below never stop, one more in the last bit of phi.  Which
    goals those are is a matter of each implementation's rounding, so the GPU's own are taken as it reports them: at
    least one of 96, each of them finite, every other instance with its count, and the well-conditioned neighbours,
    interleaved with them in one launch, bit for bit what a launch without them returns."""
    import lqr_vjp_reference as lr
    from oracle import ttmpc_oracle as to
    rng = np.random.default_rng(21)
    n = 96
    still = np.column_stack([rng.uniform(-20, 20, n), rng.uniform(-20, 20, n), rng.uniform(-3, 3, n),
                             rng.uniform(-1, 1, n), rng.uniform(-0.6, 0.6, n), np.zeros(n)])
    A = np.stack([np.eye(6) + P6["dt"] * to.jac_f(x, P6) for x in still])
    _, it_cpu = lr.doubling_dare(A, P6["dt"] * to.B_F, np.eye(6), 10 * np.eye(2))
    assert np.sum(it_cpu == -1) >= 1, "the CPU model has an instance that does not stop"
    xc_good, xg_good = _goals(golden_ref)
    xg_good, xc_good = xg_good[8:], xc_good[8:]          # the goals with motion
    m = xg_good.shape[0]
    xg = np.empty((n + m, 6))
    xc = np.empty((n + m, 6))
    pos_good = 2 * np.arange(m) + 1                       # every other slot, a standstill goal on either side
    pos_still = np.setdiff1d(np.arange(n + m), pos_good)
    xg[pos_still], xc[pos_still] = still, still + 0.1
    xg[pos_good], xc[pos_good] = xg_good, xc_good
    Q, R = np.eye(6), 10 * np.eye(2)
    s, P, it = _raw_scores(xc, xg, Q, R)
    s0, P0, it0 = _raw_scores(xc_good, xg_good, Q, R)
    print(f"standstill goals: doublings gpu {np.sort(it[pos_still]).tolist()}, cpu model {np.sort(it_cpu).tolist()}")
    assert np.all(it0 > 0) and np.all(it0 < 64)
    assert _same_bits(s[pos_good], s0) and _same_bits(P[pos_good], P0) and np.array_equal(it[pos_good], it0)
    its = it[pos_still]
    assert np.all((its == -1) | ((its > 0) & (its <= 64)))
    assert np.sum(its == -1) >= 1
    assert np.all(np.isfinite(P[pos_still])) and np.all(np.isfinite(s[pos_still]))
