"""GPU suite: the Riccati sweep's stage loop at the shapes where its structure changes.

phase_riccati runs two stages per trip with ping-pong operand buffers, a stage-0 tail for odd horizons and, in the generic
(run-time horizon) builds, a prefetch of stage -1 on the last trip.  Horizons 1, 2 and 3 are a single stage, one even trip
and one trip plus the tail.  Each horizon runs under the four bound patterns that select the four kinds of generic build:
the MPC pattern with diagonal and with non-diagonal weights, the OBCA pattern, and a pattern that is neither, which takes
the build that reads its bounds at run time.  Every case is compared with the C oracle on identical inputs: identical
statuses, |dz| <= 1e-7 * max(1, |z|) (the tolerance of tests/test_gpu_parity.py::test_matches_c_oracle).

The inertia-retry batches (tests/test_gpu_track_carry.py's hard start at s = 2) make ric_gu_shift rewrite the g_u' rows the
sweep prefetches.  At N = 20 the one-wave build must stay bitwise the two-wave build; at N = 3 (a generic build: no second
build to compare with) two solves on one handle must return identical bits, and the instances on which the oracle
converges must agree with it.
"""
import numpy as np
import pytest

from test_gpu_track_carry import _assert_tiles_bitwise, _bits, _gpu_solver, hard_batch
from track_patterns import patterns as _patterns

pytestmark = pytest.mark.gpu

P = {"M": 0.15, "L1": 7.05, "L2": 12.45, "W1": 3.05, "W2": 2.95, "dt": 0.05}
B = 8


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


@pytest.mark.parametrize("pattern", ["mpc_diag", "mpc_full", "obca", "run_time"])
@pytest.mark.parametrize("N", [1, 2, 3])
def test_short_horizons_match_c_oracle(N, pattern):
    import ttmpc
    from oracle import c_oracle as co
    from ttmpc import layout
    from ttmpc.scenarios import synthetic_batch
    Q, R, xlb, xub, ulb, uub = _patterns()[pattern]
    x0, xr, ur = synthetic_batch(B, N, seed=1000 + N, psi_range=0.3)
    X, U, st, it, kk = ttmpc.BatchSolver(N, P, Q, R, xlb, xub, ulb, uub).solve(x0, xr, ur)
    zc, stc, itc, kkc = co.solve_batch(co.make_problem(N, P, Q, R, xlb, xub, ulb, uub), x0, xr, ur)
    err = _rel(layout.pack(X, U), zc)
    print(f"N={N} {pattern}: status {st.tolist()} oracle {stc.tolist()} iters {it.tolist()} max rel dz {err:.3e}")
    assert np.array_equal(st, stc)
    assert np.all(st == 0)
    assert err <= 1e-7


def test_inertia_retry_batch_n20_is_bitwise_the_two_wave_build():
    x0, xr, ur = hard_batch(20, 2.0, 11)
    s = _gpu_solver(20)
    small = s.solve(x0, xr, ur)
    big = s.solve(np.tile(x0, (22, 1)), np.tile(xr, (22, 1, 1)), np.tile(ur, (22, 1, 1)))
    print(f"N=20 status counts {np.bincount(small[2], minlength=6).tolist()} iters max {int(small[3].max())}")
    _assert_tiles_bitwise(big, small, 22, 20)


def test_inertia_retry_batch_n3():
    from oracle import c_oracle as co
    from oracle import ttmpc_oracle as to
    from ttmpc import layout
    N = 3
    x0, xr, ur = hard_batch(N, 2.0, 11)
    s = _gpu_solver(N)
    first = s.solve(x0, xr, ur)
    second = s.solve(x0, xr, ur)
    for a, b in zip(first, second):
        assert np.array_equal(_bits(a), _bits(b))
    X, U, st, it, kk = first
    nlp = to.TrackingNLP(N)
    zc, stc, itc, kkc = co.solve_batch(co.make_problem(N, P, nlp.Q, nlp.R, nlp.xlb, nlp.xub, nlp.ulb, nlp.uub), x0, xr, ur)
    ok = stc == 0
    err = _rel(layout.pack(X, U)[ok], zc[ok])
    print(f"N=3 status counts gpu {np.bincount(st, minlength=6).tolist()} oracle {np.bincount(stc, minlength=6).tolist()} "
          f"iters max {int(it.max())} max rel dz on the oracle's converged {err:.3e}")
    assert ok.sum() >= 48, "the batch no longer has a converged half to compare"
    assert np.array_equal(st, stc)
    assert err <= 1e-7
