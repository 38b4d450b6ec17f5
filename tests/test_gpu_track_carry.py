"""GPU suite: the register-carried stage state of the stage-unrolled one-wave track_kernel builds.

The one-wave builds of N = 20, 30, 40 and the all-LDS build of N = 50 keep each lane's own x, z_L, z_U, slacks, slack
reciprocals, step and y+ in registers between the stage-parallel passes and fold the Riccati operands from registers.
The arithmetic is the same, so they must stay bitwise the builds that keep the LDS round trips: the two-wave builds
(N = 20, 30; B > 2048) and the HBM-band build of N = 50 (more than three instances per CU).  The
batches of tests/test_gpu_parity.py converge in 5-8 iterations on the straight path; the hard batch below starts far
from the reference, so that on the CPU oracle (one thread):

    s     N   statuses              iterations  line searches not accepted
    0.25  20  96 x 0                5-9         -
    0.25  30  96 x 0                5-9         -
    0.5   20  93 x 0, 3 x 4         up to 57    52
    0.5   30  94 x 0, 2 x 4         up to 52    25  (and one accepted second-order correction)
    0.5   40  95 x 0, 1 x 4         up to 39    not counted  (no build that keeps the round trips: oracle test only)
    0.5   50  93 x 0, 3 x 4         6-57        not counted  (18 instances take more than 9 iterations)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = {"M": 0.15, "L1": 7.05, "L2": 12.45, "W1": 3.05, "W2": 2.95, "dt": 0.05}
_CACHE = {}


def _gpu_solver(N):
    import ttmpc
    from oracle import ttmpc_oracle as to
    return ttmpc.BatchSolver(N, P, to.DEFAULT_Q, to.DEFAULT_R, to.MPC_XLB, to.MPC_XUB, to.MPC_ULB, to.MPC_UUB)


def hard_batch(N, s, seed=11):
    """96 instances: synthetic_batch(seed, psi 0.9) with x0 pushed away by s * N(0, 1) * (4, 4, .8, .6, .5, 5),
    clipped to 0.98 x the finite MPC bounds."""
    key = (N, s, seed)
    if key not in _CACHE:
        from oracle import ttmpc_oracle as to
        from ttmpc.scenarios import synthetic_batch
        x0, xr, ur = synthetic_batch(96, N, seed=seed, psi_range=0.9)
        x0 = x0 + s * np.random.default_rng(5).normal(0, 1, (96, 6)) * np.array([4, 4, 0.8, 0.6, 0.5, 5])
        lb, ub = np.asarray(to.MPC_XLB, dtype=float), np.asarray(to.MPC_XUB, dtype=float)
        lo = np.where(np.isfinite(lb), 0.98 * lb, -np.inf)
        hi = np.where(np.isfinite(ub), 0.98 * ub, np.inf)
        x0 = np.clip(x0, lo, hi)
        for a in (x0, xr, ur):
            a.setflags(write=False)
        _CACHE[key] = (x0, xr, ur)
    return _CACHE[key]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _assert_tiles_bitwise(big, small, reps, tag):
    """every output of every 96-instance copy inside `big` equals `small`, bit pattern for bit pattern (NaN == NaN)"""
    names = ("X", "U", "status", "iters", "kkt")
    for r in range(reps):
        for name, a, b in zip(names, big, small):
            assert np.array_equal(_bits(a[96 * r:96 * (r + 1)]), _bits(b)), (tag, name, r)


def _reps_past_three_per_cu():
    """copies of the 96 that make the first multiple of 96 above three instances per CU (9, B = 864, on 256 CUs)"""
    import torch
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return 3 * cus // 96 + 1


@pytest.mark.parametrize("N", [20, 30, 50])
def test_hard_batch_is_bitwise_across_builds(N):
    """s = 0.5 tiled 22 times (B = 2112: the two-wave build, which keeps the LDS round trips) against the same 96
    solved alone (the one-wave build with the carried state): rejected line searches, the second-order correction
    and the non-finite exits included.  N = 50: tiled past three instances per CU (the HBM-band build, which keeps
    the LDS and HBM round trips) against the 96 alone (the all-LDS carried build) -- the same comparison for the
    one-stage-per-lane slot mapping."""
    x0, xr, ur = hard_batch(N, 0.5)
    s = _gpu_solver(N)
    reps = _reps_past_three_per_cu() if N == 50 else 22
    small = s.solve(x0, xr, ur)
    big = s.solve(np.tile(x0, (reps, 1)), np.tile(xr, (reps, 1, 1)), np.tile(ur, (reps, 1, 1)))
    st, it = small[2], small[3]
    print(f"N={N} B={96 * reps} status counts {np.bincount(st, minlength=6).tolist()} iters max {int(it.max())}")
    assert it.max() > 9, "the batch no longer leaves the straight path"
    _assert_tiles_bitwise(big, small, reps, N)


# instances on which the build before the carried state already disagreed with the oracle: (N, index) -> its numbers
# (none: that build meets the tolerance on all 96 at every N, with the same figures to the printed digit)
PARENT_DISAGREES = {}


@pytest.mark.parametrize("N", [20, 30, 40, 50])
def test_hard_batch_matches_c_oracle(N):
    """s = 0.25 against c_oracle.solve_batch: identical status, |dz| <= 1e-7 * max(1, |z|) on X and U (the tolerance of
    test_matches_c_oracle)."""
    from oracle import c_oracle as co
    from oracle import ttmpc_oracle as to
    x0, xr, ur = hard_batch(N, 0.25)
    X, U, st, it, kk = _gpu_solver(N).solve(x0, xr, ur)
    nlp = to.TrackingNLP(N)
    Pp = co.make_problem(N, P, nlp.Q, nlp.R, nlp.xlb, nlp.xub, nlp.ulb, nlp.uub)
    zc, stc, itc, kkc = co.solve_batch(Pp, x0, xr, ur)
    from ttmpc import layout
    Xc, Uc = layout.unpack(zc, N)
    assert np.all(stc == 0), "the oracle converges on all 96"
    skip = sorted(i for (n, i) in PARENT_DISAGREES if n == N)
    assert len(skip) <= 5
    keep = np.setdiff1d(np.arange(96), skip)
    ex = np.max(np.abs(X - Xc) / np.maximum(1.0, np.abs(Xc)), axis=(1, 2))
    eu = np.max(np.abs(U - Uc) / np.maximum(1.0, np.abs(Uc)), axis=(1, 2))
    print(f"N={N} iters gpu {int(it.min())}-{int(it.max())} oracle {int(itc.min())}-{int(itc.max())} "
          f"max rel dX {ex[keep].max():.3e} dU {eu[keep].max():.3e} "
          f"max abs dX {np.abs(X - Xc)[keep].max():.3e} dU {np.abs(U - Uc)[keep].max():.3e}")
    assert np.array_equal(st[keep], stc[keep])
    assert ex[keep].max() <= 1e-7 and eu[keep].max() <= 1e-7


@pytest.mark.parametrize("N,seed", [(20, 11), (30, 12)])
def test_inertia_retry_batch_and_repeat_call(N, seed):
    """The s = 0.25 and 0.5 batches never take an inertia retry (stamped build of the parent commit: #riccati equals
    #iterations on every instance).  At s = 2.0 they do, on that build: N = 20, seed 11 -- instances 30 and 82, three
    extra factorisations each (80 converge, 16 end non-finite); N = 30, seed 12 -- nine instances, up to 31 extra
    factorisations (74 / 22).  ric_gu_shift re-reads the folded rows the register-fed tail wrote, so the carried
    build (96 alone) must stay bitwise the two-wave build (tiled to B = 2112) there too.  Two consecutive solves on
    one handle return identical bits: nothing of the carried state survives a launch."""
    x0, xr, ur = hard_batch(N, 2.0, seed)
    s = _gpu_solver(N)
    first = s.solve(x0, xr, ur)
    second = s.solve(x0, xr, ur)
    for a, b in zip(first, second):
        assert np.array_equal(_bits(a), _bits(b))
    print(f"N={N} status counts {np.bincount(first[2], minlength=6).tolist()} iters max {int(first[3].max())}")
    big = s.solve(np.tile(x0, (22, 1)), np.tile(xr, (22, 1, 1)), np.tile(ur, (22, 1, 1)))
    _assert_tiles_bitwise(big, first, 22, N)


def test_n50_hbm_band_hard_batch_is_bitwise_the_lds_build():
    """s = 0.25 at N = 50 tiled 11 times (B = 1056, above three instances per CU: the HBM-band build, which keeps the
    Sigma / dB rows and every LDS round trip) against the same 96 solved alone (the all-LDS build with the carried
    state)."""
    N = 50
    x0, xr, ur = hard_batch(N, 0.25)
    s = _gpu_solver(N)
    small = s.solve(x0, xr, ur)
    big = s.solve(np.tile(x0, (11, 1)), np.tile(xr, (11, 1, 1)), np.tile(ur, (11, 1, 1)))
    _assert_tiles_bitwise(big, small, 11, N)
