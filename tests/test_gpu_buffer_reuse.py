"""GPU suite: the handle-owned device buffers grow and are reused across calls of one handle.

A handle keeps grow-only device blocks (the staging block of the host calls, the multiplier workspace, the OBCA
workspace and board).  A call at a larger B replaces them, a later smaller call reuses the larger block at other
offsets: neither may change a result.  Every sequence is small -> large -> small on ONE handle, and the first and the
third call must agree to the bit in every array.
"""
import numpy as np
import pytest

import sens_reference as sr
from test_obca_oracle import P6, toy_plan

pytestmark = pytest.mark.gpu

P = sr.P


def _track_call(s, x0, xr, ur, w):
    """solve_ex with every extra output and vjp (with the model gradient, so that every field of its result is an
    array) on its outputs: all arrays of both results, by name."""
    r = s.solve_ex(x0, xr, ur, wq_wr=w, duals=True, gain=True, trajectory_sens=True)
    rng = np.random.default_rng(11)  # the same upstream gradient per instance at every B: rows are drawn in order
    gx, gu = rng.standard_normal((5,) + r.X.shape[1:])[:len(x0)], rng.standard_normal((5,) + r.U.shape[1:])[:len(x0)]
    v = s.vjp(r.X, r.U, r.dual, xr, ur, r.status, gx, gu, wq_wr=w, model=True)
    out = {k: getattr(r, k) for k in r.__slots__}
    out.update({k: getattr(v, k) for k in v.__slots__})
    assert all(a is not None for a in out.values())
    return out


def _track_sequence(N, variant, weights):
    import ttmpc
    from oracle import ttmpc_oracle as to
    from ttmpc.scenarios import synthetic_batch
    nlp = to.TrackingNLP(N, params=dict(P, horizon=N))
    x0, xr, ur = synthetic_batch(5, N, seed=70 + N, psi_range=0.3)
    w = None
    if weights:
        w = np.empty((5, 8))
        for b in range(5):
            w[b, :6], w[b, 6:] = to.fuzzy_weights(x0[b], xr[b].T)
    s = ttmpc.BatchSolver(N, P, nlp.Q, nlp.R, nlp.xlb, nlp.xub, nlp.ulb, nlp.uub, variant=variant)
    cut = lambda n: (x0[:n], xr[:n], ur[:n], None if w is None else w[:n])  # noqa: E731
    first, second, third = _track_call(s, *cut(2)), _track_call(s, *cut(5)), _track_call(s, *cut(2))
    s.close()
    assert np.all(second["status"] <= 1) and np.all(second["sens_status"] == 0) and np.all(second["vjp_status"] == 0)
    for k in first:
        assert first[k].dtype == third[k].dtype and np.array_equal(first[k], third[k]), k
        assert np.array_equal(first[k], second[k][:2]), k


@pytest.mark.parametrize("weights", [False, True], ids=["track", "fuzzy"])
def test_tracking_buffers_grow_and_are_reused(weights):
    import ttmpc
    _track_sequence(3, ttmpc.TT_VARIANT_FUZZY if weights else ttmpc.TT_VARIANT_TRACK, weights)


@pytest.mark.parametrize("N", [1, 65])
def test_tracking_buffers_single_stage_and_wrapped_lanes(N):
    """N = 1: one input stage, no P update, p_0 straight from stage 0.  N = 65: the stage-parallel loops wrap the 64
    lanes, and the solve is above the zero-copy limit, so it takes the copy path."""
    import ttmpc
    _track_sequence(N, ttmpc.TT_VARIANT_TRACK, False)


def test_obca_buffers_grow_and_are_reused():
    import ttmpc
    from ttmpc import scenarios as sc
    N, _, obs, x0, xg, zg = toy_plan()
    s = ttmpc.ObcaSolver(N, P6, sc.OBCA_Q, sc.OBCA_R, sc.OBCA_XLB, sc.OBCA_XUB, sc.OBCA_ULB, sc.OBCA_UUB, obs)
    s_iterate_len = int(ttmpc.lib().tt_obca_iterate_len(N, len(obs)))
    rep = lambda a, n: np.repeat(a[:1], n, axis=0)  # noqa: E731
    first = s.solve(rep(x0, 1), rep(xg, 1), z_guess=rep(zg, 1))
    second = s.solve(rep(x0, 3), rep(xg, 3), z_guess=rep(zg, 3))
    third = s.solve(rep(x0, 1), rep(xg, 1), z_guess=rep(zg, 1), iterate=True)
    s.close()
    assert first[3][0] == 0
    for a, b in zip(first, third[:6]):  # X, U, Z, status, iters, kkt
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert third[6].shape == (1, s_iterate_len)
    assert np.all(second[3] == second[3][0]) and np.all(second[4] == second[4][0])
