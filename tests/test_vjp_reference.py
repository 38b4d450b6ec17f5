"""CPU suite: the adjoint references of tests/vjp_reference.py pinned against the CPU oracle, no GPU.

* ``dense_vjp`` agrees with central finite differences (h = 1e-4) of ``c_oracle.solve_batch`` in x_init, xref, uref and
  the weights to <= 1e-6 absolute, for L = g . z with a fixed random g, on the free input set with and without weights.
* ``riccati_vjp`` (the CPU model of track_vjp_kernel) and ``dense_vjp`` are the same linear algebra: on an interior
  primal-dual point of both input sets they agree to 10 eps cond(K) max|ref|.
* Both once more under the non-diagonal ``mpc_full`` weights of tests/track_patterns.py, weighted, at the same bounds:
  the symmetrised off-diagonal terms and the cross terms of the weight gradient.
* dL/dxref[0] is exactly 0 (x_0 is pinned), and a loss on x_0 alone gives dL/dx_init = gX_0 exactly.
"""
import numpy as np
import pytest

import sens_reference as sr
import vjp_reference as vr


def _interior_dual(nlp, z, y, mu=1e-9):
    """y of the optimum, z = mu / slack on every finite (relaxed) bound: the export layout (N+1, 22)."""
    N = nlp.N
    lbr, ubr = sr.relaxed_bounds(nlp)
    assert np.all(z > lbr) and np.all(z < ubr)
    with np.errstate(divide="ignore"):
        zl = np.where(np.isfinite(lbr), mu / (z - lbr), 0.0)
        zu = np.where(np.isfinite(ubr), mu / (ubr - z), 0.0)
    dual = np.zeros((N + 1, 22))
    dual[:, :6] = y
    dual[:N, 6:14], dual[N, 6:12] = zl[:8 * N].reshape(N, 8), zl[8 * N:]
    dual[:N, 14:22], dual[N, 14:20] = zu[:8 * N].reshape(N, 8), zu[8 * N:]
    return dual


@pytest.mark.parametrize("weighted", [False, True])
def test_dense_vjp_matches_oracle_finite_differences(weighted):
    nlp, x0, xr, ur = sr.case_free()
    B, N = x0.shape[0], nlp.N
    w = vr.random_weights(B) if weighted else None
    gX, gU = vr.random_upstream(B, N)
    z, st, fd = vr.oracle_fd_vjp(nlp, x0, xr, ur, gX, gU, w=w, h=1e-4)
    assert np.all(st == 0)
    worst = big = 0.0
    for b in range(B):
        wq, wr = (None, None) if w is None else (w[b, :6], w[b, 6:])
        y = nlp.kkt_residual(z[b], x0[b], xr[b].T, ur[b].T, wq, wr)["y"].reshape(N + 1, 6)
        ref = vr.dense_vjp(nlp, z[b], _interior_dual(nlp, z[b], y), xr[b], ur[b], gX[b], gU[b], wq, wr)
        errs = {k: float(np.max(np.abs(fd[b][k] - ref[k]))) for k in vr.KEYS}
        print(f"weighted={weighted} instance {b}: FD vs dense " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items())
              + f", max|grad| {vr.max_abs(ref):.3f}")
        worst, big = max(worst, max(errs.values())), max(big, vr.max_abs(ref))
    print(f"weighted={weighted}: worst {worst:.3e}, largest gradient entry {big:.3f}")
    assert worst <= 1e-6
    assert big > 1e-3


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("case", ["free", "active"])
def test_riccati_vjp_is_the_dense_solve(case, weighted):
    from oracle import c_oracle as co
    nlp, x0, xr, ur = sr.case_free() if case == "free" else sr.case_active()
    B, N = x0.shape[0], nlp.N
    w = vr.random_weights(B) if weighted else None
    gX, gU = vr.random_upstream(B, N)
    z, st, _, _ = co.solve_batch(sr.oracle_problem(nlp), x0, xr, ur, wq=None if w is None else w[:, :6],
                                 wr=None if w is None else w[:, 6:])
    for b in range(0, B, 2):
        wq, wr = (None, None) if w is None else (w[b, :6], w[b, 6:])
        y = nlp.kkt_residual(z[b], x0[b], xr[b].T, ur[b].T, wq, wr)["y"].reshape(N + 1, 6)
        dual = _interior_dual(nlp, z[b], y)
        dense = vr.dense_vjp(nlp, z[b], dual, xr[b], ur[b], gX[b], gU[b], wq, wr)
        model = vr.riccati_vjp(nlp, z[b], dual, xr[b], ur[b], gX[b], gU[b], wq, wr)
        assert model["ok"]
        err, tol = vr.max_err(model, dense), 10.0 * np.finfo(float).eps * dense["cond"] * vr.max_abs(dense)
        print(f"{case} weighted={weighted} instance {b}: Riccati vs dense {err:.3e} (bound {tol:.3e}, "
              f"cond {dense['cond']:.2e})")
        assert err <= tol
        assert not model["xref"][0].any()  # x_0 is pinned: its reference has no influence
        # a loss on x_0 alone: x_0 = x_init, whatever the rest of the solve does
        g0 = np.zeros_like(gX[b])
        g0[0] = gX[b, 0]
        only = vr.riccati_vjp(nlp, z[b], dual, xr[b], ur[b], g0, np.zeros_like(gU[b]), wq, wr)
        assert np.array_equal(only["x0"], gX[b, 0])
        assert not only["xref"].any() and not only["uref"].any() and not only["w"].any()


def test_full_weights_dense_and_riccati_against_the_oracle():
    nlp, x0, xr, ur = sr.case_free("mpc_full")
    B, N = x0.shape[0], nlp.N
    w = vr.random_weights(B)
    gX, gU = vr.random_upstream(B, N)
    z, st, fd = vr.oracle_fd_vjp(nlp, x0, xr, ur, gX, gU, w=w, h=1e-4)
    assert np.all(st == 0)
    diag = sr.case_free()[0]
    for b in range(B):
        wq, wr = w[b, :6], w[b, 6:]
        y = nlp.kkt_residual(z[b], x0[b], xr[b].T, ur[b].T, wq, wr)["y"].reshape(N + 1, 6)
        dual = _interior_dual(nlp, z[b], y)
        dense = vr.dense_vjp(nlp, z[b], dual, xr[b], ur[b], gX[b], gU[b], wq, wr)
        model = vr.riccati_vjp(nlp, z[b], dual, xr[b], ur[b], gX[b], gU[b], wq, wr)
        assert model["ok"]
        errs = {k: float(np.max(np.abs(fd[b][k] - dense[k]))) for k in vr.KEYS}
        err, tol = vr.max_err(model, dense), 10.0 * np.finfo(float).eps * dense["cond"] * vr.max_abs(dense)
        off = vr.max_err(vr.riccati_vjp(diag, z[b], dual, xr[b], ur[b], gX[b], gU[b], wq, wr), model)
        print(f"mpc_full weighted instance {b}: FD vs dense " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items())
              + f"; Riccati vs dense {err:.3e} (bound {tol:.3e}); the off-diagonals move the gradient by {off:.3e}")
        assert max(errs.values()) <= 1e-6
        assert err <= tol
        assert off > 1e-4   # a reference that dropped the off-diagonal terms would differ by this much
