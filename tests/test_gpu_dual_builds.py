"""GPU suite: the multiplier export (tt_solve_batch_ex) on every build of track_kernel and at every kind of exit.

tt_track_dual.hip compiles a second, exporting copy of every build launch_track dispatches to.  The export reads the
Y, z_L, z_U rows in the kernel's epilogue and rests on those rows being current at every exit of the main loop, which is
a property of each build's update and linearisation passes.  BUILDS has one row per ``return launch<...>`` line of
launch_track (tt_track.hip), in its order.

1. Per build: solve_ex returns bitwise the outputs of solve, the exported duals pass ``check_multipliers`` (signs, zeros,
   IPOPT's stopping test), and every 64-instance tile of a tiled batch is bitwise the first.
2. The E0 identity.  At every exit with status <= 2 the kernel's ``kkt`` output is the optimality error E0 of the
   iterate it has just linearised, and X, U and the duals it exports are that iterate: ``optimality_error`` restates E0
   in numpy from the exported numbers alone and must reproduce ``kkt`` to rounding,

       |kkt - E0_numpy| <= 64 eps scale,

   scale being the largest sum of absolute terms of any row of E0's pieces.  A row is a sum of at most about 16
   products, each rounded once: <= 16 eps sum|terms| on either side, doubled once more for contraction differences and
   the 1-ulp reciprocal.  Exits at the iteration limit (max_iter 1, 2, 3: status 2, mid-way through the barrier
   schedule, where multipliers stale by one update would be off by orders of magnitude more than rounding), converged
   exits, and the hard start of tests/test_gpu_track_carry.py at s = 2 cut off after 8 iterations (inertia retries,
   second-order corrections, rejected line searches).

Every case prints its figures before it asserts (DESIGN.md "Multiplier export and x_init sensitivities" records them).
"""
import functools

import numpy as np
import pytest

import sens_reference as sr
from test_gpu_track_carry import _bits, hard_batch
from track_patterns import nlp_of, patterns

pytestmark = pytest.mark.gpu

P = sr.P
EPS = float(np.finfo(np.float64).eps)
TILE = 64
HBM = "3 CUs + 64"   # the batch at which N = 50 moves its band to HBM depends on the device: resolved by _batch

# (id, pattern, N, B), one row per dispatch branch of launch_track, in its order
BUILDS = [
    ("n20_two_wave", "mpc_diag", 20, 2304),    # launch<kMaskMPC | kDiagBit | kOccBit, 2, 20>: N = 20, B > 2048
    ("n20_one_wave", "mpc_diag", 20, 64),      # launch<kMaskMPC | kDiagBit, 1, 20>
    ("n30_two_wave", "mpc_diag", 30, 2304),    # launch<kMaskMPC | kDiagBit | kOccBit, 2, 30>: N = 30, B > 2048
    ("n30_one_wave", "mpc_diag", 30, 64),      # launch<kMaskMPC | kDiagBit, 1, 30>
    ("generic_two_wave", "mpc_diag", 8, 4160),  # launch<kMaskMPC | kDiagBit, 2>: B > 4096 and five records fit the LDS
    ("n40", "mpc_diag", 40, 64),               # launch<kMaskMPC | kDiagBit, 1, 40>
    ("n50_hbm_band", "mpc_diag", 50, HBM),     # launch<kMaskMPC | kDiagBit | kPGBit, 1, 50>: B > 3 per CU
    ("n50_lds", "mpc_diag", 50, 64),           # launch<kMaskMPC | kDiagBit, 1, 50>: B <= 3 per CU
    ("generic_mpc_diag", "mpc_diag", 8, 64),   # launch<kMaskMPC | kDiagBit>
    ("generic_mpc_full", "mpc_full", 8, 64),   # launch<kMaskMPC>: non-diagonal weights
    ("generic_obca_diag", "obca", 8, 64),      # launch<kMaskOBCA | kDiagBit>
    ("generic_obca_full", "obca_full", 8, 64),  # launch<kMaskOBCA>: the OBCA bounds with the non-diagonal weights
    ("run_time_bounds", "run_time", 8, 64),    # launch<-1>: bounds read at run time
]
IDS = [r[0] for r in BUILDS]


def _batch(B):
    """The row's batch size (a multiple of the 64-instance tile)."""
    if B != HBM:
        return B
    import torch
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    return TILE * ((3 * cus + 64 + TILE - 1) // TILE)


def _solver(pattern, N, **kw):
    import ttmpc
    Q, R, xlb, xub, ulb, uub = patterns()[pattern]
    return ttmpc.BatchSolver(N, P, Q, R, xlb, xub, ulb, uub, tol=1e-8, **kw)


@functools.lru_cache(maxsize=None)
def _inputs(N):
    from ttmpc.scenarios import synthetic_batch
    return synthetic_batch(TILE, N, seed=4000 + N, psi_range=0.3)


def _tiled(a, reps):
    return np.tile(a, (reps,) + (1,) * (a.ndim - 1))


@functools.lru_cache(maxsize=None)
def _run(name, max_iter):
    """solve_ex (duals only) of a row's tiled batch at an iteration limit (0: the default) -> (nlp, inputs, result)."""
    _, pattern, N, B = BUILDS[IDS.index(name)]
    reps = _batch(B) // TILE
    x0, xr, ur = (_tiled(a, reps) for a in _inputs(N))
    r = _solver(pattern, N, max_iter=max_iter).solve_ex(x0, xr, ur, duals=True, gain=False)
    return nlp_of(pattern, N, P), (x0, xr, ur), r


def _assert_tiles(r, tag):
    for k in ("X", "U", "status", "iters", "kkt", "dual"):
        a = _bits(getattr(r, k))
        reps = a.shape[0] // TILE
        assert np.array_equal(a, _tiled(a[:TILE], reps)), (tag, k)


def _oracle_status(nlp, x0, xr, ur, max_iter):
    from oracle import c_oracle as co
    kw = {"max_iter": max_iter} if max_iter else {}
    _, st, it, _ = co.solve_batch(sr.oracle_problem(nlp, **kw), x0, xr, ur)
    return st, it


def _e0_ratios(nlp, x0, xr, ur, r, rows):
    """(|kkt - E0_numpy| / (eps scale), E0 piece that decides) of the instances ``rows``."""
    from ttmpc import layout
    zz = layout.pack(r.X, r.U)
    ratio, piece = np.empty(len(rows)), []
    for i, b in enumerate(rows):
        e = sr.optimality_error(nlp, zz[b], x0[b], xr[b], ur[b], r.dual[b])
        ratio[i] = abs(float(r.kkt[b]) - e["E0"]) / (EPS * e["scale"])
        piece.append(max(("dinf", e["dinf"] / e["s_d"]), ("pinf", e["pinf"]), ("c0", e["c0"] / e["s_c"]),
                         key=lambda t: t[1])[0])
    return ratio, piece


# ---- 1 ----------------------------------------------------------------------------------------------------------
def test_table_is_the_whole_dispatch():
    """One row per ``return launch<...>`` of launch_track (two of its thirteen sit on one line each, behind ``d ? :``)."""
    from conftest import REPO
    src = (REPO / "car-trailer-mpc_amd" / "csrc" / "tt_track.hip").read_text()
    body = src[src.index("hipError_t launch_track(const TrackArgs& a, hipStream_t stream) {"):]
    assert body.count("launch<") == len(BUILDS) == 13


@pytest.mark.parametrize("name", IDS)
def test_export_on_every_build(name):
    _, pattern, N, B = BUILDS[IDS.index(name)]
    nlp, (x0, xr, ur), ex = _run(name, 0)
    B = _batch(B)
    assert x0.shape[0] == B
    plain = _solver(pattern, N).solve(x0, xr, ur)
    for a, b in zip(plain, (ex.X, ex.U, ex.status, ex.iters, ex.kkt)):
        assert a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))
    assert ex.dual.shape == (B, N + 1, 22)
    print(f"{name}: B {B}, status counts {np.bincount(ex.status, minlength=6).tolist()}, "
          f"iters {int(ex.iters.min())}-{int(ex.iters.max())}")
    assert np.all(ex.status[:TILE] == 0)
    first = type(ex)(**{k: getattr(ex, k)[:TILE] for k in ("X", "U", "status", "iters", "kkt", "dual")})
    sr.check_multipliers(nlp, 1e-8, x0[:TILE], xr[:TILE], ur[:TILE], first, label=name)
    _assert_tiles(ex, name)


# ---- 2 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_kkt_is_e0_of_the_exported_point(name):
    worst = 0.0
    for max_iter in (1, 2, 3, 0):
        nlp, (x0, xr, ur), r = _run(name, max_iter)
        _assert_tiles(r, (name, max_iter))
        st_o, it_o = _oracle_status(nlp, x0[:TILE], xr[:TILE], ur[:TILE], max_iter)
        st, it = r.status[:TILE], r.iters[:TILE]
        ratio, piece = _e0_ratios(nlp, x0, xr, ur, r, range(TILE))
        print(f"{name} max_iter {max_iter or 'default'}: status counts gpu {np.bincount(st, minlength=6).tolist()} "
              f"oracle {np.bincount(st_o, minlength=6).tolist()}, iters gpu {int(it.min())}-{int(it.max())} oracle "
              f"{int(it_o.min())}-{int(it_o.max())}, kkt {r.kkt[:TILE].min():.3e}..{r.kkt[:TILE].max():.3e}, "
              f"|kkt - E0| / (eps scale) max {ratio.max():.3f} (deciding piece: "
              f"{ {p: piece.count(p) for p in sorted(set(piece))} })")
        assert np.all(st <= 2), "every synthetic instance is compared"
        if max_iter:
            assert np.all(it == max_iter) and np.all(st == 2)   # the exit at the limit, not a converged one
        else:
            assert np.all(st == 0)
        assert np.all(np.isfinite(ratio))
        worst = max(worst, float(ratio.max()))
    print(f"{name}: largest |kkt - E0_numpy| / (eps scale) {worst:.3f} (bound 64)")
    assert worst <= 64.0


@pytest.mark.parametrize("N", [20, 30])
def test_kkt_is_e0_on_the_hard_batch(N):
    """hard_batch(N, 2.0, 11) cut off after 8 iterations, the one-wave builds of N = 20 and 30: on the CPU oracle 38 + 58
    (N = 20) and 26 + 70 (N = 30) instances of status 0 + status 2, none non-finite."""
    x0, xr, ur = hard_batch(N, 2.0, 11)
    nlp = nlp_of("mpc_diag", N, P)
    r = _solver("mpc_diag", N, max_iter=8).solve_ex(x0, xr, ur, duals=True, gain=False)
    st_o, it_o = _oracle_status(nlp, x0, xr, ur, 8)
    rows = np.flatnonzero(r.status <= 2)
    ratio, piece = _e0_ratios(nlp, x0, xr, ur, r, rows)
    print(f"hard N={N} max_iter 8: status counts gpu {np.bincount(r.status, minlength=6).tolist()} oracle "
          f"{np.bincount(st_o, minlength=6).tolist()}, statuses equal on {int(np.sum(r.status == st_o))} of 96, "
          f"compared {rows.size}, kkt {r.kkt[rows].min():.3e}..{r.kkt[rows].max():.3e}, |kkt - E0| / (eps scale) max "
          f"{ratio.max():.3f} (deciding piece: { {p: piece.count(p) for p in sorted(set(piece))} })")
    assert rows.size >= 90
    assert np.sum(r.status == 2) >= 20 and np.all(r.iters[r.status == 2] == 8)
    assert np.all(np.isfinite(ratio))
    assert ratio.max() <= 64.0
