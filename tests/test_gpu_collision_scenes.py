"""GPU tests of per-instance scenes in the collision check and in the switch closed loop
(tt_collision_scenes_device, collision_kernel's obstacle stride; ClosedLoop(obstacles=(B,M,4), d_min=)).

The collision poses are chosen on the CPU (``ttmpc.collision.sat_gap``) so that every body-obstacle gap is at least
1e-3 away from zero: the flag of no instance hangs on rounding.  The closed loop is the switch loop of
tests/test_gpu_switch_loop_vjp.py (case A's scene, N = 6, K = 4 steps) with B = 4: instances 0 and 1 meet their
obstacle and switch, instances 2 and 3 have theirs 2.5 m and 3 m further on and never do.  Each instance is compared
bitwise with a B = 1 loop that has its scene as the shared one.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import vjp_harness as h
from test_gpu_switch_loop_vjp import _case

pytestmark = pytest.mark.gpu

_t, _n = h.t, h.n


# ---- 8. collision ----
@functools.lru_cache(maxsize=None)
def collision_case():
    """B = 5, K = 11 poses, M = 3: (params, poses (B,K,6), scenes (B,M,4)), drawn with a fixed seed (the CPU checks of
    the test hold for it: gaps off zero, hits and misses, a flag that another instance's scene would change)."""
    from ttmpc import scenarios as sc
    rng = np.random.default_rng(11)
    B, K, M = 5, 11, 3
    poses = np.zeros((B, K, 6))
    poses[..., 0] = np.linspace(0.0, 6.0, K)[None] + rng.uniform(-0.3, 0.3, (B, 1))
    poses[..., 1] = rng.uniform(-0.5, 0.5, (B, 1)) + 0.05 * np.arange(K)[None]
    poses[..., 2] = rng.uniform(-0.3, 0.3, (B, K))
    poses[..., 3] = rng.uniform(-0.4, 0.4, (B, K))
    base = np.array([[3.0, 6.5, 2.0, 2.0], [-6.0, -12.0, 3.0, 1.5], [9.0, -5.5, 1.0, 2.5]])
    scenes = np.tile(base, (B, 1, 1))
    scenes[:, :, :2] += rng.uniform(-0.5, 0.5, (B, M, 2))
    scenes[1, 0, 1] -= 4.5          # instance 1: obstacle 0 comes down onto the path
    scenes[3, 2, :2] = (5.0, -2.4)  # instance 3: obstacle 2 beside the path, in the trailer's sweep
    scenes[4, 1, :2] = (-2.0, 0.0)  # instance 4: obstacle 1 on the trailer at the start
    return dict(sc.OBCA_PARAMS), poses, scenes


def _flags(poses, obstacles, params):
    from ttmpc import simulation as sim
    return _n(sim.collision_flags(_t(poses), None if obstacles is None else _t(obstacles), params))


def test_collision_flags_per_instance_scenes():
    import torch
    import ttmpc
    from ttmpc import collision
    from ttmpc import simulation as sim
    p, poses, scenes = collision_case()
    B, K, M = poses.shape[0], poses.shape[1], scenes.shape[1]
    gaps = np.stack([collision.sat_gap(poses[b, :, :4], p, scenes[b]) for b in range(B)])
    assert np.abs(gaps).min() >= 1e-3, np.abs(gaps).min()
    want = np.array([collision.collision_mask(poses[b, :, :4], p, scenes[b]).any() for b in range(B)])
    under0 = np.array([collision.collision_mask(poses[b, :, :4], p, scenes[0]).any() for b in range(B)])
    assert want.any() and not want.all() and np.any(want != under0), (want, under0)
    got = _flags(poses, scenes, p)
    print("flags", got.tolist(), "under scene 0", under0.astype(int).tolist())
    assert np.array_equal(got, want.astype(np.int32))
    # the old call once per scene
    for b in range(B):
        assert _flags(poses[b:b + 1], scenes[b], p)[0] == got[b], b
    # stride 0 is the old call: one shared scene through the old entry and, tiled, through the new one
    shared = _flags(poses, scenes[1], p)
    assert np.array_equal(_flags(poses, np.tile(scenes[1], (B, 1, 1)), p), shared)
    assert np.array_equal(shared, np.array([collision.collision_mask(poses[b, :, :4], p, scenes[1]).any()
                                            for b in range(B)]).astype(np.int32))
    # refusals
    with pytest.raises(ValueError):
        sim.collision_flags(_t(poses), _t(scenes[:4]), p)
    with pytest.raises(ValueError):
        sim.collision_flags(_t(poses), _t(scenes[..., :3]), p)
    L = ttmpc.lib()
    pl = sim.plant(p)
    flag = torch.zeros(B, dtype=torch.int32, device=_t(poses).device)
    assert L.tt_collision_scenes_device(B, K, None, 6 * K, 6, _t(scenes).data_ptr(), M, C.byref(pl), flag.data_ptr(),
                                        None) == -22


# ---- 9. switch closed loop ----
def _scenes():
    c = _case()
    ob = c["obs"]
    S = np.tile(ob, (4, 1, 1))
    S[1, 0, 0] -= 0.05
    S[2, 0, 0] += 2.5
    S[3, 0, 0] += 3.0
    S[3, 0, 2] += 0.3
    D = np.array([0.2, 0.25, 0.2, 0.3])
    x_init = c["x_init"][[0, 1, 0, 1]].copy()
    return S, D, x_init


def _loop(obstacles, d_min=None, scene=None):
    import ttmpc
    from ttmpc import simulation as sim
    c = _case()
    obca = ttmpc.ObcaSolver(c["N"], c["params"], c["Q"], c["R"], *c["bnd"], c["obs"],
                            variant=ttmpc.TT_VARIANT_TRACK_OBCA)
    if scene is not None:
        obca.set_scene(*scene)
    return sim.ClosedLoop(h.solver(c["nlp"], c["params"]), c["plan_x"], c["plan_u"], c["params"], None,
                          obstacles=obstacles, switch_solver=obca, switch_adjoint=True, d_min=d_min)


def test_switch_loop_per_instance_scenes():
    c = _case()
    S, D, x_init = _scenes()
    rng = np.random.default_rng(5)
    K = c["K"]
    GS, GU = rng.uniform(-1.0, 1.0, (K + 1, 4, 6)), rng.uniform(-1.0, 1.0, (K, 4, 2))
    loop = _loop(S, D)
    out = loop.run_tape(x_init, c["T"])
    g = {k: _n(v) for k, v in loop.backward(out["tape"], _t(GS), _t(GU), scene=True).items()}
    col = out["collide"]
    print("collide\n", col.astype(int), "\nstatus\n", out["status"])
    assert col[:, 0].any() and col[:, 1].any() and not col[:, 2].any() and not col[:, 3].any()
    assert g["g_obstacles"].shape == (4, 1, 4) and g["g_dmin"].shape == (4,)
    for b in range(4):
        one = _loop(S[b], scene=(S[b], D[b]))
        o1 = one.run_tape(x_init[b:b + 1], c["T"])
        for k in ("states", "controls", "status", "collide"):
            assert np.array_equal(out[k][:, b], o1[k][:, 0]), (b, k)
        g1 = {k: _n(v) for k, v in one.backward(o1["tape"], _t(GS[:, b:b + 1]), _t(GU[:, b:b + 1]),
                                                scene=True).items()}
        for k in ("g_x_init", "g_obstacles", "g_dmin"):
            assert np.array_equal(g[k][b], g1[k][0]), (b, k)
    assert np.abs(g["g_obstacles"][:2]).max() > 0.0 and np.all(g["g_obstacles"][2:] == 0.0)
    # a scalar d_min is that margin for every loop; the plain run() takes the same path
    both = _loop(S, 0.25).run(x_init, c["T"])
    one = _loop(S[1], scene=(S[1], 0.25)).run(x_init[1:2], c["T"])
    for k in ("states", "controls", "status", "collide"):
        assert np.array_equal(both[k][:, 1], one[k][:, 0]), k
    with pytest.raises(ValueError):
        _loop(S[:3], D[:3]).run(x_init, c["T"])
    with pytest.raises(ValueError):
        _loop(np.tile(S, (1, 2, 1)))
