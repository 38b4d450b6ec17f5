"""Test helper for the GPU adjoint suites (test_gpu_vjp, _loop_vjp, _model_vjp, _fuzzy_vjp, _lqr_vjp): the tensor
helpers, the golden inputs, the solver and loop builders, the converters from what ``ClosedLoop.backward`` and a
``LoopTape`` hold to the numpy references' dicts, and the comparison with the numpy chain.  torch and ttmpc are imported
inside the functions, so that collecting the suites needs neither."""
import functools

import numpy as np

import loop_vjp_reference as lr

P, DIST = lr.P, lr.DIST          # (sens_reference.P is the same dict of values)
EPS = float(np.finfo(np.float64).eps)
GRADS = {"x_init": "g_x_init", "w": "g_wq_wr", "noise": "g_noise", "plan_x": "g_plan_x", "plan_u": "g_plan_u",
         "theta": "g_fuzzy_rule"}
TAPE = ("S", "Ua", "status", "active", "consec", "X", "U", "dual", "W", "retried")


def t(a, dtype=None):
    """A host array as a CUDA tensor, float64 unless dtype says otherwise."""
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64).cuda()


def n(x):
    return x.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def golden():
    from conftest import GOLDEN
    return dict(np.load(GOLDEN / "reference_numpy.npz"))


def w_of(w, b):
    """(wq, wr) of instance b, as the numpy references take them."""
    return (None, None) if w is None else (w[b, :6], w[b, 6:])


def solver(nlp, params=P, **kw):
    import ttmpc
    return ttmpc.BatchSolver(nlp.N, params, nlp.Q, nlp.R, nlp.xlb, nlp.xub, nlp.ulb, nlp.uub, **kw)


def loop(c, policy="track", in_plant=False, per_instance=0, rule=None, params=P, solver_params=P, solver_kw=None,
         **kw):
    """The ``ClosedLoop`` of a case dict (loop_vjp_reference.loop_case and its kin) on its shared plan; per_instance = B
    gives every instance its own copy of the plan.  rule: a FuzzyRule; params / solver_params: the plant's and the
    controller's parameters; solver_kw: variant and tolerance of the solver; kw: the rest of ClosedLoop's options."""
    from ttmpc import simulation as sim
    px, pu = c["plan_x"], c["plan_u"]
    if per_instance:
        px, pu = np.tile(px.T[None], (per_instance, 1, 1)), np.tile(pu.T[None], (per_instance, 1, 1))
    return sim.ClosedLoop(solver(c["nlp"], solver_params, **(solver_kw or {})), px, pu, params, DIST, policy=policy,
                          noise_in_plant=in_plant, fuzzy_rule=rule, **kw)


def grads(g):
    """ClosedLoop.backward's dict under the numpy references' group names (theta if the rule's gradient is there)."""
    return {k: n(g[v]) for k, v in GRADS.items() if v in g}


def tape_np(tape):
    """A LoopTape's tensors as the dict the numpy chains take."""
    return {k: n(getattr(tape, k)) for k in TAPE if getattr(tape, k) is not None}


def shared_plan(g):
    """A chain's gradients with the per-instance plan gradients summed over B: those of a shared plan."""
    return dict(g, plan_x=g["plan_x"].sum(axis=0, keepdims=True), plan_u=g["plan_u"].sum(axis=0, keepdims=True))


def compare_with_chain(tag, got, dense, model, groups, per_group):
    """got (the GPU's), model (the numpy recursion the kernel runs) and dense (dense algebra), dicts over ``groups``:
    prints every group's figures, then asserts err_gpu <= 10 err_model + 1e-12 max|ref| against dense, group by group
    or on the largest of each over the groups.  -> max|ref| per group."""
    err = lambda a: {k: float(np.max(np.abs(np.asarray(a[k]) - np.asarray(dense[k])))) for k in groups}  # noqa: E731
    e_gpu, e_model = err(got), err(model)
    big = {k: float(np.max(np.abs(np.asarray(dense[k])))) for k in groups}
    for k in groups:
        print(f"{tag} {k:7s}: err_gpu {e_gpu[k]:.3e}, err_model {e_model[k]:.3e}, max|ref| {big[k]:.3e}")
    if per_group:
        for k in groups:
            assert e_gpu[k] <= 10.0 * e_model[k] + 1e-12 * big[k], k
    else:
        assert max(e_gpu.values()) <= 10.0 * max(e_model.values()) + 1e-12 * max(big.values())
    return big
