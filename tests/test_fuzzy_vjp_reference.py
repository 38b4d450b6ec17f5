"""CPU suite: the rule adjoint and the extended sweep of tests/fuzzy_vjp_reference.py pinned against the CPU oracle.

1. ``rule_vjp`` against central differences (h = 1e-6) of ``rule_weights`` on random states and several rules, every
   point at least 1e-3 from a kink: <= 1e-8, and exact zeros where the table says zero.
2. The numpy chain (``dense_vjp`` per step at the oracle's interior multipliers, with the plant, rule and window
   adjoints between the steps) against central differences (h = 1e-4) of ``to.closed_loop(policy="fuzzy",
   fuzzy=True)`` with the rule patched into the oracle: x_init, noise, plan <= 1e-6; theta <= 1e-7.
3. The same with chosen first attempts forced to fail: the retry runs with unit weights, the chain takes W = 1 and
   retried = 1 there, and the rule term of those steps is exactly 0.
"""
import numpy as np
import pytest

import fuzzy_vjp_reference as fr
import vjp_reference as vr

# (theta, note): inside and saturated |psi| come from the states; the rules move the clip and the saturation
RULES = [
    (fr.DEFAULT_THETA, "the reference's constants: saturation at 0.35, the largest weight 3.3 stays under the clip"),
    (fr.THETA, "the loop case's rule: wide linear range, hitch reaches the clip inside it"),
    ((0.5, 0.9, 0.7, 0.8, 1.3, 1.25, 1.4), "no channel ever reaches the clip"),
    ((0.2, 3.0, 2.6, 2.9, 1.2, 1.3, 1.1), "every channel clipped when saturated"),
]


# ---- 1 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta,note", RULES)
def test_rule_adjoint_against_central_differences(theta, note):
    rng = np.random.default_rng(11)
    n = 4000
    psi = rng.uniform(-1.2, 1.2, n) * rng.choice([0.2, 1.0], n)
    v = np.where(rng.uniform(size=n) < 0.5, rng.uniform(-2.0, -0.1, n), rng.uniform(-0.1, 2.0, n))
    ref_v = np.where(rng.uniform(size=n) < 0.5, rng.uniform(-2.0, -0.1, n), rng.uniform(-0.1, 2.0, n))
    keep = fr.rule_kink_distance(theta, psi, v, ref_v) > 1e-3
    psi, v, ref_v = psi[keep], v[keep], ref_v[keep]
    g_w = rng.uniform(-1.0, 1.0, (psi.size, 8))
    t = fr._terms(theta, psi, v, ref_v, fr.SETTINGS)
    inside, sat = t["s"] < 1.0, t["s"] >= 1.0
    via_v, via_ref, fwd = (v < -0.1) & (ref_v >= -0.1), (ref_v < -0.1) & (v >= -0.1), ~t["rev"]
    clipped = t["m"] >= 3.5
    print(f"{note}: {psi.size} of {n} points kept; inside {inside.sum()}, saturated {sat.sum()}; reversing through v "
          f"only {via_v.sum()}, through ref_v only {via_ref.sum()}, not {fwd.sum()}; clipped per channel "
          f"{clipped.sum(axis=0).tolist()}, passing {t['passes'].sum(axis=0).tolist()}")
    assert min(inside.sum(), sat.sum(), via_v.sum(), via_ref.sum(), fwd.sum()) > 50
    g_psi, g_th = fr.rule_vjp(theta, psi, v, ref_v, g_w)
    h = 1e-6

    def loss(th=theta, p=psi, vv=v, rv=ref_v):
        return np.sum(g_w * fr.rule_weights(th, p, vv, rv), axis=-1)

    worst = np.max(np.abs((loss(p=psi + h) - loss(p=psi - h)) / (2 * h) - g_psi))
    for i in range(7):
        e = np.zeros(7)
        e[i] = h
        worst = max(worst, np.max(np.abs((loss(th=np.asarray(theta) + e) - loss(th=np.asarray(theta) - e)) / (2 * h)
                                         - g_th[:, i])))
    # v and ref_v only switch: the differences themselves are exactly 0 away from the switch
    assert not ((loss(vv=v + h) - loss(vv=v - h)).any() or (loss(rv=ref_v + h) - loss(rv=ref_v - h)).any())
    print(f"  rule adjoint vs central differences {worst:.3e}; largest |g_psi| {np.max(np.abs(g_psi)):.2f}, "
          f"|g_theta| {np.max(np.abs(g_th), axis=0)}")
    assert worst <= 1e-8
    # exact zeros of the table
    assert not g_psi[sat].any() and not g_th[sat, 0].any()                 # saturated: psi and psi_full carry nothing
    assert not g_th[fwd, 4:7].any()                                        # not reversing: the factors carry nothing
    blocked = ~t["passes"]
    assert not g_th[:, 1:4][blocked].any() and not g_th[:, 4:7][blocked].any()
    assert not g_psi[blocked.all(axis=1)].any()
    if theta is RULES[3][0]:
        assert clipped[sat & t["rev"]].all() and clipped.sum(axis=0).min() > 50    # each channel clipped and unclipped
    assert np.max(np.abs(g_psi)) > 0.1 and np.all(np.max(np.abs(g_th), axis=0) > 0.0)


# ---- 2, 3 -------------------------------------------------------------------------------------------------------
def _check_chain(c, tape, fd, tag):
    g = fr.chain(c, vr.dense_vjp, tape)
    err, big = fr.fd_errors(g, fd), fr.group_max(g)
    for k, e in err.items():
        print(f"{tag} {k:7s}: chain vs oracle FD {e:.3e}, largest entry {big[k]:.3e}")
    print(f"{tag} theta gradient summed over B: {g['theta'].sum(axis=0)}")
    assert max(err[k] for k in ("x_init", "noise", "plan_x", "plan_u")) <= 1e-6
    assert err["theta"] <= 1e-7
    return g


def _rule_state(c, tape):
    K, B = tape["status"].shape
    x, rv = tape["x_meas"], fr.window_ref_v(c["plan_x"], c["ks"], c["Np"], B)
    return fr._terms(c["theta"], x[..., 3], x[..., 5], rv, fr.SETTINGS), fr.rule_kink_distance(
        c["theta"], x[..., 3], x[..., 5], rv)


def test_chain_against_oracle_fuzzy_loop_finite_differences(golden_ref):
    c = fr.fuzzy_case(golden_ref)
    tape = fr.oracle_tape(c)
    assert np.all(tape["status"] == 0) and not tape["retried"].any()
    t, dist = _rule_state(c, tape)
    print(f"|psi| {np.abs(t['psi']).min():.2f}..{np.abs(t['psi']).max():.2f} against psi_full {c['theta'][0]}, reversing "
          f"{t['rev'].all()}, hitch clipped by step and instance {(t['m'][..., 0] >= 3.5).astype(int).tolist()}, "
          f"smallest kink distance {dist.min():.2e}")
    assert dist.min() > 1e-3
    assert np.all(t["s"] < 1.0) and t["rev"].all()                       # the linear range, reversing
    clip2 = t["m"][:, 2, 0] >= 3.5
    assert clip2[:2].all() and not clip2[2:].any()                       # instance 2: clipped, then unclipped
    assert np.array_equal(tape["W"], fr.rule_weights(c["theta"], t["psi"], tape["x_meas"][..., 5],
                                                     fr.window_ref_v(c["plan_x"], c["ks"], c["Np"], c["B"])))
    fd, ok = fr.oracle_fd(c, h=1e-4)
    assert ok
    g = _check_chain(c, tape, fd, "fuzzy loop")
    dpsi = np.abs(g["x_init"][:, 3])
    print(f"d/dpsi entries {dpsi}, |theta| entries of the FD {np.abs(fd['theta']).sum(axis=0)}")
    th = np.abs(fd["theta"].sum(axis=0))
    assert np.all(np.delete(th, 2) > 1e-4)                               # every entry but possibly gain_steer
    assert np.max(np.abs(g["x_init"])) > 1e-3 and np.max(np.abs(g["noise"])) > 1e-3


def test_chain_with_forced_retries(golden_ref):
    """Instance 1's first attempt is made to report status 2 at t = 0 and t = 3: the retry with unit weights succeeds."""
    c = fr.fuzzy_case(golden_ref)
    force = {0: 1, 3: 1}
    tape = fr.oracle_tape(c, force={t: np.arange(c["B"]) == b for t, b in force.items()})
    want = np.zeros((c["K"], c["B"]), dtype=np.int32)
    want[0, 1] = want[3, 1] = 1
    assert np.array_equal(tape["retried"], want) and np.all(tape["status"] == 0)
    assert np.all(tape["W"][want == 1] == 1.0) and np.all(tape["W"][want == 0][:, 3] > 1.0)
    _, dist = _rule_state(c, tape)
    assert dist.min() > 1e-3
    fd, ok = fr.oracle_fd(c, h=1e-4, force=force)
    assert ok
    g = _check_chain(c, tape, fd, "forced retries")
    assert not g["rule_terms"][want == 1].any()                          # the rule term of a retried step: exactly 0
    assert np.all(np.abs(g["rule_terms"][want == 0]).max(axis=-1) > 0.0)
    plain = fr.chain(c, vr.dense_vjp, fr.oracle_tape(c))
    assert np.max(np.abs(plain["theta"][1] - g["theta"][1])) > 1e-6      # and the forcing changed that instance's gradient
