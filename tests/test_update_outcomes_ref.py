"""The case table of tests/update_outcomes_ref.py on the CPU: every case takes the branches it is listed for, clears
each decision with the admission margins in the float64 reference, and decides the same in float32; the table holds
every outcome tests/test_gpu_update_outcomes.py needs on every path.  This is the proof that the reference alone
stays inside the conditions under which a device value at the 1e-5 bar cannot flip a branch."""
import numpy as np
import pytest

import fvp_subsample_ref as S
import gauss_ref as G
import update_outcomes_ref as U
from oracle import trpo_oracle as O

ALL_IDS = [c.id for c in U.ALL_CASES]


@pytest.mark.parametrize("case_id", ALL_IDS)
def test_case_is_admitted(case_id):
    c = U.BY_ID[case_id]
    t = U.reference(case_id)
    assert t.outcome == c.expect, (t.outcome, c.expect)
    if c.outcome in U.OUTCOMES:
        assert U.OUTCOMES[c.outcome](*t.outcome), (c.outcome, t.outcome)
    assert U.margins(t) == []
    t32 = U.reference(case_id, False)
    assert t32.outcome == t.outcome, f"float32 decides {t32.outcome}, float64 {t.outcome}"
    if c.stop is not None:
        assert t.tol > 0 and t.cg_iters == c.stop
    if t.k == -1 or t.reverted:
        assert np.array_equal(t.theta_new, U.path_feed(c.path, c.seed, c.perturbed).theta.astype(np.float64))
    if t.k == -1:
        assert np.array_equal(t.losses_after, t.losses_before)


def test_table_holds_every_outcome():
    for path in U.PATHS:
        if path.startswith("mrank"):
            assert {"stop_mid", "k_ge3", "k_none"} <= {c.outcome for c in U.MRANK_CASES if c.path == path}
            continue
        if path in U.VARIANT_OF:      # a feed variant: its cases count for the engine path it varies
            v, base = U.PATHS[path], U.PATHS[U.VARIANT_OF[path]]
            assert (v.head, v.dims, v.n, v.options, v.stride, v.comm, v.damping, v.tags) == \
                   (base.head, base.dims, base.n, base.options, base.stride, base.comm, base.damping, base.tags)
            continue
        have = {c.outcome for c in U.CASES if path in (c.path, U.VARIANT_OF.get(c.path))}
        need = set(U.OUTCOMES) - {"k_ge3"} if path in U.FULL else set(U.SHORT)
        assert need <= have, f"{path}: missing {sorted(need - have)}"
    for path in U.FULL:
        tol, steps = U.GRAPH_STEPS[path]
        outs = [s[-1] for s in steps]
        assert tol > 0 and len(steps) * 2 >= 8
        assert len({it for it, _, _ in outs}) >= 3, f"{path}: fewer than three stop iterations under one tol"
        assert any(k == 0 and not rev for _, k, rev in outs) and any(k >= 3 and not rev for _, k, rev in outs)
        assert any(k == -1 for _, k, _ in outs) and any(rev for _, _, rev in outs)
        # every outcome is replayed after a different one, the wrap-around of the second round included
        ring = outs + outs[:1]
        assert all(a != b for a, b in zip(ring, ring[1:]))
        # one graph key: the rows of every step's feed are the path's
        assert {U.path_feed(path, s[1], s[2]).X.shape[0] for s in steps} == {U.PATHS[path].n}


def _same(t, r):
    assert t.outcome == (r.cg_iters, r.k, r.reverted)
    for name in ("stepdir", "fullstep", "theta_ls", "theta_new", "losses_after"):
        assert np.array_equal(getattr(t, name), getattr(r, name)), name
    assert (t.shs, t.lm, t.rate) == (r.shs, r.lm, r.rate)


@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
def test_trace_repeats_the_references(f64):
    """evaluate() is the references' own update, operation for operation: bitwise the same results"""
    import torch
    npdt, tdt = (np.float64, torch.float64) if f64 else (np.float32, torch.float32)
    c = U.BY_ID["p1_fused16-combined"]
    t = c.evaluate(f64)
    fd = U.path_feed(c.path, c.seed)
    b = O.Batch(fd.X, fd.actions, U.scaled_advant(fd, 1.0), fd.old)
    _same(t, O.trpo_update(fd.theta, b, fd.spec, npdt, 10, t.tol, c.max_kl))
    c = U.BY_ID["p8_sub3_fused16-k_ge3"]
    fd = U.path_feed(c.path, c.seed)
    b = O.Batch(fd.X, fd.actions, U.scaled_advant(fd, 1.0), fd.old)
    _same(c.evaluate(f64), S.categorical_update(fd.theta, b, fd.spec, 3, npdt, 10, 0.0, c.max_kl))
    c = U.BY_ID["p7_gauss_small-combined"]
    t = c.evaluate(f64)
    fd = U.path_feed(c.path, c.seed)
    gb = G.GaussBatch(fd.X, fd.actions, U.scaled_advant(fd, 1.0), fd.old, fd.old_logstd)
    _same(t, G.update(fd.theta, gb, fd.spec, tdt, 10, t.tol, c.max_kl, U.PATHS[c.path].damping))


def test_margins_reject_near_misses():
    """margins() itself: a tol too close to an rdotr, a ratio between the bars, a kl_after near 2 max_kl"""
    t = U.reference("p1_fused16-stop_mid")
    near = U.evaluate("p1_fused16", 7, tol=t.rdotr[5] * 1.2, max_kl=0.01)
    assert near.cg_iters == 5 and any("tol" in m for m in U.margins(near))
    # a round max_kl: k = 1 as wanted, but accepted at a ratio of 0.12, under the 0.2 bar
    loose = U.evaluate("p1_fused16", 7, max_kl=1e2)
    assert loose.k == 1 and any("accepted trial 1" in m for m in U.margins(loose))
    import dataclasses
    kl = dataclasses.replace(t, max_kl=t.kl_after / 2.0 * 1.1)     # the same trace read against a 2 max_kl 10 % off
    assert any("kl_after" in m for m in U.margins(kl))
