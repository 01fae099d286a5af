"""The diagonal-Gaussian engine where its composition of launches can go wrong, against the float64 reference
tests/gauss_ref.py: layer shapes, row counts and numerical regimes that tests/test_gpu_gauss.py does not reach
(the table and its reasons are in tests/gauss_hard_cases.py), the engine's state across feeds and call orders,
the edges of act_gaussian's one-wave-per-state layout, and two real ranks.

The bar, everywhere: max(1e-5, 4 x the float32 reference's own error on the same inputs), computed here from
gauss_ref in float32 against float64 (the engine's figures never enter it; tests/test_gauss_ref.py bounds the
float32 error of every case).  Where it is 1e-5 the check is conftest.assert_vec_close (norm and elementwise),
where it is the 4x it is rel L2.  Vectors are judged per parameter block (each W_l, each b_l, the log-std tail,
each against its own norm) and as a whole.  surr, ent and kl keep the bars of tests/test_gpu_gauss.py; after an
update they are judged at the engine's own accepted theta (which is itself held to the reference's), since under
an ill-conditioned CG the float64 reference's trial point is not the point the engine evaluated.  shs, lm and
rate: 1e-5 or 4 x the float32 reference's relative error.  Every figure is printed before it is asserted and goes
to $TRPO_MARGIN_LOG when that is set.

What would make each test fail:
  test_hard_case[shapes]    a missed zero plane block at obs <= 64, a tile bound at a width that is no multiple of
                            32, a layer index that assumes two hidden layers, a split weight gradient losing a slab
  test_hard_case[rows]      rows past n read from a plane tile, the odd row of the last row pair, a partial tile
  test_hard_case[regimes]   an operand scale taken from a stale or too-coarse running max: saturated 1 - H^2, rows
                            2^15 apart, RD_L scaled by e^10, columns of RD_L e^12 apart (the column check fails if
                            the small-1/sigma^2 columns are lost although the block passes)
  test_hard_case[colsum]    a dropped or double-counted last colsum block, a wrong rows_per_block, an unscaled tail
                            partial, row threads of cw = 128 overlapping
  test_refeed_*             stale rows past n in the planes, g_s rows kept in D[L-1] from an earlier feed, running-
                            max slots or old_logstd captured in a graph and not re-read
  test_call_order_*         another pass overwriting the g_s rows before policy_grad reduces them, eval_losses
                            leaving prepare()'s outputs of the other theta marked valid
  test_act_gaussian_edges   a lane bound at A = 1 / 33 / 64, a row bound at n = 130 (a partial last block)
  test_act_gaussian_refuses_65_*   the refusal dropped (lanes past 64 unwritten), or a refused call that leaves the
                            engine's stream, feed or cache in a state the next policy_grad / update trips over
  test_colsum_check_sees_*  nothing in the engine: it fails if the colsum check stops telling a reference that
                            lacks one row from the right one (a bar wide enough to hide a dropped row)
  test_refeed_check_sees_*  nothing in the engine: it fails if the bitwise comparison of the re-feed test cannot
                            tell a 128-row feed from the 129-row one
  test_two_ranks_gaussian_* a log-std partial not all-reduced or scaled by the local n instead of n_global (it
                            shows in stepdir and its tail; theta hides the step, Hv's tail is 2 v n/N)
"""
import os

import numpy as np
import pytest

from conftest import assert_vec_close, rel_l2
import gauss_hard_cases as GH
import gauss_ref as G
from test_gpu_gauss import _engine
from test_gpu_parity import run_mrank

pytestmark = pytest.mark.gpu
REL = 1e-5


def log_margin(line):
    path = os.environ.get("TRPO_MARGIN_LOG")
    print(line)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _check_losses(got, theta, b, spec, what):
    """the loss bars of tests/test_gpu_gauss.py (surr: 1e-5 (1/N) sum |adv r|; ent: 1e-5 sum (|s_d| + 1.42); kl:
    relative, max(1e-5, 4 x the float32 reference's own error), at most 1e-4), the figures to the margin log"""
    import torch
    ref = G.losses(theta, b, spec, torch.float64)
    ref32 = G.losses(theta, b, spec, torch.float32)
    wsum = G.surr_weight_sum(theta, b, spec)
    s = np.asarray(theta, np.float64)[spec.n_net:]
    ent_scale = float(np.sum(np.abs(s) + 1.42)) * b.X.shape[0] / b.N
    kl_ref_err = abs(float(ref32[1]) - ref[1]) / abs(ref[1])
    kl_bar = min(1e-4, max(REL, 4.0 * kl_ref_err))
    d = np.abs(np.asarray(got, np.float64) - ref)
    log_margin(f"{what}: surr err {d[0]:.3e} (bar {REL * wsum:.3e}; f32 ref {abs(float(ref32[0]) - ref[0]):.3e})  "
               f"kl rel err {d[1] / abs(ref[1]):.3e} (bar {kl_bar:.3e}; f32 ref {kl_ref_err:.3e}; kl {ref[1]:.3e})  "
               f"ent err {d[2]:.3e} (bar {REL * ent_scale:.3e})")
    assert d[0] <= REL * wsum, f"{what}: surr"
    assert d[1] <= kl_bar * abs(ref[1]), f"{what}: kl"
    assert d[2] <= REL * ent_scale, f"{what}: ent"


def check_vec(got, ref, ref32, spec, what, only=None):
    """`got` against float64 `ref` per parameter block and as a whole (`only`: these blocks alone) at the bar
    max(1e-5, 4 x the float32 reference's error on that block); one margin line, then the assertions"""
    got = np.asarray(got, np.float64)
    rows = []
    for name, sl in G.block_slices(spec) + [("all", slice(None))]:
        if only is not None and name not in only:
            continue
        f32 = rel_l2(ref32[sl], ref[sl])
        rows.append((name, sl, rel_l2(got[sl], ref[sl]), f32, max(REL, 4.0 * f32)))
    log_margin(f"{what}: " + "  ".join(f"{name} {err:.2e} (bar {bar:.1e}, f32 ref {f32:.1e})"
                                       for name, _, err, f32, bar in rows))
    assert np.all(np.isfinite(got)), what
    for name, sl, err, f32, bar in rows:
        if bar == REL:
            assert_vec_close(got[sl], ref[sl], REL, f"{what} {name}")
        else:
            assert err <= bar, f"{what} {name}: rel L2 {err:.3e} > {bar:.1e} (4 x the float32 reference's {f32:.1e})"


def check_scalar(got, ref, ref32, what):
    f32 = GH.rel(ref32, ref)
    bar, err = max(REL, 4.0 * f32), GH.rel(got, ref)
    log_margin(f"{what}: rel err {err:.2e} (bar {bar:.1e}, f32 ref {f32:.1e})")
    assert err <= bar, f"{what}: {err:.3e} > {bar:.1e}"


def check_columns(got, ref, spec, what):
    """W_L's block column by column, each of the A columns against its own norm at 1e-5"""
    sl = dict(G.block_slices(spec))[f"W{len(spec.hidden)}"]
    g, r = (np.asarray(x, np.float64)[sl].reshape(spec.hidden[-1], spec.act_dim) for x in (got, ref))
    errs = [rel_l2(g[:, j], r[:, j]) for j in range(spec.act_dim)]
    norms = np.linalg.norm(r, axis=0)
    log_margin(f"{what} W_L by column: worst {max(errs):.2e} at column {int(np.argmax(errs))} (bar {REL:.0e}); "
               f"column norms {norms.max():.2e} .. {norms.min():.2e}; errors " + " ".join(f"{e:.1e}" for e in errs))
    for j, e in enumerate(errs):
        assert e <= REL, f"{what} W_L column {j}: rel L2 {e:.3e} > {REL:.0e} (column norm {norms[j]:.2e})"


def _update_vectors(e):
    from trpo_amd._lib import VEC_FULLSTEP, VEC_G, VEC_STEPDIR
    return [e.get_vector(VEC_G), e.get_vector(VEC_STEPDIR), e.get_vector(VEC_FULLSTEP), e.get_flat()]


def _update(e, **kw):
    from trpo_amd import UpdateParams
    return e.update(UpdateParams(cg_iters=10, residual_tol=0.0, **kw))


# ---- 1. the table -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [pytest.param(c.id, id=f"{c.group}-{c.id}") for c in GH.CASES])
def test_hard_case(gpu_available, case):
    c = GH.BY_ID[case]
    spec, theta, b = GH.feed(case)
    big_n = c.shape[3] > GH.COLSUM_BIG_N
    with _engine(spec, b, theta) as e:
        assert e.dist == "gaussian" and e.num_params == spec.n_params
        if "losses" in c.checks:
            _check_losses(e.losses(), theta, b, spec, f"{case} losses")
            theta2 = (theta.astype(np.float64) * (1 + 0.01 * np.random.RandomState(5).standard_normal(theta.shape)))
            theta2 = theta2.astype(np.float32)
            _check_losses(e.eval_losses(theta2), theta2, b, spec, f"{case} eval_losses")
            # eval_losses is loss(th): it sets the parameters; back to theta before g and Hv
            _check_losses(e.eval_losses(theta), theta, b, spec, f"{case} eval_losses(theta)")
        r = GH.vec_refs(case)
        v = r["v"]
        g = e.policy_grad()
        check_vec(g, *r["g"], spec, f"{case} g", only=("logstd", "all") if big_n else None)
        for damping in ((0.0,) if c.group == "colsum" else (0.0, 0.1)):
            hv = e.fvp(v, damping)
            want = r["hv"][0] + damping * v.astype(np.float64)
            want32 = r["hv"][1] + np.float32(damping) * v
            check_vec(hv, want, want32, spec, f"{case} Hv damping {damping}", only=("logstd",) if big_n else None)
            if c.regime == "sigma_spread" and damping == 0.0:
                check_columns(hv, want, spec, f"{case} Hv")
        assert np.array_equal(e.policy_grad(), g)
    if "update" not in c.checks:
        return
    uspec, utheta, ub = GH.update_feed(case)
    r64, r32 = GH.update_refs(case)
    with _engine(uspec, ub, utheta) as e:
        st = _update(e)
        what = f"{case} update"
        log_margin(f"{what}: cg_iters {st['cg_iters']} k {st['k']} reverted {st['reverted']} "
                   f"(ref {r64.cg_iters} {r64.k} {r64.reverted})")
        assert (st["cg_iters"], st["k"], bool(st["reverted"])) == (r64.cg_iters, r64.k, r64.reverted)
        assert not r64.reverted
        vg, vs, vf, th = _update_vectors(e)
        check_vec(vg, r64.g, r32.g, uspec, what + " g")
        check_vec(vs, r64.stepdir, r32.stepdir, uspec, what + " stepdir")
        check_vec(vf, r64.fullstep, r32.fullstep, uspec, what + " fullstep")
        check_vec(th, r64.theta_new, r32.theta_new, uspec, what + " theta")
        for name in ("shs", "lm", "rate"):
            check_scalar(st[name], getattr(r64, name), getattr(r32, name), f"{what} {name}")
        _check_losses([st["surr_after"], st["kl_after"], st["ent_after"]], th, ub, uspec, what + " after-losses")


@pytest.mark.parametrize("case", [c.id for c in GH.CASES if c.group == "colsum"])
def test_colsum_check_sees_a_one_row_short_reference(gpu_available, case):
    """The colsum check is not vacuous: against a reference whose sums lack the last row (the row of the short last
    block; n_global as before), the engine's g misses the same bar on its tail and as a whole."""
    import torch
    spec, theta, b = GH.feed(case)
    n, A = b.X.shape[0], spec.act_dim
    g64, g32 = GH.vec_refs(case)["g"]
    wrong = G.policy_grad(theta, b.rows(0, n - 1, n), spec, torch.float64)
    with _engine(spec, b, theta) as e:
        g = e.policy_grad()
    for name, sl in (("tail", slice(-A, None)), ("whole", slice(None))):
        bar = max(REL, 4.0 * rel_l2(g32[sl], g64[sl]))
        right, short = rel_l2(g[sl], g64[sl]), rel_l2(g[sl], wrong[sl])
        log_margin(f"{case} g {name}: {right:.2e} against the reference, {short:.2e} against the one-row-short one "
                   f"(bar {bar:.1e})")
        assert right <= bar < short


# ---- 2. engine state ------------------------------------------------------------------------------------------
STATE_SHAPE = (128, [256, 256], 17)


def _state_feeds():
    """three feeds of one engine: n = 515, 129 (other rows), 515 again, each with its own old_logstd, which is
    also theta's log-std tail (theta_old = theta, so that the update takes its step and is not reverted); the
    network weights stay"""
    spec, theta, b = G.make_case((*STATE_SHAPE, 515), seed=21, perturb=0.0)
    rng = np.random.RandomState(22)
    feeds = []
    for lo, hi in ((0, 515), (300, 429), (0, 515)):
        th = theta.copy()
        old_logstd = b.old_logstd.copy()
        if feeds:
            old_logstd += (0.2 * rng.standard_normal(spec.act_dim)).astype(np.float32)
            th[spec.n_net:] = old_logstd
        sb = b.rows(lo, hi, 0)
        feeds.append((th, G.GaussBatch(sb.X, sb.actions, sb.advant, sb.old_mean, old_logstd)))
    return spec, feeds


def _feed_and_run(e, theta, b, v, updates):
    """set_flat + feed, then g, Hv, the losses and `updates` updates from theta; -> (stats, [arrays])"""
    e.set_flat(theta)
    e.set_batch_gaussian(b.X, b.actions, b.advant, b.old_mean, b.old_logstd)
    out = [e.policy_grad(), e.fvp(v, 0.1), e.losses()]
    for _ in range(updates):
        e.set_flat(theta)
        st = _update(e)
    assert st["cg_iters"] == 10 and not st["reverted"], st     # the step was taken: theta is a result, not theta_0
    return st, out + _update_vectors(e)


NAMES = ("g", "Hv", "losses", "update g", "stepdir", "fullstep", "theta")


def _fresh_runs(spec, feeds, v):
    """every feed on an engine of its own with max_rows = n, eager"""
    from trpo_amd import Engine
    from trpo_amd._lib import get_option, set_option
    saved = get_option("graphs")
    try:
        set_option("graphs", 0)
        out = []
        for theta, b in feeds:
            with Engine(spec.obs_dim, spec.hidden, spec.act_dim, max_rows=b.X.shape[0], dist="gaussian") as e:
                out.append(_feed_and_run(e, theta, b, v, 1))
        return out
    finally:
        set_option("graphs", saved)


def _compare_runs(got, want, what):
    """-> the names of the results that differ in any bit"""
    bad = []
    if got[0] != want[0]:
        bad.append("stats")
    for name, a, b_ in zip(NAMES, got[1], want[1]):
        assert np.all(np.isfinite(b_)), f"{what} {name}"
        if a.tobytes() != b_.tobytes():
            bad.append(f"{name} (rel L2 {rel_l2(a, b_):.2e})")
    return bad


@pytest.mark.parametrize("graphs", [0, 1])
def test_refeed_under_larger_max_rows(gpu_available, graphs):
    """One engine with max_rows = 4096 fed n = 515, 129, 515 with changing old_logstd and theta tails: after each
    feed g, Hv(damping 0.1), the losses and an update equal, bit for bit, a fresh engine with max_rows = n on the
    same feed.  graphs = 1: each feed's update runs three times (first seen, captured, replayed), so the third
    feed replays the graph captured under the first feed's old_logstd and theta."""
    from trpo_amd import Engine
    from trpo_amd._lib import get_option, set_option
    spec, feeds = _state_feeds()
    v = np.random.RandomState(23).standard_normal(spec.n_params).astype(np.float32)
    want = _fresh_runs(spec, feeds, v)
    saved = get_option("graphs")
    try:
        set_option("graphs", graphs)
        with Engine(spec.obs_dim, spec.hidden, spec.act_dim, max_rows=4096, dist="gaussian") as e:
            got = [_feed_and_run(e, theta, b, v, 3 if graphs else 1) for theta, b in feeds]
    finally:
        set_option("graphs", saved)
    # the feeds differ from each other: a stale result of an earlier feed cannot pass for the later one
    assert _compare_runs(want[2], want[0], "feed 3 vs feed 1") and want[2][1][0].tobytes() != want[0][1][0].tobytes()
    for i, (g_, w_) in enumerate(zip(got, want)):
        bad = _compare_runs(g_, w_, f"feed {i + 1}")
        log_margin(f"refeed graphs={graphs} feed {i + 1} (n = {feeds[i][1].X.shape[0]}): "
                   f"{'all bits equal' if not bad else 'differ: ' + ', '.join(bad)}")
        assert not bad, f"graphs={graphs} feed {i + 1}: {bad} differ from a fresh engine with max_rows = n"


def test_refeed_check_sees_a_one_row_short_feed(gpu_available):
    """The comparison of test_refeed_under_larger_max_rows is not vacuous: against a reference run whose second
    feed lacks its last row (a deliberately wrong reference), every result of that feed differs."""
    from trpo_amd import Engine
    spec, feeds = _state_feeds()
    v = np.random.RandomState(23).standard_normal(spec.n_params).astype(np.float32)
    theta, b = feeds[1]
    n = b.X.shape[0]
    with Engine(spec.obs_dim, spec.hidden, spec.act_dim, max_rows=4096, dist="gaussian") as e:
        got = _feed_and_run(e, theta, b, v, 1)
    wrong = _fresh_runs(spec, [(theta, b.rows(0, n - 1, 0))], v)[0]
    bad = _compare_runs(got, wrong, "one row short")
    log_margin(f"refeed against a one-row-short reference: differ: {', '.join(bad)}")
    assert len([x for x in bad if x != "stats"]) == len(NAMES)


@pytest.mark.parametrize("shape", [(17, [64, 64], 6, 515), (*STATE_SHAPE, 515)], ids=["o17h64x2a6", "c4g"])
def test_call_order_keeps_policy_grad(gpu_available, shape):
    """fvp first on a freshly fed engine, then policy_grad: the bits of policy_grad called first (the g_s rows live
    in a buffer the other passes may reuse).  eval_losses(theta2) is loss(th), which sets the parameters
    (include/trpo_engine.h): policy_grad after it has the bits of a fresh engine at theta2, and after
    eval_losses(theta) the bits of policy_grad called first again; fvp likewise."""
    spec, theta, b = G.make_case(shape, seed=24, perturb=0.02)
    v = np.random.RandomState(25).standard_normal(spec.n_params).astype(np.float32)
    theta2 = (theta.astype(np.float64) * (1 + 0.01 * np.random.RandomState(5).standard_normal(theta.shape)))
    theta2 = theta2.astype(np.float32)
    first = {}
    for name, th in (("theta", theta), ("theta2", theta2)):
        with _engine(spec, b, th) as e:
            g = e.policy_grad()
            first[name] = (g, e.fvp(v, 0.1))
            assert_vec_close(g, G.policy_grad(th, b, spec), REL, f"g at {name}")
    assert first["theta"][0].tobytes() != first["theta2"][0].tobytes()
    with _engine(spec, b, theta) as e:
        hv = e.fvp(v, 0.1)
        g_after_fvp = e.policy_grad()
        l2 = e.eval_losses(theta2)
        g2_after_eval = e.policy_grad()
        hv2 = e.fvp(v, 0.1)
        l1 = e.eval_losses(theta)
        g_back = e.policy_grad()
        hv_back = e.fvp(v, 0.1)
    assert np.all(np.isfinite(l2)) and np.all(np.isfinite(l1))
    assert hv.tobytes() == first["theta"][1].tobytes(), "fvp before policy_grad"
    assert g_after_fvp.tobytes() == first["theta"][0].tobytes(), "policy_grad after fvp"
    assert g2_after_eval.tobytes() == first["theta2"][0].tobytes(), "policy_grad after eval_losses(theta2)"
    assert hv2.tobytes() == first["theta2"][1].tobytes(), "fvp after eval_losses(theta2)"
    assert g_back.tobytes() == first["theta"][0].tobytes(), "policy_grad after eval_losses(theta2), eval_losses(theta)"
    assert hv_back.tobytes() == first["theta"][1].tobytes(), "fvp after eval_losses(theta2), eval_losses(theta)"


# ---- 3. act_gaussian's edges ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 130])
@pytest.mark.parametrize("dims", [(3, [8], 1), (24, [32], 33), (17, [256, 256], 6), (9, [40], 64)],
                         ids=["o3h8a1", "o24h32a33", "o17h256x2a6", "o9h40a64"])
def test_act_gaussian_edges(gpu_available, dims, n):
    from trpo_amd import Engine
    spec = G.GaussSpec(*dims)
    rng = np.random.RandomState(1000 * spec.act_dim + n)
    theta = G.init_theta(spec, rng)
    X = rng.standard_normal((n, spec.obs_dim)).astype(np.float32)
    xi = rng.standard_normal((n, spec.act_dim))
    with Engine(spec.obs_dim, spec.hidden, spec.act_dim, max_rows=4, dist="gaussian") as e:
        e.set_flat(theta)
        acts, mean, logstd = e.act_gaussian(X, xi, train=True)
        assert acts.shape == mean.shape == (n, spec.act_dim) and acts.dtype == mean.dtype == np.float32
        assert np.array_equal(logstd, theta[spec.n_net:])
        ref = G.mean_np(theta, X, spec)
        log_margin(f"act {dims} n={n}: mean rel L2 {rel_l2(mean, ref):.2e} (bar {REL:.0e})")
        assert_vec_close(mean, ref, REL, "act mean")
        want = (mean.astype(np.float64) + np.exp(logstd.astype(np.float64)) * xi).astype(np.float32)
        assert np.array_equal(acts, want)
        assert not np.array_equal(acts, mean)
        acts0, mean0, _ = e.act_gaussian(X, None, train=False)
        assert np.array_equal(mean0, mean) and np.array_equal(acts0, mean)
        # no rows: empty arrays and the log-std
        a0, m0, s0 = e.act_gaussian(np.zeros((0, spec.obs_dim), np.float32), np.zeros((0, spec.act_dim)), train=True)
        assert a0.shape == m0.shape == (0, spec.act_dim) and np.array_equal(s0, theta[spec.n_net:])


def test_act_gaussian_refuses_65_and_the_engine_still_updates(gpu_available):
    from trpo_amd._lib import EngineError
    spec, theta, b = G.make_case((9, [40], 65, 70), seed=26, perturb=0.0)
    xi = np.random.RandomState(27).standard_normal((70, 65))
    with _engine(spec, b, theta) as e:
        g0 = e.policy_grad()
        for train, normals in ((True, xi), (False, None)):
            with pytest.raises(EngineError, match=r"act_dim must be <= 64"):
                e.act_gaussian(b.X, normals, train=train)
        assert np.array_equal(e.policy_grad(), g0)
        assert_vec_close(g0, G.policy_grad(theta, b, spec), REL, "g at A = 65")
        st = _update(e)
        th = e.get_flat()
        assert st["cg_iters"] == 10 and np.all(np.isfinite(th)) and not np.array_equal(th, theta)
        _check_losses([st["surr_after"], st["kl_after"], st["ent_after"]], th, b, spec, "A = 65 after-losses")


# ---- 4. two ranks -------------------------------------------------------------------------------------------------
def test_two_ranks_gaussian_g17(gpu_available):
    """Two processes on one GPU run a Gaussian update on uneven shards of 3001 rows of (17, [64, 64], 6): ranks
    bitwise identical, Hv, stepdir and theta (the log-std tail also on its own) within 1e-5 of one engine holding
    all rows, the same k, every graph replay bitwise equal to eager."""
    run_mrank("--host-allreduce", "--graphs", "--dist", "gaussian", "--dims", "g17", "--rows", "3001")


def test_two_ranks_gaussian_c4(gpu_available):
    """The same at (128, [256, 256], 17) with 4001 rows: the f16-split row GEMMs' running-max scales are per rank."""
    run_mrank("--host-allreduce", "--graphs", "--dist", "gaussian", "--dims", "c4", "--rows", "4001")
