"""The diagonal-Gaussian engine (TRPO_DIST_GAUSSIAN) against the float64 reference tests/gauss_ref.py.

Bars (all set against float64; the float32 reference's own errors are in tests/test_gauss_ref.py):
  vectors (g, Hv, stepdir, fullstep, theta): conftest.assert_vec_close at 1e-5, the log-std tail also on its own;
  surr: |d| <= 1e-5 (1/N) sum |adv_n r_n|;  ent: |d| <= 1e-5 sum_d (|s_d| + 1.42);
  kl:   |d| / |kl| <= max(1e-5, 4 x the float32 reference's own relative kl error on the same inputs), at most 1e-4.
Every figure is printed before it is asserted.
"""
import functools

import numpy as np
import pytest

from conftest import assert_vec_close, rel_l2
from gae_ref import gae_ref
import gauss_ref as G
from oracle import trpo_oracle as O

pytestmark = pytest.mark.gpu

SHAPE_IDS = ["o3h8a1n1", "o11h64x2a3n257", "o17h64x2a6n3001", "o128h256x2a17n515", "o24h32a33n70"]
BIG = 3                                   # (128, [256, 256], 17, 515): fwd01, X's planes, rbwd0
WIDE = "o128h256x2a17n515-wide"           # the same shape with logstd spread over [-3, 1]
TILES4 = "o8h16a100n40"                   # beyond the issue's shapes: 100 action dimensions, four 32-lane head tiles
LOSS_CASES = SHAPE_IDS + [TILES4]
VEC_CASES = SHAPE_IDS + [WIDE, TILES4]
UPDATE_CASES = SHAPE_IDS[1:]
# the cases of tests/test_gauss_ref.py, whose float32 errors that file bounds
SEEDS = dict(zip(SHAPE_IDS, [0, 1, 2, 3, 4]))
UPDATE_SEEDS = dict(zip(SHAPE_IDS, [0, 11, 12, 14, 13]))


@functools.lru_cache(maxsize=None)
def _case(case):
    """(spec, theta, batch) of the loss / gradient / FVP tests: theta_old = theta perturbed by 2 %."""
    if case == TILES4:
        return G.make_case((8, [16], 100, 40), seed=5, perturb=0.02)
    wide = case == WIDE
    i = BIG if wide else SHAPE_IDS.index(case)
    return G.make_case(G.SHAPES[i], seed=33 if wide else SEEDS[case], perturb=0.02, wide_sigma=wide)


@functools.lru_cache(maxsize=None)
def _vec_refs(case):
    import torch
    spec, theta, b = _case(case)
    v = np.random.RandomState(77).standard_normal(spec.n_params).astype(np.float32)
    return v, G.policy_grad(theta, b, spec, torch.float64), G.fvp(theta, b, v, spec, torch.float64)


@functools.lru_cache(maxsize=None)
def _update_case(case, max_kl=0.01):
    import torch
    spec, theta, b = G.make_case(G.SHAPES[SHAPE_IDS.index(case)], UPDATE_SEEDS[case], perturb=0.0)
    return spec, theta, b, G.update(theta, b, spec, torch.float64, 10, 0.0, max_kl=max_kl)


def _engine(spec, b, theta, n_global=None):
    from trpo_amd import Engine
    e = Engine(spec.obs_dim, spec.hidden, spec.act_dim, max_rows=b.X.shape[0], dist="gaussian")
    e.set_flat(theta)
    e.set_batch_gaussian(b.X, b.actions, b.advant, b.old_mean, b.old_logstd, n_global=n_global)
    return e


def _check_losses(got, theta, b, spec, what):
    """the three bars of the module docstring for losses evaluated at `theta`"""
    import torch
    ref = G.losses(theta, b, spec, torch.float64)
    ref32 = G.losses(theta, b, spec, torch.float32)
    wsum = G.surr_weight_sum(theta, b, spec)
    s = np.asarray(theta, np.float64)[spec.n_net:]
    ent_scale = float(np.sum(np.abs(s) + 1.42)) * b.X.shape[0] / b.N
    kl_ref_err = abs(float(ref32[1]) - ref[1]) / abs(ref[1])
    kl_bar = min(1e-4, max(1e-5, 4.0 * kl_ref_err))   # tests/test_gauss_ref.py holds the float32 error to 2.5e-5
    d = np.abs(np.asarray(got, np.float64) - ref)
    print(f"{what}: surr err {d[0]:.3e} (bar {1e-5 * wsum:.3e}; f32 ref {abs(float(ref32[0]) - ref[0]):.3e})  "
          f"kl rel err {d[1] / abs(ref[1]):.3e} (bar {kl_bar:.3e}; f32 ref {kl_ref_err:.3e}; kl {ref[1]:.3e})  "
          f"ent err {d[2]:.3e} (bar {1e-5 * ent_scale:.3e})")
    assert d[0] <= 1e-5 * wsum, f"{what}: surr"
    assert d[1] <= kl_bar * abs(ref[1]), f"{what}: kl"
    assert d[2] <= 1e-5 * ent_scale, f"{what}: ent"


def _check_vec(got, ref, A, what):
    print(f"{what}: rel L2 {rel_l2(got, ref):.3e}  tail {rel_l2(got[-A:], ref[-A:]):.3e}")
    assert_vec_close(got, ref, 1e-5, what)
    assert_vec_close(got[-A:], ref[-A:], 1e-5, what + " (log-std tail)")


# ---- 1. losses -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LOSS_CASES)
def test_losses_and_eval_losses(gpu_available, case):
    spec, theta, b = _case(case)
    with _engine(spec, b, theta) as e:
        assert e.dist == "gaussian" and e.num_params == spec.n_params
        _check_losses(e.losses(), theta, b, spec, f"{case} losses")
        # another point: the line search's forward (trial weights, the loss head)
        theta2 = (theta.astype(np.float64) * (1 + 0.01 * np.random.RandomState(5).standard_normal(theta.shape)))
        theta2 = theta2.astype(np.float32)
        _check_losses(e.eval_losses(theta2), theta2, b, spec, f"{case} eval_losses")
        _check_losses(e.eval_losses(theta), theta, b, spec, f"{case} eval_losses(theta)")
        mean, logstd = e.action_mean()
        assert np.array_equal(logstd, theta[spec.n_net:])
        assert_vec_close(mean, G.mean_np(theta, b.X, spec), 1e-5, f"{case} action_mean")


# ---- 2. policy gradient and FVP -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", VEC_CASES)
def test_policy_grad_and_fvp(gpu_available, case):
    spec, theta, b = _case(case)
    v, g_ref, hv_ref = _vec_refs(case)
    A = spec.act_dim
    with _engine(spec, b, theta) as e:
        _check_vec(e.policy_grad(), g_ref, A, f"{case} g")
        for damping in (0.0, 0.1):
            _check_vec(e.fvp(v, damping), hv_ref + damping * v.astype(np.float64), A, f"{case} Hv damping {damping}")
        # deterministic: a second run of each gives the same bits
        g1, g2 = e.policy_grad(), e.policy_grad()
        h1, h2 = e.fvp(v, 0.1), e.fvp(v, 0.1)
        assert np.array_equal(g1, g2) and np.array_equal(h1, h2)


# ---- 3. the whole update ---------------------------------------------------------------------------------------
def _check_update(e, st, spec, theta, b, r, what):
    from trpo_amd._lib import VEC_FULLSTEP, VEC_G, VEC_STEPDIR
    A = spec.act_dim
    print(f"{what}: cg_iters {st['cg_iters']} k {st['k']} reverted {st['reverted']} (ref {r.cg_iters} {r.k} {r.reverted})")
    assert (st["cg_iters"], st["k"], bool(st["reverted"])) == (r.cg_iters, r.k, r.reverted)
    _check_vec(e.get_vector(VEC_G), r.g, A, what + " g")
    _check_vec(e.get_vector(VEC_STEPDIR), r.stepdir, A, what + " stepdir")
    _check_vec(e.get_vector(VEC_FULLSTEP), r.fullstep, A, what + " fullstep")
    _check_vec(e.get_flat(), r.theta_new, A, what + " theta")
    for name, ref in (("shs", r.shs), ("lm", r.lm), ("rate", r.rate)):
        err = abs(st[name] - ref) / abs(ref)
        print(f"{what}: {name} rel err {err:.3e}")
        assert err <= 1e-5, f"{what}: {name}"
    _check_losses([st["surr_after"], st["kl_after"], st["ent_after"]], r.theta_ls, b, spec, what + " after-losses")


@pytest.mark.parametrize("case", UPDATE_CASES)
def test_update(gpu_available, case):
    from trpo_amd import UpdateParams
    spec, theta, b, r = _update_case(case)
    with _engine(spec, b, theta) as e:
        st = e.update(UpdateParams(cg_iters=10, residual_tol=0.0))
        _check_update(e, st, spec, theta, b, r, case)


def test_update_backtracks(gpu_available):
    """max_kl = 100: the full step overshoots and the reference accepts the fourth trial (k = 3)"""
    from trpo_amd import UpdateParams
    case = SHAPE_IDS[1]
    spec, theta, b, r = _update_case(case, max_kl=100.0)
    assert r.k >= 1
    with _engine(spec, b, theta) as e:
        st = e.update(UpdateParams(cg_iters=10, residual_tol=0.0, max_kl=100.0))
        _check_update(e, st, spec, theta, b, r, case + " max_kl 100")


def test_update_with_gae_advantages(gpu_available):
    """compute_advantages under GAE(0.95) from rewards and a baseline, then the update on those advantages"""
    import torch
    from trpo_amd import UpdateParams
    case = SHAPE_IDS[2]
    spec, theta, b0 = G.make_case(G.SHAPES[2], 31, perturb=0.0)
    n = b0.X.shape[0]
    rng = np.random.RandomState(8)
    rewards, baseline = rng.uniform(0, 1, n), rng.standard_normal(n)
    starts = (rng.uniform(size=n) < 0.01).astype(np.uint8)
    starts[0] = 1
    adv = O.standardize(gae_ref(rewards, baseline, 0.99, 0.95, starts)[0])
    b = G.GaussBatch(b0.X, b0.actions, adv.astype(np.float32), b0.old_mean, b0.old_logstd)
    r = G.update(theta, b, spec, torch.float64, 10, 0.0)
    from trpo_amd import Engine
    with Engine(spec.obs_dim, spec.hidden, spec.act_dim, max_rows=n, dist="gaussian") as e:
        e.set_flat(theta)
        e.set_batch_gaussian(b.X, b.actions, None, b.old_mean, b.old_logstd)
        e.set_rewards(rewards, starts, baseline)
        e.set_advantage_estimator("gae", 0.95)
        st = e.update(UpdateParams(cg_iters=10, residual_tol=0.0, compute_advantages=True, gamma=0.99))
        _check_update(e, st, spec, theta, b, r, case + " GAE(0.95)")


# ---- 4. graph replay ---------------------------------------------------------------------------------------------
def _run_update(e, theta, **kw):
    from trpo_amd import UpdateParams
    from trpo_amd._lib import VEC_FULLSTEP, VEC_G, VEC_STEPDIR
    e.set_flat(theta)
    st = e.update(UpdateParams(cg_iters=10, residual_tol=0.0, **kw))
    return st, [e.get_vector(VEC_G), e.get_vector(VEC_STEPDIR), e.get_vector(VEC_FULLSTEP), e.get_flat()]


@pytest.mark.parametrize("case", [SHAPE_IDS[2], SHAPE_IDS[BIG]])
def test_graph_replay_bitwise(gpu_available, case):
    """eager (graphs = 0), first seen, captured and replayed updates on one engine: the same bits"""
    from trpo_amd._lib import get_option, set_option
    spec, theta, b, _ = _update_case(case)
    saved = get_option("graphs")
    try:
        with _engine(spec, b, theta) as e:
            set_option("graphs", 0)
            st0, v0 = _run_update(e, theta)
            set_option("graphs", 1)
            for name in ("first seen", "captured", "replayed", "replayed again"):
                st, v = _run_update(e, theta)
                assert st == st0, f"{name}: {st} vs {st0}"
                for a, b_ in zip(v, v0):
                    assert np.array_equal(a, b_), name
    finally:
        set_option("graphs", saved)


# ---- 5. shard additivity --------------------------------------------------------------------------------------
def test_shards_sum_to_the_whole_batch(gpu_available):
    """no communicator: rows [0, m) and [m, n) with n_global = n give partials that sum to the whole batch's
    g and Hv, tails included (each rank's log-std blocks are partials too)"""
    case = SHAPE_IDS[BIG]
    spec, theta, b = _case(case)
    v, g_ref, hv_ref = _vec_refs(case)
    n, m, A = b.X.shape[0], 129, spec.act_dim
    assert (n, m) == (515, 129)
    g = np.zeros(spec.n_params)
    hv = np.zeros(spec.n_params)
    for lo, hi in ((0, m), (m, n)):
        sb = b.rows(lo, hi, n)
        with _engine(spec, sb, theta, n_global=n) as e:
            g += e.policy_grad().astype(np.float64)
            hv += e.fvp(v, 0.0).astype(np.float64)
    _check_vec(g, g_ref, A, "sharded g")
    _check_vec(hv, hv_ref, A, "sharded Hv")


# ---- 6. RCCL at world 1 ---------------------------------------------------------------------------------------
def test_rccl_world1_update_bitwise(gpu_available):
    from trpo_amd import Engine
    case = SHAPE_IDS[2]
    spec, theta, b, _ = _update_case(case)
    runs = []
    for comm in (False, True):
        with _engine(spec, b, theta) as e:
            if comm:
                e.comm_init(Engine.comm_unique_id(), 0, 1)
                assert e.comm_info()["transport"] == "rccl"
            runs.append([_run_update(e, theta) for _ in range(3)])   # eager, captured, replayed
    for (st, v), (st0, v0) in zip(runs[1], runs[0]):
        assert st == st0
        for a, b_ in zip(v, v0):
            assert np.array_equal(a, b_)


# ---- 7. act ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 1000])
def test_act_gaussian(gpu_available, n):
    from trpo_amd import Engine
    spec = G.GaussSpec(17, [64, 64], 6)
    rng = np.random.RandomState(n)
    theta = G.init_theta(spec, rng)
    X = rng.standard_normal((n, spec.obs_dim)).astype(np.float32)
    xi = rng.standard_normal((n, spec.act_dim))
    with Engine(spec.obs_dim, spec.hidden, spec.act_dim, max_rows=4, dist="gaussian") as e:
        e.set_flat(theta)
        acts, mean, logstd = e.act_gaussian(X, xi, train=True)
        assert acts.shape == mean.shape == (n, spec.act_dim) and acts.dtype == np.float32
        assert np.array_equal(logstd, theta[spec.n_net:])
        assert_vec_close(mean, G.mean_np(theta, X, spec), 1e-5, "act mean")
        want = (mean.astype(np.float64) + np.exp(logstd.astype(np.float64)) * xi).astype(np.float32)
        assert np.array_equal(acts, want)
        acts0, mean0, _ = e.act_gaussian(X, None, train=False)
        assert np.array_equal(mean0, mean) and np.array_equal(acts0, mean)


# ---- 8. option sweep -------------------------------------------------------------------------------------------
def test_option_sweep(gpu_available):
    """at (128, [256, 256], 17, 515): fwd01, rbwd0, planes, split_f16 off in turn still meet the vector bars; the
    options whose kernels contain the softmax change no bit of a Gaussian FVP"""
    from trpo_amd._lib import get_option, set_option
    case = SHAPE_IDS[BIG]
    spec, theta, b = _case(case)
    v, g_ref, hv_ref = _vec_refs(case)
    A = spec.act_dim
    inert = {"fused": (0, 1, 2, 3), "tail": (0, 1), "hbwd2": (0, 1, 2), "head_fwd": (0, 1, 2), "rfwd01": (0, 1),
             "chain": (0, 1, 2, 3, 4)}
    names = ["fwd01", "rbwd0", "planes", "split_f16", *inert]
    saved = {k: get_option(k) for k in names}
    try:
        for opt in ("fwd01", "rbwd0", "planes", "split_f16"):
            set_option(opt, 0)
            with _engine(spec, b, theta) as e:     # split_f16 is read when the engine is created
                _check_vec(e.policy_grad(), g_ref, A, f"{opt}=0 g")
                for damping in (0.0, 0.1):
                    _check_vec(e.fvp(v, damping), hv_ref + damping * v.astype(np.float64), A,
                               f"{opt}=0 Hv damping {damping}")
            set_option(opt, saved[opt])
        with _engine(spec, b, theta) as e:
            base_hv, base_g = e.fvp(v, 0.1), e.policy_grad()
            for opt, values in inert.items():
                for val in values:
                    set_option(opt, val)
                    assert np.array_equal(e.fvp(v, 0.1), base_hv), f"{opt}={val} changed Hv"
                    assert np.array_equal(e.policy_grad(), base_g), f"{opt}={val} changed g"
                set_option(opt, saved[opt])
    finally:
        for k, val in saved.items():
            set_option(k, val)


# ---- 9. the wrong-kind calls ---------------------------------------------------------------------------------
def test_wrong_kind_calls_are_state_errors(gpu_available):
    from trpo_amd import Engine
    from trpo_amd._lib import EngineError, check, lib
    case = SHAPE_IDS[1]
    spec, theta, b = _case(case)
    v, g_ref, _ = _vec_refs(case)
    n = b.X.shape[0]
    with _engine(spec, b, theta) as e:
        g0 = e.policy_grad()
        calls = [
            lambda: e.set_batch(b.X, np.zeros(n, np.int64), b.advant, np.abs(b.old_mean)),
            lambda: e.action_dist(),
            lambda: e.act(b.X, np.zeros(n), train=True),
            lambda: e.rollout("CartPole-v0"),
            lambda: e.rollout_cartpole(),
            lambda: e.rollout_fetch_states(),
            lambda: e.rollout_fetch_ends(),
            lambda: check(lib.trpo_rollout_fetch(e._h, None, None, None, None, None, None, None, 0), "trpo_rollout_fetch"),
            lambda: check(lib.trpo_rollout_to_batch(e._h, n), "trpo_rollout_to_batch"),
        ]
        for call in calls:
            with pytest.raises(EngineError, match=r"rc=-4.*needs a categorical engine.*distribution is gaussian"):
                call()
        assert np.array_equal(e.policy_grad(), g0)        # the feed and the engine are as before
        _check_vec(e.policy_grad(), g_ref, spec.act_dim, "g after the refused calls")
    with Engine(spec.obs_dim, spec.hidden, 3, max_rows=n) as c:
        assert c.dist == "categorical"
        for call in (lambda: c.set_batch_gaussian(b.X, b.actions, b.advant, b.old_mean, b.old_logstd),
                     lambda: c.action_mean(),
                     lambda: c.act_gaussian(b.X, np.zeros((n, 3)), train=True)):
            with pytest.raises(EngineError, match=r"rc=-4.*needs a gaussian engine.*distribution is categorical"):
                call()
        # still usable as a categorical engine
        d = O.synthetic_batch(O.PolicySpec(spec.obs_dim, spec.hidden, 3), n, seed=1)
        c.set_flat(d["theta"])
        c.set_batch(d["X"], d["actions"], d["advant"].astype(np.float32), d["old_dist"])
        assert np.all(np.isfinite(c.losses()))
