"""Fisher-vector products on every k-th row of the batch (Engine.set_fvp_subsample; include/trpo_engine.h).

What is held to what:
  * the gather: Engine.fvp_subsample_fetch() equals the fed arrays [::k], bit for bit;
  * fvp and cg: an engine E with max_rows = M and stride k equals, bit for bit, a plain engine of max_rows =
    ceil(M / k) that was fed X[::k], actions[::k], advant[::k], old[::k] at the same theta (the Fisher child is such
    an engine: its capacity rule fixes the slab geometry and the plane strides);
  * the whole update against the float64 composition of tests/fvp_subsample_ref.py: g, stepdir, fullstep and theta
    norm-relative within max(1e-5, 4 x the float32 composition's own error), the measure and bar of
    tests/test_gpu_parity.py; the line search's k and the CG count exact;
  * graph capture / replay, the cache flags, the agent and the refusals.
"""
import functools

import numpy as np
import pytest
import torch

import fvp_subsample_ref as R
import gauss_ref as G
from conftest import assert_vec_close, golden, rel_l2, spec_of
from oracle import trpo_oracle as O

pytestmark = pytest.mark.gpu
REL = 1e-5
N_MAX = 69921


def ceil_div(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------- the gather
@functools.lru_cache(maxsize=None)
def _feed(obs, A, gaussian):
    """One feed of N_MAX rows per shape; smaller batches are its leading rows from a row offset."""
    rng = np.random.RandomState(obs * 1000 + A + (500 if gaussian else 0))
    X = rng.standard_normal((N_MAX, obs)).astype(np.float32)
    adv = rng.standard_normal(N_MAX).astype(np.float32)
    old = rng.uniform(0.1, 1.0, (N_MAX, A)).astype(np.float32)
    if gaussian:
        act = rng.standard_normal((N_MAX, A)).astype(np.float32)
    else:
        old /= old.sum(1, keepdims=True)
        act = rng.randint(0, A, N_MAX).astype(np.int64)
    for a in (X, adv, old, act):
        a.setflags(write=False)
    return X, act, adv, old


def _row_counts(k):
    return sorted({1, 2, k - 1, k, k + 1, 255, 256, 257, 2 * k * 128 + 1, N_MAX} - {0})


@pytest.mark.parametrize("k", [2, 3, 5, 7])
@pytest.mark.parametrize("obs,A,gaussian", [(3, 2, False), (11, 3, False), (128, 17, False), (128, 18, False),
                                            (3, 1, True), (11, 6, True)])
def test_gather_bit_exact(gpu_available, k, obs, A, gaussian):
    """Every array of the Fisher feed equals the fed array [::k], at every row-count edge, re-feeding one engine with
    batches of other sizes (a stale or partly overwritten child would show the previous batch's rows)."""
    from trpo_amd import Engine
    X, act, adv, old = _feed(obs, A, gaussian)
    eng = Engine(obs, [8], A, max_rows=N_MAX, dist="gaussian" if gaussian else "categorical")
    eng.set_fvp_subsample(k)
    logstd = np.linspace(-1.0, 0.5, A).astype(np.float32)
    counts = _row_counts(k)
    for j, n in enumerate(counts[::-1] + counts):      # shrinking, then growing
        lo = (7 * j) % (N_MAX - n + 1)                  # another batch every time
        sl = slice(lo, lo + n)
        if gaussian:
            eng.set_batch_gaussian(X[sl], act[sl], adv[sl], old[sl], logstd)
        else:
            eng.set_batch(X[sl], act[sl], adv[sl], old[sl])
        assert eng.fvp_subsample == (k, ceil_div(n, k))
        got = eng.fvp_subsample_fetch()
        for name, want in (("states", X[sl]), ("actions", act[sl]), ("old", old[sl]), ("advant", adv[sl])):
            assert got[name].shape == want[::k].shape, (name, n)
            assert np.array_equal(got[name], want[::k]), (name, n, k)
    eng.close()


# -------------------------------------------------------------------------- fvp and cg against a two-engine composition
def _cat_pair(obs, hidden, A, n, k, seed=7):
    """(E with stride k, E_sub plain with the rows [::k], spec, data): max_rows M = n + 5 and ceil(M / k)."""
    from trpo_amd import Engine
    spec = O.PolicySpec(obs, hidden, A)
    d = O.synthetic_batch(spec, n, seed=seed)
    adv = d["advant"].astype(np.float32)
    M = n + 5
    E = Engine(obs, hidden, A, max_rows=M)
    E.set_fvp_subsample(k)
    E.set_flat(d["theta"])
    E.set_batch(d["X"], d["actions"], adv, d["old_dist"])
    Es = Engine(obs, hidden, A, max_rows=ceil_div(M, k))
    Es.set_flat(d["theta"])
    Es.set_batch(d["X"][::k], d["actions"][::k], adv[::k], d["old_dist"][::k])
    return E, Es, spec, d


def _gauss_pair(shape, k, seed=3):
    from trpo_amd import Engine
    spec, theta, b = G.make_case(shape, seed=seed)
    n = shape[3]
    M = n + 5
    E = Engine(spec.obs_dim, spec.hidden, spec.act_dim, max_rows=M, dist="gaussian")
    E.set_fvp_subsample(k)
    E.set_flat(theta)
    E.set_batch_gaussian(b.X, b.actions, b.advant, b.old_mean, b.old_logstd)
    Es = Engine(spec.obs_dim, spec.hidden, spec.act_dim, max_rows=ceil_div(M, k), dist="gaussian")
    Es.set_flat(theta)
    bs = R.sub_gauss_batch(b, k)
    Es.set_batch_gaussian(bs.X, bs.actions, bs.advant, bs.old_mean, bs.old_logstd)
    return E, Es, spec


def _assert_fvp_cg_bitwise(E, Es, P, what):
    rs = np.random.RandomState(11)
    v = rs.standard_normal(P).astype(np.float32)
    b = (0.05 * rs.standard_normal(P)).astype(np.float32)
    for damping in (0.0, 0.1):
        assert np.array_equal(E.fvp(v, damping), Es.fvp(v, damping)), f"{what}: fvp, damping {damping}"
    x, it = E.cg(b, 10, 1e-10, 0.1)
    xs, its = Es.cg(b, 10, 1e-10, 0.1)
    assert it == its and np.array_equal(x, xs), f"{what}: cg"
    assert np.array_equal(E.fvp(v, 0.1), Es.fvp(v, 0.1)), f"{what}: fvp after cg"
    assert np.all(np.isfinite(x)) and np.any(x != 0.0)


# one shape per FVP path: fused (one hidden layer) and fused16 / chain (4, [64], 2), (11, [64, 64], 3); the fused tail
# with rfwd01 / rbwd0 (17 actions) and the per-layer path (18 actions) at n = 4001, k = 3 (neither n nor n_sub = 1334 a
# multiple of 256); three odd layers
@pytest.mark.parametrize("obs,hidden,A,n,k", [(4, [64], 2, 1537, 5), (11, [64, 64], 3, 1537, 5),
                                             (128, [256, 256], 17, 4001, 3), (128, [256, 256], 18, 4001, 3),
                                             (17, [33, 65, 31], 5, 1029, 4)])
def test_fvp_cg_bitwise_categorical(gpu_available, obs, hidden, A, n, k):
    E, Es, spec, _ = _cat_pair(obs, hidden, A, n, k)
    assert E.fvp_subsample == (k, ceil_div(n, k))
    _assert_fvp_cg_bitwise(E, Es, spec.n_params, f"{(obs, hidden, A)} x {n}, k = {k}")
    E.close()
    Es.close()


@pytest.mark.parametrize("shape,k", [((17, [64, 64], 6, 2001), 5), ((3, [64], 1, 771), 2)])
def test_fvp_cg_bitwise_gaussian(gpu_available, shape, k):
    E, Es, spec = _gauss_pair(shape, k)
    _assert_fvp_cg_bitwise(E, Es, spec.n_params, f"gaussian {shape}, k = {k}")
    E.close()
    Es.close()


# ------------------------------------------------------------------------------------- the whole update against float64
def _check_update(E, st, ref, ref32, what):
    from trpo_amd._lib import VEC_FULLSTEP, VEC_G, VEC_STEPDIR
    got = {"g": E.get_vector(VEC_G), "stepdir": E.get_vector(VEC_STEPDIR), "fullstep": E.get_vector(VEC_FULLSTEP),
           "theta": E.get_flat()}
    want = {"g": ref.g, "stepdir": ref.stepdir, "fullstep": ref.fullstep, "theta": ref.theta_new}
    want32 = {"g": ref32.g, "stepdir": ref32.stepdir, "fullstep": ref32.fullstep, "theta": ref32.theta_new}
    rows = []
    for name in got:
        bar = max(REL, 4.0 * rel_l2(want32[name], want[name]))
        rows.append((name, rel_l2(got[name], want[name]), bar))
        print(f"{what} {name}: engine rel error {rows[-1][1]:.3e}, float32 composition {rel_l2(want32[name], want[name]):.3e},"
              f" bar {bar:.3e}")
    print(f"{what}: k {st['k']} (ref {ref.k}), cg_iters {st['cg_iters']} (ref {ref.cg_iters}), reverted "
          f"{st['reverted']} (ref {ref.reverted})")
    assert st["k"] == ref.k and st["cg_iters"] == ref.cg_iters and bool(st["reverted"]) == ref.reverted
    for name, err, bar in rows:
        assert err <= bar, f"{what} {name}: {err:.3e} > {bar:.3e}"


@pytest.mark.parametrize("obs,hidden,A,n,k", [(11, [64, 64], 3, 3000, 5), (128, [256, 256], 18, 4001, 3)])
def test_update_vs_float64_categorical(gpu_available, obs, hidden, A, n, k):
    from trpo_amd import Engine, UpdateParams
    spec = O.PolicySpec(obs, hidden, A)
    d = O.synthetic_batch(spec, n, seed=7)
    batch = O.Batch(d["X"], d["actions"], d["advant"], d["old_dist"])
    ref = R.categorical_update(d["theta"], batch, spec, k, np.float64)
    ref32 = R.categorical_update(d["theta"], batch, spec, k, np.float32)
    plain = R.categorical_update(d["theta"], batch, spec, 1, np.float64)
    assert rel_l2(plain.stepdir, ref.stepdir) > 1e-3     # the case tells F_sub from F
    E = Engine(obs, hidden, A, max_rows=n)
    E.set_fvp_subsample(k)
    E.set_flat(d["theta"])
    E.set_batch(d["X"], d["actions"], d["advant"].astype(np.float32), d["old_dist"])
    st = E.update(UpdateParams())
    _check_update(E, st, ref, ref32, f"{(obs, hidden, A)} x {n}, k = {k}")
    E.close()


def test_update_vs_float64_gaussian(gpu_available):
    from trpo_amd import Engine, UpdateParams
    shape, k = (17, [64, 64], 6, 2001), 5
    spec, theta, b = G.make_case(shape, seed=3, perturb=0.0)
    ref = R.gaussian_update(theta, b, spec, k, torch.float64)
    ref32 = R.gaussian_update(theta, b, spec, k, torch.float32)
    assert rel_l2(R.gaussian_update(theta, b, spec, 1, torch.float64).stepdir, ref.stepdir) > 1e-3
    E = Engine(spec.obs_dim, spec.hidden, spec.act_dim, max_rows=shape[3], dist="gaussian")
    E.set_fvp_subsample(k)
    E.set_flat(theta)
    E.set_batch_gaussian(b.X, b.actions, b.advant, b.old_mean, b.old_logstd)
    st = E.update(UpdateParams())
    _check_update(E, st, ref, ref32, f"gaussian {shape}, k = {k}")
    E.close()


def test_stepwise_matches_fused_with_key(gpu_available):
    """update_stepwise goes through Engine.fvp / Engine.cg, so the config key reaches it: the bar of
    tests/test_gpu_parity.py::test_stepwise_utils_surface_matches_fused, and both differ from the plain update."""
    from trpo_amd import TRPOAgent
    from trpo_amd.agent import CONFIG
    d = golden("update_c2.npz")
    spec = spec_of(d)
    batch = {"state": d["X"], "action": d["actions"], "action_dist": d["old_dist"],
             "advant": np.asarray(d["advant"], np.float32)}
    thetas = {}
    for how, key in (("update", 4), ("update_stepwise", 4), ("update", None)):
        cfg = dict(CONFIG) if key is None else {**CONFIG, "fvp_subsample": key}
        ag = TRPOAgent(spec.obs_dim, spec.n_actions, spec.hidden, max_rows=4096, theta=d["theta"], config=cfg)
        assert ag.engine.fvp_subsample[0] == (key or 1)
        st = getattr(ag, how)(batch)
        thetas[(how, key)] = (ag.gf().copy(), st["kl_after"])
        ag.engine.close()
    (t1, kl1), (t2, kl2), (t0, _) = thetas[("update", 4)], thetas[("update_stepwise", 4)], thetas[("update", None)]
    assert_vec_close(t1, t2, REL, "fused vs stepwise, fvp_subsample = 4")
    assert kl2 == pytest.approx(kl1, rel=REL)
    assert rel_l2(t1, t0) > 1e-4


# ------------------------------------------------------------------------------------------------- graph and cache
def _rewards_engine(spec, d, n, k):
    from trpo_amd import Engine
    e = Engine(spec.obs_dim, spec.hidden, spec.n_actions, max_rows=n)
    if k is not None:
        e.set_fvp_subsample(k)
    e.set_flat(d["theta"])
    e.set_batch(d["X"], d["actions"], None, d["old_dist"])
    e.set_rewards(d["rewards"], d["starts"])
    return e


@pytest.mark.parametrize("dims", [((11, [64, 64], 3), 3000), ((128, [256, 256], 18), 4001)])
def test_graph_replay_bitwise(gpu_available, dims):
    """eager; then first-seen, capture, replay, replay (the pattern of tests/test_gpu_comm.py), the advantages computed
    inside the prefix so that the gather sits behind them in the graph: theta and the stats are bit-identical over
    the five runs, and differ from a plain engine's (the stride took effect)."""
    from trpo_amd import UpdateParams
    from trpo_amd._lib import get_option, set_option
    (obs, hidden, A), n = dims
    spec = O.PolicySpec(obs, hidden, A)
    d = O.synthetic_batch(spec, n, seed=7)
    prm = UpdateParams(residual_tol=0.0, compute_advantages=True)
    saved = get_option("graphs")
    try:
        e = _rewards_engine(spec, d, n, 5)
        runs = []
        for graphs in (0, 1, 1, 1, 1):
            set_option("graphs", graphs)
            e.set_flat(d["theta"])
            st = e.update(prm)
            runs.append((st, e.get_flat()))
        e.close()
        set_option("graphs", 0)
        e1 = _rewards_engine(spec, d, n, None)
        st_plain = e1.update(prm)
        th_plain = e1.get_flat()
        e1.close()
    finally:
        set_option("graphs", saved)
    st0, th0 = runs[0]
    for i, (st, th) in enumerate(runs):
        assert np.array_equal(th, th0), f"run {i}: theta differs from the eager run"
        assert st == st0, f"run {i}: {st} vs {st0}"
    assert not np.array_equal(th0, th_plain) and st0["shs"] != st_plain["shs"]   # the stride took effect


def test_stride_1_5_1_is_the_plain_engine(gpu_available):
    from trpo_amd import UpdateParams
    spec = O.PolicySpec(11, [64, 64], 3)
    n = 3000
    d = O.synthetic_batch(spec, n, seed=7)
    prm = UpdateParams(residual_tol=0.0, compute_advantages=True)
    plain = _rewards_engine(spec, d, n, None)
    want = [(plain.update(prm), plain.get_flat())]
    plain.close()
    e = _rewards_engine(spec, d, n, 1)
    got = {}
    for k in (1, 5, 1):
        e.set_fvp_subsample(k)
        assert e.fvp_subsample == (k, ceil_div(n, k))
        e.set_flat(d["theta"])
        got[k] = (e.update(prm), e.get_flat())      # the second k = 1 overwrites the first
        if k == 1:
            assert got[1][0] == want[0][0] and np.array_equal(got[1][1], want[0][1])
    e.close()
    assert not np.array_equal(got[5][1], want[0][1])


def test_set_flat_between_fvps(gpu_available):
    E, Es, spec, d = _cat_pair(11, [64, 64], 3, 1537, 3)
    v = np.random.RandomState(5).standard_normal(spec.n_params).astype(np.float32)
    h1 = E.fvp(v, 0.1)
    assert np.array_equal(h1, Es.fvp(v, 0.1))
    theta2 = (d["theta"] * (1.0 + 0.05 * np.random.RandomState(6).standard_normal(spec.n_params))).astype(np.float32)
    E.set_flat(theta2)
    Es.set_flat(theta2)
    h2 = E.fvp(v, 0.1)
    assert np.array_equal(h2, Es.fvp(v, 0.1))
    assert not np.array_equal(h1, h2)
    E.close()
    Es.close()


@pytest.mark.parametrize("obs,hidden,A,n,k,opt", [(11, [64, 64], 3, 1537, 5, "fused"),
                                                 (128, [256, 256], 17, 2049, 3, "tail")])
def test_option_change_reprepares_the_child(gpu_available, obs, hidden, A, n, k, opt):
    """The other kernel path after a prepare on the first: the child re-prepares as a plain engine does."""
    from trpo_amd._lib import get_option, set_option
    E, Es, spec, _ = _cat_pair(obs, hidden, A, n, k)
    v = np.random.RandomState(9).standard_normal(spec.n_params).astype(np.float32)
    saved = get_option(opt)
    try:
        first = E.fvp(v, 0.0)
        assert np.array_equal(first, Es.fvp(v, 0.0))
        set_option(opt, 0)
        second = E.fvp(v, 0.0)
        assert np.array_equal(second, Es.fvp(v, 0.0))
        set_option(opt, saved)
        assert np.array_equal(E.fvp(v, 0.0), first)
    finally:
        set_option(opt, saved)
    assert rel_l2(second, first) < 1e-4
    E.close()
    Es.close()


# ------------------------------------------------------------------------------------------------------- the agent
@pytest.mark.parametrize("env,extra", [("CartPole-v0", {}),
                                       ("Pendulum-v1", {"gae_lambda": 0.95, "bootstrap_truncated": True})])
def test_learn_with_key(gpu_available, env, extra):
    """Each iteration's theta is, bit for bit, what a fresh engine with stride 4 gives when fed that record's rollout
    and advantages from theta_before."""
    from trpo_amd import Engine, TRPOAgent, UpdateParams
    from trpo_amd.agent import CONFIG
    from trpo_amd.engine import CONT_ENVS, cont_env_info, env_info
    cont = env in CONT_ENVS
    info = cont_env_info(env) if cont else env_info(env)
    A = info["act_dim"] if cont else info["n_actions"]
    config = {**CONFIG, "env": env, "fvp_subsample": 4, **extra}
    n_envs = 4
    worst = n_envs * (ceil_div(config["episodes_per_roll"], n_envs) + min(config["max_steps"], info["time_limit"]) - 1)
    agent = TRPOAgent(info["obs_dim"], A, hidden=[64], max_rows=worst, config=config)
    hist = agent.learn(max_iterations=2, n_envs=n_envs, record=True, log=None)
    assert agent.engine.fvp_subsample[0] == 4
    agent.engine.close()
    assert len(hist) == 2
    prm = UpdateParams(cg_iters=10, residual_tol=1e-10, cg_damping=config["cg_damping"], max_kl=config["max_kl"],
                       compute_advantages=False)
    moved, differs = [], []
    for h in hist:
        roll = h["rollout"]
        adv = h["advantages"].astype(np.float32)
        thetas = {}
        for k in (4, 1):
            e = Engine(info["obs_dim"], [64], A, max_rows=worst, dist="gaussian" if cont else "categorical")
            e.set_fvp_subsample(k)
            e.set_flat(h["theta_before"])
            if cont:
                e.set_batch_gaussian(roll["obs32"], roll["actions"], adv, roll["means"], roll["logstd"])
            else:
                e.set_batch(roll["obs32"], roll["actions"], adv, roll["action_dists"])
            e.update(prm)
            thetas[k] = e.get_flat()
            e.close()
        assert np.array_equal(h["theta"], thetas[4]), h["iteration"]
        moved.append(not np.array_equal(h["theta"], h["theta_before"]))
        differs.append(not np.array_equal(thetas[1], thetas[4]))
        print(f"{env} iteration {h['iteration']}: k {h['k']}, reverted {h['reverted']}, moved {moved[-1]}, differs from "
              f"the plain engine's {differs[-1]}")
    # an update whose line search accepts nothing leaves theta where it was, with or without the key: the key must
    # have taken effect wherever theta moved, and it moved at least once
    assert any(moved) and differs == moved


# ------------------------------------------------------------------------------------------------------- refusals
def test_refusals(gpu_available):
    from trpo_amd import Engine, TRPOAgent, UpdateParams
    from trpo_amd._lib import EngineError
    from trpo_amd.agent import CONFIG
    spec = O.PolicySpec(11, [64, 64], 3)
    n = 600
    d = O.synthetic_batch(spec, n, seed=2)
    adv = d["advant"].astype(np.float32)
    e = Engine(11, [64, 64], 3, max_rows=n)
    e.set_flat(d["theta"])
    e.set_batch(d["X"], d["actions"], adv, d["old_dist"])
    for bad in (0, -3):
        with pytest.raises(EngineError, match="stride must be >= 1"):
            e.set_fvp_subsample(bad)
    assert e.fvp_subsample == (1, n)
    # a feed of a multi-rank run while k > 1, in either order
    e.set_fvp_subsample(3)
    with pytest.raises(EngineError, match="n_global == n"):
        e.set_batch(d["X"], d["actions"], adv, d["old_dist"], n_global=2 * n)
    assert e.fvp_subsample == (3, ceil_div(n, 3))        # the refused feed left the old one in place
    e.set_fvp_subsample(1)
    e.set_batch(d["X"], d["actions"], adv, d["old_dist"], n_global=2 * n)
    with pytest.raises(EngineError, match="n_global == n"):
        e.set_fvp_subsample(3)
    assert e.fvp_subsample[0] == 1
    e.set_batch(d["X"], d["actions"], adv, d["old_dist"])
    # world > 1, in either order
    calls = []
    e.set_fvp_subsample(3)
    with pytest.raises(EngineError, match="single-process"):
        e.comm_set_host_allreduce(lambda arr: calls.append(arr.size), 0, 2)
    with pytest.raises(EngineError, match="single-process"):
        e.comm_init(bytes(128), 0, 2)
    assert e.comm_info()["transport"] == "none" and e.comm_info()["world"] == 1
    e.set_fvp_subsample(1)
    e.comm_set_host_allreduce(lambda arr: calls.append(arr.size), 0, 2)
    with pytest.raises(EngineError, match="single-process"):
        e.set_fvp_subsample(3)
    assert e.fvp_subsample[0] == 1 and calls == []
    e.close()
    # the engine works afterwards: the same refusals, then an update equal to an engine that saw none of them
    thetas = []
    for refused in (True, False):
        e = Engine(11, [64, 64], 3, max_rows=n)
        e.set_fvp_subsample(3)
        e.set_flat(d["theta"])
        e.set_batch(d["X"], d["actions"], adv, d["old_dist"])
        if refused:
            with pytest.raises(EngineError):
                e.set_fvp_subsample(0)
            with pytest.raises(EngineError):
                e.set_batch(d["X"], d["actions"], adv, d["old_dist"], n_global=n + 1)
            with pytest.raises(EngineError):
                e.comm_set_host_allreduce(lambda arr: None, 0, 2)
        e.update(UpdateParams())
        thetas.append(e.get_flat())
        e.close()
    assert np.array_equal(thetas[0], thetas[1]) and not np.array_equal(thetas[0], d["theta"])
    # the agent: set_ranks(world > 1) with the key raises the engine's refusal
    ag = TRPOAgent(11, 3, [64, 64], max_rows=n, config={**CONFIG, "fvp_subsample": 3})
    with pytest.raises(EngineError, match="single-process"):
        ag.set_ranks(0, 2, host_allreduce=True)
    ag.engine.close()
