"""Bootstrapping cut-off paths on the device: the rollout's per-path end records (rollout.hip), V(s_T) of the
cut-off paths through the VF (vf.hip), the engine's tail values, the GAE scan and learn().

References: tests/truncation_ref.py (the path ends replayed with the oracle's CartPole-v0 dynamics),
oracle/vf_oracle.py, tests/gae_ref.py.  Bars: the flags, lengths and rows exact; s_T to rtol 1e-13 / atol
1e-15 (test_cartpole_step_vs_oracle); float32 distributions to 1e-6 and the per-step arrays as in
test_gpu_rollout.py; V(s_T) to rel-L2 1e-4 (test_gpu_vf.py); returns rtol 1e-13 and standardised
advantages rtol 1e-11 / atol 1e-12 (test_gpu_gae.py).
"""
import numpy as np
import pytest

import truncation_ref as T
from conftest import rel_l2
from gae_ref import gae_ref
from oracle import trpo_oracle as O
from oracle import vf_oracle as V

pytestmark = pytest.mark.gpu

GAMMA, LAM = 0.95, 0.95


def _engine(max_rows=4096):
    from trpo_amd import Engine
    e = Engine(4, [64], 2, max_rows=max_rows)
    e.set_flat(T.theta())
    return e


def _check_rollout(out, ref):
    for k in ("actions", "rewards", "starts", "uniforms"):
        assert np.array_equal(out[k], ref[k]), k
    assert np.allclose(out["obs"], ref["obs"], rtol=0, atol=1e-12)
    assert np.array_equal(out["obs32"], out["obs"].astype(np.float32))
    assert np.max(np.abs(out["action_dists"] - ref["action_dists"])) < 1e-6


def _check_ends(got, ref):
    for k in ("truncated", "lengths", "end_rows"):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), k
    np.testing.assert_allclose(got["final_obs"], ref["final_obs"], rtol=1e-13, atol=1e-15)
    cut = ref["truncated"] == 1
    err = float(np.max(np.abs(got["final_dists"][cut] - ref["final_dist"][cut])))
    print(f"final_dists: max abs error {err:.3e} over {int(cut.sum())} cut-off paths")
    assert err < 1e-6
    assert np.all(got["final_dists"][~cut] == 0.0)


@pytest.fixture(scope="module")
def fed(gpu_available):
    """The shared rollout on the device, loaded as the feed, with an untrained VF's tails: the engine, its
    ends, the VF's feature matrix and the tail values (test 7 checks them; test 8 scans with them)."""
    from trpo_amd.vf import VFNet, vf_xavier_params
    e = _engine()
    n, paths = T.device_rollout(e)
    ends = e.rollout_fetch_ends()
    e.rollout_to_batch()
    net = VFNet(7, 4096)
    params = vf_xavier_params(7, (64, 64), np.random.RandomState(3))
    net.set_params(params)
    net.predict_tails(e.tail_view())
    feat = net.feature_matrix()
    no_tails = e.tail_values()                 # written, not yet marked set
    e.set_tail_values_in_place()
    d = {"engine": e, "n": n, "paths": paths, "ends": ends, "feat": feat, "params": params, "net": net,
         "no_tails": no_tails, "tails": e.tail_values()}
    yield d
    net.close()
    e.close()


@pytest.mark.parametrize("max_pathlength,time_limit", [(1000, 20), (12, 200)])
def test_ends_parity(gpu_available, max_pathlength, time_limit):
    """The time limit and max_pathlength both cut paths off; a step that terminates on the limit is a
    termination (5 such paths at limit 20, 7 at max_pathlength 12)."""
    ref_out, ref_ends = T.oracle(max_pathlength, time_limit)
    e = _engine()
    n, paths = T.device_rollout(e, max_pathlength, time_limit)
    assert (n, paths) == (len(ref_out["rewards"]), len(ref_ends["truncated"]))
    _check_rollout(e.rollout_fetch(), ref_out)
    got = e.rollout_fetch_ends()
    assert int(got["truncated"].sum()) == (24 if time_limit == 20 else 89)
    _check_ends(got, ref_ends)
    _check_rollout(e.rollout_fetch(), ref_out)          # fetching the ends disturbs nothing
    e.close()


def test_fetch_ends_needs_a_rollout(gpu_available):
    from trpo_amd._lib import EngineError
    e = _engine()
    with pytest.raises(EngineError, match=r"rc=-4.*no rollout"):
        e.rollout_fetch_ends()
    e.close()


def test_tie_goes_to_termination(gpu_available):
    rng = np.random.RandomState(6)
    budget = 150
    reset_u = rng.random_sample((1, budget, 4))
    act_u = rng.random_sample((1, budget + 999))
    e = _engine()
    e.rollout_cartpole(n_envs=1, n_timesteps=budget, time_limit=1000, reset_uniforms=reset_u,
                       action_uniforms=act_u, max_episodes_per_env=budget)
    first = e.rollout_fetch_ends()
    Lp = int(first["lengths"][0])
    assert first["truncated"][0] == 0 and 1 <= Lp < 1000
    e.rollout_cartpole(n_envs=1, n_timesteps=budget, time_limit=Lp, reset_uniforms=reset_u,
                       action_uniforms=np.ascontiguousarray(act_u[:, :budget + Lp - 1]),
                       max_episodes_per_env=budget)
    again = e.rollout_fetch_ends()
    assert again["lengths"][0] == Lp and again["truncated"][0] == 0
    assert np.array_equal(again["final_obs"][0], first["final_obs"][0])
    assert np.all(again["final_dists"][0] == 0.0)
    # one step fewer and the same path is cut off
    if Lp > 1:
        e.rollout_cartpole(n_envs=1, n_timesteps=budget, time_limit=Lp - 1, reset_uniforms=reset_u,
                           action_uniforms=np.ascontiguousarray(act_u[:, :budget + Lp - 2]),
                           max_episodes_per_env=budget)
        cut = e.rollout_fetch_ends()
        assert cut["lengths"][0] == Lp - 1 and cut["truncated"][0] == 1
    e.close()


def test_ends_deterministic(gpu_available):
    e = _engine(max_rows=1 << 13)
    kw = dict(n_envs=64, n_timesteps=4000, time_limit=20, seed=7)
    r1 = e.rollout_cartpole(**kw)
    plain = e.rollout_fetch()
    r2 = e.rollout_cartpole(**kw)
    ends1 = e.rollout_fetch_ends()
    between = e.rollout_fetch()
    f = _engine(max_rows=1 << 13)
    r3 = f.rollout_cartpole(**kw)
    ends2 = f.rollout_fetch_ends()
    assert r1 == r2 == r3
    for k in plain:
        assert np.array_equal(plain[k], between[k]), k
    for k in ends1:
        assert np.array_equal(ends1[k], ends2[k]), k
    assert 0 < int(ends1["truncated"].sum()) < len(ends1["truncated"])
    # consistent with the rollout's own arrays
    starts = np.flatnonzero(plain["starts"])
    assert np.array_equal(ends1["end_rows"], np.r_[starts[1:], r1[0]] - 1)
    assert np.array_equal(ends1["lengths"], ends1["end_rows"] - starts + 1)
    assert np.all(ends1["lengths"][ends1["truncated"] == 1] == 20)
    e.close()
    f.close()


def test_vf_tails(fed):
    from trpo_amd._lib import EngineError
    ends, n = fed["ends"], fed["n"]
    _check_ends(ends, T.oracle()[1])
    # the features of s_T, built from the device's own ends: exact
    want = np.concatenate([ends["final_obs"].astype(np.float32), ends["final_dists"],
                           (ends["lengths"] / 10.0).astype(np.float32)[:, None]], axis=1)
    assert fed["feat"].shape == (fed["paths"], 7) and np.array_equal(fed["feat"], want)
    # tail_view leaves the feed without tails until they are marked set
    assert not np.any(fed["no_tails"])
    cut = ends["truncated"] == 1
    rows = ends["end_rows"][cut]
    tails = fed["tails"]
    ref = V.predict(fed["params"].astype(np.float64), want[cut])
    err = rel_l2(tails[rows], ref)
    print(f"V(s_T): rel-L2 {err:.3e} over {int(cut.sum())} cut-off paths")
    assert err < 1e-4
    other = np.ones(n, bool)
    other[rows] = False
    assert np.all(tails[other] == 0.0) and np.all(tails[rows] != 0.0)
    # any other feed has no path ends
    g = _engine()
    out = fed["engine"].rollout_fetch()
    g.set_batch(out["obs32"], out["actions"], None, out["action_dists"])
    with pytest.raises(EngineError, match=r"rc=-4.*rollout_to_batch"):
        g.tail_view()
    T.device_rollout(g)
    g.rollout_to_batch()
    g.tail_view()
    g.set_rewards(out["rewards"], out["starts"])
    with pytest.raises(EngineError, match="rollout_to_batch"):
        g.tail_view()
    g.rollout_to_batch()
    g.tail_view()
    T.device_rollout(g)                                  # a new rollout overwrites the end records
    with pytest.raises(EngineError, match="rollout_to_batch"):
        g.tail_view()
    with pytest.raises(EngineError, match="no tail_view"):
        g.set_tail_values_in_place()
    g.close()


def test_scan_uses_the_tails(fed):
    e, n, ends, tails = fed["engine"], fed["n"], fed["ends"], fed["tails"]
    out = T.oracle()[0]
    base = np.random.RandomState(2).uniform(0, 10, n)
    e.set_advantage_estimator("gae", LAM)
    e.set_baseline(base)
    assert np.array_equal(e.tail_values(), tails)
    ret, adv = e.compute_advantages(GAMMA)
    A_ref, R_ref, _ = gae_ref(out["rewards"], base, GAMMA, LAM, out["starts"], tails)
    print(f"returns: max rel error {np.max(np.abs(ret - R_ref) / np.abs(R_ref)):.3e}")
    np.testing.assert_allclose(ret, R_ref, rtol=1e-13)
    np.testing.assert_allclose(adv, O.standardize(A_ref), rtol=1e-11, atol=1e-12)
    e.set_tail_values(None)
    ret0, adv0 = e.compute_advantages(GAMMA)
    A_ref0, R_ref0, _ = gae_ref(out["rewards"], base, GAMMA, LAM, out["starts"])
    np.testing.assert_allclose(ret0, R_ref0, rtol=1e-13)
    np.testing.assert_allclose(adv0, O.standardize(A_ref0), rtol=1e-11, atol=1e-12)
    # the returns move on exactly the rows of the cut-off paths
    in_cut = np.zeros(n, bool)
    for p in np.flatnonzero(ends["truncated"]):
        in_cut[ends["end_rows"][p] - ends["lengths"][p] + 1:ends["end_rows"][p] + 1] = True
    assert np.array_equal(ret != ret0, in_cut) and in_cut.any() and not in_cut.all()
    e.set_tail_values(tails)                             # leave the fixture as it was
    e.set_advantage_estimator("returns")


# ---------------------------------------------------------------------------- learn()
def _learn_draws(seed, n_iter, n_envs=4, budget=100, ep_max=20):
    rng = np.random.RandomState(seed)
    ru = [rng.random_sample((n_envs, budget, 4)) for _ in range(n_iter)]
    au = [rng.random_sample((n_envs, budget + ep_max - 1)) for _ in range(n_iter)]
    return lambda i: (ru[i], au[i], budget)


def _learn_config(**extra):
    from trpo_amd.agent import CONFIG
    return {**CONFIG, "max_steps": 20, "episodes_per_roll": 400, "gae_lambda": LAM, **extra}


def test_learn_bootstraps_truncated_paths(gpu_available):
    from trpo_amd import TRPOAgent
    agent = TRPOAgent(4, 2, hidden=(64,), max_rows=4096, config=_learn_config(bootstrap_truncated=True))
    hist = agent.learn(max_iterations=3, n_envs=4, record=True, log=None, draws=_learn_draws(21, 3))
    assert len(hist) == 3
    assert not np.any(hist[0]["tail_values"]) and not np.any(hist[0]["baseline"])
    for i, h in enumerate(hist):
        ends, tails, roll = h["ends"], h["tail_values"], h["rollout"]
        n = h["steps"]
        assert tails.shape == (n,) and len(ends["truncated"]) == h["paths"]
        starts = np.flatnonzero(roll["starts"])
        assert np.array_equal(ends["end_rows"], np.r_[starts[1:], n] - 1)
        assert np.all(ends["lengths"][ends["truncated"] == 1] == 20)
        if i >= 1:
            rows = ends["end_rows"][ends["truncated"] == 1]
            assert len(rows) >= 1
            want = np.zeros(n, bool)
            want[rows] = True
            assert np.array_equal(tails != 0.0, want), i
        A_ref, R_ref, _ = gae_ref(roll["rewards"], h["baseline"], GAMMA, LAM, roll["starts"], tails)
        print(f"iteration {i}: returns max rel error {np.max(np.abs(h['returns'] - R_ref) / np.abs(R_ref)):.3e}, "
              f"min |R_ref| {np.min(np.abs(R_ref)):.3e}, tails in [{tails.min():.3f}, {tails.max():.3f}]")
        np.testing.assert_allclose(h["returns"], R_ref, rtol=1e-13, err_msg=str(i))
        np.testing.assert_allclose(h["advantages"], O.standardize(A_ref), rtol=1e-11, atol=1e-12, err_msg=str(i))


def test_bootstrap_needs_gae(gpu_available):
    from trpo_amd import TRPOAgent
    from trpo_amd.agent import CONFIG
    with pytest.raises(ValueError, match="gae_lambda"):
        TRPOAgent(4, 2, hidden=(64,), max_rows=256, config={**CONFIG, "bootstrap_truncated": True})


def test_bootstrap_off_changes_nothing(gpu_available):
    from trpo_amd import TRPOAgent
    runs = []
    for extra in ({}, {"bootstrap_truncated": False}):
        agent = TRPOAgent(4, 2, hidden=(64,), max_rows=4096, config=_learn_config(**extra))
        runs.append(agent.learn(max_iterations=2, n_envs=4, record=True, log=None, draws=_learn_draws(21, 2)))
    for a, b in zip(*runs):
        assert np.array_equal(a["theta"], b["theta"]) and np.array_equal(a["advantages"], b["advantages"])
        assert np.array_equal(a["returns"], b["returns"]) and not np.any(a["tail_values"])
