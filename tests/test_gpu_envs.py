"""MountainCar-v0 and Acrobot-v1 on the device (rollout.hip's environment traits through the C-ABI) against the
plain Python definition tests/envs_ref.py, and learn() on both.

The step bar.  Device and host sin / cos each differ from the true value by about an ulp, and both perturbations
pass through the same conditioning of the step.  test_step_parity measures that conditioning on its own inputs:
the float64 reference against the same code in np.longdouble, per component as |a - b| / max(1, |b|).  The bar is
8 x the largest such error (two such perturbations plus the noise of a maximum over 5000 samples), never below the
project's CartPole atol of 1e-15; a wrong term in the dynamics shows at 1e-6 or more.  A row is left out only where
the two references disagree on done or on a wrap branch, and at most 5 of 5000 may be.  The rollout tests reuse
that bar.  Other bars: done, rewards, actions, flags, lengths and reset states exact; float32 action distributions
to 1e-6 (tests/test_gpu_rollout.py); returns rtol 1e-13 and standardised advantages rtol 1e-11 / atol 1e-12
(tests/test_gpu_gae.py).

Measured on one MI355X (x86-64 host, 80-bit long double), as the tests print them; DESIGN.md §4 holds the same:
  step parity   Acrobot-v1: float64 vs longdouble 2.895e-13, bar 2.316e-12, device vs float64 1.510e-14 (state and
                obs), 0 of 5000 rows left out, done on 810 rows.  MountainCar-v0: 1.108e-16, bar 1.000e-15, device
                2.776e-17, 0 rows left out, done on 188 rows.
  replay        Acrobot-v1: 16000 steps, 32 paths, all cut off; obs 1.1e-16, step 3.3e-16, final obs 1.1e-16, dists
                1.2e-7.  MountainCar-v0: 6400 steps, 32 paths, all cut off; obs 0, step 3.5e-18, dists 1.2e-7.
  terminated    MountainCar-v0 17 paths of 86..177 steps, Acrobot-v1 20 paths of 66..194 steps.
  learn()       Acrobot-v1: iteration 0's step reverted by the kl > 2 max_kl rule (kl 0.124), iteration 1's accepted;
                returns within 8.9e-16 relative of gae_ref.  MountainCar-v0: both accepted, 16 paths each, all cut off.
"""
import numpy as np
import pytest

import envs_ref as R
from gae_ref import gae_ref
from oracle import cartpole_oracle as C
from oracle import trpo_oracle as O

pytestmark = pytest.mark.gpu

PI = R.PI
NEW_ENVS = ("MountainCar-v0", "Acrobot-v1")
N_ROWS = 5000
ATOL_FLOOR = 1e-15          # tests/test_gpu_rollout.py: the CartPole step's atol
GAMMA, LAM = 0.95, 0.95


def scaled_err(a, b):
    """max over components of |a - b| / max(1, |b|), as float64"""
    a, b = np.asarray(a), np.asarray(b)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b) / np.maximum(1, np.abs(b))))


def parity_inputs(name):
    rng = np.random.RandomState(0)
    if name == "MountainCar-v0":
        st = np.c_[rng.uniform(-1.2, 0.6, N_ROWS), rng.uniform(-0.07, 0.07, N_ROWS)]
    else:
        st = np.c_[rng.uniform(-PI, PI, (N_ROWS, 2)), rng.uniform(-4 * PI, 4 * PI, N_ROWS),
                   rng.uniform(-9 * PI, 9 * PI, N_ROWS)]
    return st, rng.randint(0, 3, N_ROWS)


_REFS = {}


def references(name):
    """The float64 and longdouble references on the parity inputs, the rows both agree on, and the step bar;
    computed once per environment and left unchanged."""
    if name not in _REFS:
        env = R.ENVS[name]
        st, act = parity_inputs(name)
        r64 = R.step_rows(env, st, act)
        rld = R.step_rows(env, st, act, np.longdouble, np.cos, np.sin)
        keep = (r64[3] == rld[3]) & np.all(r64[4] == rld[4], axis=1)
        cond = max(scaled_err(r64[0][keep], rld[0][keep]), scaled_err(r64[1][keep], rld[1][keep]))
        _REFS[name] = {"st": st, "act": act, "r64": r64, "keep": keep, "cond": cond,
                       "bar": max(8 * cond, ATOL_FLOOR)}
    return _REFS[name]


# ---------------------------------------------------------------------------- 1. step parity
@pytest.mark.parametrize("name", NEW_ENVS)
def test_step_parity(gpu_available, name):
    from trpo_amd.engine import env_step_device
    ref = references(name)
    keep, (s_ref, o_ref, r_ref, d_ref, _) = ref["keep"], ref["r64"]
    left_out = int((~keep).sum())
    so, ob, rw, dn = env_step_device(name, ref["st"], ref["act"])
    e_s, e_o = scaled_err(so[keep], s_ref[keep]), scaled_err(ob[keep], o_ref[keep])
    print(f"{name}: float64 vs longdouble {ref['cond']:.3e}, bar {ref['bar']:.3e}, {left_out} of {N_ROWS} rows left "
          f"out; device vs float64: state {e_s:.3e}, obs {e_o:.3e}; done on {int(d_ref.sum())} rows")
    assert left_out <= 5
    assert so.shape == s_ref.shape and ob.shape == o_ref.shape
    assert np.array_equal(dn[keep], d_ref[keep]) and np.array_equal(rw[keep], r_ref[keep])
    assert e_s <= ref["bar"] and e_o <= ref["bar"]
    if name == "Acrobot-v1":   # the inputs reach the clamps, the wraps and both rewards
        assert np.any(np.abs(s_ref[:, 2]) == 4 * PI) and np.any(np.abs(s_ref[:, 3]) == 9 * PI)
        assert np.any(ref["r64"][4] != 0) and 0 < d_ref.sum() < N_ROWS


# ---------------------------------------------------------------------------- 2. rollout replay
N_ENVS, N_TIMESTEPS, SEED = 32, 4000, 7
BUDGET = -(-N_TIMESTEPS // N_ENVS)


def small_engine(name, theta=None, max_rows=None):
    from trpo_amd import Engine, xavier_theta
    env = R.ENVS[name]
    rows = N_ENVS * (BUDGET + env.time_limit - 1) if max_rows is None else max_rows
    e = Engine(env.obs_dim, [16], 3, max_rows=rows)
    th = xavier_theta(env.obs_dim, [16], 3, np.random.RandomState(11)) if theta is None else theta
    e.set_flat(th)
    return e, th


def fetch_all(e):
    out = e.rollout_fetch()
    out["env_states"] = e.rollout_fetch_states()
    out.update({"end_" + k: v for k, v in e.rollout_fetch_ends().items()})
    return out


@pytest.mark.parametrize("name", NEW_ENVS)
def test_rollout_replays_and_is_deterministic(gpu_available, name):
    env = R.ENVS[name]
    bar = references(name)["bar"]
    e, theta = small_engine(name)
    ru = np.random.RandomState(5).random_sample((N_ENVS, BUDGET, env.reset_draws))
    kw = dict(n_envs=N_ENVS, n_timesteps=N_TIMESTEPS, seed=SEED, reset_uniforms=ru, max_episodes_per_env=BUDGET)
    r1 = e.rollout(name, **kw)
    out = fetch_all(e)
    r2 = e.rollout(name, **kw)
    out2 = fetch_all(e)
    e.close()
    assert r1 == r2
    for k in out:
        assert np.array_equal(out[k], out2[k]), k
    n, paths = r1
    limit = env.time_limit
    obs, st, act, rew = out["obs"], out["env_states"], out["actions"], out["rewards"]
    assert obs.shape == (n, env.obs_dim) and st.shape == (n, env.state_dim)
    assert n >= N_TIMESTEPS and n <= N_ENVS * (BUDGET + limit - 1)
    # the policy side
    assert np.array_equal(act, C.cat_sample(out["action_dists"], out["uniforms"]))
    assert np.array_equal(out["obs32"], obs.astype(np.float32))
    ref_dist = C.policy_dist32(theta, obs.astype(np.float32), [env.obs_dim, 16, 3])
    e_dist = float(np.max(np.abs(out["action_dists"] - ref_dist)))
    assert e_dist < 1e-6
    assert set(np.unique(act)) == {0, 1, 2}
    # the observation is the observation of the recorded state
    e_obs = scaled_err(obs, np.array([env.observe(s) for s in st]))
    assert e_obs <= bar
    # paths: env-major, each environment's episodes in order
    starts = np.flatnonzero(out["starts"])
    lengths, end_rows, trunc = out["end_lengths"], out["end_end_rows"], out["end_truncated"]
    assert len(starts) == paths and np.array_equal(end_rows, np.r_[starts[1:], n] - 1)
    assert np.array_equal(lengths, end_rows - starts + 1) and lengths.max() <= limit
    p = 0
    for en in range(N_ENVS):
        cnt, ep = 0, 0
        while cnt < BUDGET:
            assert st[starts[p]].tolist() == env.reset(ru[en, ep]), (en, ep)     # exactly
            cnt += int(lengths[p])
            ep += 1
            p += 1
    assert p == paths
    # every transition on the host
    last = np.zeros(n, bool)
    last[end_rows] = True
    e_step = e_final = 0.0
    done_last = np.zeros(paths, bool)
    path_of = np.cumsum(out["starts"]) - 1
    for i in range(n):
        s1, r, d = env.step(st[i].tolist(), act[i])
        assert r == rew[i], i
        if not last[i]:
            assert not d, i
            e_step = max(e_step, scaled_err(st[i + 1], s1))
        else:
            k = path_of[i]
            done_last[k] = d
            assert d or lengths[k] == limit, i
            e_final = max(e_final, scaled_err(out["end_final_obs"][k], env.observe(s1)))
    print(f"{name}: {n} steps, {paths} paths, {int(trunc.sum())} cut off; bar {bar:.3e}; obs {e_obs:.3e}, step "
          f"{e_step:.3e}, final obs {e_final:.3e}, dists {e_dist:.3e}")
    assert e_step <= bar and e_final <= bar
    assert np.array_equal(trunc.astype(bool), (lengths == limit) & ~done_last)
    assert np.all(out["end_final_dists"][trunc == 0] == 0.0)


# ---------------------------------------------------------------------------- 3. terminated paths exist
def pushing_theta(obs_dim, which, gain):
    """One hidden layer of 8: h_0 = tanh(gain * obs[which]), logits (-10 h_0, 0, +10 h_0): under argmax the torque
    or push follows the sign of obs[which]."""
    W1, b1 = np.zeros((obs_dim, 8)), np.zeros(8)
    W2, b2 = np.zeros((8, 3)), np.zeros(3)
    W1[which, 0] = gain
    W2[0] = (-10.0, 0.0, 10.0)
    return np.concatenate([W1.ravel(), b1, W2.ravel(), b2]).astype(np.float32)


@pytest.mark.parametrize("name,which,gain", [("MountainCar-v0", 1, 1000.0), ("Acrobot-v1", 5, 10.0)])
def test_terminated_paths_exist(gpu_available, name, which, gain):
    from trpo_amd import Engine
    env = R.ENVS[name]
    e = Engine(env.obs_dim, [8], 3, max_rows=4096)
    e.set_flat(pushing_theta(env.obs_dim, which, gain))
    n, paths = e.rollout(name, n_envs=8, n_timesteps=1600, seed=3, train=False)
    out, ends = e.rollout_fetch(), e.rollout_fetch_ends()
    e.close()
    print(f"{name}: {paths} paths of {ends['lengths'].min()}..{ends['lengths'].max()} steps")
    assert paths >= 8 and np.all(ends["truncated"] == 0) and np.all(ends["lengths"] < env.time_limit)
    assert np.all(ends["final_dists"] == 0.0)
    last = out["rewards"][ends["end_rows"]]
    assert np.all(last == (0.0 if name == "Acrobot-v1" else -1.0))
    inner = np.ones(n, bool)
    inner[ends["end_rows"]] = False
    assert np.all(out["rewards"][inner] == -1.0)


# ---------------------------------------------------------------------------- 4. shape errors
def test_shape_errors(gpu_available):
    from trpo_amd import Engine
    from trpo_amd._lib import EngineError
    e = Engine(4, [16], 2, max_rows=256)
    with pytest.raises(EngineError, match=r"rc=-4.*no rollout"):
        e.rollout_fetch_states()
    with pytest.raises(EngineError, match=r"rc=-1.*Acrobot-v1 needs obs_dim 6 and 3 actions.*obs_dim 4 and 2 actions"):
        e.rollout("Acrobot-v1", n_envs=2, n_timesteps=10)
    with pytest.raises(EngineError, match=r"rc=-1.*MountainCar-v0 needs obs_dim 2 and 3 actions"):
        e.rollout("MountainCar-v0", n_envs=2, n_timesteps=10)
    with pytest.raises(EngineError, match=r"rc=-4.*no rollout"):      # a refused rollout leaves none behind
        e.rollout_fetch_states()
    e.close()


# ---------------------------------------------------------------------------- 5. CartPole through the new door
def test_cartpole_through_the_new_door(gpu_available):
    from trpo_amd import Engine, xavier_theta
    e = Engine(4, [16], 2, max_rows=8192)
    e.set_flat(xavier_theta(4, [16], 2, np.random.RandomState(11)))
    kw = dict(n_envs=16, n_timesteps=2000, seed=9)
    r_old = e.rollout_cartpole(**kw)
    old = fetch_all(e)
    r_new = e.rollout("CartPole-v0", **kw)
    new = fetch_all(e)
    e.close()
    assert r_old == r_new
    for k in old:
        assert np.array_equal(old[k], new[k]), k
    assert np.array_equal(new["env_states"], new["obs"]) and r_new[1] > 16
    # and one step through the generic entry is trpo_cartpole_step's
    from trpo_amd.engine import cartpole_step_device, env_step_device
    s_old, r_old1, d_old = cartpole_step_device(new["obs"], new["actions"])
    s_new, o_new, r_new1, d_new = env_step_device("CartPole-v0", new["obs"], new["actions"])
    assert np.array_equal(s_old, s_new) and np.array_equal(s_new, o_new)
    assert np.array_equal(r_old1, r_new1) and np.array_equal(d_old, d_new) and d_new.sum() > 0


# ---------------------------------------------------------------------------- 6. the loop runs
def run_learn(name):
    from trpo_amd import TRPOAgent
    from trpo_amd.agent import CONFIG
    env = R.ENVS[name]
    n_envs, roll = 8, 2000
    worst = n_envs * (-(-roll // n_envs) + env.time_limit - 1)
    agent = TRPOAgent(env.obs_dim, 3, hidden=[16], max_rows=worst,
                      config={**CONFIG, "env": name, "gae_lambda": LAM, "bootstrap_truncated": True,
                              "episodes_per_roll": roll, "reward_target": 0.0})
    theta0 = agent.engine.get_flat().copy()
    hist = agent.learn(max_iterations=2, n_envs=n_envs, record=True, log=None)
    return agent, theta0, hist


@pytest.mark.parametrize("name", ["Acrobot-v1", "MountainCar-v0"])
def test_learn_runs(gpu_available, name):
    env = R.ENVS[name]
    agent, theta0, hist = run_learn(name)
    assert len(hist) == 2
    for i, h in enumerate(hist):
        roll, ends, tails, n = h["rollout"], h["ends"], h["tail_values"], h["steps"]
        assert roll["obs"].shape == (n, env.obs_dim) and roll["action_dists"].shape == (n, 3)
        assert set(np.unique(roll["rewards"])) <= {-1.0, 0.0}
        assert ends["lengths"].max() <= env.time_limit
        assert np.all(ends["lengths"][ends["truncated"] == 1] == env.time_limit)
        rows = ends["end_rows"][ends["truncated"] == 1]
        want = np.zeros(n, bool)
        if i >= 1:
            want[rows] = True
            assert len(rows) >= 1
        assert np.array_equal(tails != 0.0, want), i
        if name == "MountainCar-v0":     # an untrained policy never reaches the flag
            assert np.all(ends["truncated"] == 1) and np.all(roll["rewards"] == -1.0)
        A_ref, R_ref, _ = gae_ref(roll["rewards"], h["baseline"], GAMMA, LAM, roll["starts"], tails)
        nz = R_ref != 0.0
        print(f"{name} iteration {i}: {n} steps, {h['paths']} paths, {len(rows)} cut off, reward mean "
              f"{h['reward_mean']:.1f}, entropy {h['entropy']:.4f}, returns max rel error "
              f"{np.max(np.abs(h['returns'][nz] - R_ref[nz]) / np.abs(R_ref[nz])):.3e}")
        np.testing.assert_allclose(h["returns"], R_ref, rtol=1e-13, err_msg=str(i))
        np.testing.assert_allclose(h["advantages"], O.standardize(A_ref), rtol=1e-11, atol=1e-12, err_msg=str(i))
        print(f"    update: k {h['k']}, reverted {h['reverted']}, kl {h['kl']:.3e}, surr {h['surr']:.3e}, moved "
              f"{not np.array_equal(h['theta'], h['theta_before'])}")
        assert h["train"] and np.isfinite(h["entropy"])
    # theta changed: against the parameters the first update started from (the VF's creation re-draws the policy
    # before it, as the reference's initialize_all_variables does, so the constructor's theta would show nothing)
    assert np.array_equal(agent.engine.get_flat(), hist[-1]["theta"])
    assert not np.array_equal(hist[-1]["theta"], hist[0]["theta_before"])
    agent.engine.close()
