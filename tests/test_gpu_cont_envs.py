"""Pendulum-v1 and MountainCarContinuous-v0 on the device under the diagonal-Gaussian policy (rollout.hip's
continuous-action traits and Gaussian rollout through the C-ABI) against the plain Python definition
tests/cont_envs_ref.py, the device-side feed built from the rollout, and learn() on both.

The step bar, as in tests/test_gpu_envs.py: the float64 reference against the same code in np.longdouble on the
test's own inputs, per component as |a - b| / max(1, |b|) over state, obs and reward; the bar is 8 x the largest such
error, never below 1e-15.  A row is left out only where the two references take different branches (done, Pendulum's
m < 0 adjustment or its floor(y / 2 pi)), and at most 5 of 5000 may be.  The generator's bar is made the same way from
the Box-Muller expression on the same uniforms.  Other bars: done, flags, lengths, reset states and the sampling
arithmetic exact; float32 means to 1e-6 of a float32 host forward; returns rtol 1e-13 and standardised advantages
rtol 1e-11 / atol 1e-12 (tests/test_gpu_gae.py); parameter vectors conftest.assert_vec_close at 1e-5
(tests/test_gpu_gauss.py).

Measured on one MI355X (x86-64 host, 80-bit long double), as the tests print them; DESIGN.md §4 holds the same:
  step parity   Pendulum-v1: float64 vs longdouble 2.568e-16 (state), 9.086e-16 (obs), 3.227e-16 (reward), bar
                7.269e-15; device vs float64 2.582e-16, 1.721e-15, 0; 0 of 5000 rows left out, no done, action
                clamped on 1675 rows, +-8 on 163, m < 0 on 1712.  MountainCarContinuous-v0: 1.106e-16, 1.106e-16,
                7.135e-17, bar 1.000e-15; device 5.551e-17, 5.551e-17, 0; 0 rows left out, done on 277 rows, action
                clamped on 1661.
  replay        Pendulum-v1: 6400 steps, 32 paths, all cut off; obs 1.1e-16, step 2.2e-16, reward 0, final obs 0, means
                3.6e-7, final means 1.2e-7.  MountainCarContinuous-v0: 31968 steps, 32 paths, all cut off; obs 0, step
                5.6e-17, reward 0, final obs 8.7e-19, means 1.8e-7, final means 6.0e-8.
  generator     4800 normals; float64 vs longdouble 1.409e-15, bar 1.127e-14, device vs float64 2.330e-16; mean -0.0139
                (bar 0.0722), var - 1 0.0285 (bar 0.1021).
  terminated    MountainCarContinuous-v0 24 paths of 76..111 steps; Pendulum-v1 8 paths of 200, all cut off.
  learn()       Pendulum-v1: 16 paths a rollout, all cut off; iteration 0 kl 0.247, reverted by the kl > 2 max_kl rule
                in the engine and the float64 reference alike (theta equal); iteration 1 kl 7.96e-3, accepted, theta
                5.6e-5 from the float64 reference where the float32 reference is 1.2e-3 from it (printed only).
                MountainCarContinuous-v0: 4 paths of 999, all cut off; kl 1.36e-2 and 1.03e-2, both accepted; theta
                within 8.3e-8 and 7.7e-8 of the float64 reference (the float32 reference 4.2e-7, 3.5e-7).  Returns
                within 9.5e-16 relative of gae_ref.
"""
import math

import numpy as np
import pytest

import cont_envs_ref as R
import gauss_ref as G
from conftest import assert_vec_close
from gae_ref import gae_ref
from oracle import trpo_oracle as O

pytestmark = pytest.mark.gpu

PI = R.PI
NAMES = ("Pendulum-v1", "MountainCarContinuous-v0")
N_ROWS = 5000
ATOL_FLOOR = 1e-15
GAMMA, LAM = 0.95, 0.95


def scaled_err(a, b):
    """max over components of |a - b| / max(1, |b|), as float64"""
    a, b = np.asarray(a), np.asarray(b)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b) / np.maximum(1, np.abs(b))))


def parity_inputs():
    """one RandomState(0): Pendulum's th, thd, a, then MountainCarContinuous's p, v, a"""
    rng = np.random.RandomState(0)
    out = {}
    st = np.c_[rng.uniform(-3 * PI, 3 * PI, N_ROWS), rng.uniform(-8, 8, N_ROWS)]
    out["Pendulum-v1"] = (st, rng.uniform(-3, 3, N_ROWS).astype(np.float32).reshape(-1, 1))
    st = np.c_[rng.uniform(-1.2, 0.6, N_ROWS), rng.uniform(-0.07, 0.07, N_ROWS)]
    out["MountainCarContinuous-v0"] = (st, rng.uniform(-1.5, 1.5, N_ROWS).astype(np.float32).reshape(-1, 1))
    return out


_REFS = {}


def references(name):
    """The float64 and longdouble references on the parity inputs, the rows both agree on, and the step bar;
    computed once per environment and left unchanged."""
    if name not in _REFS:
        env = R.ENVS[name]
        st, act = parity_inputs()[name]
        r64 = R.step_rows(env, st, act)
        rld = R.step_rows(env, st, act, np.longdouble, np.cos, np.sin, np.fmod)
        keep = (r64[3] == rld[3]) & np.all(r64[4] == rld[4], axis=1)
        errs = tuple(scaled_err(r64[k][keep], rld[k][keep]) for k in range(3))
        _REFS[name] = {"st": st, "act": act, "r64": r64, "keep": keep, "errs": errs,
                       "bar": max(8 * max(errs), ATOL_FLOOR)}
    return _REFS[name]


def mean32(theta, X32, widths):
    """the policy's mean by a float32 host forward: tanh hidden layers, a linear last one"""
    h, off = np.asarray(X32, np.float32), 0
    for i in range(len(widths) - 1):
        a, b = widths[i], widths[i + 1]
        W = theta[off:off + a * b].reshape(a, b)
        off += a * b
        z = h @ W + theta[off:off + b]
        off += b
        h = z if i + 2 == len(widths) else np.tanh(z)
    return h.astype(np.float32)


def gaussian_engine(name, hidden=(16,), logstd=-0.5, max_rows=4096, seed=11):
    from trpo_amd import Engine, xavier_theta
    env = R.ENVS[name]
    e = Engine(env.obs_dim, list(hidden), env.act_dim, max_rows=max_rows, dist="gaussian")
    th = np.concatenate([xavier_theta(env.obs_dim, list(hidden), env.act_dim, np.random.RandomState(seed)),
                         np.full(env.act_dim, logstd, np.float32)])
    e.set_flat(th)
    return e, th


def fetch_all(e):
    out = e.rollout_gaussian_fetch()
    out.update({"end_" + k: v for k, v in e.rollout_gaussian_fetch_ends().items()})
    return out


# ---------------------------------------------------------------------------- 1. step parity
@pytest.mark.parametrize("name", NAMES)
def test_step_parity(gpu_available, name):
    from trpo_amd.engine import cont_env_step_device
    ref = references(name)
    keep, (s_ref, o_ref, r_ref, d_ref, br) = ref["keep"], ref["r64"]
    act = ref["act"]
    left_out = int((~keep).sum())
    so, ob, rw, dn = cont_env_step_device(name, ref["st"], act)
    e_s, e_o, e_r = (scaled_err(so[keep], s_ref[keep]), scaled_err(ob[keep], o_ref[keep]),
                     scaled_err(rw[keep], r_ref[keep]))
    lim = 2.0 if name == "Pendulum-v1" else 1.0
    print(f"{name}: float64 vs longdouble state {ref['errs'][0]:.3e} obs {ref['errs'][1]:.3e} reward "
          f"{ref['errs'][2]:.3e}, bar {ref['bar']:.3e}, {left_out} of {N_ROWS} rows left out; device vs float64: state "
          f"{e_s:.3e}, obs {e_o:.3e}, reward {e_r:.3e}; done on {int(d_ref.sum())} rows, action clamped on "
          f"{int((np.abs(act) > lim).sum())}")
    assert left_out <= 5
    assert so.shape == s_ref.shape and ob.shape == o_ref.shape
    assert np.array_equal(dn[keep], d_ref[keep])
    assert e_s <= ref["bar"] and e_o <= ref["bar"] and e_r <= ref["bar"]
    # the inputs reach the action clamp, the velocity clamp, both fmod branches and both done values
    assert np.any(act > lim) and np.any(act < -lim) and np.any(np.abs(act) < lim)
    if name == "Pendulum-v1":
        assert np.any(s_ref[:, 1] == 8.0) and np.any(s_ref[:, 1] == -8.0) and not d_ref.any()
        assert 0 < br[:, 0].sum() < N_ROWS
        print(f"    +-8 clamp on {int((np.abs(s_ref[:, 1]) == 8.0).sum())} rows, m < 0 on {int(br[:, 0].sum())}")
    else:
        assert np.any(s_ref[:, 1] == 0.07) and np.any(s_ref[:, 1] == -0.07) and 0 < d_ref.sum() < N_ROWS


# ---------------------------------------------------------------------------- 2. rollout replay
N_ENVS, N_TIMESTEPS, SEED = 32, 4000, 7
BUDGET = -(-N_TIMESTEPS // N_ENVS)


def walk_paths(env, out, ru, n_envs, budget):
    """The environment of every path (paths are environment-major, each environment's episodes in order until
    its steps reach the budget); checks the reset states exactly where `ru` holds the injected draws."""
    st, starts, lengths = out["env_states"], np.flatnonzero(out["starts"]), out["end_lengths"]
    env_of, p = [], 0
    for en in range(n_envs):
        cnt, ep = 0, 0
        while cnt < budget:
            if ru is not None:
                assert st[starts[p]].tolist() == env.reset(ru[en, ep]), (en, ep)     # exactly
            env_of.append(en)
            cnt += int(lengths[p])
            ep += 1
            p += 1
    assert p == len(lengths)
    return np.array(env_of)


@pytest.mark.parametrize("name", NAMES)
def test_rollout_replays_and_is_deterministic(gpu_available, name):
    env = R.ENVS[name]
    bar = references(name)["bar"]
    limit = env.time_limit
    e, theta = gaussian_engine(name, max_rows=N_ENVS * (BUDGET + limit - 1))
    ru = np.random.RandomState(5).random_sample((N_ENVS, BUDGET, env.reset_draws))
    kw = dict(n_envs=N_ENVS, n_timesteps=N_TIMESTEPS, seed=SEED, reset_uniforms=ru, max_episodes_per_env=BUDGET)
    r1 = e.rollout_gaussian(name, **kw)
    out = fetch_all(e)
    r2 = e.rollout_gaussian(name, **kw)
    out2 = fetch_all(e)
    e.close()
    assert r1 == r2
    for k in out:
        assert np.array_equal(out[k], out2[k]), k
    n, paths = r1
    obs, st, act, rew = out["obs"], out["env_states"], out["actions"], out["rewards"]
    assert obs.shape == (n, env.obs_dim) and st.shape == (n, env.state_dim) and act.shape == (n, 1)
    assert act.dtype == np.float32 and out["means"].shape == (n, 1) and out["normals"].shape == (n, 1)
    assert n >= N_TIMESTEPS and n <= N_ENVS * (BUDGET + limit - 1)
    # the policy side
    widths = [env.obs_dim, 16, 1]
    assert np.array_equal(out["obs32"], obs.astype(np.float32))
    e_mean = float(np.max(np.abs(out["means"] - mean32(theta, out["obs32"], widths))))
    assert e_mean < 1e-6
    assert np.array_equal(out["logstd"], theta[-1:])
    want = (out["means"].astype(np.float64) + np.exp(out["logstd"].astype(np.float64)) * out["normals"])
    assert np.array_equal(act, want.astype(np.float32))
    assert np.all(out["normals"] != 0.0)
    # the observation is the observation of the recorded state
    e_obs = scaled_err(obs, np.array([env.observe(s) for s in st]))
    assert e_obs <= bar
    # paths: env-major, each environment's episodes in order, reset from the injected draws
    starts = np.flatnonzero(out["starts"])
    lengths, end_rows, trunc = out["end_lengths"], out["end_end_rows"], out["end_truncated"]
    assert len(starts) == paths and np.array_equal(end_rows, np.r_[starts[1:], n] - 1)
    assert np.array_equal(lengths, end_rows - starts + 1) and lengths.max() <= limit
    walk_paths(env, out, ru, N_ENVS, BUDGET)
    # every transition on the host, from the recorded state and the recorded action
    last = np.zeros(n, bool)
    last[end_rows] = True
    e_step = e_final = e_rew = 0.0
    done_last = np.zeros(paths, bool)
    path_of = np.cumsum(out["starts"]) - 1
    for i in range(n):
        s1, r, d = env.step(st[i].tolist(), act[i])
        e_rew = max(e_rew, scaled_err(rew[i], r))
        if not last[i]:
            assert not d, i
            e_step = max(e_step, scaled_err(st[i + 1], s1))
        else:
            k = path_of[i]
            done_last[k] = d
            assert d or lengths[k] == limit, i
            e_final = max(e_final, scaled_err(out["end_final_obs"][k], env.observe(s1)))
    fm = out["end_final_means"]
    cut = trunc == 1
    e_fm = 0.0
    if cut.any():
        e_fm = float(np.max(np.abs(fm[cut] - mean32(theta, out["end_final_obs"][cut].astype(np.float32), widths))))
    print(f"{name}: {n} steps, {paths} paths, {int(trunc.sum())} cut off; bar {bar:.3e}; obs {e_obs:.3e}, step "
          f"{e_step:.3e}, reward {e_rew:.3e}, final obs {e_final:.3e}, means {e_mean:.3e}, final means {e_fm:.3e}")
    assert e_step <= bar and e_final <= bar and e_rew <= bar
    assert np.array_equal(trunc.astype(bool), (lengths == limit) & ~done_last)
    assert np.all(fm[~cut] == 0.0) and e_fm < 1e-6


# ---------------------------------------------------------------------------- 3. the generator
def test_generator(gpu_available):
    name, n_envs, n_timesteps, seed = "Pendulum-v1", 8, 4000, 12345678901234567
    env = R.ENVS[name]
    budget = -(-n_timesteps // n_envs)
    e, theta = gaussian_engine(name, max_rows=n_envs * (budget + env.time_limit - 1))
    kw = dict(n_envs=n_envs, n_timesteps=n_timesteps, seed=seed)
    e.rollout_gaussian(name, **kw)
    out = fetch_all(e)
    e.rollout_gaussian(name, train=False, **kw)
    out0 = fetch_all(e)
    e.rollout_gaussian(name, **kw)
    out2 = fetch_all(e)
    e.close()
    # the normal of component 0 at an environment's step k, counted over all its episodes
    env_of_path = walk_paths(env, out, None, n_envs, budget)
    env_of_row = env_of_path[np.cumsum(out["starts"]) - 1]
    got = out["normals"][:, 0]
    n = len(got)
    assert n >= 4000
    u = np.empty((n, 2))
    k = 0
    for i in range(n):
        k = 0 if i == 0 or env_of_row[i] != env_of_row[i - 1] else k + 1
        u[i] = R.normal_uniforms(seed, int(env_of_row[i]), k, 0)
    assert np.all((u >= 0) & (u < 1))
    ref = np.array([R.box_muller(a, b) for a, b in u])
    ref_ld = np.array([R.box_muller(a, b, np.longdouble, np.sqrt, np.log, np.cos) for a, b in u])
    cond = scaled_err(ref, ref_ld)
    bar = max(8 * cond, ATOL_FLOOR)
    err = scaled_err(got, ref)
    mean, var = float(got.mean()), float(got.var())
    print(f"generator: {n} normals; float64 vs longdouble {cond:.3e}, bar {bar:.3e}, device vs float64 {err:.3e}; "
          f"mean {mean:.4f} (bar {5 / math.sqrt(n):.4f}), var - 1 {var - 1:.4f} (bar {5 * math.sqrt(2 / n):.4f})")
    assert err <= bar
    assert abs(mean) < 5 / math.sqrt(n) and abs(var - 1) < 5 * math.sqrt(2 / n)
    # reset draws: stream 1, index episode * reset_draws + i
    first = np.flatnonzero(out["starts"])[0]
    assert out["env_states"][first].tolist() == env.reset([R.uniform53(seed, 0, 1, 0), R.uniform53(seed, 0, 1, 1)])
    # train=False draws nothing and acts with the mean; the step count advances all the same, so ...
    assert np.all(out0["normals"] == 0.0) and np.array_equal(out0["actions"], out0["means"])
    assert float(np.max(np.abs(out0["means"] - mean32(theta, out0["obs32"], [3, 16, 1])))) < 1e-6
    # ... a following train=True run with the same seed reproduces the first run's normals (and everything else)
    for key in out:
        assert np.array_equal(out[key], out2[key]), key


# ---------------------------------------------------------------------------- 4. terminated paths exist
def test_terminated_paths_exist(gpu_available):
    from trpo_amd import Engine
    name = "MountainCarContinuous-v0"
    env = R.ENVS[name]
    # one hidden layer of 8: h_0 = tanh(1000 v), mean = h_0: the push follows the velocity's sign
    W1, W2 = np.zeros((2, 8)), np.zeros((8, 1))
    W1[1, 0], W2[0, 0] = 1000.0, 1.0
    theta = np.concatenate([W1.ravel(), np.zeros(8), W2.ravel(), np.zeros(1), [-5.0]]).astype(np.float32)
    e = Engine(2, [8], 1, max_rows=8 * (200 + 999 - 1), dist="gaussian")
    e.set_flat(theta)
    n, paths = e.rollout_gaussian(name, n_envs=8, n_timesteps=1600, seed=3, train=False)
    out, ends = e.rollout_gaussian_fetch(), e.rollout_gaussian_fetch_ends()
    e.close()
    lengths = ends["lengths"]
    print(f"{name}: {paths} paths of {lengths.min()}..{lengths.max()} steps")
    assert paths >= 8 and np.all(ends["truncated"] == 0) and np.all(lengths < env.time_limit)
    assert lengths.min() >= 50 and lengths.max() <= 200
    assert np.all(ends["final_means"] == 0.0)
    a = out["actions"][:, 0].astype(np.float64)
    last = np.zeros(n, bool)
    last[ends["end_rows"]] = True
    assert np.array_equal(out["rewards"][last], 100.0 - (a[last] * a[last]) * 0.1)
    assert np.array_equal(out["rewards"][~last], 0.0 - (a[~last] * a[~last]) * 0.1)
    assert np.all(ends["final_obs"][:, 0] >= 0.45) and np.all(ends["final_obs"][:, 1] >= 0.0)
    # Pendulum never terminates: every path of a random policy is cut off at exactly 200
    e, _ = gaussian_engine("Pendulum-v1", max_rows=8 * (200 + 200 - 1))
    n, paths = e.rollout_gaussian("Pendulum-v1", n_envs=8, n_timesteps=1600, seed=3)
    ends = e.rollout_gaussian_fetch_ends()
    e.close()
    assert paths == 8 and n == 1600
    assert np.all(ends["truncated"] == 1) and np.all(ends["lengths"] == 200)


# ---------------------------------------------------------------------------- 5. wrong-kind and shape errors
def test_wrong_kind_and_shape_errors(gpu_available):
    from trpo_amd import Engine
    from trpo_amd._lib import EngineError
    with Engine(3, [16], 1, max_rows=256) as c:
        assert c.dist == "categorical"
        for call in (lambda: c.rollout_gaussian("Pendulum-v1", n_envs=2, n_timesteps=10),
                     lambda: c.rollout_gaussian_fetch(),
                     lambda: c.rollout_gaussian_fetch_ends(),
                     lambda: c.rollout_gaussian_to_batch()):
            with pytest.raises(EngineError, match=r"rc=-4.*needs a gaussian engine.*distribution is categorical"):
                call()
    with Engine(3, [16], 1, max_rows=256, dist="gaussian") as g:
        for call in (g.rollout_gaussian_fetch, g.rollout_gaussian_fetch_ends, g.rollout_gaussian_to_batch):
            with pytest.raises(EngineError, match=r"rc=-4.*no rollout"):
                call()
    with Engine(4, [16], 2, max_rows=256, dist="gaussian") as g:
        with pytest.raises(EngineError, match=r"rc=-1.*Pendulum-v1 needs obs_dim 3 and act_dim 1.*obs_dim 4 and act_dim 2"):
            g.rollout_gaussian("Pendulum-v1", n_envs=2, n_timesteps=10)
        with pytest.raises(EngineError, match=r"rc=-1.*MountainCarContinuous-v0 needs obs_dim 2 and act_dim 1"):
            g.rollout_gaussian("MountainCarContinuous-v0", n_envs=2, n_timesteps=10)
        with pytest.raises(EngineError, match=r"rc=-1.*unknown continuous environment id 2\b"):
            g.rollout_gaussian(2, n_envs=2, n_timesteps=10)
        with pytest.raises(ValueError, match="unknown continuous environment"):
            g.rollout_gaussian("CartPole-v0")
        with pytest.raises(EngineError, match=r"rc=-4.*no rollout"):      # a refused rollout leaves none behind
            g.rollout_gaussian_fetch_ends()
        with pytest.raises(EngineError, match=r"rc=-4.*no rollout"):
            g.rollout_gaussian_to_batch()


# ---------------------------------------------------------------------------- 6. to_batch equals the host feed
def test_to_batch_equals_the_host_feed(gpu_available):
    from trpo_amd import Engine
    name, n_envs, n_timesteps = "Pendulum-v1", 8, 2000
    rows = n_envs * (-(-n_timesteps // n_envs) + 200 - 1)
    e, theta = gaussian_engine(name, max_rows=rows)
    n, paths = e.rollout_gaussian(name, n_envs=n_envs, n_timesteps=n_timesteps, seed=21)
    out = e.rollout_gaussian_fetch()
    # the policy moves after the rollout: the feed's old log-std is the rollout's snapshot, not theta's tail
    theta2 = (theta.astype(np.float64) * (1 + 0.02 * np.random.RandomState(2).standard_normal(theta.shape)))
    theta2 = theta2.astype(np.float32)
    assert theta2[-1] != theta[-1]
    e.set_flat(theta2)
    e.rollout_gaussian_to_batch()
    assert e.n == n
    _, adv_dev = e.compute_advantages(GAMMA)
    v = np.random.RandomState(3).standard_normal(e.num_params).astype(np.float32)
    got = (e.losses(), e.policy_grad(), e.fvp(v, 0.1))
    view = e.tail_view()
    assert (view.n, view.n_paths, view.obs_dim, view.n_actions) == (n, paths, 3, 1)
    e.close()
    with Engine(3, [16], 1, max_rows=rows, dist="gaussian") as h:
        h.set_flat(theta2)
        h.set_batch_gaussian(out["obs32"], out["actions"], None, out["means"], out["logstd"])
        h.set_rewards(out["rewards"], out["starts"])
        _, adv_host = h.compute_advantages(GAMMA)
        want = (h.losses(), h.policy_grad(), h.fvp(v, 0.1))
    assert np.array_equal(adv_dev, adv_host)
    for a, b, what in zip(got, want, ("losses", "policy_grad", "fvp")):
        assert np.array_equal(a, b), what
    print(f"to_batch: {n} rows, losses {got[0]}")
    assert np.all(np.isfinite(got[0])) and got[0][1] > 0 and np.any(got[1] != 0)


# ---------------------------------------------------------------------------- 7. the loop runs
def run_learn(name):
    from trpo_amd import TRPOAgent
    from trpo_amd.agent import CONFIG
    env = R.ENVS[name]
    n_envs, roll = (8 if name == "Pendulum-v1" else 4), 2000
    worst = n_envs * (-(-roll // n_envs) + env.time_limit - 1)
    config = {**CONFIG, "env": name, "gae_lambda": LAM, "bootstrap_truncated": True, "episodes_per_roll": roll}
    agent = TRPOAgent(env.obs_dim, env.act_dim, hidden=[16], max_rows=worst, config=config)
    assert agent.engine.dist == "gaussian" and agent.engine.get_flat()[-1] == 0.0      # init_logstd's default
    hist = agent.learn(max_iterations=2, n_envs=n_envs, record=True, log=None)
    return agent, config, worst, hist


def paths_of(h):
    """the recorded rollout of one iteration as Gaussian paths"""
    roll, tails = h["rollout"], h["tail_values"]
    starts = np.flatnonzero(roll["starts"])
    out = []
    for a, b in zip(starts, np.r_[starts[1:], h["steps"]]):
        out.append({"obs": roll["obs"][a:b], "actions": roll["actions"][a:b], "action_means": roll["means"][a:b],
                    "logstd": roll["logstd"], "rewards": roll["rewards"][a:b], "baseline": h["baseline"][a:b],
                    "tail_value": tails[b - 1]})
    return out


@pytest.mark.parametrize("name", NAMES)
def test_learn_runs(gpu_available, name):
    import torch
    from trpo_amd import TRPOAgent
    env = R.ENVS[name]
    agent, config, worst, hist = run_learn(name)
    spec = G.GaussSpec(env.obs_dim, [16], env.act_dim)
    assert len(hist) == 2
    for i, h in enumerate(hist):
        roll, ends, tails, n = h["rollout"], h["ends"], h["tail_values"], h["steps"]
        assert set(roll) == {"obs", "obs32", "actions", "means", "logstd", "rewards", "starts", "normals", "env_states"}
        assert set(ends) == {"truncated", "final_obs", "final_means", "lengths", "end_rows"}
        assert roll["obs"].shape == (n, env.obs_dim) and roll["actions"].shape == roll["means"].shape == (n, 1)
        assert roll["env_states"].shape == (n, env.state_dim) and ends["final_means"].shape == (h["paths"], 1)
        assert ends["lengths"].max() <= env.time_limit
        assert np.all(ends["lengths"][ends["truncated"] == 1] == env.time_limit)
        rows = ends["end_rows"][ends["truncated"] == 1]
        want = np.zeros(n, bool)
        if i >= 1:
            want[rows] = True
            assert len(rows) >= 1
        assert np.array_equal(tails != 0.0, want), i
        if name == "Pendulum-v1":
            assert np.all(ends["truncated"] == 1) and np.all(roll["rewards"] <= 0.0)
        A_ref, R_ref, _ = gae_ref(roll["rewards"], h["baseline"], GAMMA, LAM, roll["starts"], tails)
        nz = R_ref != 0.0
        print(f"{name} iteration {i}: {n} steps, {h['paths']} paths, {len(rows)} cut off, reward mean "
              f"{h['reward_mean']:.1f}, entropy {h['entropy']:.4f}, returns max rel error "
              f"{np.max(np.abs(h['returns'][nz] - R_ref[nz]) / np.abs(R_ref[nz])):.3e}")
        np.testing.assert_allclose(h["returns"], R_ref, rtol=1e-13, err_msg=str(i))
        np.testing.assert_allclose(h["advantages"], O.standardize(A_ref), rtol=1e-11, atol=1e-12, err_msg=str(i))
        # the update against the float64 reference on the recorded feed, from the parameters it started from
        b = G.GaussBatch(roll["obs32"], roll["actions"], h["advantages"].astype(np.float32), roll["means"],
                         roll["logstd"])
        r = G.update(h["theta_before"], b, spec, torch.float64, 10, 1e-10, config["max_kl"], config["cg_damping"])
        err = float(np.linalg.norm(h["theta"] - r.theta_new) / np.linalg.norm(r.theta_new))
        r32 = G.update(h["theta_before"], b, spec, torch.float32, 10, 1e-10, config["max_kl"], config["cg_damping"])
        err32 = float(np.linalg.norm(r32.theta_new - r.theta_new) / np.linalg.norm(r.theta_new))
        print(f"    update: k {h['k']} (ref {r.k}), reverted {h['reverted']} (ref {r.reverted}), kl {h['kl']:.3e}, surr "
              f"{h['surr']:.3e}, cg_iters {h['cg_iters']} (ref {r.cg_iters}, float32 ref {r32.cg_iters}), theta rel err "
              f"{err:.3e} (float32 ref {err32:.3e}), moved {not np.array_equal(h['theta'], h['theta_before'])}")
        if i == 0:
            assert_vec_close(h["theta"], r.theta_new, 1e-5, f"{name} theta after iteration 0")
        assert h["train"] and np.isfinite(h["entropy"])
    assert np.array_equal(agent.engine.get_flat(), hist[-1]["theta"])
    assert not np.array_equal(hist[-1]["theta"], hist[0]["theta_before"])
    agent.engine.close()
    # update() and update_stepwise() on the same Gaussian paths (iteration 1's, from the parameters it started from)
    h = hist[1]
    paths = paths_of(h)
    thetas = []
    for how in ("update", "update_stepwise"):
        ag = TRPOAgent(env.obs_dim, env.act_dim, hidden=[16], max_rows=worst, config=config,
                       theta=h["theta_before"], reinit_policy=False)
        st = getattr(ag, how)(paths)
        thetas.append(ag.engine.get_flat().copy())
        print(f"    {how}: kl {st['kl_after']:.3e}, reverted {bool(st['reverted'])}")
        ag.engine.close()
    assert_vec_close(thetas[0], thetas[1], 1e-5, f"{name} update vs update_stepwise")
