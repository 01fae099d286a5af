"""The rollout path both policy heads share (engine.cpp's rollout(), rollout.hip's one kernel and one compaction):
a refused call keeps the previous rollout, the per-environment regions regrow and shrink without leaving a trace,
and the feed built on the device after a regrow is the feed built from the fetched arrays.  Every comparison is
bitwise; the policies are [8] wide.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# kind, environment, (obs_dim, head width)
CARTPOLE = ("categorical", "CartPole-v0", (4, 2))
ACROBOT = ("categorical", "Acrobot-v1", (6, 3))
PENDULUM = ("gaussian", "Pendulum-v1", (3, 1))
GAMMA = 0.95


def make_engine(case, max_rows=512):
    from trpo_amd import Engine, xavier_theta
    kind, _, (obs_dim, A) = case
    theta = xavier_theta(obs_dim, [8], A, np.random.RandomState(5))
    if kind == "gaussian":
        theta = np.concatenate([theta, np.full(A, -0.5, np.float32)])
    e = Engine(obs_dim, [8], A, max_rows=max_rows, dist=kind)
    e.set_flat(theta)
    return e, theta


def roll(e, case, **kw):
    kind, name, _ = case
    return e.rollout_gaussian(name, **kw) if kind == "gaussian" else e.rollout(name, **kw)


def fetch_all(e, case):
    """every array the engine hands out of its last rollout"""
    if case[0] == "gaussian":
        out = e.rollout_gaussian_fetch()
        ends = e.rollout_gaussian_fetch_ends()
    else:
        out = e.rollout_fetch()
        out["env_states"] = e.rollout_fetch_states()
        ends = e.rollout_fetch_ends()
    out.update({"end_" + k: v for k, v in ends.items()})
    return out


def assert_same_bits(got, want, what):
    assert got.keys() == want.keys(), what
    for k in want:
        a, b = got[k], want[k]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
        assert a.tobytes() == b.tobytes(), (what, k)


@pytest.mark.parametrize("case", [CARTPOLE, PENDULUM], ids=lambda c: c[1])
def test_a_failed_call_keeps_the_previous_rollout(gpu_available, case):
    from trpo_amd._lib import EngineError
    from trpo_amd.engine import cont_env_info, env_info
    info = (cont_env_info if case[0] == "gaussian" else env_info)(case[1])
    e, _ = make_engine(case)
    with e:
        n, paths = roll(e, case, n_envs=2, n_timesteps=40, seed=3)
        assert n >= 40 and paths >= 2
        before = fetch_all(e, case)
        # the same sizes, so no buffer moves; one episode's uniforms where an environment may start 20
        with pytest.raises(EngineError, match="max_episodes_per_env must be >="):
            roll(e, case, n_envs=2, n_timesteps=40, seed=3, reset_uniforms=np.full((2, 1, info["reset_draws"]), 0.5),
                 max_episodes_per_env=1)
        assert_same_bits(fetch_all(e, case), before, case[1])


SIZES = ((1, 30), (5, 300), (2, 40))   # one wave with three idle beside it; a wave alone in a second workgroup


@pytest.mark.parametrize("case", [ACROBOT, PENDULUM], ids=lambda c: c[1])
def test_regrow_and_shrink(gpu_available, case):
    e, theta = make_engine(case)
    with e:
        for n_envs, n_timesteps in SIZES:
            kw = dict(n_envs=n_envs, n_timesteps=n_timesteps, time_limit=20, seed=7)
            n, paths = roll(e, case, **kw)
            got = fetch_all(e, case)
            fresh, _ = make_engine(case)
            with fresh:
                assert roll(fresh, case, **kw) == (n, paths)
                want = fetch_all(fresh, case)
            assert n >= n_timesteps and got["env_states"].shape[0] == n
            assert_same_bits(got, want, (case[1], n_envs, n_timesteps))


@pytest.mark.parametrize("case", [ACROBOT, PENDULUM], ids=lambda c: c[1])
def test_to_batch_after_a_regrow(gpu_available, case):
    e, theta = make_engine(case)
    with e:
        roll(e, case, n_envs=1, n_timesteps=30, time_limit=20, seed=7)
        n, _ = roll(e, case, n_envs=5, n_timesteps=300, time_limit=20, seed=7)
        out = fetch_all(e, case)
        if case[0] == "gaussian":
            e.rollout_gaussian_to_batch()
        else:
            e.rollout_to_batch()
        assert e.n == n
        e.compute_advantages(GAMMA)
        got = (e.losses(), e.policy_grad())
    host, _ = make_engine(case)
    with host:
        if case[0] == "gaussian":
            host.set_batch_gaussian(out["obs32"], out["actions"], None, out["means"], out["logstd"])
        else:
            host.set_batch(out["obs32"], out["actions"], None, out["action_dists"])
        host.set_rewards(out["rewards"], out["starts"])
        host.compute_advantages(GAMMA)
        want = (host.losses(), host.policy_grad())
    for a, b, what in zip(got, want, ("losses", "policy_grad")):
        assert a.tobytes() == b.tobytes(), (case[1], what)
    assert np.all(np.isfinite(got[0])) and np.any(got[1] != 0)
