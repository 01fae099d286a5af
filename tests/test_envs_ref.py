"""The environments' reference (tests/envs_ref.py) checks itself, and the engine's host-only environment table
(trpo_env_info) matches it.  CPU only: no GPU is touched."""
import ctypes
import math

import numpy as np
import pytest

import envs_ref as R

PI = R.PI


# ---------------------------------------------------------------------------- the reference itself
def test_mountaincar_left_wall_zeroes_velocity():
    s, r, done = R.MountainCarV0.step([-1.19, -0.06], 0)
    assert s == [-1.2, 0.0] and r == -1.0 and not done
    # moving right at the wall keeps its velocity
    s, _, _ = R.MountainCarV0.step([-1.2, 0.0], 2)
    assert s[1] > 0 and s[0] > -1.2


def test_mountaincar_goal_needs_position():
    s, r, done = R.MountainCarV0.step([0.45, 0.06], 2)
    assert s[0] >= 0.5 and s[1] > 0 and done and r == -1.0           # the terminating step costs -1 too
    s, r, done = R.MountainCarV0.step([0.40, 0.07], 2)
    assert s[0] < 0.5 and s[1] > 0 and not done and r == -1.0
    # velocity and position are clamped
    s, _, _ = R.MountainCarV0.step([-PI / 6, 0.07], 2)                # cos(3p) ~ 0: the push alone, +0.001
    assert s[1] == 0.07
    s, _, done = R.MountainCarV0.step([0.59, 0.07], 2)
    assert s[0] == 0.6 and done


def test_mountaincar_reset_range():
    assert R.MountainCarV0.reset([0.0]) == [-0.6, 0.0]
    lo, hi = R.MountainCarV0.reset([0.0])[0], R.MountainCarV0.reset([1.0 - 2.0 ** -53])[0]
    assert lo == -0.6 and -0.4 - 1e-15 < hi <= -0.4 + 1e-15


def test_acrobot_upright_is_terminal():
    """t1 = pi, t2 = 0 at rest is the upright equilibrium: the step stays there, which is above the line."""
    s, r, done = R.AcrobotV1.step([PI, 0.0, 0.0, 0.0], 1)
    assert done and r == 0.0
    assert abs(abs(s[0]) - PI) < 1e-9 and abs(s[1]) < 1e-9
    # hanging down at rest is not
    s, r, done = R.AcrobotV1.step([0.0, 0.0, 0.0, 0.0], 1)
    assert not done and r == -1.0 and max(abs(x) for x in s) < 1e-15   # cos(-pi/2) is 6e-17 in float64


def test_acrobot_wrap_and_clamp_ranges():
    rng = np.random.RandomState(3)
    n = 400
    st = np.c_[rng.uniform(-PI, PI, (n, 2)), rng.uniform(-4 * PI, 4 * PI, n), rng.uniform(-9 * PI, 9 * PI, n)]
    act = rng.randint(0, 3, n)
    so, ob, rw, dn, wr = R.step_rows(R.AcrobotV1, st, act)
    assert np.all(np.abs(so[:, :2]) <= PI)
    assert np.all(np.abs(so[:, 2]) <= 4 * PI) and np.all(np.abs(so[:, 3]) <= 9 * PI)
    assert np.any(wr != 0) and np.any(np.abs(so[:, 2]) == 4 * PI) and np.any(np.abs(so[:, 3]) == 9 * PI)
    assert set(np.unique(rw)) <= {-1.0, 0.0} and np.array_equal(rw == 0.0, dn)
    # the observation is (cos t1, sin t1, cos t2, sin t2, w1, w2) of the new state
    i = 7
    assert ob[i].tolist() == [math.cos(so[i, 0]), math.sin(so[i, 0]), math.cos(so[i, 1]), math.sin(so[i, 1]),
                              so[i, 2], so[i, 3]]


def test_longdouble_evaluation_agrees():
    """The same code in extended precision: close to, and not identical with, the float64 evaluation."""
    rng = np.random.RandomState(4)
    st = np.c_[rng.uniform(-PI, PI, (50, 2)), rng.uniform(-2, 2, (50, 2))]
    act = rng.randint(0, 3, 50)
    a = R.step_rows(R.AcrobotV1, st, act)
    b = R.step_rows(R.AcrobotV1, st, act, np.longdouble, np.cos, np.sin)
    assert b[0].dtype == np.longdouble
    err = np.max(np.abs(a[0] - b[0]).astype(np.float64))
    assert err < 1e-12
    if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps:
        assert err > 0.0


# ---------------------------------------------------------------------------- the engine's table
@pytest.mark.parametrize("name", sorted(R.ENVS))
def test_env_info_matches_reference(name):
    from trpo_amd.engine import ENVS, env_info
    ref = R.ENVS[name]
    assert ENVS[name] == ref.env_id
    want = {"obs_dim": ref.obs_dim, "state_dim": ref.state_dim, "n_actions": ref.n_actions,
            "reset_draws": ref.reset_draws, "time_limit": ref.time_limit, "name": name}
    assert env_info(name) == want and env_info(ref.env_id) == want


def test_env_table_values():
    """The table of the issue, literally."""
    from trpo_amd.engine import env_info
    rows = {"CartPole-v0": (4, 4, 2, 4, 200), "MountainCar-v0": (2, 2, 3, 1, 200), "Acrobot-v1": (6, 4, 3, 4, 500)}
    for name, row in rows.items():
        i = env_info(name)
        assert (i["obs_dim"], i["state_dim"], i["n_actions"], i["reset_draws"], i["time_limit"]) == row


def test_default_rollout_params_take_the_env_time_limit():
    from trpo_amd import _lib
    base = _lib.RolloutParams()
    _lib.lib.trpo_default_rollout_params(ctypes.byref(base))
    for env_id, limit in ((0, 200), (1, 200), (2, 500)):
        p = _lib.RolloutParams()
        assert _lib.lib.trpo_default_rollout_params_env(env_id, ctypes.byref(p)) == 0
        assert p.time_limit == limit
        assert (p.n_envs, p.max_pathlength, p.n_timesteps, p.train, p.seed) == \
            (base.n_envs, base.max_pathlength, base.n_timesteps, base.train, base.seed)


def test_unknown_environment_is_rejected():
    from trpo_amd import _lib
    from trpo_amd.engine import env_info, env_step_device
    with pytest.raises(ValueError, match="unknown environment"):
        env_info("Pendulum-v0")
    with pytest.raises(_lib.EngineError, match=r"rc=-1.*unknown environment id 3"):
        env_info(3)
    with pytest.raises(_lib.EngineError, match=r"rc=-1.*unknown environment id -1"):
        env_info(-1)
    p = _lib.RolloutParams()
    assert _lib.lib.trpo_default_rollout_params_env(9, ctypes.byref(p)) == -1
    # the id is checked before anything touches a device
    with pytest.raises(_lib.EngineError, match=r"rc=-1.*unknown environment id 7"):
        _lib.check(_lib.lib.trpo_env_step(7, None, None, 0, None, None, None, None, 0), "trpo_env_step")
    with pytest.raises(ValueError, match="unknown environment"):
        env_step_device("Pendulum-v0", np.zeros((1, 3)), [0])


def test_agent_must_fit_its_environment():
    """A config that names an environment of another shape is refused before any engine is created."""
    from trpo_amd import TRPOAgent
    from trpo_amd.agent import CONFIG
    with pytest.raises(ValueError, match=r"Acrobot-v1 has obs_dim 6 and 3 actions.*obs_dim 4 and 2 actions"):
        TRPOAgent(4, 2, hidden=(16,), max_rows=256, config={**CONFIG, "env": "Acrobot-v1"})
    with pytest.raises(ValueError, match="unknown environment"):
        TRPOAgent(4, 2, hidden=(16,), max_rows=256, config={**CONFIG, "env": "Pendulum-v0"})
