"""The continuous-action environments' reference (tests/cont_envs_ref.py) against hand-computed steps, the engine's
host-only table against the reference's, the errors that must come before any device is touched, and the Philox
restatement against the published Philox4x32-10 test vectors.  CPU only."""
import math

import numpy as np
import pytest

import cont_envs_ref as C
from trpo_amd.engine import CONT_ENVS, cont_env_info, cont_env_step_device   # host-only until a step is asked for

P, M = C.PendulumV1, C.MountainCarContinuousV0


# ---------------------------------------------------------------------------- the reference, by hand
def test_pendulum_steps_by_hand():
    # at rest, hanging up, no torque: nothing moves and nothing is paid
    s, r, d = P.step([0.0, 0.0], [0.0])
    assert s == [0.0, 0.0] and r == 0.0 and d is False
    assert P.observe(s) == [1.0, 0.0, 0.0]
    # th 0, thd 1, torque 1: cost 0.1*1 + 0.001*1, thd' = 1 + 3*0.05, th' = 1.15*0.05
    s, r, _ = P.step([0.0, 1.0], [1.0])
    assert s[1] == pytest.approx(1.15, abs=1e-15) and s[0] == pytest.approx(0.0575, abs=1e-15)
    assert r == pytest.approx(-0.101, abs=1e-15)
    # the action clamp: 5 acts as 2 in the dynamics and in the cost
    s, r, _ = P.step([0.0, 0.0], [5.0])
    assert s[1] == pytest.approx(0.3, abs=1e-15) and r == pytest.approx(-0.004, abs=1e-15)
    # the velocity clamp: 7.9 + (15*1 + 6)*0.05 = 8.95 -> 8, th' = pi/2 + 0.4; cost (pi/2)^2 + 0.1*7.9^2 + 0.004
    s, r, _ = P.step([math.pi / 2, 7.9], [2.0])
    assert s == [math.pi / 2 + 8.0 * 0.05, 8.0]
    assert r == pytest.approx(-(math.pi ** 2 / 4 + 6.241 + 0.004), abs=1e-14)
    # the angle is normalised into [-pi, pi) for the cost: -4 is 2 pi - 4 from upright (the m < 0 branch) ...
    info = {}
    s, r, _ = P.step([-4.0, 0.0], [0.0], info=info)
    assert info == {"neg": True, "turns": -1}
    assert r == pytest.approx(-((2 * math.pi - 4) ** 2), abs=1e-14)
    assert s[1] == pytest.approx(15 * math.sin(-4.0) * 0.05, abs=1e-15)
    # ... and 7 is 7 - 2 pi (the other branch, one turn on)
    info = {}
    _, r, _ = P.step([7.0, -7.9], [-3.0], info=info)
    assert info == {"neg": False, "turns": 1}
    assert r == pytest.approx(-((7 - 2 * math.pi) ** 2 + 0.1 * 7.9 ** 2 + 0.001 * 4), abs=1e-14)
    assert P.reset([0.0, 0.0]) == [-math.pi, -1.0] and P.reset([0.5, 0.75]) == [0.0, 0.5]


def test_mountaincar_continuous_steps_by_hand():
    # full push right from the valley: v = 0.0015 - 0.0025 cos(-1.5)
    s, r, d = M.step([-0.5, 0.0], [1.0])
    assert s[1] == pytest.approx(0.0015 - 0.0025 * 0.0707372016677029, abs=1e-16)
    assert s[0] == pytest.approx(-0.5 + s[1], abs=1e-16) and r == pytest.approx(-0.1, abs=1e-16) and not d
    # crossing 0.45 moving right terminates and pays 100 - 0.1 a^2
    s, r, d = M.step([0.44, 0.02], [0.5])
    assert d and s[0] >= 0.45 and r == pytest.approx(99.975, abs=1e-13)
    # the left wall stops the car; the reward takes the unclamped action (0.1 * 4), the force the clamped one
    s, r, d = M.step([-1.19, -0.06], [-2.0])
    assert s == [-1.2, 0.0] and r == pytest.approx(-0.4, abs=1e-15) and not d
    s2, _, _ = M.step([-1.19, -0.06], [-1.0])
    assert s2 == s
    # the velocity clamp: 0.0699 + 0.0015 - 0.0025 cos(-1.5) = 0.0712 -> 0.07
    s, r, d = M.step([-0.5, 0.0699], [1.5])
    assert s[1] == 0.07 and r == pytest.approx(-0.225, abs=1e-15) and not d
    # the action is the float32 given
    a32 = np.float32(0.1)
    _, r, _ = M.step([-0.5, 0.0], [0.1])
    assert r == -(float(a32) * float(a32)) * 0.1
    assert M.reset([0.5]) == [-0.6 + 0.2 * 0.5, 0.0]


def test_longdouble_reference_agrees():
    """the same expressions in extended precision: close to the float64 ones, same branches"""
    for env, s, a in ((P, [-4.0, 0.5], [1.0]), (M, [0.44, 0.02], [0.5])):
        i64, ild = {}, {}
        r64 = env.step(s, a, info=i64)
        rld = env.step(s, a, np.longdouble, np.cos, np.sin, np.fmod, ild)
        assert i64 == ild and r64[2] == rld[2]
        assert np.allclose(np.array(r64[0]), np.array(rld[0], np.float64), rtol=0, atol=1e-14)
        assert abs(r64[1] - float(rld[1])) < 1e-13


# ---------------------------------------------------------------------------- the engine's table
def test_cont_env_info_is_the_references_table():
    assert set(CONT_ENVS) == set(C.ENVS)
    literal = {"Pendulum-v1": (3, 2, 1, 2, 200), "MountainCarContinuous-v0": (2, 2, 1, 1, 999)}
    for name, env in C.ENVS.items():
        for key in (name, env.env_id):
            info = cont_env_info(key)
            got = (info["obs_dim"], info["state_dim"], info["act_dim"], info["reset_draws"], info["time_limit"])
            assert got == (env.obs_dim, env.state_dim, env.act_dim, env.reset_draws, env.time_limit) == literal[name]
            assert info["name"] == name and CONT_ENVS[name] == env.env_id
        assert set(info) == {"obs_dim", "state_dim", "act_dim", "reset_draws", "time_limit", "name"}


def test_unknown_ids_and_names_are_rejected_before_a_device_is_touched():
    from trpo_amd._lib import EngineError
    for bad in (2, -1, 99):
        with pytest.raises(EngineError, match=rf"rc=-1.*unknown continuous environment id {bad}\b"):
            cont_env_info(bad)
    for bad in ("Pendulum-v0", "CartPole-v0", "MountainCar-v0"):
        with pytest.raises(ValueError, match="unknown continuous environment"):
            cont_env_info(bad)
        with pytest.raises(ValueError, match="unknown continuous environment"):
            cont_env_step_device(bad, np.zeros((1, 2)), np.zeros((1, 1), np.float32))
    with pytest.raises(EngineError, match=r"rc=-1.*unknown continuous environment id 2\b"):
        cont_env_step_device(2, np.zeros((1, 2)), np.zeros((1, 1), np.float32))
    # the default parameters carry the environment's own time limit, and refuse an unknown id too
    import ctypes
    from trpo_amd import _lib
    p = _lib.RolloutParams()
    assert _lib.lib.trpo_default_rollout_params_cont(1, ctypes.byref(p)) == 0
    assert (p.time_limit, p.n_envs, p.train) == (999, 1, 1)
    assert _lib.lib.trpo_default_rollout_params_cont(2, ctypes.byref(p)) == -1
    assert b"unknown continuous environment id 2" in _lib.lib.trpo_last_error()


def test_agent_refuses_a_shape_that_is_not_the_environments(monkeypatch):
    import trpo_amd.agent as agent_mod

    def no_engine(*a, **k):
        raise AssertionError("an engine was created")

    monkeypatch.setattr(agent_mod, "Engine", no_engine)
    with pytest.raises(ValueError, match=r"config\['env'\]: Pendulum-v1 has obs_dim 3 and act_dim 1.*act_dim 2"):
        agent_mod.TRPOAgent(3, 2, config={"env": "Pendulum-v1"})
    with pytest.raises(ValueError, match=r"MountainCarContinuous-v0 has obs_dim 2 and act_dim 1"):
        agent_mod.TRPOAgent(3, 1, config={"env": "MountainCarContinuous-v0"})


def test_gaussian_paths_to_batch():
    from trpo_amd.agent import gaussian_paths_to_batch
    ls = np.array([-0.5], np.float32)
    paths = [{"obs": np.zeros((3, 2)), "actions": np.ones((3, 1)), "action_means": np.zeros((3, 1)), "logstd": ls,
              "rewards": [1.0, 2.0, 3.0], "tail_value": 7.0},
             {"obs": np.ones((2, 2)), "actions": np.ones((2, 1)), "action_means": np.zeros((2, 1)), "logstd": ls,
              "rewards": [4.0, 5.0], "baseline": [0.5, 0.25]}]
    b = gaussian_paths_to_batch(paths)
    assert b["state"].shape == (5, 2) and b["state"].dtype == np.float32
    assert b["action"].shape == b["action_mean"].shape == (5, 1) and b["action"].dtype == np.float32
    assert np.array_equal(b["logstd"], ls) and b["starts"].tolist() == [1, 0, 0, 1, 0]
    assert b["baseline"].tolist() == [0, 0, 0, 0.5, 0.25] and b["tail_values"].tolist() == [0, 0, 7.0, 0, 0]
    paths[1]["logstd"] = np.array([0.0], np.float32)
    with pytest.raises(ValueError, match="share their logstd"):
        gaussian_paths_to_batch(paths)


# ---------------------------------------------------------------------------- Philox, the uniform, Box-Muller
def test_philox_known_answers():
    """Random123's published Philox4x32-10 vectors (kat_vectors): zeros, all ones, the digits of pi"""
    kat = [([0, 0, 0, 0], (0, 0), [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ([0xffffffff] * 4, (0xffffffff, 0xffffffff), [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], (0xa4093822, 0x299f31d0),
            [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for ctr, key, want in kat:
        assert C.philox4x32_10(ctr, key) == want
    # uniform53 of the zero key and zero counter, from the first vector: ((0x6627e8d5 >> 5) * 2^26 +
    # (0xe169c58d >> 6)) / 2^53 = (53559110 * 67108864 + 59090710) / 9007199254740992
    assert (0x6627e8d5 >> 5, 0xe169c58d >> 6) == (53559110, 59090710)
    want = 3594291088041750 / 9007199254740992
    assert 53559110 * 67108864 + 59090710 == 3594291088041750
    assert C.uniform53(0, 0, 0, 0) == want == 0.39904647231489565
    # the normal's pair takes words (c0, c1) and (c2, c3) of the same call
    u1, u2 = C.normal_uniforms(0, 0, 0, 0)
    assert u1 == want and u2 == ((0xbc57ac4c >> 5) * 67108864 + (0x9b00dbd8 >> 6)) / 9007199254740992
    # the counter's layout: (env, stream, draw lo, draw hi), the key the seed's halves
    assert C.words(0xa4093822 | (0x299f31d0 << 32), 0x243f6a88, 0x85a308d3, 0x13198a2e | (0x03707344 << 32)) == kat[2][2]
    assert C.normal_uniforms(5, 3, 7, 1, act_dim=2) == (C.u53(*C.words(5, 3, 0, 15)[:2]), C.u53(*C.words(5, 3, 0, 15)[2:]))


def test_box_muller():
    assert C.box_muller(0.0, 0.3) == 0.0                       # log(1 - 0) = 0: u1 = 0 is safe
    assert C.box_muller(1 - math.exp(-0.5), 0.0) == pytest.approx(1.0, abs=1e-15)
    assert C.box_muller(1 - math.exp(-2.0), 0.5) == pytest.approx(-2.0, abs=1e-15)
    x = C.box_muller(0.3, 0.7)
    assert x == pytest.approx(float(C.box_muller(0.3, 0.7, np.longdouble, np.sqrt, np.log, np.cos)), abs=1e-15)
    # moments over the first draws of one stream
    xs = np.array([C.box_muller(*C.normal_uniforms(11, 2, k, 0)) for k in range(4000)])
    n = len(xs)
    assert abs(xs.mean()) < 5 / math.sqrt(n) and abs(xs.var() - 1) < 5 * math.sqrt(2 / n)
