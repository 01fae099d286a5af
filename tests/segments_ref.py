"""Float64 host model of the segment rollout's bookkeeping (include/trpo_engine.h, trpo_rollout_env_segment): what a
call that gives every environment exactly H steps and continues from a carry records around the steps -- step_index,
starts, the fragments (paths) with their kinds, t0, rows and episode returns, the carry, and which draws it takes.

The steps themselves are not the model's business: it is given ``step(s, action) -> (s', reward, done)`` and
``reset(u) -> s``.  ``env_fns(name)`` makes them from tests/envs_ref.py, tests/cont_envs_ref.py and
oracle/cartpole_oracle.py (the float64 definitions), and a GPU test may pass a replay of arrays the device recorded.

``run_segment`` is one call for one environment; ``run_episodes`` is the whole-episode collection the segments are
cut from (rollout_kernel's: reset, then whole episodes, every step numbered over all of them).
"""
import numpy as np

import cont_envs_ref
import envs_ref
from oracle.cartpole_oracle import CartPoleV0 as _CartPoleDyn

KIND_TERMINATED, KIND_LIMIT, KIND_SEGMENT = 0, 1, 2
ALL_ENVS = ("CartPole-v0", "MountainCar-v0", "Acrobot-v1", "Pendulum-v1", "MountainCarContinuous-v0")


def env_fns(name):
    """(env table class, step, reset, observe) of a built-in environment, on Python floats"""
    if name in cont_envs_ref.ENVS:
        env = cont_envs_ref.ENVS[name]

        def step(s, a):
            s1, r, d = env.step(s, np.asarray(a, np.float32).reshape(-1))
            return [float(x) for x in s1], float(r), bool(d)
    else:
        env = envs_ref.ENVS[name]
        if name == "CartPole-v0":
            def step(s, a):
                s1, d = _CartPoleDyn.dynamics(s, int(a))
                return [float(x) for x in s1], 1.0, bool(d)
        else:
            def step(s, a):
                s1, r, d = env.step(s, int(a))
                return [float(x) for x in s1], float(r), bool(d)
    return env, step, env.reset, (lambda s: [float(x) for x in env.observe(s)])


def run_segment(step, reset, carry, H, ep_max, actions, reset_u):
    """One segment call for one environment.  carry: None (resume = 0: reset with reset index 0) or (s, t, ret).
    actions[k] is the action of the call's step k (its draw index is k); reset_u[i] the uniforms of the call's reset
    i.  Returns a dict: per row ``state`` (the state the row observes), ``reward``, ``step_index``, ``starts``,
    ``action_draw``; per path ``kind``, ``t0``, ``rows``, ``end_row``, ``episode_return``, ``final_state``,
    ``truncated``; ``carry`` (s, t, ret); ``resets`` (how many reset indices the call used, from 0)."""
    resets = 0
    if carry is None:
        s, t, ret = list(reset(reset_u[0])), 0, 0.0
        resets = 1
    else:
        s, t, ret = list(carry[0]), int(carry[1]), float(carry[2])
    assert 0 <= t < ep_max, "a carried episode must have a step left"
    rows = {k: [] for k in ("state", "reward", "step_index", "starts", "action_draw")}
    paths = {k: [] for k in ("kind", "t0", "rows", "end_row", "episode_return", "final_state", "truncated")}
    frag0, t0, fresh = 0, t, True
    for k in range(H):
        rows["state"].append(list(s))
        rows["step_index"].append(t)
        rows["starts"].append(1 if fresh else 0)
        rows["action_draw"].append(k)
        s, reward, done = step(s, actions[k])
        rows["reward"].append(reward)
        t += 1
        ret = ret + reward
        ended = done or t >= ep_max
        fresh = ended
        if not ended and k + 1 < H:
            continue
        paths["kind"].append(KIND_TERMINATED if done else (KIND_LIMIT if ended else KIND_SEGMENT))
        paths["truncated"].append(0 if done else 1)
        paths["t0"].append(t0)
        paths["rows"].append(k + 1 - frag0)
        paths["end_row"].append(k)
        paths["episode_return"].append(ret)
        paths["final_state"].append(list(s))
        if ended:
            s, t, ret = list(reset(reset_u[resets])), 0, 0.0
            resets += 1
            frag0, t0 = k + 1, 0
    out = {k: np.asarray(v) for k, v in rows.items()}
    out.update({k: np.asarray(v) for k, v in paths.items()})
    out["carry"] = (list(s), t, ret)
    out["resets"] = resets
    return out


def run_episodes(step, reset, n_steps, ep_max, actions, reset_u):
    """Whole episodes from a reset for n_steps steps (the last episode may be left unfinished): per step ``state``,
    ``reward``, ``t`` (its index in its episode), ``starts``, ``ended`` (0 no, 1 terminated, 2 the limit),
    ``episode`` (the index of its episode = of its reset), ``ret`` (the episode's return through this step), and
    ``next_state``: the state after the step, before any reset."""
    out = {k: [] for k in ("state", "reward", "t", "starts", "ended", "episode", "ret", "next_state")}
    episode, s, t, ret = 0, list(reset(reset_u[0])), 0, 0.0
    for g in range(n_steps):
        out["state"].append(list(s))
        out["t"].append(t)
        out["starts"].append(1 if t == 0 else 0)
        out["episode"].append(episode)
        s, reward, done = step(s, actions[g])
        t += 1
        ret = ret + reward
        out["reward"].append(reward)
        out["ret"].append(ret)
        out["next_state"].append(list(s))
        ended = 1 if done else (2 if t >= ep_max else 0)
        out["ended"].append(ended)
        if ended:
            episode += 1
            s, t, ret = list(reset(reset_u[episode])), 0, 0.0
    return {k: np.asarray(v) for k, v in out.items()}


def replay_fns(rewards, done, next_states):
    """step / cursor for run_segment and run_episodes that replay recorded steps in order instead of computing them:
    step g returns (next_states[g], rewards[g], done[g]) whatever it is given"""
    cur = {"g": 0}

    def step(_s, _a):
        g = cur["g"]
        cur["g"] = g + 1
        return [float(x) for x in next_states[g]], float(rewards[g]), bool(done[g])
    return step, cur
