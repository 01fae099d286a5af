"""Plain Python restatement of the continuous-action environments as include/trpo_engine.h defines them
(Pendulum-v1 and MountainCarContinuous-v0), in the style of tests/envs_ref.py, and of the random numbers the
Gaussian rollout draws (Philox4x32-10, the 53-bit uniform, Box-Muller).

Every operation is written once, in the header's order, on scalars of type ``T`` with ``cos`` / ``sin`` / ``fmod``
passed in: ``T=float`` with the ``math`` functions is the float64 definition the device is held to,
``T=np.longdouble`` with numpy's evaluates the same expressions, with the same float64 constants, in extended
precision.  An action component is a float32 widened to ``T``.

``step(s, action, ...)`` returns ``(state, reward, done)`` and never modifies ``s``; ``info``, when a dict, receives
the branches taken (Pendulum: ``neg``, whether the ``m < 0`` adjustment fired, and ``turns`` = floor(y / (2 pi));
MountainCarContinuous: ``done``).
"""
import math

import numpy as np

from envs_ref import PI


def clamp(x, lo, hi):
    return min(max(x, lo), hi)


class PendulumV1:
    name, env_id = "Pendulum-v1", 0
    state_dim, obs_dim, act_dim, reset_draws, time_limit = 2, 3, 1, 2, 200

    @staticmethod
    def reset(u):
        return [-PI + (PI - -PI) * float(u[0]), -1 + (1 - -1) * float(u[1])]

    @staticmethod
    def step(s, action, T=float, cos=math.cos, sin=math.sin, fmod=math.fmod, info=None):
        th, thd = T(s[0]), T(s[1])
        a = T(np.float32(action[0]))
        pi = T(PI)
        u = clamp(a, T(-2), T(2))
        y = th + pi
        m = fmod(y, 2 * pi)
        neg = bool(m < 0)
        if neg:
            m = m + 2 * pi
        an = m - pi
        cost = an * an + T(0.1) * (thd * thd) + T(0.001) * (u * u)
        thd1 = thd + (3 * T(10.0) / (2 * T(1.0)) * sin(th) + T(3.0) / (T(1.0) * (T(1.0) * T(1.0))) * u) * T(0.05)
        thd1 = clamp(thd1, T(-8), T(8))
        th1 = th + thd1 * T(0.05)
        if info is not None:
            info["neg"] = neg
            info["turns"] = int(math.floor(y / (2 * pi)))
        return [th1, thd1], -cost, False

    @staticmethod
    def observe(s, T=float, cos=math.cos, sin=math.sin):
        th = T(s[0])
        return [cos(th), sin(th), T(s[1])]


class MountainCarContinuousV0:
    name, env_id = "MountainCarContinuous-v0", 1
    state_dim, obs_dim, act_dim, reset_draws, time_limit = 2, 2, 1, 1, 999

    @staticmethod
    def reset(u):
        return [-0.6 + (-0.4 - -0.6) * float(u[0]), 0.0]

    @staticmethod
    def step(s, action, T=float, cos=math.cos, sin=math.sin, fmod=math.fmod, info=None):
        p, v = T(s[0]), T(s[1])
        a = T(np.float32(action[0]))
        f = clamp(a, T(-1), T(1))
        v = v + f * T(0.0015) + cos(T(3) * p) * T(-0.0025)
        v = clamp(v, T(-0.07), T(0.07))
        p = p + v
        p = clamp(p, T(-1.2), T(0.6))
        if p == T(-1.2) and v < 0:
            v = T(0)
        done = bool(p >= T(0.45) and v >= 0)
        if info is not None:
            info["done"] = done
        return [p, v], (T(100) if done else T(0)) - (a * a) * T(0.1), done

    @staticmethod
    def observe(s, T=float, cos=math.cos, sin=math.sin):
        return [T(s[0]), T(s[1])]


ENVS = {e.name: e for e in (PendulumV1, MountainCarContinuousV0)}


def step_rows(env, states, actions, T=float, cos=math.cos, sin=math.sin, fmod=math.fmod):
    """env.step and env.observe over rows -> (state_out [n, S], obs [n, O], reward [n], done [n], branch [n, 2]),
    arrays of dtype T (np.float64 for T=float); branch holds (neg, turns) for Pendulum and (done, 0) otherwise."""
    dt = np.float64 if T is float else T
    n = len(actions)
    so, ob, rw = np.empty((n, env.state_dim), dt), np.empty((n, env.obs_dim), dt), np.empty(n, dt)
    dn, br = np.empty(n, bool), np.zeros((n, 2), np.int64)
    for i in range(n):
        info = {}
        s1, rw[i], dn[i] = env.step([T(x) for x in states[i]], actions[i], T, cos, sin, fmod, info)
        so[i] = s1
        ob[i] = env.observe(s1, T, cos, sin)
        br[i] = (info.get("neg", info.get("done", 0)), info.get("turns", 0))
    return so, ob, rw, dn, br


# ---- the rollout's random numbers (rollout.hip): Philox4x32-10, key = seed, counter = (env, stream, draw) ----
M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    c, (k0, k1) = list(counter), key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M32, (p0 >> 32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def u53(hi, lo):
    """numpy's random_sample recipe: ((hi >> 5) * 2^26 + (lo >> 6)) / 2^53"""
    return (float(hi >> 5) * 67108864.0 + float(lo >> 6)) / 9007199254740992.0


def words(seed, env, stream, draw):
    return philox4x32_10([env, stream, draw & M32, draw >> 32], (seed & M32, (seed >> 32) & M32))


def uniform53(seed, env, stream, draw):
    c = words(seed, env, stream, draw)
    return u53(c[0], c[1])


def normal_uniforms(seed, env, step_count, d, act_dim=1):
    """(u1, u2) of action component d at the environment's step `step_count`: stream 0, draw step_count*A + d"""
    c = words(seed, env, 0, step_count * act_dim + d)
    return u53(c[0], c[1]), u53(c[2], c[3])


def box_muller(u1, u2, T=float, sqrt=math.sqrt, log=math.log, cos=math.cos):
    u1, u2 = T(u1), T(u2)
    return sqrt(T(-2.0) * log(T(1.0) - u1)) * cos(2 * T(PI) * u2)
