"""Plain Python restatement of the built-in environments as include/trpo_engine.h defines them: CartPole-v0 (only
its table and reset; oracle/cartpole_oracle.py holds its dynamics), MountainCar-v0 and Acrobot-v1.

Every operation is written once, in the header's order, on scalars of type ``T`` with ``cos`` / ``sin`` passed in:
``T=float`` with ``math.cos`` / ``math.sin`` is the float64 definition the device is held to (Python floats are IEEE
doubles and CPython never contracts a*b+c), ``T=np.longdouble`` with ``np.cos`` / ``np.sin`` evaluates the same
expressions, with the same float64 constants, in extended precision: the difference of the two on given inputs
measures how far one rounding of cos / sin or of an intermediate can move the result there.

``step(s, action, ...)`` returns ``(state, reward, done)`` and never modifies ``s``; ``info``, when a dict, receives
the branches taken (Acrobot: ``wraps``, the signed number of 2 pi shifts of each angle).
"""
import math

import numpy as np

PI = 3.141592653589793


class CartPoleV0:
    name, env_id = "CartPole-v0", 0
    state_dim, obs_dim, n_actions, reset_draws, time_limit = 4, 4, 2, 4, 200

    @staticmethod
    def reset(u):
        return [-0.05 + (0.05 - -0.05) * float(u[i]) for i in range(4)]

    @staticmethod
    def observe(s, T=float, cos=math.cos, sin=math.sin):
        return [T(x) for x in s]


class MountainCarV0:
    name, env_id = "MountainCar-v0", 1
    state_dim, obs_dim, n_actions, reset_draws, time_limit = 2, 2, 3, 1, 200

    @staticmethod
    def reset(u):
        return [-0.6 + (-0.4 - -0.6) * float(u[0]), 0.0]

    @staticmethod
    def step(s, action, T=float, cos=math.cos, sin=math.sin, info=None):
        p, v = T(s[0]), T(s[1])
        v = v + T(int(action) - 1) * T(0.001) + cos(T(3) * p) * T(-0.0025)
        v = min(max(v, T(-0.07)), T(0.07))
        p = p + v
        p = min(max(p, T(-1.2)), T(0.6))
        if p == T(-1.2) and v < 0:
            v = T(0)
        done = bool(p >= T(0.5) and v >= 0)
        return [p, v], -1.0, done

    @staticmethod
    def observe(s, T=float, cos=math.cos, sin=math.sin):
        return [T(s[0]), T(s[1])]


class AcrobotV1:
    name, env_id = "Acrobot-v1", 2
    state_dim, obs_dim, n_actions, reset_draws, time_limit = 4, 6, 3, 4, 500
    MAX_W1, MAX_W2 = 4 * PI, 9 * PI

    @staticmethod
    def reset(u):
        return [-0.1 + (0.1 - -0.1) * float(u[i]) for i in range(4)]

    @staticmethod
    def deriv(y, a, T, cos, sin):
        m1 = m2 = l1 = T(1.0)
        lc1 = lc2 = T(0.5)
        I1 = I2 = T(1.0)
        g, pi = T(9.8), T(PI)
        t1, t2, w1, w2 = y
        d1 = m1 * (lc1 * lc1) + m2 * (l1 * l1 + lc2 * lc2 + 2 * l1 * lc2 * cos(t2)) + I1 + I2
        d2 = m2 * (lc2 * lc2 + l1 * lc2 * cos(t2)) + I2
        phi2 = m2 * lc2 * g * cos(t1 + t2 - pi / 2)
        phi1 = (-m2 * l1 * lc2 * (w2 * w2) * sin(t2) - 2 * m2 * l1 * lc2 * w2 * w1 * sin(t2)
                + (m1 * lc1 + m2 * l1) * g * cos(t1 - pi / 2) + phi2)
        dd2 = ((a + d2 / d1 * phi1 - m2 * l1 * lc2 * (w1 * w1) * sin(t2) - phi2)
               / (m2 * (lc2 * lc2) + I2 - (d2 * d2) / d1))
        dd1 = -(d2 * dd2 + phi1) / d1
        return [w1, w2, dd1, dd2]

    @classmethod
    def step(cls, s, action, T=float, cos=math.cos, sin=math.sin, info=None):
        a = T(int(action) - 1)
        dt, pi = T(0.2), T(PI)
        y = [T(x) for x in s]
        f = cls.deriv
        k1 = f(y, a, T, cos, sin)
        k2 = f([y[i] + dt / 2 * k1[i] for i in range(4)], a, T, cos, sin)
        k3 = f([y[i] + dt / 2 * k2[i] for i in range(4)], a, T, cos, sin)
        k4 = f([y[i] + dt * k3[i] for i in range(4)], a, T, cos, sin)
        n = [y[i] + dt / 6 * (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]) for i in range(4)]
        wraps = []
        for i in (0, 1):
            x, w = n[i], 0
            while x > pi:
                x -= 2 * pi
                w -= 1
            while x < -pi:
                x += 2 * pi
                w += 1
            n[i] = x
            wraps.append(w)
        n[2] = min(max(n[2], T(-cls.MAX_W1)), T(cls.MAX_W1))
        n[3] = min(max(n[3], T(-cls.MAX_W2)), T(cls.MAX_W2))
        done = bool(-cos(n[0]) - cos(n[1] + n[0]) > 1.0)
        if info is not None:
            info["wraps"] = tuple(wraps)
        return n, (0.0 if done else -1.0), done

    @staticmethod
    def observe(s, T=float, cos=math.cos, sin=math.sin):
        t1, t2 = T(s[0]), T(s[1])
        return [cos(t1), sin(t1), cos(t2), sin(t2), T(s[2]), T(s[3])]


ENVS = {e.name: e for e in (CartPoleV0, MountainCarV0, AcrobotV1)}


def step_rows(env, states, actions, T=float, cos=math.cos, sin=math.sin):
    """env.step and env.observe over rows -> (state_out [n, S], obs [n, O], reward [n], done [n], wraps [n, 2]),
    arrays of dtype T (np.float64 for T=float)."""
    dt = np.float64 if T is float else T
    n = len(actions)
    so, ob = np.empty((n, env.state_dim), dt), np.empty((n, env.obs_dim), dt)
    rw, dn, wr = np.empty(n), np.empty(n, bool), np.zeros((n, 2), np.int64)
    for i in range(n):
        info = {}
        s1, rw[i], dn[i] = env.step([T(x) for x in states[i]], int(actions[i]), T, cos, sin, info)
        so[i] = s1
        ob[i] = env.observe(s1, T, cos, sin)
        wr[i] = info.get("wraps", (0, 0))
    return so, ob, rw, dn, wr
