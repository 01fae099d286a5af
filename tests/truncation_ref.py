"""Host reference for how the paths of a rollout ended, and the inputs the truncation tests share.

``ends`` replays each path's last transition with the oracle's CartPole-v0 dynamics
(oracle/cartpole_oracle.py): a path whose last step does not terminate the environment was cut off by the
time limit or by max_pathlength (truncated); a step that terminates and reaches the limit is a termination.
"""
import functools

import numpy as np

from conftest import golden
from oracle import cartpole_oracle as C

WIDTHS = [4, 64, 2]
N_ENVS, N_TIMESTEPS = 8, 1200
BUDGET = -(-N_TIMESTEPS // N_ENVS)        # 150 steps per environment, and its most episodes
CAP = BUDGET + 19                         # rows per environment region at an episode limit of 20


def ends(out, theta, widths):
    """out: the concatenated rollout (obs f64 [N,4], actions, starts).  -> dict of truncated u8 [P],
    final_obs f64 [P,4] (s_T), final_dist f32 [P,A] (the policy at float32(s_T) for truncated paths, zeros
    otherwise), lengths i64 [P], end_rows i64 [P]."""
    starts = np.flatnonzero(np.asarray(out["starts"]))
    n = len(out["starts"])
    end_rows = np.r_[starts[1:], n] - 1
    A = widths[-1]
    trunc, fobs, fdist = [], [], []
    for i in end_rows:
        s1, done = C.CartPoleV0.dynamics(out["obs"][i], int(out["actions"][i]))
        s1 = np.array(s1, np.float64)
        trunc.append(0 if done else 1)
        fobs.append(s1)
        fdist.append(np.zeros(A, np.float32) if done else C.policy_dist32(theta, s1, widths)[0])
    return {"truncated": np.array(trunc, np.uint8), "final_obs": np.array(fobs, np.float64).reshape(-1, widths[0]),
            "final_dist": np.array(fdist, np.float32).reshape(-1, A),
            "lengths": (end_rows - starts + 1).astype(np.int64), "end_rows": end_rows.astype(np.int64)}


@functools.lru_cache(maxsize=None)
def theta():
    return golden("rollout.npz")["a_theta"]


@functools.lru_cache(maxsize=None)
def draws():
    """(reset_u [8][150][4], act_u [8][169]) from RandomState(5), in that order."""
    rng = np.random.RandomState(5)
    reset_u = rng.random_sample((N_ENVS, BUDGET, 4))
    act_u = rng.random_sample((N_ENVS, CAP))
    return reset_u, act_u


@functools.lru_cache(maxsize=None)
def oracle(max_pathlength=1000, time_limit=20):
    """(rollout, ends) of the CPU oracle on the shared inputs; computed once per setting, never modified."""
    reset_u, act_u = draws()
    out = C.rollout_envs(theta(), WIDTHS, N_ENVS, N_TIMESTEPS, reset_u, act_u, max_pathlength=max_pathlength,
                         time_limit=time_limit)
    e = ends(out, theta(), WIDTHS)
    for d in (out, e):
        for v in d.values():
            v.setflags(write=False)
    return out, e


def device_rollout(engine, max_pathlength=1000, time_limit=20):
    """The shared inputs through the device rollout; -> (n, n_paths)."""
    reset_u, act_u = draws()
    cap = BUDGET + min(max_pathlength, time_limit) - 1
    return engine.rollout_cartpole(n_envs=N_ENVS, n_timesteps=N_TIMESTEPS, max_pathlength=max_pathlength,
                                   time_limit=time_limit, reset_uniforms=reset_u,
                                   action_uniforms=np.ascontiguousarray(act_u[:, :cap]),
                                   max_episodes_per_env=BUDGET)
