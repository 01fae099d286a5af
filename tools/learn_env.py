"""Run learn() (the reference's loop, trpo_inksci.py:89-177) on one of the built-in environments on the GPU and
print the reference's per-iteration statistics.
usage: python tools/learn_env.py ENV iterations n_envs [gae_lambda] [bootstrap] [fvp=K] [horizon=T]
ENV is CartPole-v0, MountainCar-v0 or Acrobot-v1 (trpo_amd.engine.ENVS), or a continuous-action environment under a
diagonal-Gaussian policy: Pendulum-v1 or MountainCarContinuous-v0 (trpo_amd.engine.CONT_ENVS).  gae_lambda given: GAE(lambda) advantages
instead of the reference's discount(rewards) - baseline; the word "bootstrap" after it: paths cut off by the time
limit are bootstrapped from V(s_T); fvp=K (anywhere after n_envs): the Fisher-vector products run on every K-th row of
the batch (config["fvp_subsample"]); horizon=T (it needs gae_lambda and bootstrap): fixed-horizon segments, every
environment takes exactly T steps per iteration and continues where the last one left it
(config["segment_horizon"]); the mean episode reward is then over the episodes that finished in the iteration and
prints as nan before the first.  Training stops at the reference's mean episode reward of 1.1*500 on
CartPole-v0; the others, whose mean episode rewards stay below it, train for all the iterations asked for."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from trpo_amd import TRPOAgent  # noqa: E402
from trpo_amd.agent import CONFIG  # noqa: E402
from trpo_amd.engine import CONT_ENVS, ENVS, cont_env_info, env_info  # noqa: E402

if len(sys.argv) < 4 or (sys.argv[1] not in ENVS and sys.argv[1] not in CONT_ENVS):
    sys.exit(__doc__)
fvp = [a for a in sys.argv[4:] if a.startswith("fvp=")]
horizon = [a for a in sys.argv[4:] if a.startswith("horizon=")]
sys.argv = [a for a in sys.argv if not a.startswith(("fvp=", "horizon="))]
env = sys.argv[1]
iters, n_envs = int(sys.argv[2]), int(sys.argv[3])
gae_lambda = float(sys.argv[4]) if len(sys.argv) > 4 else None
bootstrap = len(sys.argv) > 5
if bootstrap and sys.argv[5] != "bootstrap":
    sys.exit(f"unknown fifth argument {sys.argv[5]!r}: expected 'bootstrap'")
if env in CONT_ENVS:
    info = cont_env_info(env)
    info["n_actions"] = info["act_dim"]
else:
    info = env_info(env)
config = {**CONFIG, "env": env, "gae_lambda": gae_lambda}
if bootstrap:
    config["bootstrap_truncated"] = True
if fvp:
    config["fvp_subsample"] = int(fvp[-1][4:])
# every environment can overshoot its share of the step budget by one episode
budget = -(-config["episodes_per_roll"] // n_envs)
max_rows = n_envs * (budget + min(config["max_steps"], info["time_limit"]) - 1)
if horizon:
    config["segment_horizon"] = int(horizon[-1][8:])
    max_rows = n_envs * config["segment_horizon"]
agent = TRPOAgent(info["obs_dim"], info["n_actions"], hidden=(64,), max_rows=max_rows, config=config)
t0 = time.time()
hist = agent.learn(max_iterations=iters, n_envs=n_envs, seed=1)
dt = time.time() - t0
print(f"\n{env}: {len(hist)} iterations in {dt:.2f} s ({1000 * dt / max(1, len(hist)):.1f} ms/iteration, "
      f"n_envs={n_envs})")
print("mean episode reward per iteration:", " ".join(f"{h['reward_mean']:.0f}" for h in hist))
print("explained variance per iteration:", " ".join(f"{h['explained_variance']:.3f}" if "explained_variance" in h
                                                    else "-" for h in hist))
