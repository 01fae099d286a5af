"""Run the reference's learn() loop (trpo_inksci.py:89-177) on CartPole-v0 on the GPU and print the
reference's per-iteration statistics.
usage: python tools/learn_cartpole.py [iterations] [n_envs] [gae_lambda] [bootstrap]
(gae_lambda given: GAE(lambda) advantages instead of the reference's discount(rewards) - baseline;
the word "bootstrap" after it: paths cut off by the time limit are bootstrapped from V(s_T))"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from trpo_amd import TRPOAgent  # noqa: E402
from trpo_amd.agent import CONFIG  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 60
n_envs = int(sys.argv[2]) if len(sys.argv) > 2 else 1
gae_lambda = float(sys.argv[3]) if len(sys.argv) > 3 else None
bootstrap = len(sys.argv) > 4
if bootstrap and sys.argv[4] != "bootstrap":
    sys.exit(f"unknown fourth argument {sys.argv[4]!r}: expected 'bootstrap'")
config = {**CONFIG, "gae_lambda": gae_lambda}
if bootstrap:
    config["bootstrap_truncated"] = True
agent = TRPOAgent(4, 2, hidden=(64,), max_rows=8192, config=config)
t0 = time.time()
hist = agent.learn(max_iterations=iters, n_envs=n_envs, seed=1)
dt = time.time() - t0
print(f"\n{len(hist)} iterations in {dt:.2f} s ({1000 * dt / max(1, len(hist)):.1f} ms/iteration, n_envs={n_envs})")
print("mean episode reward per iteration:", " ".join(f"{h['reward_mean']:.0f}" for h in hist))
print("explained variance per iteration:", " ".join(f"{h['explained_variance']:.3f}" if "explained_variance" in h
                                                    else "-" for h in hist))
