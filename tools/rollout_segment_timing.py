"""Wall-clock of the rollout calls on the five built-in environments, the method of DESIGN.md §4's rollout-cost
entries: 256 environments x 20000 steps, policy 64 wide, warm, 30 repeats, one JSON line per environment.

    python tools/rollout_segment_timing.py --tag NAME [--root TREE] [--segments] [--out FILE]

--root TREE   import trpo_amd from another checkout (a build of the parent commit, to alternate with this one)
--segments    also time the segment call (Engine.rollout_segment / rollout_gaussian_segment) at the same n_envs and
              the whole-episode call's mean steps per environment, from a reset (resume=False) and resumed
us_per_step is the call's median over the steps one environment takes in it (the whole-episode call: the mean over
the environments), the latency of one environment's serial steps.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--tag", required=True)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--segments", action="store_true")
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=30)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))

from trpo_amd import Engine, xavier_theta  # noqa: E402
from trpo_amd.engine import CONT_ENVS, ENVS, cont_env_info, env_info  # noqa: E402

N_ENVS, N_STEPS, HIDDEN = 256, 20000, [64]


def timed(call):
    for _ in range(3):
        call()
    ms = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        call()
        ms.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


lines = []
for name in list(ENVS) + list(CONT_ENVS):
    cont = name in CONT_ENVS
    info = cont_env_info(name) if cont else env_info(name)
    A = info["act_dim"] if cont else info["n_actions"]
    e = Engine(info["obs_dim"], HIDDEN, A, max_rows=64, dist="gaussian" if cont else "categorical")
    th = xavier_theta(info["obs_dim"], HIDDEN, A, np.random.RandomState(1))
    e.set_flat(np.concatenate([th, np.zeros(A, np.float32)]) if cont else th)
    roll = e.rollout_gaussian if cont else e.rollout
    n, paths = roll(name, n_envs=N_ENVS, n_timesteps=N_STEPS, seed=1)
    per_env = n / N_ENVS
    rec = {"tag": args.tag, "call": "whole", "env": name, "steps": n, "paths": paths,
           **timed(lambda: roll(name, n_envs=N_ENVS, n_timesteps=N_STEPS, seed=1))}
    rec["us_per_step"] = round(1e3 * rec["median_ms"] / per_env, 3)
    lines.append(rec)
    if args.segments:
        seg = e.rollout_gaussian_segment if cont else e.rollout_segment
        T = int(round(per_env))
        for resume in (False, True):
            n, paths = seg(name, n_envs=N_ENVS, horizon=T, resume=resume, seed=1)
            rec = {"tag": args.tag, "call": "segment-resumed" if resume else "segment", "env": name, "steps": n,
                   "paths": paths, **timed(lambda: seg(name, n_envs=N_ENVS, horizon=T, resume=resume, seed=1))}
            rec["us_per_step"] = round(1e3 * rec["median_ms"] / T, 3)
            lines.append(rec)
    e.close()
text = "\n".join(json.dumps(r) for r in lines)
print(text)
if args.out:
    with open(args.out, "a") as f:
        f.write(text + "\n")
