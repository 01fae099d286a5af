#!/usr/bin/env python
"""Milliseconds per update of the Gaussian engine and of the categorical engine on its per-layer path at the same
dimensions, alternating on one GPU (the Gaussian head).

    python tools/gauss_timing.py [--rows 1000000] [--rounds 5] [--updates 4] [--out profiles/gauss/timing.json]

The categorical engine runs with fused = chain = tail = rfwd01 = hbwd2 = head_fwd = 0, i.e. the per-layer launches
the Gaussian FVP is a subset of.  Each round times `updates` updates of one engine, then of the other (host clock
around Engine.update, which ends in a device synchronise); every update starts from the same theta.  After the
timed rounds one profiled update of each engine gives the per-launch milliseconds.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIMS = [(17, [64, 64], 6), (128, [256, 256], 17)]
PER_LAYER = {"fused": 0, "chain": 0, "tail": 0, "rfwd01": 0, "hbwd2": 0, "head_fwd": 0}


def init_theta(widths, rng, tail=0):
    parts = []
    for a, b in zip(widths[:-1], widths[1:]):
        parts.append((rng.standard_normal((a, b)) / np.sqrt(a)).reshape(-1))
        parts.append(0.1 * rng.standard_normal(b))
    if tail:
        parts.append(-0.5 + 0.3 * rng.standard_normal(tail))
    return np.concatenate(parts).astype(np.float32)


def make_engines(obs, hidden, A, n, seed):
    """two engines on the same states and advantages, each fed from its own policy at theta (theta_old = theta)"""
    from trpo_amd import Engine
    rng = np.random.RandomState(seed)
    X = rng.standard_normal((n, obs)).astype(np.float32)
    adv = rng.standard_normal(n)
    adv = ((adv - adv.mean()) / adv.std()).astype(np.float32)
    widths = [obs, *hidden, A]
    g = Engine(obs, hidden, A, max_rows=n, dist="gaussian")
    th_g = init_theta(widths, rng, tail=A)
    g.set_flat(th_g)
    zeros = np.zeros((n, A), np.float32)
    g.set_batch_gaussian(X, zeros, adv, zeros, th_g[-A:])
    mean, logstd = g.action_mean()
    actions = (mean + np.exp(logstd) * rng.standard_normal((n, A))).astype(np.float32)
    g.set_batch_gaussian(X, actions, adv, mean, logstd)
    c = Engine(obs, hidden, A, max_rows=n)
    th_c = th_g[:-A].copy()
    c.set_flat(th_c)
    c.set_batch(X, np.zeros(n, np.int64), adv, np.full((n, A), 1.0 / A, np.float32))
    dist = c.action_dist()
    acts = (dist.cumsum(1) > rng.uniform(size=(n, 1))).argmax(1).astype(np.int64)
    c.set_batch(X, acts, adv, dist)
    return (g, th_g), (c, th_c)


def timed(engine, theta, updates):
    from trpo_amd import UpdateParams
    ms = []
    for _ in range(updates):
        engine.set_flat(theta)
        engine.synchronize()
        t0 = time.perf_counter()
        st = engine.update(UpdateParams(cg_iters=10, residual_tol=0.0))
        ms.append((time.perf_counter() - t0) * 1e3)
    timed.last = {"k": st["k"], "cg_iters": st["cg_iters"], "reverted": st["reverted"]}
    return ms


def profiled(engine, theta):
    from trpo_amd import UpdateParams
    engine.profile_enable(True)
    engine.profile_reset()
    engine.set_flat(theta)
    engine.update(UpdateParams(cg_iters=10, residual_tol=0.0))
    prof = engine.profile_query()
    engine.profile_enable(False)
    return {k: round(v[1], 4) for k, v in sorted(prof.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--updates", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from trpo_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("gauss_timing: no GPU visible")
    for k, v in PER_LAYER.items():
        _lib.set_option(k, v)
    results = []
    for obs, hidden, A in DIMS:
        (g, th_g), (c, th_c) = make_engines(obs, hidden, A, args.rows, seed=obs)
        for e, th in ((g, th_g), (c, th_c)):
            timed(e, th, 3)   # eager, captured, replayed
        rounds = {"gaussian": [], "categorical": []}
        stats = {}
        for _ in range(args.rounds):
            for name, e, th in (("gaussian", g, th_g), ("categorical", c, th_c)):
                rounds[name].append(float(np.median(timed(e, th, args.updates))))
                stats[name] = timed.last   # line-search trials differ between the two policies: k + 1 loss forwards
        res = {"dims": [obs, hidden, A], "rows": args.rows,
               "ms_per_update": {k: round(float(np.median(v)), 3) for k, v in rounds.items()},
               "round_medians_ms": {k: [round(x, 3) for x in v] for k, v in rounds.items()},
               "update_stats": stats,
               "profile_ms": {"gaussian": profiled(g, th_g), "categorical": profiled(c, th_c)}}
        res["gaussian_over_categorical"] = round(res["ms_per_update"]["gaussian"] / res["ms_per_update"]["categorical"], 4)
        print(json.dumps(res), flush=True)
        results.append(res)
        g.close()
        c.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
