#!/usr/bin/env python
"""Milliseconds per update with the Fisher-vector products on every k-th row of the batch
(Engine.set_fvp_subsample), k in {1, 2, 5, 10}, alternating on one GPU (Fisher subsampling).

    python tools/fvp_subsample_timing.py [--cases c3,c4,gauss] [--rounds 3] [--updates 3]
                                         [--out profiles/fvp_subsample/timing.json]
    python tools/fvp_subsample_timing.py --gather [--cases c4] [--out profiles/fvp_subsample_ranks/gather_timing.json]

Cases: c3 (17 -> 64 -> 64 -> 6, 1M rows), c4 (128 -> 256 -> 256 -> 17, 8M rows) and gauss (the diagonal-Gaussian head
at (17, [64, 64], 6), 1M rows).  One engine per case is alive at a time; a round sets each stride in turn on it (which
rebuilds the Fisher child and drops the update graph), runs three warm-up updates (eager, captured, replayed) and
times `updates` more (host clock around Engine.update, which ends in a device synchronise; every update starts from
the same theta and computes its advantages, so the gather runs inside the replayed graph).  After the rounds one
profiled update per stride gives the gather's milliseconds, the child's prepare pass and its FVP launches.

--gather times the gather launch alone at k = 5: the local mode (first row 0) against the global mode
(set_fvp_subsample(5, rows="global")) of the same feed loaded at row offsets 3 and 1 (first rows 2 and 4), n_global =
rows + 5, no transport.  It reads the same number of bytes at another start, so the times should agree.  One engine;
`--updates` profiled updates per mode, the modes alternating over `--rounds`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STRIDES = (1, 2, 5, 10)
CASES = {"c3": ("categorical", 17, [64, 64], 6, 1_000_000), "c4": ("categorical", 128, [256, 256], 17, 8_000_000),
         "gauss": ("gaussian", 17, [64, 64], 6, 1_000_000)}
EPISODE_LEN = 200
# the child's launches that belong to a Fisher-vector product or the CG around it; its other tags are its prepare pass
FVP_TAGS = ("sub.fvp", "sub.reduce", "sub.cg_vec", "sub.split_v", "sub.logstd_block")


def init_theta(widths, rng, tail=0):
    parts = []
    for a, b in zip(widths[:-1], widths[1:]):
        parts.append((rng.standard_normal((a, b)) / np.sqrt(a)).reshape(-1))
        parts.append(0.1 * rng.standard_normal(b))
    if tail:
        parts.append(-0.5 + 0.3 * rng.standard_normal(tail))
    return np.concatenate(parts).astype(np.float32)


def make_engine(dist, obs, hidden, A, n, seed=1, with_refeed=False):
    """An engine with a steady-state feed (pi_old = the policy at theta) built on the device, and its theta; with_refeed
    also a function (n_global, row_offset) that loads the same feed again as a shard of a larger batch."""
    import torch
    from trpo_amd import Engine
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    rng = np.random.RandomState(seed)
    gaussian = dist == "gaussian"
    theta = init_theta([obs, *hidden, A], rng, tail=A if gaussian else 0)
    eng = Engine(obs, hidden, A, max_rows=n, dist=dist)
    eng.set_flat(theta)
    X = torch.randn((n, obs), generator=gen, device=dev, dtype=torch.float32)
    zeros = torch.zeros((n,), device=dev, dtype=torch.float32)
    rewards = torch.rand((n,), generator=gen, device=dev, dtype=torch.float64)
    starts = ((torch.arange(n, device=dev) % EPISODE_LEN) == 0).to(torch.uint8)
    if gaussian:
        logstd = torch.from_numpy(theta[-A:].copy()).to(dev)
        zA = torch.zeros((n, A), device=dev, dtype=torch.float32)
        eng.set_batch_gaussian(X, zA, zeros, zA, logstd)
        mean, _ = eng.action_mean()
        mean = torch.from_numpy(mean).to(dev)
        actions = mean + torch.exp(logstd) * torch.randn((n, A), generator=gen, device=dev, dtype=torch.float32)
        eng.set_batch_gaussian(X, actions, zeros, mean, logstd)

        def refeed(n_global, row_offset):
            eng.set_batch_gaussian(X, actions, zeros, mean, logstd, n_global=n_global, row_offset=row_offset)
            eng.set_rewards(rewards, starts)
    else:
        actions = torch.randint(0, A, (n,), generator=gen, device=dev, dtype=torch.int64)
        uniform = torch.full((n, A), 1.0 / A, device=dev, dtype=torch.float32)
        eng.set_batch(X, actions, zeros, uniform)
        old = torch.empty((n, A), device=dev, dtype=torch.float32)
        eng.action_dist(out=old)
        eng.set_batch(X, actions, zeros, old)

        def refeed(n_global, row_offset):
            eng.set_batch(X, actions, zeros, old, n_global=n_global, row_offset=row_offset)
            eng.set_rewards(rewards, starts)
    eng.set_rewards(rewards, starts)
    torch.cuda.synchronize()
    theta_dev = torch.from_numpy(theta).to(dev)
    return (eng, theta_dev, refeed) if with_refeed else (eng, theta_dev)


def timed(engine, theta, updates):
    from trpo_amd import UpdateParams
    ms = []
    for _ in range(updates):
        engine.set_flat(theta)
        engine.synchronize()
        t0 = time.perf_counter()
        st = engine.update(UpdateParams(cg_iters=10, residual_tol=0.0, compute_advantages=True))
        ms.append((time.perf_counter() - t0) * 1e3)
    timed.last = {"k": st["k"], "cg_iters": st["cg_iters"], "reverted": st["reverted"]}
    return ms


def profiled(engine, theta):
    from trpo_amd import UpdateParams
    engine.profile_enable(True)
    engine.profile_reset()
    engine.set_flat(theta)
    engine.update(UpdateParams(cg_iters=10, residual_tol=0.0, compute_advantages=True))
    prof = engine.profile_query()
    engine.profile_enable(False)
    tags = {k: round(v[1], 4) for k, v in sorted(prof.items())}
    sub = {k: v for k, v in tags.items() if k.startswith("sub.")}
    fvp = sum(v for k, v in sub.items() if k.startswith(FVP_TAGS))
    return {"gather_ms": tags.get("fisher_gather", 0.0), "child_fvp_ms": round(fvp, 4),
            "child_prepare_ms": round(sum(sub.values()) - fvp, 4),
            "parent_fvp_ms": round(sum(v for k, v in tags.items() if k.startswith(("fvp", "reduce", "cg_vec", "split_v"))),
                                   4),
            "total_ms": round(sum(tags.values()), 4), "tags": tags}


def gather_timing(case, rounds, updates):
    from trpo_amd import UpdateParams
    dist, obs, hidden, A, n = CASES[case]
    eng, theta, refeed = make_engine(dist, obs, hidden, A, n, with_refeed=True)
    k = 5
    modes = (("local", None), ("global", 3), ("global", 1))
    ms = {m: [] for m in modes}
    eng.profile_enable(True)
    for _ in range(rounds):
        for mode in modes:
            rows, offset = mode
            eng.set_fvp_subsample(1)
            if offset is None:
                refeed(n, 0)
            else:
                refeed(n + k, offset)
            eng.set_fvp_subsample(k, rows=rows)
            for _u in range(updates):
                eng.profile_reset()
                eng.set_flat(theta)
                eng.update(UpdateParams(cg_iters=10, residual_tol=0.0, compute_advantages=True))
                count, total = eng.profile_query()["fisher_gather"]
                ms[mode].append(total / count)
    eng.close()
    out = {"case": case, "dims": [obs, hidden, A], "rows": n, "stride": k, "modes": []}
    for (rows, offset), v in ms.items():
        phase = 0 if offset is None else (k - offset % k) % k
        out["modes"].append({"rows": rows, "row_offset": offset or 0, "first_row": phase,
                             "gather_ms_median": round(float(np.median(v)), 4),
                             "gather_ms_min": round(float(np.min(v)), 4), "gather_ms_max": round(float(np.max(v)), 4),
                             "launches": len(v)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c3,c4,gauss")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--updates", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--gather", action="store_true")
    args = ap.parse_args()
    import torch
    # torch bundles its own HIP runtime, which cannot start after the engine library's: it goes first
    if not torch.cuda.is_available():
        raise SystemExit("fvp_subsample_timing: no GPU visible")
    torch.zeros(1, device="cuda:0")
    results = []
    for case in args.cases.split(",") if args.gather else ():
        res = gather_timing(case, args.rounds, args.updates)
        print(json.dumps(res), flush=True)
        results.append(res)
    for case in () if args.gather else args.cases.split(","):
        dist, obs, hidden, A, n = CASES[case]
        eng, theta = make_engine(dist, obs, hidden, A, n)
        rounds = {k: [] for k in STRIDES}
        stats = {}
        for _ in range(args.rounds):
            for k in STRIDES:
                eng.set_fvp_subsample(k)
                timed(eng, theta, 3)   # eager, captured, replayed
                rounds[k].append(float(np.median(timed(eng, theta, args.updates))))
                stats[k] = timed.last
        prof = {}
        for k in STRIDES:
            eng.set_fvp_subsample(k)
            prof[k] = profiled(eng, theta)
        ms = {k: round(float(np.median(v)), 3) for k, v in rounds.items()}
        res = {"case": case, "dist": dist, "dims": [obs, hidden, A], "rows": n,
               "ms_per_update": {str(k): v for k, v in ms.items()},
               "speedup_over_k1": {str(k): round(ms[1] / v, 3) for k, v in ms.items()},
               "round_medians_ms": {str(k): [round(x, 3) for x in v] for k, v in rounds.items()},
               "update_stats": {str(k): v for k, v in stats.items()},
               "profile": {str(k): v for k, v in prof.items()}}
        print(json.dumps({k: v for k, v in res.items() if k != "profile"}), flush=True)
        for k in STRIDES:
            p = prof[k]
            print(f"  {case} k={k}: gather {p['gather_ms']} ms, child prepare {p['child_prepare_ms']} ms, child FVPs "
                  f"{p['child_fvp_ms']} ms, parent FVPs {p['parent_fvp_ms']} ms, profiled total {p['total_ms']} ms",
                  flush=True)
        results.append(res)
        eng.close()
        del eng
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
