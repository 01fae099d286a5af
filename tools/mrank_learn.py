"""Several ranks of the learn() loop (trpo_inksci.py:89-177) against one rank holding every row.

    python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29556 \
        tools/mrank_learn.py [--host-allreduce] [--iters 3] [--env NAME] [--gae LAMBDA] [--bootstrap]
        [--fvp-subsample K] [--horizon T]

--env NAME        any built-in environment (default CartPole-v0): the discrete ones of trpo_amd.engine.ENVS, or a
                  continuous one of CONT_ENVS, which makes the policy a diagonal Gaussian; the agent's dims are the
                  environment's (env_info / cont_env_info)
--gae LAMBDA      GAE(lambda) advantages (config["gae_lambda"]); --bootstrap adds config["bootstrap_truncated"]
--fvp-subsample K the Fisher-vector products on every K-th row by global row index
                  (config["fvp_subsample_rows"] = "global"); the one-rank reference then uses the local
                  set_fvp_subsample(K) on the concatenation
--horizon T       fixed-horizon segments (config["segment_horizon"], needs --gae and --bootstrap): every rank holds
                  exactly 4 * T rows per iteration, which is checked, and the mean reward is over the episodes that
                  finished, by the ranks' rollout_segment_fetch records
--host-allreduce  ranks share a GPU (RCCL refuses duplicate devices): the engine's and the VF's all-reduces
                  run through the stream-ordered host transport, summed by gloo
Each rank rolls out its share of the timestep budget with its own draws (TRPOAgent.set_ranks). Checks:
  * after every iteration all ranks hold bitwise-identical policy and VF parameters and the same stats;
  * the episode count and mean reward are those of the ranks' rollouts concatenated;
  * iteration 0's update (zero baseline, trpo_inksci.py:103) equals a one-rank engine's update of the
    concatenated rollouts from the same parameters: theta and the line search's point within 1e-5, k and reverted
    exact, surr / kl / ent of the ranks equal to that engine's at the ranks' point (and, on the discrete
    environments, to its own update's within 1e-5).  On a continuous
    environment that engine is a Gaussian one fed the ranks' rollout_gaussian_fetch arrays, and the log-std recorded
    with the rollout must be the same on every rank.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-allreduce", action="store_true")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--env", default="CartPole-v0")
    ap.add_argument("--gae", type=float, default=None)
    ap.add_argument("--bootstrap", action="store_true")
    ap.add_argument("--fvp-subsample", type=int, default=1)
    ap.add_argument("--horizon", type=int, default=None)
    args = ap.parse_args()

    import torch
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo")
    ndev = torch.cuda.device_count()
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not args.host_allreduce and local >= ndev:
        raise SystemExit(f"LOCAL_RANK {local} but only {ndev} GPU(s): pass --host-allreduce to share them")
    dev = local % max(1, ndev)
    torch.cuda.set_device(dev)
    from trpo_amd import Engine, TRPOAgent, UpdateParams
    from trpo_amd._lib import VEC_THETA_LS
    from trpo_amd.agent import CONFIG
    from trpo_amd.engine import CONT_ENVS, ENVS, cont_env_info, env_info

    if args.env not in ENVS and args.env not in CONT_ENVS:
        ap.error(f"--env {args.env}: built in are {sorted(ENVS) + sorted(CONT_ENVS)}")
    cont = args.env in CONT_ENVS
    info = cont_env_info(args.env) if cont else env_info(args.env)
    obs_dim, A = info["obs_dim"], info["act_dim"] if cont else info["n_actions"]
    K = args.fvp_subsample
    cfg = dict(CONFIG, env=args.env)
    if args.gae is not None:
        cfg["gae_lambda"] = args.gae
    if args.bootstrap:
        cfg["bootstrap_truncated"] = True
    if K > 1:
        cfg.update(fvp_subsample=K, fvp_subsample_rows="global")
    if args.horizon is not None:
        cfg["segment_horizon"] = args.horizon
    agent = TRPOAgent(obs_dim, A, hidden=(64,), max_rows=8192, device=dev, config=cfg)
    agent.set_ranks(rank, world, host_allreduce=args.host_allreduce)
    hist = agent.learn(max_iterations=args.iters, n_envs=4, seed=5, log=None, record=True)
    keep = ("steps", "paths", "train", "reward_mean", "episodes", "k", "kl", "surr", "entropy",
            "explained_variance", "reverted", "theta_before", "theta", "theta_ls", "vf_params")
    roll_keys = ("obs", "actions", "means", "logstd", "rewards", "starts") if cont else (
        "obs", "actions", "action_dists", "rewards", "starts")
    mine = [{k: h[k] for k in keep if k in h} | {"rollout": {k: h["rollout"][k] for k in roll_keys},
                                                 "tail_values": h["tail_values"]} |
            ({"segment": h["segment"]} if "segment" in h else {}) for h in hist]
    objs = [None] * world
    dist.all_gather_object(objs, mine)
    if rank == 0:
        n_it = len(objs[0])
        assert all(len(o) == n_it for o in objs), [len(o) for o in objs]
        total_eps = 0
        for i in range(n_it):
            ref = objs[0][i]
            for r in range(1, world):
                o = objs[r][i]
                for k in ("reward_mean", "episodes", "k", "kl", "surr", "entropy", "explained_variance",
                          "reverted", "train"):
                    same = o.get(k) == ref.get(k) or (k == "reward_mean" and o[k] != o[k] and ref[k] != ref[k])
                    assert same, (i, r, k, o.get(k), ref.get(k))
                for k in ("theta_before", "theta", "theta_ls", "vf_params"):
                    if k in ref:
                        assert np.array_equal(o[k], ref[k]), (i, r, k)
            ro = [objs[r][i]["rollout"] for r in range(world)]
            rewards = np.concatenate([x["rewards"] for x in ro])
            starts = np.concatenate([x["starts"] for x in ro]).astype(bool)
            if args.horizon is not None:
                # equal row counts on every rank, and the mean over the episodes that finished in this iteration
                rows = [objs[r][i]["steps"] for r in range(world)]
                assert rows == [4 * args.horizon] * world, (i, rows)
                sg = [objs[r][i]["segment"] for r in range(world)]
                eps = np.concatenate([x["episode_returns"][x["end_kind"] < 2] for x in sg])
                if len(eps) == 0:   # none finished: the previous value (NaN before the first)
                    prev = objs[0][i - 1]["reward_mean"] if i else float("nan")
                    assert ref["reward_mean"] == prev or (prev != prev and ref["reward_mean"] != ref["reward_mean"])
            else:
                eps = np.add.reduceat(rewards, np.flatnonzero(starts))
            if len(eps):
                assert abs(ref["reward_mean"] - eps.mean()) <= 1e-12 * abs(eps.mean()), (
                    i, ref["reward_mean"], eps.mean())
            if ref.get("train"):
                total_eps += len(eps)
                assert ref["episodes"] == total_eps, (i, ref["episodes"], total_eps)
        # iteration 0 against one engine holding the concatenated rollouts
        h0 = objs[0][0]
        ro = [objs[r][0]["rollout"] for r in range(world)]
        X = np.concatenate([x["obs"] for x in ro]).astype(np.float32)
        acts = np.concatenate([x["actions"] for x in ro])
        rewards = np.concatenate([x["rewards"] for x in ro])
        starts = np.concatenate([x["starts"] for x in ro])
        N = X.shape[0]
        e = Engine(obs_dim, [64], A, max_rows=N, device=dev, dist="gaussian" if cont else "categorical")
        e.set_flat(h0["theta_before"])
        if K > 1:
            e.set_fvp_subsample(K)
        if args.gae is not None:
            e.set_advantage_estimator("gae", args.gae)
        if cont:
            for x in ro[1:]:   # one old policy: every rank sampled with the same log-std
                assert np.array_equal(x["logstd"], ro[0]["logstd"]), "ranks rolled out with different log-stds"
            e.set_batch_gaussian(X, acts, None, np.concatenate([x["means"] for x in ro]), ro[0]["logstd"])
        else:
            e.set_batch(X, acts, None, np.concatenate([x["action_dists"] for x in ro]))
        e.set_rewards(rewards, starts)
        tails = np.concatenate([objs[r][0]["tail_values"] for r in range(world)])
        if args.gae is not None and tails.any():
            e.set_tail_values(tails)
        st = e.update(UpdateParams(cg_iters=10, residual_tol=1e-10, cg_damping=0.1, max_kl=0.01,
                                   compute_advantages=True, gamma=0.95))
        th = e.get_flat()
        th_ls = e.get_vector(VEC_THETA_LS)
        at_ranks_point = e.eval_losses(h0["theta_ls"])     # [surr, kl, ent] of all rows at the ranks' trial point
        e.close()
        r_th, r_ls = rel(h0["theta"], th), rel(h0["theta_ls"], th_ls)
        assert r_th <= 1e-5, ("theta", r_th)
        assert r_ls <= 1e-5, ("theta_ls", r_ls)
        assert st["k"] == h0["k"], (st["k"], h0["k"])
        assert bool(st["reverted"]) == bool(h0["reverted"]), (st["reverted"], h0["reverted"])
        # The ranks' all-reduced losses against one engine's at the same point (the ranks' theta_ls), at the bar of
        # tests/test_gpu_parity.py's losses (rel 1e-5, abs 1e-7: the surrogate is a mean of O(1) float32 row terms
        # that cancel).  The two runs' own trial points differ by up to the theta bar above, and a loss differs by
        # its gradient times that, which no fixed relative bar on the scalar bounds where the step left the
        # quadratic region (Pendulum-v1's first update has kl_after = 6 max_kl); the discrete environments keep
        # that comparison as well, as before.
        for i, hk in enumerate(("surr", "kl", "entropy")):
            assert abs(at_ranks_point[i] - h0[hk]) <= 1e-5 * abs(at_ranks_point[i]) + 1e-7, (
                hk, float(at_ranks_point[i]), h0[hk])
        for k, hk in (("surr_after", "surr"), ("kl_after", "kl"), ("ent_after", "entropy")):
            print(f"{hk}: one rank {st[k]!r}, ranks {h0[hk]!r}, one rank at the ranks' point "
                  f"{float(at_ranks_point[('surr', 'kl', 'entropy').index(hk)])!r}")
            if not cont:
                assert abs(st[k] - h0[hk]) <= 1e-5 * abs(st[k]) + 1e-9, (k, st[k], h0[hk])
        if args.horizon is not None:
            print(f"rows per rank and iteration: {[[objs[r][i]['steps'] for r in range(world)] for i in range(n_it)]}")
        print(f"{world} ranks x {n_it} learn() iterations: ranks bitwise identical; iteration 0 vs one rank: "
              f"theta rel L2 {r_th:.2e} (line-search point {r_ls:.2e}), k {st['k']}, rows {N}")
        print("MRANK LEARN OK")
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
