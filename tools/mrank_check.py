"""Several ranks on the visible GPU(s): the engine's multi-rank update vs a single-rank engine.

    python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29555 \
        tools/mrank_check.py [--host-allreduce] [--dims c3|c4|c5|g17] [--dist gaussian] [--rows N] [--graphs]
        [--max-kl X] [--residual-tol T] [--adv-scale S] [--expect ITERS,K,REVERTED] [--fvp-subsample K]

--host-allreduce  ranks share a GPU (RCCL refuses duplicate devices): the engine's all-reduces run
                  through its stream-ordered host transport, summed by gloo on the host
--dims c4         obs 128, 256x256, 18 actions: the wide layers take the f16-split MFMA row GEMMs
--dims c5         obs 376, 1024x1024, 17 actions (BASELINE configs[4]'s layer shapes)
--graphs          also replay the update as a captured hipGraph (all-reduces inside it) and require
                  every replay to be bitwise identical to the eager update
--dist gaussian   a diagonal-Gaussian engine (set_batch_gaussian with the advantages given directly): --dims g17
                  is (17, [64, 64], 6) and c4 is read as (128, [256, 256], 17); the cut between the ranks is uneven
                  (shard_bounds moved to the next multiple of 173 rows); stepdir is held to 1e-5 too, and the
                  log-std tail of Hv, theta and stepdir also on its own
--max-kl, --residual-tol   the update's parameters (defaults 0.01 and 0: ten CG iterations, k = 0): with them the
                  update stops CG early, backtracks or rejects every trial, on every rank at the same place
--adv-scale S     the advantages times S (rdotr times S^2: another stop under the same tol); S != 1 feeds the
                  categorical engine the standardised advantages directly instead of the rewards
--expect I,K,R    what cg_iters, k and reverted must be (tests/update_outcomes_ref.py's float64 reference)
--fvp-subsample K  the Fisher-vector products on every K-th row by global row index (set_fvp_subsample(K,
                  rows="global"), each rank feeding its shard with row_offset = its first row); the one-rank
                  comparison uses the local set_fvp_subsample(K) on all rows, and the ranks' Fisher feeds, concatenated
                  in rank order, must be X[::K], actions[::K], old[::K] and advant[::K] of the whole feed bit for bit
Checks: ranks bitwise identical (theta, stepdir, the update's stats); Hv and theta within 1e-5 of one rank holding
all rows; the same cg_iters, k and reverted as that rank.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DIMS = {"c3": (128, [64, 64], 18), "c4": (128, [256, 256], 18), "c5": (376, [1024, 1024], 17),
        "g17": (17, [64, 64], 6)}
GAUSS_DIMS = {"g17": DIMS["g17"], "c4": (128, [256, 256], 17)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-allreduce", action="store_true")
    ap.add_argument("--dims", default="c3", choices=sorted(DIMS))
    ap.add_argument("--rows", type=int, default=40_000)
    ap.add_argument("--graphs", action="store_true")
    ap.add_argument("--dist", default="categorical", choices=["categorical", "gaussian"])
    ap.add_argument("--max-kl", type=float, default=0.01)
    ap.add_argument("--residual-tol", type=float, default=0.0)
    ap.add_argument("--adv-scale", type=float, default=1.0)
    ap.add_argument("--expect", default=None)
    ap.add_argument("--fvp-subsample", type=int, default=1)
    args = ap.parse_args()
    gauss = args.dist == "gaussian"
    if gauss != (args.dims == "g17") and args.dims != "c4":
        ap.error(f"--dims {args.dims} does not go with --dist {args.dist}")

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
    from trpo_amd import Engine, UpdateParams
    from trpo_amd._lib import VEC_STEPDIR, get_option, set_option
    from trpo_amd.dist import fisher_rows, init_engine_comm, shard_bounds
    from oracle import trpo_oracle as O
    n = args.rows
    if gauss:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        import gauss_ref as G
        obs, hidden, A = GAUSS_DIMS[args.dims]
        # theta_old = theta: the whole-update feed, the advantages given directly (standardised over all rows)
        spec, theta, gb = G.make_case((obs, hidden, A, n), seed=3, perturb=0.0)
        starts = (np.arange(n) % 173 == 0).astype(np.uint8)    # an uneven cut: the next multiple of 173 rows
        prm = UpdateParams(residual_tol=args.residual_tol, max_kl=args.max_kl)
        gadv = (gb.advant.astype(np.float64) * args.adv_scale).astype(np.float32)

        def new_engine(rows):
            return Engine(obs, hidden, A, max_rows=rows, device=dev, dist="gaussian")

        def feed(e, lo, hi, n_global=n, row_offset=None):
            e.set_flat(theta)
            e.set_batch_gaussian(gb.X[lo:hi], gb.actions[lo:hi], gadv[lo:hi], gb.old_mean[lo:hi], gb.old_logstd,
                                 n_global=n_global, row_offset=row_offset)
    else:
        obs, hidden, A = DIMS[args.dims]
        spec = O.PolicySpec(obs, hidden, A)
        d = O.synthetic_batch(spec, n, seed=3, episode_len=200)
        theta, starts = d["theta"], d["starts"]
        from_rewards = args.adv_scale == 1.0
        prm = UpdateParams(residual_tol=args.residual_tol, max_kl=args.max_kl, compute_advantages=from_rewards)
        cadv = (d["advant"] * args.adv_scale).astype(np.float32)     # standardised over all rows

        def new_engine(rows):
            return Engine(spec.obs_dim, spec.hidden, spec.n_actions, max_rows=rows, device=dev)

        def feed(e, lo, hi, n_global=n, row_offset=None):
            e.set_flat(theta)
            if not from_rewards:
                e.set_batch(d["X"][lo:hi], d["actions"][lo:hi], cadv[lo:hi], d["old_dist"][lo:hi], n_global=n_global,
                            row_offset=row_offset)
                return
            e.set_batch(d["X"][lo:hi], d["actions"][lo:hi], None, d["old_dist"][lo:hi], n_global=n_global,
                        row_offset=row_offset)
            e.set_rewards(d["rewards"][lo:hi], d["starts"][lo:hi])
            e.compute_advantages(0.95)
    lo, hi = shard_bounds(n, world, starts)[rank]
    assert 0 <= lo < hi <= n, f"rank {rank}: empty shard [{lo}, {hi})"
    e = new_engine(hi - lo)
    if args.host_allreduce:
        def ar(arr):
            dist.all_reduce(torch.from_numpy(arr))
        e.comm_set_host_allreduce(ar, rank, world)
    else:
        init_engine_comm(e, rank, world)
    K = args.fvp_subsample
    if K > 1:
        e.set_fvp_subsample(K, rows="global")
    feed(e, lo, hi, row_offset=lo if K > 1 else None)
    v = np.random.RandomState(1).standard_normal(spec.n_params).astype(np.float32)
    hv = e.fvp(v, 0.0)
    saved = get_option("graphs")
    set_option("graphs", 0)
    st = e.update(prm)
    th = e.get_flat()
    sd = e.get_vector(VEC_STEPDIR)
    replays = []
    if args.graphs:
        # graphs on: the 1st update with this key runs eagerly, the 2nd captures and launches,
        # the 3rd and 4th replay
        set_option("graphs", 1)
        for _ in range(4):
            e.set_flat(theta)
            stg = e.update(prm)
            replays.append((stg, e.get_flat()))
    set_option("graphs", saved)
    for i, (stg, thg) in enumerate(replays):
        assert np.array_equal(thg, th), f"rank {rank}: graph update {i} differs from eager"
        assert stg == st, f"rank {rank}: graph update {i} stats differ: {stg} vs {st}"
    # every rank must hold the same parameters; compare with a single-engine run on rank 0
    allth = [None] * world
    dist.all_gather_object(allth, (th, sd, st))
    fishers = [None] * world
    if K > 1:
        k_, ns, N_sub, phase = e.fvp_subsample_global
        assert (k_, N_sub) == (K, -(-n // K)) and (phase, ns) == fisher_rows(hi - lo, lo, K), (k_, ns, N_sub, phase)
        dist.all_gather_object(fishers, e.fvp_subsample_fetch())
    if rank == 0:
        for t, s_, st_ in allth[1:]:
            assert np.array_equal(t, allth[0][0]) and np.array_equal(s_, allth[0][1]), "ranks diverged"
            assert st_ == allth[0][2], f"ranks' stats diverged: {st_} vs {allth[0][2]}"
        e1 = new_engine(n)
        if K > 1:
            e1.set_fvp_subsample(K)
        feed(e1, 0, n)
        if K > 1:
            # the ranks' Fisher feeds in rank order are every K-th row of the whole feed (after the update: the
            # advantages are the standardised ones of all rows)
            whole = e1.fvp_subsample_fetch()
            if gauss:
                want = {"states": gb.X[::K], "actions": gb.actions[::K], "old": gb.old_mean[::K], "advant": gadv[::K]}
            else:
                want = {"states": d["X"][::K], "actions": d["actions"][::K], "old": d["old_dist"][::K],
                        "advant": whole["advant"] if from_rewards else cadv[::K]}
            for key, w_ in want.items():
                got = np.concatenate([f[key] for f in fishers])
                assert got.shape == w_.shape and np.array_equal(got, w_), f"Fisher feed: {key} is not [::{K}]"
                assert np.array_equal(whole[key], w_), f"one-rank Fisher feed: {key} is not [::{K}]"
        hv1 = e1.fvp(v, 0.0)
        st1 = e1.update(prm)
        th1 = e1.get_flat()
        r1 = np.linalg.norm(hv - hv1) / np.linalg.norm(hv1)
        r2 = np.linalg.norm(th - th1) / np.linalg.norm(th1)
        print(f"world={world} dims={args.dims} rows={n} FVP rel {r1:.2e} theta rel {r2:.2e} "
              f"k={st['k']}/{st1['k']} iters={st['cg_iters']}/{st1['cg_iters']} "
              f"reverted={st['reverted']}/{st1['reverted']} graph replays={len(replays)}", flush=True)
        assert r1 < 1e-5 and r2 < 1e-5 and st["k"] == st1["k"]
        assert st["cg_iters"] == st1["cg_iters"] and st["reverted"] == st1["reverted"]
        if args.expect:
            want = tuple(int(x) for x in args.expect.split(","))
            assert (st["cg_iters"], st["k"], st["reverted"]) == want, (st, want)
        if gauss:
            t1 = np.linalg.norm(hv[-A:] - hv1[-A:]) / np.linalg.norm(hv1[-A:])
            t2 = np.linalg.norm(th[-A:] - th1[-A:]) / np.linalg.norm(th1[-A:])
            sd1 = e1.get_vector(VEC_STEPDIR)
            t3 = np.linalg.norm(sd - sd1) / np.linalg.norm(sd1)     # theta hides the step behind theta_0
            t4 = np.linalg.norm(sd[-A:] - sd1[-A:]) / np.linalg.norm(sd1[-A:])
            print(f"dist=gaussian shards {shard_bounds(n, world, starts)} FVP rel {r1:.2e} theta rel {r2:.2e}; "
                  f"log-std tail: FVP rel {t1:.2e} theta rel {t2:.2e}; stepdir rel {t3:.2e} (tail {t4:.2e})", flush=True)
            assert t1 < 1e-5 and t2 < 1e-5 and t3 < 1e-5 and t4 < 1e-5
        print("MRANK OK", flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
