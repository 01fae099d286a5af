"""learn() on fixed-horizon segments (config["segment_horizon"]) against a manual loop over the Engine / VF calls it
is made of, its refusal, the default path left as it was, and two ranks on one GPU.

The comparisons with the manual loop are exact: both run the same device calls with the same seeds.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T, N_ENVS, ITERS, SEED = 16, 3, 4, 7


def config_for(name, segment=True):
    from trpo_amd.agent import CONFIG
    cfg = dict(CONFIG, env=name, gae_lambda=0.95, bootstrap_truncated=True)
    if name == "Pendulum-v1":
        cfg["max_steps"] = 40      # an episode ends in the third segment; none finishes in the first two
    if segment:
        cfg["segment_horizon"] = T
    return cfg


def make_agent(name, cfg, max_rows=N_ENVS * T):
    from trpo_amd import TRPOAgent
    from trpo_amd.engine import CONT_ENVS, cont_env_info, env_info
    info = cont_env_info(name) if name in CONT_ENVS else env_info(name)
    A = info["act_dim"] if name in CONT_ENVS else info["n_actions"]
    return TRPOAgent(info["obs_dim"], A, hidden=(8,), max_rows=max_rows, config=cfg)


def manual_loop(agent, iters, segment):
    """learn()'s device calls, written out; returns per iteration (theta after the update or None, the
    rollout_segment_fetch dict or None, steps)"""
    from trpo_amd import UpdateParams
    from trpo_amd.agent import rollout_seed
    cfg, eng, vf, cont = agent.config, agent.engine, agent.vf, agent.continuous
    train, out = True, []
    for i in range(iters):
        kw = dict(n_envs=N_ENVS, max_pathlength=cfg["max_steps"], seed=rollout_seed(SEED, i, 0), train=train)
        if segment:
            roll = eng.rollout_gaussian_segment if cont else eng.rollout_segment
            n, _ = roll(agent.env, horizon=T, resume=i > 0, **kw)
        else:
            roll = eng.rollout_gaussian if cont else eng.rollout
            n, _ = roll(agent.env, n_timesteps=cfg["episodes_per_roll"], **kw)
        (eng.rollout_gaussian_to_batch if cont else eng.rollout_to_batch)(n_global=n, row_offset=0)
        vf.predict_engine(eng)
        vf.predict_tails_engine(eng)
        eng.compute_advantages_device(cfg["gamma"])
        sf = eng.rollout_segment_fetch() if segment else None
        theta = None
        if train:
            vf.fit_engine(eng)
            eng.update(UpdateParams(cg_iters=10, residual_tol=1e-10, cg_damping=cfg["cg_damping"],
                                    max_kl=cfg["max_kl"], compute_advantages=False))
            theta = eng.get_flat().copy()
            if eng.explained_variance() > 0.8:
                train = False
        out.append((theta, sf, n))
    return out


@pytest.mark.parametrize("name", ("CartPole-v0", "Pendulum-v1"))
def test_learn_against_a_manual_loop(gpu_available, name):
    cfg = config_for(name)
    agent = make_agent(name, cfg)
    hist = agent.learn(max_iterations=ITERS, n_envs=N_ENVS, seed=SEED, log=None, record=True)
    ref = manual_loop(make_agent(name, cfg), ITERS, True)
    assert len(hist) == ITERS
    mean, episodes, saw_none, saw_some = float("nan"), 0, False, False
    for i, (h, (theta, sf, n)) in enumerate(zip(hist, ref)):
        assert h["steps"] == n == N_ENVS * T == 48
        for k in sf:
            assert np.array_equal(h["segment"][k], sf[k]), (i, k)
        assert h["paths"] == len(sf["end_kind"])
        ends = h["ends"]
        for e_i in range(N_ENVS):      # the carry continues the path that ends on the environment's last row
            p = int(np.flatnonzero(ends["end_rows"] == e_i * T + T - 1)[0])
            cut = sf["end_kind"][p] == 2
            assert h["carry"]["t"][e_i] == (sf["t0"][p] + ends["lengths"][p] if cut else 0)
            assert h["carry"]["returns"][e_i] == (sf["episode_returns"][p] if cut else 0.0)
        if theta is None:
            assert "theta" not in h
        else:
            assert h["theta"].tobytes() == theta.tobytes(), i
        finished = sf["episode_returns"][sf["end_kind"] < 2]
        if len(finished):
            mean, saw_some = float(finished.mean()), True
        else:
            saw_none = True
        assert h["reward_mean"] == mean or (np.isnan(mean) and np.isnan(h["reward_mean"])), (i, h["reward_mean"], mean)
        if "episodes" in h:
            episodes += len(finished)
            assert h["episodes"] == episodes
    assert saw_some
    if name == "Pendulum-v1":
        # no episode finishes in the first two segments (NaN, no stop rule fires), three do in the third, none in
        # the fourth, which keeps the third's mean
        assert np.isnan(hist[0]["reward_mean"]) and np.isnan(hist[1]["reward_mean"]) and hist[0]["train"]
        assert list(hist[2]["segment"]["end_kind"]) == [1, 2] * N_ENVS
        assert hist[3]["reward_mean"] == hist[2]["reward_mean"] and saw_none
        assert list(hist[3]["segment"]["step_index"][:2]) == [8, 9]
    agent.engine.close()


def test_segments_need_gae_and_bootstrap(gpu_available):
    from trpo_amd.agent import CONFIG
    for extra in ({}, {"gae_lambda": 0.95}):
        with pytest.raises(ValueError, match="segment_horizon"):
            make_agent("CartPole-v0", dict(CONFIG, env="CartPole-v0", segment_horizon=T, **extra))
    with pytest.raises(ValueError, match="segment_horizon"):
        make_agent("CartPole-v0", dict(CONFIG, env="CartPole-v0", segment_horizon=0, gae_lambda=0.95,
                                       bootstrap_truncated=True))


def test_default_path_is_the_whole_episode_one(gpu_available):
    name = "CartPole-v0"
    cfg = dict(config_for(name, segment=False), episodes_per_roll=200)
    rows = N_ENVS * (-(-200 // N_ENVS) + 200 - 1)
    agent = make_agent(name, cfg, max_rows=rows)
    hist = agent.learn(max_iterations=2, n_envs=N_ENVS, seed=SEED, log=None, record=True)
    ref = manual_loop(make_agent(name, cfg, max_rows=rows), 2, False)
    for i, (h, (theta, _sf, n)) in enumerate(zip(hist, ref)):
        assert "segment" not in h and "carry" not in h
        assert h["steps"] == n and h["steps"] >= 200
        assert h["theta"].tobytes() == theta.tobytes(), i
        eps = np.add.reduceat(h["rollout"]["rewards"], np.flatnonzero(h["rollout"]["starts"]))
        assert h["reward_mean"] == float(eps.mean()) and h["paths"] == len(eps)
    from trpo_amd._lib import EngineError
    with pytest.raises(EngineError, match="rc=-4"):
        agent.engine.rollout_carry()          # the whole-episode path never makes a carry
    agent.engine.close()


def test_learn_two_ranks_on_segments(gpu_available):
    """learn() on 16-step segments as two ranks on one GPU (tools/mrank_learn.py --horizon): every rank holds
    4 * 16 rows in every iteration, theta and the VF stay bitwise equal across the ranks, the mean reward is the
    finished episodes', and iteration 0's update equals one engine's on the concatenated rows"""
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(root, "tools", "mrank_learn.py"),
           "--host-allreduce", "--iters", "3", "--gae", "0.95", "--bootstrap", "--horizon", "16"]
    res = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "MRANK LEARN OK" in res.stdout
    assert "rows per rank and iteration: [[64, 64], [64, 64], [64, 64]]" in res.stdout
    print("\n".join(res.stdout.strip().splitlines()[-3:]))
