"""``TRPOAgent`` — the update block of ``trpo_inksci.py:101-158`` on the HIP engine.

Two ways to run one policy update, both on the GPU:

* :meth:`TRPOAgent.update` — the fused path: one ``trpo_update`` C-ABI call does
  discount + standardise + pg + CG + step scaling + line search + revert on
  the device with no host round trip except the line search's accept flag.
* :meth:`TRPOAgent.update_stepwise` — the reference's block written line for
  line over the ``trpo_amd.utils`` surface (``conjugate_gradient``,
  ``linesearch``, ``GetFlat``/``SetFromFlat``), i.e. what
  ``trpo_inksci.py`` looks like once its TF session is replaced.

* :meth:`TRPOAgent.learn` — the whole loop of ``trpo_inksci.py:89-177`` on the
  device: rollouts of ``config["env"]`` (CartPole-v0 by default; ``rollout.hip``), VF baselines and fit
  (``vf.hip``), advantages, the update, explained variance and the reference's
  stop rules; only the print-out statistics come back to the host.

For the update methods, paths come in as the reference's dicts
(``utils.py:36-39``) with an optional ``"baseline"`` entry (zeros otherwise, as
``VF.predict`` returns before its first fit, ``utils.py:88-89``).

``config["gae_lambda"]`` (not in the reference) switches the advantages of all three
from ``discount(rewards) - baseline`` to GAE(lambda); paths may then carry a
``"tail_value"`` scalar, V(s_T) of a path that was cut off rather than terminated.
learn() keeps the environment's time limit as a termination, as the reference does, unless
``config["bootstrap_truncated"]`` is true (it needs ``gae_lambda``): the rollout then tells cut-off paths from
terminated ones, and from the VF's first fit on the scan bootstraps every cut-off path from V(s_T).
"""
from __future__ import annotations

import math
import time
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from ._lib import VEC_THETA_LS
from .engine import CONT_ENVS, Engine, UpdateParams, cont_env_info, env_info
from .vf import VF
from .utils import (EngineLoss, GetFlat, KLFirstFixedGVP, SetFromFlat, SurrogateLoss, conjugate_gradient,
                    flatgrad, linesearch)

CONFIG = {"max_steps": 1000, "episodes_per_roll": 1000, "gamma": 0.95, "cg_damping": 0.1,
          "max_kl": 0.01}   # trpo_inksci.py:17
# An optional "gae_lambda" key (absent or None here: the reference's discount(rewards) - baseline) selects
# GAE(lambda) advantages on the engine, with the VF's baseline as V.  With it, an optional
# "bootstrap_truncated": True makes learn() bootstrap paths cut off by the time limit or max_steps from V(s_T).
# Two more optional keys, neither in the reference: "env" (default "CartPole-v0"), the built-in environment
# learn() rolls out (trpo_amd.engine.ENVS), and "reward_target" (default the reference's 1.1*500), the mean
# episode reward above which learn() stops training.
# "env" may also name a continuous-action environment (trpo_amd.engine.CONT_ENVS: Pendulum-v1,
# MountainCarContinuous-v0): the agent then builds a diagonal-Gaussian engine, its second argument counts action
# dimensions, "init_logstd" (default 0.0) is the initial log-std of every one, the paths feed() / update() take are
# Gaussian paths (gaussian_paths_to_batch) and learn() rolls out with Engine.rollout_gaussian.
# "fvp_subsample": k (absent: 1) evaluates the Fisher-vector products of update(), update_stepwise() and learn() on
# every k-th row of the batch (Engine.set_fvp_subsample), as modular_rl and baselines' trpo_mpi do; the gradient,
# the losses and the line search stay on all rows.  Single-process: set_ranks(world > 1) then raises the engine's
# refusal, unless "fvp_subsample_rows": "global" (absent: "local") takes the stride over the rows' global indices
# (Engine.set_fvp_subsample(k, rows="global"), trpo_amd.dist.fisher_rows): learn() then hands each rank's rollout
# feed its row offset, and feed() / update() / update_stepwise() take one next to n_global.
# "segment_horizon": T (absent: whole episodes) makes learn() collect as baselines' traj_segment_generator does
# (Engine.rollout_segment): every environment takes exactly T steps per iteration and continues where the last
# iteration left it, through the train = False tail of the loop too; a batch is n_envs * T rows on every rank.  It
# needs "gae_lambda" and "bootstrap_truncated", which bootstrap the paths a segment cut from V(s_T).  The mean
# episode reward is then over the episodes that finished in the iteration, with their whole returns; it keeps its
# previous value when none did and is NaN before the first, so that no stop rule fires on it.
DEFAULT_ENV = "CartPole-v0"
REWARD_TARGET = 1.1 * 500   # trpo_inksci.py:135


class Session:
    """Stands in for the ``tf.Session`` the reference threads through utils (trpo_inksci.py:23)."""

    def __init__(self, engine: Engine, init_rng: Optional[np.random.RandomState] = None,
                 reinit_policy: bool = True, init_logstd: Optional[float] = None):
        self.engine = engine
        self.init_rng = init_rng or np.random.RandomState(1)
        self.reinit_policy = reinit_policy
        self.init_logstd = init_logstd     # a Gaussian engine's log-std tail; None: a categorical engine

    def draw_theta(self) -> np.ndarray:
        """A fresh initialisation of the engine's flat parameters: xavier_theta, then on a Gaussian engine the
        log-std tail at init_logstd."""
        e = self.engine
        theta = xavier_theta(e.obs_dim, e.hidden, e.n_actions, self.init_rng)
        if self.init_logstd is None:
            return theta
        return np.concatenate([theta, np.full(e.n_actions, self.init_logstd, np.float32)])

    def initialize_all_variables(self):
        """tf.initialize_all_variables() re-draws every variable, the policy included; the reference
        runs it again when the VF creates its net (utils.py:66), so its first update starts from a
        fresh initialisation.  reinit_policy=False keeps the current policy instead."""
        if self.reinit_policy:
            self.engine.set_flat(self.draw_theta())


def xavier_theta(obs_dim: int, hidden: Sequence[int], n_actions: int,
                 rng: Optional[np.random.RandomState] = None) -> np.ndarray:
    """Initial parameters: W ~ U(+-sqrt(6/(fan_in+fan_out))), b = 0 (prettytensor's
    fully_connected defaults, trpo_inksci.py:38-40), flat in var_list order."""
    rng = rng or np.random.RandomState(1)   # utils.py:7-9 seed
    widths = [obs_dim, *hidden, n_actions]
    parts = []
    for a, b in zip(widths[:-1], widths[1:]):
        lim = math.sqrt(6.0 / (a + b))
        parts.append(rng.uniform(-lim, lim, size=a * b))
        parts.append(np.zeros(b))
    return np.concatenate(parts).astype(np.float32)


def paths_to_batch(paths: List[Dict]) -> Dict[str, np.ndarray]:
    """Concatenate rollout paths (trpo_inksci.py:108-115) and mark episode starts."""
    starts = []
    for path in paths:
        s = np.zeros(len(path["rewards"]), np.uint8)
        s[0] = 1
        starts.append(s)
    obs = np.concatenate([np.asarray(p["obs"], np.float32).reshape(len(p["rewards"]), -1) for p in paths])
    out = {
        "state": obs,
        "action_dist": np.concatenate([np.asarray(p["action_dists"], np.float32).reshape(len(p["rewards"]), -1)
                                       for p in paths]),
        "action": np.concatenate([np.asarray(p["actions"], np.int64) for p in paths]),
        "rewards": np.concatenate([np.asarray(p["rewards"], np.float64) for p in paths]),
        "baseline": np.concatenate([np.asarray(p.get("baseline", np.zeros(len(p["rewards"]))), np.float64)
                                    for p in paths]),
        "starts": np.concatenate(starts),
    }
    if any("tail_value" in p for p in paths):
        # V(s_T) of a path that was cut off rather than terminated (GAE's bootstrap), at its last row
        tails = []
        for p in paths:
            t = np.zeros(len(p["rewards"]), np.float64)
            t[-1] = float(p.get("tail_value", 0.0))
            tails.append(t)
        out["tail_values"] = np.concatenate(tails)
    return out


def gaussian_paths_to_batch(paths: List[Dict]) -> Dict[str, np.ndarray]:
    """paths_to_batch for a Gaussian policy's paths: dicts with obs, actions [T][A] f32, action_means [T][A], logstd
    [A] (one vector for the whole batch: the old policy's), rewards and optional baseline / tail_value."""
    T = [len(p["rewards"]) for p in paths]
    logstd = np.asarray(paths[0]["logstd"], np.float32).reshape(-1)
    A = logstd.shape[0]
    for p in paths[1:]:
        if not np.array_equal(np.asarray(p["logstd"], np.float32).reshape(-1), logstd):
            raise ValueError("the paths of one batch must share their logstd (one old policy)")
    starts = []
    for t in T:
        s = np.zeros(t, np.uint8)
        s[0] = 1
        starts.append(s)
    out = {
        "state": np.concatenate([np.asarray(p["obs"], np.float32).reshape(t, -1) for p, t in zip(paths, T)]),
        "action": np.concatenate([np.asarray(p["actions"], np.float32).reshape(t, A) for p, t in zip(paths, T)]),
        "action_mean": np.concatenate([np.asarray(p["action_means"], np.float32).reshape(t, A)
                                       for p, t in zip(paths, T)]),
        "logstd": logstd,
        "rewards": np.concatenate([np.asarray(p["rewards"], np.float64) for p in paths]),
        "baseline": np.concatenate([np.asarray(p.get("baseline", np.zeros(t)), np.float64)
                                    for p, t in zip(paths, T)]),
        "starts": np.concatenate(starts),
    }
    if any("tail_value" in p for p in paths):
        tails = []
        for p, t in zip(paths, T):
            tv = np.zeros(t, np.float64)
            tv[-1] = float(p.get("tail_value", 0.0))
            tails.append(tv)
        out["tail_values"] = np.concatenate(tails)
    return out


def rollout_seed(seed: int, iteration: int, rank: int) -> int:
    """The Philox key of one rank's rollout at one iteration: ranks live 2^40 keys apart, so no rank
    ever draws another rank's stream at any reachable iteration count."""
    return (seed * 1000003 + iteration + (rank << 40)) & ((1 << 64) - 1)


class TRPOAgent:
    def __init__(self, obs_dim: int, n_actions: int, hidden: Sequence[int] = (64,), max_rows: int = 4096,
                 device: int = 0, theta: Optional[np.ndarray] = None, config: Optional[dict] = None,
                 reinit_policy: bool = True):
        self.config = dict(CONFIG if config is None else config)
        self.bootstrap_truncated = bool(self.config.get("bootstrap_truncated", False))
        if self.bootstrap_truncated and self.config.get("gae_lambda") is None:
            raise ValueError("config['bootstrap_truncated'] needs config['gae_lambda']: the reference's "
                             "returns - baseline estimator takes no tail values")
        self.segment_horizon = self.config.get("segment_horizon")
        if self.segment_horizon is not None:
            if int(self.segment_horizon) < 1:
                raise ValueError("config['segment_horizon'] must be >= 1")
            if self.config.get("gae_lambda") is None or not self.bootstrap_truncated:
                raise ValueError("config['segment_horizon'] needs config['gae_lambda'] and "
                                 "config['bootstrap_truncated']: without them a path the segment cut would be "
                                 "scored as a termination")
            self.segment_horizon = int(self.segment_horizon)
        self.env = self.config.get("env", DEFAULT_ENV)
        # a continuous-action environment (trpo_amd.engine.CONT_ENVS) makes the policy a diagonal Gaussian over
        # its act_dim action dimensions, which n_actions then counts; any other name is a discrete one's, as before
        self.continuous = isinstance(self.env, str) and self.env in CONT_ENVS
        if self.continuous:
            self.env_info = cont_env_info(self.env)
            self.env_info["n_actions"] = self.env_info["act_dim"]
        else:
            self.env_info = env_info(self.env)
        count = (lambda k: f"act_dim {k}") if self.continuous else (lambda k: f"{k} actions")
        # A config that names its environment must fit it.  Without the key the agent may be one that only
        # updates from given paths, of any shape; learn() then refuses the default environment if it does not fit.
        self.env_mismatch = None
        if (int(obs_dim), int(n_actions)) != (self.env_info["obs_dim"], self.env_info["n_actions"]):
            self.env_mismatch = (f"{self.env} has obs_dim {self.env_info['obs_dim']} and "
                                 f"{count(self.env_info['n_actions'])}; the agent was given obs_dim {obs_dim} "
                                 f"and {count(n_actions)}")
            if "env" in self.config:
                raise ValueError("config['env']: " + self.env_mismatch)
        self.engine = Engine(obs_dim, hidden, n_actions, max_rows, device,
                             dist="gaussian" if self.continuous else "categorical")
        self.session = Session(self.engine, reinit_policy=reinit_policy,
                               init_logstd=float(self.config.get("init_logstd", 0.0)) if self.continuous else None)
        self.gf = GetFlat(self.session)                          # trpo_inksci.py:71
        self.sff = SetFromFlat(self.session)                     # :72
        self.pg = flatgrad(SurrogateLoss(self.engine))           # :54
        self.fvp = flatgrad(KLFirstFixedGVP(self.engine))        # :56-70 (flatgrad(gvp))
        self.sff(self.session.draw_theta() if theta is None else theta)
        self.train = True                                        # :28
        self.end_count = 0                                       # :29
        self.vf = VF(self.session, max_rows=max_rows, device=device)   # :73
        self.rank, self.world, self.group = 0, 1, None
        if self.config.get("gae_lambda") is not None:
            self.engine.set_advantage_estimator("gae", self.config["gae_lambda"])
        if self.config.get("fvp_subsample") is not None:
            self.engine.set_fvp_subsample(int(self.config["fvp_subsample"]),
                                          rows=self.config.get("fvp_subsample_rows", "local"))

    def set_ranks(self, rank: int, world: int, group=None, host_allreduce: bool = False):
        """Run learn() as one of `world` ranks (one process per GPU, torch.distributed initialised by the
        caller; `group` a gloo group for the host-side scalars, None = the default group, which must then
        be gloo). Each rank rolls out its own share of the episode budget; the update's partial sums,
        the advantage standardisation, the explained variance and the VF gradient are summed over the
        ranks (the engine's and the VF's RCCL communicators, or with host_allreduce the stream-ordered
        host transport over gloo, for ranks that share a GPU). Policy and VF parameters start identical
        on every rank and stay so: every rank applies the same all-reduced step."""
        self.rank, self.world, self.group = int(rank), int(world), group
        if self.world <= 1:
            return
        import torch
        import torch.distributed as dist
        from .dist import broadcast_unique_id, init_engine_comm

        def ar(arr):
            dist.all_reduce(torch.from_numpy(arr), group=group)

        if host_allreduce:
            self.engine.comm_set_host_allreduce(ar, self.rank, self.world)
        else:
            init_engine_comm(self.engine, self.rank, self.world, group)

        def vf_comm(net):   # the VF net is created at its first fit (utils.py:83)
            if host_allreduce:
                net.comm_set_host_allreduce(ar, self.rank, self.world)
            else:
                net.comm_init(broadcast_unique_id(Engine.comm_unique_id, self.rank, group), self.rank, self.world)

        self.vf.on_create = vf_comm
        if self.vf.net is not None:   # set_ranks after a fit: the existing net's gradient is summed from now on
            vf_comm(self.vf.net)

    def _host_sum(self, *vals: float) -> np.ndarray:
        """Sum of host scalars over the ranks (gloo), float64; identity for one rank."""
        a = np.array(vals, np.float64)
        if self.world > 1:
            import torch
            import torch.distributed as dist
            t = torch.from_numpy(a)
            dist.all_reduce(t, group=self.group)
        return a

    def _rank_rows(self, n: int):
        """(n_global, row_offset) of this rank's n rows: one gloo all-gather of the ranks' row counts, the offset
        their exclusive prefix in rank order; one rank: (n, 0) and no collective."""
        if self.world <= 1:
            return int(n), 0
        import torch
        import torch.distributed as dist
        mine = torch.tensor([int(n)], dtype=torch.int64)
        every = [torch.zeros(1, dtype=torch.int64) for _ in range(self.world)]
        dist.all_gather(every, mine, group=self.group)
        counts = [int(t[0]) for t in every]
        return sum(counts), sum(counts[:self.rank])

    def feed(self, paths_or_batch, n_global: Optional[int] = None, row_offset: Optional[int] = None):
        """The feed dict of trpo_inksci.py:119-122 (+ rewards for :102-117).  row_offset: the global index of the
        batch's first row (config["fvp_subsample_rows"] = "global")."""
        if self.continuous:
            b = gaussian_paths_to_batch(paths_or_batch) if isinstance(paths_or_batch, list) else paths_or_batch
            self.engine.set_batch_gaussian(b["state"], b["action"], b.get("advant"), b["action_mean"], b["logstd"],
                                           n_global, row_offset=row_offset)
        else:
            b = paths_to_batch(paths_or_batch) if isinstance(paths_or_batch, list) else paths_or_batch
            self.engine.set_batch(b["state"], b["action"], b.get("advant"), b["action_dist"], n_global,
                                  row_offset=row_offset)
        if "rewards" in b:
            self.engine.set_rewards(b["rewards"], b["starts"], b.get("baseline"))
            if b.get("tail_values") is not None:
                self.engine.set_tail_values(b["tail_values"])
        return b

    def update(self, paths_or_batch, n_global: Optional[int] = None, cg_iters: int = 10,
               residual_tol: float = 1e-10, row_offset: Optional[int] = None) -> dict:
        """trpo_inksci.py:101-158 as one device call."""
        b = self.feed(paths_or_batch, n_global, row_offset)
        prm = UpdateParams(cg_iters=cg_iters, residual_tol=residual_tol,
                           cg_damping=self.config["cg_damping"], max_kl=self.config["max_kl"],
                           compute_advantages="rewards" in b, gamma=self.config["gamma"])
        return self.engine.update(prm)

    def update_stepwise(self, paths_or_batch, n_global: Optional[int] = None,
                        row_offset: Optional[int] = None) -> dict:
        """trpo_inksci.py:101-158 line for line over the utils surface."""
        b = self.feed(paths_or_batch, n_global, row_offset)
        if "rewards" in b:
            self.engine.compute_advantages(self.config["gamma"])      # :102-117
        fisher_vector_product = self.fvp.damped(self.config["cg_damping"])                   # :124-126
        loss = EngineLoss(self.engine)                                                        # :127-129
        thprev = self.gf()                                                     # :144
        g = self.pg()                                                          # :146
        stepdir = conjugate_gradient(fisher_vector_product, -g)                # :147
        shs = .5 * float(stepdir.dot(fisher_vector_product(stepdir)))         # :148
        lm = np.sqrt(shs / self.config["max_kl"])                              # :149
        fullstep = (stepdir / np.float32(lm)).astype(np.float32)               # :150
        neggdotstepdir = -g.dot(stepdir)                                       # :151
        theta = linesearch(loss, thprev, fullstep, float(neggdotstepdir) / lm)   # :153
        self.sff(theta)                                                        # :154
        surrafter, kloldnew, entropy = self.engine.losses()                    # :156
        reverted = bool(kloldnew > 2.0 * self.config["max_kl"])
        if reverted:                                                           # :157-158
            self.sff(thprev)
        return {"surr_after": float(surrafter), "kl_after": float(kloldnew), "ent_after": float(entropy),
                "reverted": reverted, "shs": shs, "lm": float(lm)}

    # ------------------------------------------------------------------ trpo_inksci.py:89-177
    def learn(self, max_iterations: Optional[int] = None, n_envs: int = 1, seed: int = 1,
              log: Optional[Callable[[str], None]] = print,
              draws: Optional[Callable[[int], tuple]] = None, record: bool = False) -> List[dict]:
        """The reference's learn() loop on config["env"] (CartPole-v0 unless set), device-resident.  Stop rules
        as trpo_inksci.py:131-141,172-175: training stops when the mean episode reward exceeds
        config["reward_target"] (the reference's 1.1*500 unless set) or the baseline explains > 0.8 of the
        returns' variance; the loop then keeps rolling out the argmax policy and ends after 100 such iterations; a NaN entropy ends it
        (the reference calls exit(-1)).  max_iterations bounds the loop (None: as the reference).
        draws(i) -> (reset_uniforms, action_uniforms, max_episodes_per_env) injects the random draws
        of iteration i's rollout (env.reset and cat_sample; tests), else a Philox stream per iteration.
        On a continuous-action environment the rollout calls are the Gaussian ones: draws(i)'s second entry is
        then the standard normals of the act, and the record's "rollout" / "ends" are the Gaussian fetch dicts.
        record=True also returns each iteration's parameters (theta_before, theta, theta_ls: the line search's
        point before a revert), rollout arrays, baselines, returns and
        standardised advantages, and how its paths ended ("ends", Engine.rollout_fetch_ends) with the
        feed's "tail_values" (zeros unless config["bootstrap_truncated"] set some) (host copies; parity tests).
        With config["segment_horizon"] = T every iteration is a segment rollout of n_envs * T rows that resumes the
        last one's environments (from a reset at iteration 0); draws(i)'s arrays are then those of
        Engine.rollout_segment, "reward_mean" is over the episodes that finished in the iteration (NaN before the
        first, the previous value when none did), "episodes" counts those, and record=True adds "segment"
        (Engine.rollout_segment_fetch) and "carry" (Engine.rollout_carry).
        Returns one stats dict per iteration."""
        cfg = self.config
        eng = self.engine
        if self.env_mismatch:
            raise ValueError("learn(): " + self.env_mismatch + "; name the environment in config['env']")
        reward_target = cfg.get("reward_target", REWARD_TARGET)
        # this rank's share of the timestep budget (trpo_inksci.py:96-100 over `world` ranks)
        n_timesteps = -(-cfg["episodes_per_roll"] // self.world)
        # worst case rows of one rollout: every environment overshoots its budget by one episode
        budget = -(-n_timesteps // n_envs)
        worst = n_envs * (budget + min(cfg["max_steps"], self.env_info["time_limit"]) - 1)
        seg = self.segment_horizon        # None: whole episodes, as the reference collects
        if seg is not None:
            worst = n_envs * seg          # a segment rollout has exactly that many rows, on every rank
            reward_mean = float("nan")    # until an episode has finished: no stop rule fires on it
        if worst > eng.max_rows:
            raise ValueError(f"learn(): a rollout of {n_envs} environments can reach {worst} steps, more than "
                             f"max_rows={eng.max_rows}; create the agent with max_rows >= {worst}")
        say = log or (lambda _s: None)
        start_time = time.time()
        i = 0
        numeptotal = 0
        history = []
        while max_iterations is None or i < max_iterations:
            say("Rollout")
            inj = {}
            if draws is not None:
                ru, au, me = draws(i)
                inj = {"reset_uniforms": ru, "action_normals" if self.continuous else "action_uniforms": au,
                       "max_episodes_per_env": me}
            if seg is not None:
                # every environment takes seg steps from where iteration i - 1 left it, train or not
                roll = eng.rollout_gaussian_segment if self.continuous else eng.rollout_segment
                n, n_paths = roll(self.env, n_envs=n_envs, horizon=seg, resume=i > 0,
                                  max_pathlength=cfg["max_steps"], seed=rollout_seed(seed, i, self.rank),
                                  train=self.train, **inj)
                n_global, row_offset = n * self.world, n * self.rank   # equal row counts: nothing to gather
            else:
                roll = eng.rollout_gaussian if self.continuous else eng.rollout
                n, n_paths = roll(self.env, n_envs=n_envs, n_timesteps=n_timesteps,
                                  max_pathlength=cfg["max_steps"],
                                  seed=rollout_seed(seed, i, self.rank),
                                  train=self.train, **inj)                               # :96-100
                n_global, row_offset = self._rank_rows(n)
            if self.continuous:
                eng.rollout_gaussian_to_batch(n_global=n_global, row_offset=row_offset)
            else:
                eng.rollout_to_batch(n_global=n_global, row_offset=row_offset)           # :108-122
            have_base = self.vf.predict_engine(eng)                                      # :103
            if record:
                rb = self.vf.net.predict(np.empty(n, np.float64)) if have_base else np.zeros(n)
            if self.bootstrap_truncated:
                self.vf.predict_tails_engine(eng)   # V(s_T) of the cut-off paths; none before the first fit
            if record:
                r_tail = eng.tail_values()
                r_ret, r_adv = np.empty(n), np.empty(n)
                eng.compute_advantages_device(cfg["gamma"], returns_out=r_ret, advant_out=r_adv)
            else:
                eng.compute_advantages_device(cfg["gamma"])                              # :104-117
            if seg is not None:
                # the episodes that finished in this segment (kinds 0 and 1), with their whole returns; an
                # iteration in which none finished on any rank keeps the previous mean
                sf = eng.rollout_segment_fetch()
                episoderewards = sf["episode_returns"][sf["end_kind"] < 2]
                ep_sum, ep_cnt = self._host_sum(episoderewards.sum(), len(episoderewards))
                if ep_cnt > 0:
                    reward_mean = ep_sum / ep_cnt if self.world > 1 else float(episoderewards.mean())
            else:
                ep = eng.rollout_fetch_stats()
                episoderewards = np.add.reduceat(ep["rewards"], np.flatnonzero(ep["starts"]))   # :131
                # the mean over every rank's episodes (one rank: episoderewards.mean())
                ep_sum, ep_cnt = self._host_sum(episoderewards.sum(), len(episoderewards))
                reward_mean = ep_sum / ep_cnt if self.world > 1 else float(episoderewards.mean())
            say("\n********** Iteration %i ************" % i)
            rec = {"iteration": i, "steps": n, "paths": n_paths, "train": self.train,
                   "reward_mean": float(reward_mean), "end_count": self.end_count}
            if record:
                fetch, fetch_ends = ((eng.rollout_gaussian_fetch, eng.rollout_gaussian_fetch_ends)
                                     if self.continuous else (eng.rollout_fetch, eng.rollout_fetch_ends))
                rec.update({"rollout": fetch(), "baseline": rb, "returns": r_ret, "advantages": r_adv,
                            "ends": fetch_ends(), "tail_values": r_tail})
                if seg is not None:
                    rec.update({"segment": sf, "carry": eng.rollout_carry()})
            if reward_mean > reward_target:                                              # :135-136
                self.train = False
            rec["train"] = self.train                    # whether this iteration updates the policy
            if not self.train:                                                           # :137-141
                say("Episode mean: %f" % reward_mean)
                self.end_count += 1
                rec["end_count"] = self.end_count
                if self.end_count > 100:
                    history.append(rec)
                    break
            if self.train:
                self.vf.fit_engine(eng)                                                  # :143
                if record:
                    rec["theta_before"] = eng.get_flat().copy()
                st = eng.update(UpdateParams(cg_iters=10, residual_tol=1e-10, cg_damping=cfg["cg_damping"],
                                             max_kl=cfg["max_kl"], compute_advantages=False))     # :144-158
                if record:
                    rec["theta"] = eng.get_flat().copy()
                    rec["theta_ls"] = eng.get_vector(VEC_THETA_LS).copy()   # the line search's point, before a revert
                    rec["vf_params"] = self.vf.net.get_params().copy()
                numeptotal += int(ep_cnt)
                exp = eng.explained_variance()                                           # :167
                stats = {
                    "Total number of episodes": numeptotal,
                    "Average sum of rewards per episode": reward_mean,
                    "Entropy": st["ent_after"],
                    "Baseline explained": exp,
                    "Time elapsed": "%.2f mins" % ((time.time() - start_time) / 60.0),
                    "KL between old and new distribution": st["kl_after"],
                    "Surrogate loss": st["surr_after"],
                }
                for k, v in stats.items():
                    say(k + ": " + " " * (40 - len(k)) + str(v))
                rec.update({"entropy": float(st["ent_after"]), "kl": float(st["kl_after"]),
                            "surr": float(st["surr_after"]), "explained_variance": float(exp),
                            "reverted": bool(st["reverted"]), "k": int(st["k"]), "episodes": numeptotal,
                            "cg_iters": int(st["cg_iters"]), "shs": float(st["shs"])})
                history.append(rec)
                if st["ent_after"] != st["ent_after"]:                                    # :172-173
                    rec["nan_exit"] = True
                    break
                if exp > 0.8:                                                            # :174-175
                    self.train = False
            else:
                history.append(rec)
            i += 1
        return history
