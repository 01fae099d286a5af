"""Python handle over the HIP TRPO update engine (``include/trpo_engine.h``).

Arrays may be numpy arrays (host; copied in/out) or torch-ROCm tensors on the
engine's GPU (device pointers; no host round trip).  Results come back as fresh
numpy arrays unless an ``out`` tensor is given — the reference's
"caller-owned numpy in, fresh numpy out" convention.
"""
from __future__ import annotations

import ctypes
import json
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import MEM_DEVICE, MEM_HOST, check, lib

__all__ = ["Engine", "UpdateParams", "ENVS", "env_info", "env_step_device", "CONT_ENVS", "cont_env_info",
           "cont_env_step_device"]

_ADV_KINDS = {"returns": _lib.ADV_RETURNS, "gae": _lib.ADV_GAE}
_DISTS = {"categorical": _lib.DIST_CATEGORICAL, "gaussian": _lib.DIST_GAUSSIAN}

# the built-in environments of rollout.hip: name -> TRPO_ENV_* id
ENVS = {"CartPole-v0": _lib.ENV_CARTPOLE_V0, "MountainCar-v0": _lib.ENV_MOUNTAINCAR_V0,
        "Acrobot-v1": _lib.ENV_ACROBOT_V1}


def _env_id(env) -> int:
    if isinstance(env, str):
        if env not in ENVS:
            raise ValueError(f"unknown environment {env!r}; built in: {sorted(ENVS)}")
        return ENVS[env]
    return int(env)


def env_info(env) -> dict:
    """The table of a built-in environment (a name of ENVS or a TRPO_ENV_* id): obs_dim, state_dim, n_actions,
    reset_draws, time_limit, name.  Host-only: needs no GPU."""
    info = _lib.EnvInfo()
    check(lib.trpo_env_info(_env_id(env), ctypes.byref(info)), "trpo_env_info")
    return {"obs_dim": info.obs_dim, "state_dim": info.state_dim, "n_actions": info.n_actions,
            "reset_draws": info.reset_draws, "time_limit": info.time_limit, "name": info.name.decode()}


# the continuous-action environments a Gaussian engine rolls out: name -> TRPO_CENV_* id
CONT_ENVS = {"Pendulum-v1": _lib.CENV_PENDULUM_V1,
             "MountainCarContinuous-v0": _lib.CENV_MOUNTAINCAR_CONTINUOUS_V0}


def _cont_env_id(env) -> int:
    if isinstance(env, str):
        if env not in CONT_ENVS:
            raise ValueError(f"unknown continuous environment {env!r}; built in: {sorted(CONT_ENVS)}")
        return CONT_ENVS[env]
    return int(env)


def cont_env_info(env) -> dict:
    """The table of a continuous-action environment (a name of CONT_ENVS or a TRPO_CENV_* id): obs_dim, state_dim,
    act_dim, reset_draws, time_limit, name.  Host-only: needs no GPU."""
    info = _lib.ContEnvInfo()
    check(lib.trpo_cont_env_info(_cont_env_id(env), ctypes.byref(info)), "trpo_cont_env_info")
    return {"obs_dim": info.obs_dim, "state_dim": info.state_dim, "act_dim": info.act_dim,
            "reset_draws": info.reset_draws, "time_limit": info.time_limit, "name": info.name.decode()}


def _is_torch(x) -> bool:
    mod = type(x).__module__
    return mod.startswith("torch")


class _Arg:
    """A (pointer, mem-kind) pair that keeps its backing array alive."""

    def __init__(self, x, dtype, shape=None, writable=False):
        if x is None:
            self.ptr, self.mem, self.obj = None, MEM_HOST, None
            return
        if _is_torch(x):
            import torch
            tdt = {np.float32: torch.float32, np.float64: torch.float64, np.int64: torch.int64,
                   np.uint8: torch.uint8}[dtype]
            if x.dtype != tdt or not x.is_contiguous():
                if writable:
                    raise TypeError(f"output tensor must be contiguous {tdt}")
                x = x.to(tdt).contiguous()
            if shape is not None and x.numel() != int(np.prod(shape)):
                raise ValueError(f"expected {int(np.prod(shape))} elements, got {x.numel()}")
            self.obj = x
            if x.is_cuda:
                self.ptr, self.mem = ctypes.c_void_p(x.data_ptr()), MEM_DEVICE
            else:
                self.ptr, self.mem = ctypes.c_void_p(x.data_ptr()), MEM_HOST
            return
        a = np.asarray(x)
        if a.dtype != dtype or not a.flags.c_contiguous:
            if writable:
                raise TypeError(f"output array must be C-contiguous {np.dtype(dtype)}")
            a = np.ascontiguousarray(a, dtype=dtype)
        if shape is not None and a.size != int(np.prod(shape)):
            raise ValueError(f"expected {int(np.prod(shape))} elements, got {a.size}")
        self.obj = a
        self.ptr, self.mem = a.ctypes.data_as(ctypes.c_void_p), MEM_HOST


class UpdateParams:
    """Defaults: trpo_inksci.py:17 config and utils.py:171-172,185."""

    def __init__(self, cg_iters=10, residual_tol=1e-10, cg_damping=0.1, max_kl=0.01,
                 compute_advantages=False, gamma=0.95):
        self.cg_iters = cg_iters
        self.residual_tol = residual_tol
        self.cg_damping = cg_damping
        self.max_kl = max_kl
        self.compute_advantages = compute_advantages
        self.gamma = gamma

    def to_c(self) -> _lib.UpdateParams:
        return _lib.UpdateParams(int(self.cg_iters), float(self.residual_tol), float(self.cg_damping),
                                 float(self.max_kl), int(bool(self.compute_advantages)), float(self.gamma))


class Engine:
    def __init__(self, obs_dim: int, hidden: Sequence[int], n_actions: int, max_rows: int,
                 device: int = 0, dist: str = "categorical"):
        """dist="categorical" is the reference's softmax policy over n_actions; dist="gaussian" a diagonal
        Gaussian over n_actions action dimensions (include/trpo_engine.h, TRPO_DIST_GAUSSIAN): its feed is
        set_batch_gaussian, its forward action_mean, its sampling act_gaussian."""
        if dist not in _DISTS:
            raise ValueError(f"Engine: dist must be one of {sorted(_DISTS)}, got {dist!r}")
        self.obs_dim = int(obs_dim)
        self.hidden = [int(h) for h in hidden]
        self.n_actions = int(n_actions)
        self.max_rows = int(max_rows)
        self.device = int(device)
        h = (ctypes.c_int * max(1, len(self.hidden)))(*self.hidden)
        handle = ctypes.c_void_p()
        if dist == "categorical":
            check(lib.trpo_create(ctypes.byref(handle), self.obs_dim, h, len(self.hidden), self.n_actions,
                                  self.max_rows, self.device), "trpo_create")
        else:
            check(lib.trpo_create_dist(ctypes.byref(handle), _DISTS[dist], self.obs_dim, h, len(self.hidden),
                                       self.n_actions, self.max_rows, self.device), "trpo_create_dist")
        self._h = handle
        self._gaussian = dist == "gaussian"
        self.num_params = int(lib.trpo_num_params(self._h))
        self.n = 0
        self.n_global = 0

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "_h", None):
            lib.trpo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def synchronize(self):
        check(lib.trpo_synchronize(self._h), "trpo_synchronize")

    @property
    def dist(self) -> str:
        """The policy's distribution family, as the engine reports it: "categorical" or "gaussian"."""
        d = ctypes.c_int(0)
        check(lib.trpo_get_dist(self._h, ctypes.byref(d)), "trpo_get_dist")
        return {v: k for k, v in _DISTS.items()}[d.value]

    @property
    def stream_handle(self) -> int:
        return int(lib.trpo_stream(self._h) or 0)

    # ------------------------------------------------------------------ comm
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = (ctypes.c_uint8 * 128)()
        check(lib.trpo_comm_unique_id(buf), "trpo_comm_unique_id")
        return bytes(buf)

    def comm_init(self, uid: bytes, rank: int, world: int):
        assert len(uid) == 128
        buf = (ctypes.c_uint8 * 128)(*uid)
        check(lib.trpo_comm_init(self._h, buf, int(rank), int(world)), "trpo_comm_init")

    def comm_set_host_allreduce(self, fn, rank: int, world: int):
        """Test transport: fn(numpy_array) must sum the array across ranks in place."""
        def cb(ptr, count, dtype, _ctx):
            try:
                ct = ctypes.c_double if dtype == _lib.F64 else ctypes.c_float
                arr = np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ct)), shape=(count,))
                fn(arr)
                return 0
            except Exception:   # pragma: no cover
                return 1
        self._host_ar = _lib.ALLREDUCE_CB(cb)   # keep alive
        check(lib.trpo_comm_set_host_allreduce(self._h, self._host_ar, None, int(rank), int(world)),
              "trpo_comm_set_host_allreduce")

    def comm_info(self) -> dict:
        """What carries the all-reduces: transport ("none" / "rccl" / "host"), rank, world, the RCCL
        communicator's rank count / user rank / device, this engine's HIP device and its PCI bus id."""
        ci = _lib.CommInfo()
        check(lib.trpo_comm_info(self._h, ctypes.byref(ci)), "trpo_comm_info")
        return {"transport": ("none", "rccl", "host")[ci.transport], "rank": ci.rank, "world": ci.world,
                "comm_count": ci.comm_count, "comm_rank": ci.comm_rank, "comm_device": ci.comm_device,
                "device": ci.device, "pci_bus_id": ci.pci_bus_id.decode()}

    # ------------------------------------------------------------------ params
    def _out(self, out, dtype, n):
        if out is None:
            arr = np.empty(n, dtype)
            return arr, _Arg(arr, dtype, writable=True)
        return out, _Arg(out, dtype, shape=(n,), writable=True)

    def set_flat(self, theta):
        a = _Arg(theta, np.float32, (self.num_params,))
        check(lib.trpo_set_flat(self._h, a.ptr, a.mem), "trpo_set_flat")

    def get_flat(self, out=None):
        res, a = self._out(out, np.float32, self.num_params)
        check(lib.trpo_get_flat(self._h, a.ptr, a.mem), "trpo_get_flat")
        return res

    def get_vector(self, which: int, out=None):
        res, a = self._out(out, np.float32, self.num_params)
        check(lib.trpo_get_vector(self._h, int(which), a.ptr, a.mem), "trpo_get_vector")
        return res

    # ------------------------------------------------------------------ feed
    def set_batch(self, states, actions, advant, old_dist, n_global: Optional[int] = None,
                  row_offset: Optional[int] = None):
        n = int(states.shape[0])
        if row_offset is not None:
            self.set_row_offset(row_offset)
        n_global = n if n_global is None else int(n_global)
        s = _Arg(states, np.float32, (n, self.obs_dim))
        a = _Arg(actions, np.int64, (n,))
        adv = _Arg(advant, np.float32, (n,)) if advant is not None else _Arg(None, np.float32)
        o = _Arg(old_dist, np.float32, (n, self.n_actions))
        mems = {x.mem for x in (s, a, o) if x.ptr is not None} | ({adv.mem} if adv.ptr is not None else set())
        if len(mems) != 1:
            raise ValueError("set_batch: pass all host arrays or all device tensors")
        check(lib.trpo_set_batch(self._h, n, n_global, s.ptr, a.ptr, adv.ptr, o.ptr, mems.pop()),
              "trpo_set_batch")
        self.n, self.n_global = n, n_global
        self._tail_ptr = None

    def set_batch_gaussian(self, states, actions, advant, old_mean, old_logstd, n_global: Optional[int] = None,
                           row_offset: Optional[int] = None):
        """The Gaussian engine's feed: states [n, obs_dim], actions [n, A], advant [n] (or None), old_mean [n, A]
        and old_logstd [A], float32; all host arrays or all device tensors."""
        n = int(states.shape[0])
        if row_offset is not None:
            self.set_row_offset(row_offset)
        n_global = n if n_global is None else int(n_global)
        A = self.n_actions
        s = _Arg(states, np.float32, (n, self.obs_dim))
        a = _Arg(actions, np.float32, (n, A))
        adv = _Arg(advant, np.float32, (n,)) if advant is not None else _Arg(None, np.float32)
        m = _Arg(old_mean, np.float32, (n, A))
        ls = _Arg(old_logstd, np.float32, (A,))
        mems = {x.mem for x in (s, a, m, ls, adv) if x.ptr is not None}
        if len(mems) != 1:
            raise ValueError("set_batch_gaussian: pass all host arrays or all device tensors")
        check(lib.trpo_set_batch_gaussian(self._h, n, n_global, s.ptr, a.ptr, adv.ptr, m.ptr, ls.ptr, mems.pop()),
              "trpo_set_batch_gaussian")
        self.n, self.n_global = n, n_global
        self._tail_ptr = None

    def set_rewards(self, rewards, episode_starts, baseline=None):
        n = self.n
        r = _Arg(rewards, np.float64, (n,))
        st = _Arg(np.asarray(episode_starts).astype(np.uint8) if not _is_torch(episode_starts)
                  else episode_starts, np.uint8, (n,))
        b = _Arg(baseline, np.float64, (n,)) if baseline is not None else _Arg(None, np.float64)
        check(lib.trpo_set_rewards(self._h, r.ptr, st.ptr, b.ptr, r.mem), "trpo_set_rewards")
        self._tail_ptr = None

    def set_baseline(self, baseline):
        """The VF.predict baselines of the current feed (trpo_inksci.py:103), f64 [n]."""
        b = _Arg(baseline, np.float64, (self.n,))
        check(lib.trpo_set_baseline(self._h, b.ptr, b.mem), "trpo_set_baseline")

    def set_advantage_estimator(self, kind: str = "returns", lam: float = 1.0):
        """What compute_advantages / update(compute_advantages=True) standardise: "returns" (the
        reference's returns - baseline, the default) or "gae" (GAE(lambda), 0 <= lam <= 1, with the feed's
        baseline as V).  Engine state: it holds across feeds until set again."""
        if kind not in _ADV_KINDS:
            raise ValueError(f"set_advantage_estimator: kind must be one of {sorted(_ADV_KINDS)}, got {kind!r}")
        check(lib.trpo_set_advantage_estimator(self._h, _ADV_KINDS[kind], float(lam)),
              "trpo_set_advantage_estimator")

    @property
    def advantage_estimator(self):
        """(kind, lam) in force: ("returns", 1.0) unless set_advantage_estimator chose otherwise."""
        kind, lam = ctypes.c_int(0), ctypes.c_double(0.0)
        check(lib.trpo_get_advantage_estimator(self._h, ctypes.byref(kind), ctypes.byref(lam)),
              "trpo_get_advantage_estimator")
        return {v: k for k, v in _ADV_KINDS.items()}[kind.value], lam.value

    def set_tail_values(self, tail_values):
        """V(s_T) of the current feed's cut-off paths for GAE, f64 [n], read only at path-end rows; None
        clears them (as set_batch, set_rewards and rollout_to_batch do)."""
        t = _Arg(tail_values, np.float64, (self.n,)) if tail_values is not None else _Arg(None, np.float64)
        check(lib.trpo_set_tail_values(self._h, t.ptr, t.mem), "trpo_set_tail_values")

    def feed_view(self) -> "_lib.FeedView":
        """Device pointers into the current feed (synchronises the engine stream)."""
        v = _lib.FeedView()
        check(lib.trpo_get_feed_view(self._h, ctypes.byref(v)), "trpo_get_feed_view")
        return v

    def set_baseline_in_place(self):
        """Mark the feed's own baseline buffer (written through feed_view().baseline) as set."""
        v = self.feed_view()
        check(lib.trpo_set_baseline(self._h, v.baseline, MEM_DEVICE), "trpo_set_baseline")

    def explained_variance(self) -> float:
        """explained_variance(baseline, returns) (utils.py:208-211) over the feed, on the device."""
        out = ctypes.c_double(0.0)
        check(lib.trpo_explained_variance(self._h, ctypes.byref(out)), "trpo_explained_variance")
        return out.value

    def compute_advantages_device(self, gamma: float, returns_out=None, advant_out=None):
        """trpo_inksci.py:102-117 on the device; optional device/host outputs (f64 [n])."""
        r = _Arg(returns_out, np.float64, (self.n,), writable=True) if returns_out is not None else _Arg(None, np.float64)
        a = _Arg(advant_out, np.float64, (self.n,), writable=True) if advant_out is not None else _Arg(None, np.float64)
        mem = r.mem if r.ptr is not None else (a.mem if a.ptr is not None else MEM_HOST)
        check(lib.trpo_compute_advantages(self._h, float(gamma), r.ptr, a.ptr, mem), "trpo_compute_advantages")

    def compute_advantages(self, gamma: float = 0.95):
        ret = np.empty(self.n, np.float64)
        adv = np.empty(self.n, np.float64)
        check(lib.trpo_compute_advantages(self._h, float(gamma), ret.ctypes.data_as(ctypes.c_void_p),
                                          adv.ctypes.data_as(ctypes.c_void_p), MEM_HOST),
              "trpo_compute_advantages")
        return ret, adv

    def standardize(self, adv, n_global: Optional[int] = None, adv32_out=None):
        """trpo_inksci.py:115-117 on the device, summed over the engine's ranks: adv (f64 [n]) is
        standardised in place (a numpy array is updated too); returns adv."""
        return _standardize(self._h, adv, n_global, adv32_out)

    # ------------------------------------------------------------------ graph outputs
    def losses(self):
        out = (ctypes.c_float * 3)()
        check(lib.trpo_losses(self._h, out), "trpo_losses")
        return np.array(out[:], np.float32)

    def eval_losses(self, theta):
        t = _Arg(theta, np.float32, (self.num_params,))
        out = (ctypes.c_float * 3)()
        check(lib.trpo_eval_losses(self._h, t.ptr, out, t.mem), "trpo_eval_losses")
        return np.array(out[:], np.float32)

    def action_dist(self, out=None):
        """session.run(action_dist): the policy's softmax at the current parameters, [n, A]."""
        if out is None:
            res = np.empty((self.n, self.n_actions), np.float32)
            a = _Arg(res, np.float32, writable=True)
        else:
            res, a = out, _Arg(out, np.float32, shape=(self.n, self.n_actions), writable=True)
        check(lib.trpo_action_dist(self._h, a.ptr, a.mem), "trpo_action_dist")
        return res

    def action_mean(self):
        """The Gaussian policy forward at the current parameters over the feed: (mean f32 [n, A], logstd f32 [A])."""
        mean = np.empty((self.n, self.n_actions), np.float32)
        logstd = np.empty(self.n_actions, np.float32)
        check(lib.trpo_action_mean(self._h, mean.ctypes.data_as(ctypes.c_void_p),
                                   logstd.ctypes.data_as(ctypes.c_void_p), MEM_HOST), "trpo_action_mean")
        return mean, logstd

    def policy_grad(self, out=None):
        res, a = self._out(out, np.float32, self.num_params)
        check(lib.trpo_policy_grad(self._h, a.ptr, a.mem), "trpo_policy_grad")
        return res

    def fvp(self, v, damping: float = 0.1, out=None):
        vi = _Arg(v, np.float32, (self.num_params,))
        res, a = self._out(out, np.float32, self.num_params)
        if vi.mem != a.mem:
            raise ValueError("fvp: v and out must live in the same memory")
        check(lib.trpo_fvp(self._h, vi.ptr, a.ptr, float(damping), vi.mem), "trpo_fvp")
        return res

    def set_fvp_subsample(self, k: int, rows: str = "local"):
        """Evaluate every Fisher-vector product (fvp, cg, and the CG and shs products inside update) on rows
        0, k, 2k, ... of the feed, F_sub v + damping v; everything else stays on all rows.  k = 1 (the default)
        is the plain engine.  rows="local" is single-process only; rows="global" takes the stride over global row
        indices (set_row_offset, n_global) and works across ranks (include/trpo_engine.h)."""
        if rows == "local":
            check(lib.trpo_set_fvp_subsample(self._h, int(k)), "trpo_set_fvp_subsample")
        elif rows == "global":
            check(lib.trpo_set_fvp_subsample_global(self._h, int(k)), "trpo_set_fvp_subsample_global")
        else:
            raise ValueError(f"set_fvp_subsample: rows must be 'local' or 'global', got {rows!r}")

    def set_row_offset(self, row0: int):
        """The global index of the first row of the feeds that follow (default 0); read only by
        set_fvp_subsample(k, rows="global")."""
        check(lib.trpo_set_row_offset(self._h, int(row0)), "trpo_set_row_offset")

    @property
    def fvp_subsample(self):
        """(k, n_sub): the stride in force and this engine's Fisher rows of the current feed, ceil(n / k) in the
        local mode."""
        k, ns = ctypes.c_int(0), ctypes.c_int64(0)
        check(lib.trpo_get_fvp_subsample(self._h, ctypes.byref(k), ctypes.byref(ns)), "trpo_get_fvp_subsample")
        return k.value, ns.value

    @property
    def fvp_subsample_global(self):
        """(k, n_sub_r, N_sub, phase) in the global mode (trpo_amd.dist.fisher_rows), None in the local one."""
        g, N, ph = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int64(0)
        check(lib.trpo_get_fvp_subsample_global(self._h, ctypes.byref(g), ctypes.byref(N), ctypes.byref(ph), None),
              "trpo_get_fvp_subsample_global")
        if not g.value:
            return None
        k, ns = self.fvp_subsample
        return k, ns, N.value, ph.value

    def fvp_subsample_fetch(self) -> dict:
        """The Fisher feed as the engine holds it (host copies, unpadded): states, actions (int64 [n_sub], or
        float32 [n_sub, A] on a Gaussian engine), old (old_dist / old_mean) and advant.  For tests of the gather."""
        _, ns = self.fvp_subsample
        A = self.n_actions
        states = np.empty((ns, self.obs_dim), np.float32)
        old = np.empty((ns, A), np.float32)
        adv = np.empty(ns, np.float32)
        act = np.empty((ns, A), np.float32) if self._gaussian else np.empty(ns, np.int32)
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        check(lib.trpo_fvp_subsample_fetch(self._h, ptr(states), ptr(act), ptr(old), ptr(adv), MEM_HOST),
              "trpo_fvp_subsample_fetch")
        return {"states": states, "actions": act if self._gaussian else act.astype(np.int64), "old": old,
                "advant": adv}

    def cg(self, b, cg_iters=10, residual_tol=1e-10, damping=0.1, out=None):
        bi = _Arg(b, np.float32, (self.num_params,))
        res, a = self._out(out, np.float32, self.num_params)
        it = ctypes.c_int(0)
        check(lib.trpo_cg(self._h, bi.ptr, a.ptr, int(cg_iters), float(residual_tol), float(damping),
                          ctypes.byref(it), bi.mem), "trpo_cg")
        return res, it.value

    def linesearch(self, x, fullstep, expected_improve_rate: float):
        xi = _Arg(x, np.float32, (self.num_params,))
        fi = _Arg(fullstep, np.float32, (self.num_params,))
        out = np.empty(self.num_params, np.float32)
        k = ctypes.c_int(-1)
        if xi.mem != MEM_HOST or fi.mem != MEM_HOST:
            raise ValueError("linesearch: host arrays expected")
        check(lib.trpo_linesearch(self._h, xi.ptr, fi.ptr, float(expected_improve_rate),
                                  out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(k), MEM_HOST),
              "trpo_linesearch")
        return out, k.value

    # ------------------------------------------------------------------ the update
    def update(self, params: Optional[UpdateParams] = None, **kw) -> dict:
        prm = params or UpdateParams(**kw)
        cp = prm.to_c()
        st = _lib.UpdateStats()
        check(lib.trpo_update(self._h, ctypes.byref(cp), ctypes.byref(st)), "trpo_update")
        return st.as_dict()

    # ------------------------------------------------------------------ sampling / rollouts
    def act(self, states, uniforms=None, train: bool = True):
        """agent.act on a batch (trpo_inksci.py:76-87): (actions int64 [n], action_dist f32 [n, A])."""
        n = int(states.shape[0])
        s = _Arg(states, np.float32, (n, self.obs_dim))
        if s.mem == MEM_DEVICE:
            import torch
            acts = torch.empty(n, dtype=torch.int64, device=s.obj.device)
            dists = torch.empty((n, self.n_actions), dtype=torch.float32, device=s.obj.device)
        else:
            acts = np.empty(n, np.int64)
            dists = np.empty((n, self.n_actions), np.float32)
        u = _Arg(uniforms, np.float64, (n,)) if uniforms is not None else _Arg(None, np.float64)
        a = _Arg(acts, np.int64, writable=True)
        d = _Arg(dists, np.float32, writable=True)
        check(lib.trpo_act(self._h, s.ptr, n, u.ptr, int(bool(train)), a.ptr, d.ptr, s.mem), "trpo_act")
        return acts, dists

    def act_gaussian(self, states, normals=None, train: bool = True):
        """The Gaussian policy's act on a batch: (actions f32 [n, A], mean f32 [n, A], logstd f32 [A]) with
        actions = float32(mean + exp(logstd) * normals), normals f64 [n, A] standard normals from the caller
        (train=True), or actions = mean (train=False).  Host arrays."""
        n = int(states.shape[0])
        A = self.n_actions
        s = _Arg(states, np.float32, (n, self.obs_dim))
        xi = _Arg(normals, np.float64, (n, A)) if normals is not None else _Arg(None, np.float64)
        if s.mem != MEM_HOST or (xi.ptr is not None and xi.mem != MEM_HOST):
            raise ValueError("act_gaussian: host arrays expected")
        acts, mean = np.empty((n, A), np.float32), np.empty((n, A), np.float32)
        logstd = np.empty(A, np.float32)
        ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        check(lib.trpo_act_gaussian(self._h, s.ptr, n, xi.ptr, int(bool(train)), ptr(acts), ptr(mean), ptr(logstd),
                                    MEM_HOST), "trpo_act_gaussian")
        return acts, mean, logstd

    def rollout_cartpole(self, n_envs: int = 1, n_timesteps: int = 1000, max_pathlength: int = 1000,
                         seed: int = 1, train: bool = True, time_limit: int = 200,
                         reset_uniforms=None, action_uniforms=None, max_episodes_per_env: int = 0):
        """rollout(env, agent, max_pathlength, n_timesteps) (utils.py:18-45) over n_envs CartPole-v0
        instances on the GPU.  Returns (total steps, number of paths)."""
        p = _lib.RolloutParams()
        lib.trpo_default_rollout_params(ctypes.byref(p))
        return self._rollout("trpo_rollout_cartpole", (), env_info, _lib.ENV_CARTPOLE_V0, p, n_envs, n_timesteps,
                             max_pathlength, seed, train, time_limit, reset_uniforms, action_uniforms,
                             max_episodes_per_env)

    def rollout(self, env="CartPole-v0", n_envs: int = 1, n_timesteps: int = 1000, max_pathlength: int = 1000,
                seed: int = 1, train: bool = True, time_limit: Optional[int] = None,
                reset_uniforms=None, action_uniforms=None, max_episodes_per_env: int = 0):
        """rollout_cartpole for any built-in environment (a name of ENVS): the engine's obs_dim and n_actions
        must be the environment's.  time_limit=None is the environment's own; injected reset_uniforms are
        [n_envs, max_episodes_per_env, reset_draws].  Returns (total steps, number of paths)."""
        eid = _env_id(env)
        p = _lib.RolloutParams()
        check(lib.trpo_default_rollout_params_env(eid, ctypes.byref(p)), "trpo_default_rollout_params_env")
        return self._rollout("trpo_rollout_env", (eid,), env_info, eid, p, n_envs, n_timesteps, max_pathlength, seed,
                             train, time_limit, reset_uniforms, action_uniforms, max_episodes_per_env)

    def _rollout(self, fn, ids, info, eid, p, n_envs, n_timesteps, max_pathlength, seed, train, time_limit,
                 reset_uniforms, action_draws, max_episodes_per_env, after=()):
        """Stage a rollout's parameters into p (time_limit=None keeps p's) and call the entry point `fn` with the
        environment ids it takes (and, after p, a segment call's `resume`); `info` is the table lookup of eid's
        kind."""
        p.n_envs, p.n_timesteps, p.max_pathlength = int(n_envs), int(n_timesteps), int(max_pathlength)
        p.seed, p.train = int(seed) & ((1 << 64) - 1), int(bool(train))
        if time_limit is not None:
            p.time_limit = int(time_limit)
        keep = []
        if reset_uniforms is not None:
            ru = _Arg(reset_uniforms, np.float64)
            keep.append(ru)
            p.reset_uniforms = ru.ptr
            p.max_episodes_per_env = int(max_episodes_per_env)
            p.mem = ru.mem
        if action_draws is not None:
            ad = _Arg(action_draws, np.float64)
            keep.append(ad)
            p.action_uniforms = ad.ptr
            p.mem = ad.mem
        n, paths = ctypes.c_int64(0), ctypes.c_int64(0)
        check(getattr(lib, fn)(self._h, *ids, ctypes.byref(p), *after, ctypes.byref(n), ctypes.byref(paths)), fn)
        self.rollout_steps, self.rollout_paths = n.value, paths.value
        self.rollout_state_dim = info(eid)["state_dim"]
        self._tail_ptr = None
        return n.value, paths.value

    def rollout_fetch_states(self) -> np.ndarray:
        """The environment state every observation of the last rollout was made from, f64 [N, state_dim] (host);
        for CartPole-v0 and MountainCar-v0 it equals obs."""
        if getattr(self, "rollout_steps", None) is None:
            # no rollout yet: the engine reports the state error
            check(lib.trpo_rollout_fetch_states(self._h, None, MEM_HOST), "trpo_rollout_fetch_states")
        out = np.empty((self.rollout_steps, self.rollout_state_dim))
        check(lib.trpo_rollout_fetch_states(self._h, out.ctypes.data_as(ctypes.c_void_p), MEM_HOST),
              "trpo_rollout_fetch_states")
        return out

    def rollout_fetch(self, device=None):
        """The concatenated rollout as the reference's arrays: obs f64 [N,obs_dim] (and f32), actions i64,
        action_dists f32 [N,A], rewards f64, episode starts u8, cat_sample uniforms f64 (numpy, or torch
        tensors on `device` -- torch must have initialised its GPU context before the first engine was
        created: it bundles its own HIP runtime, which cannot start after ours)."""
        N = self.rollout_steps
        if device is not None:
            import torch
            mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)   # noqa: E731
            out = {"obs": mk((N, self.obs_dim), torch.float64), "obs32": mk((N, self.obs_dim), torch.float32),
                   "actions": mk(N, torch.int64),
                   "action_dists": mk((N, self.n_actions), torch.float32), "rewards": mk(N, torch.float64),
                   "starts": mk(N, torch.uint8), "uniforms": mk(N, torch.float64)}
            mem = MEM_DEVICE
            ptr = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
        else:
            out = {"obs": np.empty((N, self.obs_dim)), "obs32": np.empty((N, self.obs_dim), np.float32),
                   "actions": np.empty(N, np.int64),
                   "action_dists": np.empty((N, self.n_actions), np.float32), "rewards": np.empty(N),
                   "starts": np.empty(N, np.uint8), "uniforms": np.empty(N)}
            mem = MEM_HOST
            ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        check(lib.trpo_rollout_fetch(self._h, ptr(out["obs"]), ptr(out["obs32"]), ptr(out["actions"]),
                                     ptr(out["action_dists"]),
                                     ptr(out["rewards"]), ptr(out["starts"]), ptr(out["uniforms"]), mem),
              "trpo_rollout_fetch")
        return out

    def rollout_fetch_stats(self):
        """Rewards and path starts of the last rollout (host; for the print-out statistics)."""
        N = self.rollout_steps
        rew, st = np.empty(N), np.empty(N, np.uint8)
        if self._gaussian:
            check(lib.trpo_rollout_gaussian_fetch(self._h, None, None, None, None, None,
                                                  rew.ctypes.data_as(ctypes.c_void_p),
                                                  st.ctypes.data_as(ctypes.c_void_p), None, None, MEM_HOST),
                  "trpo_rollout_gaussian_fetch")
            return {"rewards": rew, "starts": st}
        check(lib.trpo_rollout_fetch(self._h, None, None, None, None, rew.ctypes.data_as(ctypes.c_void_p),
                                     st.ctypes.data_as(ctypes.c_void_p), None, MEM_HOST), "trpo_rollout_fetch")
        return {"rewards": rew, "starts": st}

    def rollout_fetch_ends(self):
        """How each path of the last rollout ended, in the order of the concatenated rollout (host arrays):
        truncated u8 [P] (1 = cut off by the time limit or max_pathlength, 0 = the environment terminated),
        final_obs f64 [P,obs_dim] (the observation of s_T, the state after the last step), final_dists f32 [P,A] (the policy at
        float32(s_T) for cut-off paths, zeros otherwise), lengths i64 [P] and end_rows i64 [P] (the row of
        each path's last step)."""
        return self._fetch_ends("trpo_rollout_fetch_ends", "final_dists")

    def _fetch_ends(self, fn, head_key):
        if getattr(self, "rollout_paths", None) is None:
            # no rollout yet: the engine reports the state error
            check(getattr(lib, fn)(self._h, None, None, None, None, None, MEM_HOST), fn)
        P = self.rollout_paths
        out = {"truncated": np.empty(P, np.uint8), "final_obs": np.empty((P, self.obs_dim)),
               head_key: np.empty((P, self.n_actions), np.float32), "lengths": np.empty(P, np.int64),
               "end_rows": np.empty(P, np.int64)}
        check(getattr(lib, fn)(self._h, *(a.ctypes.data_as(ctypes.c_void_p) for a in out.values()), MEM_HOST), fn)
        return out

    def tail_view(self) -> "_lib.TailView":
        """Device pointers to the path ends of the feed rollout_to_batch loaded and to the engine's tail
        buffer, which it zero-fills (synchronises the engine stream); any other feed is a state error."""
        v = _lib.TailView()
        self._tail_ptr = None
        check(lib.trpo_get_tail_view(self._h, ctypes.byref(v)), "trpo_get_tail_view")
        self._tail_ptr = v.tail
        return v

    def set_tail_values_in_place(self):
        """Mark the engine's own tail buffer, written through the last tail_view().tail, as the feed's tail
        values (a fresh tail_view() would zero it, so the pointer of the last one is kept)."""
        if getattr(self, "_tail_ptr", None) is None:
            raise _lib.EngineError("set_tail_values_in_place: no tail_view() was taken of this feed")
        check(lib.trpo_set_tail_values(self._h, self._tail_ptr, MEM_DEVICE), "trpo_set_tail_values")

    def tail_values(self) -> np.ndarray:
        """The feed's tail values as the GAE scan reads them, f64 [n]: zeros when none are set."""
        out = np.empty(self.n, np.float64)
        check(lib.trpo_get_tail_values(self._h, out.ctypes.data_as(ctypes.c_void_p), MEM_HOST),
              "trpo_get_tail_values")
        return out

    def rollout_to_batch(self, n_global: Optional[int] = None, row_offset: Optional[int] = None):
        """Load the rollout as the feed (states, actions, oldaction_dist, rewards, path starts) on the device."""
        N = self.rollout_steps
        if row_offset is not None:
            self.set_row_offset(row_offset)
        check(lib.trpo_rollout_to_batch(self._h, N if n_global is None else int(n_global)), "trpo_rollout_to_batch")
        self.n, self.n_global = N, (N if n_global is None else int(n_global))
        self._tail_ptr = None

    # ------------------------------------------------------------------ continuous-action rollouts (Gaussian engine)
    def rollout_gaussian(self, env="Pendulum-v1", n_envs: int = 1, n_timesteps: int = 1000,
                         max_pathlength: int = 1000, seed: int = 1, train: bool = True,
                         time_limit: Optional[int] = None, reset_uniforms=None, action_normals=None,
                         max_episodes_per_env: int = 0):
        """rollout() of a continuous-action environment (a name of CONT_ENVS) under this Gaussian engine's policy:
        the engine's obs_dim and n_actions must be the environment's obs_dim and act_dim.  train=True samples
        a = float32(mean + exp(logstd) * normal), train=False acts with the mean.  time_limit=None is the
        environment's own; injected reset_uniforms are [n_envs, max_episodes_per_env, reset_draws], injected
        action_normals [n_envs, ceil(n_timesteps/n_envs) + min(max_pathlength, time_limit) - 1, act_dim] standard
        normals.  Returns (total steps, number of paths)."""
        cid = _cont_env_id(env)
        p = _lib.RolloutParams()
        check(lib.trpo_default_rollout_params_cont(cid, ctypes.byref(p)), "trpo_default_rollout_params_cont")
        return self._rollout("trpo_rollout_gaussian", (cid,), cont_env_info, cid, p, n_envs, n_timesteps,
                             max_pathlength, seed, train, time_limit, reset_uniforms, action_normals,
                             max_episodes_per_env)

    def rollout_gaussian_fetch(self):
        """The concatenated Gaussian rollout (host arrays): obs f64 [N,obs_dim] and obs32, actions and means f32
        [N,A], logstd f32 [A] (what the rollout sampled with), rewards f64, starts u8, normals f64 [N,A] (zeros for
        train=False) and env_states f64 [N,state_dim]."""
        if getattr(self, "rollout_steps", None) is None:
            # no rollout yet: the engine reports the state error
            check(lib.trpo_rollout_gaussian_fetch(self._h, None, None, None, None, None, None, None, None, None,
                                                  MEM_HOST), "trpo_rollout_gaussian_fetch")
        N, A = self.rollout_steps, self.n_actions
        out = {"obs": np.empty((N, self.obs_dim)), "obs32": np.empty((N, self.obs_dim), np.float32),
               "actions": np.empty((N, A), np.float32), "means": np.empty((N, A), np.float32),
               "logstd": np.empty(A, np.float32), "rewards": np.empty(N), "starts": np.empty(N, np.uint8),
               "normals": np.empty((N, A)), "env_states": np.empty((N, getattr(self, "rollout_state_dim", 1)))}
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        check(lib.trpo_rollout_gaussian_fetch(self._h, *(ptr(out[k]) for k in (
            "obs", "obs32", "actions", "means", "logstd", "rewards", "starts", "normals", "env_states")), MEM_HOST),
            "trpo_rollout_gaussian_fetch")
        return out

    def rollout_gaussian_fetch_ends(self):
        """rollout_fetch_ends of a Gaussian rollout: truncated, final_obs, final_means f32 [P,A] (the policy's mean
        at float32(s_T) for cut-off paths, zeros otherwise), lengths, end_rows."""
        return self._fetch_ends("trpo_rollout_gaussian_fetch_ends", "final_means")

    def rollout_gaussian_to_batch(self, n_global: Optional[int] = None, row_offset: Optional[int] = None):
        """Load the Gaussian rollout as the feed (states, actions, old mean, the rollout's logstd, rewards, path
        starts) on the device."""
        N = getattr(self, "rollout_steps", None) or 0
        if row_offset is not None:
            self.set_row_offset(row_offset)
        ng = N if n_global is None else int(n_global)
        check(lib.trpo_rollout_gaussian_to_batch(self._h, ng), "trpo_rollout_gaussian_to_batch")
        self.n, self.n_global = N, ng
        self._tail_ptr = None

    # ------------------------------------------------------------------ fixed-horizon segment rollouts
    def rollout_segment(self, env="CartPole-v0", n_envs: int = 1, horizon: int = 1000, resume: bool = False,
                        seed: int = 1, train: bool = True, max_pathlength: int = 1000,
                        time_limit: Optional[int] = None, reset_uniforms=None, action_uniforms=None,
                        max_episodes_per_env: int = 0):
        """A segment rollout (include/trpo_engine.h, trpo_rollout_env_segment): each of n_envs environments takes
        exactly `horizon` steps, from a reset (resume=False) or from where the previous segment call left it
        (resume=True: the carry, rollout_carry()).  The fetch and to_batch calls of rollout() then work on it;
        rollout_segment_fetch() has its own columns.  Draws are indexed per call: injected action_uniforms are
        [n_envs, horizon], reset_uniforms [n_envs, max_episodes_per_env, reset_draws] with max_episodes_per_env >=
        horizon + (0 if resume else 1).  Returns (n_envs * horizon, number of paths)."""
        eid = _env_id(env)
        p = _lib.RolloutParams()
        check(lib.trpo_default_rollout_params_env(eid, ctypes.byref(p)), "trpo_default_rollout_params_env")
        return self._rollout("trpo_rollout_env_segment", (eid,), env_info, eid, p, n_envs, int(n_envs) * int(horizon),
                             max_pathlength, seed, train, time_limit, reset_uniforms, action_uniforms,
                             max_episodes_per_env, after=(int(bool(resume)),))

    def rollout_gaussian_segment(self, env="Pendulum-v1", n_envs: int = 1, horizon: int = 1000, resume: bool = False,
                                 seed: int = 1, train: bool = True, max_pathlength: int = 1000,
                                 time_limit: Optional[int] = None, reset_uniforms=None, action_normals=None,
                                 max_episodes_per_env: int = 0):
        """rollout_segment of a continuous-action environment under this Gaussian engine's policy; injected
        action_normals are [n_envs, horizon, act_dim]."""
        cid = _cont_env_id(env)
        p = _lib.RolloutParams()
        check(lib.trpo_default_rollout_params_cont(cid, ctypes.byref(p)), "trpo_default_rollout_params_cont")
        return self._rollout("trpo_rollout_gaussian_segment", (cid,), cont_env_info, cid, p, n_envs,
                             int(n_envs) * int(horizon), max_pathlength, seed, train, time_limit, reset_uniforms,
                             action_normals, max_episodes_per_env, after=(int(bool(resume)),))

    def rollout_segment_fetch(self) -> dict:
        """The segment columns of the last rollout, a segment rollout (host arrays): end_kind u8 [P] (0 terminated,
        1 cut by the time limit or max_pathlength, 2 cut by the segment), t0 i64 [P] (the episode step index of
        each path's first row), episode_returns f64 [P] (the episode's return at the path's end, earlier segments
        included) and step_index i64 [N]."""
        P, N = getattr(self, "rollout_paths", None) or 0, getattr(self, "rollout_steps", None) or 0
        out = {"end_kind": np.empty(P, np.uint8), "t0": np.empty(P, np.int64), "episode_returns": np.empty(P),
               "step_index": np.empty(N, np.int64)}
        check(lib.trpo_rollout_segment_fetch(self._h, *(a.ctypes.data_as(ctypes.c_void_p) for a in out.values()),
                                             MEM_HOST), "trpo_rollout_segment_fetch")
        return out

    def rollout_carry(self) -> dict:
        """The segment rollouts' carry (host copies): env (the id), n_envs, states f64 [n_envs, state_dim], t i64
        [n_envs] (steps taken in each environment's current episode) and returns f64 [n_envs] (its rewards so
        far).  A state error when there is none."""
        env, n = ctypes.c_int(0), ctypes.c_int(0)
        check(lib.trpo_rollout_carry_get(self._h, ctypes.byref(env), ctypes.byref(n), None, None, None, MEM_HOST),
              "trpo_rollout_carry_get")
        info = (cont_env_info if self._gaussian else env_info)(env.value)
        out = {"env": env.value, "n_envs": n.value, "states": np.empty((n.value, info["state_dim"])),
               "t": np.empty(n.value, np.int64), "returns": np.empty(n.value)}
        check(lib.trpo_rollout_carry_get(self._h, None, None, *(out[k].ctypes.data_as(ctypes.c_void_p)
                                                                 for k in ("states", "t", "returns")), MEM_HOST),
              "trpo_rollout_carry_get")
        return out

    def set_rollout_carry(self, env, states, t, returns):
        """Install a carry for rollout_segment(resume=True): states [n_envs, state_dim] f64, t [n_envs] and returns
        [n_envs] of `env`, a name (or id) of this engine's kind of environment."""
        eid = (_cont_env_id if self._gaussian else _env_id)(env)
        s = np.ascontiguousarray(states, np.float64)
        s = s.reshape(1, -1) if s.ndim == 1 else s
        tt, rr = np.ascontiguousarray(t, np.int64).reshape(-1), np.ascontiguousarray(returns, np.float64).reshape(-1)
        if not (s.ndim == 2 and s.shape[0] == tt.shape[0] == rr.shape[0]):
            raise ValueError("set_rollout_carry: states [n_envs, state_dim], t [n_envs] and returns [n_envs]")
        sd = (cont_env_info if self._gaussian else env_info)(eid)["state_dim"]
        if s.shape[1] != sd:
            raise ValueError(f"set_rollout_carry: states must have {sd} columns")
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
        check(lib.trpo_rollout_carry_set(self._h, eid, s.shape[0], ptr(s), ptr(tt), ptr(rr), MEM_HOST),
              "trpo_rollout_carry_set")

    def clear_rollout_carry(self):
        check(lib.trpo_rollout_carry_clear(self._h), "trpo_rollout_carry_clear")

    # ------------------------------------------------------------------ profiling
    def profile_enable(self, on: bool = True):
        check(lib.trpo_profile_enable(self._h, int(bool(on))), "trpo_profile_enable")

    def profile_reset(self):
        check(lib.trpo_profile_reset(self._h), "trpo_profile_reset")

    def profile_query(self) -> dict:
        need = lib.trpo_profile_query(self._h, None, 0)
        if need < 0:
            check(need, "trpo_profile_query")
        buf = ctypes.create_string_buffer(need + 1)
        lib.trpo_profile_query(self._h, buf, need + 1)
        return json.loads(buf.value.decode())


def cat_sample_device(prob_nk, uniforms) -> np.ndarray:
    """cat_sample (utils.py:95-105) on the current GPU with the uniforms given."""
    p = np.ascontiguousarray(prob_nk, np.float32)
    r = np.ascontiguousarray(uniforms, np.float64)
    assert p.ndim == 2 and r.shape == (p.shape[0],)
    out = np.empty(p.shape[0], np.int64)
    check(lib.trpo_cat_sample(p.ctypes.data_as(ctypes.c_void_p), p.shape[0], p.shape[1],
                              r.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), MEM_HOST),
          "trpo_cat_sample")
    return out


def cartpole_step_device(state, action):
    """One CartPole-v0 step per row on the current GPU: (state_out [n,4], reward [n], done [n] bool)."""
    s = np.ascontiguousarray(state, np.float64).reshape(-1, 4)
    a = np.ascontiguousarray(action, np.int64).reshape(-1)
    n = s.shape[0]
    so, rw, dn = np.empty((n, 4)), np.empty(n), np.empty(n, np.uint8)
    check(lib.trpo_cartpole_step(s.ctypes.data_as(ctypes.c_void_p), a.ctypes.data_as(ctypes.c_void_p), n,
                                 so.ctypes.data_as(ctypes.c_void_p), rw.ctypes.data_as(ctypes.c_void_p),
                                 dn.ctypes.data_as(ctypes.c_void_p), MEM_HOST), "trpo_cartpole_step")
    return so, rw, dn.astype(bool)


def env_step_device(env, state, action):
    """One step per row of a built-in environment on the current GPU: (state_out [n, state_dim], obs
    [n, obs_dim] of state_out, reward [n], done [n] bool; done is termination, not the time limit)."""
    eid = _env_id(env)
    info = env_info(eid)
    s = np.ascontiguousarray(state, np.float64).reshape(-1, info["state_dim"])
    a = np.ascontiguousarray(action, np.int64).reshape(-1)
    n = s.shape[0]
    if a.shape[0] != n:
        raise ValueError(f"{n} states but {a.shape[0]} actions")
    so, ob = np.empty((n, info["state_dim"])), np.empty((n, info["obs_dim"]))
    rw, dn = np.empty(n), np.empty(n, np.uint8)
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    check(lib.trpo_env_step(eid, ptr(s), ptr(a), n, ptr(so), ptr(ob), ptr(rw), ptr(dn), MEM_HOST), "trpo_env_step")
    return so, ob, rw, dn.astype(bool)


def cont_env_step_device(env, state, action):
    """env_step_device for a continuous-action environment: action [n, act_dim] float32 (the components the
    policy produced).  Returns (state_out [n, state_dim], obs [n, obs_dim], reward [n], done [n] bool)."""
    cid = _cont_env_id(env)
    info = cont_env_info(cid)
    s = np.ascontiguousarray(state, np.float64).reshape(-1, info["state_dim"])
    a = np.ascontiguousarray(action, np.float32).reshape(-1, info["act_dim"])
    n = s.shape[0]
    if a.shape[0] != n:
        raise ValueError(f"{n} states but {a.shape[0]} actions")
    so, ob = np.empty((n, info["state_dim"])), np.empty((n, info["obs_dim"]))
    rw, dn = np.empty(n), np.empty(n, np.uint8)
    ptr = lambda x: x.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    check(lib.trpo_cont_env_step(cid, ptr(s), ptr(a), n, ptr(so), ptr(ob), ptr(rw), ptr(dn), MEM_HOST),
          "trpo_cont_env_step")
    return so, ob, rw, dn.astype(bool)


def discount_device(x, gamma: float, episode_starts=None) -> np.ndarray:
    """Engine-free discounted-return scan (utils.py:14-16) on the current GPU."""
    xa = _Arg(x, np.float64)
    n = int(np.asarray(xa.obj).shape[0]) if xa.mem == MEM_HOST else int(xa.obj.numel())
    st = _Arg(None, np.uint8) if episode_starts is None else _Arg(
        np.asarray(episode_starts).astype(np.uint8) if not _is_torch(episode_starts) else episode_starts,
        np.uint8, (n,))
    if xa.mem == MEM_DEVICE:
        import torch
        out = torch.empty(n, dtype=torch.float64, device=xa.obj.device)
        oa = _Arg(out, np.float64, writable=True)
    else:
        out = np.empty(n, np.float64)
        oa = _Arg(out, np.float64, writable=True)
    check(lib.trpo_discount(xa.ptr, st.ptr, n, float(gamma), oa.ptr, xa.mem), "trpo_discount")
    return out


def gae_device(rewards, values, gamma: float, lam: float, episode_starts=None, tail_values=None):
    """Engine-free GAE(lambda) on the current GPU (include/trpo_engine.h, TRPO_ADV_GAE): returns
    (advantages, returns), f64 [n].  values=None is V = 0, episode_starts=None one path, tail_values=None
    zero bootstrap values.  Host arrays or device tensors (all of one kind)."""
    ra = _Arg(rewards, np.float64)
    dev = ra.mem == MEM_DEVICE
    n = int(ra.obj.numel()) if _is_torch(ra.obj) else int(ra.obj.shape[0])
    opt = lambda x: _Arg(x, np.float64, (n,)) if x is not None else _Arg(None, np.float64)   # noqa: E731
    va, ta = opt(values), opt(tail_values)
    st = _Arg(None, np.uint8) if episode_starts is None else _Arg(
        np.asarray(episode_starts).astype(np.uint8) if not _is_torch(episode_starts) else episode_starts,
        np.uint8, (n,))
    if any(x.ptr is not None and x.mem != ra.mem for x in (va, ta, st)):
        raise ValueError("gae_device: pass all host arrays or all device tensors")
    if dev:
        import torch
        adv = torch.empty(n, dtype=torch.float64, device=ra.obj.device)
        ret = torch.empty(n, dtype=torch.float64, device=ra.obj.device)
    else:
        adv, ret = np.empty(n, np.float64), np.empty(n, np.float64)
    aa, rr = _Arg(adv, np.float64, writable=True), _Arg(ret, np.float64, writable=True)
    check(lib.trpo_gae(ra.ptr, va.ptr, st.ptr, ta.ptr, n, float(gamma), float(lam), aa.ptr, rr.ptr, ra.mem),
          "trpo_gae")
    return adv, ret


def _standardize(handle, adv, n_global, adv32_out):
    if not _is_torch(adv):
        if not (isinstance(adv, np.ndarray) and adv.dtype == np.float64 and adv.flags.c_contiguous):
            raise TypeError("standardize: adv must be a C-contiguous float64 array (updated in place)")
    a = _Arg(adv, np.float64, writable=True)
    n = int(adv.numel()) if _is_torch(adv) else int(adv.size)
    o = _Arg(adv32_out, np.float32, (n,), writable=True) if adv32_out is not None else _Arg(None, np.float32)
    if o.ptr is not None and o.mem != a.mem:
        raise ValueError("standardize: adv and adv32_out must live in the same memory")
    check(lib.trpo_standardize(handle, a.ptr, n, n if n_global is None else int(n_global), o.ptr, a.mem),
          "trpo_standardize")
    return adv


def standardize_device(adv, adv32_out=None):
    """adv = (adv - mean)/(std + 1e-8) (trpo_inksci.py:115-117) in place on the current GPU, one
    process (engine-free)."""
    return _standardize(None, adv, None, adv32_out)


def cg_callback(f_Ax, b, cg_iters=10, residual_tol=1e-10):
    """conjugate_gradient(f_Ax, b) for an arbitrary host callable (utils.py:185-201):
    vectors, dots and axpys on the current GPU in b's dtype (float32 or float64).
    Returns (x, iterations)."""
    b = np.asarray(b)
    if b.dtype not in (np.float32, np.float64) or b.ndim != 1:
        raise TypeError("conjugate_gradient: b must be a 1-D float32/float64 array")
    b = np.ascontiguousarray(b)
    n = b.shape[0]
    dt = b.dtype
    err = []

    def cb(p_ptr, z_ptr, _ctx):
        try:
            p = np.ctypeslib.as_array(ctypes.cast(p_ptr, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dt))),
                                      shape=(n,)).copy()
            z = np.asarray(f_Ax(p), dtype=dt).reshape(n)
            np.ctypeslib.as_array(ctypes.cast(z_ptr, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dt))),
                                  shape=(n,))[:] = z
            return 0
        except Exception as exc:  # re-raised after the C call returns
            err.append(exc)
            return 1

    cfn = _lib.FAX_CB(cb)
    x = np.empty(n, dt)
    it = ctypes.c_int(0)
    rc = lib.trpo_cg_callback(cfn, None, b.ctypes.data_as(ctypes.c_void_p),
                              x.ctypes.data_as(ctypes.c_void_p), n,
                              _lib.F64 if dt == np.float64 else _lib.F32, int(cg_iters),
                              float(residual_tol), ctypes.byref(it))
    if err:
        raise err[0]
    check(rc, "trpo_cg_callback")
    return x, it.value
