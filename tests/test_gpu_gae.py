"""GAE(lambda) on the device (gae.hip, TRPO_ADV_GAE) against the sequential reference tests/gae_ref.py:
the engine-free scan, the engine's advantages path, the update (eager, captured, replayed), the graph key,
the state rules, the communicator path and TRPOAgent.

Bars.  A: |A - A_ref| <= 1e-12 max|A_ref| elementwise.  Each step adds at most 3 roundings, weighted
geometrically: <= 3 u max|A| / (1 - gamma lambda) ~ 3e-14 max|A| at gamma lambda = 0.99.  R: rtol 1e-13, the
bar of test_discount_vs_golden.  That bar has no absolute part, so it can only be asked of returns that stay
away from zero: the sequential reference itself is off by ~u max|R| / (1 - gamma) in absolute terms, which
is an unbounded relative error where R_t crosses zero.  The cases held to it therefore draw non-negative
tail values (with r ~ U(0, 1) every term of R_t is then non-negative, as in the discount tests); signed
tail values, where R_t changes sign inside a path, are held to the max-norm form of the same bound,
|R - R_ref| <= 1e-12 max|R_ref| (test_gae_device_signed_tails).
"""
import numpy as np
import pytest

from conftest import golden, spec_of
from gae_ref import gae_ref
from oracle import trpo_oracle as O

pytestmark = pytest.mark.gpu

TILE = 2048          # gae.hip: kChunk (8) x kGaeThreads (256)
GAMMAS = (0.95, 0.99)
LAMBDAS = (0.0, 0.97, 1.0)
# 1 row; every row its own path; odd and small; one tile + 1; two tiles + 3 (a partial chunk); 257 block maps
# (pass 2 gives its first threads two each)
SHAPES = [(1, 0.0), (2, 1.0), (17, 0.3), (TILE + 1, 0.0), (2 * TILE + 3, 0.01), (256 * TILE + 1, 0.005)]
VARIANTS = ["values+tails", "values", "tails", "neither", "one_path"]


def _inputs(n, p_start, signed_tails=False):
    rng = np.random.RandomState(n)
    r = rng.uniform(0, 1, n)
    v = 10.0 * rng.standard_normal(n)
    starts = (rng.uniform(size=n) < p_start).astype(np.uint8)
    starts[0] = 1
    tails = 10.0 * rng.standard_normal(n)
    return r, v, starts, tails if signed_tails else np.abs(tails)


def _check_A(A, A_ref, what):
    scale = float(np.max(np.abs(A_ref)))
    err = float(np.max(np.abs(A - A_ref)))
    print(f"{what}: max|A - A_ref| = {err:.3e} = {err / max(scale, 1e-300):.3e} max|A_ref|")
    assert err <= 1e-12 * scale, what


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n,p_start", SHAPES)
def test_gae_device_vs_reference(gpu_available, n, p_start, variant):
    from trpo_amd.engine import gae_device
    r, v, starts, tails = _inputs(n, p_start)
    values = v if variant in ("values+tails", "values", "one_path") else None
    tail_values = tails if variant in ("values+tails", "tails", "one_path") else None
    st = None if variant == "one_path" else starts
    for gamma in GAMMAS:
        for lam in LAMBDAS:
            what = f"n={n} {variant} gamma={gamma} lambda={lam}"
            A_ref, R_ref, _ = gae_ref(r, values, gamma, lam, st, tail_values)
            A, R = gae_device(r, values, gamma, lam, st, tail_values)
            _check_A(A, A_ref, what)
            rel = float(np.max(np.abs(R - R_ref) / np.abs(R_ref)))
            print(f"{what}: max rel |R - R_ref| = {rel:.3e}")
            np.testing.assert_allclose(R, R_ref, rtol=1e-13, err_msg=what)
            if lam == 1.0 and tail_values is None:
                _check_A(A, R_ref - (0.0 if values is None else values), what + " vs R - V")


@pytest.mark.parametrize("n,p_start", [(2 * TILE + 3, 0.01), (256 * TILE + 1, 0.005)])
def test_gae_device_signed_tails(gpu_available, n, p_start):
    """Tail values of either sign: the returns cross zero inside paths, so both outputs are held to the
    max-norm bound (module docstring)."""
    from trpo_amd.engine import gae_device
    r, v, starts, tails = _inputs(n, p_start, signed_tails=True)
    for gamma, lam in ((0.95, 0.97), (0.99, 1.0)):
        A_ref, R_ref, _ = gae_ref(r, v, gamma, lam, starts, tails)
        A, R = gae_device(r, v, gamma, lam, starts, tails)
        _check_A(A, A_ref, f"n={n} signed tails gamma={gamma} lambda={lam}")
        assert np.max(np.abs(R - R_ref)) <= 1e-12 * np.max(np.abs(R_ref))


def test_utils_gae_and_optional_outputs(gpu_available):
    """utils.gae returns the advantages of gae_device; the C entry takes NULL for either output."""
    import ctypes
    from trpo_amd import _lib, utils
    from trpo_amd.engine import gae_device
    r, v, starts, tails = _inputs(5000, 0.01)
    A, R = gae_device(r, v, 0.99, 0.95, starts, tails)
    assert np.array_equal(utils.gae(r, v, 0.99, 0.95, starts, tails), A)
    assert np.array_equal(utils.gae(list(r), list(v), 0.99, 0.95, starts.astype(bool), tails), A)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    for want_adv in (True, False):
        out = np.empty(5000)
        rc = _lib.lib.trpo_gae(ptr(r), ptr(v), ptr(starts), ptr(tails), 5000, 0.99, 0.95,
                               ptr(out) if want_adv else None, None if want_adv else ptr(out), _lib.MEM_HOST)
        assert rc == 0 and np.array_equal(out, A if want_adv else R)
    with pytest.raises(_lib.EngineError, match="lambda"):
        gae_device(r, v, 0.99, 1.5, starts)


_DEVICE_SCRIPT = r"""
import sys, numpy as np, torch
torch.cuda.init()                      # torch's HIP runtime first (engine.py: rollout_fetch note)
sys.path.insert(0, sys.argv[1])
from trpo_amd import utils
from trpo_amd.engine import gae_device
n = 10_000
rng = np.random.RandomState(4)
r, v = rng.uniform(0, 1, n), 10.0 * rng.standard_normal(n)
starts = (rng.uniform(size=n) < 0.01).astype(np.uint8)
tails = np.abs(10.0 * rng.standard_normal(n))
A, R = gae_device(r, v, 0.99, 0.95, starts, tails)
dev = lambda a: torch.from_numpy(a).cuda()
At, Rt = gae_device(dev(r), dev(v), 0.99, 0.95, dev(starts), dev(tails))
assert At.is_cuda and Rt.is_cuda
assert np.array_equal(At.cpu().numpy(), A) and np.array_equal(Rt.cpu().numpy(), R)
assert np.array_equal(utils.gae(dev(r), None, 0.99, 0.95).cpu().numpy(), gae_device(r, None, 0.99, 0.95)[0])
print("DEVICE GAE OK")
"""


def test_gae_device_tensors(gpu_available):
    """mem = TRPO_MEM_DEVICE on torch-ROCm tensors (own process: torch initialises HIP first)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", _DEVICE_SCRIPT, root], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "DEVICE GAE OK" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]


# ---------------------------------------------------------------------------- the engine's advantages path
def _c3_engine():
    from trpo_amd import Engine
    d = golden("update_c3.npz")
    spec = spec_of(d)
    e = Engine(spec.obs_dim, spec.hidden, spec.n_actions, max_rows=d["X"].shape[0])
    e.set_flat(d["theta"])
    e.set_batch(d["X"], d["actions"], None, d["old_dist"])
    return e, d


def test_engine_advantages_under_gae(gpu_available):
    from trpo_amd.engine import gae_device
    e, d = _c3_engine()
    n = d["X"].shape[0]
    base = 0.5 * d["returns"] + np.random.RandomState(0).standard_normal(n)
    e.set_rewards(d["rewards"], d["starts"], base)
    e.set_advantage_estimator("gae", 0.97)
    assert e.advantage_estimator == ("gae", 0.97)
    ret, adv = e.compute_advantages(0.95)
    A_ref, R_ref, _ = gae_ref(d["rewards"], base, 0.95, 0.97, d["starts"])
    np.testing.assert_allclose(ret, R_ref, rtol=1e-13)
    np.testing.assert_allclose(adv, O.standardize(A_ref), rtol=1e-11, atol=1e-12)
    # the same scan and the same standardisation launches as the standalone entries: bitwise
    A_dev, R_dev = gae_device(d["rewards"], base, 0.95, 0.97, d["starts"])
    assert np.array_equal(ret, R_dev)
    assert np.array_equal(adv, e.standardize(A_dev.copy()))
    assert e.explained_variance() == pytest.approx(O.explained_variance(base, R_ref), abs=1e-10)
    # tail values reach the scan
    tails = np.abs(np.random.RandomState(1).standard_normal(n)) * 5.0
    e.set_tail_values(tails)
    ret_t, adv_t = e.compute_advantages(0.95)
    A_ref_t, R_ref_t, _ = gae_ref(d["rewards"], base, 0.95, 0.97, d["starts"], tails)
    np.testing.assert_allclose(ret_t, R_ref_t, rtol=1e-13)
    np.testing.assert_allclose(adv_t, O.standardize(A_ref_t), rtol=1e-11, atol=1e-12)
    assert not np.array_equal(ret_t, ret)
    e.close()


def test_default_estimator_untouched(gpu_available):
    e0, d = _c3_engine()
    assert e0.advantage_estimator == ("returns", 1.0)
    e0.set_rewards(d["rewards"], d["starts"])
    ret0, adv0 = e0.compute_advantages(0.95)
    e0.close()
    e1, _ = _c3_engine()
    e1.set_advantage_estimator("gae", 0.5)
    e1.set_advantage_estimator("returns")
    assert e1.advantage_estimator == ("returns", 1.0)
    e1.set_rewards(d["rewards"], d["starts"])
    ret1, adv1 = e1.compute_advantages(0.95)
    e1.close()
    assert np.array_equal(ret0, ret1) and np.array_equal(adv0, adv1)
    np.testing.assert_allclose(ret0, d["returns"], rtol=1e-13)
    np.testing.assert_allclose(adv0, d["advant"], rtol=1e-11, atol=1e-12)


def test_state_errors(gpu_available):
    from trpo_amd import UpdateParams
    from trpo_amd._lib import EngineError
    e, d = _c3_engine()
    n = d["X"].shape[0]
    tails = np.ones(n)
    e.set_rewards(d["rewards"], d["starts"])
    ret0, adv0 = e.compute_advantages(0.95)
    e.set_tail_values(tails)
    with pytest.raises(EngineError, match="tail values"):
        e.compute_advantages(0.95)
    with pytest.raises(EngineError, match="tail values"):
        e.update(UpdateParams(compute_advantages=True))
    e.set_tail_values(None)
    ret1, adv1 = e.compute_advantages(0.95)
    assert np.array_equal(ret1, ret0) and np.array_equal(adv1, adv0)
    # set_batch and set_rewards clear them
    e.set_tail_values(tails)
    e.set_batch(d["X"], d["actions"], None, d["old_dist"])
    e.set_rewards(d["rewards"], d["starts"])
    ret2, _ = e.compute_advantages(0.95)
    assert np.array_equal(ret2, ret0)
    e.set_advantage_estimator("gae", 0.9)
    retg, advg = e.compute_advantages(0.95)
    e.set_tail_values(tails)
    rett, _ = e.compute_advantages(0.95)
    assert not np.array_equal(rett, retg)
    e.set_rewards(d["rewards"], d["starts"])
    retc, advc = e.compute_advantages(0.95)
    assert np.array_equal(retc, retg) and np.array_equal(advc, advg)
    with pytest.raises(ValueError):
        e.set_advantage_estimator("td", 0.9)
    with pytest.raises(EngineError, match="lambda"):
        e.set_advantage_estimator("gae", 1.5)
    assert e.advantage_estimator == ("gae", 0.9)
    e.close()


# ---------------------------------------------------------------------------- the update
SPEC = O.PolicySpec(11, [64, 64], 3)
N_UPD = 3000
PRM = dict(residual_tol=0.0, compute_advantages=True)


@pytest.fixture(scope="module")
def upd_batch():
    d = dict(O.synthetic_batch(SPEC, N_UPD, seed=7))
    rng = np.random.RandomState(5)
    d["baseline"] = 0.5 * d["returns"] + rng.standard_normal(N_UPD)
    d["tails"] = np.abs(rng.standard_normal(N_UPD)) * 5.0
    return d


def _upd_engine(d, estimator=None, tails=False, comm=False, advant=None):
    from trpo_amd import Engine
    e = Engine(SPEC.obs_dim, SPEC.hidden, SPEC.n_actions, max_rows=N_UPD)
    if comm:
        e.comm_init(Engine.comm_unique_id(), 0, 1)
    if estimator:
        e.set_advantage_estimator(*estimator)
    e.set_flat(d["theta"])
    e.set_batch(d["X"], d["actions"], advant, d["old_dist"])
    e.set_rewards(d["rewards"], d["starts"], d["baseline"])
    if tails:
        e.set_tail_values(d["tails"])
    return e


def _one_update(e, d, **kw):
    from trpo_amd import UpdateParams
    e.set_flat(d["theta"])
    st = e.update(UpdateParams(**{**PRM, **kw}))
    return st, e.get_flat()


def _same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1])


def test_update_under_gae_bitwise(gpu_available, upd_batch):
    """The GAE update equals an update fed the standardised advantages of the standalone scan, and five
    consecutive updates from theta_0 (first-seen eager, capture, replays) equal each other."""
    from trpo_amd.engine import gae_device
    d = upd_batch
    e = _upd_engine(d, ("gae", 0.95))
    runs = [_one_update(e, d) for _ in range(5)]
    e.close()
    A_dev, _ = gae_device(d["rewards"], d["baseline"], 0.95, 0.95, d["starts"])
    fed = _upd_engine(d, advant=O.standardize(A_dev).astype(np.float32))
    ref = _one_update(fed, d, compute_advantages=False)
    fed.close()
    for i, run in enumerate(runs):
        assert _same(run, ref), f"update {i}: {run[0]} vs {ref[0]}"


def test_no_stale_graph_replay(gpu_available, upd_batch):
    """A captured update graph is never replayed after the estimator, lambda or the tail values change."""
    d = upd_batch
    fresh = {}
    for key, est, tails in (("returns", None, False), ("gae0.9", ("gae", 0.9), False),
                            ("gae0.5", ("gae", 0.5), False), ("gae0.9+tails", ("gae", 0.9), True)):
        f = _upd_engine(d, est, tails)
        fresh[key] = _one_update(f, d)
        f.close()
    assert not _same(fresh["returns"], fresh["gae0.9"]) and not _same(fresh["gae0.9"], fresh["gae0.5"])
    assert not _same(fresh["gae0.9"], fresh["gae0.9+tails"])
    e = _upd_engine(d)
    for _ in range(3):                                  # first-seen eager, capture, replay
        assert _same(_one_update(e, d), fresh["returns"])
    e.set_advantage_estimator("gae", 0.9)
    assert _same(_one_update(e, d), fresh["gae0.9"])
    e.set_advantage_estimator("returns")
    assert _same(_one_update(e, d), fresh["returns"])
    e.set_advantage_estimator("gae", 0.9)
    for _ in range(3):
        assert _same(_one_update(e, d), fresh["gae0.9"])
    e.set_advantage_estimator("gae", 0.5)               # lambda alone
    assert _same(_one_update(e, d), fresh["gae0.5"])
    e.set_advantage_estimator("gae", 0.9)
    for _ in range(3):
        assert _same(_one_update(e, d), fresh["gae0.9"])
    e.set_tail_values(d["tails"])
    for _ in range(3):
        assert _same(_one_update(e, d), fresh["gae0.9+tails"])
    e.set_tail_values(None)
    assert _same(_one_update(e, d), fresh["gae0.9"])
    e.close()


def test_rccl_world1_gae_update_bitwise(gpu_available, upd_batch):
    """As test_rccl_world1_update_bitwise: a one-rank RCCL communicator carries the standardisation sums
    of the GAE path, eager and inside the captured graph, and changes nothing."""
    from trpo_amd._lib import get_option, set_option
    d = upd_batch
    saved = get_option("graphs")
    try:
        set_option("graphs", 0)
        e0 = _upd_engine(d, ("gae", 0.95), tails=True)
        ref = _one_update(e0, d)
        e0.close()
        e1 = _upd_engine(d, ("gae", 0.95), tails=True, comm=True)
        runs = []
        for graphs in (0, 1, 1, 1, 1):       # eager; graphs: first-seen eager, capture, replay, replay
            set_option("graphs", graphs)
            runs.append(_one_update(e1, d))
        e1.close()
    finally:
        set_option("graphs", saved)
    for i, run in enumerate(runs):
        assert _same(run, ref), f"run {i}: {run[0]} vs {ref[0]}"


# ---------------------------------------------------------------------------- TRPOAgent
def _draws(seed, n_iter, n_timesteps=1000, ep_max=200):
    """Recorded env.reset / cat_sample uniforms per iteration (tests/test_gpu_learn.py)."""
    rng = np.random.RandomState(seed)
    ru = [rng.random_sample((1, n_timesteps, 4)) for _ in range(n_iter)]
    au = [rng.random_sample((1, n_timesteps + ep_max - 1)) for _ in range(n_iter)]
    return lambda i: (ru[i], au[i], n_timesteps)


def test_agent_learn_with_gae(gpu_available):
    from trpo_amd import TRPOAgent
    from trpo_amd.agent import CONFIG
    assert CONFIG.get("gae_lambda") is None
    gamma, lam = CONFIG["gamma"], 0.95
    agent = TRPOAgent(4, 2, hidden=(64,), max_rows=4096, config={**CONFIG, "gae_lambda": lam})
    assert agent.engine.advantage_estimator == ("gae", lam)
    hist = agent.learn(max_iterations=2, n_envs=1, log=None, draws=_draws(11, 2), record=True)
    assert len(hist) == 2
    for i, h in enumerate(hist):
        r, starts = h["rollout"]["rewards"], h["rollout"]["starts"]
        A_ref, _, _ = gae_ref(r, h["baseline"], gamma, lam, starts)
        np.testing.assert_allclose(h["advantages"], O.standardize(A_ref), rtol=1e-11, atol=1e-12, err_msg=str(i))
        np.testing.assert_allclose(h["returns"], O.discount_segmented(r, starts, gamma), rtol=1e-13)
    assert not np.any(hist[0]["baseline"]) and np.any(hist[1]["baseline"])
    r, starts = hist[0]["rollout"]["rewards"], hist[0]["rollout"]["starts"]
    np.testing.assert_allclose(hist[0]["advantages"], O.standardize(O.discount_segmented(r, starts, gamma * lam)),
                               rtol=1e-11, atol=1e-12)


def test_agent_update_passes_tail_values(gpu_available):
    """paths_to_batch turns per-path "tail_value" scalars into the feed's tail values; update and
    update_stepwise use the configured estimator."""
    from trpo_amd import TRPOAgent
    from trpo_amd.agent import CONFIG, paths_to_batch
    rng = np.random.RandomState(3)
    paths = []
    for j, T in enumerate((40, 25, 60)):
        dist = rng.dirichlet(np.ones(2), T).astype(np.float32)
        p = {"obs": rng.standard_normal((T, 4)), "action_dists": dist, "actions": rng.randint(0, 2, T),
             "rewards": np.ones(T), "baseline": rng.uniform(0, 10, T)}
        if j != 1:
            p["tail_value"] = 3.0 + j
        paths.append(p)
    b = paths_to_batch(paths)
    want = np.zeros(125)
    want[39], want[124] = 3.0, 5.0
    assert np.array_equal(b["tail_values"], want)
    assert "tail_values" not in paths_to_batch([{k: v for k, v in p.items() if k != "tail_value"} for p in paths])
    cfg = {**CONFIG, "gae_lambda": 0.9}
    theta = None
    for method in ("update", "update_stepwise"):
        agent = TRPOAgent(4, 2, hidden=(64,), max_rows=256, config=cfg)
        theta = agent.gf() if theta is None else theta
        agent.sff(theta)
        getattr(agent, method)(paths)
        ret, adv = agent.engine.compute_advantages(cfg["gamma"])
        A_ref, R_ref, _ = gae_ref(b["rewards"], b["baseline"], cfg["gamma"], 0.9, b["starts"], b["tail_values"])
        np.testing.assert_allclose(ret, R_ref, rtol=1e-13)
        np.testing.assert_allclose(adv, O.standardize(A_ref), rtol=1e-11, atol=1e-12)
        assert np.all(np.isfinite(agent.gf()))
