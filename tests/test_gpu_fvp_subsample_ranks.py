"""fvp_subsample across ranks: the Fisher rows taken by global row index (Engine.set_fvp_subsample(k, rows="global"),
Engine.set_row_offset; include/trpo_engine.h, trpo_amd.dist.fisher_rows).

What is held to what:
  * a one-rank RCCL communicator: the global mode at offset 0 is the local mode with every all-reduce an identity, so
    theta, stepdir and the stats are bitwise those of a communicator-free engine with set_fvp_subsample(k), eager and
    over first-seen / capture / replay / replay;
  * shards in one process: an engine fed rows [lo, hi) with row_offset = lo and n_global = N holds exactly
    X[lo:hi][phase::k] (and actions, old, advant), bit for bit; over a tiling the engines' undamped products sum to
    the whole engine's local-mode product within 1e-5 norm-relative (the project's bar for Hv);
  * the refusals leave the engine as it was; a row offset outside the global mode changes no bit and adds no launch;
  * two ranks on one GPU through tools/mrank_check.py and tools/mrank_learn.py.
"""
import functools

import numpy as np
import pytest

import update_outcomes_ref as U
from conftest import rel_l2
from oracle import trpo_oracle as O
from test_gpu_fvp_subsample import _feed
from trpo_amd.dist import fisher_rows

pytestmark = pytest.mark.gpu
REL = 1e-5
N = 1003


def ceil_div(a, b):
    return -(-a // b)


# ----------------------------------------------------------------------------------- world 1, RCCL communicator
def _update_engine(spec, d, comm, rows):
    from trpo_amd import Engine
    e = Engine(spec.obs_dim, spec.hidden, spec.n_actions, max_rows=d["X"].shape[0])
    if comm:
        e.comm_init(Engine.comm_unique_id(), 0, 1)
    e.set_fvp_subsample(3, rows=rows)
    e.set_flat(d["theta"])
    e.set_batch(d["X"], d["actions"], None, d["old_dist"], row_offset=0 if rows == "global" else None)
    e.set_rewards(d["rewards"], d["starts"])
    return e


@pytest.mark.parametrize("dims", [((11, [64, 64], 3), 3000), ((128, [256, 256], 18), 4001)])
def test_rccl_world1_global_rows_bitwise(gpu_available, dims):
    from trpo_amd import UpdateParams
    from trpo_amd._lib import VEC_STEPDIR, get_option, set_option
    (obs, hidden, A), n = dims
    spec = O.PolicySpec(obs, hidden, A)
    d = O.synthetic_batch(spec, n, seed=7)
    prm = UpdateParams(residual_tol=0.0, compute_advantages=True)
    saved = get_option("graphs")
    try:
        set_option("graphs", 0)
        e0 = _update_engine(spec, d, comm=False, rows="local")
        st0 = e0.update(prm)
        th0, sd0 = e0.get_flat(), e0.get_vector(VEC_STEPDIR)
        e0.close()
        e1 = _update_engine(spec, d, comm=True, rows="global")
        assert e1.fvp_subsample == (3, ceil_div(n, 3))
        assert e1.fvp_subsample_global == (3, ceil_div(n, 3), ceil_div(n, 3), 0)
        runs = []
        for graphs in (0, 1, 1, 1, 1):       # eager; graphs: first-seen eager, capture, replay, replay
            set_option("graphs", graphs)
            e1.set_flat(d["theta"])
            st = e1.update(prm)
            runs.append((st, e1.get_flat(), e1.get_vector(VEC_STEPDIR)))
        e1.close()
    finally:
        set_option("graphs", saved)
    for i, (st, th, sd) in enumerate(runs):
        assert np.array_equal(th, th0), f"run {i}: theta differs from the communicator-free local-mode engine"
        assert np.array_equal(sd, sd0), f"run {i}: stepdir differs"
        assert st == st0, f"run {i}: {st} vs {st0}"


# ------------------------------------------------------------------------------------------ shards in one process
def _shard_cases():
    cases = [(0, 400, 3), (400, N, 3), (401, N, 5), (999, N, 3), (1002, N, 3)]
    for k in (2, 7):                        # n - phase an exact multiple of k
        phase = fisher_rows(1, 7, k)[0]
        cases.append((7, 7 + 4 * k + phase, k))
    for n in (25, 28, 31, 34):              # phase 1 and n_sub = 8, 9, 10, 11: the scalar gather's tail of 0..3 rows
        cases.append((2, 2 + n, 3))
    return cases


def test_shard_cases_cover_the_edges():
    """(CPU arithmetic) the cases above are the ones their comments name."""
    got = {(lo, hi, k): fisher_rows(hi - lo, lo, k) for lo, hi, k in _shard_cases()}
    assert got[(400, N, 3)][0] == 2 and got[(401, N, 5)][0] == 4
    assert got[(999, N, 3)] == (0, 2) and got[(1002, N, 3)] == (0, 1)
    for k in (2, 7):
        lo, hi = 7, 7 + 4 * k + fisher_rows(1, 7, k)[0]
        assert (hi - lo - got[(lo, hi, k)][0]) % k == 0 and got[(lo, hi, k)][1] == 4
    assert {got[(2, 2 + n, 3)][1] % 4 for n in (25, 28, 31, 34)} == {0, 1, 2, 3}


@pytest.mark.parametrize("gaussian", [False, True])
def test_shard_feed_bit_exact(gpu_available, gaussian):
    """One engine, re-fed with every shard (a stale child would show the previous shard's rows)."""
    from trpo_amd import Engine
    obs, A = (17, 6) if gaussian else (11, 3)
    X, act, adv, old = (a[:N] for a in _feed(obs, A, gaussian))
    logstd = np.linspace(-1.0, 0.5, A).astype(np.float32)
    eng = Engine(obs, [64, 64], A, max_rows=N, dist="gaussian" if gaussian else "categorical")
    for lo, hi, k in _shard_cases():
        eng.set_fvp_subsample(k, rows="global")
        sl = slice(lo, hi)
        if gaussian:
            eng.set_batch_gaussian(X[sl], act[sl], adv[sl], old[sl], logstd, n_global=N, row_offset=lo)
        else:
            eng.set_batch(X[sl], act[sl], adv[sl], old[sl], n_global=N, row_offset=lo)
        phase, ns = fisher_rows(hi - lo, lo, k)
        assert eng.fvp_subsample == (k, ns), (lo, hi, k)
        assert eng.fvp_subsample_global == (k, ns, ceil_div(N, k), phase), (lo, hi, k)
        got = eng.fvp_subsample_fetch()
        for name, whole in (("states", X), ("actions", act), ("old", old), ("advant", adv)):
            want = whole[sl][phase::k]
            assert got[name].shape == want.shape, (name, lo, hi, k)
            assert np.array_equal(got[name], want), (name, lo, hi, k)
            # the same rows by their global index
            assert np.array_equal(want, whole[lo + phase:hi:k])
    eng.close()


@pytest.mark.parametrize("dims,n,cut", [((11, [64, 64], 3), N, 400), ((128, [256, 256], 18), 301, 100)])
def test_shard_products_sum_to_the_whole(gpu_available, dims, n, cut):
    """No transport: each engine's product is its shard's partial, scaled by 1 / N_sub."""
    from trpo_amd import Engine
    obs, hidden, A = dims
    k = 3
    spec = O.PolicySpec(obs, hidden, A)
    theta = O.synthetic_batch(spec, 8, seed=1)["theta"]
    X, act, adv, old = (a[:n] for a in _feed(obs, A, False))
    v = np.random.RandomState(4).standard_normal(spec.n_params).astype(np.float32)
    whole = Engine(obs, hidden, A, max_rows=n)
    whole.set_fvp_subsample(k)
    whole.set_flat(theta)
    whole.set_batch(X, act, adv, old)
    ref = whole.fvp(v, 0.0)
    whole.close()
    acc = np.zeros(spec.n_params, np.float64)
    for lo, hi in ((0, cut), (cut, n)):
        e = Engine(obs, hidden, A, max_rows=hi - lo)
        e.set_fvp_subsample(k, rows="global")
        e.set_flat(theta)
        e.set_batch(X[lo:hi], act[lo:hi], adv[lo:hi], old[lo:hi], n_global=n, row_offset=lo)
        acc += e.fvp(v, 0.0)
        e.close()
    err = rel_l2(acc, ref)
    print(f"{dims} x {n}, cut {cut}: sum of the shards' products vs the whole: rel {err:.2e}")
    assert err <= REL, err


# ------------------------------------------------------------------------------- refusals and unchanged defaults
@functools.lru_cache(maxsize=None)
def _small():
    spec = O.PolicySpec(11, [64, 64], 3)
    d = O.synthetic_batch(spec, 600, seed=2)
    return spec, d, d["advant"].astype(np.float32)


def test_global_refusals_leave_the_engine_as_it_was(gpu_available):
    from trpo_amd import Engine, UpdateParams
    from trpo_amd._lib import EngineError
    spec, d, adv = _small()
    n, n_global, lo = 600, 1500, 300
    out = []
    for refused in (True, False):
        e = Engine(11, [64, 64], 3, max_rows=n)
        e.set_fvp_subsample(5, rows="global")
        e.set_flat(d["theta"])
        e.set_batch(d["X"], d["actions"], adv, d["old_dist"], n_global=n_global, row_offset=lo)
        if refused:
            with pytest.raises(EngineError, match="row0 must be >= 0"):
                e.set_row_offset(-1)
            with pytest.raises(EngineError, match="exceeds n_global"):
                e.set_batch(d["X"], d["actions"], adv, d["old_dist"], n_global=n_global, row_offset=n_global - n + 1)
            with pytest.raises(EngineError, match="no multiple of the stride"):     # lo = 1, n = 2, k = 5: phase 4
                e.set_batch(d["X"][:2], d["actions"][:2], adv[:2], d["old_dist"][:2], n_global=n_global, row_offset=1)
            # the refused feeds left the old one in place, with its offset
            phase, ns = fisher_rows(n, lo, 5)
            assert e.fvp_subsample_global == (5, ns, ceil_div(n_global, 5), phase)
            e.set_row_offset(lo)
        out.append((e.update(UpdateParams(residual_tol=0.0)), e.get_flat()))
        e.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("k", [1, 3])
def test_row_offset_outside_the_global_mode_changes_nothing(gpu_available, k):
    from trpo_amd import Engine, UpdateParams
    from trpo_amd._lib import VEC_STEPDIR
    spec, d, adv = _small()
    out = []
    for offset in (None, 7):
        e = Engine(11, [64, 64], 3, max_rows=600)
        e.set_fvp_subsample(k)
        e.set_flat(d["theta"])
        e.profile_enable(True)
        if offset is not None:
            e.set_row_offset(offset)
        e.set_batch(d["X"], d["actions"], adv, d["old_dist"], row_offset=offset)
        st = e.update(UpdateParams(residual_tol=0.0))
        prof = e.profile_query()
        assert e.fvp_subsample == (k, ceil_div(600, k)) and e.fvp_subsample_global is None
        out.append((st, e.get_flat(), e.get_vector(VEC_STEPDIR), {t: c for t, (c, _ms) in prof.items()}))
        e.close()
    assert out[0][0] == out[1][0]
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    assert out[0][3] == out[1][3], "a row offset outside the global mode changed the launches"


def test_local_mode_keeps_its_refusals(gpu_available):
    from trpo_amd import Engine
    from trpo_amd._lib import EngineError
    spec, d, adv = _small()
    e = Engine(11, [64, 64], 3, max_rows=600)
    e.set_flat(d["theta"])
    e.set_batch(d["X"], d["actions"], adv, d["old_dist"])
    e.set_fvp_subsample(3)
    with pytest.raises(EngineError, match="n_global == n"):
        e.set_batch(d["X"], d["actions"], adv, d["old_dist"], n_global=1200, row_offset=600)
    with pytest.raises(EngineError, match="single-process"):
        e.comm_set_host_allreduce(lambda arr: None, 0, 2)
    assert e.comm_info()["transport"] == "none" and e.fvp_subsample == (3, 200)
    # the global mode takes both, before or after the transport; back in the local mode they are refused again
    e.set_fvp_subsample(3, rows="global")
    e.comm_set_host_allreduce(lambda arr: None, 0, 1)
    e.set_batch(d["X"], d["actions"], adv, d["old_dist"], n_global=1200, row_offset=600)
    assert e.fvp_subsample_global == (3, 200, 400, 0)
    with pytest.raises(EngineError, match="single-process"):
        e.set_fvp_subsample(3)
    assert e.fvp_subsample_global == (3, 200, 400, 0)
    e.close()


# ------------------------------------------------------------------------------------------ two ranks on one GPU
@pytest.mark.parametrize("extra", [("--dims", "c3", "--rows", "3000", "--fvp-subsample", "3"),
                                   ("--dims", "c4", "--rows", "1500", "--fvp-subsample", "7"),
                                   ("--dist", "gaussian", "--dims", "g17", "--rows", "3000", "--fvp-subsample", "3")],
                         ids=["c3-k3", "c4-k7", "g17-k3"])
def test_two_ranks_global_rows(gpu_available, extra):
    from test_gpu_parity import run_mrank
    run_mrank("--host-allreduce", "--graphs", *extra, timeout=300)


def test_two_ranks_backtrack_together(gpu_available):
    """update_outcomes_ref's mrank_c3 backtracking case with a subsampled Fisher matrix: what cg_iters, k and reverted
    must be comes from the float64 reference run here with stride K on the tool's own feed."""
    from test_gpu_parity import run_mrank
    K = 3
    c = U.BY_ID["mrank_c3-k_ge3"]
    p = U.PATHS[c.path]
    feed = U.make_feed(p.head, p.dims[0], tuple(p.dims[1]), p.dims[2], p.n, c.seed, c.perturbed, K, p.damping)
    ops = U.make_ops(feed, c.adv_scale)
    t = U.finish(ops, feed.theta, U._cg_trace(ops, feed.theta), c.tol, c.max_kl)
    print(f"float64 reference at stride {K}: outcome {t.outcome}, margins {U.margins(t)}")
    run_mrank("--host-allreduce", "--graphs", "--dims", "c3", "--rows", str(p.n), "--max-kl", repr(c.max_kl),
              "--residual-tol", repr(t.tol), "--adv-scale", repr(c.adv_scale), "--fvp-subsample", str(K),
              "--expect", ",".join(str(int(x)) for x in t.outcome), timeout=300)


# --------------------------------------------------------------------------------------------- two-rank learn()
@pytest.mark.parametrize("extra", [("--env", "Pendulum-v1", "--gae", "0.95", "--bootstrap"),
                                   ("--env", "CartPole-v0", "--fvp-subsample", "5")], ids=["pendulum-gae", "cartpole-k5"])
def test_learn_two_ranks(gpu_available, extra):
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
           "--host-allreduce", "--iters", "2", *extra]
    res = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "MRANK LEARN OK" in res.stdout
    print(res.stdout.strip().splitlines()[-2])
