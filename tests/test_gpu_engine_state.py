"""The engine runtime's bookkeeping (engine.cpp CacheState, abi_util.h Staging) seen from outside:

* a replayed update graph leaves the engine in the state an eager update leaves it in: the policy gradient and
  the FVP that follow, which trust the cache flags, are bitwise those of an engine that never replayed;
* the engine-free entries (standalone.cpp) give bitwise the same results for host arrays and device tensors,
  and those results meet the float64 references at the bars of the tests that own them (test_gpu_gae.py,
  test_gpu_parity.py, test_gpu_rollout.py).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import trpo_oracle as O

pytestmark = pytest.mark.gpu

# (obs, hidden, actions, rows) and the profile tags that prove the shape took the path whose flags it is here for:
# hbwd2 (ds_ready, d1_plane, d1_tiled), rbwd0 and the tail on two 256-row plane tiles, one of them partial; the same
# with an obs width whose planes also feed rfwd01 / fwd01; fused16 with its prepare-time policy-gradient slabs
# (pg_ready, pg_grid) on one and two hidden layers
REPLAY_SHAPES = [
    ((8, [256, 256], 18, 300), {"bwd2_l2", "fvp_rbwdwg_l1", "fvp_tail_l2"}),
    ((64, [256, 256], 18, 300), {"bwd2_l2", "fvp_rbwdwg_l1", "fvp_tail_l2", "fvp_rfwd01", "fwd_l01"}),
    ((4, [64], 2, 70), {"bwd_pg", "fvp_fused"}),
    ((11, [64, 64], 3, 257), {"bwd_pg", "fvp_fused"}),
]


def _after_three_updates(spec, d, v, graphs):
    """Three updates (with graphs: first-seen eager, capture, replay), then g, Hv and g again from the state
    they leave, theta and the batch untouched."""
    from trpo_amd import Engine, UpdateParams
    from trpo_amd._lib import set_option
    set_option("graphs", graphs)
    e = Engine(spec.obs_dim, spec.hidden, spec.n_actions, max_rows=d["X"].shape[0])
    e.set_flat(d["theta"])
    e.set_batch(d["X"], d["actions"], d["advant"].astype(np.float32), d["old_dist"])
    stats = [e.update(UpdateParams(cg_iters=10, residual_tol=0.0)) for _ in range(3)]
    out = [e.get_flat(), e.policy_grad(), e.fvp(v, 0.1), e.policy_grad()]
    return e, stats, out


@pytest.mark.parametrize("shape,tags", REPLAY_SHAPES,
                         ids=[f"{s[0]}-{'x'.join(map(str, s[1]))}-{s[2]}-n{s[3]}" for s, _ in REPLAY_SHAPES])
def test_state_after_replay_equals_eager(gpu_available, shape, tags):
    from trpo_amd import UpdateParams
    from trpo_amd._lib import get_option, set_option
    obs, hidden, A, n = shape
    spec = O.PolicySpec(obs, hidden, A)
    d = O.synthetic_batch(spec, n, seed=n)
    v = np.random.RandomState(1).standard_normal(spec.n_params).astype(np.float32)
    saved = get_option("graphs")
    try:
        replayed, st1, out1 = _after_three_updates(spec, d, v, 1)
        replayed.close()
        eager, st0, out0 = _after_three_updates(spec, d, v, 0)
        # the paths the shape is here for (profiling runs the prefix eagerly: on the eager engine, afterwards)
        eager.profile_enable()
        eager.set_flat(d["theta"])   # a new theta: the update starts from the prepare pass
        eager.update(UpdateParams(cg_iters=10, residual_tol=0.0))
        seen = set(eager.profile_query())
        eager.close()
    finally:
        set_option("graphs", saved)
    assert tags <= seen, f"{shape}: paths not taken: {sorted(tags - seen)} (tags seen: {sorted(seen)})"
    assert st1 == st0
    for name, a, b in zip(("theta", "g", "Hv", "g after Hv"), out1, out0):
        assert np.all(np.isfinite(b)), name
        assert a.tobytes() == b.tobytes(), f"{shape}: {name} differs after a replayed update"


_MEM_SCRIPT = r"""
import ctypes, sys, numpy as np, torch
torch.cuda.init()                      # torch's HIP runtime first (engine.py: rollout_fetch note)
root = sys.argv[1]
sys.path[:0] = [root, root + "/tests"]
from gae_ref import gae_ref
from oracle import cartpole_oracle as C
from trpo_amd._lib import MEM_DEVICE, check, lib
from trpo_amd.engine import cartpole_step_device, cat_sample_device, discount_device, gae_device
dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
ptr = lambda t: ctypes.c_void_p(t.data_ptr())
same = lambda t, a: t.is_cuda and t.cpu().numpy().dtype == a.dtype and t.cpu().numpy().tobytes() == a.tobytes()

gold = np.load(root + "/tests/golden/discount.npz", allow_pickle=False)
for k in sorted(x[:-2] for x in gold.files if x.endswith("_x")):
    gamma = float(k.split("_")[0][1:])
    y = discount_device(gold[k + "_x"], gamma)
    np.testing.assert_allclose(y, gold[k + "_y"], rtol=1e-13, err_msg=k)         # test_discount_vs_golden
    assert same(discount_device(dev(gold[k + "_x"]), gamma), y), k

for n in (1, 4099):                    # one row; two scan tiles and three rows
    rng = np.random.RandomState(n)
    r, v = rng.uniform(0, 1, n), 10.0 * rng.standard_normal(n)
    starts = (rng.uniform(size=n) < 0.01).astype(np.uint8)
    starts[0] = 1
    tails = np.abs(10.0 * rng.standard_normal(n))
    for st in (None, starts):
        y = discount_device(r, 0.99, st)
        assert same(discount_device(dev(r), 0.99, dev(st)), y), ("discount", n, st is None)
        np.testing.assert_allclose(y, gae_ref(r, None, 0.99, 1.0, st)[1], rtol=1e-12)   # test_discount_segmented_large
    for tv in (None, tails):
        A, R = gae_device(r, v, 0.99, 0.95, starts, tv)
        At, Rt = gae_device(dev(r), dev(v), 0.99, 0.95, dev(starts), dev(tv))
        assert same(At, A) and same(Rt, R), ("gae", n, tv is None)
        A_ref, R_ref, _ = gae_ref(r, v, 0.99, 0.95, starts, tv)
        assert np.max(np.abs(A - A_ref)) <= 1e-12 * np.max(np.abs(A_ref))        # test_gpu_gae.py, bars A and R
        np.testing.assert_allclose(R, R_ref, rtol=1e-13)

    prob = rng.dirichlet(np.ones(3), n).astype(np.float32)
    u = rng.random_sample(n)
    a = cat_sample_device(prob, u)
    assert np.array_equal(a, C.cat_sample(prob, u))                              # test_cat_sample_bit_exact
    at = torch.empty(n, dtype=torch.int64, device="cuda")
    tp, tu = dev(prob), dev(u)
    check(lib.trpo_cat_sample(ptr(tp), n, 3, ptr(tu), ptr(at), MEM_DEVICE), "trpo_cat_sample")
    assert same(at, a), ("cat_sample", n)

    s = rng.uniform(-0.3, 0.3, (n, 4)) * np.array([8, 3, 1, 3])
    act = rng.randint(0, 2, n).astype(np.int64)
    so, rw, dn = cartpole_step_device(s, act)
    ref = [C.CartPoleV0.dynamics(s[i], act[i]) for i in range(n)]
    assert np.allclose(so, np.array([x[0] for x in ref]), rtol=1e-13, atol=1e-15)   # test_cartpole_step_vs_oracle
    assert np.array_equal(dn, np.array([x[1] for x in ref])) and (rw == 1.0).all()
    ts, ta = dev(s), dev(act)
    tso = torch.empty((n, 4), dtype=torch.float64, device="cuda")
    trw = torch.empty(n, dtype=torch.float64, device="cuda")
    tdn = torch.empty(n, dtype=torch.uint8, device="cuda")
    check(lib.trpo_cartpole_step(ptr(ts), ptr(ta), n, ptr(tso), ptr(trw), ptr(tdn), MEM_DEVICE), "trpo_cartpole_step")
    assert same(tso, so) and same(trw, rw) and same(tdn, dn.astype(np.uint8)), ("cartpole_step", n)
print("HOST DEVICE MEM OK")
"""


def test_standalone_host_and_device_mem_agree(gpu_available):
    """trpo_discount (with and without starts), trpo_gae (with and without tail values), trpo_cat_sample and
    trpo_cartpole_step on host arrays and on torch-ROCm tensors (own process: torch initialises HIP first)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", _MEM_SCRIPT, root], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "HOST DEVICE MEM OK" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
