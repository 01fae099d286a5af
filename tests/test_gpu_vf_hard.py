"""GPU hardening of the value-function baseline (trpo_vf_*, csrc/vf.cpp + vf.hip + the ReLU epilogues of rowepi.h)
against the float64 oracle on the cases of tests/vf_hard_cases.py.  Bars: the gradient per parameter block, the loss
and the predictions at the project's 1e-5 (conftest.assert_vec_close; tests/test_vf_hard_ref.py shows the float32
oracle within 2.5e-6 of float64 on every case and block); what the reference has exactly zero is exactly zero; the
Adam kernel against the float32 oracle stepped with the GPU's own gradient: m, v and the beta powers bit-equal,
theta to 1e-6 (sqrtf and the division may differ by an ulp); features and every buffer-reuse path bit-exact.
Every net is created with max_rows == n: a store past the last row has nowhere harmless to land."""
import numpy as np
import pytest

import vf_hard_cases as H
from conftest import assert_vec_close, rel_l2
from oracle import vf_oracle as V

pytestmark = pytest.mark.gpu

ADAM_ALT = dict(lr=0.01, beta1=0.5, beta2=0.9, epsilon=1e-3)


def new_net(F, hidden, theta, max_rows):
    from trpo_amd.vf import VFNet
    net = VFNet(F, max(1, int(max_rows)), hidden=hidden)
    net.set_params(theta)
    return net


def fed_net(case):
    """the case's net with max_rows == n, features and targets set"""
    c, d = H.BY_ID[case], H.inputs(case)
    net = new_net(c.F, c.hidden, d["theta"], c.shape[0])
    net.set_features(d["obs"], d["dist"], d["starts"])
    net.set_targets(d["y"])
    return net


# ------------------------------------------------------------------ 1. gradient, loss, predict per case
@pytest.mark.parametrize("case", H.IDS)
def test_gradient_loss_predict(gpu_available, case):
    c, r = H.BY_ID[case], H.refs(case)
    net = fed_net(case)
    try:
        assert np.array_equal(net.feature_matrix(), r["feat"])
        g, loss = net.gradient()
        pred = net.predict()
    finally:
        net.close()
    errs = H.block_errors(g, r["g"][0], c.F, c.hidden)
    print(f"{case} g: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()) +
          f"  | pred {rel_l2(pred, r['pred'][0]):.2e}  loss {abs(loss - r['loss'][0]) / r['loss'][0]:.2e}")
    assert g.dtype == np.float32 and np.isfinite(g).all()
    H.assert_blocks_close(g, r["g"][0], c.F, c.hidden, 1e-5, f"{case} VF gradient")
    if case in H.DEAD_IDS:
        assert not g[H.dead_mask(c.F, c.hidden)].any(), "a dead unit's gradient entries must be exactly zero"
    assert loss == pytest.approx(r["loss"][0], rel=1e-5)
    assert_vec_close(pred, r["pred"][0], 1e-5, f"{case} VF predict")


@pytest.mark.parametrize("hidden", [(513, 64), (64, 513), (0, 64), (64, 0), (4096, 4096)])
def test_width_outside_the_accepted_range_is_refused(gpu_available, hidden):
    from trpo_amd._lib import EngineError
    from trpo_amd.vf import VFNet
    with pytest.raises(EngineError, match="hidden widths"):
        VFNet(7, 16, hidden=hidden)


def test_widest_accepted_net_is_created(gpu_available):
    from trpo_amd.vf import VFNet
    net = VFNet(7, 16, hidden=(512, 512))
    assert net.num_params == 7 * 512 + 512 + 512 * 512 + 512 + 512 + 1
    net.close()


# ------------------------------------------------------------------ 2. the Adam kernel in isolation
def _adam_steps(net, theta, hyper, steps=3):
    """`steps` x (read the GPU's gradient, fit(1), step the float32 oracle with that gradient), comparing the state
    after every step; returns the oracle's theta"""
    kw = {} if hyper is None else dict(lr=hyper["lr"], beta1=hyper["beta1"], beta2=hyper["beta2"],
                                       eps=hyper["epsilon"])
    adam = V.Adam(theta.size, dtype=np.float32, **kw)
    th = theta.copy()
    for step in range(1, steps + 1):
        g, _ = net.gradient()
        net.fit(1)
        th = adam.step(th, g)
        assert th.dtype == np.float32
        st = net.optimizer_state()
        assert st["steps"] == step == adam.t
        assert st["beta1_power"] == adam.b1p and st["beta2_power"] == adam.b2p
        # adam_kernel is the oracle's IEEE operation sequence with contraction off: m and v are bit-equal
        assert np.array_equal(st["m"], adam.m), f"m after step {step}"
        assert np.array_equal(st["v"], adam.v), f"v after step {step}"
        np.testing.assert_allclose(net.get_params(), th, rtol=1e-6, atol=1e-6 * float(adam.lr),
                                   err_msg=f"theta after step {step}")
    return th


@pytest.mark.parametrize("alt", [False, True], ids=["defaults", "set_adam"])
@pytest.mark.parametrize("hidden", [(17, 33), (256, 256)])
def test_adam_kernel_against_float32_oracle(gpu_available, hidden, alt):
    case = H.case_id(hidden)
    d = H.inputs(case)
    net = fed_net(case)
    try:
        if alt:
            net.set_adam(**ADAM_ALT)
        th = _adam_steps(net, d["theta"], ADAM_ALT if alt else None)
        assert not np.array_equal(th, d["theta"])
    finally:
        net.close()


@pytest.mark.parametrize("case", H.DEAD_IDS)
def test_adam_leaves_dead_units_bit_unchanged(gpu_available, case):
    c, d = H.BY_ID[case], H.inputs(case)
    net = fed_net(case)
    try:
        _adam_steps(net, d["theta"], None)
        th = net.get_params()
        st = net.optimizer_state()
    finally:
        net.close()
    mask = H.dead_mask(c.F, c.hidden)
    assert np.array_equal(th[mask], d["theta"][mask])
    assert not st["m"][mask].any() and not st["v"][mask].any()
    assert (th[~mask] != d["theta"][~mask]).mean() > 0.9


def test_set_adam_and_reset_optimizer_clear_the_state(gpu_available):
    case = H.case_id((17, 33))
    net = fed_net(case)
    try:
        def cleared(b1, b2):
            st = net.optimizer_state()
            assert st["steps"] == 0 and not st["m"].any() and not st["v"].any()
            assert st["beta1_power"] == np.float32(b1) and st["beta2_power"] == np.float32(b2)
        cleared(0.9, 0.999)
        net.fit(2)
        st = net.optimizer_state()
        assert st["steps"] == 2 and st["m"].any() and st["v"].any()
        assert st["beta1_power"] == np.float32(np.float32(0.9) * np.float32(0.9) * np.float32(0.9))
        net.set_adam(**ADAM_ALT)
        cleared(0.5, 0.9)
        net.fit(2)
        assert net.optimizer_state()["steps"] == 2
        net.reset_optimizer()
        cleared(0.5, 0.9)          # the hyper-parameters stay, the state goes
        from trpo_amd._lib import EngineError
        with pytest.raises(EngineError, match="Adam"):
            net.set_adam(lr=0.0)
    finally:
        net.close()


# ------------------------------------------------------------------ 3. three-step fit against the float64 oracle
@pytest.mark.parametrize("hidden", [(17, 33), (65, 130), (256, 256)])
def test_three_step_fit_against_float64_oracle(gpu_available, hidden):
    case = H.case_id(hidden)
    c, d, r = H.BY_ID[case], H.inputs(case), H.refs(case)
    net = fed_net(case)
    try:
        net.fit(3)
        th, pred = net.get_params(), net.predict()
    finally:
        net.close()
    th_ref, _ = V.fit(d["theta"].astype(np.float64), r["feat"], d["y"], 3, c.hidden)
    e_th, e_pred = rel_l2(th, th_ref), rel_l2(pred, V.predict(th_ref, r["feat"], c.hidden))
    print(f"{case} fit(3): theta {e_th:.2e}  pred {e_pred:.2e}")
    assert e_th < 1e-5
    assert e_pred < 1e-5


# ------------------------------------------------------------------ 4. long paths and the chunk carry
K = 4096      # rows per block of the position scan (vf.hip kPosBlock); its block prefix runs in chunks of 256 blocks
LONG = [
    # no start in row 0; a path from 3 K + 7 to 255 K + 4095 leaves most blocks without a start; starts in the
    # second chunk of blocks (256 K, 256 K + 4097) read the carry of the first
    (257 * K + 5, (K - 1, K, 3 * K + 7, 255 * K + 4095, 256 * K, 256 * K + 4097)),
    (3 * K + 1, (K,)),
    # the same without the start at 256 K: block 256 holds no start at all, so its rows, and row 257 K before the
    # start at 257 K + 1, have only the carry across the chunk boundary to find 255 K + 4095 by
    (257 * K + 5, (K - 1, K, 3 * K + 7, 255 * K + 4095, 256 * K + 4097)),
]


@pytest.mark.parametrize("n,start_rows", LONG, ids=["n257x4096+5", "n3x4096+1", "n257x4096+5-carry"])
def test_long_paths_and_block_carry_bit_exact(gpu_available, n, start_rows):
    rng = np.random.RandomState(n % 1000)
    o = rng.standard_normal((n, 1)).astype(np.float32)
    d = np.ones((n, 1), np.float32)
    starts = np.zeros(n, np.uint8)
    starts[list(start_rows)] = 1
    net = new_net(3, (1, 1), H.vf_xavier_params(3, (1, 1)), n)
    try:
        net.set_features(o, d, starts)
        got = net.feature_matrix()
    finally:
        net.close()
    ref = V.features_concat_vec(o, d, starts)
    assert ref[:, 2].max() == np.float32((max(np.diff(np.r_[0, start_rows, n])) - 1) / 10.0)
    assert np.array_equal(got, ref)


# ------------------------------------------------------------------ 5. buffer reuse and state
def _feed(n, seed, obs=4, A=2):
    o, d, starts, y = H.batch(n, obs, A, seed)
    return {"obs": o, "dist": d, "starts": starts, "y": y}


def _run(net, b):
    net.set_features(b["obs"], b["dist"], b["starts"])
    net.set_targets(b["y"])
    g, loss = net.gradient()
    return g, loss, net.predict(), net.feature_matrix()


@pytest.mark.parametrize("hidden", [(64, 64), (129, 64)])
def test_refeed_fewer_then_more_rows_equals_fresh_nets(gpu_available, hidden):
    F = 7
    theta = H.theta_for(F, hidden, 3)
    feeds = [_feed(3001, 21), _feed(513, 22), _feed(3001, 23)]
    net = new_net(F, hidden, theta, 3001)
    try:
        for i, b in enumerate(feeds):
            got = _run(net, b)
            fresh = new_net(F, hidden, theta, len(b["y"]))
            try:
                want = _run(fresh, b)
            finally:
                fresh.close()
            for name, x, y in zip(("gradient", "loss", "predict", "features"), got, want):
                assert np.array_equal(x, y), f"feed {i}: {name} differs from a fresh net's"
        assert not np.array_equal(got[0], _run(net, feeds[0])[0])     # the feeds do differ
    finally:
        net.close()


def test_targets_go_stale_with_the_row_count_only(gpu_available):
    from trpo_amd._lib import EngineError
    F, hidden = 7, (64, 64)
    a, b, c = _feed(600, 31), _feed(600, 32), _feed(257, 33)
    net = new_net(F, hidden, H.theta_for(F, hidden, 3), 600)
    try:
        with pytest.raises(EngineError, match="features and targets"):
            net.gradient()
        net.set_features(a["obs"], a["dist"], a["starts"])
        with pytest.raises(EngineError, match="features and targets"):
            net.gradient()
        net.set_targets(a["y"])
        g_a, _ = net.gradient()
        net.set_features(b["obs"], b["dist"], b["starts"])        # same row count: the targets stay
        g_b, _ = net.gradient()
        assert not np.array_equal(g_a, g_b)
        net.set_features(c["obs"], c["dist"], c["starts"])        # another row count: they do not
        with pytest.raises(EngineError, match="features and targets"):
            net.gradient()
        net.set_targets(c["y"])
        net.gradient()
        big = _feed(601, 34)
        with pytest.raises(EngineError, match="max_rows"):
            net.set_features(big["obs"], big["dist"], big["starts"])
        with pytest.raises(EngineError, match="max_rows"):
            net.set_feature_matrix(np.zeros((601, F), np.float32))
    finally:
        net.close()


def test_targets_host_float64_and_float32_bit_equal(gpu_available):
    """float64 host targets go through the float32 staging buffer and the device conversion; float32 ones straight in"""
    F, hidden = 7, (64, 64)
    b = _feed(1000, 41)
    net = new_net(F, hidden, H.theta_for(F, hidden, 3), 1000)
    try:
        net.set_features(b["obs"], b["dist"], b["starts"])
        net.set_targets(b["y"].astype(np.float64))
        g64, l64 = net.gradient()
        net.set_targets(np.zeros(1000, np.float32))
        assert not np.array_equal(net.gradient()[0], g64)
        net.set_targets(b["y"])
        g32, l32 = net.gradient()
        assert np.array_equal(g32, g64) and l32 == l64
    finally:
        net.close()


@pytest.mark.parametrize("F", [8, 7], ids=["F8-direct-copy", "F7-copy-rows"])
def test_feature_matrix_round_trip(gpu_available, F):
    n = 1001
    feat = np.random.RandomState(F).standard_normal((n, F)).astype(np.float32)
    theta = H.theta_for(F, (64, 64), 3)
    net = new_net(F, (64, 64), theta, n)
    try:
        net.set_feature_matrix(feat)
        assert np.array_equal(net.feature_matrix(), feat)
        assert_vec_close(net.predict(), V.predict(theta.astype(np.float64), feat), 1e-5, "predict")
        net.set_feature_matrix(feat[:17])          # fewer rows: the matrix read back is the new one
        assert np.array_equal(net.feature_matrix(), feat[:17])
    finally:
        net.close()


def test_predict_float64_equals_predict_float32(gpu_available):
    case = H.case_id((129, 64))
    net = fed_net(case)
    n = H.BY_ID[case].shape[0]
    try:
        p32 = net.predict()
        assert p32.dtype == np.float32 and p32.shape == (n,)
        p64 = net.predict(dtype=np.float64)
        assert p64.dtype == np.float64 and np.array_equal(p64, p32.astype(np.float64))
        out = np.full(n, -7.0)
        assert net.predict(out) is out and np.array_equal(out, p64)
    finally:
        net.close()


_DEVICE_SCRIPT = r"""
import sys, numpy as np, torch
torch.cuda.init()                      # torch's HIP runtime first (engine.py: rollout_fetch note)
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import vf_hard_cases as H
from oracle import vf_oracle as V
from trpo_amd.vf import VFNet
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
F, hidden, n = 7, (64, 64), 1000
o, d, starts, y32 = H.batch(n, 4, 2, 41)
theta = H.theta_for(F, hidden, 3)
net = VFNet(F, n, hidden=hidden)
net.set_params(theta)

# targets: float64 / float32, host / device
net.set_features(o, d, starts)
feat_host = net.feature_matrix()
y64 = y32.astype(np.float64)
targets = [y64, y32, dev(y64), dev(y32)]
torch.cuda.synchronize()
grads = []
for y in targets:
    net.set_targets(np.zeros(n, np.float32))
    net.set_targets(y)
    grads.append(net.gradient())
for g, loss in grads[1:]:
    assert np.array_equal(g, grads[0][0]) and loss == grads[0][1]

# set_features from device tensors, with starts and as one path
fdev = [dev(o), dev(d), dev(starts)]
torch.cuda.synchronize()
net.set_feature_matrix(np.zeros((n, F), np.float32))
net.set_features(*fdev)
assert np.array_equal(net.feature_matrix(), feat_host)
g, loss = net.gradient()
assert np.array_equal(g, grads[0][0]) and loss == grads[0][1]
net.set_features(fdev[0], fdev[1], None)
assert np.array_equal(net.feature_matrix(), V.features_concat_vec(o, d, np.r_[1, np.zeros(n - 1, np.uint8)]))
try:
    net.set_features(fdev[0], d, None)
    raise SystemExit("mixed host / device inputs were accepted")
except ValueError:
    pass

# predict into device buffers (one element of slack: nothing is written past row n - 1)
net.set_features(*fdev)
p32 = net.predict()
for tdt, ndt in ((torch.float64, np.float64), (torch.float32, np.float32)):
    buf = torch.full((n + 1,), -7.0, dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    net.predict_to_device(buf.data_ptr(), ndt)
    out = buf.cpu().numpy()
    assert np.array_equal(out[:n], p32.astype(ndt)) and out[n] == -7.0
    buf2 = torch.full((n,), -7.0, dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    assert net.predict(buf2) is buf2 and np.array_equal(buf2.cpu().numpy(), p32.astype(ndt))
net.close()

# set_feature_matrix from a device tensor: F % 4 == 0 copies straight in, F % 4 != 0 goes through copy_rows
for Fm in (8, 7):
    feat = np.random.RandomState(Fm).standard_normal((1001, Fm)).astype(np.float32)
    m = VFNet(Fm, 1001, hidden=hidden)
    m.set_params(H.theta_for(Fm, hidden, 3))
    m.set_feature_matrix(feat)
    p_host = m.predict()
    m.set_feature_matrix(np.zeros((1001, Fm), np.float32))
    t = dev(feat)
    torch.cuda.synchronize()
    m.set_feature_matrix(t)
    assert np.array_equal(m.feature_matrix(), feat)
    assert np.array_equal(m.predict(), p_host)
    m.close()
print("DEVICE VF OK")
"""


def test_device_tensor_inputs_and_outputs(gpu_available):
    """mem = TRPO_MEM_DEVICE on torch-ROCm tensors: targets, features, the feature matrix, predict into device
    buffers, all bit-equal to the host forms (own process: torch initialises HIP first)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", _DEVICE_SCRIPT, root], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "DEVICE VF OK" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]


# ------------------------------------------------------------------ 6. sharding at a wide shape
def test_three_uneven_shards_sum_to_full_wide(gpu_available):
    """tests/test_gpu_vf.py::test_sharded_gradient_sums_to_full at (129, 64): shards of 1, 64 and 712 rows"""
    case = H.case_id((129, 64))
    c, d = H.BY_ID[case], H.inputs(case)
    n = c.shape[0]
    cuts = (0, 1, 65, n)
    assert n == 777 and np.diff(cuts).tolist() == [1, 64, 712]
    starts = d["starts"].copy()
    starts[list(cuts[:-1])] = 1               # shards begin at a path start
    total = np.zeros(H.block_bounds(c.F, c.hidden)[-1][1], np.float64)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        net = new_net(c.F, c.hidden, d["theta"], hi - lo)
        try:
            net.set_features(d["obs"][lo:hi], d["dist"][lo:hi], starts[lo:hi], n_global=n)
            net.set_targets(d["y"][lo:hi])
            total += net.gradient()[0]
        finally:
            net.close()
    full = new_net(c.F, c.hidden, d["theta"], n)
    try:
        full.set_features(d["obs"], d["dist"], starts)
        full.set_targets(d["y"])
        g_full, _ = full.gradient()
    finally:
        full.close()
    H.assert_blocks_close(total, g_full, c.F, c.hidden, 1e-5, "sharded VF gradient")
    feat = V.features_concat_vec(d["obs"], d["dist"], starts)
    g_ref, _ = V.gradient(d["theta"].astype(np.float64), feat, d["y"], c.hidden)
    H.assert_blocks_close(total, g_ref, c.F, c.hidden, 1e-5, "sharded VF gradient against the oracle")
