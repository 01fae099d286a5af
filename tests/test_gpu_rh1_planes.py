"""RH1 as row-paired f16 planes (option rh1_planes; rfwd.hip writes them, rbwd0.hip's epilogue and gemm.hip's
wgrad3 read them) at the C4 layer shapes.

The option moves the low_seg decision from "how many products" to "how many bytes": where the test fires the readers
fetch RH1's hi plane alone, where it does not they fetch hi + lo.  Both must meet the float64 oracle
(trpo_inksci.py:56-70) at the bar of test_rfwd01_vs_two_launches_and_oracle, and the f32 form (rh1_planes = 0)
at the same bar.  Row counts: one state, one row pair, a partial 128-state tile, two 256-row plane tiles with one
partial, many tiles with an odd count (the last pair's odd row is past n).
"""
import numpy as np
import pytest

from conftest import assert_vec_close, rel_l2
from oracle import trpo_oracle as O

pytestmark = pytest.mark.gpu

REL = 1e-5
SPEC = O.PolicySpec(128, [256, 256], 18)


def _block_slices(spec):
    w = [spec.obs_dim] + list(spec.hidden) + [spec.n_actions]
    out, o = [], 0
    for l in range(len(w) - 1):
        out += [slice(o, o + w[l] * w[l + 1]), slice(o + w[l] * w[l + 1], o + w[l] * w[l + 1] + w[l + 1])]
        o += w[l] * w[l + 1] + w[l + 1]
    return out


def make_case(case, n):
    """theta, X, v, actions, advantages, old_dist of a regime (the constructions of
    test_rfwd01_vs_two_launches_and_oracle and test_saturated_softmax_fvp_vs_oracle)."""
    spec = SPEC
    dd = O.synthetic_batch(spec, n, seed=41)
    th = dd["theta"].astype(np.float32).copy()
    X = dd["X"].astype(np.float32).copy()
    v = np.random.RandomState(42).standard_normal(spec.n_params).astype(np.float32)
    w0, b0 = _block_slices(spec)[:2]
    old = dd["old_dist"]
    if case == "v0_big":
        v[w0] *= 100.0
        v[b0] *= 100.0
    elif case == "v0_small":
        v[w0] *= 1e-3
        v[b0] *= 1e-3
    elif case == "tanh_sat":
        th[w0] *= 20.0
    elif case == "mixed":
        W0 = th.astype(np.float64)[w0].reshape(spec.obs_dim, spec.hidden[0])
        W0[-3:, :] = 0.0
        th[w0] = W0.reshape(-1).astype(np.float32)
        rs = np.random.RandomState(43)
        for i in range(5, n, 29):
            X[i, -3:] = (2.0 ** 15 * rs.standard_normal(3)).astype(np.float32)
    elif case == "softmax_sat":
        params = O.unflatten(th.astype(np.float64).copy(), spec)
        W, b = params[-1]
        W *= 25.0
        b *= 25.0
        th = O.flatten(params).astype(np.float32)
        old = O.action_dist(th.astype(np.float64), X.astype(np.float64), spec, np.float64).astype(np.float32)
        assert (old < 1e-6).mean() > 0.2   # the regime: the O(eps) terms comparable to the R-terms
    else:
        assert case == "random"
    return dict(theta=th, X=X, v=v, actions=dd["actions"], advant=dd["advant"].astype(np.float32), old=old)


class _Options:
    """Set engine options for a block, restore them after."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from trpo_amd._lib import get_option, set_option
        self.saved = {k: get_option(k) for k in self.kw}
        for k, val in self.kw.items():
            set_option(k, val)

    def __exit__(self, *exc):
        from trpo_amd._lib import set_option
        for k, val in self.saved.items():
            set_option(k, val)


def _engine(c):
    from trpo_amd import Engine
    e = Engine(SPEC.obs_dim, SPEC.hidden, SPEC.n_actions, max_rows=c["X"].shape[0])
    e.set_flat(c["theta"])
    e.set_batch(c["X"], c["actions"], c["advant"], c["old"])
    return e


def _hv(c, **opts):
    with _Options(**opts):
        e = _engine(c)
        out = e.fvp(c["v"], 0.0)
        e.close()
    return out


CASES = [("random", 1), ("random", 2), ("random", 129), ("random", 300), ("random", 3001),
         ("v0_big", 3001), ("v0_small", 3001), ("mixed", 3001), ("tanh_sat", 3001), ("softmax_sat", 3001)]


@pytest.mark.parametrize("case,n", CASES, ids=[f"{c}-n{n}" for c, n in CASES])
def test_fvp_planes_vs_oracle_and_f32(gpu_available, case, n):
    """Hv per parameter block against the float64 oracle and against rh1_planes = 0 at 1e-5, with the low_seg test
    live (14: the hi plane alone where it fires) and off (0: hi + lo everywhere).  The oracle's own float32
    evaluation is within the bar on every input here (checked when the cases were chosen, asserted below)."""
    c = make_case(case, n)
    ref = O.fvp_undamped(c["theta"].astype(np.float64), c["X"].astype(np.float64), c["v"].astype(np.float64), SPEC)
    ref32 = O.fvp_undamped(c["theta"], c["X"], c["v"], SPEC, dtype=np.float32)
    hv = {(p, ls): _hv(c, rh1_planes=p, low_seg=ls) for p in (1, 0) for ls in (14, 0)}
    for sl in _block_slices(SPEC):
        assert rel_l2(ref32[sl], ref[sl]) <= REL, (case, n, "the float32 oracle misses the bar on this input")
    for ls in (14, 0):
        for i, sl in enumerate(_block_slices(SPEC)):
            print(f"{case} n={n} low_seg={ls} block {i}: planes {rel_l2(hv[1, ls][sl], ref[sl]):.3e} "
                  f"f32 {rel_l2(hv[0, ls][sl], ref[sl]):.3e} planes vs f32 {rel_l2(hv[1, ls][sl], hv[0, ls][sl]):.3e}")
        for i, sl in enumerate(_block_slices(SPEC)):
            assert_vec_close(hv[1, ls][sl], ref[sl], REL, f"{case} n={n} low_seg={ls} block {i} vs oracle")
            assert_vec_close(hv[1, ls][sl], hv[0, ls][sl], REL, f"{case} n={n} low_seg={ls} block {i} vs rh1_planes=0")
    if case == "random":
        # the test fires on random data: one product and the hi plane alone give other bits than three products
        # and both planes
        assert hv[1, 14].tobytes() != hv[1, 0].tobytes()
        assert hv[0, 14].tobytes() != hv[0, 0].tobytes()
    if (case, n) == ("random", 3001):
        assert hv[1, 14].tobytes() != hv[0, 14].tobytes()   # the planes were read (their hi half rounds toward zero)


def test_update_planes_on_vs_off(gpu_available):
    """One whole update (cg_iters = 10, residual_tol = 0) with the option on against off."""
    from trpo_amd import UpdateParams
    from trpo_amd._lib import VEC_G, VEC_STEPDIR
    c = make_case("random", 3001)
    res = {}
    for p in (1, 0):
        with _Options(rh1_planes=p):
            e = _engine(c)
            st = e.update(UpdateParams(cg_iters=10, residual_tol=0.0))
            res[p] = (st, e.get_flat(), e.get_vector(VEC_G), e.get_vector(VEC_STEPDIR))
            e.close()
    for k in ("k", "cg_iters", "reverted"):
        assert res[1][0][k] == res[0][0][k], (k, res[1][0][k], res[0][0][k])
    for name, a, b in zip(("theta", "g", "stepdir"), res[1][1:], res[0][1:]):
        assert np.all(np.isfinite(a)), name
        assert_vec_close(a, b, REL, name)


def _three_updates(c, graphs, reset_theta):
    from trpo_amd import UpdateParams
    with _Options(graphs=graphs, rh1_planes=1):
        e = _engine(c)
        stats = []
        for _ in range(3):
            stats.append(e.update(UpdateParams(cg_iters=10, residual_tol=0.0)))
            if reset_theta:
                e.set_flat(c["theta"])   # a new theta between updates: everything prepare() derived is stale
        out = [e.get_flat(), e.policy_grad(), e.fvp(c["v"], 0.1), e.policy_grad()]
        e.close()
    return stats, out


@pytest.mark.parametrize("reset_theta", [False, True], ids=["plain", "set_flat_between"])
def test_replay_equals_eager_with_planes(gpu_available, reset_theta):
    """As test_state_after_replay_equals_eager: three updates with graphs on and off leave identical bytes."""
    c = make_case("random", 300)
    st1, out1 = _three_updates(c, 1, reset_theta)
    st0, out0 = _three_updates(c, 0, reset_theta)
    assert st1 == st0
    for name, a, b in zip(("theta", "g", "Hv", "g after Hv"), out1, out0):
        assert np.all(np.isfinite(b)), name
        assert a.tobytes() == b.tobytes(), f"{name} differs after a replayed update"


def test_option_switch_on_live_engine(gpu_available):
    """on -> off -> on between fvp() calls of one engine: each call gives its own form's result, bit for bit (no
    plane of an earlier call is consumed, no f32 RH1 either)."""
    from trpo_amd._lib import get_option, set_option
    c = make_case("random", 3001)
    want = {p: _hv(c, rh1_planes=p) for p in (1, 0)}
    assert want[1].tobytes() != want[0].tobytes()
    saved = get_option("rh1_planes")
    try:
        e = _engine(c)
        for p in (1, 0, 1, 0):
            set_option("rh1_planes", p)
            assert e.fvp(c["v"], 0.0).tobytes() == want[p].tobytes(), f"rh1_planes={p} on a live engine"
        e.close()
    finally:
        set_option("rh1_planes", saved)
