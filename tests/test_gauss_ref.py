"""The diagonal-Gaussian reference (tests/gauss_ref.py) checked against itself, and the new surface without a
GPU.  CPU only.

1. the definition's closed forms (head deltas, g_s, the FVP) equal autodiff to 1e-12 at the five test shapes;
2. the float32 evaluation of the reference stays within 2.5e-6 of float64 on g and Hv (five shapes) and on
   stepdir, fullstep and theta of whole updates (the last four shapes), and within 2.5e-5 on kl: the GPU
   tests' 1e-5 bars, and their kl bar max(1e-5, 4 x this error) <= 1e-4, rest on these;
3. the new calls are bound, and Engine(dist="gaussian") without a GPU fails with the usual error.

(3, [8], 1, .) is left out of the whole updates on purpose: P = 41 is within reach of 10 CG iterations with
residual_tol = 0, where float32 CG is off by 1e-2.
"""
import numpy as np
import pytest
import torch

import gauss_ref as G
from conftest import rel_l2

SHAPE_IDS = ["o3h8a1n1", "o11h64x2a3n257", "o17h64x2a6n3001", "o128h256x2a17n515", "o24h32a33n70"]
# one seed per shape; if a float32 case misses its bar, change its seed here, not the bar
SEEDS = dict(zip(SHAPE_IDS, [0, 1, 2, 3, 4]))
UPDATE_SEEDS = dict(zip(SHAPE_IDS, [0, 11, 12, 14, 13]))

CASES = [pytest.param(s, id=i) for s, i in zip(G.SHAPES, SHAPE_IDS)]
UPDATE_CASES = CASES[1:]


def _id(shape):
    return SHAPE_IDS[G.SHAPES.index(shape)]


def _direction(spec, seed):
    return np.random.RandomState(1000 + seed).standard_normal(spec.n_params).astype(np.float32)


def _close(a, b, tol, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
    assert err <= tol, f"{what}: rel L2 {err:.3e} > {tol:.1e}"


@pytest.mark.parametrize("shape", CASES)
def test_closed_forms_equal_autodiff(shape):
    seed = SEEDS[_id(shape)]
    spec, theta, b = G.make_case(shape, seed)
    v = _direction(spec, seed)
    A = spec.act_dim
    # the FVP: reverse-over-reverse of KL_ff against R-forward / scaled head / backprop / 2 v_s n/N
    hv, hv_c = G.fvp(theta, b, v, spec), G.fvp_closed(theta, b, v, spec)
    _close(hv_c, hv, 1e-12, "Hv")
    _close(hv_c[-A:], hv[-A:], 1e-12, "Hv logstd block")
    # g and its logstd block
    g, g_c = G.policy_grad(theta, b, spec), G.policy_grad_closed(theta, b, spec)
    _close(g_c, g, 1e-12, "g")
    _close(g_c[-A:], g[-A:], 1e-12, "g_s")
    # the head deltas: d surr / d mu and d surr / d logstd by autograd over the head's outputs
    dt = torch.float64
    th = torch.as_tensor(theta, dtype=dt)
    mu = torch.as_tensor(G.mean_np(theta, b.X, spec), dtype=dt).requires_grad_(True)
    s = th[spec.n_net:].clone().requires_grad_(True)
    dmu, ds = torch.autograd.grad(G.losses_of_head(mu, s, b, dt)[0], [mu, s])
    ds_c, gs_c = G.head_deltas(theta, b, spec)
    _close(ds_c, dmu.numpy(), 1e-12, "DS_L")
    _close(gs_c, ds.numpy(), 1e-12, "g_s (head)")


@pytest.mark.parametrize("shape", CASES)
def test_float32_reference_error_g_hv_kl(shape):
    seed = SEEDS[_id(shape)]
    spec, theta, b = G.make_case(shape, seed)
    v = _direction(spec, seed)
    g64, g32 = G.policy_grad(theta, b, spec), G.policy_grad(theta, b, spec, torch.float32)
    hv64, hv32 = G.fvp(theta, b, v, spec), G.fvp(theta, b, v, spec, torch.float32)
    l64, l32 = G.losses(theta, b, spec), G.losses(theta, b, spec, torch.float32)
    kl_err = abs(float(l32[1]) - float(l64[1])) / abs(float(l64[1]))
    print(f"{_id(shape)}: g {rel_l2(g32, g64):.2e}  Hv {rel_l2(hv32, hv64):.2e}  kl {kl_err:.2e} (kl {l64[1]:.3e})")
    assert g32.dtype == np.float32 and hv32.dtype == np.float32 and l32.dtype == np.float32
    _close(g32, g64, 2.5e-6, "g float32 vs float64")
    _close(hv32, hv64, 2.5e-6, "Hv float32 vs float64")
    assert kl_err <= 2.5e-5, f"kl float32 vs float64: {kl_err:.3e}"


@pytest.mark.parametrize("shape", UPDATE_CASES)
def test_float32_reference_error_whole_update(shape):
    spec, theta, b = G.make_case(shape, UPDATE_SEEDS[_id(shape)], perturb=0.0)
    r64 = G.update(theta, b, spec, torch.float64, 10, 0.0)
    r32 = G.update(theta, b, spec, torch.float32, 10, 0.0)
    print(f"{_id(shape)}: stepdir {rel_l2(r32.stepdir, r64.stepdir):.2e}  fullstep "
          f"{rel_l2(r32.fullstep, r64.fullstep):.2e}  theta {rel_l2(r32.theta_new, r64.theta_new):.2e}  k {r64.k}")
    assert r32.stepdir.dtype == np.float32
    assert (r32.cg_iters, r32.k, r32.reverted) == (r64.cg_iters, r64.k, r64.reverted)
    _close(r32.stepdir, r64.stepdir, 2.5e-6, "stepdir float32 vs float64")
    _close(r32.fullstep, r64.fullstep, 2.5e-6, "fullstep float32 vs float64")
    _close(r32.theta_new, r64.theta_new, 2.5e-6, "theta float32 vs float64")


def test_gaussian_calls_are_bound():
    from trpo_amd import _lib
    for name in ("trpo_create_dist", "trpo_get_dist", "trpo_set_batch_gaussian", "trpo_action_mean",
                 "trpo_act_gaussian"):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert (_lib.DIST_CATEGORICAL, _lib.DIST_GAUSSIAN) == (0, 1)
    from trpo_amd import Engine
    for name in ("set_batch_gaussian", "action_mean", "act_gaussian", "dist"):
        assert hasattr(Engine, name)


def test_gaussian_engine_creation_reports_errors():
    """Without a GPU the creation fails with the usual engine error, not a crash; bad arguments are errors with
    or without one."""
    import ctypes
    from trpo_amd import Engine, _lib
    with pytest.raises(ValueError, match="dist must be one of"):
        Engine(3, [8], 1, max_rows=4, dist="beta")
    h = ctypes.c_void_p()
    hid = (ctypes.c_int * 1)(8)
    assert _lib.lib.trpo_create_dist(ctypes.byref(h), 7, 3, hid, 1, 1, 4, 0) == -1    # TRPO_ERR_ARG
    assert b"dist" in _lib.lib.trpo_last_error()
    assert _lib.lib.trpo_create_dist(ctypes.byref(h), _lib.DIST_GAUSSIAN, 3, hid, 1, 200, 4, 0) == -1
    assert b"act_dim" in _lib.lib.trpo_last_error()
    if _lib.device_count() < 1:
        with pytest.raises(_lib.EngineError, match="trpo_create_dist failed"):
            Engine(3, [8], 1, max_rows=4, dist="gaussian")
    else:
        with Engine(3, [8], 1, max_rows=4, dist="gaussian") as e:
            assert e.dist == "gaussian" and e.num_params == 3 * 8 + 8 + 8 + 1 + 1
