"""The CPU reference of the subsampled-Fisher update (tests/fvp_subsample_ref.py) against the oracle it is composed
from: at k = 1 it is the oracle's own update exactly, the row rule gives n_sub = ceil(n / k), F_sub is a symmetric
positive semi-definite matrix, and the float32 composition stays as close to float64 at k > 1 as at k = 1, which is
what lets tests/test_gpu_fvp_subsample.py hold the engine to the project's 1e-5 bar."""
import dataclasses

import numpy as np
import pytest
import torch

import fvp_subsample_ref as R
import gauss_ref as G
from conftest import rel_l2
from oracle import trpo_oracle as O


def _cat_case(obs, hidden, A, n, seed=5):
    spec = O.PolicySpec(obs, hidden, A)
    d = O.synthetic_batch(spec, n, seed=seed, steady_state=False, perturb=0.02)
    return spec, d["theta"], O.Batch(d["X"], d["actions"], d["advant"], d["old_dist"])


def _same(a, b):
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x, y), f.name
        else:
            assert x == y or (x != x and y != y), f.name


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_k1_is_the_oracle_update_categorical(dtype):
    spec, theta, batch = _cat_case(4, [64], 2, 1000)
    _same(R.categorical_update(theta, batch, spec, 1, dtype), O.trpo_update(theta, batch, spec, dtype))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_k1_is_the_reference_update_gaussian(dtype):
    spec, theta, b = G.make_case((3, [8], 1, 300), seed=3, perturb=0.0)
    _same(R.gaussian_update(theta, b, spec, 1, dtype), G.update(theta, b, spec, dtype))


@pytest.mark.parametrize("k", [2, 3, 5, 7])
def test_row_rule(k):
    for n in sorted({1, max(1, k - 1), k, k + 1, 2 * k - 1}):
        rows = np.arange(n)[::k]
        assert R.n_sub(n, k) == len(rows) == -(-n // k)
        assert np.array_equal(rows, [i for i in range(n) if i % k == 0])
        batch = O.Batch(np.arange(n, dtype=np.float32)[:, None], np.arange(n), np.arange(n, dtype=np.float64),
                        np.arange(n, dtype=np.float32)[:, None])
        s = R.sub_batch(batch, k)
        assert all(np.array_equal(np.ravel(x), rows) for x in (s.X, s.actions, s.advant, s.old_dist))


@pytest.mark.parametrize("k", [1, 3, 5])
def test_f_sub_symmetric_psd(k):
    spec, theta, batch = _cat_case(3, [5], 3, 41)
    F = R.fisher_matrix(theta, batch.X, spec, k)
    # KL_ff's Hessian at its own theta: symmetric and PSD up to the eps = 1e-6 of trpo_inksci.py:16 inside the logs
    scale = np.abs(F).max()
    assert np.abs(F - F.T).max() <= 1e-5 * scale
    assert np.linalg.eigvalsh(0.5 * (F + F.T)).min() >= -1e-5 * scale
    # and it is the mean over the sampled rows: the Fisher matrices of the rows' singletons average to it
    rows = np.arange(batch.X.shape[0])[::k]
    mean = sum(R.fisher_matrix(theta, batch.X[i:i + 1], spec, 1) for i in rows) / len(rows)
    assert np.abs(mean - F).max() <= 1e-12 * scale


@pytest.mark.parametrize("k", [2, 5])
def test_float32_composition_error(k):
    """float32 against float64 at k > 1 is no worse than at k = 1 (within 4x), and the CG counts agree: the 1e-5 bar
    is reachable for the engine."""
    spec, theta, batch = _cat_case(4, [64], 2, 1000)
    err = {}
    for kk in (1, k):
        r64 = R.categorical_update(theta, batch, spec, kk, np.float64)
        r32 = R.categorical_update(theta, batch, spec, kk, np.float32)
        assert r32.cg_iters == r64.cg_iters and r32.k == r64.k
        err[kk] = max(rel_l2(r32.g, r64.g), rel_l2(r32.stepdir, r64.stepdir), rel_l2(r32.fullstep, r64.fullstep))
        print(f"k={kk}: float32 vs float64 max rel error {err[kk]:.2e}")
    assert err[k] <= max(1e-5, 4.0 * err[1])


def test_subsample_changes_the_step():
    """k > 1 is a different estimator: same g, another stepdir."""
    spec, theta, batch = _cat_case(4, [64], 2, 1000)
    r1 = R.categorical_update(theta, batch, spec, 1)
    r5 = R.categorical_update(theta, batch, spec, 5)
    assert np.array_equal(r1.g, r5.g)
    assert rel_l2(r5.stepdir, r1.stepdir) > 1e-3
