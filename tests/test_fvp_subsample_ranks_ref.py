"""fvp_subsample over ranks, by global row index (trpo_set_fvp_subsample_global, include/trpo_engine.h), on the CPU.

  * trpo_amd.dist.fisher_rows (phase, n_sub) against brute force, and over tilings of [0, N): the shards' Fisher rows
    are exactly range(0, N, k), so sum_r n_sub_r = ceil(N / k) with no exchange between the ranks;
  * the estimator: sum_r (n_sub_r / N_sub) F_r v over a tiling equals the whole batch's F_sub v in float64, which pins
    the 1 / N_sub scaling the engine applies to a shard's partial.
"""
import numpy as np
import pytest

import fvp_subsample_ref as R
from oracle import trpo_oracle as O
from trpo_amd.dist import fisher_rows


def test_fisher_rows_brute_force():
    for k in range(1, 10):
        for n in range(1, 41):
            for off in range(0, 21):
                rows = [i for i in range(n) if (off + i) % k == 0]
                phase, ns = fisher_rows(n, off, k)
                assert ns == len(rows), (k, n, off)
                assert phase == (k - off % k) % k, (k, n, off)
                if rows:
                    assert phase == rows[0] and rows == list(range(phase, n, k)), (k, n, off)
                else:
                    assert phase >= n, (k, n, off)


def test_fisher_rows_offset_zero_is_the_local_mode():
    for k in range(1, 10):
        for n in range(1, 41):
            assert fisher_rows(n, 0, k) == (0, R.n_sub(n, k))


def test_fisher_rows_tilings():
    rng = np.random.RandomState(0)
    for _ in range(400):
        N = int(rng.randint(1, 200))
        k = int(rng.randint(1, 10))
        shards = int(rng.randint(1, 6))
        cuts = sorted(int(c) for c in rng.randint(0, N + 1, shards - 1))
        bounds = [0, *cuts, N]
        rows, total = [], 0
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            phase, ns = fisher_rows(hi - lo, lo, k)
            rows += list(range(lo + phase, hi, k))
            assert len(range(lo + phase, hi, k)) == ns, (N, k, bounds)
            total += ns
        assert rows == list(range(0, N, k)), (N, k, bounds)
        assert total == -(-N // k), (N, k, bounds)


def test_fisher_rows_rejects_bad_arguments():
    for args in ((5, 0, 0), (-1, 0, 2), (5, -1, 2)):
        with pytest.raises(ValueError):
            fisher_rows(*args)


@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("cut", [40, 41])
def test_sharded_reference_equals_whole(k, cut):
    spec = O.PolicySpec(11, [8], 3)
    N = 103
    d = O.synthetic_batch(spec, N, seed=5)
    theta = d["theta"].astype(np.float64)
    X = d["X"]
    v = np.random.RandomState(2).standard_normal(spec.n_params)
    whole = O.fvp_undamped(theta, X[::k], v, spec)
    N_sub = R.n_sub(N, k)
    acc = np.zeros(spec.n_params)
    count = 0
    for lo, hi in ((0, cut), (cut, N)):
        phase, ns = fisher_rows(hi - lo, lo, k)
        assert ns > 0
        Xr = X[lo:hi][phase::k]
        assert Xr.shape[0] == ns
        acc += (ns / N_sub) * O.fvp_undamped(theta, Xr, v, spec)
        count += ns
    assert count == N_sub
    err = np.linalg.norm(acc - whole) / np.linalg.norm(whole)
    assert err <= 1e-12, err
