"""The sequential GAE(lambda) reference (tests/gae_ref.py) against hand-worked numbers and the identities
of the definition, and the argument checks of the C-ABI that need no GPU."""
import ctypes

import numpy as np

from gae_ref import gae_ref


def test_hand_worked_two_paths():
    """5 rows, paths [0..2] and [3..4], gamma = 0.5, lambda = 0.5 (binary fractions: every step is exact).
    Path 1 ends on a termination (no tail value), path 2 is cut off with V(s_T) = 4."""
    r = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    v = np.array([2.0, 4.0, 6.0, 8.0, 10.0])
    starts = np.array([1, 0, 0, 1, 0], np.uint8)
    tail = np.array([99.0, 99.0, 0.0, 99.0, 4.0])     # only rows 2 and 4 (path ends) are read
    A, R, D = gae_ref(r, v, 0.5, 0.5, starts, tail)
    # delta: row 4: 5 + .5*4 - 10 = -3 ; row 3: 4 + .5*10 - 8 = 1 ; row 2: 3 + 0 - 6 = -3 ;
    #        row 1: 2 + .5*6 - 4 = 1 ; row 0: 1 + .5*4 - 2 = 1
    assert D.tolist() == [1.0, 1.0, -3.0, 1.0, -3.0]
    # A (gamma*lambda = .25): A4 = -3 ; A3 = 1 - .75 = .25 ; A2 = -3 ; A1 = 1 - .75 = .25 ; A0 = 1 + .0625
    assert A.tolist() == [1.0625, 0.25, -3.0, 0.25, -3.0]
    # R: R4 = 5 + .5*4 = 7 ; R3 = 4 + 3.5 = 7.5 ; R2 = 3 ; R1 = 2 + 1.5 = 3.5 ; R0 = 1 + 1.75 = 2.75
    assert R.tolist() == [2.75, 3.5, 3.0, 7.5, 7.0]
    # without tail values the cut-off path bootstraps from 0
    A0, R0, D0 = gae_ref(r, v, 0.5, 0.5, starts)
    assert D0.tolist() == [1.0, 1.0, -3.0, 1.0, -5.0] and R0.tolist() == [2.75, 3.5, 3.0, 6.5, 5.0]
    assert A0.tolist() == [1.0625, 0.25, -3.0, -0.25, -5.0]


def _inputs(n, p_start, seed=0):
    rng = np.random.RandomState(seed)
    r = rng.uniform(0, 1, n)
    v = 10.0 * rng.standard_normal(n)
    starts = (rng.uniform(size=n) < p_start).astype(np.uint8)
    starts[0] = 1
    tail = 10.0 * rng.standard_normal(n)
    return r, v, starts, tail


def test_lambda_zero_is_delta_bitwise():
    r, v, starts, tail = _inputs(1000, 0.02)
    for tv in (None, tail):
        A, _, D = gae_ref(r, v, 0.99, 0.0, starts, tv)
        assert np.array_equal(A, D)


def test_lambda_one_is_returns_minus_values():
    """The deltas telescope: sum_k gamma^k delta_{t+k} = R_t - V_t when every path bootstraps from 0.  Each
    step of either side rounds at most 3 times at magnitude <= max|V| + max|R| ~ 150, damped by gamma:
    <= 3 u 150 / (1 - gamma) ~ 5e-12 in the worst case here; the bar is 1e-11."""
    r, v, starts, _ = _inputs(5000, 0.01, seed=1)
    A, R, _ = gae_ref(r, v, 0.99, 1.0, starts)
    assert np.max(np.abs(A - (R - v))) <= 1e-11


def test_zero_values_is_discount_bitwise():
    from oracle.trpo_oracle import discount_segmented
    r, _, starts, _ = _inputs(3000, 0.01, seed=2)
    for gamma, lam in ((0.95, 0.97), (0.99, 1.0), (0.95, 0.0)):
        A, R, _ = gae_ref(r, None, gamma, lam, starts)
        assert np.array_equal(A, discount_segmented(r, starts, gamma * lam))
        assert np.array_equal(R, discount_segmented(r, starts, gamma))


def test_set_advantage_estimator_rejects_bad_arguments():
    """kind and lambda are checked before the engine is touched, so no GPU (and no engine) is needed."""
    from trpo_amd import _lib
    lib = _lib.lib
    for kind, lam, word in ((_lib.ADV_GAE, -0.1, b"lambda"), (_lib.ADV_GAE, 1.5, b"lambda"),
                            (_lib.ADV_GAE, float("nan"), b"lambda"), (7, 0.5, b"kind")):
        rc = lib.trpo_set_advantage_estimator(None, kind, lam)
        assert rc == -1, (kind, lam, rc)                       # TRPO_ERR_ARG
        assert word in lib.trpo_last_error(), (kind, lam, lib.trpo_last_error())
    # valid arguments get as far as the engine check
    assert lib.trpo_set_advantage_estimator(None, _lib.ADV_GAE, 0.95) == -1
    assert b"engine" in lib.trpo_last_error()


def test_trpo_gae_empty_succeeds():
    from trpo_amd import _lib
    assert _lib.lib.trpo_gae(None, None, None, None, 0, 0.99, 0.95, None, None, _lib.MEM_HOST) == 0
    out = np.full(3, 7.0)
    ptr = out.ctypes.data_as(ctypes.c_void_p)
    assert _lib.lib.trpo_gae(ptr, None, None, None, 0, 0.99, 0.95, ptr, ptr, _lib.MEM_HOST) == 0
    assert np.all(out == 7.0)
