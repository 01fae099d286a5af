"""CPU checks behind the truncation tests: the shared fixture holds both kinds of path end (so the GPU tests
cannot pass vacuously), and the C-ABI declares the entries that expose them."""
import numpy as np

import truncation_ref as T
from test_abi import header_functions


def test_shared_inputs_have_both_kinds_of_end():
    out, e = T.oracle()
    assert len(out["rewards"]) == 1258 and len(e["truncated"]) == 75
    n_trunc = int(e["truncated"].sum())
    assert n_trunc >= 10 and len(e["truncated"]) - n_trunc >= 10
    assert (n_trunc, len(e["truncated"]) - n_trunc) == (24, 51)
    # only the time limit of 20 cuts a path off here
    assert np.all(e["lengths"][e["truncated"] == 1] == 20)
    assert np.all(e["lengths"] <= 20)
    # the records are consistent with the rollout
    assert np.array_equal(e["end_rows"], np.cumsum(e["lengths"]) - 1)
    assert e["end_rows"][-1] == len(out["rewards"]) - 1
    assert np.all(e["final_dist"][e["truncated"] == 0] == 0.0)
    np.testing.assert_allclose(e["final_dist"][e["truncated"] == 1].sum(axis=1), 1.0, atol=1e-6)


def test_max_pathlength_truncates_in_the_oracle():
    out, e = T.oracle(max_pathlength=12, time_limit=200)
    # 96 paths reach step 12; 7 of them terminate on that very step and count as terminated
    assert len(e["truncated"]) == 104 and int(e["truncated"].sum()) == 89
    assert np.all(e["lengths"][e["truncated"] == 1] == 12)
    assert int(((e["lengths"] == 12) & (e["truncated"] == 0)).sum()) == 7


def test_header_declares_the_truncation_api():
    names = header_functions()
    for must in ("trpo_rollout_fetch_ends", "trpo_get_tail_view", "trpo_vf_predict_tails", "trpo_get_tail_values"):
        assert must in names, must
