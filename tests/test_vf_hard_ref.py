"""CPU check of the VF hard cases themselves (tests/vf_hard_cases.py): conditions on the inputs, not measurements of
the kernels.  On every case the float32 oracle, with its own summation order and its own ReLU-mask flips, sits within
a quarter of the GPU bar per parameter block (2.5e-6 against 1e-5), so a GPU result outside 1e-5 is the runtime's
error, not float32's; every block and prediction is non-zero, and what the "dead" regime promises to be exactly zero
is.  `python tests/test_vf_hard_ref.py` rewrites profiles/vf_hard/ref_f32.txt from the same figures."""
import os
import sys

import numpy as np
import pytest

from conftest import assert_vec_close, rel_l2      # first: puts the repository root on sys.path
import vf_hard_cases as H
from oracle import vf_oracle as V

QUARTER = 2.5e-6


def test_table_holds_the_cases_of_the_plan():
    shapes = [c.shape for c in H.WIDTHS]
    assert shapes == [(513, 4, 2, (1, 1)), (300, 4, 2, (5, 3)), (1000, 11, 3, (17, 33)), (3001, 128, 18, (128, 128)),
                      (1000, 11, 3, (65, 130)), (777, 128, 18, (129, 64)), (777, 4, 2, (64, 129)),
                      (1029, 17, 6, (256, 256)), (513, 376, 17, (384, 132))]
    rows = {(c.shape[0], c.hidden) for c in H.ROWS}
    assert rows == ({(n, (64, 64)) for n in (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 69921)} |
                    {(n, (33, 65)) for n in (1, 17, 129, 257)})
    assert all(c.shape[1:3] == (4, 2) for c in H.ROWS)
    assert sorted((c.id.split("-")[0], c.hidden) for c in H.REGIMES) == sorted(
        (r, h) for r in ("dead", "big", "cols") for h in ((64, 64), (256, 256)))
    assert set(H.WIDE_IDS) >= {H.case_id(h) for h in ((65, 130), (129, 64), (64, 129), (256, 256), (384, 132))}


def test_blocks_split_and_per_block_bar():
    F, hidden = 7, (5, 3)
    P = F * 5 + 5 + 5 * 3 + 3 + 3 + 1
    flat = np.arange(P, dtype=np.float64) + 1.0
    bl = H.blocks(flat, F, hidden)
    assert [b.shape for b in bl] == [(7, 5), (5,), (5, 3), (3,), (3, 1), (1,)]
    assert np.array_equal(np.concatenate([b.ravel() for b in bl]), flat)
    assert H.block_bounds(F, hidden)[-1] == (P - 1, P)
    # an error in a small block that the whole-vector bar cannot see: b3 dominates max|g| and the norm
    ref = np.full(P, 1e-3)
    ref[-1] = 1e3
    got = ref.copy()
    got[:F * 5] *= 1.0 + 1e-3
    assert_vec_close(got, ref, 1e-5, "whole vector")
    with pytest.raises(AssertionError, match="W1"):
        H.assert_blocks_close(got, ref, F, hidden, 1e-5, "per block")
    # a zero reference block must be matched exactly
    ref[F * 5:F * 5 + 5] = 0.0
    got = ref.copy()
    H.assert_blocks_close(got, ref, F, hidden, 1e-5, "zero block")
    got[F * 5] = 1e-30
    with pytest.raises(AssertionError, match="b1"):
        H.assert_blocks_close(got, ref, F, hidden, 1e-5, "zero block")


def test_xavier_restated_matches_the_package_source():
    """vf_hard_cases restates trpo_amd.vf.vf_xavier_params (importing it would load the GPU library): same text"""
    import inspect
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "trpo_amd", "vf.py")).read()
    body = re.search(r"def vf_xavier_params\(.*?\n(    rng = rng or.*?astype\(np\.float32\))", src, re.S).group(1)
    mine = inspect.getsource(H.vf_xavier_params)
    assert body in mine


def test_features_concat_vec_equals_the_loop():
    rng = np.random.RandomState(5)
    n = 10000
    o = rng.standard_normal((n, 3)).astype(np.float32)
    d = rng.dirichlet(np.ones(2), n).astype(np.float32)
    for first in (1, 0):
        starts = (rng.uniform(size=n) < 0.01).astype(np.uint8)
        starts[0] = first
        starts[1:40] = 0          # first = 0: rows before the first start count from row 0
        assert np.array_equal(V.features_concat_vec(o, d, starts), V.features_concat(o, d, starts))


@pytest.mark.parametrize("case", H.IDS)
def test_float32_oracle_within_a_quarter_of_the_bar(case):
    c = H.BY_ID[case]
    r = H.refs(case)
    errs = H.float32_errors(case)
    print(_line(case, errs))
    g64, g32 = r["g"]
    assert g32.dtype == np.float32 and g64.dtype == np.float64
    H.assert_blocks_close(g32, g64, c.F, c.hidden, QUARTER, f"{case} float32 gradient")
    assert_vec_close(r["pred"][1], r["pred"][0], QUARTER, f"{case} float32 predict")
    assert errs["loss"]["rel"] <= QUARTER
    # nothing degenerate: every block and the prediction carry signal
    assert np.linalg.norm(r["pred"][0]) > 0
    for name, b in zip(H.BLOCK_NAMES, H.blocks(g64, c.F, c.hidden)):
        assert np.linalg.norm(b) > 0, f"{case}: block {name} of the reference gradient is zero"


@pytest.mark.parametrize("case", H.DEAD_IDS)
def test_dead_regime_is_what_it_says(case):
    c = H.BY_ID[case]
    d = H.inputs(case)
    r = H.refs(case)
    d1, d2 = H.dead_units(c.hidden)
    assert len(d1) == len(set(d1)) == H.N_DEAD and len(d2) == len(set(d2)) == H.N_DEAD
    zero_rows = np.arange(0, c.shape[0], 4)
    assert not r["feat"][zero_rows].any() and len(zero_rows) == c.shape[0] // 4
    alive1 = np.setdiff1d(np.arange(c.hidden[0]), d1)
    for dt in (np.float32, np.float64):
        W1, b1, W2, b2, _, _ = H.blocks(d["theta"].astype(dt), c.F, c.hidden)
        pre1 = r["feat"].astype(dt) @ W1 + b1
        assert np.array_equal(pre1[np.ix_(zero_rows, alive1)], np.zeros((len(zero_rows), len(alive1))))
        z1 = np.maximum(pre1, 0)
        pre2 = z1 @ W2 + b2
        assert (pre1[:, d1] < -5).all() and (pre2[:, d2] < -5).all()      # dead on every row, far from a flip
        assert (z1[:, alive1] > 0).mean() > 0.2                            # and the rest is not
    mask = H.dead_mask(c.F, c.hidden)
    for g in r["g"]:
        assert not g[mask].any()                 # exactly zero in float64 and in float32
        assert (g[~mask] != 0).mean() > 0.9
    # the zero rows still pass gradient to b2 / W3 through relu(b2) > 0, and none to b1: the ReLU mask is `> 0`
    _, _, _, b2, _, _ = H.blocks(d["theta"], c.F, c.hidden)
    assert (b2[np.setdiff1d(np.arange(c.hidden[1]), d2)] > 0).all()


def _line(case, errs):
    return (f"{case} g: " + "  ".join(f"{k} {v:.2e}" for k, v in errs["g"].items()) +
            f"  | pred {errs['pred']['rel']:.2e}  loss {errs['loss']['rel']:.2e}")


def fit_float32_errors(steps=3):
    """the float32 oracle's `steps`-step fit against the float64 one, on the cases of the GPU fit test"""
    out = {}
    for hidden in ((17, 33), (65, 130), (256, 256)):
        case = H.case_id(hidden)
        c, d, r = H.BY_ID[case], H.inputs(case), H.refs(case)
        th64, _ = V.fit(d["theta"].astype(np.float64), r["feat"], d["y"], steps, c.hidden)
        th32, _ = V.fit(d["theta"], r["feat"], d["y"], steps, c.hidden, np.float32)
        out[case] = (rel_l2(th32, th64),
                     rel_l2(V.predict(th32, r["feat"], c.hidden, np.float32), V.predict(th64, r["feat"], c.hidden)))
    return out


def test_float32_three_step_fit_theta_within_a_quarter_of_the_bar():
    """Three Adam steps in float32 stay within 2.5e-6 of float64 on theta.  The predictions at these near-initial
    parameters are sums that cancel, so the same theta error shows larger on them (6e-6 at (65, 130)); their figures
    are recorded in profiles/vf_hard/ref_f32.txt beside the GPU fit test's bar, not asserted here."""
    for case, (eth, epred) in fit_float32_errors().items():
        print(f"{case} fit(3): theta {eth:.2e}  pred {epred:.2e}")
        assert eth <= QUARTER, (case, eth)


def write_ref_f32(path):
    with open(path, "w") as f:
        for case in H.IDS:
            f.write(_line(case, H.float32_errors(case)) + "\n")
        for case, (eth, epred) in fit_float32_errors().items():
            f.write(f"{case} fit(3): theta {eth:.2e}  pred {epred:.2e}\n")


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = os.path.join(root, "profiles", "vf_hard", "ref_f32.txt")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    write_ref_f32(sys.argv[1] if len(sys.argv) > 1 else out)
