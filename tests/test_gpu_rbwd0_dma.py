"""rbwd0.hip's k-loop with the weight planes by LDS-DMA (option rbwd0_bdma) against the register-staged form.

The DMA form moves the same pre-split planes into the same LDS image and runs the same products in the same order,
so Engine.fvp and the policy gradient must be bit-identical between rbwd0_bdma = 1 and 0.  What can go wrong is
the copy itself (the swizzle folded into the source offsets, the zero fill past Npad and past ldk), the ring
(three slots against a loop unrolled by two, wrap across the tiles of one workgroup, the X image taking the ring's
bytes after the k-loop) and the wait counts; each shows as different bits.

Shapes: the C4 layers (K = 256: 8 k-tiles per segment, every column real); (20, [160, 168], 5): 160 columns, so
three of the eight waves copy only zeros, K = 168 leaves a partial sixth k-tile (ldk = 176: chunks 2 and 3 of
it are past the plane row); (20, [160, 136], 5): five k-tiles, an odd count, so the policy gradient's one-segment
loop ends on the first half of its unrolled pair and the plane-tile form never runs.
Rows: one, one pair, a tile less one, a whole tile, a tile and one, many tiles; and 1000 rows in two split-K
slabs, where one workgroup loops over four tiles.  low_seg at its default (one-product tiles where the test
fires) and 0 (three products everywhere).
"""
import numpy as np
import pytest

from oracle import trpo_oracle as O

pytestmark = pytest.mark.gpu

SPECS = {
    "c4": O.PolicySpec(128, [256, 256], 18),
    "k168": O.PolicySpec(20, [160, 168], 5),
    "k136": O.PolicySpec(20, [160, 136], 5),
}
ROWS = [(1, 0), (2, 0), (127, 0), (128, 0), (129, 0), (1000, 0), (1000, 2)]   # (n, option splits)


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


_CASES = {}


def _case(name, n):
    if (name, n) not in _CASES:
        spec = SPECS[name]
        dd = O.synthetic_batch(spec, n, seed=41)
        v = np.random.RandomState(42).standard_normal(spec.n_params).astype(np.float32)
        _CASES[name, n] = dict(theta=dd["theta"].astype(np.float32), X=dd["X"].astype(np.float32), v=v,
                               actions=dd["actions"], advant=dd["advant"].astype(np.float32), old=dd["old_dist"])
    return _CASES[name, n]


def _hv_and_g(name, n, **opts):
    """(Engine.fvp(v, 0), policy gradient) of a fresh engine under the options."""
    from trpo_amd import Engine
    spec, c = SPECS[name], _case(name, n)
    with _Options(**opts):
        e = Engine(spec.obs_dim, spec.hidden, spec.n_actions, max_rows=n)
        e.set_flat(c["theta"])
        e.set_batch(c["X"], c["actions"], c["advant"], c["old"])
        out = (e.fvp(c["v"], 0.0), e.policy_grad())
        e.close()
    return out


@pytest.mark.parametrize("n,splits", ROWS, ids=[f"n{n}" + (f"-splits{s}" if s else "") for n, s in ROWS])
@pytest.mark.parametrize("name", list(SPECS))
def test_bdma_bit_identical(gpu_available, name, n, splits):
    from trpo_amd._lib import get_option
    assert get_option("rbwd0_bdma") in (0, 1)
    for low_seg in (get_option("low_seg"), 0):
        hv1, g1 = _hv_and_g(name, n, rbwd0_bdma=1, low_seg=low_seg, splits=splits)
        hv0, g0 = _hv_and_g(name, n, rbwd0_bdma=0, low_seg=low_seg, splits=splits)
        assert np.all(np.isfinite(hv0)) and np.all(np.isfinite(g0))
        assert hv1.tobytes() == hv0.tobytes(), f"{name} n={n} splits={splits} low_seg={low_seg}: Hv differs"
        assert g1.tobytes() == g0.tobytes(), f"{name} n={n} splits={splits} low_seg={low_seg}: g differs"


@pytest.mark.parametrize("name", list(SPECS))
def test_shape_runs_the_fused_kernel(gpu_available, name):
    """The comparison above is about rbwd0.hip only where the engine takes it: without it (per-layer launches,
    another summation order) the W_0 block of Hv has other bits."""
    hv1, _ = _hv_and_g(name, 1000, rbwd0=1)
    hv0, _ = _hv_and_g(name, 1000, rbwd0=0)
    spec = SPECS[name]
    w0 = slice(0, spec.obs_dim * spec.hidden[0])
    assert hv1[w0].tobytes() != hv0[w0].tobytes()
