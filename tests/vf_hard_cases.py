"""The hard cases of the value-function baseline: one table for tests/test_vf_hard_ref.py (CPU: the float32 oracle's
own error on every case, which shows the 1e-5 bar has room) and tests/test_gpu_vf_hard.py (GPU: the trpo_vf_* runtime
against the float64 oracle, per parameter block).  No GPU imports: trpo_amd is never loaded from here.

A case is (id, group, (n, obs, A, hidden), seed, builder); the builder returns obs, dist, y and theta as float32 and
starts as uint8.  The references of a case are computed once per process and shared.

  widths   hidden widths of 1, under 4, odd, one past a 32 / 64 / 128 tile, 128 exactly, above 128 in either layer
           (the 256-column f32 row tile and the split weight-gradient tiles), two full 256 tiles, 384 (a full and a
           partial 256 tile)
  rows     row counts around the head kernel's 16 rows per block, the split-K minimum of 64 rows, the 128 / 256 row
           tiles, at default and at odd widths; 69921 rows: 437 splits of 160 rows and a last split of one row
  regimes  dead units and exactly-zero pre-activations, targets at Pendulum's scale with long paths, observation
           columns spread over six decades; each at (64, 64) and at (256, 256)
"""
import functools
import math
from typing import Callable, NamedTuple

import numpy as np

from oracle import vf_oracle as V

BLOCK_NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")
ROW_EDGES = (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257)
ROW_EDGES_ODD = (1, 17, 129, 257)
N_DEAD = 4     # dead units per hidden layer of the "dead" regime


def vf_xavier_params(feat_dim, hidden=(64, 64), rng=None):
    """trpo_amd.vf.vf_xavier_params restated (that module loads the GPU library)."""
    rng = rng or np.random.RandomState(1)
    widths = [int(feat_dim), *[int(h) for h in hidden], 1]
    parts = []
    for a, b in zip(widths[:-1], widths[1:]):
        lim = math.sqrt(6.0 / (a + b))
        parts.append(rng.uniform(-lim, lim, size=a * b))
        parts.append(np.zeros(b))
    return np.concatenate(parts).astype(np.float32)


def block_bounds(F, hidden):
    """[(lo, hi)] of W1, b1, W2, b2, W3, b3 in the flat vector"""
    H1, H2 = hidden
    sizes = [F * H1, H1, H1 * H2, H2, H2, 1]
    ends = np.cumsum(sizes)
    return [(int(e - s), int(e)) for s, e in zip(sizes, ends)]


def blocks(flat, F, hidden):
    """a flat parameter-shaped vector as [W1, b1, W2, b2, W3, b3] (W row-major [fan_in][fan_out])"""
    flat = np.asarray(flat)
    H1, H2 = hidden
    bounds = block_bounds(F, hidden)
    assert flat.shape == (bounds[-1][1],)
    shapes = [(F, H1), (H1,), (H1, H2), (H2,), (H2, 1), (1,)]
    return [flat[lo:hi].reshape(s) for (lo, hi), s in zip(bounds, shapes)]


def assert_blocks_close(a, b, F, hidden, rel, what):
    """conftest.assert_vec_close on each block against that block's own norm and maximum; a block whose reference is
    all zero must be exactly zero."""
    from conftest import assert_vec_close
    for name, x, y in zip(BLOCK_NAMES, blocks(a, F, hidden), blocks(b, F, hidden)):
        if not np.any(y):
            assert np.array_equal(x, y), f"{what} {name}: the reference is zero, got max |x| {np.max(np.abs(x)):.3e}"
        else:
            assert_vec_close(x.ravel(), y.ravel(), rel, f"{what} {name}")


def block_errors(a, b, F, hidden):
    from conftest import rel_l2
    return {name: rel_l2(x, y) for name, x, y in zip(BLOCK_NAMES, blocks(a, F, hidden), blocks(b, F, hidden))}


# ---------------------------------------------------------------------------------------------- builders
def batch(n, obs, A, seed, path_len=37, extra_starts=5):
    """tests/test_gpu_vf.py::batch, y as float32"""
    rng = np.random.RandomState(seed)
    o = rng.standard_normal((n, obs)).astype(np.float32)
    d = rng.dirichlet(np.ones(A), n).astype(np.float32)
    starts = np.zeros(n, np.uint8)
    starts[::path_len] = 1
    if extra_starts:
        starts[rng.randint(0, n, extra_starts)] = 1
    y = (np.cumsum(rng.uniform(0, 1, n))[::-1].copy() % 20.0).astype(np.float32)
    return o, d, starts, y


def theta_for(F, hidden, seed):
    """Xavier weights, first-layer biases 0.05 (test_gpu_vf.py::net_for), second-layer biases 0.02 .. 0.06"""
    th = vf_xavier_params(F, hidden, np.random.RandomState(seed))
    (_, _), (b1lo, b1hi), (_, _), (b2lo, b2hi), _, _ = block_bounds(F, hidden)
    th[b1lo:b1hi] = 0.05
    th[b2lo:b2hi] = 0.02 + 0.01 * (np.arange(hidden[1]) % 5)
    return th


def _pack(o, d, starts, y, th):
    return {"obs": np.ascontiguousarray(o, np.float32), "dist": np.ascontiguousarray(d, np.float32),
            "starts": np.ascontiguousarray(starts, np.uint8), "y": np.ascontiguousarray(y, np.float32),
            "theta": np.ascontiguousarray(th, np.float32)}


def build_random(case):
    n, obs, A, hidden = case.shape
    o, d, starts, y = batch(n, obs, A, case.seed)
    return _pack(o, d, starts, y, theta_for(obs + A + 1, hidden, case.seed + 1))


def build_alive_1x1(case):
    """(1, 1): small positive weights under a bias of 0.5 keep the one unit of each layer alive on every row"""
    n, obs, A, hidden = case.shape
    assert tuple(hidden) == (1, 1)
    o, d, starts, y = batch(n, obs, A, case.seed)
    F = obs + A + 1
    th = np.concatenate([np.full(F, 0.01), [0.5], [0.7], [0.05], [0.9], [0.0]]).astype(np.float32)
    return _pack(o, d, starts, y, th)


def dead_units(hidden):
    """the units of each hidden layer that the "dead" regime kills"""
    H1, H2 = hidden
    return [1, 17, 40, H1 - 1], [0, 9, 33, H2 - 2]


def dead_mask(F, hidden):
    """flat boolean: the entries of W1, b1, W2, b2, W3 that belong to a dead unit (its incoming column, its bias,
    its outgoing row): zero in the gradient, hence untouched by Adam"""
    d1, d2 = dead_units(hidden)
    m = [np.zeros(s, bool) for s in [(F, hidden[0]), (hidden[0],), (hidden[0], hidden[1]), (hidden[1],),
                                     (hidden[1], 1), (1,)]]
    m[0][:, d1] = True
    m[1][d1] = True
    m[2][d1, :] = True
    m[2][:, d2] = True
    m[3][d2] = True
    m[4][d2, :] = True
    return np.concatenate([x.ravel() for x in m])


def build_dead(case):
    """A quarter of the rows are all-zero feature rows (zero obs and dist at a path start) under b1 = 0: their
    layer-1 pre-activations are exactly 0 in any precision.  Four units per hidden layer have bias -10 and weights
    scaled by 0.01: dead on every row."""
    n, obs, A, hidden = case.shape
    o, d, starts, y = batch(n, obs, A, case.seed)
    zero = np.arange(0, n, 4)
    o[zero] = 0.0
    d[zero] = 0.0
    starts[zero] = 1
    F = obs + A + 1
    th = theta_for(F, hidden, case.seed + 1)
    W1, b1, W2, b2, _, _ = blocks(th, F, hidden)      # views
    d1, d2 = dead_units(hidden)
    b1[:] = 0.0
    W1[:, d1] *= 0.01
    b1[d1] = -10.0
    W2[:, d2] *= 0.01
    b2[d2] = -10.0
    return _pack(o, d, starts, y, th)


def build_big_targets(case):
    """y in [-1500, 0] (Pendulum-v1 returns), paths of 1000 rows: t/10 reaches 99.9"""
    n, obs, A, hidden = case.shape
    o, d, starts, _ = batch(n, obs, A, case.seed, path_len=1000, extra_starts=0)
    y = (-1500.0 * np.random.RandomState(case.seed + 2).uniform(0, 1, n)).astype(np.float32)
    return _pack(o, d, starts, y, theta_for(obs + A + 1, hidden, case.seed + 1))


def build_col_scales(case):
    """observation column c multiplied by 10^(c mod 7 - 3)"""
    n, obs, A, hidden = case.shape
    o, d, starts, y = batch(n, obs, A, case.seed)
    o = (o * (10.0 ** (np.arange(obs) % 7 - 3))).astype(np.float32)
    return _pack(o, d, starts, y, theta_for(obs + A + 1, hidden, case.seed + 1))


# ---------------------------------------------------------------------------------------------- the table
class Case(NamedTuple):
    id: str
    group: str
    shape: tuple           # (n, obs, A, hidden)
    seed: int
    build: Callable

    @property
    def F(self):
        return self.shape[1] + self.shape[2] + 1

    @property
    def hidden(self):
        return self.shape[3]


def _hid(hidden):
    return f"h{hidden[0]}x{hidden[1]}"


def _case(group, n, obs, A, hidden, build=build_random, tag=None, seed=None):
    id_ = f"{tag or group}-{_hid(hidden)}-o{obs}a{A}n{n}"
    return Case(id_, group, (n, obs, A, tuple(hidden)), 7 * n + hidden[0] if seed is None else seed, build)


WIDTHS = [
    _case("widths", 513, 4, 2, (1, 1), build_alive_1x1),
    _case("widths", 300, 4, 2, (5, 3)),
    _case("widths", 1000, 11, 3, (17, 33)),
    _case("widths", 3001, 128, 18, (128, 128)),
    _case("widths", 1000, 11, 3, (65, 130)),
    _case("widths", 777, 128, 18, (129, 64)),
    _case("widths", 777, 4, 2, (64, 129)),
    _case("widths", 1029, 17, 6, (256, 256)),
    _case("widths", 513, 376, 17, (384, 132)),
]
ROWS = ([_case("rows", n, 4, 2, (64, 64)) for n in ROW_EDGES] +
        [_case("rows", n, 4, 2, (33, 65)) for n in ROW_EDGES_ODD] +
        [_case("rows", 69921, 4, 2, (64, 64))])
REGIMES = [c for hidden in ((64, 64), (256, 256)) for c in (
    _case("regimes", 1000, 11, 3, hidden, build_dead, "dead"),
    _case("regimes", 1003, 11, 3, hidden, build_big_targets, "big"),
    _case("regimes", 1001, 11, 3, hidden, build_col_scales, "cols"),
)]
CASES = WIDTHS + ROWS + REGIMES
BY_ID = {c.id: c for c in CASES}
IDS = [c.id for c in CASES]
assert len(BY_ID) == len(CASES)
DEAD_IDS = [c.id for c in REGIMES if c.build is build_dead]
# the cases whose hidden widths pass 128: they need the f32 row tiles for the VF's ReLU GEMMs (gemm.hip
# rowgemm_uses_split) and run the split weight-gradient tiles
WIDE_IDS = [c.id for c in CASES if max(c.hidden) > 128]


def case_id(hidden, group="widths"):
    """the one case of `group` with these widths"""
    (c,) = [c for c in CASES if c.group == group and c.hidden == tuple(hidden)]
    return c.id


@functools.lru_cache(maxsize=None)
def inputs(case_id_):
    c = BY_ID[case_id_]
    d = c.build(c)
    for a in d.values():
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def refs(case_id_):
    """{"feat", "g": (f64, f32), "loss": (f64, f32), "pred": (f64, f32)}: the oracle on the case's float32 inputs"""
    c = BY_ID[case_id_]
    d = inputs(case_id_)
    feat = V.features_concat_vec(d["obs"], d["dist"], d["starts"])
    g64, l64 = V.gradient(d["theta"].astype(np.float64), feat, d["y"], c.hidden)
    g32, l32 = V.gradient(d["theta"], feat, d["y"], c.hidden, np.float32)
    p64 = V.predict(d["theta"].astype(np.float64), feat, c.hidden)
    p32 = V.predict(d["theta"], feat, c.hidden, np.float32)
    out = {"feat": feat, "g": (g64, g32), "loss": (l64, l32), "pred": (p64, p32)}
    for v in (feat, g64, g32, p64, p32):
        v.setflags(write=False)
    return out


def float32_errors(case_id_):
    """{"g": {block: rel L2}, "pred": {"rel": .}, "loss": {"rel": .}}: the float32 oracle against the float64 one"""
    from conftest import rel_l2
    c = BY_ID[case_id_]
    r = refs(case_id_)
    return {"g": block_errors(r["g"][1], r["g"][0], c.F, c.hidden),
            "pred": {"rel": rel_l2(r["pred"][1], r["pred"][0])},
            "loss": {"rel": abs(r["loss"][1] - r["loss"][0]) / abs(r["loss"][0])}}
