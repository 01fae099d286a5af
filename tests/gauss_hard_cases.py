"""The hard cases of the diagonal-Gaussian engine: one table for tests/test_gauss_ref.py (CPU: the float32
reference's own error on every case, which founds the bars) and tests/test_gpu_gauss_hard.py (GPU: the engine
against float64 under those bars).  The references are computed once per case and process and shared.

A case is (id, group, (obs, hidden, A, n), regime, checks): checks a set of "losses", "vec" (g and Hv), "update".
The sizes are the smallest that still reach the path the case is named for:

  shapes   three hidden layers and odd widths; one hidden layer of a width that is no multiple of 32; widths under
           32 and one past a tile; obs <= 64 under 256-wide layers (fwd01 / X planes / rbwd0 with zero-filled
           plane blocks), also at one row; the C5 layer shapes (split weight gradients, 1024-wide row GEMMs)
  rows     (128, [256, 256], 17) at one state, one row pair, a partial 128-tile, a full 256-row plane tile + 1
  regimes  saturated tanh, 2^15 row spread, sigma = e^-5, 1/sigma^2 spread by e^12 across the columns
  colsum   the f64 column reduction of g's log-std block: 1 -> 2 blocks, all 256 blocks with more than 1024 rows
           per block and a short last block, and A = 128 (cw = 128, two row threads, three blocks, four head tiles)
"""
import functools
from typing import NamedTuple

import numpy as np

import gauss_ref as G

SEED = 7
COLSUM_BIG_N = 100000     # above it a colsum case is judged on g (whole and tail) and Hv's tail alone
C4G = (128, [256, 256], 17)


class Case(NamedTuple):
    id: str
    group: str
    shape: tuple
    regime: str
    checks: frozenset


def _c(id_, group, shape, regime="random", checks=("losses", "vec", "update")):
    return Case(id_, group, shape, regime, frozenset(checks))


NO_UPDATE = ("losses", "vec")
CASES = [
    _c("o11h64-48-32a3n257", "shapes", (11, [64, 48, 32], 3, 257)),
    _c("o23h100a5n130", "shapes", (23, [100], 5, 130)),
    _c("o40h17-33a2n65", "shapes", (40, [17, 33], 2, 65)),
    _c("o17h256x2a6n515", "shapes", (17, [256, 256], 6, 515)),
    _c("o17h256x2a6n1", "shapes", (17, [256, 256], 6, 1), checks=NO_UPDATE),
    _c("c5-n300", "shapes", (376, [1024, 1024], 17, 300)),
    _c("c4g-n1", "rows", (*C4G, 1), checks=NO_UPDATE),
    _c("c4g-n2", "rows", (*C4G, 2), checks=NO_UPDATE),
    _c("c4g-n129", "rows", (*C4G, 129), checks=NO_UPDATE),
    _c("c4g-n257", "rows", (*C4G, 257)),
    _c("o17h64x2a6-tanh20", "regimes", (17, [64, 64], 6, 515), "tanh20"),
    _c("o17h64x2a6-mixed", "regimes", (17, [64, 64], 6, 515), "mixed"),
    _c("c4g-tanh20", "regimes", (*C4G, 515), "tanh20"),
    _c("c4g-mixed", "regimes", (*C4G, 515), "mixed"),
    _c("o17h64x2a6-sigma_small", "regimes", (17, [64, 64], 6, 515), "sigma_small"),
    _c("c4g-sigma_spread", "regimes", (*C4G, 515), "sigma_spread"),
    _c("colsum-n1024", "colsum", (3, [8], 1, 1024), checks=("vec",)),
    _c("colsum-n1025", "colsum", (3, [8], 1, 1025), checks=("vec",)),
    _c("colsum-n262145", "colsum", (3, [8], 1, 262145), checks=("vec",)),
    _c("colsum-n300001", "colsum", (3, [8], 1, 300001), checks=("vec",)),
    _c("colsum-a128n2100", "colsum", (5, [16], 128, 2100), checks=("vec",)),
]
BY_ID = {c.id: c for c in CASES}
IDS = [c.id for c in CASES]
UPDATE_IDS = [c.id for c in CASES if "update" in c.checks]
# SEED everywhere, except where its float32 reference sits within a quarter of the firm bound of
# tests/test_gauss_ref.py (2.5e-6; kl 2.5e-5) or just over it, or where float32 and float64 disagree on cg_iters /
# k / reverted: there another seed is chosen for that feed, never another bar.  At (11, [64, 48, 32], 3) and
# (17, [256, 256], 6) every seed from 1 to 14 leaves the update's stepdir at 0.75 of the bound or above; they take
# the lowest.
SEED_OVERRIDES = {
    "feed": {"o11h64-48-32a3n257": 2, "o40h17-33a2n65": 4, "c5-n300": 9, "c4g-n1": 4, "c4g-n129": 9, "c4g-n257": 3,
             "c4g-mixed": 13, "colsum-n262145": 4},
    "update": {"o11h64-48-32a3n257": 1, "o40h17-33a2n65": 5, "o17h256x2a6n515": 8, "c5-n300": 9,
               "o17h64x2a6-tanh20": 12, "o17h64x2a6-sigma_small": 9, "c4g-sigma_spread": 2},
}


def seed_of(case_id, kind):
    return SEED_OVERRIDES[kind].get(case_id, SEED)


@functools.lru_cache(maxsize=None)
def feed(case_id):
    """(spec, theta, batch) of the loss / g / Hv checks: theta_old = theta perturbed by 2 %."""
    c = BY_ID[case_id]
    return G.make_hard_case(c.shape, c.regime, seed_of(case_id, "feed"), perturb=0.02)


@functools.lru_cache(maxsize=None)
def update_feed(case_id):
    """(spec, theta, batch) of the whole update: theta_old = theta."""
    c = BY_ID[case_id]
    return G.make_hard_case(c.shape, c.regime, seed_of(case_id, "update"), perturb=0.0)


def direction(spec):
    return np.random.RandomState(77).standard_normal(spec.n_params).astype(np.float32)


@functools.lru_cache(maxsize=None)
def vec_refs(case_id):
    """{"v", "g": (f64, f32), "hv": (f64, f32)}: the policy gradient and the undamped Hv in both precisions"""
    import torch
    spec, theta, b = feed(case_id)
    v = direction(spec)
    return {"v": v,
            "g": tuple(G.policy_grad(theta, b, spec, dt) for dt in (torch.float64, torch.float32)),
            "hv": tuple(G.fvp(theta, b, v, spec, dt) for dt in (torch.float64, torch.float32))}


@functools.lru_cache(maxsize=None)
def update_refs(case_id):
    """(float64 update, float32 update) with cg_iters = 10 and residual_tol = 0"""
    import torch
    spec, theta, b = update_feed(case_id)
    return tuple(G.update(theta, b, spec, dt, 10, 0.0) for dt in (torch.float64, torch.float32))


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def block_errors(got, ref, spec):
    """{block name: rel L2 against the block's own norm} over W_l, b_l, logstd, and "all" for the whole vector"""
    from conftest import rel_l2
    out = {name: rel_l2(got[sl], ref[sl]) for name, sl in G.block_slices(spec)}
    out["all"] = rel_l2(got, ref)
    return out


def float32_errors(case_id):
    """{quantity: {block: the float32 reference's error against float64}} over the case's checks; scalars have
    the one block "rel".  The quantities: g, Hv, kl, and of the update stepdir, fullstep, theta, shs, lm, rate."""
    c = BY_ID[case_id]
    spec, theta, b = feed(case_id)
    out = {}
    if "vec" in c.checks:
        r = vec_refs(case_id)
        out["g"] = block_errors(r["g"][1], r["g"][0], spec)
        out["Hv"] = block_errors(r["hv"][1], r["hv"][0], spec)
        if c.shape[3] > COLSUM_BIG_N:
            # the column reduction's edges: g whole and its tail entry, Hv's tail (the network blocks at these n
            # are float32 sums over 3e5 rows, whose order and error follow the BLAS's thread count)
            out["g"] = {k: out["g"][k] for k in ("logstd", "all")}
            out["Hv"] = {"logstd": out["Hv"]["logstd"]}
    if "losses" in c.checks:
        import torch
        l64, l32 = G.losses(theta, b, spec, torch.float64), G.losses(theta, b, spec, torch.float32)
        out["kl"] = {"rel": rel(l32[1], l64[1])}
    if "update" in c.checks:
        r64, r32 = update_refs(case_id)
        for name in ("stepdir", "fullstep"):
            out[name] = block_errors(getattr(r32, name), getattr(r64, name), spec)
        out["theta"] = block_errors(r32.theta_new, r64.theta_new, spec)
        for name in ("shs", "lm", "rate"):
            out[name] = {"rel": rel(getattr(r32, name), getattr(r64, name))}
    return out
