"""Torch reference of the diagonal-Gaussian policy update as include/trpo_engine.h defines it
(TRPO_DIST_GAUSSIAN): the losses, the policy gradient by autograd of surr, the FVP by reverse-over-reverse of
KL_ff, the closed forms beside them, and the whole update on oracle.trpo_oracle's conjugate_gradient and
linesearch with the step scaling and revert check of trpo_inksci.py:147-158.

Everything takes a torch `dtype`: float64 is the reference, float32 the same code at the engine's precision
(its own error is what the GPU tests' bars are measured against).

Flat layout: [W1, b1, ..., WL, bL, logstd], W_l row-major [fan_in][fan_out]; the last layer is linear (the
mean), the hidden layers tanh.
"""
from dataclasses import dataclass
from typing import List

import numpy as np
import torch

from oracle.trpo_oracle import conjugate_gradient, linesearch

HALF_LOG_2PIE = 0.5 * float(np.log(2.0 * np.pi * np.e))

# (obs, hidden, A, n): the smallest shapes that reach every code path of the engine
SHAPES = [(3, [8], 1, 1), (11, [64, 64], 3, 257), (17, [64, 64], 6, 3001), (128, [256, 256], 17, 515),
          (24, [32], 33, 70)]


@dataclass
class GaussSpec:
    obs_dim: int
    hidden: List[int]
    act_dim: int

    @property
    def widths(self):
        return [self.obs_dim, *self.hidden, self.act_dim]

    @property
    def n_net(self):
        w = self.widths
        return sum(w[i] * w[i + 1] + w[i + 1] for i in range(len(w) - 1))

    @property
    def n_params(self):
        return self.n_net + self.act_dim


@dataclass
class GaussBatch:
    X: np.ndarray            # [n, obs] float32
    actions: np.ndarray      # [n, A] float32
    advant: np.ndarray       # [n] float32
    old_mean: np.ndarray     # [n, A] float32
    old_logstd: np.ndarray   # [A] float32
    n_global: int = 0        # 0: the batch's own rows

    @property
    def N(self):
        return self.n_global or self.X.shape[0]

    def rows(self, lo, hi, n_global):
        return GaussBatch(self.X[lo:hi], self.actions[lo:hi], self.advant[lo:hi], self.old_mean[lo:hi],
                          self.old_logstd, n_global)


def _t(x, dtype):
    return torch.as_tensor(np.asarray(x), dtype=dtype)


def unflatten(theta, spec):
    """theta (torch, flat) -> ([(W, b), ...], logstd) as views."""
    w = spec.widths
    out, off = [], 0
    for i in range(len(w) - 1):
        W = theta[off:off + w[i] * w[i + 1]].reshape(w[i], w[i + 1])
        off += w[i] * w[i + 1]
        b = theta[off:off + w[i + 1]]
        off += w[i + 1]
        out.append((W, b))
    return out, theta[off:off + spec.act_dim]


def _forward(theta, X, spec):
    """-> (hidden activations [X, H1, ...], mean, logstd)"""
    layers, s = unflatten(theta, spec)
    hs, h = [X], X
    for i, (W, b) in enumerate(layers):
        z = h @ W + b
        if i + 1 < len(layers):
            h = torch.tanh(z)
            hs.append(h)
    return hs, z, s


def mean_np(theta, X, spec, dtype=torch.float64):
    with torch.no_grad():
        return _forward(_t(theta, dtype), _t(X, dtype), spec)[1].numpy()


def _losses_t(theta, b, spec, dtype):
    _, mu, s = _forward(theta, _t(b.X, dtype), spec)
    return losses_of_head(mu, s, b, dtype)


def losses_of_head(mu, s, b, dtype):
    """(surr, kl, ent) as torch scalars of the head's outputs: mean [n, A] and logstd [A]."""
    a, adv = _t(b.actions, dtype), _t(b.advant, dtype)
    mu0, s0 = _t(b.old_mean, dtype), _t(b.old_logstd, dtype)
    z = (a - mu) * torch.exp(-s)
    z0 = (a - mu0) * torch.exp(-s0)
    logr = ((s0 - s) + 0.5 * (z0 * z0 - z * z)).sum(1)
    surr = -(adv * torch.exp(logr)).sum() / b.N
    kl = (s - s0 + (torch.exp(2 * s0) + (mu0 - mu) ** 2) / (2 * torch.exp(2 * s)) - 0.5).sum() / b.N
    ent = (s + HALF_LOG_2PIE).sum() * (mu.shape[0] / b.N)
    return surr, kl, ent


def losses(theta, b, spec, dtype=torch.float64):
    """[surr, kl, ent] as a numpy array of `dtype`."""
    with torch.no_grad():
        return torch.stack(_losses_t(_t(theta, dtype), b, spec, dtype)).numpy()


def surr_weight_sum(theta, b, spec):
    """(1/N) sum_n |adv_n r_n| in float64: the scale of surr's rounding error."""
    with torch.no_grad():
        dtype = torch.float64
        X, a = _t(b.X, dtype), _t(b.actions, dtype)
        _, mu, s = _forward(_t(theta, dtype), X, spec)
        z = (a - mu) * torch.exp(-s)
        z0 = (a - _t(b.old_mean, dtype)) * torch.exp(-_t(b.old_logstd, dtype))
        logr = ((_t(b.old_logstd, dtype) - s) + 0.5 * (z0 * z0 - z * z)).sum(1)
        return float((_t(b.advant, dtype) * torch.exp(logr)).abs().sum() / b.N)


def policy_grad(theta, b, spec, dtype=torch.float64):
    """g = grad_theta surr by autograd."""
    th = _t(theta, dtype).clone().requires_grad_(True)
    surr = _losses_t(th, b, spec, dtype)[0]
    return torch.autograd.grad(surr, th)[0].numpy()


def _kl_ff(th, X, spec, N):
    _, mu, s = _forward(th, X, spec)
    mu0, s0 = mu.detach(), s.detach()
    return (s - s0 + (torch.exp(2 * s0) + (mu0 - mu) ** 2) / (2 * torch.exp(2 * s)) - 0.5).sum() / N


def fvp(theta, b, v, spec, dtype=torch.float64):
    """Hv (undamped) of KL_ff by reverse-over-reverse (trpo_inksci.py:56-70)."""
    th = _t(theta, dtype).clone().requires_grad_(True)
    kl = _kl_ff(th, _t(b.X, dtype), spec, b.N)
    g = torch.autograd.grad(kl, th, create_graph=True)[0]
    gvp = (g * _t(v, dtype)).sum()
    return torch.autograd.grad(gvp, th)[0].numpy()


# ---- the closed forms --------------------------------------------------------------------------------------
def _backprop(layers, hs, delta):
    """flat network gradient of a head delta [n, A] (the usual backprop through the tanh layers)."""
    grads = []
    for i in range(len(layers) - 1, -1, -1):
        W, _ = layers[i]
        grads.append((hs[i].T @ delta, delta.sum(0)))
        if i > 0:
            delta = (delta @ W.T) * (1 - hs[i] * hs[i])
    return torch.cat([torch.cat([gw.reshape(-1), gb]) for gw, gb in reversed(grads)])


def head_deltas(theta, b, spec, dtype=torch.float64):
    """(DS_L [n, A], g_s [A]) of the definition's closed form."""
    with torch.no_grad():
        th = _t(theta, dtype)
        X, a, adv = _t(b.X, dtype), _t(b.actions, dtype), _t(b.advant, dtype)
        _, mu, s = _forward(th, X, spec)
        z = (a - mu) * torch.exp(-s)
        z0 = (a - _t(b.old_mean, dtype)) * torch.exp(-_t(b.old_logstd, dtype))
        ar = adv * torch.exp(((_t(b.old_logstd, dtype) - s) + 0.5 * (z0 * z0 - z * z)).sum(1))
        ds = -(ar / b.N)[:, None] * z * torch.exp(-s)
        gs = -(ar[:, None] * (z * z - 1)).sum(0) / b.N
        return ds.numpy(), gs.numpy()


def policy_grad_closed(theta, b, spec, dtype=torch.float64):
    with torch.no_grad():
        th = _t(theta, dtype)
        layers, _ = unflatten(th, spec)
        hs, _, _ = _forward(th, _t(b.X, dtype), spec)
        ds, gs = head_deltas(theta, b, spec, dtype)
        return torch.cat([_backprop(layers, hs, _t(ds, dtype)), _t(gs, dtype)]).numpy()


def fvp_closed(theta, b, v, spec, dtype=torch.float64):
    """R-forward R{mu} = J_mu v, RD_L = R{mu}/(sigma^2 N), backprop, Hv_s = 2 v_s n/N."""
    with torch.no_grad():
        th, vt = _t(theta, dtype), _t(v, dtype)
        layers, s = unflatten(th, spec)
        vl, vs = unflatten(vt, spec)
        X = _t(b.X, dtype)
        hs, _, _ = _forward(th, X, spec)
        rh = torch.zeros_like(X)
        for i, ((W, _), (V, c)) in enumerate(zip(layers, vl)):
            rz = rh @ W + hs[i] @ V + c
            if i + 1 < len(layers):
                rh = (1 - hs[i + 1] * hs[i + 1]) * rz
        rd = rz * torch.exp(-2 * s) / b.N
        return torch.cat([_backprop(layers, hs, rd), 2.0 * vs * (X.shape[0] / b.N)]).numpy()


# ---- the whole update (trpo_inksci.py:144-158) ---------------------------------------------------------------
@dataclass
class GaussUpdate:
    g: np.ndarray
    stepdir: np.ndarray
    cg_iters: int
    shs: float
    lm: float
    fullstep: np.ndarray
    rate: float
    theta_ls: np.ndarray
    k: int
    losses_before: np.ndarray
    losses_after: np.ndarray
    reverted: bool
    theta_new: np.ndarray


def update(theta_prev, b, spec, dtype=torch.float64, cg_iters=10, residual_tol=1e-10, max_kl=0.01, cg_damping=0.1):
    npdt = np.float64 if dtype == torch.float64 else np.float32
    thprev = np.asarray(theta_prev, npdt).copy()

    def f_Ax(p):
        return fvp(thprev, b, p, spec, dtype) + npdt(cg_damping) * p

    losses_before = losses(thprev, b, spec, dtype)
    g = policy_grad(thprev, b, spec, dtype)
    stepdir, iters = conjugate_gradient(f_Ax, -g, cg_iters, residual_tol)
    shs = 0.5 * float(stepdir.dot(f_Ax(stepdir)))
    with np.errstate(invalid="ignore", divide="ignore"):
        lm = float(np.sqrt(np.float64(shs / max_kl)))
        fullstep = (stepdir / npdt(lm)).astype(npdt)
        rate = float(np.float64(-g.dot(stepdir)) / np.float64(lm))
    theta_ls, k = linesearch(lambda x: losses(x, b, spec, dtype)[0], thprev, fullstep, rate)
    la = losses(theta_ls, b, spec, dtype)
    reverted = bool(la[1] > 2.0 * max_kl)
    theta_new = thprev.copy() if reverted else np.asarray(theta_ls, npdt).copy()
    return GaussUpdate(g, stepdir, iters, shs, lm, fullstep, rate, np.asarray(theta_ls, npdt), k, losses_before, la,
                       reverted, theta_new)


# ---- the data recipe ------------------------------------------------------------------------------------------
def init_theta(spec, rng, logstd=None):
    """weights N(0, 1/fan_in), biases 0.1 N(0, 1), logstd -0.5 + 0.3 N(0, 1) (or the vector given); float32"""
    w = spec.widths
    parts = []
    for i in range(len(w) - 1):
        parts.append((rng.standard_normal((w[i], w[i + 1])) / np.sqrt(w[i])).reshape(-1))
        parts.append(0.1 * rng.standard_normal(w[i + 1]))
    parts.append(-0.5 + 0.3 * rng.standard_normal(spec.act_dim) if logstd is None else np.asarray(logstd, np.float64))
    return np.concatenate(parts).astype(np.float32)


def make_case(shape, seed=0, perturb=0.02, wide_sigma=False):
    """-> (spec, theta float32, GaussBatch).  theta_old = theta (1 + perturb N(0, 1)) elementwise (perturb = 0:
    theta_old = theta, the whole-update feed); X ~ N(0, 1); the actions are sampled from the old policy; the
    advantages are standardised.  wide_sigma spreads logstd evenly over [-3, 1]."""
    obs, hidden, A, n = shape
    spec = GaussSpec(obs, list(hidden), A)
    rng = np.random.RandomState(seed)
    theta = init_theta(spec, rng, np.linspace(-3.0, 1.0, A) if wide_sigma else None)
    theta_old = (theta.astype(np.float64) * (1.0 + perturb * rng.standard_normal(theta.shape))).astype(np.float32)
    X = rng.standard_normal((n, obs)).astype(np.float32)
    old_logstd = theta_old[spec.n_net:].copy()
    old_mean = mean_np(theta_old, X, spec).astype(np.float32)
    actions = (old_mean.astype(np.float64)
               + np.exp(old_logstd.astype(np.float64)) * rng.standard_normal((n, A))).astype(np.float32)
    adv = rng.standard_normal(n)
    if n > 1:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    return spec, theta, GaussBatch(X, actions, adv.astype(np.float32), old_mean, old_logstd)


REGIMES = ("random", "tanh20", "mixed", "sigma_small", "sigma_spread")


def make_hard_case(shape, regime, seed=0, perturb=0.02):
    """make_case in the regimes where the engine's scaled f16 hi + lo split can fail (the constructions of
    tests/test_gpu_fused16_hard.py and tests/test_gpu_rh1_planes.py) -> (spec, theta float32, GaussBatch):
      random        as make_case;
      tanh20        X *= 20: the first tanh layer saturated, 1 - H^2 near H's own rounding;
      mixed         the last 3 rows of W_0 zero (theta and theta_old), rows 5, 34, 63, ... carry 2^15 N(0, 1) in
                    those 3 features: X W_0 is exact, H_1 unsaturated, RH_1 2^15 larger on those rows;
      sigma_small   logstd = -5 in every action dimension: 1/sigma^2 = e^10 in RD_L and DS_L;
      sigma_spread  logstd = linspace(-4.5, 1.5, A): 1/sigma^2 spread by e^12 across the columns of RD_L and DS_L.
    perturb = 0.02 is the loss / g / Hv feed, perturb = 0 the whole-update feed; the actions are sampled from the
    old policy."""
    if regime not in REGIMES:
        raise ValueError(f"make_hard_case: regime must be one of {REGIMES}, got {regime!r}")
    if regime == "random":
        return make_case(shape, seed, perturb)
    obs, hidden, A, n = shape
    spec = GaussSpec(obs, list(hidden), A)
    rng = np.random.RandomState(seed)
    logstd = {"sigma_small": np.full(A, -5.0), "sigma_spread": np.linspace(-4.5, 1.5, A)}.get(regime)
    theta = init_theta(spec, rng, logstd)
    theta_old = (theta.astype(np.float64) * (1.0 + perturb * rng.standard_normal(theta.shape))).astype(np.float32)
    X = rng.standard_normal((n, obs))
    if regime == "tanh20":
        X *= 20.0
    elif regime == "mixed":
        nz = min(3, obs)
        for th in (theta, theta_old):
            th[:obs * hidden[0]].reshape(obs, hidden[0])[obs - nz:, :] = 0.0
        rows = np.arange(5, n, 29)
        X[rows, obs - nz:] = 2.0 ** 15 * rng.standard_normal((rows.size, nz))
    X = X.astype(np.float32)
    old_logstd = theta_old[spec.n_net:].copy()
    old_mean = mean_np(theta_old, X, spec).astype(np.float32)
    actions = (old_mean.astype(np.float64)
               + np.exp(old_logstd.astype(np.float64)) * rng.standard_normal((n, A))).astype(np.float32)
    adv = rng.standard_normal(n)
    if n > 1:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    return spec, theta, GaussBatch(X, actions, adv.astype(np.float32), old_mean, old_logstd)


def block_slices(spec):
    """[(name, slice)] of the flat vector's parameter blocks: W0, b0, ..., WL, bL, logstd."""
    w = spec.widths
    out, off = [], 0
    for i in range(len(w) - 1):
        out.append((f"W{i}", slice(off, off + w[i] * w[i + 1])))
        off += w[i] * w[i + 1]
        out.append((f"b{i}", slice(off, off + w[i + 1])))
        off += w[i + 1]
    out.append(("logstd", slice(off, off + spec.act_dim)))
    return out
