"""CPU reference of the TRPO update with Fisher-vector products on every k-th row of the batch
(trpo_set_fvp_subsample, include/trpo_engine.h): the update block of trpo_inksci.py:144-158 composed from the
oracle's pieces, with policy_grad, losses and linesearch on all rows and fisher_vector_product on X[::k].
categorical_update is that composition over oracle.trpo_oracle, gaussian_update over tests/gauss_ref.py; at k = 1
each repeats its module's own whole update operation for operation."""
import numpy as np

import gauss_ref as G
from oracle import trpo_oracle as O


def n_sub(n, k):
    """rows i < n with i % k == 0"""
    return -(-n // k)


def sub_batch(batch, k):
    """The Fisher feed of an O.Batch: every k-th row of every array."""
    return O.Batch(batch.X[::k], batch.actions[::k], batch.advant[::k], batch.old_dist[::k])


def sub_gauss_batch(b, k):
    return G.GaussBatch(b.X[::k], b.actions[::k], b.advant[::k], b.old_mean[::k], b.old_logstd)


def fisher_matrix(theta, X, spec, k):
    """F_sub as a dense matrix (small policies only): column j = F_sub e_j, undamped, float64."""
    P = spec.n_params
    th = np.asarray(theta, np.float64)
    eye = np.eye(P)
    return np.stack([O.fvp_undamped(th, X[::k], eye[j], spec) for j in range(P)], axis=1)


def categorical_update(theta_prev, batch, spec, k, dtype=np.float64, cg_iters=10, residual_tol=1e-10,
                       max_kl=O.CONFIG["max_kl"], cg_damping=O.CONFIG["cg_damping"]):
    """O.trpo_update with the Fisher matrix of rows 0, k, 2k, ...; returns an O.UpdateResult."""
    thprev = np.asarray(theta_prev, dtype).copy()
    X, a, adv, old = batch.X, batch.actions, batch.advant, batch.old_dist
    Xs = X[::k]

    def fvp(p):
        return O.fisher_vector_product(thprev, Xs, p, spec, cg_damping, dtype)

    losses_before = O.losses(thprev, X, a, adv, old, spec, dtype=dtype)
    g = O.policy_grad(thprev, X, a, adv, old, spec, dtype=dtype)
    stepdir, iters = O.conjugate_gradient(fvp, -g, cg_iters, residual_tol)
    shs = 0.5 * float(stepdir.dot(fvp(stepdir)))
    with np.errstate(invalid="ignore"):
        lm = float(np.sqrt(np.float64(shs / max_kl)))
    with np.errstate(divide="ignore", invalid="ignore"):
        fullstep = (stepdir / dtype(lm)).astype(dtype)
    neggdotstepdir = -g.dot(stepdir)
    with np.errstate(divide="ignore", invalid="ignore"):
        rate = float(np.float64(neggdotstepdir) / np.float64(lm))

    def loss(x):
        return O.losses(x, X, a, adv, old, spec, dtype=dtype)[0]

    theta_ls, kk = O.linesearch(loss, thprev, fullstep, rate)
    la = O.losses(theta_ls, X, a, adv, old, spec, dtype=dtype)
    reverted = bool(la[1] > 2.0 * max_kl)
    theta_new = thprev.copy() if reverted else np.asarray(theta_ls, dtype).copy()
    return O.UpdateResult(g=g, stepdir=stepdir, cg_iters=iters, shs=shs, lm=lm, fullstep=fullstep,
                          neggdotstepdir=float(neggdotstepdir), rate=rate, theta_ls=np.asarray(theta_ls, dtype), k=kk,
                          losses_after=la, reverted=reverted, theta_new=theta_new, losses_before=losses_before)


def gaussian_update(theta_prev, b, spec, k, dtype=None, cg_iters=10, residual_tol=1e-10, max_kl=0.01,
                    cg_damping=0.1):
    """G.update with the Fisher matrix of rows 0, k, 2k, ...; returns a G.GaussUpdate."""
    import torch
    dtype = torch.float64 if dtype is None else dtype
    npdt = np.float64 if dtype == torch.float64 else np.float32
    thprev = np.asarray(theta_prev, npdt).copy()
    bs = sub_gauss_batch(b, k)

    def f_Ax(p):
        return G.fvp(thprev, bs, p, spec, dtype) + npdt(cg_damping) * p

    losses_before = G.losses(thprev, b, spec, dtype)
    g = G.policy_grad(thprev, b, spec, dtype)
    stepdir, iters = G.conjugate_gradient(f_Ax, -g, cg_iters, residual_tol)
    shs = 0.5 * float(stepdir.dot(f_Ax(stepdir)))
    with np.errstate(invalid="ignore", divide="ignore"):
        lm = float(np.sqrt(np.float64(shs / max_kl)))
        fullstep = (stepdir / npdt(lm)).astype(npdt)
        rate = float(np.float64(-g.dot(stepdir)) / np.float64(lm))
    theta_ls, kk = G.linesearch(lambda x: G.losses(x, b, spec, dtype)[0], thprev, fullstep, rate)
    la = G.losses(theta_ls, b, spec, dtype)
    reverted = bool(la[1] > 2.0 * max_kl)
    theta_new = thprev.copy() if reverted else np.asarray(theta_ls, npdt).copy()
    return G.GaussUpdate(g, stepdir, iters, shs, lm, fullstep, rate, np.asarray(theta_ls, npdt), kk, losses_before, la,
                         reverted, theta_new)
