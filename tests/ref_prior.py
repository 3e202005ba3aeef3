"""fp64 restatement of the empirical reference priors (reference careless/models/priors/empirical.py:9-131) and of a whole ELBO step under
one, for the tests of `cl_ref_prior` and of the engine (tests/test_ref_prior.py, tests/test_ref_prior_gpu.py).

The whole-step reference sits ON TOP of the unchanged oracle: `O.elbo_forward` computes the step under the Wilson prior, and because the
prior enters the loss only through  kl = mean/sum of (log q - log p)(z_f),  trading the Wilson term for the reference prior's on the SAME
attached samples z_f gives the step under the reference prior:
    kl_ref   = kl   + w   sum over the KL's reflections of (wilson_log_prob(z_f) - ref_log_prob(z_f))
    loss_ref = loss + w_l (the same sum)
with w = 1 / S (sum mode), or w = 1 / (S R), w_l = kl_weight w in `kl_weight` mode -- the mean runs over all R columns, the zeros of the
unobserved ones included, as tf.reduce_mean does (reference variational.py:133).  Gradients by torch.autograd.grad.
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import elbo_oracle as O

KINDS = ("normal", "laplace", "studentt", "rice_woolfson")


def f64(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64) if not torch.is_tensor(a) else a.to(torch.float64)


def base_log_prob(kind, z, loc, scale, centric=None, dof=None):
    """log-density of the base distribution at z (..., R); loc / scale (R,) are the BASE distribution's parameters (Laplace: b = SigFobs / sqrt 2)."""
    if kind == "normal":                                # tfd.Normal (empirical.py:85)
        return O.normal_log_prob(z, loc, scale)
    if kind == "laplace":                               # tfd.Laplace (empirical.py:64): -|z - loc| / b - log(2 b)
        return -torch.abs(z - loc) / scale - torch.log(2.0 * scale)
    if kind == "studentt":                              # tfd.StudentT (empirical.py:108)
        return O.studentt_log_prob(z, float(dof), loc, scale)
    if kind == "rice_woolfson":                         # RiceWoolfson.log_prob (surrogate_posteriors.py:168-169)
        return torch.where(centric, O.folded_normal_log_prob(z, loc, scale), O.rice_log_prob(z, loc, scale))
    raise ValueError(kind)


def ref_log_prob(kind, z, loc, scale, observed=None, centric=None, dof=None):
    """`ReferencePrior.log_prob` (empirical.py:33-43) with FULL-length (R,) parameter arrays: the base density on observed reflections,
    exact zeros elsewhere (the parameters of unobserved reflections are not looked at).  Differentiable in z."""
    z, loc, scale = f64(z), f64(loc), f64(scale)
    if centric is not None:
        centric = torch.as_tensor(np.asarray(centric), dtype=torch.bool) if not torch.is_tensor(centric) else centric.bool()
    if observed is None:
        return base_log_prob(kind, z, loc, scale, centric, dof)
    obs = torch.as_tensor(np.asarray(observed), dtype=torch.bool) if not torch.is_tensor(observed) else observed.bool()
    one = torch.ones_like(loc)
    lp = base_log_prob(kind, z, torch.where(obs, loc, one), torch.where(obs, scale, one), centric, dof)
    return torch.where(obs, lp, torch.zeros_like(lp))


def prior_arrays(prior, R):
    """(kind, loc, scale, observed, centric, dof) of a careless_amd reference prior, full length: what `ref_log_prob` takes."""
    return (prior.engine_kind, prior.loc_full(R), prior.scale_full(R), prior.observed_mask(R), prior.centric_full(R), prior.dof)


def elbo_value_and_grads(params, x, cfg, u_f, eta, prior, kl_mask=None, flips=None, near=None):
    """Loss terms and gradients of one step under the reference prior `prior` (see the module docstring); the signature and the return
    value of `O.elbo_value_and_grads`, `flips` / `near` passed through."""
    assert cfg.prior == "wilson"
    q = params.clone(requires_grad=True)
    out = O.elbo_forward(q, x, cfg, f64(u_f), f64(eta), kl_mask, flips=flips, near=near)
    z = out["z_f"]                                      # (S, R), attached
    S, R = z.shape
    kind, loc, scale, observed, centric, dof = prior_arrays(prior, R)
    swap = O.wilson_log_prob(z, x.centric, x.multiplicity, x.sigma) - ref_log_prob(kind, z, loc, scale, observed, centric, dof)
    if kl_mask is not None:
        swap = swap[:, kl_mask]
    if cfg.kl_weight is None:
        w, wl = 1.0 / S, 1.0 / S
    else:                                               # (with a kl_mask the oracle's mean runs over the masked columns)
        w = 1.0 / (S * swap.shape[1])
        wl = cfg.kl_weight * w
    tot = swap.sum()
    out = dict(out, kl=out["kl"] + w * tot, loss=out["loss"] + wl * tot)
    ts = q.tensors()
    grads = torch.autograd.grad(out["loss"], ts, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, ts)]
    return {k: v.detach() for k, v in out.items()}, grads


def train_step(p, x, cfg, st, u_f, eta, prior):
    """`O.train_step` with this module's gradients: global norm before the sanitise, non-finite -> 0, clipping, Adam (variational.py:185-224)."""
    out, grads = elbo_value_and_grads(p, x, cfg, u_f, eta, prior)
    gnorm = O.global_norm(grads)
    grads = [torch.where(torch.isfinite(g), g, torch.zeros_like(g)) for g in grads]
    grads = O.clip_grads(grads, cfg)
    O.adam_apply(p.tensors(), grads, st, cfg)
    return {"loss": float(out["loss"]), "F KLDiv": float(out["kl"]), "NLL": float(out["nll"]), "Grad Norm": float(gnorm)}

