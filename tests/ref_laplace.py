"""fp64 restatement of the Laplace likelihood (reference careless/models/likelihoods/mono.py:20-23, laue.py:76-81:
tfd.Laplace(Iobs, SigIobs / sqrt 2)) and of a whole ELBO step under it, for tests/test_laplace.py and tests/test_laplace_gpu.py.

The whole-step reference sits ON TOP of the unchanged oracle, like tests/ref_prior.py: `O.elbo_forward` computes the step under the
Normal likelihood, and because the likelihood enters the loss only through  nll = -w sum ll(ipred),  trading the Normal term for the
Laplace one on the SAME attached predictions -- through `O.laue_convolve` for Laue data, over all N slots, the padded ones included, as
the oracle's own `ll` -- gives the step under the Laplace likelihood:
    nll_laplace  = nll  + w sum (normal_log_prob - laplace_log_prob)(ipred),      loss_laplace = loss + (the same)
with w = 1 / S, or 1 / (S N) under `kl_weight`.  Gradients by torch.autograd.grad (the gradient of abs is sign, 0 at 0, as TensorFlow's).

The problems of util.make_problem put every prediction far below its observation: every residual has one sign and the derivative of the
Laplace term is one constant.  `rewrite_observations` moves the observations onto the predictions (see there)."""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import elbo_oracle as O

GUARD_REL = 1e-4          # the guard round the kink, relative to gmax * max|ipred|: every test asserts the engine's ipred within 1e-4 of max|ipred|, so a
                          # sum over a harmonic group of gmax rows is within one guard and no sample outside the guard changes sides


def f64(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64) if not torch.is_tensor(a) else a.to(torch.float64)


def laplace_log_prob(x, loc, sig):
    """`tfd.Laplace(loc, sig / sqrt 2).log_prob(x)`: -|x - loc| / b - log(2 b)."""
    b = sig / math.sqrt(2.0)
    return -torch.abs(x - loc) / b - torch.log(2.0 * b)


def convolved(ipred, x, cfg):
    return O.laue_convolve(ipred, x.harmonic_id) if cfg.laue else ipred


def elbo_value_and_grads(params, x, cfg, u_f, eta, kl_mask=None, flips=None, near=None):
    """Loss terms and gradients of one step under the Laplace likelihood (module docstring); signature and return value of
    `O.elbo_value_and_grads`, plus out["ipred_l"], what the likelihood saw (S, N)."""
    assert cfg.likelihood == "normal" and not cfg.ev11
    q = params.clone(requires_grad=True)
    out = O.elbo_forward(q, x, cfg, f64(u_f), f64(eta), kl_mask, flips=flips, near=near)
    ipl = convolved(out["ipred"], x, cfg)
    S, N = ipl.shape
    swap = O.normal_log_prob(ipl, x.iobs[None, :], x.sigiobs[None, :]) - laplace_log_prob(ipl, x.iobs[None, :], x.sigiobs[None, :])
    w = 1.0 / S if cfg.kl_weight is None else 1.0 / (S * N)
    tot = w * swap.sum()
    out = dict(out, nll=out["nll"] + tot, loss=out["loss"] + tot, ipred_l=ipl)
    ts = q.tensors()
    grads = torch.autograd.grad(out["loss"], ts, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, ts)]
    return {k: v.detach() for k, v in out.items()}, grads


def train_step(p, x, cfg, st, u_f, eta):
    """`O.train_step` with this module's gradients: global norm before the sanitise, non-finite -> 0, clipping, Adam (variational.py:185-224)."""
    out, grads = elbo_value_and_grads(p, x, cfg, u_f, eta)
    gnorm = O.global_norm(grads)
    grads = [torch.where(torch.isfinite(g), g, torch.zeros_like(g)) for g in grads]
    grads = O.clip_grads(grads, cfg)
    O.adam_apply(p.tensors(), grads, st, cfg)
    return {"loss": float(out["loss"]), "F KLDiv": float(out["kl"]), "NLL": float(out["nll"]), "Grad Norm": float(gnorm)}


def validation_nll(p, x_val, cfg, u_f, eta, n_train):
    """`O.validation_nll` under the Laplace likelihood."""
    out, _ = elbo_value_and_grads(p, x_val, cfg, u_f, eta)
    return float(out["nll"]) * n_train / int(x_val.refl_id.shape[0])


# ---- the problem: observations on both sides of the predictions, none on the kink -----------------------------------------------------------
def counted_slots(data):
    """Slots that hold an observation: every row (monochromatic), the first n_groups slots (Laue; the rest is the (1.0, 1.0) padding)."""
    N = len(data["refl_id"])
    return N if data.get("harmonic_id") is None else int(np.max(data["harmonic_id"])) + 1


def guard_of(data, ipred):
    gmax = 1 if data.get("harmonic_id") is None else int(np.bincount(np.asarray(data["harmonic_id"]).reshape(-1)).max())
    return GUARD_REL * gmax * float(np.max(np.abs(ipred)))


def predictions(data, cfg, params, u_f, eta):
    """(ipred (S, N), what the likelihood sees (S, N)) of the fp64 reference: independent of Iobs / SigIobs."""
    x = O.inputs_from_numpy(data)
    with torch.no_grad():
        out = O.elbo_forward(params, x, cfg, f64(u_f), f64(eta))
    return out["ipred"].numpy(), convolved(out["ipred"], x, cfg).numpy()


def rewrite_observations(data, cfg, params, noises, seed=0):
    """A copy of `data` with  Iobs := m + 1.5 sigma n,  SigIobs := sigma  on the counted slots: m the sample-mean reference prediction of the
    slot (over every (u_f, eta) of `noises`), sigma = 0.1 |m| + 0.05 mean|m|, n standard normal.  Then every observation with a sample of any
    of the noises inside TWO guards is moved up by 3 guards, until none is (the tests ask for one guard: the second is margin).  Returns
    (data, nudging rounds)."""
    data = dict(data)
    preds = [predictions(data, cfg, params, u, e) for u, e in noises]
    ipl = np.concatenate([p[1] for p in preds], axis=0)                 # (samples of every noise, N)
    guard = max(guard_of(data, p[0]) for p in preds)
    G = counted_slots(data)
    m = ipl[:, :G].mean(axis=0)
    sigma = 0.1 * np.abs(m) + 0.05 * np.mean(np.abs(m))
    rng = np.random.default_rng(1000 + seed)
    iobs = np.array(data["iobs"], dtype=np.float32, copy=True).reshape(-1)
    sig = np.array(data["sigiobs"], dtype=np.float32, copy=True).reshape(-1)
    iobs[:G] = (m + 1.5 * sigma * rng.normal(size=G)).astype(np.float32)
    sig[:G] = sigma.astype(np.float32)
    rounds = 0
    while True:
        bad = (np.abs(ipl - iobs[None, :].astype(np.float64)) < 2.0 * guard).any(axis=0)
        if not bad.any():
            break
        iobs[bad] = (iobs[bad].astype(np.float64) + 3.0 * guard).astype(np.float32)
        rounds += 1
        assert rounds < 50
    data["iobs"], data["sigiobs"] = iobs, sig
    return data, rounds


def assert_conditions(data, ipred, ipred_l):
    """The two conditions every test on injected noise asserts on the fp64 reference alone: no (slot, sample) pair within the guard of its
    observation, each sign of the residual on at least 25 % of the counted pairs.  Returns (smallest gap / guard, positive fraction)."""
    guard = guard_of(data, ipred)
    res = np.asarray(ipred_l, dtype=np.float64) - np.asarray(data["iobs"], dtype=np.float64).reshape(-1)[None, :]
    gap = float(np.min(np.abs(res))) / guard
    pos = float(np.mean(res[:, :counted_slots(data)] > 0))
    assert gap >= 1.0, gap
    assert 0.25 <= pos <= 0.75, pos
    return gap, pos
