"""fp64 restatement of the Rice-Woolfson surrogate posterior (reference careless/models/merging/surrogate_posteriors.py:133-172 on
careless/utils/distributions.py:228-348) and of whole ELBO steps under it, for tests/test_rw_posterior.py and tests/test_rw_posterior_gpu.py.

The whole-step reference sits ON TOP of the unchanged oracle: `patched(centric)` swaps `O.tn_sample` and `O.tn_log_prob` -- the only two
places where `O.elbo_forward` touches the family of q(F) -- for the versions below, which take `centric` from a closure and ignore
`low` / `high`, and puts them back on exit.  Inside it `O.elbo_forward`, `O.elbo_value_and_grads`, `O.train_step` and `O.validation_nll`
are the reference of a step under the Rice-Woolfson posterior; the (2, S, R) standard normals n1, n2 go in through their `u_f` argument.
`patched(centric, moments=True)` also swaps `O.tn_mean`, `O.tn_variance` and the `scipy.stats.truncnorm.moment` behind the oracle's
`merged_results` / `prediction_mean_stddev` for the Rice-Woolfson moments."""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from oracle import elbo_oracle as O

EPS32 = float(np.finfo(np.float32).eps)
KINK_GUARD = 1e-4         # no centric draw with |loc + scale n1| < KINK_GUARD * scale: fp32 could land on the other side of |.|'s kink


def f64(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64) if not torch.is_tensor(a) else a.to(torch.float64)


def rw_sample(loc, scale, centric, n):
    """n: (2, S, R) standard normals.  Centric: |loc + scale n1| + eps32 (surrogate_posteriors.py:166; n2 unused); acentric:
    sqrt((scale n1)^2 + (loc + scale n2)^2) (distributions.py:252-258: s1 alone, s2 + nu).  Differentiable: the pathwise gradient is autograd's
    (the gradient of abs is sign, 0 at 0, as TensorFlow's)."""
    n1, n2 = n[0], n[1]
    zc = torch.abs(loc + scale * n1) + EPS32
    za = torch.sqrt((scale * n1) ** 2 + (loc + scale * n2) ** 2)
    return torch.where(centric, zc, za)


def rw_log_prob(z, loc, scale, centric):
    """tf.where(centric, FoldedNormal.log_prob, Rice.log_prob) (surrogate_posteriors.py:168-169) on the oracle's two densities."""
    return torch.where(centric, O.folded_normal_log_prob(z, loc, scale), O.rice_log_prob(z, loc, scale))


def kink_margin(loc, scale, centric, n):
    """min over the centric draws of |loc + scale n1| / scale (inf without a centric reflection)."""
    c = np.asarray(centric, dtype=bool)
    if not c.any():
        return np.inf
    loc, scale, n1 = (np.asarray(a, dtype=np.float64) for a in (loc, scale, np.asarray(n)[0]))
    return float(np.min(np.abs(loc + scale * n1)[..., c] / scale[c]))


def rw_moments(loc, scale, centric):
    """(mean, variance, fourth raw moment) in fp64 numpy: `RiceWoolfson._moments` of the package's host class (pinned to scipy by
    tests/test_ref_prior.py) and the two closed-form fourth moments."""
    from careless_amd.models.merging.surrogate_posteriors import RiceWoolfson
    loc, scale, c = np.asarray(loc, dtype=np.float64), np.asarray(scale, dtype=np.float64), np.asarray(centric, dtype=bool)
    host = RiceWoolfson(loc, scale, c)
    host.loc, host.scale = loc, scale                      # (the constructor rounds to fp32: keep the fp64 values)
    (wm, rm), (wv, rv) = host._moments()
    m4 = np.where(c, loc ** 4 + 6 * loc ** 2 * scale ** 2 + 3 * scale ** 4, loc ** 4 + 8 * scale ** 2 * loc ** 2 + 8 * scale ** 4)
    return np.where(c, wm, rm), np.where(c, wv, rv), m4


@contextlib.contextmanager
def patched(centric, moments=False):
    c = torch.as_tensor(np.asarray(centric, dtype=bool))
    saved = (O.tn_sample, O.tn_log_prob, O.tn_mean, O.tn_variance)
    O.tn_sample = lambda loc, scale, low, high, n: rw_sample(loc, scale, c, n)
    O.tn_log_prob = lambda z, loc, scale, low, high: rw_log_prob(z, loc, scale, c)
    tm = None
    if moments:
        import scipy.stats
        O.tn_mean = lambda loc, scale, low, high: torch.as_tensor(rw_moments(loc.numpy(), scale.numpy(), c.numpy())[0])
        O.tn_variance = lambda loc, scale, low, high: torch.as_tensor(rw_moments(loc.numpy(), scale.numpy(), c.numpy())[1])
        tm = scipy.stats.truncnorm
        tm.moment = lambda k, a, b, loc, scale: rw_moments(loc, scale, c.numpy())[2]       # (an instance attribute over the method)
    try:
        yield
    finally:
        O.tn_sample, O.tn_log_prob, O.tn_mean, O.tn_variance = saved
        if tm is not None:
            del tm.moment


def elbo_value_and_grads(params, x, cfg, n_f, eta, centric, kl_mask=None, flips=None, near=None):
    with patched(centric):
        return O.elbo_value_and_grads(params, x, cfg, f64(n_f), f64(eta), kl_mask, flips=flips, near=near)


def train_step(p, x, cfg, st, n_f, eta, centric):
    with patched(centric):
        return O.train_step(p, x, cfg, st, f64(n_f), f64(eta))


def validation_nll(p, x_val, cfg, n_f, eta, n_train, centric):
    with patched(centric):
        return O.validation_nll(p, x_val, cfg, f64(n_f), f64(eta), n_train)


def noise_for(loc, scale, centric, S, seed):
    """(2, S, R) fp32 standard normals whose centric draws keep KINK_GUARD (the first seed from `seed` on that does; checked on the CPU)."""
    R = len(np.asarray(loc))
    for k in range(seed, seed + 100):
        n = np.random.default_rng(k).normal(size=(2, S, R)).astype(np.float32)
        if kink_margin(loc, scale, centric, n) >= KINK_GUARD:
            return n
    raise AssertionError("no seed keeps the centric draws off the kink")
