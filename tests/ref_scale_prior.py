"""fp64 reference of the ELBO with a prior on the scale distribution: the oracle's loss (oracle/elbo_oracle.py: `elbo_forward`) plus the
"Σ KLDiv" term of `VariationalMergingModel.call` (careless/models/merging/variational.py:156-163 through `add_kl_div`, :123-139), with
gradients by autograd over every trainable tensor.  Built on the oracle's public functions only (`elbo_forward`, `mlp_forward`,
`scale_bijector`, `image_scales`).

As the reference executes it with a `scale_prior` and a `scale_kl_weight` that is not None -- `add_kl_div(scale_dist, scale_prior, z_scale,
weight=1., reduction='mean')`: the loss gains mean(kl_div) with weight 1 whatever `kl_weight` is, where kl_div is
  * `scale_dist.kl_divergence(scale_prior)` when TFP has one registered: a bare `tfd.Normal(loc, sigma)` (no `tfb.Shift`, nn.py:84-87, no
    `tfb.Scale`, image.py:60-63) against a Normal prior -- KL_i = log(s / sigma_i) + (sigma_i^2 + (loc_i - m)^2) / (2 s^2) - 1/2, (N,);
  * else `scale_dist.log_prob(z_scale) - scale_prior.log_prob(z_scale)`, (S, N), with z = a_i (loc_i + sigma_i eta_is + c) and
    log q(z) = -log sigma_i - eta_is^2 / 2 - log(2 pi) / 2 - log|a_i| (the Normal's density at the draw, minus the bijectors' log-Jacobian).
A shift is present where `cfg.scale_shift` is non-zero: the convention of tests/util.build_model, which hands the scaler
`scale_multiplier=None` for 0.  The mean is over rows (and samples), also for Laue data: the scale distribution is per row, not per slot.

`prior`: ("normal", loc, scale) | ("laplace", loc, scale) | ("studentt", df, loc, scale), floats.
"""
from __future__ import annotations

import math

import torch

from oracle import elbo_oracle as O


def prior_log_prob(prior, z: torch.Tensor) -> torch.Tensor:
    """log p(z) of the scale prior, differentiable in z.  The Laplace density's |.| has the derivative sign(.) (0 at the kink), as
    TensorFlow's gradient of abs."""
    kind = prior[0]
    if kind == "normal":
        _, m, s = prior
        y = (z - m) / s
        return -0.5 * y * y - 0.5 * O.LOG_2PI - math.log(s)
    if kind == "laplace":
        _, m, s = prior
        return -(z - m).abs() / s - math.log(2.0 * s)
    if kind == "studentt":
        _, df, m, s = prior
        y = (z - m) / s
        return (-0.5 * (df + 1.0) * torch.log1p(y * y / df) - math.log(s) - 0.5 * math.log(df * math.pi)
                - math.lgamma(0.5 * df) + math.lgamma(0.5 * (df + 1.0)))
    raise ValueError(kind)


def is_analytic(prior, cfg: O.ElboConfig) -> bool:
    """TFP has a registered KL: a bare Normal scale distribution against a Normal prior."""
    return prior[0] == "normal" and cfg.scale_shift == 0.0 and not cfg.use_image_scales


def scale_loc_sigma(p: O.ElboParams, x: O.ElboInputs, cfg: O.ElboConfig, flips=None, near=None):
    """(loc, sigma) of the scale distribution's Normal, (N,) each -- what `elbo_forward` computes inside."""
    out = O.mlp_forward(x.metadata, p.mlp_w, p.mlp_b, cfg.leakiness, x.image_id, p.imgl_w or (), p.imgl_b or (), flips=flips, near=near)
    return out[:, 0], O.scale_bijector(out[:, 1], cfg.scale_bijector, cfg.epsilon)


def analytic_kl(loc, sigma, m: float, s: float) -> torch.Tensor:
    """KL(N(loc, sigma) || N(m, s)) per row."""
    return torch.log(s / sigma) + (sigma * sigma + (loc - m) ** 2) / (2.0 * s * s) - 0.5


def sample_kl(loc, sigma, eta, prior, shift: float = 0.0, a=None):
    """log q(z) - log p(z) per (sample, row), and z: eta (S, N); a (N,) image scales or None."""
    y = loc[None, :] + sigma[None, :] * eta + shift
    log_q = -torch.log(sigma)[None, :] - 0.5 * eta * eta - 0.5 * O.LOG_2PI
    z = y
    if a is not None:
        z = a[None, :] * y
        log_q = log_q - torch.log(a.abs())[None, :]
    return log_q - prior_log_prob(prior, z), z


def scale_kl(p: O.ElboParams, x: O.ElboInputs, cfg: O.ElboConfig, eta, prior, rows=None, flips=None):
    """Σ KLDiv: dict(value, z or None, kl_div).  `rows`: an index of rows whose terms are kept (the data-parallel shard tests); the mean
    stays over all N rows, so the shards' values add up."""
    loc, sigma = scale_loc_sigma(p, x, cfg, flips=flips)
    N = loc.shape[0]
    if is_analytic(prior, cfg):
        kl, z = analytic_kl(loc, sigma, float(prior[1]), float(prior[2])), None
        kept = kl if rows is None else kl[rows]
        return dict(value=kept.sum() / N, z=z, kl_div=kl)
    a = O.image_scales(p.img_raw)[x.image_id] if cfg.use_image_scales else None
    kl, z = sample_kl(loc, sigma, eta, prior, cfg.scale_shift, a)
    kept = kl if rows is None else kl[:, rows]
    return dict(value=kept.sum() / (kl.shape[0] * N), z=z, kl_div=kl)


def forward(p, x, cfg, u_f, eta, prior, kl_mask=None, rows=None, flips=None, near=None):
    """The oracle's forward pass plus the term: its dict with `scale_kl` added and `loss` = oracle loss + Σ KLDiv."""
    out = O.elbo_forward(p, x, cfg, u_f, eta, kl_mask, flips=flips, near=near)
    t = scale_kl(p, x, cfg, eta, prior, rows=rows, flips=flips)
    out = dict(out)
    out["scale_kl"], out["z_scale"] = t["value"], t["z"]
    out["loss"] = out["loss"] + t["value"]
    return out


def value_and_grads(p, x, cfg, u_f, eta, prior, kl_mask=None, rows=None, flips=None, near=None):
    """Loss + reverse-mode gradients of every trainable tensor, in `ElboParams.tensors()` order."""
    q = p.clone(requires_grad=True)
    out = forward(q, x, cfg, u_f, eta, prior, kl_mask, rows, flips=flips, near=near)
    ts = q.tensors()
    grads = torch.autograd.grad(out["loss"], ts, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, ts)]
    return {k: v.detach() if torch.is_tensor(v) else v for k, v in out.items()}, grads


def train_step(p, x, cfg, st: O.AdamState, u_f, eta, prior):
    """The oracle's `train_step` with the term: grads -> global norm -> non-finite -> 0 -> clip -> Adam.  Mutates `p` and `st`."""
    out, grads = value_and_grads(p, x, cfg, u_f, eta, prior)
    gnorm = O.global_norm(grads)
    grads = [torch.where(torch.isfinite(g), g, torch.zeros_like(g)) for g in grads]
    grads = O.clip_grads(grads, cfg)
    O.adam_apply(p.tensors(), grads, st, cfg)
    return {"loss": float(out["loss"]), "F KLDiv": float(out["kl"]), "NLL": float(out["nll"]), "Σ KLDiv": float(out["scale_kl"]),
            "Grad Norm": float(gnorm)}
