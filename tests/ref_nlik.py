"""fp64 restatement of the neural likelihood (reference careless/models/likelihoods/mono.py:75-110) and of a whole ELBO step under it,
for tests/test_nlik.py and tests/test_nlik_gpu.py.

    network = mlp_layers x Dense(mlp_width, LeakyReLU(0.3)) -> Dense(1, softplus)        delta   = network(concat(iobs, sigiobs))
    sigpred = sigiobs * delta / mean(delta)  (over all rows of the set)                    ll      = Normal(iobs, sigpred).log_prob(ipred)

The whole-step reference sits ON TOP of the unchanged oracle, like tests/ref_laplace.py: `O.elbo_forward` computes the step under the Normal
likelihood, and because the likelihood enters the loss only through  nll = -w sum ll(ipred),  trading the Normal term on SigIobs for the one
on sigpred on the SAME attached predictions gives the step under the neural likelihood:
    nll += w sum (normal_lp(ipred; iobs, sigiobs) - normal_lp(ipred; iobs, sigpred)),        w = 1 / S, or 1 / (S N) under `kl_weight`.
sigpred comes from an fp64 torch network whose tensors require grad; every gradient by torch.autograd.grad.  `forward` also reports the
smallest |pre-activation| of the network's LeakyReLU units relative to its layer's largest: every parity case asserts that it exceeds
`KINK_REL`, so no unit of the fp32 engine can sit on the other branch."""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import elbo_oracle as O

LEAK = 0.3                # tfk.layers.LeakyReLU()'s default slope
KINK_REL = 1e-4
ZH_MIN = -10.0            # `pick_net`: delta >= softplus(-10) = 4.5e-5 on every row


def f64(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64) if not torch.is_tensor(a) else a.to(torch.float64)


def init_net(L, w, seed, bias=0.1):
    """Keras-ordered fp64 tensors [W_0 (2, w), b_0, ..., W_head (w, 1), b_head (1,)]: glorot-uniform kernels; `bias`: the standard deviation
    of normal biases (Keras starts them at zero: a test wants every tensor's gradient exercised at non-trivial values)."""
    g = torch.Generator().manual_seed(int(seed))
    dims = [2] + [w] * L + [1]
    out = []
    for i, o in zip(dims[:-1], dims[1:]):
        lim = math.sqrt(6.0 / (i + o))
        out += [(torch.rand(i, o, generator=g, dtype=torch.float64) * 2 - 1) * lim, bias * torch.randn(o, generator=g, dtype=torch.float64)]
    return out


def forward(net, iobs, sigiobs):
    """(delta (N,), sigpred (N,), head pre-activation (N,), smallest |hidden pre-activation| relative to its layer's largest)."""
    h = torch.stack([f64(iobs).reshape(-1), f64(sigiobs).reshape(-1)], dim=1)
    kink = math.inf
    for k in range(len(net) // 2 - 1):
        z = h @ net[2 * k] + net[2 * k + 1]
        with torch.no_grad():
            fin = z[torch.isfinite(z)].abs()
            if fin.numel():
                kink = min(kink, float(fin.min() / fin.max()))
        h = torch.where(z > 0, z, LEAK * z)
    zh = (h @ net[-2] + net[-1])[:, 0]
    delta = torch.nn.functional.softplus(zh)
    return delta, f64(sigiobs).reshape(-1) * delta / delta.mean(), zh, kink


def elbo_value_and_grads(params, net, x, cfg, u_f, eta, kl_mask=None, flips=None, near=None):
    """Loss terms and gradients of one step under the neural likelihood: `O.elbo_value_and_grads`' return value with the network's
    gradients (Keras order) behind the model's, plus out["sigpred"], out["delta"], out["kink"]."""
    assert cfg.likelihood == "normal" and not cfg.ev11 and not cfg.laue
    q = params.clone(requires_grad=True)
    nt = [t.detach().clone().requires_grad_() for t in net]
    out = O.elbo_forward(q, x, cfg, f64(u_f), f64(eta), kl_mask, flips=flips, near=near)
    ipred = out["ipred"]
    S, N = ipred.shape
    delta, sigpred, _, kink = forward(nt, x.iobs, x.sigiobs)
    swap = O.normal_log_prob(ipred, x.iobs[None, :], x.sigiobs[None, :]) - O.normal_log_prob(ipred, x.iobs[None, :], sigpred[None, :])
    w = 1.0 / S if cfg.kl_weight is None else 1.0 / (S * N)
    tot = w * swap.sum()
    out = dict(out, nll=out["nll"] + tot, loss=out["loss"] + tot, sigpred=sigpred, delta=delta)
    ts = q.tensors() + nt
    grads = torch.autograd.grad(out["loss"], ts, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, ts)]
    out = {k: v.detach() for k, v in out.items()}
    out["kink"] = kink
    return out, grads


def train_step(p, net, x, cfg, st, u_f, eta):
    """`O.train_step` with this module's gradients on model + network: global norm before the sanitise, non-finite -> 0, clipping, Adam
    (variational.py:185-224).  `p` and `net` are updated in place; `st`: `O.AdamState.zeros_like(p.tensors() + net)`."""
    out, grads = elbo_value_and_grads(p, net, x, cfg, u_f, eta)
    gnorm = O.global_norm(grads)
    grads = [torch.where(torch.isfinite(g), g, torch.zeros_like(g)) for g in grads]
    grads = O.clip_grads(grads, cfg)
    O.adam_apply(p.tensors() + net, grads, st, cfg)
    return {"loss": float(out["loss"]), "F KLDiv": float(out["kl"]), "NLL": float(out["nll"]), "Grad Norm": float(gnorm), "kink": out["kink"]}


def validation_nll(p, net, x_val, cfg, u_f, eta, n_train):
    """`O.validation_nll` under the neural likelihood: the mean of delta over the validation set's own rows."""
    out, _ = elbo_value_and_grads(p, net, x_val, cfg, u_f, eta)
    return float(out["nll"]) * n_train / int(x_val.refl_id.shape[0])


# ---- the kernels' own contract, on injected predictions --------------------------------------------------------------------------------------
def kernel_reference(net, iobs, sigiobs, ipred, w_ll):
    """What cl_nlik_forward / cl_nlik_backward compute from ipred (N, S): (delta, sigpred, gradients of  -w_ll sum ll  by autograd, kink)."""
    nt = [t.detach().clone().requires_grad_() for t in net]
    delta, sigpred, _, kink = forward(nt, iobs, sigiobs)
    nll = -w_ll * O.normal_log_prob(f64(ipred), f64(iobs).reshape(-1)[:, None], sigpred[:, None]).sum()
    return delta.detach(), sigpred.detach(), [g for g in torch.autograd.grad(nll, nt)], kink


def flat_of(net):
    """Keras-ordered tensors -> the flat W^T layout of `NeuralLikelihood.raw` (fp32 numpy)."""
    out = []
    for k in range(0, len(net), 2):
        out += [net[k].detach().t().contiguous().reshape(-1), net[k + 1].detach().reshape(-1)]
    return torch.cat(out).to(torch.float32).numpy()


def pick_net(L, w, iobs, sigiobs, first_seed=0, bias=0.1, tries=3000):
    """(net, seed): a glorot-uniform network (`init_net`'s distributions, generator seeded with `first_seed`) whose LeakyReLU units all stay
    clear of their kink on these rows by twice `KINK_REL` (the tests assert one: the second is margin) and whose head stays above `ZH_MIN`
    on every row.  Both are properties of the draw, established on the CPU, unit by unit: the smallest of N pre-activations of a unit
    relative to the layer's largest is ~ 1 / N, so a layer is drawn, the units with a row inside the margin are drawn again -- against the
    layer's own largest pre-activation, until none is left -- and the next layer follows; the head is drawn again until no row sits below
    `ZH_MIN` (the network sees RAW intensities, hundreds to thousands: half the draws put the head's pre-activation at minus a few
    hundred, where softplus underflows to 0 in fp32 and sigpred = 0 -- a non-finite step by the reference's own rules, not a parity case)."""
    g = torch.Generator().manual_seed(int(first_seed))
    dims = [2] + [w] * L + [1]
    h = torch.stack([f64(iobs).reshape(-1), f64(sigiobs).reshape(-1)], dim=1)

    def draw(i, o, n):
        lim = math.sqrt(6.0 / (i + o))
        return (torch.rand(i, n, generator=g, dtype=torch.float64) * 2 - 1) * lim, bias * torch.randn(n, generator=g, dtype=torch.float64)
    net = []
    for k in range(L):
        i, o = dims[k], dims[k + 1]
        W, b = draw(i, o, o)
        for _ in range(tries):
            az = (h @ W + b).abs()
            bad = az.min(dim=0).values < 2.0 * KINK_REL * az.max()
            if not bool(bad.any()):
                break
            W[:, bad], b[bad] = draw(i, o, int(bad.sum()))
        else:
            raise AssertionError(f"layer {k} of a {L} x {w} network: no draw keeps every unit off its kink on {h.shape[0]} rows")
        net += [W, b]
        z = h @ W + b
        h = torch.where(z > 0, z, LEAK * z)
    for _ in range(tries):
        W, b = draw(w, 1, 1)
        if float((h @ W + b).min()) > ZH_MIN:
            return net + [W, b], int(first_seed)
    raise AssertionError(f"no head of a {L} x {w} network stays above {ZH_MIN} on {h.shape[0]} rows")
