"""The problems of the neural-likelihood tests (tests/test_nlik.py, tests/test_nlik_gpu.py): networks whose LeakyReLU units stay clear of
their kink, the kernels' own contract on injected predictions, the engine's flat layout.  The network and the whole step under the
likelihood are the oracle's (`O.nlik_forward`, `ElboConfig.likelihood = "neural"` with `ElboParams.nlik`); `O.nlik_forward` reports the
smallest |pre-activation| of the network's LeakyReLU units relative to its layer's largest: every parity case asserts that it exceeds
`KINK_REL`, so no unit of the fp32 engine can sit on the other branch."""
from __future__ import annotations

import math
from dataclasses import replace

import torch

from oracle import elbo_oracle as O

KINK_REL = 1e-4
ZH_MIN = -10.0            # `pick_net`: delta >= softplus(-10) = 4.5e-5 on every row


def under(cfg):
    """`cfg` with the neural likelihood."""
    return replace(cfg, likelihood="neural")


def with_net(params, net):
    """`params` carrying the network `net`: the same tensor objects, so an optimizer step on the result updates `params` and `net` in place."""
    return replace(params, nlik=list(net))


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


# ---- the kernels' own contract, on injected predictions --------------------------------------------------------------------------------------
def kernel_reference(net, iobs, sigiobs, ipred, w_ll):
    """What cl_nlik_forward / cl_nlik_backward compute from ipred (N, S): (delta, sigpred, gradients of  -w_ll sum ll  by autograd, kink)."""
    nt = [t.detach().clone().requires_grad_() for t in net]
    delta, sigpred, _, kink = O.nlik_forward(nt, iobs, sigiobs)
    nll = -w_ll * O.normal_log_prob(O.f64(ipred), O.f64(iobs).reshape(-1)[:, None], sigpred[:, None]).sum()
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
    h = torch.stack([O.f64(iobs).reshape(-1), O.f64(sigiobs).reshape(-1)], dim=1)

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
        h = torch.where(z > 0, z, O.NLIK_LEAK * z)
    for _ in range(tries):
        W, b = draw(w, 1, 1)
        if float((h @ W + b).min()) > ZH_MIN:
            return net + [W, b], int(first_seed)
    raise AssertionError(f"no head of a {L} x {w} network stays above {ZH_MIN} on {h.shape[0]} rows")
