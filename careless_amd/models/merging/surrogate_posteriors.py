"""Learnable surrogate posterior over structure-factor amplitudes.

Mirror of `careless/models/merging/surrogate_posteriors.py:11-131` (reference): `TruncatedNormal` with
`from_loc_and_scale` (loc = Exp(raw), scale = Shift(eps)(Exp(raw))), `sample` clamped at `low`, `log_prob`, `mean`,
`stddev`, `moment_4`.  Sampling, log-prob and their gradients on the training path run in the HIP kernels
`cl_tn_forward` / `cl_tn_backward`; the moment accessors used by the output step (`mean`, `stddev`, `moment_4(method='tf')`) run
in `cl_tn_moments`.  `moment_4(method='scipy')` is scipy on the host, as in the reference.

`RiceWoolfson` (reference surrogate_posteriors.py:133-172) has two forms.  `RiceWoolfson(loc, scale, centric)` on fixed arrays is the
host-side base distribution of `RiceWoolfsonReferencePrior` (careless_amd/models/priors/empirical.py).
`RiceWoolfson.from_loc_and_scale(loc, scale, centric)` is a trainable surrogate posterior of the HIP engine (`TrainableRiceWoolfson`):
sampling, log-prob and gradients in `cl_rw_forward` / `cl_rw_backward`, the output step's moments in `cl_rw_moments`.
"""
from __future__ import annotations

import math

import numpy as np
import torch


def _t(x, device=None):
    if torch.is_tensor(x):
        return x.detach().to(dtype=torch.float32, device=device)
    return torch.as_tensor(np.asarray(x, dtype=np.float32), device=device)


def _ndtr(x):
    return torch.special.ndtr(x)


class SurrogatePosterior:
    """Base class for learnable variational distributions over structure factor amplitudes."""
    trainable = True

    def moment_4(self):
        raise NotImplementedError("The fourth moment of this distribution is not implemented yet.")


class TruncatedNormal(SurrogatePosterior):
    """q(F): one truncated normal per reflection (reference surrogate_posteriors.py:12-131).  `sample`, `mean`, `stddev`, `variance` and
    `moment_4` run on the GPU through the C-ABI (`cl_tn_forward`, `cl_tn_moments`: fp64 closed forms on the device) and return CUDA tensors
    without autograd history; without the library or a GPU they raise `CarelessHipError` (there is no CPU path: `engine.require_gpu`).  A
    host-side reader of a saved posterior (a pickle opened on a login node) takes the moments from the written MTZ columns, or from
    `scipy.stats.truncnorm((low - loc) / scale, (high - loc) / scale, loc, scale)` on `loc` / `scale`, which are plain tensors.
    `log_prob` is torch arithmetic on the parameters' device."""

    def __init__(self, loc_raw, scale_raw, low, high=1e10, scale_shift=1e-7):
        """Holds the *raw* trainable vectors a = log(loc), b = log(scale - scale_shift)."""
        self.loc_raw = _t(loc_raw)
        self.scale_raw = _t(scale_raw)
        low = _t(low)
        self.low = low.expand_as(self.loc_raw).contiguous() if low.dim() == 0 or low.numel() == 1 else low
        self.high = float(high)
        self.scale_shift = float(scale_shift)
        self.trainable = True

    @classmethod
    def from_loc_and_scale(cls, loc, scale, low=0.0, high=1e10, scale_shift=1e-7):
        """Instantiate a learnable distribution with the reference's bijectors (surrogate_posteriors.py:104-131)."""
        loc = np.asarray(loc.detach().cpu() if torch.is_tensor(loc) else loc, dtype=np.float64)
        scale = np.asarray(scale.detach().cpu() if torch.is_tensor(scale) else scale, dtype=np.float64)
        return cls(np.log(loc).astype(np.float32), np.log(scale - scale_shift).astype(np.float32), low, high, scale_shift)

    # -- parameters ---------------------------------------------------------------------------------------
    @property
    def loc(self):
        return torch.exp(self.loc_raw)

    @property
    def scale(self):
        return torch.exp(self.scale_raw) + self.scale_shift

    @property
    def parameters(self):
        return {"loc": self.loc, "scale": self.scale, "low": self.low, "high": self.high}

    def parameter_properties(self):
        return {"loc": None, "scale": None, "low": None, "high": None}

    @property
    def trainable_variables(self):
        return [self.loc_raw, self.scale_raw] if self.trainable else []

    def save_weights(self, path):
        torch.save({"loc_raw": self.loc_raw.detach().cpu(), "scale_raw": self.scale_raw.detach().cpu()}, path)

    def load_weights(self, path):
        st = torch.load(path)
        self.loc_raw.copy_(st["loc_raw"])
        self.scale_raw.copy_(st["scale_raw"])

    # -- distribution protocol ------------------------------------------------------------------------------
    def sample(self, sample_shape=(), seed=None):
        """max(low, TruncatedNormal sample) (surrogate_posteriors.py:50-53); runs `cl_tn_forward` on the GPU."""
        from careless_amd.engine import tn_sample
        n = 1 if sample_shape in ((), None) else int(sample_shape)
        z = tn_sample(self, n, seed=seed)
        return z[0] if sample_shape in ((), None) else z

    def _std_bounds(self):
        loc, scale = self.loc, self.scale
        return (self.low - loc) / scale, (self.high - loc) / scale

    def log_prob(self, z):
        z = _t(z, self.loc_raw.device)
        loc, scale = self.loc, self.scale
        a, b = self._std_bounds()
        zn = _ndtr(-a) - _ndtr(-b)
        y = (z - loc) / scale
        lp = -(0.5 * y * y + 0.5 * math.log(2 * math.pi) + torch.log(scale) + torch.log(zn))
        return torch.where((z < self.low) | (z > self.high), torch.full_like(lp, -math.inf), lp)

    def mean(self):
        """E[z] of the truncated normal (tfd.TruncatedNormal.mean behind surrogate_posteriors.py:23-24); `cl_tn_moments` on the GPU."""
        from careless_amd.engine import tn_moments
        return tn_moments(self, want=("mean",))["mean"]

    def stddev(self):
        """sqrt(Var[z]) (surrogate_posteriors.py:26-27); `cl_tn_moments` on the GPU."""
        from careless_amd.engine import tn_moments
        return tn_moments(self, want=("std",))["std"]

    def variance(self):
        sd = self.stddev()
        return sd * sd

    def moment_4(self, high=np.inf, method="scipy"):
        """Fourth raw moment (surrogate_posteriors.py:55-102).  'scipy' = scipy.stats.truncnorm.moment,
        'tf' = the closed form of `_tf_moment_4`, evaluated by `cl_tn_moments` on the GPU (fp64)."""
        if method == "scipy":
            from scipy.stats import truncnorm
            loc = self.loc.detach().cpu().numpy().astype(np.float64)
            scale = self.scale.detach().cpu().numpy().astype(np.float64)
            low = self.low.detach().cpu().numpy().astype(np.float64)
            hi = self.high if high is None else high
            a, b = (low - loc) / scale, (hi - loc) / scale
            return truncnorm.moment(4, a, b, loc, scale)
        if method == "tf":
            from careless_amd.engine import tn_moments
            hi = self.high if high is None else high
            return tn_moments(self, high_m4=hi, want=("m4",))["m4"].cpu().numpy()
        raise ValueError(f"Unknown method {method} for computing moment_4")


class RiceWoolfson:
    """Rice(loc, scale) for acentric and FoldedNormal ("Woolfson") for centric reflections: the hybrid distribution of reference
    surrogate_posteriors.py:133-172.  Built from fixed arrays, `RiceWoolfson(loc, scale, centric)`, it is host-side (numpy / scipy, float64
    arithmetic, float32 results): the base distribution of `RiceWoolfsonReferencePrior`, whose density on the training path is
    `cl_ref_prior`'s (csrc/cl_math.h: cl_rice_log_prob, cl_folded_normal_log_prob).  `RiceWoolfson.from_loc_and_scale(loc, scale, centric)`
    gives the trainable surrogate posterior of the HIP engine, `TrainableRiceWoolfson`."""

    def __init__(self, loc, scale, centric):
        self.loc = np.array(loc, dtype=np.float32)
        self.scale = np.array(scale, dtype=np.float32)
        self.centric = np.array(centric, dtype=bool)
        self.eps = np.finfo(np.float32).eps

    @classmethod
    def from_loc_and_scale(cls, loc, scale, centric, scale_shift=1e-7):
        """A learnable Rice-Woolfson posterior with the bijectors of `TruncatedNormal.from_loc_and_scale`: loc = Exp(raw),
        scale = Shift(scale_shift)(Exp(raw)).  (The reference wraps `loc_var` / `scale_var` the caller made; it has no such constructor.)"""
        loc = np.asarray(loc.detach().cpu() if torch.is_tensor(loc) else loc, dtype=np.float64)
        scale = np.asarray(scale.detach().cpu() if torch.is_tensor(scale) else scale, dtype=np.float64)
        return TrainableRiceWoolfson(np.log(loc).astype(np.float32), np.log(scale - scale_shift).astype(np.float32), centric, scale_shift)

    def _pick(self, woolfson, rice):
        return np.where(self.centric, woolfson, rice).astype(np.float32)

    def _moments(self):
        """(mean, variance) of both families in float64.  Folded normal: scipy.stats.foldnorm.  Rice: mean = scale sqrt(pi / 2) L_1/2(-t),
        t = loc^2 / (2 scale^2), with the Laguerre function written on exponentially scaled Bessel functions, L_1/2(-t) = (1 + t) i0e(t / 2) +
        t i1e(t / 2) -- finite at any loc / scale, where the unscaled closed form overflows; variance = 2 scale^2 + loc^2 - mean^2."""
        from scipy import special, stats
        loc, scale = self.loc.astype(np.float64), self.scale.astype(np.float64)
        w = stats.foldnorm(loc / scale, scale=scale)
        t = 0.5 * (loc / scale) ** 2
        r_mean = scale * math.sqrt(0.5 * math.pi) * ((1.0 + t) * special.i0e(0.5 * t) + t * special.i1e(0.5 * t))
        r_var = np.maximum(2.0 * scale ** 2 + loc ** 2 - r_mean ** 2, 0.0)
        return (w.mean(), r_mean), (w.var(), r_var)

    def mean(self):
        return self._pick(*self._moments()[0])

    def variance(self):
        return self._pick(*self._moments()[1])

    def stddev(self):
        return self._pick(*np.sqrt(self._moments()[1]))

    def sample(self, sample_shape=(), seed=None):
        """Folded normal draws (+ float32 eps, as the reference: off the boundary of the support) and Rice draws |loc + scale (n1 + i n2)|."""
        rng = np.random.default_rng(seed)
        shape = (() if sample_shape in ((), None) else (int(sample_shape),)) + self.loc.shape
        loc, scale = self.loc.astype(np.float64), self.scale.astype(np.float64)
        n1, n2 = rng.normal(size=shape), rng.normal(size=shape)
        return self._pick(np.abs(loc + scale * n1) + self.eps, np.hypot(loc + scale * n1, scale * n2))

    def log_prob(self, x):
        """where(centric, FoldedNormal.log_prob(x), Rice.log_prob(x)) (reference surrogate_posteriors.py:168-169)."""
        from scipy import special
        x = np.asarray(x, dtype=np.float64)
        loc, scale = self.loc.astype(np.float64), self.scale.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            arg = x * loc / scale ** 2
            rice = np.log(x) - 2 * np.log(scale) - (x * x + loc * loc) / (2 * scale ** 2) + np.log(special.i0e(arg)) + np.abs(arg)
            fn = np.logaddexp(-0.5 * ((x - loc) / scale) ** 2, -0.5 * ((-x - loc) / scale) ** 2) - 0.5 * math.log(2 * math.pi) - np.log(scale)
        return self._pick(fn, rice)

    def prob(self, x):
        return np.exp(self.log_prob(x))


class TrainableRiceWoolfson(SurrogatePosterior):
    """q(F): Rice(loc, scale) per acentric and FoldedNormal(loc, scale) per centric reflection with trainable loc = exp(a) and
    scale = exp(b) + scale_shift -- reference surrogate_posteriors.py:133-172 around two `TransformedVariable`s, which is what
    `VariationalMergingModel(RiceWoolfson(loc_var, scale_var, centric), ...)` trains there.  Made by `RiceWoolfson.from_loc_and_scale`.

    Sampling, log-density and their gradients on the training path run in the HIP kernels `cl_rw_forward` / `cl_rw_backward`
    (csrc/elbo_q.hip): a centric draw is |loc + scale n1| + eps32 (reference :166), an acentric one sqrt((scale n1)^2 + (loc + scale n2)^2)
    (careless/utils/distributions.py:252-258), differentiated pathwise.  `sample`, `mean`, `stddev`, `variance` and `moment_4` run on the
    GPU (`cl_rw_forward`, `cl_rw_moments`) and raise `CarelessHipError` without one; `log_prob` is torch arithmetic on the host.

    `mean` / `stddev` are those of the host class `RiceWoolfson._moments`: the exact Rice mean on exponentially scaled Bessel functions at
    any loc / scale (the reference's Rice switches to the normal limit beyond loc / scale = 40) and scipy.stats.foldnorm's.  `moment_4` is
    OURS: the reference defines none for this class, so its `get_predictions` would raise; here it is the closed form
    loc^4 + 8 scale^2 loc^2 + 8 scale^4 (Rice) and loc^4 + 6 loc^2 scale^2 + 3 scale^4 (folded normal)."""
    posterior_kind = "rice_woolfson"

    def __init__(self, loc_raw, scale_raw, centric, scale_shift=1e-7):
        """Holds the *raw* trainable vectors a = log(loc), b = log(scale - scale_shift) and the 0/1 family flag per reflection."""
        self.loc_raw = _t(loc_raw)
        self.scale_raw = _t(scale_raw)
        self.centric = np.array(centric.detach().cpu() if torch.is_tensor(centric) else centric, dtype=bool).reshape(-1)
        if self.centric.size != self.loc_raw.numel() or self.scale_raw.numel() != self.loc_raw.numel():
            raise ValueError("loc, scale and centric must have one entry per reflection")
        self.scale_shift = float(scale_shift)
        self.eps = float(np.finfo(np.float32).eps)
        # the support is [0, inf) without a truncation bound; the engine's argument fill names the two all the same (never read by cl_rw_*)
        self.low = torch.zeros_like(self.loc_raw)
        self.high = 1e10
        self.trainable = True

    @property
    def loc(self):
        return torch.exp(self.loc_raw)

    @property
    def scale(self):
        return torch.exp(self.scale_raw) + self.scale_shift

    @property
    def parameters(self):
        return {"loc": self.loc, "scale": self.scale, "centric": self.centric}

    def parameter_properties(self):
        return {"loc": None, "scale": None, "centric": None}

    @property
    def trainable_variables(self):
        return [self.loc_raw, self.scale_raw] if self.trainable else []

    def save_weights(self, path):
        torch.save({"loc_raw": self.loc_raw.detach().cpu(), "scale_raw": self.scale_raw.detach().cpu()}, path)

    def load_weights(self, path):
        st = torch.load(path)
        self.loc_raw.copy_(st["loc_raw"])
        self.scale_raw.copy_(st["scale_raw"])

    def sample(self, sample_shape=(), seed=None):
        """Reference surrogate_posteriors.py:162-166; runs `cl_rw_forward` on the GPU."""
        from careless_amd.engine import tn_sample
        n = 1 if sample_shape in ((), None) else int(sample_shape)
        z = tn_sample(self, n, seed=seed)
        return z[0] if sample_shape in ((), None) else z

    def log_prob(self, z):
        """where(centric, FoldedNormal.log_prob(z), Rice.log_prob(z)) (reference :168-169), float64 torch arithmetic, float32 result.  The
        Rice exponent is taken as -(z - loc)^2 / 2 scale^2 + log i0e(z loc / scale^2): no cancellation at loc >> scale."""
        dev = self.loc_raw.device
        z = _t(z, dev).double()
        loc, scale = self.loc.double(), self.scale.double()
        c = torch.as_tensor(self.centric, device=dev)
        rice = torch.log(z) - 2 * torch.log(scale) - 0.5 * ((z - loc) / scale) ** 2 + torch.log(torch.special.i0e(z * loc / scale ** 2))
        fn = torch.logaddexp(-0.5 * ((z - loc) / scale) ** 2, -0.5 * ((-z - loc) / scale) ** 2) - 0.5 * math.log(2 * math.pi) - torch.log(scale)
        return torch.where(c, fn, rice).float()

    def mean(self):
        from careless_amd.engine import tn_moments
        return tn_moments(self, want=("mean",))["mean"]

    def stddev(self):
        from careless_amd.engine import tn_moments
        return tn_moments(self, want=("std",))["std"]

    def variance(self):
        sd = self.stddev()
        return sd * sd

    def moment_4(self, high=None, method=None):
        """Fourth raw moment, closed form, fp64 on the GPU (`cl_rw_moments`).  Not in the reference (class docstring); `high` and `method`
        are accepted for the call sites written for `TruncatedNormal.moment_4` and ignored."""
        from careless_amd.engine import tn_moments
        return tn_moments(self, want=("m4",))["m4"].cpu().numpy()
