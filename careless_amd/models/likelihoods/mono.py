"""Monochromatic likelihoods.

Mirror of `careless/models/likelihoods/mono.py:10-73` (reference).  `likelihood(inputs)` returns a small object
bound to (Iobs, SigIobs) with `.log_prob(ipred)`, like the tfd distribution the reference returns.  On the hot path
the engine reads `kind` / `dof` from the likelihood and evaluates log-prob and its derivative inside the fused HIP
kernel `cl_elbo_mono_fwd_bwd` (careless_amd/csrc/elbo_mlp.hip).
"""
from __future__ import annotations

import math

import numpy as np

from careless_amd.models.likelihoods.base import Likelihood


def _squeeze(x):
    x = x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    return np.squeeze(x)


class _BoundLocationScale:
    def __init__(self, kind, loc, scale, dof=None):
        self.kind, self.loc, self.scale, self.dof = kind, loc, scale, dof

    def log_prob(self, x):
        x = np.asarray(x, dtype=np.float64)
        y = (x - self.loc) / self.scale
        if self.kind == "normal":
            return (-0.5 * y * y - 0.5 * math.log(2 * math.pi) - np.log(self.scale)).astype(np.float32)
        if self.kind == "laplace":          # tfd.Laplace(loc, scale): -|x - loc| / scale - log(2 scale)
            return (-np.abs(y) - math.log(2.0) - np.log(self.scale)).astype(np.float32)
        nu = float(self.dof)
        return (-0.5 * (nu + 1.0) * np.log1p(y * y / nu) - np.log(np.abs(self.scale)) - 0.5 * math.log(nu)
                - 0.5 * math.log(math.pi) - math.lgamma(0.5 * nu) + math.lgamma(0.5 * (nu + 1.0))).astype(np.float32)

    def mean(self):
        return self.loc

    def stddev(self):
        if self.kind == "laplace":          # (as tfd.Laplace answers: sqrt 2 * scale)
            return math.sqrt(2.0) * self.scale
        return self.scale


class LocationScaleLikelihood(Likelihood):
    kind = None
    dof = None

    def get_loc_and_scale(self, inputs):
        return _squeeze(self.get_intensities(inputs)), _squeeze(self.get_uncertainties(inputs))


class NormalLikelihood(LocationScaleLikelihood):
    """Normal(Iobs, SigIobs)  (reference mono.py:16-18)."""
    kind = "normal"

    def call(self, inputs):
        return _BoundLocationScale("normal", *self.get_loc_and_scale(inputs))


class LaplaceLikelihood(LocationScaleLikelihood):
    """Laplace(Iobs, SigIobs / sqrt 2)  (reference mono.py:20-23)."""
    kind = "laplace"

    def call(self, inputs):
        loc, scale = self.get_loc_and_scale(inputs)
        return _BoundLocationScale("laplace", loc, scale / math.sqrt(2.0))


class StudentTLikelihood(LocationScaleLikelihood):
    """StudentT(dof, Iobs, SigIobs)  (reference mono.py:25-37)."""
    kind = "studentt"

    def __init__(self, dof):
        super().__init__()
        self.dof = dof

    def call(self, inputs):
        return _BoundLocationScale("studentt", *self.get_loc_and_scale(inputs), dof=self.dof)


_SOFTPLUS_INV_ONE = float(np.log(np.e - 1.0))      # softplus(raw) == 1


class Ev11Likelihood(LocationScaleLikelihood):
    """Evans-2011 error model with three learnable scalars Sdfac, Sdadd, SdB (each Softplus-transformed, initial value 1):
    sigma_c = Sdfac * sqrt(SigIobs^2 + SdB * softplus(ipred) + Sdadd * softplus(ipred)^2)  (reference mono.py:39-59)."""
    ev11 = True

    def __init__(self, *args, **kwargs):
        super().__init__()
        import torch
        # raw (pre-softplus) values in the reference's variable order: Sdfac, Sdadd, SdB
        self.raw = torch.full((3,), _SOFTPLUS_INV_ONE, dtype=torch.float32)
        self.loc = None
        self.scale = None

    @property
    def Sdfac(self):
        return float(np.log1p(np.exp(float(self.raw[0]))))

    @property
    def Sdadd(self):
        return float(np.log1p(np.exp(float(self.raw[1]))))

    @property
    def SdB(self):
        return float(np.log1p(np.exp(float(self.raw[2]))))

    @property
    def trainable_variables(self):
        return [self.raw]

    def call(self, inputs):
        self.loc, self.scale = self.get_loc_and_scale(inputs)
        return self

    def corrected_sigiobs(self, ipred):
        ipred = np.asarray(ipred, dtype=np.float64)
        sp = np.logaddexp(0.0, ipred)
        return self.Sdfac * np.sqrt(np.square(self.scale) + self.SdB * sp + self.Sdadd * np.square(sp))

    def log_prob(self, ipred):
        return _BoundLocationScale(self.kind, self.loc, self.corrected_sigiobs(ipred), dof=self.dof).log_prob(ipred)


class NormalEv11Likelihood(Ev11Likelihood):
    kind = "normal"


class StudentTEv11Likelihood(Ev11Likelihood):
    kind = "studentt"

    def __init__(self, dof, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.dof = dof


# ------------------------------------------------------------------------------------------------------------
# the neural likelihood: an error model learned from the data
# ------------------------------------------------------------------------------------------------------------
def lik_dense_slices(L: int, w: int):
    """The likelihood network's flat layout tensor by tensor, [(kernel offset, out, in, bias offset)]: the scaler's W^T layout
    (`models.scaling.nn.dense_layout`) on the two columns (Iobs, SigIobs), with a one-row head [1][fan-in] + 1 bias in place of Dense(2)."""
    from careless_amd.models.scaling.nn import dense_layout
    layers, head = dense_layout(2, w, L)
    fan_in = w if L else 2
    return [(ow, w, i, ob) for ow, ob, i in layers] + [(head, 1, fan_in, head + fan_in)]


def lik_param_count(L: int, w: int) -> int:
    return lik_dense_slices(L, w)[-1][3] + 1


class NeuralLikelihood(LocationScaleLikelihood):
    """Likelihood whose uncertainties come from a small network on the raw (Iobs, SigIobs) of every observation (reference mono.py:75-106):
        network = mlp_layers x Dense(mlp_width, LeakyReLU(0.3)) -> Dense(1, softplus)       delta = network(concat(iobs, sigiobs))
        sigpred = sigiobs * delta / mean(delta)        (the mean over ALL rows of the set the likelihood is called on)
    The parameters live in one flat float32 tensor `raw` (`lik_dense_slices`); `weights` are Keras-shaped views of it.  On the hot path the
    engine evaluates and differentiates the network in csrc/elbo_nlik.hip; `call` answers on the host in fp64."""
    neural = True
    leakiness = 0.3          # tfk.layers.LeakyReLU() -- tf_keras' default slope, not the scaler's 0.01

    def __init__(self, mlp_layers, mlp_width):
        super().__init__()
        self.n_layers, self.width = int(mlp_layers), int(mlp_width)
        if self.n_layers < 1 or self.width < 1:
            raise ValueError("NeuralLikelihood needs mlp_layers >= 1 and mlp_width >= 1")
        self.raw = None
        self.trainable = True

    def base_dist(self, loc, scale):
        raise NotImplementedError("extensions of this class must implement a base_dist(loc, scale) method")

    # -- parameters ---------------------------------------------------------------------------------------
    def layer_slices(self):
        return lik_dense_slices(self.n_layers, self.width)

    def param_count(self) -> int:
        return lik_param_count(self.n_layers, self.width)

    def build(self, device=None, seed=None):
        """Keras' defaults: glorot-uniform kernels (limit sqrt(6 / (fan_in + fan_out))), zero biases; `seed` seeds a torch generator."""
        import torch
        if self.raw is not None:
            return
        gen = torch.Generator()
        if seed is not None:
            gen.manual_seed(int(seed))
        raw = torch.zeros(self.param_count(), dtype=torch.float32)
        for off, o, i, _ in self.layer_slices():
            lim = math.sqrt(6.0 / (i + o))
            raw[off:off + o * i] = (torch.rand(o * i, generator=gen, dtype=torch.float32) * 2.0 - 1.0) * lim
        self.raw = raw.to(device) if device is not None else raw

    @property
    def weights(self):
        """[kernel_0 (in, out), bias_0, ..., head kernel (in, 1), head bias (1,)] -- Keras order, views into `raw`."""
        self.build()
        out = []
        for off, o, i, boff in self.layer_slices():
            out.append(self.raw[off:off + o * i].view(o, i).t())
            out.append(self.raw[boff:boff + o])
        return out

    def set_weights(self, weights):
        import torch
        for dst, src in zip(self.weights, weights):
            dst.copy_(torch.as_tensor(np.asarray(src), dtype=torch.float32))

    @property
    def trainable_variables(self):
        return self.weights if self.trainable else []

    def save_weights(self, path):
        import torch
        self.build()
        torch.save({"raw": self.raw.detach().cpu(), "n_layers": self.n_layers, "width": self.width}, path)

    def load_weights(self, path):
        import torch
        st = torch.load(path)
        if int(st["n_layers"]) != self.n_layers or int(st["width"]) != self.width:
            raise ValueError(f"weights of a {int(st['n_layers'])} x {int(st['width'])} network, this likelihood is {self.n_layers} x {self.width}")
        self.build()
        self.raw.copy_(st["raw"])

    # -- forward (host, fp64) -----------------------------------------------------------------------------
    def delta(self, iobs, sigiobs):
        """The network's output for the rows given, in fp64 on the host from the current weights."""
        ws = [np.asarray(t.detach().cpu().numpy(), dtype=np.float64) for t in self.weights]
        h = np.stack([np.asarray(iobs, dtype=np.float64).reshape(-1), np.asarray(sigiobs, dtype=np.float64).reshape(-1)], axis=1)
        for k in range(self.n_layers):
            z = h @ ws[2 * k] + ws[2 * k + 1]
            h = np.where(z > 0, z, self.leakiness * z)
        return np.logaddexp(0.0, h @ ws[-2] + ws[-1])[:, 0]

    def sigpred(self, iobs, sigiobs):
        """sigiobs * delta / mean(delta) of the rows given (host, fp64)."""
        delta = self.delta(iobs, sigiobs)
        return np.asarray(sigiobs, dtype=np.float64).reshape(-1) * delta / np.mean(delta)

    def call(self, inputs):
        loc, scale = self.get_loc_and_scale(inputs)
        return self.base_dist(np.asarray(loc, dtype=np.float64), self.sigpred(loc, scale))


class NeuralNormalLikelihood(NeuralLikelihood):
    """Normal(Iobs, sigpred)  (reference mono.py:108-110)."""
    kind = "normal"

    def base_dist(self, loc, scale):
        return _BoundLocationScale("normal", loc, scale)
