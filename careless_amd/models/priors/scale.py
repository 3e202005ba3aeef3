"""Priors on the scale distribution: what a user hands `VariationalMergingModel(..., scale_prior=...)`.

The reference takes any `tfd` distribution there (careless/models/merging/variational.py:22-36) and uses it in one place: the
"Σ KLDiv" term of `call` (:156-163).  These classes are host-side stand-ins for the `tfd` objects, in the style of
`ReferencePrior.engine_kind`: the full-support location-scale families whose log-density and derivative the HIP library already
evaluates (csrc/cl_math.h: cl_ref_prior_log_prob), each with scalar parameters.  On the hot path a scale prior is only a description --
`cl_scale_kl` (csrc/elbo_sprior.hip) evaluates the term from `engine_kind`, `loc`, `scale` and `df` --; `log_prob` is host-side (float64
arithmetic on host tensors or arrays) for users and tests.  Priors without full support (Exponential, HalfNormal) are not offered: a scale
sample may be negative, where their log-density is -inf in the reference too.
"""
from __future__ import annotations

import math

import numpy as np
import torch


class ScalePrior:
    """A location-scale density with scalar parameters.  Subclasses set `engine_kind` and `_log_density(y)`, y = (x - loc) / scale."""
    engine_kind = None              # "normal" | "laplace" | "studentt": cl_sprior_args.kind
    df = 0.0                        # Student-t only

    def __init__(self, loc, scale):
        self.loc, self.scale = float(loc), float(scale)
        if not (math.isfinite(self.loc) and math.isfinite(self.scale) and self.scale > 0.0):
            raise ValueError(f"{type(self).__name__} needs a finite loc and a finite scale > 0 (got loc={loc}, scale={scale})")

    def _log_density(self, y):
        raise NotImplementedError

    def log_prob(self, x):
        """log p(x), elementwise: a float64 tensor for a tensor, a float64 array for anything else."""
        if torch.is_tensor(x):
            y = (x.detach().cpu().double() - self.loc) / self.scale
            return self._log_density(y) - math.log(self.scale)
        y = (np.asarray(x, dtype=np.float64) - self.loc) / self.scale
        return self._log_density(torch.as_tensor(y)).numpy() - math.log(self.scale)

    def __repr__(self):
        df = f"df={self.df}, " if self.engine_kind == "studentt" else ""
        return f"{type(self).__name__}({df}loc={self.loc}, scale={self.scale})"


class NormalScalePrior(ScalePrior):
    """tfd.Normal(loc, scale).  Against a bare Normal scale distribution the term is the analytic KL, as in TFP."""
    engine_kind = "normal"

    def _log_density(self, y):
        return -0.5 * y * y - 0.5 * math.log(2.0 * math.pi)


class LaplaceScalePrior(ScalePrior):
    """tfd.Laplace(loc, scale)."""
    engine_kind = "laplace"

    def _log_density(self, y):
        return -y.abs() - math.log(2.0)


class StudentTScalePrior(ScalePrior):
    """tfd.StudentT(df, loc, scale)."""
    engine_kind = "studentt"

    def __init__(self, df, loc, scale):
        super().__init__(loc, scale)
        self.df = float(df)
        if not (math.isfinite(self.df) and self.df > 0.0):
            raise ValueError(f"StudentTScalePrior needs a finite df > 0 (got {df})")

    def _log_density(self, y):
        df = self.df
        return (-0.5 * (df + 1.0) * torch.log1p(y * y / df) - 0.5 * math.log(df * math.pi) - math.lgamma(0.5 * df) + math.lgamma(0.5 * (df + 1.0)))
