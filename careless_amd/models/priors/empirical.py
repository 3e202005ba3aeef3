"""Empirical reference priors: a density centred on structure-factor amplitudes from a conventional experiment, zero on unobserved
Miller indices.

Mirror of `careless/models/priors/empirical.py:9-131` (reference): `ReferencePrior`, `LaplaceReferencePrior`, `NormalReferencePrior`,
`StudentTReferencePrior`, `RiceWoolfsonReferencePrior`, with the reference's constructor signatures.  `Fobs` / `SigFobs` (and `centric`)
hold one entry per OBSERVED reflection when `observed` is given, and are stored as float32.  Like the Wilson priors, on the hot path a
reference prior is only a description: its log-density and z-derivative are evaluated by `cl_ref_prior` (careless_amd/csrc/elbo_q.hip:
ref_prior_kernel) from the arrays of the "what the engine consumes" block below; `log_prob`, `mean` and `stddev` are host-side numpy
(float64 arithmetic, float32 results) for users and tests.
"""
from __future__ import annotations

import math

import numpy as np

from careless_amd.models.merging.surrogate_posteriors import RiceWoolfson
from careless_amd.models.priors.base import Prior


class _LocationScale:
    """Host-side stand-in of a `tfd` location-scale family: float32 parameters, float64 arithmetic."""

    def __init__(self, loc, scale):
        self.loc = np.array(loc, dtype=np.float32)
        self.scale = np.array(scale, dtype=np.float32)

    def _y(self, x):
        return (np.asarray(x, dtype=np.float64) - self.loc.astype(np.float64)) / self.scale.astype(np.float64)

    def mean(self):
        return self.loc.copy()


class Normal(_LocationScale):
    def log_prob(self, x):
        y = self._y(x)
        return (-0.5 * y * y - 0.5 * math.log(2.0 * math.pi) - np.log(self.scale.astype(np.float64))).astype(np.float32)

    def stddev(self):
        return self.scale.copy()


class Laplace(_LocationScale):
    def log_prob(self, x):
        return (-np.abs(self._y(x)) - np.log(2.0 * self.scale.astype(np.float64))).astype(np.float32)

    def stddev(self):
        return (math.sqrt(2.0) * self.scale.astype(np.float64)).astype(np.float32)


class StudentT(_LocationScale):
    def __init__(self, df, loc, scale):
        super().__init__(loc, scale)
        self.df = float(df)

    def log_prob(self, x):
        y, df = self._y(x), self.df
        return (-0.5 * (df + 1.0) * np.log1p(y * y / df) - np.log(np.abs(self.scale.astype(np.float64))) - 0.5 * math.log(df) - 0.5 * math.log(math.pi)
                - math.lgamma(0.5 * df) + math.lgamma(0.5 * (df + 1.0))).astype(np.float32)

    # (tfd.StudentT with allow_nan_stats=True: the mean is undefined for df <= 1, the variance infinite for 1 < df <= 2 and undefined below)
    def mean(self):
        return self.loc.copy() if self.df > 1.0 else np.full_like(self.loc, np.nan)

    def stddev(self):
        if self.df > 2.0:
            return (self.scale.astype(np.float64) * math.sqrt(self.df / (self.df - 2.0))).astype(np.float32)
        return np.full_like(self.scale, np.inf if self.df > 1.0 else np.nan)


class ReferencePrior(Prior):
    """A prior whose `log_prob` is `base_dist.log_prob` on the observed Miller indices and zero on the others (reference
    empirical.py:9-43).  Not meant to be used directly: subclasses set `base_dist` (anything with `log_prob`, `mean`, `stddev`) and
    `engine_kind`."""
    base_dist = None
    engine_kind = None              # "normal" | "laplace" | "studentt" | "rice_woolfson": the density `cl_ref_prior` evaluates
    dof = 0.0                       # Student-t only
    centric = None                  # Rice-Woolfson only (one entry per observed reflection, like Fobs)

    def __init__(self, observed=None):
        super().__init__()
        if observed is None:
            self.idx, self.n_reflections = None, None
        else:
            observed = np.asarray(observed, dtype=bool).reshape(-1)
            self.idx, self.n_reflections = np.nonzero(observed)[0], int(observed.size)

    # -- reference protocol ------------------------------------------------------------------------
    def mean(self):
        """Passes through to `base_dist` (one entry per observed reflection when `observed` was given)."""
        return self.base_dist.mean()

    def stddev(self):
        """Passes through to `base_dist`."""
        return self.base_dist.stddev()

    def log_prob(self, values):
        """values: (..., R).  Zeros on unobserved indices, the base density elsewhere (reference empirical.py:33-43)."""
        values = np.asarray(values)
        if self.idx is None:
            return self.base_dist.log_prob(values)
        out = np.zeros(values.shape, dtype=np.float32)
        out[..., self.idx] = self.base_dist.log_prob(values[..., self.idx])
        return out

    # -- what the engine consumes -----------------------------------------------------------------
    def _full(self, compact, R: int, fill, dtype):
        compact = np.asarray(compact).reshape(-1)
        if self.idx is None:
            if compact.size != R:
                raise ValueError(f"{type(self).__name__} holds {compact.size} reflections, the surrogate posterior {R}")
            return compact.astype(dtype)
        if self.n_reflections != R:
            raise ValueError(f"{type(self).__name__}: `observed` has {self.n_reflections} entries, the surrogate posterior {R} reflections")
        if compact.size != self.idx.size:
            raise ValueError(f"{type(self).__name__}: {compact.size} reference values for {self.idx.size} observed reflections")
        out = np.full(R, fill, dtype=dtype)
        out[self.idx] = compact
        return out

    def loc_full(self, R: int) -> np.ndarray:
        """Fobs of every reflection, float32 (the `loc` array of `cl_refprior_args`; 1 where unobserved: never read)."""
        return self._full(self.base_dist.loc, R, 1.0, np.float32)

    def scale_full(self, R: int) -> np.ndarray:
        """The base distribution's scale of every reflection, float32 (`scale` of `cl_refprior_args`)."""
        return self._full(self.base_dist.scale, R, 1.0, np.float32)

    def observed_mask(self, R: int):
        """0/1 per reflection (`observed` of `cl_refprior_args`), or None: every reflection is observed."""
        if self.idx is None:
            return None
        if self.n_reflections != R:
            raise ValueError(f"{type(self).__name__}: `observed` has {self.n_reflections} entries, the surrogate posterior {R} reflections")
        out = np.zeros(R, dtype=np.uint8)
        out[self.idx] = 1
        return out

    def centric_full(self, R: int):
        """0/1 per reflection (`centric` of `cl_refprior_args`), or None for the kinds that have no centric flag."""
        return None if self.centric is None else self._full(self.centric, R, 0, np.uint8)


class LaplaceReferencePrior(ReferencePrior):
    """Laplace(Fobs, SigFobs / sqrt 2): the scale that gives the density the standard deviation SigFobs (reference empirical.py:45-64)."""
    engine_kind = "laplace"

    def __init__(self, Fobs, SigFobs, observed=None):
        super().__init__(observed)
        self.base_dist = Laplace(np.array(Fobs, dtype=np.float32), np.array(SigFobs, dtype=np.float32) / math.sqrt(2.0))


class NormalReferencePrior(ReferencePrior):
    """Normal(Fobs, SigFobs) (reference empirical.py:66-85)."""
    engine_kind = "normal"

    def __init__(self, Fobs, SigFobs, observed=None):
        super().__init__(observed)
        self.base_dist = Normal(Fobs, SigFobs)


class StudentTReferencePrior(ReferencePrior):
    """StudentT(dof, Fobs, SigFobs) (reference empirical.py:87-108)."""
    engine_kind = "studentt"

    def __init__(self, Fobs, SigFobs, dof, observed=None):
        super().__init__(observed)
        self.dof = float(dof)
        self.base_dist = StudentT(self.dof, Fobs, SigFobs)


class RiceWoolfsonReferencePrior(ReferencePrior):
    """Rice(Fobs, SigFobs) on acentric, FoldedNormal(Fobs, SigFobs) on centric reflections (reference empirical.py:110-131)."""
    engine_kind = "rice_woolfson"

    def __init__(self, Fobs, SigFobs, centric, observed=None):
        super().__init__(observed)
        self.centric = np.array(centric, dtype=bool).reshape(-1)
        self.base_dist = RiceWoolfson(Fobs, SigFobs, self.centric)
