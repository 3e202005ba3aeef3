"""The empirical reference priors of the tests (tests/test_ref_prior.py, tests/test_ref_prior_gpu.py) as the oracle takes them.  The densities
and the whole step under one are the oracle's (`O.ref_log_prob`, `ElboConfig.prior = "reference"` with `ElboInputs.ref`)."""
from __future__ import annotations

from dataclasses import replace

from oracle import elbo_oracle as O

KINDS = ("normal", "laplace", "studentt", "rice_woolfson")


def prior_arrays(prior, R):
    """(kind, loc, scale, observed, centric, dof) of a careless_amd reference prior, full length: what `O.ref_log_prob` takes."""
    return O.RefPrior(prior.engine_kind, prior.loc_full(R), prior.scale_full(R), prior.observed_mask(R), prior.centric_full(R), prior.dof)


def under(x, cfg, prior):
    """(`x` carrying the arrays of `prior`, `cfg` with the reference prior)."""
    return replace(x, ref=prior_arrays(prior, len(x.centric))), replace(cfg, prior="reference")
