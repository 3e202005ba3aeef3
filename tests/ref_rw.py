"""The problems of the Rice-Woolfson posterior's tests (tests/test_rw_posterior.py, tests/test_rw_posterior_gpu.py): noise whose centric draws
stay off the kink of |.|.  The posterior and whole steps under it are the oracle's (`O.rw_sample`, `O.rw_log_prob`, `O.rw_moments`,
`ElboConfig.posterior = "rice_woolfson"`); the (2, S, R) standard normals n1, n2 go in through the `u_f` argument."""
from __future__ import annotations

from dataclasses import replace

import numpy as np

KINK_GUARD = 1e-4         # no centric draw with |loc + scale n1| < KINK_GUARD * scale: fp32 could land on the other side of |.|'s kink


def under(cfg):
    """`cfg` with the Rice-Woolfson posterior."""
    return replace(cfg, posterior="rice_woolfson")


def kink_margin(loc, scale, centric, n):
    """min over the centric draws of |loc + scale n1| / scale (inf without a centric reflection)."""
    c = np.asarray(centric, dtype=bool)
    if not c.any():
        return np.inf
    loc, scale, n1 = (np.asarray(a, dtype=np.float64) for a in (loc, scale, np.asarray(n)[0]))
    return float(np.min(np.abs(loc + scale * n1)[..., c] / scale[c]))


def noise_for(loc, scale, centric, S, seed):
    """(2, S, R) fp32 standard normals whose centric draws keep KINK_GUARD (the first seed from `seed` on that does; checked on the CPU)."""
    R = len(np.asarray(loc))
    for k in range(seed, seed + 100):
        n = np.random.default_rng(k).normal(size=(2, S, R)).astype(np.float32)
        if kink_margin(loc, scale, centric, n) >= KINK_GUARD:
            return n
    raise AssertionError("no seed keeps the centric draws off the kink")
