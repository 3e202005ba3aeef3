"""The problems of the Laplace-likelihood tests (tests/test_laplace.py, tests/test_laplace_gpu.py).  The density and the whole step under it
are the oracle's (`O.laplace_log_prob`, `ElboConfig.likelihood = "laplace"`; the gradient of abs is sign, 0 at 0, as TensorFlow's).

The problems of util.make_problem put every prediction far below its observation: every residual has one sign and the derivative of the
Laplace term is one constant.  `rewrite_observations` moves the observations onto the predictions (see there)."""
from __future__ import annotations

from dataclasses import replace

import numpy as np
import torch

from oracle import elbo_oracle as O

GUARD_REL = 1e-4          # the guard round the kink, relative to gmax * max|ipred|: every test asserts the engine's ipred within 1e-4 of max|ipred|, so a
                          # sum over a harmonic group of gmax rows is within one guard and no sample outside the guard changes sides


def under(cfg):
    """`cfg` with the Laplace likelihood."""
    return replace(cfg, likelihood="laplace")


# ---- the problem: observations on both sides of the predictions, none on the kink -----------------------------------------------------------
def counted_slots(data):
    """Slots that hold an observation: every row (monochromatic), the first n_groups slots (Laue; the rest is the (1.0, 1.0) padding)."""
    N = len(data["refl_id"])
    return N if data.get("harmonic_id") is None else int(np.max(data["harmonic_id"])) + 1


def guard_of(data, ipred):
    gmax = 1 if data.get("harmonic_id") is None else int(np.bincount(np.asarray(data["harmonic_id"]).reshape(-1)).max())
    return GUARD_REL * gmax * float(np.max(np.abs(ipred)))


def predictions(data, cfg, params, u_f, eta):
    """(ipred (S, N), what the likelihood sees (S, N)) of the fp64 reference: independent of Iobs / SigIobs."""
    x = O.inputs_from_numpy(data)
    with torch.no_grad():
        out = O.elbo_forward(params, x, cfg, O.f64(u_f), O.f64(eta))
    return out["ipred"].numpy(), out["ipred_l"].numpy()


def rewrite_observations(data, cfg, params, noises, seed=0):
    """A copy of `data` with  Iobs := m + 1.5 sigma n,  SigIobs := sigma  on the counted slots: m the sample-mean reference prediction of the
    slot (over every (u_f, eta) of `noises`), sigma = 0.1 |m| + 0.05 mean|m|, n standard normal.  Then every observation with a sample of any
    of the noises inside TWO guards is moved up by 3 guards, until none is (the tests ask for one guard: the second is margin).  Returns
    (data, nudging rounds)."""
    data = dict(data)
    preds = [predictions(data, cfg, params, u, e) for u, e in noises]
    ipl = np.concatenate([p[1] for p in preds], axis=0)                 # (samples of every noise, N)
    guard = max(guard_of(data, p[0]) for p in preds)
    G = counted_slots(data)
    m = ipl[:, :G].mean(axis=0)
    sigma = 0.1 * np.abs(m) + 0.05 * np.mean(np.abs(m))
    rng = np.random.default_rng(1000 + seed)
    iobs = np.array(data["iobs"], dtype=np.float32, copy=True).reshape(-1)
    sig = np.array(data["sigiobs"], dtype=np.float32, copy=True).reshape(-1)
    iobs[:G] = (m + 1.5 * sigma * rng.normal(size=G)).astype(np.float32)
    sig[:G] = sigma.astype(np.float32)
    rounds = 0
    while True:
        bad = (np.abs(ipl - iobs[None, :].astype(np.float64)) < 2.0 * guard).any(axis=0)
        if not bad.any():
            break
        iobs[bad] = (iobs[bad].astype(np.float64) + 3.0 * guard).astype(np.float32)
        rounds += 1
        assert rounds < 50
    data["iobs"], data["sigiobs"] = iobs, sig
    return data, rounds


def assert_conditions(data, ipred, ipred_l):
    """The two conditions every test on injected noise asserts on the fp64 reference alone: no (slot, sample) pair within the guard of its
    observation, each sign of the residual on at least 25 % of the counted pairs.  Returns (smallest gap / guard, positive fraction)."""
    guard = guard_of(data, ipred)
    res = np.asarray(ipred_l, dtype=np.float64) - np.asarray(data["iobs"], dtype=np.float64).reshape(-1)[None, :]
    gap = float(np.min(np.abs(res))) / guard
    pos = float(np.mean(res[:, :counted_slots(data)] > 0))
    assert gap >= 1.0, gap
    assert 0.25 <= pos <= 0.75, pos
    return gap, pos
