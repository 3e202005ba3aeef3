"""The oracle's later families against the derivation their first references used: a family enters the loss through one term only, so the
step under it is the golden-pinned baseline step with that term traded on the SAME attached predictions / samples,

    likelihood:  nll  += w sum (baseline_lp - family_lp)(ipred_l),                 w = 1 / S, or 1 / (S N) under `kl_weight`
    prior:       kl   += w sum over the KL's columns of (wilson_lp - ref_lp)(z_f),  w = 1 / S, or 1 / (S columns) under `kl_weight`,

`loss` moving with `nll`, and with `kl_weight` times the `kl` term.  `O.elbo_forward` computes each family directly; here the trade is done
by hand on the baseline's graph and the two are compared -- loss terms, predictions and every gradient -- at the bounds tests/test_golden.py
uses to say "the oracle did not move".  CPU only, on util.make_problem's default shape (N = 300, R = 40, 2 x 32, S = 3)."""
import functools
from dataclasses import replace

import numpy as np
import pytest
import torch

from oracle import elbo_oracle as O
from tests import ref_laplace as RL
from tests import ref_nlik as RN
from tests import ref_prior as RP
from tests import ref_rw as RR
from tests import util
from tests.test_ref_prior_gpu import make_prior

RTOL_TERM, TOL_IPRED, TOL_GRAD = 1e-10, dict(rtol=1e-9, atol=1e-12), dict(rtol=1e-8, atol=1e-10)      # tests/test_golden.py
POSTERIORS = ("truncated_normal", "rice_woolfson")
MODES = {"sum": None, "kl_weight": 0.5}


@functools.lru_cache(maxsize=None)
def problem(laue, kl_weight, posterior):
    """(data with observations on both sides of the predictions, baseline cfg, params, x, the posterior's noise, eta), shared: left unchanged."""
    data, cfg, params, x, u_f, eta = util.make_problem(laue=laue, kl_weight=kl_weight)
    data, _ = RL.rewrite_observations(data, cfg, params, [(u_f, eta)])
    if posterior == "rice_woolfson":
        loc, scale = (t.numpy() for t in O.tn_loc_scale(params.q_loc_raw, params.q_scale_raw, cfg.epsilon))
        u_f = RR.noise_for(loc, scale, data["centric"], cfg.mc_samples, 3)
    return data, replace(cfg, posterior=posterior), params, O.inputs_from_numpy(data), O.f64(u_f), O.f64(eta)


# ---- the corrections: (d nll, d kl) from a forward pass `out` of the baseline on the parameters `q` ----------------------------------------
def likelihood_trade(family_lp):
    def trade(out, q, x, cfg, kl_mask):
        ipl = out["ipred_l"]
        S, N = ipl.shape
        w = 1.0 / S if cfg.kl_weight is None else 1.0 / (S * N)
        return w * (O.normal_log_prob(ipl, x.iobs[None, :], x.sigiobs[None, :]) - family_lp(ipl, q, x)).sum(), 0.0
    return trade


laplace_trade = likelihood_trade(lambda ipl, q, x: O.laplace_log_prob(ipl, x.iobs[None, :], x.sigiobs[None, :]))
neural_trade = likelihood_trade(lambda ipl, q, x: O.normal_log_prob(ipl, x.iobs[None, :], O.nlik_forward(q.nlik, x.iobs, x.sigiobs)[1][None, :]))


def prior_trade(ref):
    def trade(out, q, x, cfg, kl_mask):
        z = out["z_f"]
        swap = O.wilson_log_prob(z, x.centric, x.multiplicity, x.sigma) - O.ref_log_prob(ref.kind, z, *ref[1:])
        if kl_mask is not None:
            swap = swap[:, kl_mask]
        w = 1.0 / z.shape[0] if cfg.kl_weight is None else 1.0 / (z.shape[0] * swap.shape[1])      # (the oracle's mean runs over the KL's columns)
        return 0.0, w * swap.sum()
    return trade


def traded_step(params, x, cfg, u_f, eta, trades, kl_mask):
    """The baseline step under `cfg` with every correction of `trades` added on its own graph: (loss terms, gradients by autograd)."""
    q = params.clone(requires_grad=True)
    out = O.elbo_forward(q, x, cfg, u_f, eta, kl_mask)
    nll, kl = out["nll"], out["kl"]
    for trade in trades:
        d_nll, d_kl = trade(out, q, x, cfg, kl_mask)
        nll, kl = nll + d_nll, kl + d_kl
    loss = nll + (1.0 if cfg.kl_weight is None else cfg.kl_weight) * kl
    ts = q.tensors()
    grads = torch.autograd.grad(loss, ts, allow_unused=True)
    return dict(loss=loss, nll=nll, kl=kl), [torch.zeros_like(t) if g is None else g for g, t in zip(grads, ts)]


def assert_family_is_the_traded_baseline(params, x, base_cfg, family_x, family_cfg, u_f, eta, trades, kl_mask=None):
    out, grads = O.elbo_value_and_grads(params, family_x, family_cfg, u_f, eta, kl_mask)
    base, _ = O.elbo_value_and_grads(params, x, base_cfg, u_f, eta, kl_mask)
    want, want_grads = traded_step(params, x, base_cfg, u_f, eta, trades, kl_mask)
    # the corrections, evaluated on the family step's OWN ipred_l / z_f, are the difference of the two steps' terms
    d_nll, d_kl = (sum(t) for t in zip(*(trade(out, params, x, base_cfg, kl_mask) for trade in trades)))
    klw = 1.0 if base_cfg.kl_weight is None else base_cfg.kl_weight
    for k, d in (("nll", d_nll), ("kl", d_kl), ("loss", d_nll + klw * d_kl)):
        print(f"{k}: family {float(out[k]):.16g} = baseline {float(base[k]):.16g} + correction {float(d):.16g}, off by {float(out[k]) - float(base[k]) - float(d):.1e}")
        assert np.isclose(float(out[k]), float(base[k]) + float(d), rtol=RTOL_TERM, atol=0.0), k
        assert np.isclose(float(out[k]), float(want[k].detach()), rtol=RTOL_TERM, atol=0.0), k
    assert abs(float(d_nll)) + abs(float(d_kl)) > 0.0                                # (the family is not the baseline)
    for k in ("ipred", "ipred_l", "z_f"):
        assert np.allclose(out[k].numpy(), base[k].numpy(), **TOL_IPRED), k
    assert len(grads) == len(want_grads) == len(params.tensors())
    for i, (g, wg) in enumerate(zip(grads, want_grads)):
        assert torch.isfinite(g).all(), i
        assert np.allclose(g.numpy(), wg.numpy(), **TOL_GRAD), i
    return out, grads


# ---- one family at a time, under either posterior ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("posterior", POSTERIORS)
@pytest.mark.parametrize("laue", [False, True], ids=["mono", "laue"])
@pytest.mark.parametrize("mode", MODES)
def test_laplace_step_is_the_normal_step_with_the_likelihood_term_traded(mode, laue, posterior):
    data, cfg, params, x, u_f, eta = problem(laue, MODES[mode], posterior)
    out, _ = assert_family_is_the_traded_baseline(params, x, cfg, x, RL.under(cfg), u_f, eta, [laplace_trade])
    if posterior == "truncated_normal":              # (the observations were rewritten under this posterior's predictions: both signs of the residual occur)
        RL.assert_conditions(data, out["ipred"].numpy(), out["ipred_l"].numpy())


@pytest.mark.parametrize("posterior", POSTERIORS)
@pytest.mark.parametrize("mode", MODES)
def test_neural_step_is_the_normal_step_with_sigiobs_traded_for_sigpred(mode, posterior):
    data, cfg, params, x, u_f, eta = problem(False, MODES[mode], posterior)
    net, _ = RN.pick_net(2, 8, x.iobs, x.sigiobs, first_seed=7)
    out, grads = assert_family_is_the_traded_baseline(RN.with_net(params, net), x, cfg, x, RN.under(cfg), u_f, eta, [neural_trade])
    assert out["kink"] > RN.KINK_REL and torch.equal(out["sigpred"], O.nlik_forward(net, x.iobs, x.sigiobs)[1])
    assert len(grads) == len(params.tensors()) + len(net) and all(float(g.abs().max()) > 0.0 for g in grads[-len(net):])      # the network's gradients, behind the model's


@pytest.mark.parametrize("posterior", POSTERIORS)
@pytest.mark.parametrize("kind", RP.KINDS)
@pytest.mark.parametrize("mode", ["sum", "kl_weight", "sum_kl_mask", "kl_weight_kl_mask"])
def test_reference_prior_step_is_the_wilson_step_with_the_prior_term_traded(mode, kind, posterior):
    data, cfg, params, x, u_f, eta = problem(False, MODES[mode.replace("_kl_mask", "")], posterior)
    prior = make_prior(kind, data, params, masked=True)
    kl_mask = None
    if mode.endswith("kl_mask"):
        kl_mask = torch.zeros(len(x.centric), dtype=torch.bool)
        kl_mask[7:29] = True
    fx, fcfg = RP.under(x, cfg, prior)
    assert_family_is_the_traded_baseline(params, x, cfg, fx, fcfg, u_f, eta, [prior_trade(fx.ref)], kl_mask)


# ---- the three choices together: no reference could state this step before ---------------------------------------------------------------------
@pytest.mark.parametrize("laue", [False, True], ids=["mono", "laue"])
@pytest.mark.parametrize("mode", MODES)
def test_laplace_under_a_reference_prior_and_the_rice_woolfson_posterior(mode, laue):
    data, cfg, params, x, u_f, eta = problem(laue, MODES[mode], "rice_woolfson")
    fx, fcfg = RP.under(x, RL.under(cfg), make_prior("rice_woolfson", data, params, masked=True))
    assert (fcfg.likelihood, fcfg.prior, fcfg.posterior) == ("laplace", "reference", "rice_woolfson")
    assert_family_is_the_traded_baseline(params, x, cfg, fx, fcfg, u_f, eta, [laplace_trade, prior_trade(fx.ref)])


@pytest.mark.parametrize("column", ["iobs", "sigiobs", "metadata"])
def test_a_non_finite_observation_reaches_the_laplace_gradients_as_it_reaches_the_normal_ones(column):
    """The non-finite step contract (tests/test_nonfinite.py) is stated on which gradient entries a poisoned row makes non-finite.  The Laplace
    term's derivative holds the residual only through sign(): the oracle's `laplace_log_prob` keeps a NaN residual NaN there, so the masks
    are the Normal step's (torch.abs alone would leave every gradient finite under a NaN observation)."""
    data, cfg, params, x, u_f, eta = problem(False, None, "truncated_normal")
    bad = x.metadata.clone() if column == "metadata" else getattr(x, column).clone()
    if column == "metadata":
        bad[11, 2] = float("nan")
    else:
        bad[11] = float("nan")
    xp = replace(x, **{column: bad})
    (on, gn), (ol, gl) = (O.elbo_value_and_grads(params, xp, c, u_f, eta) for c in (cfg, RL.under(cfg)))
    assert not np.isfinite(float(ol["nll"])) and np.isfinite(float(ol["kl"]))
    assert not all(torch.isfinite(g).all() for g in gl[:2])
    for i, (a, b) in enumerate(zip(gn, gl)):
        assert torch.equal(torch.isfinite(a), torch.isfinite(b)), i
