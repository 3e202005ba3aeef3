"""The scale prior on the engine ("Σ KLDiv": reference careless/models/merging/variational.py:156-163), GPU part: whole engine steps on
injected noise against the fp64 reference of tests/ref_scale_prior.py, at the project's tolerances (tests/test_gpu_parity.py: RTOL_LOSS,
RTOL_GRAD on every tensor with its LeakyReLU branch gate); Σ KLDiv itself within RTOL_LOSS relative to max(|value|, 1).  The shapes are the
smallest that reach each code path; keyword dictionaries come from tests/test_nonfinite.py's MATRIX where a row fits."""
import itertools

import numpy as np
import pytest
import torch

from careless_amd import _lib
from careless_amd.models.priors.scale import LaplaceScalePrior, NormalScalePrior, StudentTScalePrior
from careless_amd.plan import Route
from oracle import elbo_oracle as O
from tests import ref_nlik as RN
from tests import ref_scale_prior as RS
from tests import test_gpu_parity as P
from tests import test_nonfinite as NF
from tests import util

pytestmark = pytest.mark.gpu

KEY = "Σ KLDiv"


def plugin(prior):
    """The plugin object of a reference prior tuple."""
    return {"normal": NormalScalePrior, "laplace": LaplaceScalePrior, "studentt": StudentTScalePrior}[prior[0]](*prior[1:])


def laplace_location(params, x, cfg, eta, scale):
    """A location for the Laplace prior at which no sample of the reference lies within 1e-3 scale of the kink: the middle of the widest
    gap between neighbouring samples of the central half of the reference's z_scale.  Chosen from the reference alone."""
    z = RS.scale_kl(params, x, cfg, O.f64(eta), ("laplace", 0.0, scale))["z"]
    zs = np.sort(z.numpy().reshape(-1))
    mid = zs[len(zs) // 4: 3 * len(zs) // 4]
    k = int(np.argmax(np.diff(mid)))
    return float(np.float32(0.5 * (mid[k] + mid[k + 1])))


def build(kw, prior, scale_kl_weight=1.0, net=None, **attrs):
    """(model, inputs, problem) of a keyword dictionary of the parity tests with a scale prior; `net`: a neural likelihood's network."""
    kw = dict(kw)
    opts = {k: kw.pop(k, None) for k in ("two_pass", "regroup", "shuffle_rows", "grid")}
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    model = util.build_model(data, cfg, params, kw["L"], kw["w"])
    model.laue_two_pass, model.kernel_grid = bool(opts["two_pass"]), opts["grid"]
    if net is not None:
        from careless_amd.models.likelihoods import NeuralNormalLikelihood
        lik = NeuralNormalLikelihood(len(net) // 2 - 1, net[0].shape[1])
        lik.set_weights([t.numpy() for t in net])
        model.likelihood = lik
        params, cfg = RN.with_net(params, net), RN.under(cfg)
    if isinstance(prior, float):                # the Laplace prior's scale: its location comes from the reference
        prior = ("laplace", laplace_location(params, x, cfg, eta, prior), prior)
    model.scale_prior, model.scale_kl_weight = plugin(prior), scale_kl_weight
    for k, v in attrs.items():
        setattr(model, k, v)
    return model, util.reference_inputs(data), (data, cfg, params, x, u_f, eta, prior)


def assert_terms(terms, out, name):
    for k, rk in (("nll", "nll"), ("kl", "kl"), ("scale_kl", "scale_kl"), ("loss", "loss")):
        ref = float(out[rk])
        den = abs(ref) if k in ("nll", "loss") else max(abs(ref), 1.0)
        print(f"{name}: {k} engine {terms[k]:.9g} reference {ref:.9g}")
        assert abs(terms[k] - ref) <= P.RTOL_LOSS * den, (name, k, terms, ref)


def assert_grads(g_hip, grads, prob, name):
    """tests/test_gpu_parity.py's gate with the reference of this file behind it: every tensor at RTOL_GRAD; a LeakyReLU pre-activation of
    the scaler within fp32 rounding of zero may sit on the engine's branch."""
    data, cfg, params, x, u_f, eta, prior = prob
    assert len(g_hip) == len(grads) and [a.shape for a in g_hip] == [tuple(b.shape) for b in grads]
    errs = [util.rel_err(a, b.numpy()) for a, b in zip(g_hip, grads)]
    print(f"{name}: gradient errors {['%.1e' % e for e in errs]}")
    if max(errs) < P.RTOL_GRAD:
        return
    near = []
    RS.value_and_grads(params, x, cfg, O.f64(u_f), O.f64(eta), prior, near=near)
    near.sort()
    cand = [(l, r, u) for _, l, r, u in near[:P.MAX_FLIP_CANDIDATES]]
    assert cand, f"{name}: gradient errors {errs} and no LeakyReLU pre-activation within fp32 rounding of zero: not a branch flip"
    for k in range(1, len(cand) + 1):
        for sub in itertools.combinations(cand, k):
            _, gf = RS.value_and_grads(params, x, cfg, O.f64(u_f), O.f64(eta), prior, flips=sub)
            if max(util.rel_err(a, b.numpy()) for a, b in zip(g_hip, gf)) < P.RTOL_GRAD:
                print(f"{name}: gradients match with the LeakyReLU unit(s) {list(sub)} on the engine's branch")
                return
    raise AssertionError(f"{name}: gradient errors {errs}; no forced-branch assignment of {cand} brings them under {P.RTOL_GRAD}")


def step(model, inputs, prob, name):
    """One forward + backward on injected noise against the reference; returns (engine, reference dict)."""
    data, cfg, params, x, u_f, eta, prior = prob
    out, grads = RS.value_and_grads(params, x, cfg, O.f64(u_f), O.f64(eta), prior)
    if prior[0] == "laplace":                   # a condition of the case: no sample at the kink of the prior's density
        assert float((out["z_scale"] - prior[1]).abs().min()) > 1e-3 * prior[2]
    ipred = model(inputs, u_f=u_f, eta=eta)
    eng = model._engine
    torch.cuda.synchronize()
    assert util.rel_err(ipred.cpu().numpy(), out["ipred"].numpy()) < 1e-4
    assert_terms(eng.loss_terms(), out, name)
    assert_grads([g.cpu().numpy() for g in eng.grad_tensors()], grads, prob, name)
    return eng, out


CASES = {
    # (keywords, prior, analytic form?)   -- a Laplace prior is given by its scale: `laplace_location` picks the location
    "a_2x32_bare_normal_analytic": (dict(N=300, R=40, d0=5, L=2, w=32, S=2, use_image_scales=False), ("normal", 0.8, 0.6), True),
    "b_2x32_shift_image_scales_sample": (dict(N=300, R=40, d0=5, L=2, w=32, S=2, bijector="softplus", shift=3.5), ("normal", 4.0, 1.5), False),
    "c_20x10_laplace_S1": (NF.MATRIX["lane_20x10_d5_S1"].kw, 0.5, False),
    "c_10x10_laplace_S1": (NF.MATRIX["lane_per_depth_unit_10x10"].kw, 0.5, False),
    "d_5x64_d21_studentt_S4": (dict(N=600, R=50, d0=5, posenc=True, L=5, w=64, S=4), ("studentt", 3.0, 1.0, 0.7), False),
    "e_2x16_image_layer1_packed": (dict(N=500, R=40, d0=5, L=2, w=16, S=2, n_images=5, image_layers=1), ("studentt", 3.0, 1.0, 0.7), False),
    "e_2x16_image_layer1_packed_analytic": (dict(N=500, R=40, d0=5, L=2, w=16, S=2, n_images=5, image_layers=1), ("normal", 1.0, 0.8), True),
    "f_laue_two_pass_2x32_S3": (NF.MATRIX["laue_two_pass_2x32"].kw, ("studentt", 5.0, 1.0, 0.5), False),
    "f_laue_single_pass_data_take_two_passes": (dict(N=400, R=40, L=2, w=32, S=3, laue=True), ("normal", 1.0, 0.5), False),
    "g_chain_12x32": (dict(N=600, R=40, d0=5, L=12, w=32, S=2), ("normal", 1.0, 0.8), False),
    "g_chain_12x32_noimg_analytic": (dict(N=600, R=40, d0=5, L=12, w=32, S=2, use_image_scales=False), ("normal", 1.0, 0.8), True),
    "h_klweight_4x48": (NF.MATRIX["klweight_4x48"].kw, ("studentt", 4.0, 1.0, 0.5), False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_whole_step_matches_the_fp64_reference(name):
    kw, prior, analytic = CASES[name]
    model, inputs, prob = build(kw, prior)
    data, cfg, params, x, u_f, eta, prior = prob
    assert RS.is_analytic(prior, cfg) == analytic
    eng, out = step(model, inputs, prob, name)
    assert eng.sprior_buf.form == (_lib.CL_SPRIOR_ANALYTIC if analytic else _lib.CL_SPRIOR_SAMPLE)
    assert kw["L"] == len(params.mlp_w) - 1 and eng.d == np.asarray(data["metadata"]).shape[1]
    if name.startswith("d_"):
        assert eng.d == 21
    piece = eng.obs
    assert eng._route(piece, None, eng.wide) is (Route.CHAIN if name.startswith("g_") else Route.TWO_PASS)
    assert (eng.blocks is not None) == name.startswith("g_") and not eng.chain_lane and not eng.wide
    if kw.get("laue"):
        assert not eng.obs.fused_laue and eng.two_pass
    if name.startswith("e_"):
        assert eng.imgl is not None and eng.obs.row_map is not None and getattr(eng.obs, "slot_rows", None) is not None
    # the term matters, and with weight 1 and the mean whatever kl_weight is
    plain = O.elbo_forward(params, x, cfg, O.f64(u_f), O.f64(eta))
    assert abs(float(out["scale_kl"])) > 1e-3 and float(out["loss"]) == float(plain["loss"]) + float(out["scale_kl"])
    if cfg.kl_weight is not None:
        t = eng.loss_terms()
        assert abs(t["loss"] - (t["nll"] + cfg.kl_weight * t["kl"] + t["scale_kl"])) <= 1e-12 * abs(t["loss"])
        mean = RS.scale_kl(params, x, cfg, O.f64(eta), prior)["kl_div"].mean()
        assert abs(float(mean) - float(out["scale_kl"])) <= 1e-13 * abs(float(mean))


def test_the_value_of_scale_kl_weight_is_not_used():
    kw, prior, _ = CASES["b_2x32_shift_image_scales_sample"]
    got = []
    for weight in (1.0, 0.0, 37.5):
        model, inputs, prob = build(kw, prior, scale_kl_weight=weight)
        data, cfg, params, x, u_f, eta, _ = prob
        model(inputs, u_f=u_f, eta=eta)
        torch.cuda.synchronize()
        got.append((model._engine.scale_kl_value(), model._engine.grads.clone()))
    assert got[0][0] == got[1][0] == got[2][0] != 0.0
    for other in got[1:]:           # (the data term's float atomics: the summation order alone differs between two runs)
        assert util.rel_err(other[1].cpu().numpy(), got[0][1].cpu().numpy()) < 2e-5
    model, inputs, _ = build(kw, prior, scale_kl_weight=None)
    with pytest.raises(TypeError, match=r"variational\.py:160-161"):
        model.engine(inputs)


def test_refused_at_construction():
    from careless_amd.engine import ElboEngine, make_shard
    model, inputs, _ = build(dict(N=300, R=40, d0=5, L=2, w=96, S=2), ("normal", 1.0, 1.0))
    with pytest.raises(NotImplementedError, match="layer-by-layer"):
        model.engine(inputs)
    model, inputs, _ = build(dict(N=300, R=40, d0=5, L=2, w=32, S=2), ("normal", 1.0, 1.0), owner_shard=True)
    with pytest.raises(NotImplementedError, match="reflection-owner"):
        ElboEngine(model, inputs, shard=make_shard(300, 40, 0, 2))

    class Exponential:
        pass
    model.scale_prior = Exponential()
    with pytest.raises(NotImplementedError, match="NormalScalePrior"):
        model.engine(inputs)


def test_neural_likelihood_beside_a_scale_prior():
    kw = dict(N=300, R=40, d0=5, L=2, w=32, S=2)
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    net, _ = RN.pick_net(2, 16, data["iobs"], data["sigiobs"], first_seed=7)
    net = [O.f64(t.to(torch.float32)) for t in net]
    model, inputs, prob = build(kw, ("studentt", 4.0, 1.0, 0.5), net=net)
    eng, out = step(model, inputs, prob, "i_neural_2x16")
    assert eng.neural and out["kink"] > RN.KINK_REL
    g = [t.cpu().numpy() for t in eng.grad_tensors()]
    assert all(float(np.abs(t).max()) > 0.0 for t in g[-len(net):])


def test_in_kernel_noise_is_the_data_terms_draw():
    """Production mode: the engine's step equals the reference fed with `debug_noise`'s draws for the same seed and step; and two fresh
    engines agree on the value bit for bit."""
    from careless_amd.engine import ElboEngine, debug_noise
    kw = dict(N=300, R=40, d0=5, L=2, w=32, S=3)
    prior = ("studentt", 3.0, 1.0, 0.6)
    model, inputs, prob = build(kw, prior)
    data, cfg, params, x, _, _, _ = prob
    model.seed = 4321
    model(inputs)
    eng = model._engine
    torch.cuda.synchronize()
    u = debug_noise(4321, 0, 3, 40, 0, kind=0).t().cpu().numpy()
    e = debug_noise(4321, 0, 3, 300, 0, kind=1).t().cpu().numpy()
    out, grads = RS.value_and_grads(params, x, cfg, O.f64(u), O.f64(e), prior)
    assert_terms(eng.loss_terms(), out, "philox")
    assert_grads([g.cpu().numpy() for g in eng.grad_tensors()], grads, (data, cfg, params, x, u, e, prior), "philox")
    other = ElboEngine(build(kw, prior)[0], inputs, seed=4321)
    other.forward_backward(0)
    torch.cuda.synchronize()
    assert other.scale_kl_value() == eng.scale_kl_value()
    # another step draws other noise
    other.forward_backward(1)
    torch.cuda.synchronize()
    assert other.scale_kl_value() != eng.scale_kl_value()


@pytest.mark.parametrize("kw,prior", [(dict(N=517, R=41, d0=5, L=2, w=32, S=3), ("studentt", 3.0, 1.0, 0.6)),
                                      (dict(N=600, R=50, L=2, w=32, S=2, laue=True), ("normal", 1.0, 0.5))], ids=["mono", "laue"])
def test_two_row_split_shards_sum_to_the_one_rank_step(kw, prior):
    from careless_amd.engine import ElboEngine, make_shard
    model, inputs, prob = build(kw, prior)
    data = prob[0]
    if kw.get("laue"):                                  # rows of a harmonic group are not contiguous in real inputs
        perm = np.random.default_rng(1).permutation(kw["N"])
        for k in ("refl_id", "image_id", "file_id", "metadata", "wavelength", "harmonic_id"):
            data[k] = np.asarray(data[k])[perm]
        inputs = util.reference_inputs(data)
    full = ElboEngine(model, inputs, seed=99)
    full.forward_backward(3)
    torch.cuda.synchronize()
    g_full, t_full = full.grads.clone(), full.loss_terms()
    g_sum, tot = torch.zeros_like(g_full), dict(nll=0.0, kl=0.0, scale_kl=0.0)
    for r in range(2):
        eng = ElboEngine(build(kw, prior)[0], inputs, seed=99, shard=make_shard(kw["N"], kw["R"], r, 2))
        assert not eng.owner
        eng.local_only = True
        eng.forward_backward(3)
        torch.cuda.synchronize()
        g_sum += eng.grads
        t = eng.loss_terms()
        for k in tot:
            tot[k] += t[k]
        assert 0.0 < abs(t["scale_kl"]) < abs(t_full["scale_kl"])
    for k in tot:
        print(f"shards {k}: {tot[k]:.9g} one rank {t_full[k]:.9g}")
        assert abs(tot[k] - t_full[k]) <= 1e-5 * max(abs(t_full[k]), 1.0 if k != "nll" else 0.0)
    assert util.rel_err(g_sum.cpu().numpy(), g_full.cpu().numpy()) < 2e-5


def test_shard_cut_into_three_launches_equals_the_uncut_step(monkeypatch):
    from careless_amd.engine import ElboEngine, ObsChunks
    kw, prior = dict(N=900, R=50, d0=5, L=2, w=32, S=2), ("studentt", 3.0, 1.0, 0.6)
    monkeypatch.setenv("CARELESS_HIP_MAX_LAUNCH_BYTES", str(4 * 8 * 384))           # 384 rows of 5 -> 8 columns per launch: 384 + 384 + 132
    model, inputs, prob = build(kw, prior)
    eng, out = step(model, inputs, prob, "three launches")               # injected noise: every piece reads its own rows of eta
    assert isinstance(eng.obs, ObsChunks) and len(eng.obs.children) == 3
    cut = ElboEngine(build(kw, prior)[0], inputs, seed=31)
    cut.forward_backward(2)
    monkeypatch.delenv("CARELESS_HIP_MAX_LAUNCH_BYTES")
    one = ElboEngine(build(kw, prior)[0], inputs, seed=31)
    assert not isinstance(one.obs, ObsChunks)
    one.forward_backward(2)
    torch.cuda.synchronize()
    ta, tb = cut.loss_terms(), one.loss_terms()
    assert abs(ta["nll"] - tb["nll"]) <= 1e-6 * abs(tb["nll"]) and ta["kl"] == tb["kl"]
    assert abs(ta["scale_kl"] - tb["scale_kl"]) <= 1e-12 * abs(tb["scale_kl"])          # (fp64 partials: the summation order alone differs)
    assert util.rel_err(cut.grads.cpu().numpy(), one.grads.cpu().numpy()) < 2e-5


@pytest.mark.parametrize("kw,prior,pieces", [(dict(N=500, R=40, d0=5, L=2, w=32, S=2), ("studentt", 3.0, 1.0, 0.6), 1),
                                             (dict(N=500, R=40, d0=5, L=5, w=64, S=4, use_image_scales=False), ("normal", 1.0, 0.8), 1),
                                             (dict(N=900, R=50, d0=5, L=2, w=32, S=2), ("studentt", 3.0, 1.0, 0.6), 3),
                                             (dict(N=600, R=40, d0=5, L=12, w=32, S=2), ("normal", 1.0, 0.8), 1)],
                         ids=["image_scales_sample", "5x64_analytic", "three_launches", "chain_12x32"])
def test_deterministic_mode_matches_the_reference_and_repeats_bit_for_bit(kw, prior, pieces, monkeypatch):
    from careless_amd.engine import ObsChunks
    if pieces > 1:
        monkeypatch.setenv("CARELESS_HIP_MAX_LAUNCH_BYTES", str(4 * 8 * 384))
    runs = []
    for _ in range(2):
        model, inputs, prob = build(kw, prior, deterministic=True)
        data, cfg, params, x, u_f, eta, _ = prob
        eng, out = step(model, inputs, prob, "deterministic")
        assert eng.deterministic and (len(eng.obs.children) if isinstance(eng.obs, ObsChunks) else 1) == pieces
        g = eng.grads.clone()
        model.train_model(inputs, 3, progress=False, noise=lambda i: (u_f, eta))
        runs.append((g, eng.scale_kl_value(), eng.params.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] and torch.equal(runs[0][2], runs[1][2])


def test_deterministic_mode_refusals_stay():
    model, inputs, _ = build(dict(N=400, R=40, L=2, w=32, S=2, laue=True), ("normal", 1.0, 0.5), deterministic=True)
    with pytest.raises(NotImplementedError):
        model.engine(inputs)
    model, inputs, _ = build(dict(N=300, R=40, d0=5, L=2, w=32, S=3), ("normal", 1.0, 0.5), deterministic=True)
    with pytest.raises(NotImplementedError, match="deterministic mode covers"):
        model.engine(inputs)


def test_frozen_scaler_keeps_the_term_and_masks_the_scaler():
    kw, prior = dict(N=300, R=40, d0=5, L=2, w=32, S=2), ("studentt", 3.0, 1.0, 0.6)
    model, inputs, prob = build(kw, prior)
    data, cfg, params, x, u_f, eta, _ = prob
    model(inputs, u_f=u_f, eta=eta)
    torch.cuda.synchronize()
    free = [g.cpu().numpy() for g in model._engine.grad_tensors()]
    frozen, _, _ = build(kw, prior)
    frozen.scaling_model.trainable = False
    frozen.frozen_scaler_fast_path = True
    eng = frozen.engine(inputs)
    assert eng.scaler_frozen and not eng._frozen_layout and eng._frozen_form(eng.obs) is None          # the fast path is not taken
    assert eng._route(eng.obs, eng._frozen_form(eng.obs), eng.wide) is Route.TWO_PASS
    frozen(inputs, u_f=u_f, eta=eta)
    torch.cuda.synchronize()
    g = [t.cpu().numpy() for t in eng.grad_tensors()]
    for k in (0, 1):
        assert util.rel_err(g[k], free[k]) < 2e-5
    w0 = frozen.scaling_model.mlp_scaler.flat.clone()
    s0 = frozen.scaling_model.image_scaler._scales.clone()
    q0 = frozen.surrogate_posterior.loc_raw.clone()
    hist = frozen.train_model(inputs, 3, progress=False, noise=lambda i: (u_f, eta))
    assert torch.equal(frozen.scaling_model.mlp_scaler.flat, w0) and torch.equal(frozen.scaling_model.image_scaler._scales, s0)
    assert not torch.equal(frozen.surrogate_posterior.loc_raw, q0)
    want = float(RS.scale_kl(params, x, cfg, O.f64(eta), prior)["value"])
    assert len(hist[KEY]) == 3 and all(abs(v - want) <= P.RTOL_LOSS * max(abs(want), 1.0) for v in hist[KEY])


def test_adam_trajectory_of_twenty_steps():
    # (a tight prior: its gradient on a row is of the size of the likelihood's, so the trajectory is the term's as much as the data's)
    kw, prior = dict(N=384, R=48, d0=5, L=2, w=32, S=2), ("normal", 1.0, 0.02)
    model, inputs, prob = build(kw, prior)
    data, cfg, params, x, _, _, _ = prob
    steps = 20
    rng = np.random.default_rng(11)
    noises = [(rng.random((2, 48)).astype(np.float32), rng.normal(size=(2, 384)).astype(np.float32)) for _ in range(steps)]
    hist = model.train_model(inputs, steps, progress=False, noise=lambda i: noises[i])
    p = params.clone()
    st = O.AdamState.zeros_like(p.tensors())
    ref = [RS.train_step(p, x, cfg, st, O.f64(u), O.f64(e), prior) for u, e in noises]
    for k in ("loss", "NLL", "F KLDiv", KEY, "Grad Norm"):
        a, b = np.array(hist[k]), np.array([r[k] for r in ref])
        err = float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)))
        print(f"trajectory {k}: {err:.2e}")
        assert err < 1e-4, (k, a, b)
    eng = model._engine
    got = [t.cpu().numpy() for t in eng.param_tensors()]
    errs = [util.rel_err(a, b.detach().numpy()) for a, b in zip(got, p.tensors())]
    print(f"trajectory parameters: {['%.1e' % e for e in errs]}")
    assert max(errs) < 1e-4, errs
    # the term moved the scaler: the same trajectory without a prior ends elsewhere
    plain = util.build_model(data, cfg, params, 2, 32)
    plain.train_model(inputs, steps, progress=False, noise=lambda i: noises[i])
    assert util.rel_err(plain._engine.param_tensors()[2].cpu().numpy(), got[2]) > 1e-3


def test_nan_metadata_cell_stops_training_with_finite_parameters():
    kw, prior = dict(N=300, R=40, d0=5, L=2, w=32, S=2), ("studentt", 3.0, 1.0, 0.6)
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    model, _, _ = build(kw, prior)
    bad = dict(data)
    bad["metadata"] = np.array(data["metadata"], dtype=np.float32, copy=True)
    bad["metadata"][151, 2] = np.nan
    hist = model.train_model(util.reference_inputs(bad), 4, progress=False)
    assert len(hist["loss"]) == 1 and len(hist[KEY]) == 1 and not np.isfinite(hist["Grad Norm"][0])
    assert not np.isfinite(hist[KEY][0]) and not np.isfinite(hist["loss"][0])          # the NaN reaches the value
    assert all(bool(torch.isfinite(t).all()) for t in model._engine.param_tensors())


def test_train_model_history_has_the_metric_and_the_loss_is_the_sum_of_its_terms():
    for klw in (None, 0.5):
        kw, prior = dict(N=300, R=40, d0=5, L=2, w=32, S=2, kl_weight=klw), ("normal", 4.0, 1.5)
        model, inputs, prob = build(kw, prior)
        hist = model.train_model(inputs, 5, progress=False)
        assert KEY in hist and len(hist[KEY]) == len(hist["loss"]) == 5
        mult = 1.0 if klw is None else klw
        for loss, nll, kl, skl in zip(hist["loss"], hist["NLL"], hist["F KLDiv"], hist[KEY]):
            assert skl != 0.0 and abs(loss - (nll + mult * kl + skl)) <= 1e-14 * abs(loss)
        # without a prior: the history is today's
        plain = util.build_model(prob[0], prob[1], prob[2], 2, 32)
        h0 = plain.train_model(inputs, 2, progress=False)
        assert KEY not in h0 and set(h0) == {"loss", "F KLDiv", "NLL", "Grad Norm"}
        assert float(plain._engine.history_buf.view(-1, _lib.CL_HIST_STRIDE)[:2, 5:].abs().max()) == 0.0
