"""The Laplace likelihood on the GPU: whole training steps of the engine against the fp64 oracle under its Laplace likelihood
(`ElboConfig.likelihood = "laplace"`), deterministic mode, the frozen scaler, row-split and reflection-owner
shards, NLL_val, an Adam trajectory, the non-finite step contract and the slot kernels' Laplace instances called directly.

The cases are the rows of tests/test_nonfinite.py's MATRIX (its keyword dictionaries, routes and kernel-name fragments; the four Ev11 /
double-Wilson rows left out) with `likelihood` / `dof` / `ev11` dropped and `model.likelihood = LaplaceLikelihood()`.  The likelihood kind
does not change the routing, with ONE documented exception: the lane and the narrow kernel have no Laplace instance, so a
shape they would take runs on the instance of csrc/elbo_mlp.hip it ran on before those kernels existed (no peeled first layer, no lane
block at the end of a chain; deterministic per-image layers, a lane-only feature, are refused) -- those rows assert that fallback, every
other row its own route, kernel-name fragment, layout and, 64 wide, the generic epilogue.  Observations are rewritten by
`ref_laplace.rewrite_observations`, so that both signs of the residual occur and no sample sits within the guard of the kink; every test
on injected noise asserts that on the reference, and that the engine's predictions are within 1e-4 of the reference's in max-norm -- then
no sample is on the other side of its observation.

Tolerances are the project's own: `RTOL_LOSS` / `RTOL_GRAD` of tests/test_gpu_parity.py with its LeakyReLU branch gate."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from careless_amd import _lib
from oracle import elbo_oracle as O
from tests import ref_laplace as RL
from tests import test_gpu_parity as P
from tests import test_nonfinite as NF
from tests import util

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

EXCLUDED = ("double_wilson_2x32", "double_wilson_trainable_r", "ev11_normal_2x32", "ev11_studentt_5x64_S8")
STEP_ROWS = [n for n in NF.MATRIX if n not in EXCLUDED]
NONFINITE_ROWS = [n for n in NF.MATRIX if NF.MATRIX[n].primary] + ["mlp_packed_laue_single_pass_2x32", "laue_two_pass_2x32", "wide_3x96", "frozen_mono_20x10"]
NONFINITE_POISONS = ("iobs_nan", "sigiobs_nan", "metadata_nan")
# The seed of the standard normals of `rewrite_observations` is the row's own, except where the two NLLs of the REFERENCE would come out
# within 1 % of each other: at Iobs = m + 1.5 sigma n the expectations of the Normal and of the Laplace term nearly agree (2.04 each), so for
# S = 1 the relative difference is a zero-mean sum over the N rows -- 0.3 % on the 3000 rows of this case at its own seed, -2.0 % at seed 2.
REWRITE_SEED = {"lane_image_layers1_20x10": 2}


# ---- the problem of a matrix row under the Laplace likelihood ----------------------------------------------------------------------------------
def problem(name, poison=None, where="inner"):
    """tests/test_nonfinite.py's `_problem` with the likelihood keys dropped and the observations rewritten BEFORE the poison goes in.
    Returns (case, kw, opts, clean data, data, cfg, params, u_f, eta)."""
    case = NF.MATRIX[name] if isinstance(name, str) else name
    kw = dict(case.kw, seed=case.seed)
    for k in ("likelihood", "dof", "ev11"):
        kw.pop(k, None)
    opts = {k: kw.pop(k, None) for k in ("two_pass", "regroup", "shuffle_rows", "grid")}
    assert not opts["shuffle_rows"]
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    if opts["regroup"]:
        data = P._regroup_laue(data, opts["regroup"])
    clean, _ = RL.rewrite_observations(data, cfg, params, [(u_f, eta)], seed=REWRITE_SEED.get(name if isinstance(name, str) else None, case.seed))
    data = dict(clean)
    if poison is not None:
        row = NF._pick_row(data, where)
        column, value = NF.POISONS[poison]
        a = np.array(data[column], dtype=np.float32, copy=True)
        if column == "metadata":
            a[row, row % a.shape[1]] = value
        else:
            a[NF._groups(data)[row]] = value
        data[column] = a
    return case, kw, opts, clean, data, cfg, params, u_f, eta


def laplace_model(case, kw, opts, data, cfg, params, **attrs):
    from careless_amd.models.likelihoods import laue as laue_lik, mono as mono_lik
    model = NF._model(case, kw, opts, data, cfg, params)
    model.likelihood = (laue_lik if cfg.laue else mono_lik).LaplaceLikelihood()
    for k, v in attrs.items():
        setattr(model, k, v)
    return model


def plan_of(case, kw, opts, data, cfg):
    from careless_amd.engine import plan_scaler
    gmax = int(np.bincount(np.asarray(data["harmonic_id"])).max()) if cfg.laue else 1
    return plan_scaler(_lib.get_lib(), np.asarray(data["metadata"]).shape[1], kw["w"], kw["L"], cfg.image_layers, laue=cfg.laue,
                       two_pass=bool(opts["two_pass"]), gmax=gmax, ev11=False, deterministic=case.det, lik_kind=_lib.CL_LIK_LAPLACE)


LANE_FAMILY = ("LANE", "LANE_IMGL", "NARROW")          # the kernels without a Laplace instance


def falls_back(case):
    return case.route in LANE_FAMILY or "LANE_BLOCK" in case.block_routes


def assert_route(eng, case, plan):
    """tests/test_nonfinite.py's `_assert_route` under the Laplace likelihood: the row's own route, fragment and layout -- or, for a row of
    the lane / narrow kernel, the documented fallback onto elbo_mlp.hip."""
    assert eng.lik_kind == _lib.CL_LIK_LAPLACE and eng.dof == 0.0 and eng.lik_const == 0.0
    off_limits = {NF._route(r) for r in LANE_FAMILY}
    assert eng.plan == plan and plan.route not in off_limits and not plan.chain_lane, (eng.plan, plan)
    assert bool(eng.deterministic) == case.det
    if falls_back(case):
        assert not eng.wide and not eng.peel and plan.route != _lib.CL_ROUTE_NONE
        assert (eng.blocks is None) == (case.blocks is None)
    else:
        assert plan.route == NF._route(case.route)
        assert (bool(eng.peel), bool(eng.wide), None if eng.blocks is None else len(eng.blocks)) == (case.peel, case.wide, case.blocks)
    if case.frozen:
        assert eng.scaler_frozen and eng._frozen_layout and eng.frozen_fast
        return
    name = eng.kernel_name()
    assert ("elbo_mlp_kernel<" in name and "lane" not in name and "narrow" not in name) if falls_back(case) else (case.frag in name), name
    if not eng.wide:
        ma, mode = eng.training_launch()
        assert ma.lik_kind == _lib.CL_LIK_LAPLACE
        assert eng.lib.cl_mlp_route(C.byref(ma), mode) == plan.route
        if "elbo_mlp_kernel<64, " in name:
            assert eng.lib.cl_mlp_epilogue(C.byref(ma), mode) == _lib.CL_EPI_GENERIC
        if case.blocks and not falls_back(case):
            obs = eng.obs.children[0] if hasattr(eng.obs, "children") else eng.obs
            assert NF._block_routes(plan, (eng, eng._mlp_args(0, None, None, obs), obs)) == {NF._route(r) for r in case.block_routes}
    if case.single_pass is not None:
        assert bool(eng.obs.fused_laue) == case.single_pass


def det_offered(case, cfg):
    """Deterministic mode with per-image layers exists on the lane kernel's instances only (include/careless_hip.h: dzf_obs); the lane kernel
    has no Laplace instance, so the engine refuses that combination by name.  Everything else is offered as for the other likelihoods."""
    return not (case.det and cfg.image_layers)


def assert_terms(terms, out, name):
    for k in ("nll", "kl", "loss"):
        den = max(abs(float(out[k])), 1.0) if k == "kl" else abs(float(out[k]))
        print(f"{name}: {k} engine {terms[k]:.9g} reference {float(out[k]):.9g}")
        assert abs(terms[k] - float(out[k])) <= P.RTOL_LOSS * den, (name, k, terms, float(out[k]))


def assert_grads(g_hip, grads, prob, name):
    """tests/test_gpu_parity.py's gate (every tensor at RTOL_GRAD; a LeakyReLU pre-activation within fp32 rounding of zero may sit on the
    engine's branch), as tests/test_ref_prior_gpu.py rebuilds it, with tests/ref_laplace.py behind it.  Compares the leading len(g_hip) tensors."""
    n = len(g_hip)
    errs = [util.rel_err(a, b.numpy()) for a, b in zip(g_hip, grads[:n])]
    print(f"{name}: gradient errors {['%.1e' % e for e in errs]}")
    if max(errs) < P.RTOL_GRAD:
        return
    data, cfg, params, u_f, eta = prob
    x = O.inputs_from_numpy(data)
    near = []
    O.elbo_value_and_grads(params, x, RL.under(cfg), O.f64(u_f), O.f64(eta), near=near)
    near.sort()
    cand = [(l, r, u) for _, l, r, u in near[:P.MAX_FLIP_CANDIDATES]]
    assert cand, f"{name}: gradient errors {errs} and no LeakyReLU pre-activation within fp32 rounding of zero: not a branch flip"
    for k in range(1, len(cand) + 1):
        for sub in itertools.combinations(cand, k):
            _, gf = O.elbo_value_and_grads(params, x, RL.under(cfg), O.f64(u_f), O.f64(eta), flips=sub)
            if max(util.rel_err(a, b.numpy()) for a, b in zip(g_hip, gf[:n])) < P.RTOL_GRAD:
                print(f"{name}: gradients match with the LeakyReLU unit(s) {list(sub)} on the engine's branch")
                return
    raise AssertionError(f"{name}: gradient errors {errs}; no forced-branch assignment of {cand} brings them under {P.RTOL_GRAD}")


# ---- whole steps ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STEP_ROWS)
def test_whole_step_matches_the_fp64_reference(name):
    case, kw, opts, _, data, cfg, params, u_f, eta = problem(name)
    x = O.inputs_from_numpy(data)
    out, grads = O.elbo_value_and_grads(params, x, RL.under(cfg), O.f64(u_f), O.f64(eta))
    gap, pos = RL.assert_conditions(data, out["ipred"].numpy(), out["ipred_l"].numpy())
    print(f"{name}: smallest gap {gap:.2f} guards, {100 * pos:.0f} % positive residuals")
    model = laplace_model(case, kw, opts, data, cfg, params)
    inputs = util.reference_inputs(data)
    if not det_offered(case, cfg):
        with pytest.raises(NotImplementedError, match="deterministic mode"):
            model.engine(inputs)
        return
    eng = model.engine(inputs)
    assert_route(eng, case, plan_of(case, kw, opts, data, cfg))
    ipred = model(inputs, u_f=u_f, eta=eta)
    torch.cuda.synchronize()
    assert util.rel_err(ipred.cpu().numpy(), out["ipred"].numpy()) < 1e-4          # ... so no sample changed sides
    assert_terms(eng.loss_terms(), out, name)
    g_hip = [g.cpu().numpy() for g in eng.grad_tensors()]
    assert len(g_hip) == len(grads)
    if case.frozen:                  # the scaler's gradient is not computed: q's two tensors lead both lists
        g_hip = g_hip[:2]
    assert_grads(g_hip, grads, (data, cfg, params, u_f, eta), name)
    # the likelihood matters: the same step under the Normal likelihood has another NLL
    nll_n = float(O.elbo_value_and_grads(params, x, cfg, O.f64(u_f), O.f64(eta))[0]["nll"])
    assert abs(float(out["nll"]) - nll_n) > 1e-2 * abs(nll_n)


@pytest.mark.parametrize("name", ["det_mlp_5x64", "det_packed_laue_5x64", "det_lane_image_layers2_20x10"])
def test_deterministic_mode_repeats_bit_for_bit(name):
    from careless_amd.engine import ElboEngine
    case, kw, opts, _, data, cfg, params, u_f, eta = problem(name)
    inputs = util.reference_inputs(data)
    if not det_offered(case, cfg):          # (the lane kernel's per-image-layer stores: no Laplace instance)
        with pytest.raises(NotImplementedError, match="deterministic mode"):
            ElboEngine(laplace_model(case, kw, opts, data, cfg, params), inputs, seed=5)
        return
    runs = []
    for _ in range(2):
        e = ElboEngine(laplace_model(case, kw, opts, data, cfg, params), inputs, seed=5)
        assert e.deterministic and e.lik_kind == _lib.CL_LIK_LAPLACE and case.frag in e.kernel_name()
        e.forward_backward(1)
        torch.cuda.synchronize()
        g, terms = e.grads.clone(), e.loss_terms()
        e.alloc_history(4)
        for i in range(4):
            e.train_step(i)
        torch.cuda.synchronize()
        runs.append((g, terms, e.params.clone(), e.read_history(4)))
    (g0, t0, p0, h0), (g1, t1, p1, h1) = runs
    assert torch.equal(g0, g1) and t0 == t1 and torch.equal(p0, p1)
    assert all(h0[k] == h1[k] for k in ("loss", "F KLDiv", "NLL", "Grad Norm"))
    assert np.all(np.isfinite(h0["loss"])) and len(h0["loss"]) == 4 and float(g0.abs().max()) > 0.0


@pytest.mark.parametrize("name", ["frozen_mono_20x10", "frozen_laue_two_call_form_2x32"])
def test_frozen_scaler_step_equals_the_fused_step(name):
    """Fast path on against fast path off, the same in-kernel noise on both engines."""
    from careless_amd.engine import ElboEngine
    case, kw, opts, _, data, cfg, params, u_f, eta = problem(name)
    inputs = util.reference_inputs(data)
    engs = {}
    for fast in (True, False):
        m = laplace_model(case, kw, opts, data, cfg, params, frozen_scaler_fast_path=fast)
        engs[fast] = ElboEngine(m, inputs, seed=31)
        engs[fast].forward_backward(4)
    torch.cuda.synchronize()
    fast, full = engs[True], engs[False]
    assert fast.scaler_frozen and fast._frozen_layout and not full._frozen_layout and fast.lik_kind == full.lik_kind == _lib.CL_LIK_LAPLACE
    assert getattr(fast.obs, "frozen_sorted", None) is not None      # (cl_frozen_rows' Laplace instances)
    tf, tu = fast.loss_terms(), full.loss_terms()
    print("frozen / fused nll", tf["nll"], tu["nll"])
    assert abs(tf["nll"] - tu["nll"]) <= P.RTOL_LOSS * abs(tu["nll"])
    R = fast.R
    gf, gu = fast.grads[: 2 * R].cpu().numpy(), full.grads[: 2 * R].cpu().numpy()
    print("frozen / fused q gradient", util.rel_err(gf[:R], gu[:R]), util.rel_err(gf[R:], gu[R:]))
    assert util.rel_err(gf[:R], gu[:R]) < P.RTOL_GRAD and util.rel_err(gf[R:], gu[R:]) < P.RTOL_GRAD


def _plain_problem(kw, seed=7):
    """A rewritten monochromatic problem off the matrix: (fresh model factory, data, cfg, params, u_f, eta)."""
    from careless_amd.models.likelihoods.mono import LaplaceLikelihood
    data, cfg, params, x, u_f, eta = util.make_problem(seed=seed, **kw)
    data, _ = RL.rewrite_observations(data, cfg, params, [(u_f, eta)], seed=seed)

    def fresh(**attrs):
        m = util.build_model(data, cfg, params, kw["L"], kw["w"])
        m.likelihood = LaplaceLikelihood()
        for k, v in attrs.items():
            setattr(m, k, v)
        return m
    return fresh, data, cfg, params, u_f, eta


@pytest.mark.parametrize("owner", [False, True], ids=["row_split", "owner_split"])
def test_two_shards_sum_to_the_one_rank_step(owner):
    from careless_amd.engine import ElboEngine, make_shard
    kw = dict(N=600, R=50, d0=5, L=2, w=32, S=2)
    fresh, data, cfg, params, _, _ = _plain_problem(kw)
    inputs = util.reference_inputs(data)
    full = ElboEngine(fresh(), inputs, seed=99)
    full.forward_backward(3)
    torch.cuda.synchronize()
    g_full, t_full = full.grads.clone(), full.loss_terms()
    g_sum, nll, kl = torch.zeros_like(g_full), 0.0, 0.0
    for r in range(2):
        eng = ElboEngine(fresh(owner_shard=owner), inputs, seed=99, shard=make_shard(kw["N"], kw["R"], r, 2))
        assert bool(eng.owner) == owner and eng.lik_kind == _lib.CL_LIK_LAPLACE and 0 < eng.shard.kl_end - eng.shard.kl_begin < kw["R"]
        eng.local_only = True
        eng.forward_backward(3)
        torch.cuda.synchronize()
        g_sum += eng.grads
        t = eng.loss_terms()
        nll += t["nll"]; kl += t["kl"]
    assert abs(nll - t_full["nll"]) <= 1e-5 * abs(t_full["nll"]) and abs(kl - t_full["kl"]) <= 1e-5 * max(abs(t_full["kl"]), 1.0)
    assert util.rel_err(g_sum.cpu().numpy(), g_full.cpu().numpy()) < 2e-5


def test_validation_nll_matches_the_reference():
    kw = dict(N=384, R=48, d0=5, L=2, w=32, S=2)
    fresh, data, cfg, params, u_f, eta = _plain_problem(kw)
    inputs = util.reference_inputs(data)
    n_tr = 300
    train, test = tuple(a[:n_tr] for a in inputs), tuple(a[n_tr:] for a in inputs)

    def as_inputs(t):
        d = dict(data)
        d.update(refl_id=t[0][:, 0], image_id=t[1][:, 0], metadata=t[3], iobs=t[4][:, 0], sigiobs=t[5][:, 0])
        return d, O.inputs_from_numpy(d)
    (d_tr, x_tr), (d_te, x_te) = as_inputs(train), as_inputs(test)
    rng = np.random.default_rng(12)
    noise = (u_f, eta[:, :n_tr])                             # the training rows' share of the noise the observations were rewritten under
    vnoise = (rng.random((2, 48)).astype(np.float32), rng.normal(size=(2, kw["N"] - n_tr)).astype(np.float32))
    out, _ = O.elbo_value_and_grads(params, x_tr, RL.under(cfg), *map(O.f64, noise))
    RL.assert_conditions(d_tr, out["ipred"].numpy(), out["ipred_l"].numpy())
    probe = fresh()                                          # the first step's predictions: no sample on the other side of its observation
    assert util.rel_err(probe(train, u_f=noise[0], eta=noise[1]).cpu().numpy(), out["ipred"].numpy()) < 1e-4
    model = fresh()
    hist = model.train_model(train, 1, progress=False, validation_data=test, validation_frequency=1, noise=lambda i: noise,
                             validation_noise=lambda i: vnoise)
    p = params.clone()
    rec = O.train_step(p, x_tr, RL.under(cfg), O.AdamState.zeros_like(p.tensors()), *map(O.f64, noise))
    ref = O.validation_nll(p, x_te, RL.under(cfg), O.f64(vnoise[0]), O.f64(vnoise[1]), n_tr)
    normal = O.validation_nll(p, x_te, cfg, O.f64(vnoise[0]), O.f64(vnoise[1]), n_tr)
    print("NLL_val", hist["NLL_val"], "reference", ref, "under the Normal likelihood", normal)
    assert len(hist["NLL_val"]) == 1 and abs(hist["NLL_val"][0] - ref) <= P.RTOL_LOSS * abs(ref)
    assert abs(hist["NLL"][0] - rec["NLL"]) <= P.RTOL_LOSS * abs(rec["NLL"]) and abs(ref - normal) > 1e-2 * abs(normal)


TRAJECTORY_SEED = 30          # the first seed (from 7 on) of `_trajectory` whose reference trajectory meets both conditions at every step (found on the CPU; asserted below)


def _trajectory(seed, steps=5):
    from careless_amd.models.likelihoods.mono import LaplaceLikelihood
    kw = dict(N=384, R=48, d0=5, L=2, w=32, S=2)
    data, cfg, params, x, _, _ = util.make_problem(seed=seed, **kw)
    rng = np.random.default_rng(11 + seed)
    noises = [(rng.random((2, 48)).astype(np.float32), rng.normal(size=(2, 384)).astype(np.float32)) for _ in range(steps)]
    data, _ = RL.rewrite_observations(data, cfg, params, noises, seed=seed)
    x = O.inputs_from_numpy(data)
    p = params.clone()
    st = O.AdamState.zeros_like(p.tensors())
    ref, worst, first = [], np.inf, None
    for u, e in noises:
        out, _ = O.elbo_value_and_grads(p, x, RL.under(cfg), O.f64(u), O.f64(e))
        first = out if first is None else first
        gap, pos = RL.assert_conditions(data, out["ipred"].numpy(), out["ipred_l"].numpy())
        worst = min(worst, gap)
        ref.append(O.train_step(p, x, RL.under(cfg), st, O.f64(u), O.f64(e)))

    def fresh():
        m = util.build_model(data, cfg, params, kw["L"], kw["w"])
        m.likelihood = LaplaceLikelihood()
        return m
    return fresh, data, noises, ref, p, worst, first["ipred"].numpy()


def test_adam_trajectory_matches_the_reference_loop():
    fresh, data, noises, ref, p, worst, ipred0 = _trajectory(TRAJECTORY_SEED)
    print(f"smallest gap along the reference trajectory: {worst:.2f} guards")
    # the first step's predictions are within 1e-4 of the reference's; the later steps' parameters are held to 2e-4 below, each step's NLL and
    # gradient norm to 2e-4 as it is taken -- a sample that changed sides (one of 768 derivatives flipped) shows in that step's gradient norm
    assert util.rel_err(fresh()(util.reference_inputs(data), u_f=noises[0][0], eta=noises[0][1]).cpu().numpy(), ipred0) < 1e-4
    model = fresh()
    hist = model.train_model(util.reference_inputs(data), len(noises), progress=False, noise=lambda i: noises[i])
    for k in ("loss", "NLL", "F KLDiv", "Grad Norm"):
        a, b = np.array(hist[k]), np.array([r[k] for r in ref])
        assert len(a) == len(noises) and np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)) < 2e-4, (k, a, b)
    got = [t.cpu().numpy() for t in model._engine.param_tensors()]
    for a, b in zip(got, p.tensors()):
        assert util.rel_err(a, b.numpy()) < 2e-4


# ---- the non-finite step contract ----------------------------------------------------------------------------------------------------------
def _reference_of_a_poisoned_step(name, poison):
    case, kw, opts, clean, data, cfg, params, u_f, eta = problem(name, poison, "inner")
    # the clean twin meets the two conditions; the poisoned step's LeakyReLU branches are not in doubt (tests/test_nonfinite.py: `_oracle_grads`)
    co, _ = O.elbo_value_and_grads(params, O.inputs_from_numpy(clean), RL.under(cfg), O.f64(u_f), O.f64(eta))
    RL.assert_conditions(clean, co["ipred"].numpy(), co["ipred_l"].numpy())
    near = []
    out, grads = O.elbo_value_and_grads(params, O.inputs_from_numpy(data), RL.under(cfg), O.f64(u_f), O.f64(eta), near=near)
    near = [t for t in near if np.isfinite(t[0])]
    assert not near, sorted(near)[:5]
    assert float(out["z_f"].min()) >= 1e-2
    return case, kw, opts, data, cfg, params, u_f, eta, out, [g.numpy() for g in grads]


NONFINITE_PARAMS = [(n, p) for n in NONFINITE_ROWS for p in NONFINITE_POISONS]


@pytest.mark.parametrize("name,poison", NONFINITE_PARAMS, ids=[f"{n}-{p}" for n, p in NONFINITE_PARAMS])
def test_gradient_masks_and_values_match_the_reference(name, poison):
    """Part A of tests/test_nonfinite.py under the Laplace likelihood.  `iobs_nan` is the one only the sign() of this branch can break."""
    case, kw, opts, data, cfg, params, u_f, eta, out, grads = _reference_of_a_poisoned_step(name, poison)
    model = laplace_model(case, kw, opts, data, cfg, params)
    inputs = util.reference_inputs(data)
    eng = model.engine(inputs)
    assert_route(eng, case, plan_of(case, kw, opts, data, cfg))
    model(inputs, u_f=u_f, eta=eta)
    torch.cuda.synchronize()
    terms = eng.loss_terms()
    g_hip = [g.cpu().numpy() for g in eng.grad_tensors()]
    names = NF._tensor_names(params)
    assert len(g_hip) == len(grads) == len(names)
    assert not all(np.isfinite(g).all() for g in grads[:2])            # the reference's mask is not empty
    if case.frozen:
        names, g_hip, grads = names[:2], g_hip[:2], grads[:2]
    NF._assert_masks_and_values(names, g_hip, grads)
    kl = float(out["kl"])
    assert abs(terms["kl"] - kl) <= P.RTOL_LOSS * max(abs(kl), 1.0), (terms, kl)
    for k in ("nll", "loss"):
        assert not np.isfinite(float(out[k])) and not np.isfinite(terms[k]), (k, terms, float(out[k]))


@pytest.mark.parametrize("name,poison", NONFINITE_PARAMS, ids=[f"{n}-{p}" for n, p in NONFINITE_PARAMS])
def test_training_stops_after_the_sanitised_step(name, poison):
    """Part B: four steps asked for, one applied."""
    case, kw, opts, data, cfg, params, u_f, eta, out, grads = _reference_of_a_poisoned_step(name, poison)
    model = laplace_model(case, kw, opts, data, cfg, params)
    inputs = util.reference_inputs(data)
    assert_route(model.engine(inputs), case, plan_of(case, kw, opts, data, cfg))
    p = params.clone()
    rec = O.train_step(p, O.inputs_from_numpy(data), RL.under(cfg), O.AdamState.zeros_like(p.tensors()), O.f64(u_f), O.f64(eta))
    after = [t.numpy() for t in p.tensors()]
    hist = model.train_model(inputs, 4, progress=False, noise=lambda i: (u_f, eta))
    eng = model._engine
    assert len(hist["loss"]) == 1 and not np.isfinite(hist["Grad Norm"][0]) and not np.isfinite(rec["Grad Norm"])
    assert abs(hist["F KLDiv"][0] - rec["F KLDiv"]) <= 1e-4 * max(abs(rec["F KLDiv"]), 1.0), (hist["F KLDiv"], rec["F KLDiv"])
    names, got = NF._tensor_names(params), [t.cpu().numpy() for t in eng.param_tensors()]
    assert len(names) == len(got) == len(after)
    if case.frozen:
        names, got, after = names[:2], got[:2], after[:2]
    for n, a, b in zip(names, got, after):
        assert np.isfinite(a).all() and np.isfinite(b).all(), n
        assert util.rel_err(a, b) < 2e-4, (n, util.rel_err(a, b))


# ---- what the engine refuses ---------------------------------------------------------------------------------------------------------------
def test_engine_refuses_a_laplace_likelihood_with_the_evans_error_model():
    from careless_amd.engine import ElboEngine
    from careless_amd.models.likelihoods.mono import LaplaceLikelihood

    class LaplaceEv11Likelihood(LaplaceLikelihood):
        ev11 = True

    kw = dict(N=300, R=40, d0=5, L=2, w=32, S=3)
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    m = util.build_model(data, cfg, params, kw["L"], kw["w"])
    m.likelihood = LaplaceEv11Likelihood()
    with pytest.raises(NotImplementedError, match="LaplaceEv11Likelihood"):
        ElboEngine(m, util.reference_inputs(data), seed=1)


# ---- the slot kernel's Laplace instance, called directly ---------------------------------------------------------------------------------------
def test_cl_laue_likelihood_laplace_instance_and_its_entry_checks():
    """cl_laue_likelihood on real buffers (so a check that did not hold would launch on valid memory): an unknown kind and Laplace beside an
    Evans-2011 buffer return -1 and write nothing; CL_LIK_LAPLACE runs laue_likelihood_laplace_kernel -- iconv := -w dlog p / d iconv and the
    NLL against fp64, an exact zero residual and a NaN observation included.  n = 300 slots x S = 3: four workgroups, the last one ragged."""
    lib = _lib.get_lib()
    rng = np.random.default_rng(5)
    n, S, w = 300, 3, 1.0 / 3
    iobs = (rng.normal(size=n) * 50).astype(np.float32)
    sig = (0.5 + 5 * rng.random(n)).astype(np.float32)
    iconv = (iobs[:, None] + sig[:, None] * 2 * rng.normal(size=(n, S))).astype(np.float32)
    iconv[7, 1] = iobs[7]                   # on the kink: derivative 0
    iobs[11] = np.nan
    dev = lambda a: torch.as_tensor(a, device="cuda")
    t_iobs, t_sig, ev = dev(iobs), dev(sig), torch.zeros(3, device="cuda")

    def call(kind, with_ev=False):
        t_iconv, scal = dev(iconv.copy()), torch.zeros(4, dtype=torch.float64, device="cuda")
        a = _lib.LaueArgs()
        a.iobs, a.sig, a.iconv, a.scalars = t_iobs.data_ptr(), t_sig.data_ptr(), t_iconv.data_ptr(), scal.data_ptr()
        a.n_obs, a.S, a.lik_kind, a.dof, a.w_ll = n, S, kind, 4.0, w
        if with_ev:
            a.ev11, a.d_ev11 = ev.data_ptr(), ev.data_ptr()
        rc = int(lib.cl_laue_likelihood(C.byref(a), None))
        torch.cuda.synchronize()
        return rc, t_iconv.cpu().numpy(), scal.cpu().numpy()
    for kind, with_ev in ((3, False), (7, False), (-1, False), (_lib.CL_LIK_LAPLACE, True)):
        rc, out, scal = call(kind, with_ev)
        assert rc == -1 and np.array_equal(out, iconv, equal_nan=True) and not scal.any(), (kind, with_ev)
    rc, out, scal = call(_lib.CL_LIK_LAPLACE)
    assert rc == 0
    x = O.f64(iconv).requires_grad_(True)
    lp = O.laplace_log_prob(x, O.f64(iobs)[:, None], O.f64(sig)[:, None])
    fin = np.ones((n, S), bool); fin[11] = False
    (g,) = torch.autograd.grad(lp[torch.as_tensor(fin)].sum(), x)
    ref = -np.float64(np.float32(w)) * g.numpy()
    assert out[7, 1] == 0.0 and np.isnan(out[11]).all() and np.isnan(scal[_lib.CL_SC_NLL])
    assert util.rel_err(out[fin], ref[fin]) < 1e-6
    # the NLL without the poisoned slot (a second launch on the finite rows)
    iobs[11] = iconv[11, 0]
    t_iobs = dev(iobs)
    rc, out, scal = call(_lib.CL_LIK_LAPLACE)
    nll = -np.float64(np.float32(w)) * float(O.laplace_log_prob(O.f64(iconv), O.f64(iobs)[:, None], O.f64(sig)[:, None]).sum())
    assert rc == 0 and abs(scal[_lib.CL_SC_NLL] - nll) <= P.RTOL_LOSS * abs(nll) and np.isfinite(out).all()


def test_cl_slot_rows_entry_checks_and_laplace_instance():
    """cl_slot_rows on real buffers: an unknown kind and Laplace beside an Evans-2011 buffer return -1 and write nothing; CL_LIK_LAPLACE
    launches slot_rows_laplace_kernel: the NLL against fp64 (in-kernel noise cannot be restated: eta injected)."""
    lib = _lib.get_lib()
    rng = np.random.default_rng(6)
    n, S, R = 200, 2, 20
    dev = lambda a: torch.as_tensor(a, device="cuda")
    rid = rng.integers(0, R, n).astype(np.int32)
    loc, sigma = (1.0 + rng.random(n)).astype(np.float32), (0.1 * rng.random(n)).astype(np.float32)
    zf = (0.5 + rng.random((R, S))).astype(np.float32)
    eta = rng.normal(size=(n, S)).astype(np.float32)
    ipred = (loc[:, None] + sigma[:, None] * eta) * zf[rid] ** 2
    sig = (0.05 + 0.2 * rng.random(n)).astype(np.float32)
    iobs = (ipred.mean(axis=1) + 3 * sig * rng.normal(size=n)).astype(np.float32)
    t = dict(rid=dev(rid), loc=dev(loc), sigma=dev(sigma), zf=dev(zf), eta=dev(eta), iobs=dev(iobs), sig=dev(sig), iconv=torch.zeros(n * S, device="cuda"),
             ev=torch.zeros(3, device="cuda"))

    def call(kind, with_ev=False):
        dzf, dO, scal = torch.zeros(R * S, device="cuda"), torch.zeros(2 * n, device="cuda"), torch.zeros(4, dtype=torch.float64, device="cuda")
        a = _lib.LaueArgs()
        a.refl_id, a.loc, a.sigma, a.z_f, a.eta, a.iobs, a.sig, a.iconv = (t[k].data_ptr() for k in ("rid", "loc", "sigma", "zf", "eta", "iobs", "sig", "iconv"))
        a.dz_f, a.dO, a.scalars = dzf.data_ptr(), dO.data_ptr(), scal.data_ptr()
        a.n_obs, a.R, a.S, a.lik_kind, a.dof, a.w_ll = n, R, S, kind, 4.0, 0.5
        if with_ev:
            a.ev11, a.d_ev11 = t["ev"].data_ptr(), t["ev"].data_ptr()
        rc = int(lib.cl_slot_rows(C.byref(a), None))
        torch.cuda.synchronize()
        return rc, dzf.cpu().numpy(), dO.cpu().numpy(), scal.cpu().numpy()
    for kind, with_ev in ((3, False), (-1, False), (_lib.CL_LIK_LAPLACE, True)):
        rc, dzf, dO, scal = call(kind, with_ev)
        assert rc == -1 and not dzf.any() and not dO.any() and not scal.any(), (kind, with_ev)
    rc, dzf, dO, scal = call(_lib.CL_LIK_LAPLACE)
    nll = -0.5 * float(O.laplace_log_prob(O.f64(ipred), O.f64(iobs)[:, None], O.f64(sig)[:, None]).sum())
    assert rc == 0 and abs(scal[_lib.CL_SC_NLL] - nll) <= P.RTOL_LOSS * abs(nll) and dzf.any() and np.isfinite(dzf).all()
