"""The Rice-Woolfson surrogate posterior on the GPU: `cl_rw_forward` / `cl_rw_backward` / `cl_rw_moments` called directly on injected
normals, whole training steps of the engine against the fp64 oracle under `ElboConfig.posterior = "rice_woolfson"`, deterministic mode, shards, the non-finite step contract, the production noise, the output step and an
oracle-independent recovery run.

Whole-step cases are rows of tests/test_nonfinite.py's MATRIX with `model.surrogate_posterior` replaced and that file's routing assertions
unchanged: the posterior must not move a route or a kernel name.  Every test on injected noise asserts on the reference alone that no
centric draw has |loc + scale n1| < 1e-4 scale (fp32 could land on the other side of the kink of |.|); `ref_rw.noise_for` picks the first
seed that keeps it.  Tolerances are the project's: `RTOL_LOSS` / `RTOL_GRAD` of tests/test_gpu_parity.py with its LeakyReLU branch gate,
1e-5 element by element on z_f and the moments (the bar of `cl_tn_moments`), 2e-4 on a trajectory, 1e-4 on the output step."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from careless_amd import _lib
from oracle import elbo_oracle as O
from tests import ref_prior as RP
from tests import ref_rw as RR
from tests import ref_step
from tests import test_gpu_parity as P
from tests import test_nonfinite as NF
from tests import util

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda"
EPS = 1e-7
KL_BEFORE, SENT = 3.5, -7.25e30      # scalars[CL_SC_KL] before a call that ADDS; what a kl_part slot / z_f element holds before a call that STORES


# ---- the kernels, called directly --------------------------------------------------------------------------------------------------------------
def direct_inputs(R, S, family, seed):
    """loc / scale from 1e-3 to 1e3 (both sides of every branch of cl_i0e_i1e, of cl_one_minus_i1_over_i0 and of the reference's 40), scales
    from 0.03 to 30; a Wilson prior commensurate with every reflection's own q (es = (loc^2 + scale^2) x 0.5 .. 2), so that no reflection's
    terms drown the others' in the KL or in a gradient's max-norm."""
    rng = np.random.default_rng(1000 * seed + 10 * R + S)
    ratio = 10 ** np.linspace(-3, 3, R)[rng.permutation(R)] if R > 1 else np.array([2.0])
    scale = 10 ** rng.uniform(-1.5, 1.5, R)
    a = np.log(ratio * scale).astype(np.float32)
    b = np.log(scale - EPS).astype(np.float32)
    centric = {"centric": np.ones(R, bool), "acentric": np.zeros(R, bool), "alternating": np.arange(R) % 2 == 0}[family]
    loc64, scale64 = np.exp(a.astype(np.float64)), np.exp(b.astype(np.float64)) + float(np.float32(EPS))
    n_f = RR.noise_for(loc64, scale64, centric, S, 50 * seed)
    es = ((loc64 ** 2 + scale64 ** 2) * (0.5 + 1.5 * rng.random(R))).astype(np.float32)
    dz = (rng.normal(size=(R, S)) / (loc64 + scale64)[:, None]).astype(np.float32)       # dL/dz of a loss of O(1) per reflection
    pre = rng.normal(size=(2, R)).astype(np.float32)
    return a, b, centric, loc64, scale64, n_f, es, dz, pre


def run_direct(R, S, family, with_part, inner_kl, owned, prior="wilson", stop=False, seed=0):
    lib = _lib.get_lib()
    a, b, centric, loc64, scale64, n_f, es, dz, pre = direct_inputs(R, S, family, seed)
    assert RR.kink_margin(loc64, scale64, centric, n_f) >= RR.KINK_GUARD
    k0, k1 = (R // 3, R - R // 4) if inner_kl and R >= 4 else (0, R)
    r0, r1 = (R // 5, R - R // 6) if owned and R >= 6 else (0, 0)
    own = np.ones(R, bool) if r1 <= r0 else (np.arange(R) >= r0) & (np.arange(R) < r1)
    in_kl = (np.arange(R) >= k0) & (np.arange(R) < k1) & own
    nb = (int(own.sum()) + 255) // 256
    w_kl, mult = 1.0 / S, (0.5 if S == 3 else 1.0)
    ref_kind = prior == "reference"
    junk = np.full(37, 5.5, np.float32)
    g = ref_step.Guarded(DEV).add("a", a).add("b", b).add("qc", centric.astype(np.uint8)).add("n_f", np.ascontiguousarray(n_f.transpose(0, 2, 1)))
    g.add("pc", centric.astype(np.uint8)).add("es", es)
    g.add("z_f", np.full((R, S), SENT, np.float32), np.repeat(own[:, None], S, axis=1))
    g.add("dz_in", dz).add("dz_zero", np.full((R, S), 2.5, np.float32), np.repeat(own[:, None], S, axis=1) if with_part else False)
    g.add("d_a", pre[0], own).add("d_b", pre[1], own)
    g.add("kl_part", np.full(nb + 3, SENT), ([True] * nb + [False] * 3) if with_part else False)
    g.add("kl_part_dw", np.arange(1.0, (R + 255) // 256 + 1.0))
    g.add("zero", junk, with_part)
    g.add("scalars", np.array([1.25, KL_BEFORE, 7.0, 6.0]), [False, True, False, False])
    g.add("stop", np.array([1 if stop else 0], np.int32)).build()
    A = _lib.RwArgs()
    t = A.tn
    t.q_loc_raw, t.q_scale_raw, t.low = g.ptr("a"), g.ptr("b"), None
    t.centric, t.es = (None, None) if ref_kind else (g.ptr("pc"), g.ptr("es"))
    t.prior_kind = _lib.CL_PRIOR_REFERENCE if ref_kind else _lib.CL_PRIOR_WILSON
    t.R, t.S, t.high, t.eps, t.w_kl, t.kl_grad_mult = R, S, 1e10, EPS, w_kl, mult
    t.kl_begin, t.kl_end, t.r_begin, t.r_end = k0, k1, r0, r1
    t.z_f, t.dz_f, t.d_loc_raw, t.d_scale_raw, t.scalars, t.stop_flag = g.ptr("z_f"), g.ptr("dz_in"), g.ptr("d_a"), g.ptr("d_b"), g.ptr("scalars"), g.ptr("stop")
    if with_part:
        t.kl_part, t.kl_part_dw = g.ptr("kl_part"), g.ptr("kl_part_dw")
        t.zero_ptr, t.zero_n, t.zero_dzf = g.ptr("zero"), len(junk), g.ptr("dz_zero")
    A.q_centric, A.n_f = g.ptr("qc"), g.ptr("n_f")
    assert int(lib.cl_rw_forward(C.byref(A), None)) == 0
    assert int(lib.cl_rw_backward(C.byref(A), None)) == 0
    torch.cuda.synchronize()
    g.verify(untouched=stop)             # guards, inputs, rows outside the owned range, unused slots: bit-identical; a raised flag: everything
    if stop:
        return
    what = (R, S, family, with_part, inner_kl, owned, prior)
    # fp64 reference, [S][R] orientation
    ta, tb = O.f64(a).requires_grad_(True), O.f64(b).requires_grad_(True)
    loc, scale = torch.exp(ta), torch.exp(tb) + float(np.float32(EPS))
    ct = torch.as_tensor(centric)
    z = O.rw_sample(loc, scale, ct, O.f64(n_f))
    lq = O.rw_log_prob(z, loc, scale, ct)
    lp = torch.zeros_like(lq) if ref_kind else O.wilson_log_prob(z, ct, O.f64(np.ones(R)), O.f64(es))
    wk = np.float64(np.float32(w_kl))
    kl_e = ((lq - lp) * O.f64(in_kl.astype(np.float64))).sum()
    loss = (O.f64(dz.T) * z * O.f64(own.astype(np.float64))).sum() + wk * mult * kl_e
    ga, gb = torch.autograd.grad(loss, [ta, tb])
    zf = g.get("z_f")
    zr = z.detach().numpy().T
    assert np.all(zf[~own] == np.float32(SENT))
    err = np.max(np.abs(zf[own] - zr[own]) / zr[own])
    assert err < 1e-5, (what, "z_f", err)
    kl_ref = wk * float(kl_e.detach())
    if with_part:
        assert g.changed("kl_part")[:nb].all() and np.all(g.get("zero") == 0.0) and np.all(g.get("dz_zero")[own] == 0.0), what
        kl_ref += float(np.arange(1.0, (R + 255) // 256 + 1.0).sum()) if ref_kind else 0.0        # (kl_part_dw: the reference prior's parts ride along)
    kl = float(g.get("scalars")[_lib.CL_SC_KL]) - KL_BEFORE
    print(f"{what}: kl {kl:.9g} reference {kl_ref:.9g}")
    assert abs(kl - kl_ref) <= P.RTOL_LOSS * max(abs(kl_ref), 1.0), (what, kl, kl_ref)
    for name, got, ref, p in (("d_loc_raw", g.get("d_a"), ga.numpy(), pre[0]), ("d_scale_raw", g.get("d_b"), gb.numpy(), pre[1])):
        inc = got.astype(np.float64) - p.astype(np.float64)
        assert np.all(inc[~own] == 0.0), (what, name)
        e = np.max(np.abs(inc - ref)) / np.max(np.abs(ref))
        print(f"{what}: {name} error / max-norm {e:.2e}")
        assert e < P.RTOL_GRAD, (what, name, e)


@pytest.mark.parametrize("family", ["centric", "acentric", "alternating"])
@pytest.mark.parametrize("R", [1, 255, 256, 257, 600])
def test_direct_calls_match_fp64(R, family):
    for S, with_part, inner_kl, owned in itertools.product((1, 3, 8), (True, False), (False, True), (False, True)):
        if R == 1 and (inner_kl or owned):
            continue
        run_direct(R, S, family, with_part, inner_kl, owned)


def test_direct_calls_under_a_reference_prior_leave_the_prior_term_out():
    for with_part in (True, False):
        run_direct(600, 3, "alternating", with_part, True, False, prior="reference")


@pytest.mark.parametrize("with_part", [True, False])
def test_direct_calls_with_a_raised_stop_flag_write_nothing(with_part):
    run_direct(600, 3, "alternating", with_part, False, False, stop=True)
    run_direct(600, 3, "alternating", with_part, True, True, stop=True)


def test_cl_rw_moments_matches_the_host_class_and_the_closed_forms():
    from careless_amd.models.merging.surrogate_posteriors import RiceWoolfson
    R = 600
    a, b, centric, loc64, scale64, *_ = direct_inputs(R, 1, "alternating", 3)
    q = RiceWoolfson.from_loc_and_scale(np.ones(R), np.ones(R), centric, scale_shift=EPS)
    q.loc_raw, q.scale_raw = torch.as_tensor(a), torch.as_tensor(b)
    mean, var, m4 = O.rw_moments(loc64, scale64, centric)
    host = RiceWoolfson(loc64, scale64, centric)                       # the fp32 host class itself, pinned to scipy by tests/test_ref_prior.py
    assert np.allclose(host.mean(), mean, rtol=1e-5)
    for got, ref, k in ((q.mean(), mean, "mean"), (q.stddev(), np.sqrt(var), "std"), (q.variance(), var, "var"), (q.moment_4(), m4, "m4")):
        got = got.cpu().numpy() if torch.is_tensor(got) else got
        err = np.max(np.abs(got - ref) / np.abs(ref))
        print(k, err)
        assert err < (2e-5 if k == "var" else 1e-5), (k, err)           # (the variance is the fp32 std squared: twice its rounding)
    assert (loc64 / scale64 > 40).sum() > 100 and (loc64 / scale64 < 0.1).sum() > 100
    z = q.sample(4, seed=3)
    assert z.shape == (4, R) and bool(torch.isfinite(z).all()) and float(z.min()) > 0.0 and q.sample(seed=1).shape == (R,)


# ---- whole steps: rows of tests/test_nonfinite.py's MATRIX under the Rice-Woolfson posterior -----------------------------------------------------
STEP_ROWS = ["mlp64_5x64_posenc_studentt_S8", "lane_20x10_d5_S1", "lane_image_layers1_20x10", "mlp_packed_laue_single_pass_2x32", "laue_two_pass_2x32",
             "wide_3x96", "double_wilson_2x32", "double_wilson_trainable_r", "ev11_studentt_5x64_S8", "frozen_mono_20x10", "klweight_4x48",
             "chain_24x10_lane_block", "mlp_image_layers1_2x32"]


def q_loc_scale(params, cfg):
    return tuple(t.numpy() for t in O.tn_loc_scale(params.q_loc_raw.double(), params.q_scale_raw.double(), cfg.epsilon))


def problem(name, poison=None):
    """The row's problem (tests/test_nonfinite.py: `_problem`, optionally poisoned) with the (2, S, R) normals in place of the uniforms.
    Returns (case, kw, opts, data, cfg, params, n_f, eta, centric)."""
    case = NF.MATRIX[name]
    if poison is not None:
        case, kw, opts, data, cfg, params, _, eta, _ = NF._problem(name, poison, "inner")
    else:
        kw = dict(case.kw, seed=case.seed)
        opts = {k: kw.pop(k, None) for k in ("two_pass", "regroup", "shuffle_rows", "grid")}
        data, cfg, params, _, _, eta = util.make_problem(**kw)
        if opts["regroup"]:
            data = P._regroup_laue(data, opts["regroup"])
    centric = np.asarray(data["centric"], dtype=bool)
    loc, scale = q_loc_scale(params, cfg)
    n_f = RR.noise_for(loc, scale, centric, cfg.mc_samples, case.seed)
    return case, kw, opts, data, cfg, params, n_f, eta, centric


def rw_posterior(params, cfg, centric):
    from careless_amd.models.merging.surrogate_posteriors import TrainableRiceWoolfson
    return TrainableRiceWoolfson(params.q_loc_raw.numpy().astype(np.float32), params.q_scale_raw.numpy().astype(np.float32), centric, scale_shift=cfg.epsilon)


def rw_model(case, kw, opts, data, cfg, params, centric, **attrs):
    model = NF._model(case, kw, opts, data, cfg, params)
    model.surrogate_posterior = rw_posterior(params, cfg, centric)
    for k, v in attrs.items():
        setattr(model, k, v)
    return model


def assert_terms(terms, out, name):
    for k in ("nll", "kl", "loss"):
        den = max(abs(float(out[k])), 1.0) if k == "kl" else abs(float(out[k]))
        print(f"{name}: {k} engine {terms[k]:.9g} reference {float(out[k]):.9g}")
        assert abs(terms[k] - float(out[k])) <= P.RTOL_LOSS * den, (name, k, terms, float(out[k]))


def assert_grads(g_hip, reference, name):
    """tests/test_gpu_parity.py's gate: every tensor at RTOL_GRAD; a LeakyReLU pre-activation within fp32 rounding of zero may sit on the
    engine's branch.  `reference(flips=, near=)` -> (out, grads).  Compares the leading len(g_hip) tensors."""
    n = len(g_hip)
    _, grads = reference()
    errs = [util.rel_err(a, b.numpy()) for a, b in zip(g_hip, grads[:n])]
    print(f"{name}: gradient errors {['%.1e' % e for e in errs]}")
    if max(errs) < P.RTOL_GRAD:
        return
    near = []
    reference(near=near)
    near.sort()
    cand = [(l, r, u) for _, l, r, u in near[:P.MAX_FLIP_CANDIDATES]]
    assert cand, f"{name}: gradient errors {errs} and no LeakyReLU pre-activation within fp32 rounding of zero: not a branch flip"
    for k in range(1, len(cand) + 1):
        for sub in itertools.combinations(cand, k):
            _, gf = reference(flips=sub)
            if max(util.rel_err(a, b.numpy()) for a, b in zip(g_hip, gf[:n])) < P.RTOL_GRAD:
                print(f"{name}: gradients match with the LeakyReLU unit(s) {list(sub)} on the engine's branch")
                return
    raise AssertionError(f"{name}: gradient errors {errs}; no forced-branch assignment of {cand} brings them under {P.RTOL_GRAD}")


def assert_samples(eng, out, name):
    z = eng.z_f.view(eng.R, eng.S).t().cpu().numpy()
    ref = out["z_f"].numpy()
    err = float(np.max(np.abs(z - ref) / ref))
    print(f"{name}: z_f element error {err:.2e}")
    assert err < 1e-5, (name, err)


@pytest.mark.parametrize("name", STEP_ROWS)
def test_whole_step_matches_the_fp64_reference(name):
    case, kw, opts, data, cfg, params, n_f, eta, centric = problem(name)
    x = O.inputs_from_numpy(data)
    assert RR.kink_margin(*q_loc_scale(params, cfg), centric, n_f) >= RR.KINK_GUARD
    reference = lambda **k: O.elbo_value_and_grads(params, x, RR.under(cfg), O.f64(n_f), O.f64(eta), **k)
    out, grads = reference()
    model = rw_model(case, kw, opts, data, cfg, params, centric)
    inputs = util.reference_inputs(data)
    eng = model.engine(inputs)
    NF._assert_route(eng, case)                      # the posterior moves no route and no kernel name
    assert eng.rw
    ipred = model(inputs, u_f=n_f, eta=eta)
    torch.cuda.synchronize()
    assert_samples(eng, out, name)
    assert util.rel_err(ipred.cpu().numpy(), out["ipred"].numpy()) < 1e-4
    assert_terms(eng.loss_terms(), out, name)
    g_hip = [g.cpu().numpy() for g in eng.grad_tensors()]
    assert len(g_hip) == len(grads)
    if case.frozen:                                  # the scaler's gradient is not computed: q's two tensors lead both lists
        g_hip = g_hip[:2]
    assert_grads(g_hip, reference, name)
    # the posterior matters: the same problem under the truncated normal has another KL
    u = np.random.default_rng(1).random((cfg.mc_samples, len(centric)))
    assert abs(float(out["kl"]) - float(O.elbo_value_and_grads(params, x, cfg, O.f64(u), O.f64(eta))[0]["kl"])) > 1e-3


def test_whole_step_under_a_reference_prior():
    from tests.test_ref_prior_gpu import make_prior
    name, kw = "rice_woolfson_reference_prior_masked_20x10", dict(N=500, R=50, d0=5, L=20, w=10, S=2, perturb=0.02)
    data, cfg, params, x, _, eta = util.make_problem(**kw)
    centric = np.asarray(data["centric"], dtype=bool)
    prior = make_prior("rice_woolfson", data, params, True)
    n_f = RR.noise_for(*q_loc_scale(params, cfg), centric, kw["S"], 7)

    reference = lambda **k: O.elbo_value_and_grads(params, *RP.under(x, RR.under(cfg), prior), O.f64(n_f), O.f64(eta), **k)
    out, grads = reference()
    model = util.build_model(data, cfg, params, kw["L"], kw["w"])
    model.prior, model.surrogate_posterior = prior, rw_posterior(params, cfg, centric)
    inputs = util.reference_inputs(data)
    ipred = model(inputs, u_f=n_f, eta=eta)
    eng = model._engine
    torch.cuda.synchronize()
    assert eng.rw and eng.ref_prior and eng.centric is None and "elbo_lane_kernel" in eng.kernel_name()
    assert_samples(eng, out, name)
    assert util.rel_err(ipred.cpu().numpy(), out["ipred"].numpy()) < 1e-4
    assert_terms(eng.loss_terms(), out, name)
    assert_grads([g.cpu().numpy() for g in eng.grad_tensors()], reference, name)


def _plain(kw, seed=7):
    data, cfg, params, x, _, _ = util.make_problem(seed=seed, **kw)
    centric = np.asarray(data["centric"], dtype=bool)

    def fresh(**attrs):
        m = util.build_model(data, cfg, params, kw["L"], kw["w"])
        m.surrogate_posterior = rw_posterior(params, cfg, centric)
        for k, v in attrs.items():
            setattr(m, k, v)
        return m
    return fresh, data, cfg, params, x, centric


def test_adam_trajectory_matches_the_reference_loop():
    kw, steps = dict(N=384, R=48, d0=5, L=2, w=32, S=2), 20
    fresh, data, cfg, params, x, centric = _plain(kw)
    rng = np.random.default_rng(11)
    p = params.clone()
    st = O.AdamState.zeros_like(p.tensors())
    noises, ref = [], []
    for i in range(steps):                           # the noise of step i keeps the kink guard at the reference's parameters of step i
        n_f = RR.noise_for(*q_loc_scale(p, cfg), centric, kw["S"], 100 + 10 * i)
        noises.append((n_f, rng.normal(size=(kw["S"], kw["N"])).astype(np.float32)))
        ref.append(O.train_step(p, x, RR.under(cfg), st, *map(O.f64, noises[-1])))
    model = fresh()
    hist = model.train_model(util.reference_inputs(data), steps, progress=False, noise=lambda i: noises[i])
    for k in ("loss", "NLL", "F KLDiv", "Grad Norm"):
        a, b = np.array(hist[k]), np.array([r[k] for r in ref])
        assert len(a) == steps and np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)) < 2e-4, (k, a, b)
    got = [t.cpu().numpy() for t in model._engine.param_tensors()]
    for a, b in zip(got, p.tensors()):
        assert util.rel_err(a, b.numpy()) < 2e-4
    assert util.rel_err(got[0], params.q_loc_raw.numpy()) > 1e-3            # the posterior moved


def test_validation_nll_matches_the_reference():
    kw, n_tr = dict(N=384, R=48, d0=5, L=2, w=32, S=2), 300
    fresh, data, cfg, params, x, centric = _plain(kw)
    inputs = util.reference_inputs(data)
    train, test = tuple(a[:n_tr] for a in inputs), tuple(a[n_tr:] for a in inputs)

    def as_inputs(t):
        d = dict(data)
        d.update(refl_id=t[0][:, 0], image_id=t[1][:, 0], metadata=t[3], iobs=t[4][:, 0], sigiobs=t[5][:, 0])
        return O.inputs_from_numpy(d)
    x_tr, x_te = as_inputs(train), as_inputs(test)
    rng = np.random.default_rng(12)
    noise = (RR.noise_for(*q_loc_scale(params, cfg), centric, 2, 3), rng.normal(size=(2, n_tr)).astype(np.float32))
    p = params.clone()
    rec = O.train_step(p, x_tr, RR.under(cfg), O.AdamState.zeros_like(p.tensors()), *map(O.f64, noise))
    vnoise = (RR.noise_for(*q_loc_scale(p, cfg), centric, 2, 40), rng.normal(size=(2, kw["N"] - n_tr)).astype(np.float32))
    ref = O.validation_nll(p, x_te, RR.under(cfg), O.f64(vnoise[0]), O.f64(vnoise[1]), n_tr)
    model = fresh()
    hist = model.train_model(train, 1, progress=False, validation_data=test, validation_frequency=1, noise=lambda i: noise, validation_noise=lambda i: vnoise)
    print("NLL_val", hist["NLL_val"], "reference", ref)
    assert len(hist["NLL_val"]) == 1 and abs(hist["NLL_val"][0] - ref) <= P.RTOL_LOSS * abs(ref)
    assert abs(hist["NLL"][0] - rec["NLL"]) <= P.RTOL_LOSS * abs(rec["NLL"])


# ---- deterministic mode ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["det_mlp_5x64", "det_packed_laue_5x64"])
def test_deterministic_mode_repeats_bit_for_bit(name):
    from careless_amd.engine import ElboEngine
    case, kw, opts, data, cfg, params, _, _, centric = problem(name)
    inputs = util.reference_inputs(data)
    runs = []
    for _ in range(2):
        e = ElboEngine(rw_model(case, kw, opts, data, cfg, params, centric), inputs, seed=5)
        assert e.deterministic and e.rw and case.frag in e.kernel_name()
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


# ---- shards ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("owner", [False, True], ids=["row_split", "owner_split"])
def test_shards_sum_to_the_one_rank_step(owner, world):
    """Production noise: every shard draws the numbers of its GLOBAL reflection indices, or the sum would not be the full step's."""
    from careless_amd.engine import ElboEngine, make_shard
    kw = dict(N=600, R=50, d0=5, L=2, w=32, S=2)
    fresh, data, cfg, params, x, centric = _plain(kw)
    inputs = util.reference_inputs(data)
    full = ElboEngine(fresh(), inputs, seed=99)
    full.forward_backward(3)
    torch.cuda.synchronize()
    g_full, t_full, z_full = full.grads.clone(), full.loss_terms(), full.z_f.view(kw["R"], kw["S"]).clone()
    g_sum, nll, kl = torch.zeros_like(g_full), 0.0, 0.0
    for r in range(world):
        eng = ElboEngine(fresh(owner_shard=owner), inputs, seed=99, shard=make_shard(kw["N"], kw["R"], r, world))
        k0, k1 = eng.shard.kl_begin, eng.shard.kl_end
        assert bool(eng.owner) == owner and eng.rw and 0 < k1 - k0 < kw["R"]
        eng.local_only = True
        eng.forward_backward(3)
        torch.cuda.synchronize()
        z = eng.z_f.view(kw["R"], kw["S"])
        assert torch.equal(z[k0:k1], z_full[k0:k1]) and (owner or torch.equal(z, z_full))
        g_sum += eng.grads
        t = eng.loss_terms()
        nll += t["nll"]; kl += t["kl"]
    assert abs(nll - t_full["nll"]) <= 1e-5 * abs(t_full["nll"]) and abs(kl - t_full["kl"]) <= 1e-5 * max(abs(t_full["kl"]), 1.0)
    assert util.rel_err(g_sum.cpu().numpy(), g_full.cpu().numpy()) < 2e-5


# ---- the non-finite step contract --------------------------------------------------------------------------------------------------------------
NONFINITE_ROWS = ["lane_20x10_d5_S1", "mlp64_5x64_posenc_studentt_S8"]


def _poisoned(name):
    case, kw, opts, data, cfg, params, n_f, eta, centric = problem(name, "iobs_nan")
    near = []
    out, grads = O.elbo_value_and_grads(params, O.inputs_from_numpy(data), RR.under(cfg), O.f64(n_f), O.f64(eta), near=near)
    assert not [t for t in near if np.isfinite(t[0])]          # no LeakyReLU branch in doubt (tests/test_nonfinite.py: `_oracle_grads`)
    return case, kw, opts, data, cfg, params, n_f, eta, centric, out, [g.numpy() for g in grads]


@pytest.mark.parametrize("name", NONFINITE_ROWS)
def test_gradient_masks_and_values_match_the_reference(name):
    case, kw, opts, data, cfg, params, n_f, eta, centric, out, grads = _poisoned(name)
    model = rw_model(case, kw, opts, data, cfg, params, centric)
    inputs = util.reference_inputs(data)
    eng = model.engine(inputs)
    NF._assert_route(eng, case)
    model(inputs, u_f=n_f, eta=eta)
    torch.cuda.synchronize()
    terms = eng.loss_terms()
    g_hip = [g.cpu().numpy() for g in eng.grad_tensors()]
    names = NF._tensor_names(params)
    assert len(g_hip) == len(grads) == len(names)
    assert not all(np.isfinite(g).all() for g in grads[:2]) and np.isfinite(grads[0]).mean() >= 0.9
    NF._assert_masks_and_values(names, g_hip, grads)
    kl = float(out["kl"])
    assert abs(terms["kl"] - kl) <= P.RTOL_LOSS * max(abs(kl), 1.0), (terms, kl)
    for k in ("nll", "loss"):
        assert not np.isfinite(float(out[k])) and not np.isfinite(terms[k]), (k, terms, float(out[k]))


@pytest.mark.parametrize("name", NONFINITE_ROWS)
def test_training_stops_after_the_sanitised_step(name):
    case, kw, opts, data, cfg, params, n_f, eta, centric, out, grads = _poisoned(name)
    model = rw_model(case, kw, opts, data, cfg, params, centric)
    inputs = util.reference_inputs(data)
    NF._assert_route(model.engine(inputs), case)
    p = params.clone()
    rec = O.train_step(p, O.inputs_from_numpy(data), RR.under(cfg), O.AdamState.zeros_like(p.tensors()), O.f64(n_f), O.f64(eta))
    after = [t.numpy() for t in p.tensors()]
    hist = model.train_model(inputs, 4, progress=False, noise=lambda i: (n_f, eta))
    assert len(hist["loss"]) == 1 and not np.isfinite(hist["Grad Norm"][0]) and not np.isfinite(rec["Grad Norm"])
    assert abs(hist["F KLDiv"][0] - rec["F KLDiv"]) <= 1e-4 * max(abs(rec["F KLDiv"]), 1.0), (hist["F KLDiv"], rec["F KLDiv"])
    names, got = NF._tensor_names(params), [t.cpu().numpy() for t in model._engine.param_tensors()]
    assert len(names) == len(got) == len(after)
    for n, a, b in zip(names, got, after):
        assert np.isfinite(a).all() and np.isfinite(b).all(), n
        assert util.rel_err(a, b) < 2e-4, (n, util.rel_err(a, b))


# ---- production noise ----------------------------------------------------------------------------------------------------------------------------
def test_debug_noise_kind_2_is_what_a_step_consumes():
    from careless_amd.engine import ElboEngine, debug_noise
    kw = dict(N=600, R=50, d0=5, L=2, w=32, S=3)
    fresh, data, cfg, params, x, centric = _plain(kw)
    inputs = util.reference_inputs(data)
    eng = ElboEngine(fresh(), inputs, seed=77)
    eng.forward_backward(6)
    torch.cuda.synchronize()
    z_drawn, g_drawn = eng.z_f.clone(), eng.grads[: 2 * kw["R"]].clone()
    pairs = debug_noise(77, 6, kw["S"], kw["R"], kind=2)                  # [R][S][2]
    assert pairs.shape == (kw["R"], kw["S"], 2)
    eng.forward_backward(6, pairs.permute(2, 0, 1).contiguous())        # the device layout of injected normals: [2][R][S]
    torch.cuda.synchronize()
    assert torch.equal(eng.z_f, z_drawn) and float(z_drawn.min()) > 0.0
    assert util.rel_err(eng.grads[: 2 * kw["R"]].cpu().numpy(), g_drawn.cpu().numpy()) < 1e-5      # (the data term's atomics reorder sums)
    # another step, another seed: other numbers; a shard's reflections: the numbers of their global indices
    assert not torch.equal(debug_noise(77, 7, kw["S"], kw["R"], kind=2), pairs) and not torch.equal(debug_noise(78, 6, kw["S"], kw["R"], kind=2), pairs)
    assert torch.equal(debug_noise(77, 6, kw["S"], 20, offset=30, kind=2), pairs[30:])
    # ... and not the scale noise's stream at equal indices
    scale_n = debug_noise(77, 6, kw["S"], kw["R"], kind=1)
    assert not bool((pairs[..., 0] == scale_n).any()) and not bool((pairs[..., 1] == scale_n).any())


def test_production_noise_is_standard_normal_and_the_pair_is_independent():
    from careless_amd.engine import debug_noise
    n, S = 125_000, 8
    p = debug_noise(20260, 3, S, n, kind=2).double().reshape(-1, 2)
    N = p.shape[0]
    assert N == 1_000_000 and bool(torch.isfinite(p).all())
    se_mean, se_var, se_cor = 1.0 / np.sqrt(N), np.sqrt(2.0 / N), 1.0 / np.sqrt(N)
    for k in range(2):
        m, v = float(p[:, k].mean()), float(p[:, k].var())
        print(f"n{k + 1}: mean {m:.2e} variance {v:.6f}")
        assert abs(m) < 5 * se_mean and abs(v - 1.0) < 5 * se_var
    cor = float((p[:, 0] * p[:, 1]).mean())
    cor2 = float(((p[:, 0] ** 2 - 1) * (p[:, 1] ** 2 - 1)).mean())        # (a shared radius shows here: E = 0 for an independent pair, sd 2)
    print(f"pair correlation {cor:.2e}, of the squares {cor2:.2e}")
    assert abs(cor) < 5 * se_cor and abs(cor2) < 5 * 2.0 / np.sqrt(N)
    # neighbouring samples and neighbouring reflections are not copies of each other
    q = p.reshape(n, S, 2)
    assert abs(float((q[:, 0, 0] * q[:, 1, 0]).mean())) < 5 / np.sqrt(n) and abs(float((q[:-1, 0, 0] * q[1:, 0, 0]).mean())) < 5 / np.sqrt(n)


# ---- the output step -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(N=500, R=40, d0=5, L=2, w=32, S=2), dict(N=600, R=50, L=2, w=32, S=2, laue=True)], ids=["mono_2x32", "laue_2x32"])
def test_predictions_and_results_match_the_reference(kw):
    from careless_amd import results
    from tests.test_output_step import _close
    fresh, data, cfg, params, x, centric = _plain(kw)
    # off the initial state: loc / scale spread over two decades
    rng = np.random.default_rng(4)
    params.q_scale_raw = params.q_scale_raw + torch.as_tensor(rng.uniform(-3.0, 1.0, kw["R"]))
    model = fresh()
    inputs = util.reference_inputs(data)
    pred = results.get_predictions(model, inputs)
    res = results.get_results(model.surrogate_posterior, inputs)
    ie, isd = O.prediction_mean_stddev(params, x, RR.under(cfg))
    sm, ssd = O.scale_mean_stddev(params, x, RR.under(cfg))
    ref = O.merged_results(params, x, RR.under(cfg))
    for k, r in (("Ipred", ie), ("SigIpred", isd), ("Scale", sm), ("SigScale", ssd)):
        assert len(pred[k]) == kw["N"] and _close(pred[k], r.numpy()), k
    for k in ("F", "SigF", "I", "SigI"):
        assert _close(res[k], ref[k].numpy()), k
    assert np.array_equal(res["N"], np.bincount(np.asarray(data["refl_id"]), minlength=kw["R"]))
    assert np.array_equal(res["centric"], centric.astype(np.float32)) and np.allclose(res["loc"], np.exp(params.q_loc_raw.numpy()), rtol=1e-6)


def test_data_manager_builds_a_model_around_the_posterior():
    from careless_amd.manager import DataManager, default_args
    from careless_amd.models.merging.surrogate_posteriors import RiceWoolfson
    from careless_amd.synthetic import make_synthetic
    from careless_amd.workloads import reference_inputs
    d = make_synthetic(20_000)
    args = default_args(mlp_layers=2, mlp_width=32, iterations=10)
    dm = DataManager(reference_inputs(d), d["centric"], d["multiplicity"], parser=args)
    q0 = dm.build_model().surrogate_posterior
    q = RiceWoolfson.from_loc_and_scale(q0.loc, q0.scale, d["centric"], scale_shift=args.epsilon)
    model = dm.build_model(surrogate_posterior=q)
    hist = model.train_model(dm.inputs, 10, progress=False)
    assert model.surrogate_posterior is q and model._engine.rw and len(hist["loss"]) == 10 and np.all(np.isfinite(hist["loss"]))
    res = dm.get_results(q)
    assert np.isfinite(res["F"]).all() and np.isfinite(res["SigI"]).all() and (res["SigF"] > 0).all()
    # --freeze-structure-factors: the posterior's two tensors stay where they are
    q.trainable = False
    before = q.loc_raw.clone()
    model.train_model(dm.inputs, 3, progress=False)
    assert torch.equal(q.loc_raw, before)


# ---- oracle-independent ----------------------------------------------------------------------------------------------------------------------------
def test_training_recovers_the_true_amplitudes_under_both_posteriors():
    """tests/test_recovery.py's bar, CC(F, F_true) >= 0.99, on the same data and seed under the truncated normal and under Rice-Woolfson:
    mono, 200 k observations, 1 500 steps, production noise."""
    from careless_amd.manager import DataManager, default_args
    from careless_amd.models.merging.surrogate_posteriors import RiceWoolfson
    from careless_amd.synthetic import make_synthetic
    from careless_amd.workloads import reference_inputs
    from tests.test_recovery import _cc
    steps = 1500
    d = make_synthetic(200_000)
    inputs = reference_inputs(d)
    cc = {}
    for kind in ("truncated_normal", "rice_woolfson"):
        args = default_args(mlp_layers=5, mlp_width=64, iterations=steps, learning_rate=0.01)
        np.random.seed(args.seed)
        dm = DataManager(inputs, d["centric"], d["multiplicity"], parser=args)
        model = dm.build_model()
        if kind == "rice_woolfson":
            q0 = model.surrogate_posterior
            model = dm.build_model(surrogate_posterior=RiceWoolfson.from_loc_and_scale(q0.loc, q0.scale, d["centric"], scale_shift=args.epsilon))
        hist = model.train_model(dm.inputs, steps, progress=False)
        assert len(hist["loss"]) == steps and np.all(np.isfinite(hist["loss"])) and hist["loss"][-1] < hist["loss"][200]
        res = dm.get_results(model.surrogate_posterior)
        obs = res["observed"]
        cc[kind] = (_cc(res["F"][obs], d["f_true"][obs]), _cc(res["I"][obs], d["f_true"][obs] ** 2))
        print(f"{kind}: CC(F, F_true) {cc[kind][0]:.5f}  CC(I, F_true^2) {cc[kind][1]:.5f}  final loss {hist['loss'][-1]:.6g}")
    for kind, (cf, ci) in cc.items():
        assert cf >= 0.99 and ci >= 0.99, (kind, cf, ci)
