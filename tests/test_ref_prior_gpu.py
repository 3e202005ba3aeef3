"""Empirical reference priors on the GPU: `cl_ref_prior` (csrc/elbo_q.hip: ref_prior_kernel) called directly, one launch per case, on
operands carved from one guarded allocation, and whole training steps of the engine under the four prior classes, both against the fp64
oracle (`O.ref_log_prob`; whole steps under `ElboConfig.prior = "reference"` with the arrays of tests/ref_prior.py in `ElboInputs.ref`).

Tolerances are the project's own: an fp32 gradient tensor within 2e-4 of its max-norm, a loss term within 1e-4 relative
(denominator max(|kl|, 1) for the KL), `RTOL_LOSS` / `RTOL_GRAD` of tests/test_gpu_parity.py with its LeakyReLU branch gate.

Shape -> grid of the direct calls, from the launcher: `dim3((R + 255) / 256), dim3(256)`, one thread per reflection and a loop over S:
R = 1 one thread, 255 a ragged single workgroup, 257 a second workgroup with one thread at work, 600 three."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from careless_amd import _lib
from oracle import elbo_oracle as O
from tests import ref_prior as RP
from tests import ref_step
from tests import test_gpu_parity as P
from tests import util

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda"
KIND_ID = {"normal": _lib.CL_REFPRIOR_NORMAL, "laplace": _lib.CL_REFPRIOR_LAPLACE, "studentt": _lib.CL_REFPRIOR_STUDENTT,
           "rice_woolfson": _lib.CL_REFPRIOR_RICE_WOOLFSON}
KL_BEFORE = 3.5               # what scalars[CL_SC_KL] holds before a call without kl_part: the kernel ADDS
SENT = -7.25e30               # what every kl_part slot holds before the call: the kernel STORES


# ---- direct calls ----------------------------------------------------------------------------------------------------------------------
def direct_inputs(kind, R, S, seed=0):
    """z, loc, scale in the densities' bulk: loc in [0.5, 1.5], scale in [0.1, 0.4] (Rice argument z loc / scale^2 <= ~250), samples
    within a few scales of loc and positive; dz_f preloaded with O(1) values (its fp32 rounding, 6e-8, is far below 2e-4 of the increment's
    max-norm, which is >= ~1 / scale for every kind)."""
    rng = np.random.default_rng(1000 * seed + 10 * R + S)
    loc = (0.5 + rng.random(R)).astype(np.float32)
    scale = (0.1 + 0.3 * rng.random(R)).astype(np.float32)
    z = (np.abs(loc[:, None] + 1.5 * scale[:, None] * rng.normal(size=(R, S))) + 0.02).astype(np.float32)      # [R][S]
    centric = (rng.random(R) < 0.4).astype(np.uint8)
    pre = rng.normal(size=(R, S)).astype(np.float32)
    return z, loc, scale, centric, pre


def masks(R, which, rng_seed=5):
    rng = np.random.default_rng(rng_seed + R)
    observed = {"none": None, "mixed": (rng.random(R) < 0.6).astype(np.uint8), "all_zero": np.zeros(R, np.uint8)}[which]
    if which == "mixed" and R > 1:
        observed[0], observed[R - 1] = 1, 0
    return observed


def ranges(R):
    return {"whole": (0, R), "middle": (R // 3, R - R // 4), "empty": (R // 2, R // 2)}


# the first seed of `direct_inputs` per (R, S) at which no Laplace sample lies within 2e-4 loc of loc (found on the CPU; the test asserts it)
LAPLACE_SEED = {(255, 1): 1, (255, 8): 5, (257, 3): 2, (600, 1): 2, (600, 8): 5}


def run_direct(kind, R, S, obs_kind, rng_kind, with_part, stop=False):
    lib = _lib.get_lib()
    seed = LAPLACE_SEED.get((R, S), 0)
    z, loc, scale, centric, pre = direct_inputs(kind, R, S, seed)
    if kind == "laplace":
        # no sample on the kink of |z - loc| (the derivative jumps there; a sample within rounding of loc may take either side)
        assert np.min(np.abs(z - loc[:, None]) / loc[:, None]) > 1e-4, (R, S, seed)
    observed = masks(R, obs_kind)
    k0, k1 = ranges(R)[rng_kind]
    w_kl, mult, dof = 1.0 / S, (0.5 if S == 3 else 1.0), 4.0
    active = np.ones(R, bool) if observed is None else observed.astype(bool)
    active &= (np.arange(R) >= k0) & (np.arange(R) < k1)
    nblk = (R + 255) // 256
    a = ref_step.Guarded(DEV).add("z_f", z).add("loc", loc).add("scale", scale).add("dz_f", pre, np.repeat(active[:, None], S, axis=1))
    if observed is not None:
        a.add("observed", observed)
    if kind == "rice_woolfson":
        a.add("centric", centric)
    if with_part:
        a.add("kl_part", np.full(nblk + 3, SENT), [True] * nblk + [False] * 3)
    a.add("scalars", np.array([1.25, KL_BEFORE, 7.0, 6.0]), [False, not with_part, False, False])
    a.add("stop", np.array([1 if stop else 0], np.int32)).build()
    A = _lib.RefPriorArgs()
    A.z_f, A.loc, A.scale, A.dz_f = a.ptr("z_f"), a.ptr("loc"), a.ptr("scale"), a.ptr("dz_f")
    A.observed = a.ptr("observed") if observed is not None else None
    A.centric = a.ptr("centric") if kind == "rice_woolfson" else None
    A.kind, A.dof, A.R, A.S = KIND_ID[kind], dof, R, S
    A.w_kl, A.kl_grad_mult, A.kl_begin, A.kl_end = w_kl, mult, k0, k1
    A.kl_part = a.ptr("kl_part") if with_part else None
    A.scalars, A.stop_flag = a.ptr("scalars"), a.ptr("stop")
    code = int(lib.cl_ref_prior(C.byref(A), None))
    torch.cuda.synchronize()
    assert code == 0
    a.verify(untouched=stop)            # guards, inputs, dz_f of unobserved / out-of-range reflections, the other scalars: bit-identical
    if stop:
        return
    what = (kind, R, S, obs_kind, rng_kind, with_part)
    # fp64 reference: [S][R] orientation
    zt = O.f64(z.T).requires_grad_(True)
    lp = O.ref_log_prob(kind, zt, loc, scale, None if observed is None else observed.astype(bool), centric.astype(bool), dof)
    lp = lp * O.f64(active.astype(np.float64))
    (dlp,) = torch.autograd.grad(lp.sum(), zt)
    inc_ref = (-np.float64(np.float32(w_kl)) * mult * dlp.numpy()).T
    kl_ref = -np.float64(np.float32(w_kl)) * float(lp.detach().sum())
    inc = a.get("dz_f").astype(np.float64) - pre.astype(np.float64)
    assert np.all(inc[~active] == 0.0), what
    if active.any():
        den = np.max(np.abs(inc_ref))
        err = np.max(np.abs(inc - inc_ref)) / den
        print(f"{what}: increment error / max-norm {err:.2e} (max-norm {den:.3g})")
        assert err < 2e-4, (what, err)
    if with_part:
        part = a.get("kl_part")[:nblk]
        assert a.changed("kl_part")[:nblk].all(), (what, "a kl_part slot was not written")
        kl = float(np.sum(part))
    else:
        kl = float(a.get("scalars")[_lib.CL_SC_KL]) - KL_BEFORE
    print(f"{what}: kl {kl:.9g} reference {kl_ref:.9g}")
    assert abs(kl - kl_ref) <= 1e-4 * max(abs(kl_ref), 1.0), (what, kl, kl_ref)
    if not active.any():
        assert kl == 0.0, what


@pytest.mark.parametrize("R", [1, 255, 257, 600])
@pytest.mark.parametrize("kind", RP.KINDS)
def test_direct_calls_match_fp64(kind, R):
    """every S, observed mask, KL range and KL route of the issue's grid at this (kind, R): 54 launches, one per case"""
    for S, obs_kind, rng_kind, with_part in itertools.product((1, 3, 8), ("none", "mixed", "all_zero"), ("whole", "middle", "empty"), (True, False)):
        run_direct(kind, R, S, obs_kind, rng_kind, with_part)


@pytest.mark.parametrize("kind", RP.KINDS)
def test_direct_call_with_a_raised_stop_flag_writes_nothing(kind):
    for with_part in (True, False):
        run_direct(kind, 600, 3, "mixed", "whole", with_part, stop=True)


# ---- whole steps -------------------------------------------------------------------------------------------------------------------------
def make_prior(kind, data, params, masked, seed=3, nan_at=None):
    """A reference data set near where q sits (Fobs within ~10 % of q's location, SigFobs 15 .. 45 % of it), full length, and the prior
    class of `kind` built from its compact form when `masked`."""
    from careless_amd.models.priors import empirical as E
    R = params.q_loc_raw.numel()
    rng = np.random.default_rng(seed)
    fobs = (np.exp(params.q_loc_raw.numpy()) * (1.0 + 0.1 * rng.normal(size=R))).clip(0.05, None).astype(np.float32)
    sig = (fobs * (0.15 + 0.3 * rng.random(R))).astype(np.float32)
    observed = None
    if masked:
        observed = rng.random(R) < 0.6
        observed[0], observed[1] = True, False
    if nan_at is not None:
        assert observed is None or observed[nan_at]
        sig[nan_at] = np.nan
    sel = slice(None) if observed is None else observed
    centric = np.asarray(data["centric"], dtype=bool)
    if kind == "normal":
        return E.NormalReferencePrior(fobs[sel], sig[sel], observed)
    if kind == "laplace":
        return E.LaplaceReferencePrior(fobs[sel], sig[sel], observed)
    if kind == "studentt":
        return E.StudentTReferencePrior(fobs[sel], sig[sel], 4.0, observed)
    return E.RiceWoolfsonReferencePrior(fobs[sel], sig[sel], centric[sel], observed)


def assert_grads(g_hip, grads, prob, prior, name):
    """tests/test_gpu_parity.py's gate (`_assert_grads`: every tensor at RTOL_GRAD, a LeakyReLU pre-activation within fp32 rounding of zero
    may sit on the engine's branch) with this module's reference behind it."""
    errs = [util.rel_err(a, b.numpy()) for a, b in zip(g_hip, grads)]
    assert len(g_hip) == len(grads)
    if max(errs) < P.RTOL_GRAD:
        return
    data, cfg, params, u_f, eta = prob
    x = O.inputs_from_numpy(data)
    near = []
    O.elbo_value_and_grads(params, *RP.under(x, cfg, prior), O.f64(u_f), O.f64(eta), near=near)
    near.sort()
    cand = [(l, r, u) for _, l, r, u in near[:P.MAX_FLIP_CANDIDATES]]
    assert cand, f"{name}: gradient errors {errs} and no LeakyReLU pre-activation within fp32 rounding of zero: not a branch flip"
    for k in range(1, len(cand) + 1):
        for sub in itertools.combinations(cand, k):
            _, gf = O.elbo_value_and_grads(params, *RP.under(x, cfg, prior), O.f64(u_f), O.f64(eta), flips=sub)
            if max(util.rel_err(a, b.numpy()) for a, b in zip(g_hip, gf)) < P.RTOL_GRAD:
                print(f"{name}: gradients match with the LeakyReLU unit(s) {list(sub)} on the engine's branch")
                return
    raise AssertionError(f"{name}: gradient errors {errs}; no forced-branch assignment of {cand} brings them under {P.RTOL_GRAD}")


def assert_terms(terms, out, name):
    for k in ("nll", "kl", "loss"):
        den = max(abs(float(out[k])), 1.0) if k == "kl" else abs(float(out[k]))
        print(f"{name}: {k} engine {terms[k]:.9g} reference {float(out[k]):.9g}")
        assert abs(terms[k] - float(out[k])) <= P.RTOL_LOSS * den, (name, k, terms, float(out[k]))


STEP_CASES = {
    "normal_all_observed_2x32_S3": ("normal", False, dict(N=300, R=40, d0=5, L=2, w=32, S=3)),
    "laplace_masked_studentt_likelihood_klweight": ("laplace", True, dict(N=400, R=50, d0=5, L=2, w=32, S=2, likelihood="studentt", dof=6.0, kl_weight=0.5)),
    "studentt_dof4_laue_single_pass": ("studentt", True, dict(N=400, R=40, L=2, w=32, S=3, laue=True)),
    "rice_woolfson_masked_cli_default_20x10": ("rice_woolfson", True, dict(N=500, R=50, d0=5, L=20, w=10, S=2, perturb=0.02)),
    "normal_masked_ev11": ("normal", True, dict(N=400, R=40, d0=5, L=2, w=32, S=3, ev11=True)),
    "laplace_all_observed_wide_2x96": ("laplace", False, dict(N=400, R=40, d0=5, L=2, w=96, S=2)),
    "rice_woolfson_chained_12x32": ("rice_woolfson", True, dict(N=400, R=40, d0=5, L=12, w=32, S=2)),
    "studentt_laue_two_pass": ("studentt", False, dict(N=400, R=40, L=2, w=32, S=2, laue=True, two_pass=True)),
}


def build(kind, masked, kw, nan_at=None, **attrs):
    kw = dict(kw)
    two_pass = kw.pop("two_pass", False)
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    prior = make_prior(kind, data, params, masked, nan_at=nan_at)

    def fresh():
        m = util.build_model(data, cfg, params, kw["L"], kw["w"])
        m.prior = prior
        m.laue_two_pass = two_pass
        for k, v in attrs.items():
            setattr(m, k, v)
        return m
    return fresh, prior, (data, cfg, params, u_f, eta), x, util.reference_inputs(data)


def check_laplace_kink(kind, out, prior):
    if kind != "laplace":
        return
    z = out["z_f"].numpy()
    loc = prior.loc_full(z.shape[1]).astype(np.float64)
    assert np.min(np.abs(z - loc) / loc) > 1e-4          # the case's own samples: none on the kink


@pytest.mark.parametrize("name", list(STEP_CASES))
def test_whole_step_matches_the_fp64_reference(name):
    kind, masked, kw = STEP_CASES[name]
    fresh, prior, prob, x, inputs = build(kind, masked, kw)
    data, cfg, params, u_f, eta = prob
    out, grads = O.elbo_value_and_grads(params, *RP.under(x, cfg, prior), O.f64(u_f), O.f64(eta))
    check_laplace_kink(kind, out, prior)
    model = fresh()
    ipred = model(inputs, u_f=u_f, eta=eta)
    eng = model._engine
    torch.cuda.synchronize()
    assert eng.ref_prior and eng.ref["kind"] == KIND_ID[kind]
    assert_terms(eng.loss_terms(), out, name)
    assert util.rel_err(ipred.cpu().numpy(), out["ipred"].numpy()) < 1e-4
    assert_grads([g.cpu().numpy() for g in eng.grad_tensors()], grads, prob, prior, name)
    # the prior matters: the same step under the Wilson prior has another KL (the comparison above is not vacuous)
    assert abs(float(out["kl"]) - float(O.elbo_value_and_grads(params, x, cfg, O.f64(u_f), O.f64(eta))[0]["kl"])) > 1e-2


def test_deterministic_mode_matches_and_repeats_bit_for_bit():
    from careless_amd.engine import ElboEngine
    kind, masked, kw = "rice_woolfson", True, dict(N=900, R=50, d0=5, L=5, w=64, S=3)
    fresh, prior, prob, x, inputs = build(kind, masked, kw, deterministic=True)
    data, cfg, params, u_f, eta = prob
    out, grads = O.elbo_value_and_grads(params, *RP.under(x, cfg, prior), O.f64(u_f), O.f64(eta))
    model = fresh()
    model(inputs, u_f=u_f, eta=eta)
    eng = model._engine
    torch.cuda.synchronize()
    assert eng.deterministic and eng.ref_prior and "deterministic" in eng.kernel_name()
    assert_terms(eng.loss_terms(), out, "deterministic")
    assert_grads([g.cpu().numpy() for g in eng.grad_tensors()], grads, prob, prior, "deterministic")
    runs = []
    for _ in range(2):
        e = ElboEngine(fresh(), inputs, seed=5)
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
    assert np.all(np.isfinite(h0["loss"])) and len(h0["loss"]) == 4


@pytest.mark.parametrize("kw", [dict(N=2000, R=60, d0=5, L=20, w=10, S=3, perturb=0.02), dict(N=900, R=60, L=2, w=32, S=2, laue=True)],
                         ids=["mono_20x10", "laue_2x32"])
def test_frozen_scaler_step_equals_the_fused_step(kw):
    """`cl_frozen_rows` STORES dz_f: the prior's term must be added behind it.  Same in-kernel noise on both engines."""
    from careless_amd.engine import ElboEngine
    engs = {}
    for fast in (True, False):
        fresh, prior, prob, x, inputs = build("normal", True, kw, frozen_scaler_fast_path=fast)
        m = fresh()
        m.scaling_model.trainable = False
        engs[fast] = ElboEngine(m, inputs, seed=31)
        engs[fast].forward_backward(4)
    torch.cuda.synchronize()
    fast, full = engs[True], engs[False]
    assert fast.scaler_frozen and fast._frozen_layout and not full._frozen_layout and fast.ref_prior
    assert getattr(fast.obs, "frozen_sorted", None) is not None
    tf, tu = fast.loss_terms(), full.loss_terms()
    print("frozen / fused kl", tf["kl"], tu["kl"])
    assert abs(tf["kl"] - tu["kl"]) <= P.RTOL_LOSS * max(abs(tu["kl"]), 1.0)
    R = fast.R
    gf, gu = fast.grads[: 2 * R].cpu().numpy(), full.grads[: 2 * R].cpu().numpy()
    print("frozen / fused q gradient", util.rel_err(gf[:R], gu[:R]), util.rel_err(gf[R:], gu[R:]))
    assert util.rel_err(gf[:R], gu[:R]) < P.RTOL_GRAD and util.rel_err(gf[R:], gu[R:]) < P.RTOL_GRAD
    observed = fast.ref["observed"].cpu().numpy().astype(bool)
    assert observed.any() and not observed.all()


def test_two_row_split_shards_sum_to_the_one_rank_step():
    from careless_amd.engine import ElboEngine, make_shard
    kw = dict(N=600, R=50, d0=5, L=2, w=32, S=2)
    fresh, prior, prob, x, inputs = build("studentt", True, kw)
    full = ElboEngine(fresh(), inputs, seed=99)
    full.forward_backward(3)
    torch.cuda.synchronize()
    g_full, t_full = full.grads.clone(), full.loss_terms()
    g_sum, nll, kl = torch.zeros_like(g_full), 0.0, 0.0
    for r in range(2):
        eng = ElboEngine(fresh(), inputs, seed=99, shard=make_shard(kw["N"], kw["R"], r, 2))
        assert not eng.owner and eng.ref_prior and 0 < eng.shard.kl_end - eng.shard.kl_begin < kw["R"]
        eng.local_only = True
        eng.forward_backward(3)
        torch.cuda.synchronize()
        g_sum += eng.grads
        t = eng.loss_terms()
        nll += t["nll"]; kl += t["kl"]
    assert abs(nll - t_full["nll"]) <= 1e-5 * abs(t_full["nll"]) and abs(kl - t_full["kl"]) <= 1e-5 * max(abs(t_full["kl"]), 1.0)
    assert util.rel_err(g_sum.cpu().numpy(), g_full.cpu().numpy()) < 2e-5
    m = fresh()
    m.owner_shard = True
    with pytest.raises(NotImplementedError, match="StudentTReferencePrior"):
        ElboEngine(m, inputs, seed=99, shard=make_shard(kw["N"], kw["R"], 0, 2))


def test_adam_trajectory_matches_the_reference_loop():
    kw = dict(N=384, R=48, d0=5, L=2, w=32, S=2)
    fresh, prior, prob, x, inputs = build("rice_woolfson", True, kw)
    data, cfg, params, _, _ = prob
    steps = 5
    rng = np.random.default_rng(11)
    noises = [(rng.random((2, 48)).astype(np.float32), rng.normal(size=(2, 384)).astype(np.float32)) for _ in range(steps)]
    model = fresh()
    hist = model.train_model(inputs, steps, progress=False, noise=lambda i: noises[i])
    p = params.clone()
    st = O.AdamState.zeros_like(p.tensors())
    ref = [O.train_step(p, *RP.under(x, cfg, prior), st, O.f64(u), O.f64(e)) for u, e in noises]
    for k in ("loss", "NLL", "F KLDiv", "Grad Norm"):
        a, b = np.array(hist[k]), np.array([r[k] for r in ref])
        assert len(a) == steps and np.max(np.abs(a - b) / np.maximum(np.abs(b), 1.0)) < 2e-4, (k, a, b)
    got = [t.cpu().numpy() for t in model._engine.param_tensors()]
    for a, b in zip(got, p.tensors()):
        assert util.rel_err(a, b.numpy()) < 2e-4


def test_nan_in_the_reference_data_follows_the_non_finite_step_contract():
    """tests/test_nonfinite.py's contract with the poison in the PRIOR: one observed reflection has SigFobs = NaN.  The non-finite mask of the
    gradient is the fp64 reference's -- that reflection's a and b entries and nothing else --, the norm is non-finite, the step is applied
    with those entries zeroed, the following steps are skipped."""
    kw = dict(N=300, R=40, d0=5, L=2, w=32, S=3)
    h = 7
    fresh, prior, prob, x, inputs = build("normal", False, kw, nan_at=h)
    data, cfg, params, u_f, eta = prob
    out, grads = O.elbo_value_and_grads(params, *RP.under(x, cfg, prior), O.f64(u_f), O.f64(eta))
    grads = [g.numpy() for g in grads]
    for k, g in enumerate(grads):                        # the reference's mask is sharp
        bad = ~np.isfinite(g)
        assert (bad.sum() == 1 and bad[h]) if k < 2 else not bad.any(), k
    assert not np.isfinite(float(out["kl"])) and not np.isfinite(float(out["loss"])) and np.isfinite(float(out["nll"]))
    model = fresh()
    model(inputs, u_f=u_f, eta=eta)
    eng = model._engine
    torch.cuda.synchronize()
    g_hip = [g.cpu().numpy() for g in eng.grad_tensors()]
    zeroed = lambda a: np.where(np.isfinite(a), a, 0.0)
    for k, (a, b) in enumerate(zip(g_hip, grads)):
        assert np.array_equal(np.isfinite(a), np.isfinite(b)), (k, np.argwhere(np.isfinite(a) != np.isfinite(b))[:4].tolist())
        assert util.rel_err(zeroed(a), zeroed(b)) < P.RTOL_GRAD, k
    terms = eng.loss_terms()
    assert not np.isfinite(terms["kl"]) and not np.isfinite(terms["loss"])
    assert abs(terms["nll"] - float(out["nll"])) <= P.RTOL_LOSS * abs(float(out["nll"]))
    # four steps asked for, one applied
    p = params.clone()
    rec = O.train_step(p, *RP.under(x, cfg, prior), O.AdamState.zeros_like(p.tensors()), O.f64(u_f), O.f64(eta))
    model = fresh()
    hist = model.train_model(inputs, 4, progress=False, noise=lambda i: (u_f, eta))
    assert len(hist["loss"]) == 1 and not np.isfinite(hist["Grad Norm"][0]) and not np.isfinite(rec["Grad Norm"])
    for a, b in zip([t.cpu().numpy() for t in model._engine.param_tensors()], p.tensors()):
        assert np.isfinite(a).all() and np.isfinite(b.numpy()).all() and util.rel_err(a, b.numpy()) < 2e-4
