"""Empirical reference priors without a device: the oracle's fp64 restatement of them against independent closed forms, the
plugin classes of careless_amd/models/priors/empirical.py held to the reference's own test (tests/models/priors/test_empirical.py:30-47 of
the reference), the C-ABI of `cl_ref_prior` (struct size, entry checks that answer before any launch) and the engine's acceptance rules."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from careless_amd import _lib
from oracle import elbo_oracle as O
from tests import ref_prior as RP

KINDS = RP.KINDS


def _problem(n=64, seed=3):
    rng = np.random.default_rng(seed)
    loc = (0.2 + 2.0 * rng.random(n))
    scale = (0.05 + 0.6 * rng.random(n))
    z = np.abs(loc + scale * rng.normal(size=(3, n))) + 1e-3
    centric = rng.random(n) < 0.4
    return z, loc, scale, centric


# ---- the reference functions ---------------------------------------------------------------------------------------------------------
def test_normal_laplace_studentt_match_torch_distributions():
    z, loc, scale, _ = _problem()
    zt, lt, st = O.f64(z), O.f64(loc), O.f64(scale)
    want = {"normal": torch.distributions.Normal(lt, st), "laplace": torch.distributions.Laplace(lt, st),
            "studentt": torch.distributions.StudentT(torch.tensor(4.0, dtype=torch.float64), lt, st)}
    for kind, dist in want.items():
        got = O.ref_log_prob(kind, zt, lt, st, dof=4.0)
        assert got.dtype == torch.float64 and float((got - dist.log_prob(zt)).abs().max()) < 1e-12, kind


def test_rice_and_folded_normal_match_scipy():
    from scipy import stats
    z, loc, scale, centric = _problem()
    got = O.ref_log_prob("rice_woolfson", z, loc, scale, centric=centric).numpy()
    rice = stats.rice.logpdf(z, loc / scale, scale=scale)
    fold = stats.foldnorm.logpdf(z, loc / scale, scale=scale)
    assert centric.any() and not centric.all()
    assert np.max(np.abs(got - np.where(centric, fold, rice))) < 1e-10
    for all_c, want in ((True, fold), (False, rice)):
        got = O.ref_log_prob("rice_woolfson", z, loc, scale, centric=np.full(len(loc), all_c)).numpy()
        assert np.max(np.abs(got - want)) < 1e-10


@pytest.mark.parametrize("kind", KINDS)
def test_z_derivatives_match_central_differences(kind):
    z, loc, scale, centric = _problem()
    if kind == "laplace":
        assert np.min(np.abs(z - loc)) > 1e-4              # (no sample on the kink: the difference quotient would straddle it)
    zt = O.f64(z).requires_grad_(True)
    lp = O.ref_log_prob(kind, zt, loc, scale, centric=centric, dof=4.0)
    (g,) = torch.autograd.grad(lp.sum(), zt)
    h = 1e-6
    with torch.no_grad():
        fd = (O.ref_log_prob(kind, O.f64(z) + h, loc, scale, centric=centric, dof=4.0) -
              O.ref_log_prob(kind, O.f64(z) - h, loc, scale, centric=centric, dof=4.0)) / (2 * h)
    # central differences in fp64: truncation h^2 f''' / 6 ~ 1e-12 |f'''|, rounding eps |f| / h ~ 1e-10 |f|; |f|, |f'''| reach ~1e3 at scale 0.05
    assert float((g - fd).abs().max()) < 1e-6 * max(1.0, float(g.abs().max())), kind


def test_unobserved_reflections_are_exact_zeros_with_zero_gradient():
    z, loc, scale, centric = _problem()
    observed = np.arange(len(loc)) % 3 != 1
    loc = np.where(observed, loc, np.nan)                   # the parameters of unobserved reflections are never looked at
    for kind in KINDS:
        zt = O.f64(z).requires_grad_(True)
        lp = O.ref_log_prob(kind, zt, loc, scale, observed=observed, centric=centric, dof=4.0)
        (g,) = torch.autograd.grad(lp.sum(), zt)
        assert torch.isfinite(lp).all() and torch.isfinite(g).all()
        assert (lp[:, ~observed] == 0).all() and (g[:, ~observed] == 0).all() and (lp[:, observed] != 0).all()


# ---- the plugin classes ----------------------------------------------------------------------------------------------------------------
def _reference_data(n=100, seed=0):
    rng = np.random.default_rng(seed)
    observed = rng.choice([True, False], n)
    observed[0], observed[1] = True, False
    fobs, sig = rng.random((2, n)).astype(np.float32)
    fobs[~observed] = 1.0
    sig[~observed] = 1.0
    centric = rng.choice([True, False], n)
    centric[np.nonzero(observed)[0][:2]] = [True, False]
    return observed, fobs, sig, centric


def _make(kind, observed, fobs, sig, centric, masked=True):
    from careless_amd.models.priors import empirical as E
    sel = observed if masked else slice(None)
    obs = observed if masked else None
    if kind == "laplace":
        return E.LaplaceReferencePrior(fobs[sel], sig[sel], obs)
    if kind == "normal":
        return E.NormalReferencePrior(fobs[sel], sig[sel], obs)
    if kind == "studentt":
        return E.StudentTReferencePrior(fobs[sel], sig[sel], 4.0, obs)
    return E.RiceWoolfsonReferencePrior(fobs[sel], sig[sel], centric[sel], obs)


@pytest.mark.parametrize("mc_samples", [(), 1, 3], ids=["no_sample_axis", "S1", "S3"])
@pytest.mark.parametrize("kind", KINDS)
def test_plugin_classes_follow_the_reference_test(kind, mc_samples):
    observed, fobs, sig, centric = _reference_data()
    R = len(observed)
    p = _make(kind, observed, fobs, sig, centric)
    assert observed.any() and not observed.all()
    rng = np.random.default_rng(1)
    shape = (() if mc_samples == () else (mc_samples,)) + (R,)
    z = (np.abs(fobs + sig * rng.normal(size=shape)) + 1e-3).astype(np.float32)     # positive: Rice / folded normal support
    lp = p.log_prob(z)
    assert lp.shape == z.shape and lp.dtype == np.float32 and np.all(np.isfinite(lp))
    assert np.all(lp[..., ~observed] == 0.0)
    want = O.ref_log_prob(*RP.prior_arrays(p, R)[:1], z, *RP.prior_arrays(p, R)[1:]).numpy()
    assert np.allclose(lp[..., observed], want[..., observed], atol=1e-5)
    # ... and against the full-length distribution the reference's test builds (Laplace: the float32 SigFobs / sqrt 2)
    scale = (sig / math.sqrt(2.0)).astype(np.float32) if kind == "laplace" else sig
    full = O.ref_log_prob(kind, z, fobs, scale, None, centric, 4.0).numpy()
    assert np.allclose(lp[..., observed], full[..., observed], atol=1e-5)
    # without `observed` every index is evaluated
    q = _make(kind, observed, fobs, sig, centric, masked=False)
    assert np.allclose(q.log_prob(z), full, atol=1e-5)


def test_plugin_class_parameters_and_moments():
    from scipy import stats
    observed, fobs, sig, centric = _reference_data()
    R, n = len(observed), int(observed.sum())
    for kind in KINDS:
        p = _make(kind, observed, fobs, sig, centric)
        assert p.base_dist.loc.dtype == np.float32 and p.base_dist.scale.dtype == np.float32
        assert p.mean().shape == (n,) and p.stddev().shape == (n,)                  # compact: passes through to the base distribution
        assert p.loc_full(R).shape == (R,) and np.array_equal(p.loc_full(R)[observed], fobs[observed])
        assert np.array_equal(p.observed_mask(R), observed.astype(np.uint8))
        assert (p.centric_full(R) is None) == (kind != "rice_woolfson")
    lap = _make("laplace", observed, fobs, sig, centric)
    assert np.array_equal(lap.base_dist.scale, sig[observed] / np.float32(math.sqrt(2.0))) or \
        np.array_equal(lap.base_dist.scale, (sig[observed] / math.sqrt(2.0)).astype(np.float32))
    assert np.allclose(lap.stddev(), sig[observed], rtol=1e-6) and np.array_equal(lap.mean(), fobs[observed])
    nrm = _make("normal", observed, fobs, sig, centric)
    assert np.array_equal(nrm.mean(), fobs[observed]) and np.array_equal(nrm.stddev(), sig[observed])
    from careless_amd.models.priors.empirical import StudentTReferencePrior
    for dof, mean_ok, sd in ((4.0, True, math.sqrt(2.0)), (2.0, True, np.inf), (1.5, True, np.inf), (1.0, False, np.nan), (0.5, False, np.nan)):
        t = StudentTReferencePrior(fobs, sig, dof)
        assert np.array_equal(t.mean(), fobs) if mean_ok else np.isnan(t.mean()).all()
        assert np.isnan(t.stddev()).all() if np.isnan(sd) else np.allclose(t.stddev(), sig * np.float32(sd), rtol=1e-6)
    rw = _make("rice_woolfson", observed, fobs, sig, centric)
    f, s, c = fobs[observed].astype(np.float64), sig[observed].astype(np.float64), centric[observed]
    with np.errstate(invalid="ignore", over="ignore"):       # (scipy's unscaled Rice moments overflow at large Fobs / SigFobs)
        rice_mean, rice_std = stats.rice.mean(f / s, scale=s), stats.rice.std(f / s, scale=s)
    ok = np.isfinite(rice_mean) & np.isfinite(rice_std) & (f / s < 30)
    assert ok[~c].sum() >= 10
    pick = c | ok
    assert np.isfinite(rw.mean()).all() and np.isfinite(rw.stddev()).all()
    assert np.allclose(rw.mean()[pick], np.where(c, stats.foldnorm.mean(f / s, scale=s), rice_mean)[pick], rtol=1e-6)
    assert np.allclose(rw.stddev()[pick], np.where(c, stats.foldnorm.std(f / s, scale=s), rice_std)[pick], rtol=1e-5)
    from careless_amd.models.merging.surrogate_posteriors import RiceWoolfson
    d = RiceWoolfson(fobs, sig, centric)
    x = d.sample(3, seed=2)
    assert x.shape == (3, R) and (x > 0).all() and np.isfinite(d.log_prob(x)).all() and np.allclose(d.prob(x), np.exp(d.log_prob(x)))


def test_bare_reference_prior_has_no_base_distribution():
    from careless_amd.models.priors.empirical import ReferencePrior
    p = ReferencePrior(np.array([True, False, True]))
    assert p.base_dist is None and np.array_equal(p.idx, [0, 2])
    assert ReferencePrior().idx is None


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------------------
PINNED_STRUCTS = ("cl_tn_args", "cl_mlp_args", "cl_adam_args", "cl_laue_args", "cl_det_args")
PARENT_ABI_SIZES = (304, 392, 168, 272, 136)      # ... before cl_ref_prior existed


def pinned_abi_sizes(lib):
    """The library's sizes of PINNED_STRUCTS, asked by name (cl_abi_sizeof)."""
    return tuple(int(lib.cl_abi_sizeof(n.encode())) for n in PINNED_STRUCTS)


def test_abi_sizes():
    lib = _lib.get_lib()
    assert int(lib.cl_abi_sizeof(b"cl_refprior_args")) == C.sizeof(_lib.RefPriorArgs)
    assert pinned_abi_sizes(lib) == PARENT_ABI_SIZES    # the feature added a struct of its own: none of the pinned ones grew
    assert (_lib.CL_PRIOR_WILSON, _lib.CL_PRIOR_DOUBLE_WILSON, _lib.CL_PRIOR_REFERENCE) == (0, 1, 2)


def _accepted():
    """Arguments `cl_ref_prior` would launch with (made-up addresses: the call is never made with them)."""
    p = 0x10000
    return dict(z_f=p, loc=p, scale=p, observed=p, centric=p, kind=_lib.CL_REFPRIOR_NORMAL, dof=0.0, R=300, S=3, w_kl=1.0 / 3, kl_grad_mult=1.0,
                kl_begin=0, kl_end=300, dz_f=p, kl_part=p, scalars=p, stop_flag=p)


def test_ref_prior_entry_checks_answer_without_a_launch():
    """One rejecting call per clause of the entry check; every one returns before the launch (csrc/elbo_q.hip: cl_ref_prior), so the
    made-up pointers are never dereferenced -- whoever reorders that check must keep it ahead of the launch."""
    lib = _lib.get_lib()
    assert lib.cl_ref_prior(None, None) == -1
    ST, RW = _lib.CL_REFPRIOR_STUDENTT, _lib.CL_REFPRIOR_RICE_WOOLFSON
    cases = [dict(z_f=None), dict(loc=None), dict(scale=None), dict(dz_f=None), dict(R=0), dict(R=-5), dict(S=0), dict(S=-1),
             dict(kind=-1), dict(kind=4), dict(kind=ST, dof=0.0), dict(kind=ST, dof=-2.0), dict(kind=ST, dof=float("nan")),
             dict(kind=RW, centric=None), dict(kl_part=None, scalars=None)]
    for over in cases:
        a = _lib.RefPriorArgs(**dict(_accepted(), **over))
        assert lib.cl_ref_prior(C.byref(a), None) == -1, over


# ---- the engine's acceptance rules (host logic) --------------------------------------------------------------------------------------------
def test_engine_accepts_the_four_classes_and_refuses_the_rest():
    from careless_amd import engine
    from careless_amd.models.priors.empirical import ReferencePrior
    from careless_amd.models.priors.wilson import WilsonPrior
    observed, fobs, sig, centric = _reference_data()
    R = len(observed)
    for kind in KINDS:
        for masked in (True, False):
            p = _make(kind, observed, fobs, sig, centric, masked)
            assert engine.prior_kind(p) == _lib.CL_PRIOR_REFERENCE
            arr = engine.reference_prior_arrays(p, R)
            assert arr["kind"] == engine.REFPRIOR_KINDS[kind] and arr["loc"].shape == arr["scale"].shape == (R,)
            assert (arr["observed"] is None) == (not masked) and (arr["centric"] is None) == (kind != "rice_woolfson")
            with pytest.raises(NotImplementedError, match=type(p).__name__):
                engine.prior_kind(p, owner=True)                    # the reflection-owner split stays Wilson-only
            with pytest.raises(ValueError):
                engine.reference_prior_arrays(p, R + 1)
    with pytest.raises(NotImplementedError, match="ReferencePrior"):
        engine.prior_kind(ReferencePrior(observed))
    assert engine.prior_kind(WilsonPrior(centric, np.ones(R), 1.0), owner=True) == _lib.CL_PRIOR_WILSON
    with pytest.raises(NotImplementedError):
        engine.prior_kind(object())
    from careless_amd.models.priors.empirical import NormalReferencePrior, StudentTReferencePrior
    with pytest.raises(ValueError):
        engine.reference_prior_arrays(NormalReferencePrior(fobs[:5], sig[observed], observed), R)     # compact arrays of the wrong length
    with pytest.raises(ValueError):
        engine.reference_prior_arrays(StudentTReferencePrior(fobs, sig, 0.0), R)
