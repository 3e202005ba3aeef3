"""The Laplace likelihood without a GPU: the oracle's fp64 restatement of it and the two plugin classes against torch and scipy, the
reference's own unit tests restated (careless tests/models/likelihoods/test_mono.py:25-36, test_laue.py:38-66), a host build of
csrc/cl_math.h -- cl_lik_laplace_log_prob against fp64, the Normal and Student-T results of the three two-way forms bit for bit against the
expressions they had before --, the constants, the entry checks that need no launch, and the problem construction the GPU tests stand on."""
import ctypes
import math
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch
from scipy import stats

from careless_amd import _lib
from careless_amd.models.base import BaseModel
from careless_amd.models.likelihoods import laue as laue_lik
from careless_amd.models.likelihoods import mono as mono_lik
from oracle import elbo_oracle as O
from tests import ref_laplace as RL
from tests import util

HERE = os.path.dirname(os.path.abspath(__file__))
fp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
SQRT2 = math.sqrt(2.0)


def _inputs(laue, N=300, R=40, seed=3):
    data = O.make_synthetic_laue(N, R=R, n_images=4, seed=seed) if laue else O.make_synthetic(N, R=R, d0=5, n_images=4, seed=seed)
    return data, util.reference_inputs(data)


# ---- density -------------------------------------------------------------------------------------------------------------------------------
def test_reference_density_is_torch_and_scipy_laplace():
    rng = np.random.default_rng(0)
    loc, sig = rng.normal(size=500) * 30, 0.1 + 5 * rng.random(500)
    x = loc + sig * rng.normal(size=(3, 500)) * 2
    got = O.laplace_log_prob(O.f64(x), O.f64(loc), O.f64(sig)).numpy()
    a = torch.distributions.Laplace(O.f64(loc), O.f64(sig) / SQRT2).log_prob(O.f64(x)).numpy()
    b = stats.laplace.logpdf(x, loc=loc, scale=sig / SQRT2)
    assert np.allclose(got, a, rtol=1e-13, atol=1e-13) and np.allclose(got, b, rtol=1e-13, atol=1e-13)
    # the issue's second form
    assert np.allclose(got, -SQRT2 * np.abs(x - loc) / sig - np.log(sig) - 0.5 * math.log(2.0), rtol=1e-13, atol=1e-13)


def test_mono_class_is_the_reference_class():
    """careless tests/models/likelihoods/test_mono.py:25-36, tfd.Laplace taken from torch / scipy"""
    data, inputs = _inputs(False)
    lik = mono_lik.LaplaceLikelihood()
    assert lik.kind == "laplace" and isinstance(lik, mono_lik.LocationScaleLikelihood) and not getattr(lik, "ev11", False)
    bound = lik(inputs)
    iobs, sig = np.squeeze(BaseModel.get_intensities(inputs)), np.squeeze(BaseModel.get_uncertainties(inputs))
    true = torch.distributions.Laplace(torch.as_tensor(iobs, dtype=torch.float64), torch.as_tensor(sig, dtype=torch.float64) / SQRT2)
    torch.manual_seed(0)
    z = true.sample().numpy()
    assert np.allclose(bound.log_prob(z), true.log_prob(torch.as_tensor(z)).numpy())
    assert np.allclose(bound.log_prob(z), stats.laplace.logpdf(z, loc=iobs.astype(np.float64), scale=sig.astype(np.float64) / SQRT2))
    assert np.array_equal(bound.mean(), iobs)
    assert np.allclose(bound.stddev(), sig) and np.allclose(bound.stddev(), true.stddev.numpy())        # sqrt 2 * (sig / sqrt 2), as tfd.Laplace answers
    assert np.allclose(bound.scale, sig / SQRT2)
    # the siblings are as they were
    assert np.array_equal(mono_lik.NormalLikelihood()(inputs).stddev(), sig)


def _fake_ipred(inputs):
    hid = BaseModel.get_harmonic_id(inputs).flatten()
    iobs = BaseModel.get_intensities(inputs).flatten()
    return (iobs[hid] / np.bincount(hid)[hid])[None, :].astype("float32")


def test_laue_class_is_the_reference_class():
    """careless tests/models/likelihoods/test_laue.py:38-66: convolve of iobs[hid] / count[hid] reproduces iobs; a batch of 3 works"""
    data, inputs = _inputs(True)
    lik = laue_lik.LaplaceLikelihood()
    assert lik.kind == "laplace" and isinstance(lik, laue_lik.LaueBase)
    bound = lik(inputs)
    assert isinstance(bound, laue_lik.ConvolvedLikelihood)
    iobs, sig = BaseModel.get_intensities(inputs), BaseModel.get_uncertainties(inputs)
    ipred = _fake_ipred(inputs)
    nobs = int(BaseModel.get_harmonic_id(inputs).max()) + 1
    assert np.allclose(bound.convolve(ipred)[:, :nobs], iobs.T[:, :nobs], rtol=1e-5)
    true = torch.distributions.Laplace(torch.as_tensor(iobs, dtype=torch.float64), torch.as_tensor(sig, dtype=torch.float64) / SQRT2)
    expected = true.log_prob(torch.as_tensor(iobs, dtype=torch.float64)).numpy().T[:, :nobs]
    test = bound.log_prob(ipred)
    assert test.shape == (1, iobs.shape[0])
    assert np.allclose(expected, test[:, :nobs], atol=1e-4)          # (the group sums are fp32 sums of iobs / count: |d| / b of a few 1e-6)
    ipred3 = np.concatenate((ipred, ipred, ipred), axis=0)
    assert bound.convolve(ipred3).shape == ipred3.shape
    test3 = bound.log_prob(ipred3)
    assert test3.shape == (3, iobs.shape[0]) and np.array_equal(test3[0], test[0]) and np.array_equal(test3[2], test[0])
    assert np.array_equal(np.squeeze(bound.mean()), np.squeeze(iobs)) and np.allclose(np.squeeze(bound.stddev()), np.squeeze(sig))


# ---- constants -----------------------------------------------------------------------------------------------------------------------------
def test_the_kind_is_2_in_the_binding_the_header_and_the_device_math():
    assert (_lib.CL_LIK_NORMAL, _lib.CL_LIK_STUDENTT, _lib.CL_LIK_LAPLACE) == (0, 1, 2)
    root = os.path.dirname(HERE)
    header = open(os.path.join(root, "include", "careless_hip.h")).read()
    assert re.search(r"enum \{ CL_LIK_NORMAL_ = 0, CL_LIK_STUDENTT_ = 1, CL_LIK_LAPLACE_ = 2 \};", header)
    math_h = open(os.path.join(root, "careless_amd", "csrc", "cl_math.h")).read()
    assert re.search(r"enum \{ CL_LIK_NORMAL = 0, CL_LIK_STUDENTT = 1, CL_LIK_LAPLACE = 2 \};", math_h)


# ---- host build of cl_math.h -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lm():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tempfile.mkdtemp(prefix="cl_lm_")
    so = os.path.join(d, "liblm.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "laplace_math_check.cpp")])
    lib = ctypes.CDLL(so)
    lib.lm_lik.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_float,
                           ctypes.c_int, ctypes.c_void_p]
    return lib


def _lik(lm, ipred, iobs, sig, kind, dof=0.0, const=0.0, old=0):
    ipred, iobs, sig = (np.ascontiguousarray(a, dtype=np.float32) for a in (ipred, iobs, sig))
    out = np.full((len(ipred), 6), 777.0, np.float32)
    lm.lm_lik(len(ipred), fp(ipred), fp(iobs), fp(sig), kind, dof, const, old, fp(out))
    return out


def _lap(lm, ipred, iobs, sig, hoisted=False):
    ipred, iobs, sig = (np.ascontiguousarray(a, dtype=np.float32) for a in (ipred, iobs, sig))
    out = np.full((len(ipred), 2), 777.0, np.float32)
    (lm.lm_laplace2 if hoisted else lm.lm_laplace)(len(ipred), fp(ipred), fp(iobs), fp(sig), fp(out))
    return out


def _grid(seed=4, n=4000):
    rng = np.random.default_rng(seed)
    iobs = (rng.normal(size=n) * 10 ** rng.uniform(-1, 3, n)).astype(np.float32)
    sig = (10 ** rng.uniform(-2, 2, n)).astype(np.float32)
    ipred = (iobs + sig * rng.normal(size=n) * 10 ** rng.uniform(-3, 1.5, n)).astype(np.float32)
    return ipred, iobs, sig


def test_host_laplace_matches_fp64(lm):
    assert lm.lm_kind_laplace() == 2
    ipred, iobs, sig = _grid()
    d = ipred.astype(np.float64) - iobs.astype(np.float64)
    s = sig.astype(np.float64)
    ll = stats.laplace.logpdf(ipred.astype(np.float64), loc=iobs.astype(np.float64), scale=s / SQRT2)
    dll = -np.sign(d) * SQRT2 / s
    # value: absolute error of a few ulp of its largest term (|d| / b, log sig or the constant)
    nat = SQRT2 * np.abs(d) / s + np.abs(np.log(s)) + 1.0
    for hoisted in (False, True):
        out = _lap(lm, ipred, iobs, sig, hoisted)
        assert np.max(np.abs(out[:, 0] - ll) / nat) < 1e-6, hoisted
        assert np.max(np.abs(out[:, 1] - dll) * s) < 1e-6, hoisted


def test_host_laplace_kink_and_non_finite_inputs(lm):
    one = np.float32(1.0)
    up, down = np.nextafter(one, np.float32(2)), np.nextafter(one, np.float32(0))
    tiny = np.float32(1e-45)
    nan = np.float32(np.nan)
    #                 d = 0    +ulp  -ulp   +denormal -denormal   NaN iobs  NaN sig  sig = 0 (d != 0)  sig = 0 (d = 0)   NaN ipred
    ipred = np.array([1.0,     up,   down,  tiny,     -tiny,      1.0,      1.0,     2.0,              1.0,              nan], np.float32)
    iobs = np.array([1.0,      1.0,  1.0,   0.0,      0.0,        nan,      1.0,     1.0,              1.0,              1.0], np.float32)
    sig = np.array([0.5,       0.5,  0.5,   0.5,      0.5,        0.5,      nan,     0.0,              0.0,              0.5], np.float32)
    c = SQRT2 / 0.5
    for hoisted in (False, True):                  # the unhoisted form and the kernels' hoisted one
        out = _lap(lm, ipred, iobs, sig, hoisted).astype(np.float64)
        ll, dll = out[:, 0], out[:, 1]
        assert dll[0] == 0.0 and abs(ll[0] + math.log(SQRT2 * 0.5)) < 1e-6                     # sign(+-0) = 0, value -log(sqrt2 sig)
        assert abs(dll[1] + c) < 1e-6 and abs(dll[2] - c) < 1e-6                               # one ulp off the kink: the full derivative
        assert abs(dll[3] + c) < 1e-6 and abs(dll[4] - c) < 1e-6                               # ... a denormal residual too
        assert np.isnan(ll[5]) and np.isnan(dll[5])                                            # NaN Iobs: value AND derivative
        assert np.isnan(ll[6]) and np.isnan(dll[6])                                            # NaN SigIobs
        assert np.isnan(ll[7]) and dll[7] == -np.inf                                           # as fp64: -inf - log 0 = NaN; -sign(d) sqrt2 / 0 = -inf
        assert np.isnan(dll[8])                                                                # 0 * inf
        assert np.isnan(ll[9]) and np.isnan(dll[9])
    sgn = np.empty(8, np.float32)
    dd = np.array([0.0, -0.0, 3.0, -3.0, np.inf, -np.inf, tiny, nan], np.float32)
    lm.lm_sign(8, fp(dd), fp(sgn))
    assert np.array_equal(sgn[:7], np.array([0.0, -0.0, 1.0, -1.0, 1.0, -1.0, 1.0], np.float32)) and np.signbit(sgn[1]) and np.isnan(sgn[7])


@pytest.mark.parametrize("kind,dof", [(0, 0.0), (1, 4.0), (1, 16.0)])
def test_host_normal_and_studentt_are_bit_identical_to_the_two_way_forms(lm, kind, dof):
    ipred, iobs, sig = _grid(seed=5)
    nan = np.float32(np.nan)
    ipred = np.concatenate([ipred, [1.0, 1.0, nan, 1.0]]).astype(np.float32)
    iobs = np.concatenate([iobs, [1.0, nan, 1.0, 1.0]]).astype(np.float32)
    sig = np.concatenate([sig, [0.0, 1.0, 1.0, nan]]).astype(np.float32)
    const = math.lgamma(0.5 * (dof + 1.0)) - math.lgamma(0.5 * dof) - 0.5 * math.log(dof * math.pi) if kind == 1 else 0.0
    new = _lik(lm, ipred, iobs, sig, kind, dof, const, old=0)
    old = _lik(lm, ipred, iobs, sig, kind, dof, const, old=1)
    assert np.array_equal(new.view(np.uint32), old.view(np.uint32))


# ---- the problem construction of the GPU tests ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(N=300, R=30, d0=5, L=20, w=10, S=1, perturb=0.02), dict(N=300, R=40, L=2, w=32, S=3, laue=True),
                                dict(N=384, R=48, d0=5, L=2, w=32, S=2)], ids=["20x10_S1", "laue_2x32_S3", "2x32_S2"])
def test_rewritten_observations_put_the_kink_inside_the_data(kw):
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    ipred, ipl = RL.predictions(data, cfg, params, u_f, eta)
    G = RL.counted_slots(data)
    before = np.mean(ipl[:, :G] - np.asarray(data["iobs"], dtype=np.float64)[None, :G] > 0)
    new, rounds = RL.rewrite_observations(data, cfg, params, [(u_f, eta)], seed=kw.get("seed", 7))
    gap, pos = RL.assert_conditions(new, ipred, ipl)
    print(f"positive residuals before {before:.2f} after {pos:.2f}; {rounds} nudging rounds, smallest gap {gap:.2f} guards")
    assert rounds <= 10
    if cfg.laue:                # the (1.0, 1.0) padding stays as generated
        assert np.array_equal(new["iobs"][G:], data["iobs"][G:]) and np.array_equal(new["sigiobs"][G:], data["sigiobs"][G:]) and G < len(new["iobs"])
    # the step under the Laplace likelihood differs from the Normal step, and its data gradient is finite
    xn = O.inputs_from_numpy(new)
    out, grads = O.elbo_value_and_grads(params, xn, RL.under(cfg), O.f64(u_f), O.f64(eta))
    on, _ = O.elbo_value_and_grads(params, xn, cfg, O.f64(u_f), O.f64(eta))
    assert abs(float(out["nll"]) - float(on["nll"])) > 1e-2 * abs(float(on["nll"]))
    assert abs(float(out["kl"]) - float(on["kl"])) == 0.0 and all(torch.isfinite(g).all() for g in grads)
    # ... and is the hand-written derivative: d nll / d ipred_l = w sign(d) sqrt2 / sig
    S = cfg.mc_samples
    ipl_t = torch.as_tensor(ipl).requires_grad_(True)
    (g,) = torch.autograd.grad(-O.laplace_log_prob(ipl_t, xn.iobs[None, :], xn.sigiobs[None, :]).sum() / S, ipl_t)
    d = ipl - new["iobs"].astype(np.float64)[None, :]
    assert np.allclose(g.numpy(), np.sign(d) * SQRT2 / new["sigiobs"].astype(np.float64)[None, :] / S, rtol=1e-12)


# ---- entry checks without a launch -----------------------------------------------------------------------------------------------------
def test_launch_entry_refuses_unknown_kinds_and_laplace_beside_the_evans_buffers():
    """cl_mlp_check runs the checks of cl_elbo_mono_fwd_bwd and launches nothing: no device needed.  (The entries that can only be told
    apart from a NULL-pointer error on real buffers -- cl_laue_likelihood, cl_slot_rows -- are in tests/test_laplace_gpu.py.)"""
    lib = _lib.get_lib()
    proto = dict(refl_id=1, meta_t=1, iobs=1, sig=1, mlp=1, z_f=1, dz_f=1, partials=1, scalars=1, stop_flag=1, n_obs=256, n_pad=256, d=5, w=32, L=2,
                 S=2, R=10)
    check = lambda **f: int(lib.cl_mlp_check(ctypes.byref(_lib.MlpArgs(**dict(proto, **f))), 0, 4))
    assert [check(lik_kind=k) for k in (_lib.CL_LIK_NORMAL, _lib.CL_LIK_STUDENTT, _lib.CL_LIK_LAPLACE)] == [0, 0, 0]
    assert [check(lik_kind=k) for k in (3, 7, -1)] == [-1, -1, -1]                     # (was: ran as Student-T)
    for ev in (dict(ev11=1), dict(d_ev11=1), dict(ev11_part=1), dict(ev11=1, d_ev11=1)):
        assert check(lik_kind=_lib.CL_LIK_LAPLACE, **ev) == -1, ev
    assert check(lik_kind=_lib.CL_LIK_NORMAL, ev11=1, d_ev11=1) == 0 and check(lik_kind=_lib.CL_LIK_STUDENTT, dof=4.0, ev11=1, d_ev11=1) == 0
    # the epilogue query still answers for a kind the launch refuses (tests/test_epilogue_plain.py); Laplace keeps the generic epilogue
    full = dict(proto, w=64, L=5, S=8)
    assert len({_lib.mlp_route(lib, 0, **dict(full, lik_kind=k)) for k in (0, 1, 2)}) == 1
    assert _lib.mlp_epilogue(lib, 0, **dict(full, lik_kind=_lib.CL_LIK_NORMAL)) == _lib.CL_EPI_PLAIN_NORMAL
    assert _lib.mlp_epilogue(lib, 0, **dict(full, lik_kind=_lib.CL_LIK_LAPLACE)) == _lib.CL_EPI_GENERIC
    assert _lib.mlp_epilogue(lib, 0, **dict(full, lik_kind=7)) == _lib.CL_EPI_GENERIC


def test_laplace_changes_the_plan_only_where_the_lane_or_narrow_kernel_would_run():
    """The one documented routing exception: no Laplace instance of the lane / narrow kernel -- their shapes run on
    elbo_mlp.hip, unpeeled, a chain without a lane block; every other plan is the Normal one."""
    from careless_amd.engine import plan_scaler
    lib = _lib.get_lib()
    lane_family = (_lib.CL_ROUTE_LANE, _lib.CL_ROUTE_LANE_IMGL, _lib.CL_ROUTE_NARROW)
    fell = 0
    for d, w, L, K in ((5, 10, 20, 0), (5, 13, 20, 0), (37, 10, 20, 0), (5, 10, 20, 2), (5, 10, 24, 0), (5, 64, 5, 0), (6, 32, 2, 0), (5, 16, 10, 0),
                       (5, 64, 12, 0), (5, 32, 2, 1), (5, 96, 3, 0)):
        pn, pl = plan_scaler(lib, d, w, L, K), plan_scaler(lib, d, w, L, K, lik_kind=_lib.CL_LIK_LAPLACE)
        assert pl.route not in lane_family and not pl.chain_lane and pl.wide == pn.wide, (d, w, L, K, pl)
        if pn.route in lane_family or pn.chain_lane:
            fell += 1
            assert not pl.peel and pl.route in (_lib.CL_ROUTE_MLP, _lib.CL_ROUTE_MLP_IMGL, _lib.CL_ROUTE_MLP_CHAIN), (d, w, L, K, pl)
        else:
            assert pl == pn, (d, w, L, K, pn, pl)
    assert fell == 5
