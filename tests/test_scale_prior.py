"""The scale prior ("Σ KLDiv": reference careless/models/merging/variational.py:156-163), CPU part: the plugin classes, what the engine refuses,
the route decision, the library's surface and argument checks, and the fp64 reference of tests/ref_scale_prior.py checked by something
other than itself (a closed form, a Monte-Carlo bound derived from the sample's own variance, central finite differences).  The GPU part
is tests/test_scale_prior_gpu.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from careless_amd import _lib
from careless_amd.models.priors.scale import LaplaceScalePrior, NormalScalePrior, ScalePrior, StudentTScalePrior
from careless_amd.plan import Route, check_scale_prior, check_scale_prior_route, data_term_route, plan_scaler
from careless_amd.sprior import SCALE_KL_KEY, scale_kl_form
from oracle import elbo_oracle as O
from tests import ref_scale_prior as RS
from tests import util

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the plugin classes ----------------------------------------------------------------------------------------------------------------
def test_plugin_classes_log_prob_against_scipy():
    from scipy import stats
    x = np.linspace(-7.0, 9.0, 41)
    for prior, dist in ((NormalScalePrior(0.7, 1.9), stats.norm(0.7, 1.9)), (LaplaceScalePrior(-0.4, 0.6), stats.laplace(-0.4, 0.6)),
                        (StudentTScalePrior(3.5, 1.2, 0.8), stats.t(3.5, 1.2, 0.8))):
        want = dist.logpdf(x)
        got = prior.log_prob(x)
        assert got.dtype == np.float64 and np.allclose(got, want, rtol=1e-12, atol=1e-12), type(prior).__name__
        t = prior.log_prob(torch.as_tensor(x, dtype=torch.float32))            # host tensors
        assert torch.is_tensor(t) and np.allclose(t.numpy(), want, rtol=1e-6, atol=1e-6)
        assert isinstance(prior, ScalePrior) and prior.engine_kind in ("normal", "laplace", "studentt")
    assert (NormalScalePrior(0, 1).engine_kind, LaplaceScalePrior(0, 1).engine_kind, StudentTScalePrior(4, 0, 1).engine_kind) == ("normal", "laplace", "studentt")
    assert StudentTScalePrior(4, 0, 1).df == 4.0
    for bad in (lambda: NormalScalePrior(0.0, 0.0), lambda: LaplaceScalePrior(0.0, -1.0), lambda: StudentTScalePrior(0.0, 0.0, 1.0),
                lambda: NormalScalePrior(float("nan"), 1.0)):
        with pytest.raises(ValueError):
            bad()


def test_reference_prior_log_prob_is_the_plugin_classes():
    z = O.f64(np.linspace(-3.0, 4.0, 29))
    for prior, spec in ((NormalScalePrior(0.7, 1.9), ("normal", 0.7, 1.9)), (LaplaceScalePrior(-0.4, 0.6), ("laplace", -0.4, 0.6)),
                        (StudentTScalePrior(3.5, 1.2, 0.8), ("studentt", 3.5, 1.2, 0.8))):
        assert np.allclose(RS.prior_log_prob(spec, z).numpy(), prior.log_prob(z).numpy(), rtol=1e-13, atol=1e-13)


# ---- what the engine refuses -----------------------------------------------------------------------------------------------------------
def test_scale_kl_weight_none_is_the_references_type_error():
    assert check_scale_prior(None, None) is None and check_scale_prior(None, 1.0) is None
    with pytest.raises(TypeError, match=r"variational\.py:160-161"):
        check_scale_prior(NormalScalePrior(1.0, 1.0), None)
    p = LaplaceScalePrior(1.0, 2.0)
    # only that the weight is not None is read: any value gives the same prior back
    assert check_scale_prior(p, 1.0) is p and check_scale_prior(p, 0.0) is p and check_scale_prior(p, 123.0) is p


def test_the_three_refusals():
    class Exponential:
        def log_prob(self, x):
            return -x
    for bad in (Exponential(), "normal", torch.distributions.Normal(0.0, 1.0)):
        with pytest.raises(NotImplementedError, match="NormalScalePrior, LaplaceScalePrior or StudentTScalePrior"):
            check_scale_prior(bad, 1.0)
    with pytest.raises(NotImplementedError, match="layer-by-layer"):
        check_scale_prior_route(wide=True, owner=False)
    with pytest.raises(NotImplementedError, match="reflection-owner"):
        check_scale_prior_route(wide=False, owner=True)
    check_scale_prior_route(wide=False, owner=False)
    # deterministic mode: monochromatic rows without per-image layers, a sample count that divides 64 (cl_slot_rows' store form)
    check_scale_prior_route(False, False, deterministic=True, S=4)
    for over in (dict(laue=True), dict(imgl=True), dict(S=3)):
        with pytest.raises(NotImplementedError, match="deterministic mode covers"):
            check_scale_prior_route(False, False, deterministic=True, **over)


def test_engine_construction_raises_before_anything_touches_a_device():
    """`ElboEngine` asks `check_scale_prior` while it reads the plugin objects: the model class stores what it is given."""
    data, cfg, params, x, u_f, eta = util.make_problem(N=50, R=10, S=1)
    model = util.build_model(data, cfg, params, 2, 32)
    assert model.scale_prior is None and model.scale_kl_weight is None
    from careless_amd.models.merging.variational import VariationalMergingModel
    m = VariationalMergingModel(model.surrogate_posterior, model.prior, model.likelihood, model.scaling_model, 1, None, None, NormalScalePrior(1.0, 1.0))
    with pytest.raises(TypeError, match="scale_kl_weight=None"):
        check_scale_prior(m.scale_prior, m.scale_kl_weight)


# ---- the route -------------------------------------------------------------------------------------------------------------------------
def test_a_mono_engine_with_the_flag_takes_the_two_pass_route():
    # without the flag: today's answers, positionally and by keyword
    assert data_term_route(None, False, False, False, False, False) is Route.FUSED
    assert data_term_route(None, False, False, False, False, True) is Route.PEEL
    assert data_term_route(None, False, False, True, False, False) is Route.TWO_PASS
    assert data_term_route(None, False, False, False, False, False, scale_prior=False) is Route.FUSED
    # with it: monochromatic rows take the two-pass launches, also where the plan says peel; frozen, wide and chain keep their precedence
    assert data_term_route(None, False, False, False, False, False, scale_prior=True) is Route.TWO_PASS
    assert data_term_route(None, False, False, False, False, True, scale_prior=True) is Route.TWO_PASS
    assert data_term_route(None, False, True, False, False, False, scale_prior=True) is Route.CHAIN
    assert data_term_route(None, True, False, False, False, False, scale_prior=True) is Route.WIDE
    assert data_term_route(object(), False, False, False, False, False, scale_prior=True) is Route.FROZEN


@pytest.mark.parametrize("d,w,L", [(5, 32, 2), (5, 10, 20), (5, 10, 10), (21, 64, 5), (5, 16, 2)])
def test_plan_scaler_answers_the_two_pass_launches_for_a_mono_engine_with_the_flag(d, w, L):
    lib = _lib.get_lib()
    plain = plan_scaler(lib, d, w, L)
    assert plain == plan_scaler(lib, d, w, L, scale_prior=False)              # unchanged without the flag
    flagged = plan_scaler(lib, d, w, L, scale_prior=True)
    assert not flagged.wide and flagged.blocks is None
    # the plan's route is the backward launch's (mode 2, dL/d(loc, sigma) in), as for two-pass Laue data
    proto = dict(d=d, w=w, L=L, S=1, refl_id=1, meta_t=1, iobs=1, sig=1, mlp=1, z_f=1, dz_f=1, partials=1, scalars=1, stop_flag=1)
    assert flagged.route == _lib.mlp_route(lib, 2, **proto, dO_ext=1) != _lib.CL_ROUTE_NONE
    assert flagged.route == plan_scaler(lib, d, w, L, laue=True, two_pass=True).route
    assert _lib.mlp_route(lib, 1, **proto, loc_out=1, sig_out=1) != _lib.CL_ROUTE_NONE


def test_a_chained_scaler_with_the_flag_keeps_its_last_block_off_the_lane_kernel():
    lib = _lib.get_lib()
    plain, flagged = plan_scaler(lib, 5, 10, 24), plan_scaler(lib, 5, 10, 24, scale_prior=True)
    assert plain.blocks is not None and plain.chain_lane
    assert flagged.blocks is not None and not flagged.chain_lane             # (the lane kernel is a full step: no room for the term)
    deep32 = plan_scaler(lib, 5, 32, 12, scale_prior=True)
    assert deep32.blocks is not None and len(deep32.blocks) == 2 and not deep32.wide
    assert plan_scaler(lib, 5, 96, 3, scale_prior=True).wide                    # ... which the engine then refuses


def test_form_follows_from_the_scale_distribution():
    A, S_ = _lib.CL_SPRIOR_ANALYTIC, _lib.CL_SPRIOR_SAMPLE
    assert scale_kl_form("normal", False, False) == A
    assert scale_kl_form("normal", True, False) == S_ and scale_kl_form("normal", False, True) == S_
    assert scale_kl_form("laplace", False, False) == S_ and scale_kl_form("studentt", False, False) == S_
    assert SCALE_KL_KEY == "Σ KLDiv"


# ---- the library's surface -------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("cl_scale_kl", "cl_scale_kl_grid", "cl_scale_kl_record")


def test_new_symbols_are_exported_and_declared():
    lib = _lib.get_lib()
    with open(os.path.join(os.path.dirname(HERE), "include", "careless_hip.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and getattr(lib, name) is not None and name + "(" in header, name
    assert "typedef struct cl_sprior_args" in header and "variational.py:156-163" in header and ":123-139" in header
    assert int(lib.cl_abi_sizeof(b"cl_sprior_args")) == C.sizeof(_lib.SpriorArgs) > 0
    assert _lib.ABI_STRUCTS["cl_sprior_args"] is _lib.SpriorArgs
    from careless_amd import build
    assert any(u[0] == "elbo_sprior.hip" and "-fno-honor-nans" not in u[2] for u in build.UNITS)
    assert _lib.CL_HIST_SCALE_KL == 5 < _lib.CL_HIST_STRIDE == 8              # the sixth double of a record; stride and layout unchanged
    assert [int(lib.cl_scale_kl_grid(n)) for n in (0, 1, 256, 257, 10 ** 7)] == [0, 1, 1, 2, _lib.CL_LAUE_LIK_MAX_BLOCKS]


def _args(**over):
    """Arguments every clause of the entry check accepts (addresses that are never read: a rejected call does not touch the device)."""
    a = _lib.SpriorArgs()
    a.loc, a.sigma, a.dO, a.kl_part, a.value = 1024, 2048, 4096, 8192, 1 << 14
    a.image_id, a.img, a.d_img, a.use_img = 1 << 15, 1 << 16, 1 << 17, 1
    a.kind, a.p_loc, a.p_scale, a.p_df = _lib.CL_SPRIOR_STUDENTT, 0.5, 1.5, 4.0
    a.form, a.n, a.S, a.weight = _lib.CL_SPRIOR_SAMPLE, 100, 3, 0.01
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_entry_check_rejects_one_clause_at_a_time():
    fn = _lib.get_lib().cl_scale_kl
    N_, L_, T_ = _lib.CL_SPRIOR_NORMAL, _lib.CL_SPRIOR_LAPLACE, _lib.CL_SPRIOR_STUDENTT
    AN = _lib.CL_SPRIOR_ANALYTIC
    assert fn(None, None) == -1
    for field in ("loc", "sigma", "dO", "kl_part", "value"):
        assert fn(C.byref(_args(**{field: None})), None) == -1, field
    assert fn(C.byref(_args(n=0)), None) == -1
    assert fn(C.byref(_args(S=0)), None) == -1                                  # the sample form
    for over in (dict(kind=3), dict(kind=-1), dict(form=2), dict(form=-1), dict(p_scale=0.0), dict(p_scale=-1.0), dict(p_scale=float("nan")),
                 dict(p_df=0.0), dict(p_df=-2.0)):
        assert fn(C.byref(_args(**over)), None) == -1, over
    for field in ("image_id", "img", "d_img"):                                  # image scales without their arrays
        assert fn(C.byref(_args(**{field: None})), None) == -1, field
    # -2: the analytic form is the registered Normal || Normal KL of a bare Normal alone
    for kind in (L_, T_):
        assert fn(C.byref(_args(form=AN, kind=kind, use_img=0)), None) == -2, kind
    assert fn(C.byref(_args(form=AN, kind=N_, use_img=0, has_shift=1)), None) == -2
    assert fn(C.byref(_args(form=AN, kind=N_, use_img=1)), None) == -2
    # (-1 before -2: a bad parameter of a non-Normal prior asked in the analytic form)
    assert fn(C.byref(_args(form=AN, kind=T_, p_df=0.0, use_img=0)), None) == -1
    rec = _lib.get_lib().cl_scale_kl_record
    assert rec(None, 1024, 0, None) == -1 and rec(1024, None, 0, None) == -1 and rec(1024, 2048, -1, None) == -1


# ---- the reference, checked by something other than itself -----------------------------------------------------------------------------
def test_analytic_form_is_torch_distributions_kl_divergence():
    rng = np.random.default_rng(3)
    loc, sigma = O.f64(rng.normal(1.0, 0.5, 200)), O.f64(rng.uniform(0.05, 2.0, 200))
    for m, s in ((0.0, 1.0), (1.3, 0.4), (-2.0, 5.0)):
        want = torch.distributions.kl_divergence(torch.distributions.Normal(loc, sigma), torch.distributions.Normal(O.f64(m), O.f64(s)))
        assert torch.allclose(RS.analytic_kl(loc, sigma, m, s), want, rtol=1e-13, atol=1e-13)


def test_sample_form_agrees_with_the_analytic_form_within_five_standard_errors():
    """A bare Normal scale distribution against a Normal prior: the sample form's mean over S = 4096 draws of N = 64 rows estimates the
    analytic value; the bound is five standard errors of that sample mean, taken from the sample's own variance."""
    S, N = 4096, 64
    rng = np.random.default_rng(11)
    loc, sigma = O.f64(rng.normal(1.0, 0.3, N)), O.f64(rng.uniform(0.1, 0.8, N))
    eta = O.f64(rng.normal(size=(S, N)))
    prior = ("normal", 0.8, 0.6)
    kl, _ = RS.sample_kl(loc, sigma, eta, prior)
    per_draw = kl.mean(dim=1)                           # S independent estimates of (1/N) sum_i KL_i
    est, se = float(per_draw.mean()), float(per_draw.std(unbiased=True)) / math.sqrt(S)
    want = float(RS.analytic_kl(loc, sigma, 0.8, 0.6).mean())
    assert se > 0.0 and abs(est - want) <= 5.0 * se, (est, want, se)


def _branches(p, x, cfg):
    """The LeakyReLU branch of every hidden unit of every row (the loss has a kink where one changes)."""
    h, out = x.metadata, []
    for w, b in zip(p.mlp_w[:-1], p.mlp_b[:-1]):
        z = h @ w + b
        out.append(z > 0)
        h = torch.where(z > 0, z, cfg.leakiness * z)
    return torch.cat([t.reshape(-1) for t in out])


def _directional_fd(fun, ts, grads, rng, loss):
    for k, t in enumerate(ts):
        v = O.f64(rng.normal(size=tuple(t.shape)))
        h = 1e-6 * max(float(t.abs().max()), 1e-2)
        fd = (fun(k, h * v) - fun(k, -h * v)) / (2 * h)           # (`fun` holds both evaluations to the base point's LeakyReLU branches)
        an = float((grads[k] * v).sum())
        # (central differences: truncation ~ h^2, rounding ~ eps64 |loss| / h)
        assert abs(fd - an) <= 1e-5 * abs(an) + 1e-13 * abs(loss) / h, (k, fd, an)


@pytest.mark.parametrize("prior", [("laplace", 0.31, 0.9), ("studentt", 3.0, 1.1, 0.7)], ids=["laplace", "studentt"])
def test_reference_gradient_matches_finite_differences_with_shift_and_image_scales(prior):
    data, cfg, params, x, u_f, eta = util.make_problem(N=120, R=20, S=2, bijector="softplus", shift=1.5, seed=6)
    assert cfg.use_image_scales and not RS.is_analytic(prior, cfg)
    u64, e64 = O.f64(u_f), O.f64(eta)
    out, grads = RS.value_and_grads(params, x, cfg, u64, e64, prior)
    if prior[0] == "laplace":                           # no sample at the kink, nor within the finite-difference step of it
        assert float((out["z_scale"] - prior[1]).abs().min()) > 1e-3 * prior[2]
    assert abs(float(out["scale_kl"])) > 1e-3 and np.isfinite(float(out["loss"]))

    base = _branches(params, x, cfg)

    def fun(k, dv):
        q = params.clone()
        q.tensors()[k].add_(dv)
        # a condition of the draw, not a skip: no hidden unit changes its LeakyReLU branch inside the difference step (the kink is the
        # oracle's, not the term's; the seed is the first one that meets it)
        assert torch.equal(_branches(q, x, cfg), base), k
        return float(RS.forward(q, x, cfg, u64, e64, prior)["loss"])
    ts = params.tensors()
    _directional_fd(fun, ts, grads, np.random.default_rng(1), float(out["loss"]))
    # the term reaches the scaler and the image scales, not q
    _, g_plain = O.elbo_value_and_grads(params, x, cfg, u64, e64)
    assert torch.equal(grads[0], g_plain[0]) and torch.equal(grads[1], g_plain[1])
    n_mlp = 2 * len(params.mlp_w)
    assert util.rel_err(grads[2 + n_mlp].numpy(), g_plain[2 + n_mlp].numpy()) > 1e-6       # image scales
    assert util.rel_err(grads[2].numpy(), g_plain[2].numpy()) > 1e-6


def test_reference_shards_add_up_and_kl_weight_leaves_the_term_alone():
    data, cfg, params, x, u_f, eta = util.make_problem(N=90, R=15, S=3, seed=4)
    prior = ("studentt", 4.0, 1.0, 0.5)
    e64 = O.f64(eta)
    whole = RS.scale_kl(params, x, cfg, e64, prior)["value"]
    a = RS.scale_kl(params, x, cfg, e64, prior, rows=torch.arange(0, 40))["value"]
    b = RS.scale_kl(params, x, cfg, e64, prior, rows=torch.arange(40, 90))["value"]
    assert abs(float(a + b - whole)) <= 1e-14 * abs(float(whole))
    data, cfg2, params2, x2, _, _ = util.make_problem(N=90, R=15, S=3, seed=4, kl_weight=0.25)
    assert float(RS.scale_kl(params2, x2, cfg2, e64, prior)["value"]) == float(whole)
    out = RS.forward(params2, x2, cfg2, O.f64(u_f), e64, prior)
    assert abs(float(out["loss"]) - (float(out["nll"]) + 0.25 * float(out["kl"]) + float(whole))) <= 1e-13 * abs(float(out["loss"]))


# ---- the history's column across ranks -------------------------------------------------------------------------------------------------
def _history_worker(rank, world, port, q):
    import torch.distributed as dist
    from careless_amd.distributed import allreduce_history_
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    stride = _lib.CL_HIST_STRIDE
    h = torch.zeros(3, stride, dtype=torch.float64)
    for i in range(3):              # this rank's shares of KL, NLL and Σ KLDiv; the loss column holds the rank's own partial sum
        h[i, 1], h[i, 2], h[i, 5] = 0.25 * (rank + 1) * (i + 1), 10.0 * (rank + 1) + i, 0.125 * (rank + 2) * (i + 1)
        h[i, 0] = h[i, 2] + 0.5 * h[i, 1] + h[i, 5]
    h[1, 4], h[1, 0], h[1, 5] = 1.0, 0.0, 0.0         # a skipped step
    plain = h.clone()
    allreduce_history_(h.view(-1), stride, 0.5, scale_kl=True)
    allreduce_history_(plain.view(-1), stride, 0.5)
    if rank == 0:
        q.put((h.numpy(), plain.numpy()))
    dist.barrier()
    dist.destroy_process_group()


def test_allreduce_history_carries_the_term_across_ranks():
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_history_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    h, plain = q.get(timeout=180)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for i in (0, 2):
        kl, nll, skl = 0.25 * 3 * (i + 1), 30.0 + 2 * i, 0.125 * 5 * (i + 1)
        assert (h[i, 1], h[i, 2], h[i, 5]) == (kl, nll, skl) and h[i, 0] == nll + 0.5 * kl + skl
        # without the flag: today's arithmetic, the sixth double is left alone
        assert plain[i, 0] == nll + 0.5 * kl and plain[i, 5] == 0.125 * 2 * (i + 1)
    assert h[1, 0] == 0.0 and h[1, 4] == 1.0 and h[1, 5] == 0.0
