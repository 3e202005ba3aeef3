"""The neural likelihood on the GPU: cl_nlik_forward / cl_nlik_backward called directly on injected predictions against fp64, whole
training steps of the engine against the fp64 oracle under its neural likelihood
(`ElboConfig.likelihood = "neural"`, the network in `ElboParams.nlik`), the frozen scaler, NLL_val, a shard cut into pieces, an Adam trajectory, the non-finite step contract
and finite differences of the engine's own loss.

The whole-step cases are the monochromatic rows without Ev11 of tests/test_nonfinite.py's MATRIX (its keyword dictionaries, routes and
kernel-name fragments) with `likelihood` / `dof` dropped and `model.likelihood = NeuralNormalLikelihood(L, w)`; the Laue and Ev11 rows
assert the refusal.  The likelihood does not change the routing.  Networks come from `ref_nlik.pick_net`: every case asserts on the fp64
reference that no LeakyReLU unit of the likelihood's network is within `ref_nlik.KINK_REL` of its kink (relative to its layer's largest
pre-activation), so the fp32 engine's branches are the reference's.

Tolerances are the project's own: `RTOL_LOSS` / `RTOL_GRAD` of tests/test_gpu_parity.py, tensor-level max-norm, with its LeakyReLU branch
gate for the SCALER's units."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from careless_amd import _lib
from oracle import elbo_oracle as O
from tests import ref_nlik as RN
from tests import test_gpu_parity as P
from tests import test_nonfinite as NF
from tests import util

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


# ---- (a) the kernels called directly ------------------------------------------------------------------------------------------------------------
# (N, (L, w), S, pos map, w_ll as 1 / (S N) -- the kl_weight form): every N, every network shape and every S of the issue at least once
KERNEL_CASES = [(1, (1, 1), 1, False, False), (37, (4, 32), 3, True, False), (64, (2, 16), 8, False, False), (65, (3, 32), 1, True, False),
                (300, (2, 17), 3, True, True), (1000, (1, 5), 8, False, False), (1000, (2, 16), 3, True, True), (300, (3, 32), 3, False, False),
                (65, (1, 1), 8, True, False), (37, (2, 17), 1, False, True)]


def _kernel_problem(N, L, w, S, seed=0):
    rng = np.random.default_rng(100 + seed + N)
    iobs = (rng.gamma(1.0, 400.0, size=N) + 2.0).astype(np.float32)
    sig = (5.0 + 0.05 * iobs * rng.uniform(0.5, 1.5, size=N)).astype(np.float32)
    ipred = (iobs[:, None] + 1.5 * sig[:, None] * rng.normal(size=(N, S))).astype(np.float32)
    net, _ = RN.pick_net(L, w, iobs, sig, first_seed=seed)
    net = [O.f64(t.to(torch.float32)) for t in net]                         # the fp32 values the kernels read
    return iobs, sig, ipred, net


class _Launch:
    """Device buffers of one forward + backward call on the library; outputs prefilled with `fill`."""

    def __init__(self, iobs, sig, ipred, net, L, w, w_ll, pos=None, image_len=0, stop=0, fill=0.0):
        lib = _lib.get_lib()
        N, S = ipred.shape
        self.lib, self.N = lib, N
        self.iobs, self.sig, self.ipred, self.net = _dev(iobs), _dev(sig), _dev(ipred), _dev(RN.flat_of(net))
        assert self.net.numel() == int(lib.cl_nlik_param_count(L, w))
        nbytes = int(lib.cl_nlik_workspace_bytes(N, L, w))
        self.ws = torch.full(((nbytes + 3) // 4,), fill, dtype=torch.float32, device="cuda")
        self.sigpred = torch.full((N,), fill, dtype=torch.float32, device="cuda")
        self.d_net = torch.full((self.net.numel(),), fill, dtype=torch.float32, device="cuda")
        self.pos = None if pos is None else _dev(pos, torch.int32)
        self.image = None if pos is None else torch.ones(image_len, dtype=torch.float32, device="cuda")
        self.stop = torch.full((1,), stop, dtype=torch.int32, device="cuda")
        a = self.args = _lib.NlikArgs()
        a.iobs, a.sigiobs, a.net, a.L, a.w, a.leak, a.n = self.iobs.data_ptr(), self.sig.data_ptr(), self.net.data_ptr(), L, w, 0.3, N
        a.sigpred, a.workspace, a.ipred, a.S, a.w_ll, a.d_net = self.sigpred.data_ptr(), self.ws.data_ptr(), self.ipred.data_ptr(), S, w_ll, self.d_net.data_ptr()
        a.pos, a.sig_image = _lib.ptr(self.pos), _lib.ptr(self.image)
        a.stop_flag = self.stop.data_ptr()

    def run(self):
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(self.lib.cl_nlik_forward(C.byref(self.args), st), "cl_nlik_forward")
        _lib.check(self.lib.cl_nlik_backward(C.byref(self.args), st), "cl_nlik_backward")
        torch.cuda.synchronize()
        return self

    @property
    def delta(self):
        return self.ws[: self.N]


def _split_net(flat, L, w):
    from careless_amd.models.likelihoods.mono import lik_dense_slices
    return [t for ow, o, i, ob in lik_dense_slices(L, w) for t in (flat[ow:ow + o * i].reshape(o, i).T, flat[ob:ob + o])]


@pytest.mark.parametrize("N,shape,S,with_pos,klw", KERNEL_CASES, ids=[f"N{c[0]}_{c[1][0]}x{c[1][1]}_S{c[2]}{'_pos' if c[3] else ''}{'_klw' if c[4] else ''}" for c in KERNEL_CASES])
def test_kernels_match_fp64_and_repeat_bit_for_bit(N, shape, S, with_pos, klw):
    L, w = shape
    iobs, sig, ipred, net = _kernel_problem(N, L, w, S)
    w_ll = 1.0 / (S * N) if klw else 1.0 / S
    delta, sigpred, grads, kink = RN.kernel_reference(net, iobs, sig, ipred, w_ll)
    assert kink > RN.KINK_REL and float(delta.min()) > 4e-5
    pos = image_len = None
    if with_pos:
        image_len = N + 13
        pos = np.random.default_rng(N).permutation(image_len)[:N].astype(np.int32)             # permutes and pads
    runs = [_Launch(iobs, sig, ipred, net, L, w, w_ll, pos, image_len).run() for _ in range(2)]
    a, b = runs
    for name in ("sigpred", "d_net", "delta") + (("image",) if with_pos else ()):
        assert torch.equal(getattr(a, name), getattr(b, name)), name                              # no atomics: bit-identical
    e_d, e_s = util.rel_err(a.delta.cpu().numpy(), delta.numpy()), util.rel_err(a.sigpred.cpu().numpy(), sigpred.numpy())
    errs = [util.rel_err(g, r.numpy()) for g, r in zip(_split_net(a.d_net.cpu().numpy(), L, w), grads)]
    print(f"N {N} {L}x{w} S {S}: delta {e_d:.1e} sigpred {e_s:.1e} gradient tensors {['%.1e' % e for e in errs]}")
    assert e_d < P.RTOL_GRAD and e_s < P.RTOL_GRAD
    if N == 1:
        # a lone row: sigpred = sigiobs whatever the network says, so the gradient is exactly zero (the reference's is fp64 rounding noise).
        # fp32: dL/ddelta = (g sigiobs - T) / m with the two terms equal to rounding, |.| <= 4 eps32 |g sigiobs| / m, times dz / dtheta,
        # at most (1 + |iobs| + |sigiobs|) (1 + max|weight|) for one unit
        gs = w_ll * float(np.sum(1.0 + ((ipred[0] - iobs[0]) / sig[0]) ** 2))               # >= |g sigiobs|
        bound = 4 * 2.0 ** -23 * gs / float(delta[0]) * (1 + float(iobs[0]) + float(sig[0])) * (1 + max(float(t.abs().max()) for t in net))
        assert float(a.d_net.abs().max()) <= bound, (float(a.d_net.abs().max()), bound)
    else:
        assert max(errs) < P.RTOL_GRAD
    if with_pos:
        img = a.image.cpu().numpy()
        assert np.array_equal(img[pos], a.sigpred.cpu().numpy())
        pad = np.ones(image_len, dtype=bool)
        pad[pos] = False
        assert pad.sum() == 13 and np.all(img[pad] == 1.0)                                       # padding is never written


def test_kernels_write_nothing_when_the_stop_flag_is_set():
    L, w, N, S = 2, 16, 300, 3
    iobs, sig, ipred, net = _kernel_problem(N, L, w, S)
    pos = np.arange(N, dtype=np.int32)[::-1].copy()
    r = _Launch(iobs, sig, ipred, net, L, w, 1.0 / S, pos, N, stop=1, fill=-7.0).run()
    assert bool((r.sigpred == -7.0).all()) and bool((r.d_net == -7.0).all()) and bool((r.ws == -7.0).all()) and bool((r.image == 1.0).all())


# ---- the problem of a matrix row under the neural likelihood ------------------------------------------------------------------------------------
def _is_refused(case):
    return bool(case.kw.get("laue") or case.kw.get("ev11"))


STEP_ROWS = [n for n in NF.MATRIX if not _is_refused(NF.MATRIX[n])]
REFUSED_ROWS = [n for n in NF.MATRIX if _is_refused(NF.MATRIX[n])]
# the network of a row: 2 x 8 unless named here (the widest instance, the 16-wide one and one layer)
NET_SHAPE = {"mlp64_5x64_posenc_studentt_S8": (3, 32), "lane_20x10_d5_S1": (2, 16), "narrow_20x13": (1, 5), "wide_3x96": (4, 32), "klweight_4x48": (2, 17),
             "det_mlp_5x64": (3, 32), "frozen_mono_20x10": (2, 16)}


def problem(name, poison=None, where="inner", keep_lik=False):
    """tests/test_nonfinite.py's `_problem` with the likelihood keys dropped.  Returns (case, kw, opts, data, cfg, params, u_f, eta, net):
    `net` the likelihood's network as Keras-ordered fp64 tensors holding fp32 values, picked on the CLEAN data."""
    case = NF.MATRIX[name]
    kw = dict(case.kw, seed=case.seed)
    if not keep_lik:
        for k in ("likelihood", "dof"):
            kw.pop(k, None)
    opts = {k: kw.pop(k, None) for k in ("two_pass", "regroup", "shuffle_rows", "grid")}
    assert not opts["shuffle_rows"]
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    if opts["regroup"]:
        data = P._regroup_laue(data, opts["regroup"])
    data = dict(data)
    L, w = NET_SHAPE.get(name, (2, 8))
    net = None
    if not _is_refused(case):
        net, _ = RN.pick_net(L, w, data["iobs"], data["sigiobs"], first_seed=case.seed)
        net = [O.f64(t.to(torch.float32)) for t in net]
    if poison is not None:
        row = NF._pick_row(data, where)
        column, value = NF.POISONS[poison]
        a = np.array(data[column], dtype=np.float32, copy=True)
        a[row] = value
        data[column] = a
    return case, kw, opts, data, cfg, params, u_f, eta, net


def neural_model(case, kw, opts, data, cfg, params, net, **attrs):
    from careless_amd.models.likelihoods import NeuralNormalLikelihood
    model = NF._model(case, kw, opts, data, cfg, params)
    lik = NeuralNormalLikelihood(len(net) // 2 - 1, net[0].shape[1])
    lik.set_weights([t.numpy() for t in net])
    model.likelihood = lik
    for k, v in attrs.items():
        setattr(model, k, v)
    return model


def assert_terms(terms, out, name):
    for k in ("nll", "kl", "loss"):
        den = max(abs(float(out[k])), 1.0) if k == "kl" else abs(float(out[k]))
        print(f"{name}: {k} engine {terms[k]:.9g} reference {float(out[k]):.9g}")
        assert abs(terms[k] - float(out[k])) <= P.RTOL_LOSS * den, (name, k, terms, float(out[k]))


def assert_grads(g_hip, grads, prob, name, order=lambda g: g):
    """tests/test_gpu_parity.py's gate (every tensor at RTOL_GRAD; a LeakyReLU pre-activation of the SCALER within fp32 rounding of zero may
    sit on the engine's branch), as tests/test_laplace_gpu.py rebuilds it, with tests/ref_nlik.py behind it."""
    errs = [util.rel_err(a, b.numpy()) for a, b in zip(g_hip, grads)]
    print(f"{name}: gradient errors {['%.1e' % e for e in errs]}")
    if max(errs) < P.RTOL_GRAD:
        return
    data, cfg, params, u_f, eta, net = prob
    x = O.inputs_from_numpy(data)
    near = []
    O.elbo_value_and_grads(RN.with_net(params, net), x, RN.under(cfg), O.f64(u_f), O.f64(eta), near=near)
    near.sort()
    cand = [(l, r, u) for _, l, r, u in near[:P.MAX_FLIP_CANDIDATES]]
    assert cand, f"{name}: gradient errors {errs} and no LeakyReLU pre-activation of the scaler within fp32 rounding of zero: not a branch flip"
    for k in range(1, len(cand) + 1):
        for sub in itertools.combinations(cand, k):
            _, gf = O.elbo_value_and_grads(RN.with_net(params, net), x, RN.under(cfg), O.f64(u_f), O.f64(eta), flips=sub)
            if max(util.rel_err(a, b.numpy()) for a, b in zip(g_hip, order(gf))) < P.RTOL_GRAD:
                print(f"{name}: gradients match with the scaler's LeakyReLU unit(s) {list(sub)} on the engine's branch")
                return
    raise AssertionError(f"{name}: gradient errors {errs}; no forced-branch assignment of {cand} brings them under {P.RTOL_GRAD}")


# ---- (b) whole steps ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STEP_ROWS)
def test_whole_step_matches_the_fp64_reference(name):
    case, kw, opts, data, cfg, params, u_f, eta, net = problem(name)
    x = O.inputs_from_numpy(data)
    out, grads = O.elbo_value_and_grads(RN.with_net(params, net), x, RN.under(cfg), O.f64(u_f), O.f64(eta))
    assert out["kink"] > RN.KINK_REL and float(out["delta"].min()) > 4e-5, (out["kink"], float(out["delta"].min()))
    model = neural_model(case, kw, opts, data, cfg, params, net)
    inputs = util.reference_inputs(data)
    eng = model.engine(inputs)
    assert eng.neural and eng.lik_kind == _lib.CL_LIK_NORMAL
    NF._assert_route(eng, case)
    ipred = model(inputs, u_f=u_f, eta=eta)
    torch.cuda.synchronize()
    assert util.rel_err(ipred.cpu().numpy(), out["ipred"].numpy()) < 1e-4
    sp = eng.obs.nlik.sigpred[: eng.obs.nlik.n].cpu().numpy()
    if getattr(eng.obs, "perm", None) is not None:          # (the wide path's image-sorted layout keeps its rows, eta and ipred in that order)
        back = np.empty_like(sp)
        back[np.asarray(eng.obs.perm)] = sp
        sp = back
    print(f"{name}: sigpred {util.rel_err(sp, out['sigpred'].numpy()):.1e}, kink {out['kink']:.1e}")
    assert util.rel_err(sp, out["sigpred"].numpy()) < P.RTOL_GRAD
    assert_terms(eng.loss_terms(), out, name)
    order = list                     # (`ElboParams.tensors()` is in the engine's order: the likelihood's group in front of the double-Wilson r)
    g_hip = [g.cpu().numpy() for g in eng.grad_tensors()]
    g_ref = order(grads)
    assert len(g_hip) == len(g_ref) and [a.shape for a in g_hip] == [tuple(b.shape) for b in g_ref]
    if case.frozen:                  # the scaler's gradient is not computed: q's two tensors and the network's are compared
        keep = [0, 1] + list(range(len(g_hip) - len(net), len(g_hip)))
        assert all(float(np.abs(g_hip[k]).max()) == 0.0 for k in range(2, len(g_hip) - len(net)))
        g_hip, g_ref, pick = [g_hip[k] for k in keep], [g_ref[k] for k in keep], (lambda g: [order(g)[k] for k in keep])
    else:
        pick = order
    assert all(float(np.abs(g).max()) > 0.0 for g in g_hip[-len(net):])
    assert_grads(g_hip, g_ref, (data, cfg, params, u_f, eta, net), name, pick)
    # the likelihood matters: the same step under the plain Normal likelihood has another NLL
    nll_n = float(O.elbo_value_and_grads(params, x, cfg, O.f64(u_f), O.f64(eta))[0]["nll"])
    assert abs(float(out["nll"]) - nll_n) > 1e-2 * abs(nll_n)


@pytest.mark.parametrize("name", REFUSED_ROWS)
def test_laue_and_ev11_rows_are_refused(name):
    from careless_amd.models.likelihoods import NeuralNormalLikelihood
    case, kw, opts, data, cfg, params, u_f, eta, _ = problem(name, keep_lik=True)
    model = NF._model(case, kw, opts, data, cfg, params)
    lik = NeuralNormalLikelihood(2, 8)
    if cfg.ev11 and not cfg.laue:
        lik.ev11 = True              # the Evans-2011 error model beside the network: no such class in the reference
    model.likelihood = lik
    with pytest.raises(NotImplementedError, match="monochromatic only" if cfg.laue else "Evans-2011"):
        model.engine(util.reference_inputs(data))


def test_unsupported_network_is_refused_at_construction():
    from careless_amd.models.likelihoods import NeuralNormalLikelihood
    case, kw, opts, data, cfg, params, *_ = problem("mlp32_2x32")
    model = NF._model(case, kw, opts, data, cfg, params)
    model.likelihood = NeuralNormalLikelihood(2, 33)
    with pytest.raises(NotImplementedError, match=r"1 \.\. 4 hidden layers of width 1 \.\. 32"):
        model.engine(util.reference_inputs(data))


# ---- (c) frozen scaler -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["sorted_rows", "slots"])
def test_frozen_scaler_trains_the_network_and_repeats_bit_for_bit(form):
    from careless_amd.engine import ElboEngine
    from careless_amd.frozen import FrozenForm
    name = "frozen_mono_20x10"
    case, kw, opts, data, cfg, params, u_f, eta, net = problem(name)
    x = O.inputs_from_numpy(data)
    out, grads = O.elbo_value_and_grads(RN.with_net(params, net), x, RN.under(cfg), O.f64(u_f), O.f64(eta))
    assert out["kink"] > RN.KINK_REL
    inputs = util.reference_inputs(data)
    n = len(net)

    def fresh():
        e = ElboEngine(neural_model(case, kw, opts, data, cfg, params, net), inputs, seed=31)
        e.FROZEN_SORTED_ROWS = form == "sorted_rows"
        return e
    eng = fresh()
    du, de = eng._noise_to_device(u_f, eta)
    eng.forward_backward(0, du, de)
    torch.cuda.synchronize()
    assert eng.scaler_frozen and eng._frozen_form(eng.obs, injected=True) is (FrozenForm.SORTED_ROWS if form == "sorted_rows" else FrozenForm.SLOTS)
    assert_terms(eng.loss_terms(), out, name)
    g_hip = [g.cpu().numpy() for g in eng.grad_tensors()]
    keep = [0, 1] + list(range(len(g_hip) - n, len(g_hip)))
    if form == "sorted_rows":        # the scaler's gradient is absent (the slot kernels still form the image scales' term: masked, below) ...
        assert all(float(np.abs(g_hip[k]).max()) == 0.0 for k in range(2, len(g_hip) - n))
    errs = [util.rel_err(g_hip[k], grads[k].numpy()) for k in keep]
    print(f"frozen {form}: gradient errors {['%.1e' % e for e in errs]}")
    assert max(errs) < P.RTOL_GRAD and all(float(np.abs(g_hip[k]).max()) > 0.0 for k in keep)
    # ... from the norm too: one training step's "Grad Norm" is the norm over q and the network
    model = neural_model(case, kw, opts, data, cfg, params, net)
    hist = model.train_model(inputs, 1, progress=False, noise=lambda i: (u_f, eta))
    want = float(np.sqrt(sum(float((grads[k].double() ** 2).sum()) for k in keep)))
    assert abs(hist["Grad Norm"][0] - want) <= P.RTOL_GRAD * want, (hist["Grad Norm"], want)
    # in-kernel noise, two engines: the network's gradient and sigpred agree bit for bit
    runs = []
    for _ in range(2):
        e = fresh()
        e.forward_backward(3)
        torch.cuda.synchronize()
        runs.append((e.layout.view(e.grads, "ev11").clone(), e.obs.nlik.sigpred.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and float(runs[0][0].abs().max()) > 0.0


def test_likelihood_not_trainable_skips_its_backward_and_masks_its_segments():
    case, kw, opts, data, cfg, params, u_f, eta, net = problem("mlp32_2x32")
    model = neural_model(case, kw, opts, data, cfg, params, net)
    model.likelihood.trainable = False
    inputs = util.reference_inputs(data)
    before = model.likelihood.raw.clone() if model.likelihood.raw is not None else None
    hist = model.train_model(inputs, 2, progress=False, noise=lambda i: (u_f, eta))
    eng = model._engine
    assert len(hist["loss"]) == 2 and np.isfinite(hist["loss"]).all()
    assert float(eng.layout.view(eng.grads, "ev11").abs().max()) == 0.0
    assert torch.equal(eng.layout.view(eng.params, "ev11").cpu(), torch.as_tensor(RN.flat_of(net)))
    assert before is None or torch.equal(before.cpu(), model.likelihood.raw.cpu())
    owners = eng.layout.seg_owner
    assert [bool(f) for f in eng.frozen.cpu().tolist()] == [o == "likelihood" for o in owners]


# ---- (d) NLL_val -----------------------------------------------------------------------------------------------------------------------------------
def test_validation_nll_takes_the_mean_over_the_validation_rows():
    from careless_amd.models.likelihoods import NeuralNormalLikelihood
    kw = dict(N=384, R=48, d0=5, L=2, w=32, S=2)
    data, cfg, params, x, u_f, eta = util.make_problem(seed=7, **kw)
    inputs = util.reference_inputs(data)
    n_tr = 300
    train, test = tuple(a[:n_tr] for a in inputs), tuple(a[n_tr:] for a in inputs)

    def as_x(t):
        d = dict(data)
        d.update(refl_id=t[0][:, 0], image_id=t[1][:, 0], metadata=t[3], iobs=t[4][:, 0], sigiobs=t[5][:, 0])
        return O.inputs_from_numpy(d)
    x_tr, x_te = as_x(train), as_x(test)
    net, _ = RN.pick_net(2, 8, data["iobs"], data["sigiobs"], first_seed=3)
    net = [O.f64(t.to(torch.float32)) for t in net]
    rng = np.random.default_rng(12)
    noise = (u_f, eta[:, :n_tr])
    vnoise = (rng.random((2, 48)).astype(np.float32), rng.normal(size=(2, kw["N"] - n_tr)).astype(np.float32))
    model = util.build_model(data, cfg, params, kw["L"], kw["w"])
    model.likelihood = NeuralNormalLikelihood(2, 8)
    model.likelihood.set_weights([t.numpy() for t in net])
    hist = model.train_model(train, 1, progress=False, validation_data=test, validation_frequency=1, noise=lambda i: noise, validation_noise=lambda i: vnoise)
    p, nt = params.clone(), [t.clone() for t in net]
    rec = O.train_step(RN.with_net(p, nt), x_tr, RN.under(cfg), O.AdamState.zeros_like(p.tensors() + nt), *map(O.f64, noise))
    assert rec["kink"] > RN.KINK_REL
    ref = O.validation_nll(RN.with_net(p, nt), x_te, RN.under(cfg), O.f64(vnoise[0]), O.f64(vnoise[1]), n_tr)
    # ... not the training set's mean: sigpred of the validation rows under the mean over ALL rows is another number
    _, sp_all, _, _ = O.nlik_forward(nt, data["iobs"], data["sigiobs"])
    _, sp_te, _, kink_te = O.nlik_forward(nt, data["iobs"][n_tr:], data["sigiobs"][n_tr:])
    assert kink_te > RN.KINK_REL and util.rel_err(sp_all[n_tr:].detach().numpy(), sp_te.detach().numpy()) > 1e-3
    print("NLL_val", hist["NLL_val"], "reference", ref)
    assert len(hist["NLL_val"]) == 1 and abs(hist["NLL_val"][0] - ref) <= P.RTOL_LOSS * abs(ref)
    assert abs(hist["NLL"][0] - rec["NLL"]) <= P.RTOL_LOSS * abs(rec["NLL"])


# ---- (e) a shard cut into pieces ----------------------------------------------------------------------------------------------------------------------
def test_chunked_shard_equals_the_uncut_step(monkeypatch):
    from careless_amd.engine import ElboEngine, ObsChunks
    name = "mlp32_2x32"
    case, kw, opts, data, cfg, params, u_f, eta, net = problem(name)
    inputs = util.reference_inputs(data)
    out, grads = O.elbo_value_and_grads(RN.with_net(params, net), O.inputs_from_numpy(data), RN.under(cfg), O.f64(u_f), O.f64(eta))
    assert out["kink"] > RN.KINK_REL
    whole = ElboEngine(neural_model(case, kw, opts, data, cfg, params, net), inputs, seed=5)
    monkeypatch.setenv("CARELESS_HIP_MAX_LAUNCH_BYTES", str(32 * 128))            # 128 rows of 8 metadata floats per launch
    cut = ElboEngine(neural_model(case, kw, opts, data, cfg, params, net), inputs, seed=5)
    monkeypatch.delenv("CARELESS_HIP_MAX_LAUNCH_BYTES")
    assert isinstance(cut.obs, ObsChunks) and len(cut.obs.children) == 3 and not isinstance(whole.obs, ObsChunks)
    res = []
    for e in (whole, cut):
        du, de = e._noise_to_device(u_f, eta)
        e.forward_backward(0, du, de)
        torch.cuda.synchronize()
        res.append((e.loss_terms(), [g.cpu().numpy() for g in e.grad_tensors()], e.obs.nlik.sigpred[: kw["N"]].clone()))
    (tw, gw, sw), (tc, gc, sc) = res
    assert torch.equal(sw, sc)                                          # one forward over the whole shard, the same mean
    assert_terms(tc, out, name + " (cut)")
    assert abs(tc["nll"] - tw["nll"]) <= P.RTOL_LOSS * abs(tw["nll"])
    assert_grads(gc, grads, (data, cfg, params, u_f, eta, net), name + " (cut)")
    assert max(util.rel_err(a, b) for a, b in zip(gc, gw)) < P.RTOL_GRAD


# ---- (f) an Adam trajectory -----------------------------------------------------------------------------------------------------------------------------
def test_adam_trajectory_of_twenty_steps():
    from careless_amd.models.likelihoods import NeuralNormalLikelihood
    kw = dict(N=384, R=48, d0=5, L=2, w=32, S=2)
    steps = 20
    data, cfg, params, x, _, _ = util.make_problem(seed=7, **kw)
    rng = np.random.default_rng(18)
    noises = [(rng.random((2, 48)).astype(np.float32), rng.normal(size=(2, 384)).astype(np.float32)) for _ in range(steps)]
    net, _ = RN.pick_net(2, 8, data["iobs"], data["sigiobs"], first_seed=3)
    net = [O.f64(t.to(torch.float32)) for t in net]
    model = util.build_model(data, cfg, params, kw["L"], kw["w"])
    model.likelihood = NeuralNormalLikelihood(2, 8)
    model.likelihood.set_weights([t.numpy() for t in net])
    p, nt = params.clone(), [t.clone() for t in net]
    st = O.AdamState.zeros_like(p.tensors() + nt)
    ref = [O.train_step(RN.with_net(p, nt), x, RN.under(cfg), st, O.f64(u), O.f64(e)) for u, e in noises]
    assert min(r["kink"] for r in ref) > RN.KINK_REL, min(r["kink"] for r in ref)
    hist = model.train_model(util.reference_inputs(data), steps, progress=False, noise=lambda i: noises[i])
    assert len(hist["loss"]) == steps
    for k in ("loss", "NLL", "F KLDiv", "Grad Norm"):
        err = max(abs(a - r[k]) / max(abs(r[k]), 1.0 if k == "F KLDiv" else 0.0) for a, r in zip(hist[k], ref))
        print(f"trajectory: {k} worst relative error {err:.2e}")
        assert err <= 1e-4, (k, err)
    got = [t.cpu().numpy() for t in model._engine.param_tensors()]
    errs = [util.rel_err(a, b.detach().numpy()) for a, b in zip(got, p.tensors() + nt)]
    print("trajectory: parameters", ["%.1e" % e for e in errs])
    assert max(errs) < 2e-4
    assert util.rel_err(net[0].numpy(), nt[0].detach().numpy()) > 1e-3        # the network moved


# ---- (g) the non-finite contract ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", ["iobs_nan", "sigiobs_nan"])
@pytest.mark.parametrize("name", ["lane_20x10_d5_S1", "mlp64_5x64_posenc_studentt_S8", "frozen_mono_20x10"])
def test_nan_observation_stops_training_with_finite_parameters(name, poison):
    case, kw, opts, data, cfg, params, u_f, eta, net = problem(name, poison)
    model = neural_model(case, kw, opts, data, cfg, params, net)
    inputs = util.reference_inputs(data)
    hist = model.train_model(inputs, 4, progress=False, noise=lambda i: (u_f, eta))
    eng = model._engine
    assert len(hist["loss"]) == 1 and not np.isfinite(hist["Grad Norm"][0]) and not np.isfinite(hist["NLL"][0])
    assert bool(torch.isnan(eng.obs.nlik.sigpred[: eng.obs.nlik.n]).all())                   # the mean couples all rows
    assert bool(torch.isfinite(eng.params).all())
    assert all(bool(torch.isfinite(t).all()) for t in model.likelihood.weights)


# ---- (h) the engine's gradient is the derivative of its own loss ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mlp32_2x32", "lane_20x10_d5_S1"])
def test_network_gradient_is_the_derivative_of_the_engines_own_loss(name):
    from careless_amd.engine import ElboEngine
    case, kw, opts, data, cfg, params, u_f, eta, net = problem(name)
    model = neural_model(case, kw, opts, data, cfg, params, net, deterministic=True)
    eng = ElboEngine(model, util.reference_inputs(data), seed=3)
    du, de = eng._noise_to_device(u_f, eta)

    def loss():
        eng.forward_backward(0, du, de)
        torch.cuda.synchronize()
        return eng.loss_terms()["loss"]
    l0 = loss()
    g, p0 = eng.grads.clone().double(), eng.params.clone()
    rng = np.random.default_rng(5)
    lay = eng.layout
    segs = [(lo, hi) for lo, hi, o in zip(lay.seg_off[:-1], lay.seg_off[1:], lay.seg_owner) if o == "likelihood"]
    assert len(segs) == len(net)
    for lo, hi in segs:
        assert float(g[lo:hi].abs().max()) > 0.0
        v = torch.zeros_like(p0, dtype=torch.float64)
        v[lo:hi] = g[lo:hi] / float(g[lo:hi].norm())
        if hi - lo >= 4:
            r = torch.as_tensor(rng.normal(size=hi - lo), device=p0.device)
            v[lo:hi] += r / float(r.norm())
        slope, vmax, best = abs(float((g * v).sum())), float(v[lo:hi].abs().max()), None
        # the pattern of tests/test_self_consistency.py; the caps are relative to the tensor's own scale (raw intensities in: a step of
        # 1e-3 of a first-layer weight moves pre-activations by units)
        scale = float(p0[lo:hi].abs().max())
        for target, cap in ((4e-4, 2e-3), (1e-4, 5e-4), (3e-5, 1e-4)):
            h = min(target * abs(l0) / max(slope, 1e-30), cap * scale / vmax)
            eng.params.copy_((p0.double() + h * v).float())
            hp = eng.params.double() - p0.double()
            lp = loss()
            eng.params.copy_((p0.double() - h * v).float())
            hm = eng.params.double() - p0.double()
            lm = loss()
            exp = float((g * (hp - hm)).sum())
            err = abs((lp - lm) - exp) / max(abs(exp), 1e-6 * abs(l0))
            best = err if best is None else min(best, err)
        eng.params.copy_(p0)
        print(f"{name}: segment [{lo}, {hi}) finite-difference error {best:.2e}")
        assert best < 3e-2, (name, lo, hi, best, slope, l0)
