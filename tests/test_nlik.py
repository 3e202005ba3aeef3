"""The neural likelihood off the GPU: the plugin class, its place in the flat parameter vector, the engine's refusals, the entry checks of
cl_nlik_forward / cl_nlik_backward, and the fp64 reference (the oracle's neural likelihood) checked by finite differences of its own loss."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from careless_amd import _lib
from careless_amd.engine import FLAT_GROUPS, FlatLayout, bind_flat, check_neural_likelihood, make_layout, split_flat
from careless_amd.models.likelihoods import NeuralLikelihood, NeuralNormalLikelihood
from careless_amd.models.likelihoods.mono import Ev11Likelihood, lik_dense_slices, lik_param_count
from careless_amd.models.scaling.image import image_layer_layout
from careless_amd.models.scaling.nn import dense_slices
from oracle import elbo_oracle as O
from tests import ref_nlik as RN
from tests import util

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- the class surface -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,w", [(1, 1), (2, 16), (3, 32), (4, 5)])
def test_weights_are_keras_ordered_views_of_one_flat_tensor(L, w):
    lik = NeuralNormalLikelihood(L, w)
    assert (lik.kind, lik.neural, lik.leakiness) == ("normal", True, 0.3)
    lik.build(seed=5)
    dims = [2] + [w] * L + [1]
    assert [tuple(t.shape) for t in lik.weights] == [s for i, o in zip(dims[:-1], dims[1:]) for s in ((i, o), (o,))]
    assert lik.raw.dtype == torch.float32 and lik.raw.numel() == lik.param_count() == lik_param_count(L, w) == sum(i * o + o for i, o in zip(dims[:-1], dims[1:]))
    assert len(lik.trainable_variables) == 2 * (L + 1)
    # glorot-uniform kernels, zero biases
    for k, (i, o) in enumerate(zip(dims[:-1], dims[1:])):
        W, b = lik.weights[2 * k], lik.weights[2 * k + 1]
        assert float(W.abs().max()) <= math.sqrt(6.0 / (i + o)) and float(b.abs().max()) == 0.0
        assert i * o < 8 or float(W.abs().max()) > 0.5 * math.sqrt(6.0 / (i + o))
    # views: a write through `weights` lands in `raw`, in the W^T layout (kernel transposed, then bias)
    lik.weights[0][1, 0] = 7.0
    lik.weights[1][0] = -3.0
    assert float(lik.raw[1]) == 7.0 and float(lik.raw[2 * w]) == -3.0
    lik.trainable = False
    assert lik.trainable_variables == []


def test_same_seed_same_weights_and_save_load_round_trip(tmp_path):
    a, b, c = (NeuralNormalLikelihood(2, 9) for _ in range(3))
    a.build(seed=11); b.build(seed=11); c.build(seed=12)
    assert torch.equal(a.raw, b.raw) and not torch.equal(a.raw, c.raw)
    path = str(tmp_path / "lik.pt")
    a.save_weights(path)
    c.load_weights(path)
    assert torch.equal(a.raw, c.raw)
    ws = [np.asarray(t) + 1.0 for t in a.weights]
    b.set_weights(ws)
    assert all(np.array_equal(np.asarray(t), s) for t, s in zip(b.weights, ws))
    with pytest.raises(ValueError):
        NeuralNormalLikelihood(3, 9).load_weights(path)


def test_base_class_has_no_base_dist():
    lik = NeuralLikelihood(1, 4)
    with pytest.raises(NotImplementedError, match="base_dist"):
        lik.base_dist(0.0, 1.0)
    data, *_ = util.make_problem(N=20, R=5)
    with pytest.raises(NotImplementedError, match="base_dist"):
        lik(util.reference_inputs(data))


@pytest.mark.parametrize("L,w,seed", [(2, 8, 7), (3, 32, 8), (1, 5, 3)])
def test_call_log_prob_matches_the_fp64_reference(L, w, seed):
    data, cfg, params, x, u_f, eta = util.make_problem(N=300, S=3, seed=seed)
    net, _ = RN.pick_net(L, w, x.iobs, x.sigiobs, first_seed=seed)
    lik = NeuralNormalLikelihood(L, w)
    lik.set_weights([t.numpy() for t in net])
    net = [O.f64(np.asarray(t)) for t in lik.weights]            # (the fp32 values the class holds)
    ipred = O.elbo_forward(params, x, cfg, O.f64(u_f), O.f64(eta))["ipred"].detach()
    delta, sigpred, _, _ = O.nlik_forward(net, x.iobs, x.sigiobs)
    want = O.normal_log_prob(ipred, x.iobs[None, :], sigpred[None, :]).numpy()
    dist = lik(util.reference_inputs(data))
    got = dist.log_prob(ipred.numpy())
    assert got.shape == want.shape and util.rel_err(got, want) < 1e-6
    assert util.rel_err(dist.stddev(), sigpred.numpy()) < 1e-9 and np.array_equal(dist.mean(), np.asarray(data["iobs"], dtype=np.float64))
    assert abs(float(np.mean(dist.stddev() / np.asarray(data["sigiobs"], dtype=np.float64))) - 1.0) < 1e-9      # mean(delta / mean(delta)) = 1


# ---- the flat vector -----------------------------------------------------------------------------------------------------------------------
def _layout_before(R, d, w, L, n_img, n_ev11=0, n_dwr=0, imgl=None):
    """`make_layout` as it was before the likelihood's group could hold a network (restated: the comparison below needs the old answer)."""
    seg, owner = [0, R, 2 * R], ["q", "q"]
    for _, out, _, ob in dense_slices(d, w, L):
        seg += [2 * R + ob, 2 * R + ob + out]; owner += ["scaler", "scaler"]
    off = seg[-1]
    P = off - 2 * R
    if n_img > 0:
        off += n_img; seg.append(off); owner.append("scaler")
    n_imgl = 0
    if imgl is not None:
        K, M = imgl
        blocks, n_imgl = image_layer_layout(K, M, w)
        for ow, ob in blocks:
            seg += [off + ob, off + ob + M * w]; owner += ["scaler", "scaler"]
        off += n_imgl
    for _ in range(n_ev11):
        off += 1; seg.append(off); owner.append("likelihood")
    if n_dwr > 0:
        off += n_dwr; seg.append(off); owner.append("prior")
    return dict(R=R, P=P, n_img=n_img, seg_off=seg, seg_owner=owner, n_ev11=n_ev11, n_dwr=n_dwr, n_imgl=n_imgl)


def test_layout_without_the_keyword_is_what_it_was():
    for L, w, d in ((2, 32, 5), (20, 10, 5)):
        for R in (1, 3, 100):
            for n_img in (0, 9):
                for imgl in (None, (2, 7)):
                    for n_ev11 in (0, 3):
                        for n_dwr in (0, 4):
                            lay = make_layout(R=R, d=d, w=w, L=L, n_img=n_img, n_ev11=n_ev11, n_dwr=n_dwr, imgl=imgl)
                            want = _layout_before(R, d, w, L, n_img, n_ev11, n_dwr, imgl)
                            assert {k: getattr(lay, k) for k in want} == want and lay.lik_dense is None
                            assert lay == FlatLayout(**want)


@pytest.mark.parametrize("Ln,wn", [(1, 1), (2, 16), (3, 32)])
def test_layout_with_the_network_has_one_segment_per_kernel_and_bias(Ln, wn):
    assert FLAT_GROUPS == ("q_loc", "q_scale", "mlp", "img", "imgl", "ev11", "dwr")
    slices = lik_dense_slices(Ln, wn)
    P_lik = lik_param_count(Ln, wn)
    assert P_lik == int(_lib.get_lib().cl_nlik_param_count(Ln, wn)) and slices[-1][1:3] == (1, wn) and slices[0][2] == 2
    for R, n_img, imgl, n_dwr in ((40, 3, None, 0), (7, 0, (2, 5), 4)):
        base = make_layout(R=R, d=5, w=10, L=3, n_img=n_img, n_dwr=n_dwr, imgl=imgl)
        lay = make_layout(R=R, d=5, w=10, L=3, n_img=n_img, n_dwr=n_dwr, imgl=imgl, lik_dense=slices)
        assert [g[0] for g in lay.groups] == list(FLAT_GROUPS)
        assert lay.n_ev11 == P_lik and lay.n == base.n + P_lik and lay.off_ev11 == base.off_ev11 and lay.off_dwr == base.off_dwr + P_lik
        cut = len(base.seg_off) - (1 if n_dwr else 0)                  # the network's segments sit in front of the double-Wilson r
        assert lay.seg_off[:cut] == base.seg_off[:cut] and lay.seg_owner[:cut - 1] == base.seg_owner[:cut - 1]
        mine = lay.seg_off[cut - 1:cut + 2 * len(slices)]
        want = [lay.off_ev11]
        for ow, o, i, ob in slices:
            assert want[-1] == lay.off_ev11 + ow
            want += [lay.off_ev11 + ob, lay.off_ev11 + ob + o]
        assert mine == want and mine[-1] == lay.off_ev11 + P_lik
        assert lay.seg_owner[cut - 1:cut - 1 + 2 * len(slices)] == ["likelihood"] * (2 * len(slices))
        assert lay.seg_owner[cut - 1 + 2 * len(slices):] == (["prior"] if n_dwr else []) and lay.seg_off[-1] == lay.n
        assert len(lay.seg_off) == len(lay.seg_owner) + 1 and sorted(lay.seg_off) == lay.seg_off
    with pytest.raises(NotImplementedError, match="mutually exclusive"):
        make_layout(R=4, d=5, w=10, L=3, n_img=0, n_ev11=3, lik_dense=slices)


def test_bind_and_split_with_the_network():
    from careless_amd.models.scaling.nn import MetadataScaler

    class Q:
        pass
    R, d, w, L = 6, 5, 4, 2
    q = Q()
    q.loc_raw, q.scale_raw = torch.arange(R, dtype=torch.float32), torch.arange(R, dtype=torch.float32) + 100
    mlp = MetadataScaler(L, w)
    mlp.build(d)
    lik = NeuralNormalLikelihood(2, 3)
    lik.build(seed=1)
    before = [t.clone() for t in lik.weights]
    lay = make_layout(R, d, w, L, 0, lik_dense=lik.layer_slices())
    flat = torch.zeros(lay.n)
    bind_flat(flat, lay, q, mlp, lik=lik)
    assert lik.raw.data_ptr() == flat[lay.off_ev11:].data_ptr() and lik.raw.numel() == lik.param_count()
    assert all(torch.equal(a, b) for a, b in zip(lik.weights, before))
    lik.weights[2][0, 1] = 42.0                                     # the plugin's views are views of the engine's vector
    assert float(flat[lay.off_ev11 + lik.layer_slices()[1][0] + 1 * 3 + 0]) == 42.0
    parts = split_flat(flat, lay, mlp.layer_slices(d))
    n_model = 2 + 2 * (L + 1)
    assert len(parts) == n_model + 6
    assert [tuple(t.shape) for t in parts[n_model:]] == [(2, 3), (3,), (3, 3), (3,), (3, 1), (1,)]
    assert all(torch.equal(a, b) for a, b in zip(parts[n_model:], lik.weights))
    assert sum(t.numel() for t in parts) == lay.n


# ---- refusals (host logic of ElboEngine.__init__) -------------------------------------------------------------------------------------------------
def test_engine_refuses_what_the_neural_likelihood_does_not_run_on():
    lib = _lib.get_lib()
    lik = NeuralNormalLikelihood(2, 16)
    assert check_neural_likelihood(lik, laue=False, world=1, lib=lib) is True
    from careless_amd.models.likelihoods.mono import NormalLikelihood
    assert check_neural_likelihood(NormalLikelihood(), laue=True, world=8, lib=lib) is False
    with pytest.raises(NotImplementedError, match="monochromatic only"):
        check_neural_likelihood(lik, laue=True, lib=lib)
    with pytest.raises(NotImplementedError, match="one rank"):
        check_neural_likelihood(lik, laue=False, world=2, lib=lib)

    class Both(NeuralNormalLikelihood):
        ev11 = True
    with pytest.raises(NotImplementedError, match="Evans-2011"):
        check_neural_likelihood(Both(2, 16), laue=False, lib=lib)
    for L, w in ((5, 16), (2, 33)):
        with pytest.raises(NotImplementedError, match=r"1 \.\. 4 hidden layers of width 1 \.\. 32"):
            check_neural_likelihood(NeuralNormalLikelihood(L, w), laue=False, lib=lib)
    assert not getattr(Ev11Likelihood(), "neural", False)


# ---- the library's surface -------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("cl_nlik_forward", "cl_nlik_backward", "cl_nlik_supports", "cl_nlik_param_count", "cl_nlik_workspace_bytes", "cl_nlik_grid")


def test_new_symbols_are_exported_and_declared():
    lib = _lib.get_lib()
    with open(os.path.join(os.path.dirname(HERE), "include", "careless_hip.h")) as f:
        header = f.read()
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTS and getattr(lib, name) is not None and name + "(" in header, name
    assert "typedef struct cl_nlik_args" in header and "mono.py:75-110" in header
    assert int(lib.cl_abi_sizeof(b"cl_nlik_args")) == C.sizeof(_lib.NlikArgs)
    from careless_amd import build
    assert any(u[0] == "elbo_nlik.hip" and "-fno-honor-nans" not in u[2] for u in build.UNITS)


def test_supports_is_one_to_four_layers_of_width_one_to_thirty_two():
    lib = _lib.get_lib()
    for L in range(0, 7):
        for w in range(0, 41):
            assert bool(lib.cl_nlik_supports(L, w)) == (1 <= L <= 4 and 1 <= w <= 32), (L, w)
            assert (int(lib.cl_nlik_workspace_bytes(1000, L, w)) > 0) == bool(lib.cl_nlik_supports(L, w))
    assert int(lib.cl_nlik_workspace_bytes(0, 2, 16)) == 0 and int(lib.cl_nlik_grid(0)) == 0
    assert [int(lib.cl_nlik_grid(n)) for n in (1, 256, 257, 10 ** 7)] == [1, 1, 2, 1024]
    G, P = 2, lik_param_count(2, 16)
    assert int(lib.cl_nlik_workspace_bytes(300, 2, 16)) == 8 * 300 + 16 * G + 4 * G * P


def _args(**over):
    """Arguments every clause of the entry checks accepts (addresses that are never read: a rejected call does not touch the device)."""
    a = _lib.NlikArgs()
    a.iobs, a.sigiobs, a.net, a.sigpred, a.workspace = 1024, 2048, 4096, 8192, 1 << 16
    a.L, a.w, a.leak, a.n = 2, 16, 0.3, 100
    a.ipred, a.d_net, a.S, a.w_ll = 1 << 17, 1 << 18, 3, 1.0
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("which", ["cl_nlik_forward", "cl_nlik_backward"])
def test_entry_checks_reject_one_clause_at_a_time(which):
    fn = getattr(_lib.get_lib(), which)
    assert fn(None, None) == -1
    for field in ("iobs", "sigiobs", "net", "sigpred", "workspace"):
        assert fn(C.byref(_args(**{field: None})), None) == -1, field
    assert fn(C.byref(_args(n=0)), None) == -1
    assert fn(C.byref(_args(workspace=(1 << 16) + 8)), None) == -1                   # not 16-byte aligned
    assert fn(C.byref(_args(pos=512)), None) == -1 and fn(C.byref(_args(sig_image=512)), None) == -1      # exactly one of the pair
    for L, w in ((0, 16), (5, 16), (2, 0), (2, 33)):
        assert fn(C.byref(_args(L=L, w=w)), None) == -2, (L, w)
    if which == "cl_nlik_backward":
        for over in (dict(ipred=None), dict(d_net=None), dict(S=0)):
            assert fn(C.byref(_args(**over)), None) == -1, over
    with pytest.raises(NotImplementedError, match="1 .. 4 hidden layers"):
        _lib.check(-2, which)


# ---- the reference, checked by something other than itself -------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,w,seed,klw", [(2, 8, 7, None), (1, 5, 3, None), (3, 32, 8, 0.5)])
def test_reference_gradient_matches_finite_differences_of_its_own_loss(L, w, seed, klw):
    data, cfg, params, x, u_f, eta = util.make_problem(N=120, R=20, S=2, seed=seed, kl_weight=klw)
    net, _ = RN.pick_net(L, w, x.iobs, x.sigiobs, first_seed=seed)
    out, grads = O.elbo_value_and_grads(RN.with_net(params, net), x, RN.under(cfg), O.f64(u_f), O.f64(eta))
    assert out["kink"] > RN.KINK_REL
    g_net = grads[-len(net):]
    rng = np.random.default_rng(seed)
    for k, t in enumerate(net):
        v = O.f64(rng.normal(size=tuple(t.shape)))
        h = 1e-6 * max(float(t.abs().max()), 1e-2)
        lo, hi = ([s.clone() for s in net] for _ in range(2))
        lo[k] -= h * v
        hi[k] += h * v
        fd = (float(O.elbo_value_and_grads(RN.with_net(params, hi), x, RN.under(cfg), O.f64(u_f), O.f64(eta))[0]["loss"]) -
              float(O.elbo_value_and_grads(RN.with_net(params, lo), x, RN.under(cfg), O.f64(u_f), O.f64(eta))[0]["loss"])) / (2 * h)
        an = float((g_net[k] * v).sum())
        # (central differences: truncation ~ h^2, rounding ~ eps64 |loss| / h)
        assert abs(fd - an) <= 1e-5 * abs(an) + 1e-14 * abs(float(out["loss"])) / h, (k, fd, an)
    # the model's own gradients are the oracle's with the Normal term traded: they differ from the plain Normal step's
    _, g_plain = O.elbo_value_and_grads(params, x, cfg, O.f64(u_f), O.f64(eta))
    assert util.rel_err(grads[0].numpy(), g_plain[0].numpy()) > 1e-3


def test_kernel_reference_agrees_with_the_whole_step_reference():
    """`kernel_reference` (what the GPU kernels are held to on injected predictions) is the network part of the whole-step reference."""
    data, cfg, params, x, u_f, eta = util.make_problem(N=150, R=20, S=3, seed=9)
    net, _ = RN.pick_net(2, 10, x.iobs, x.sigiobs, first_seed=4)
    out, grads = O.elbo_value_and_grads(RN.with_net(params, net), x, RN.under(cfg), O.f64(u_f), O.f64(eta))
    assert np.isfinite(float(out["loss"])) and float(out["delta"].min()) > 4e-5
    delta, sigpred, g, kink = RN.kernel_reference(net, x.iobs, x.sigiobs, out["ipred"].t(), 1.0 / 3)
    assert torch.equal(sigpred, out["sigpred"]) and kink == out["kink"]
    for a, b in zip(g, grads[-len(net):]):
        assert util.rel_err(a.numpy(), b.numpy()) < 1e-12
    # the closed form the kernels implement (the issue's formulas) against autograd
    S = 3
    ip, io, sg = out["ipred"].t(), x.iobs.double(), x.sigiobs.double()
    gi = (1.0 / S) * (1.0 / sigpred[:, None] - (ip - io[:, None]) ** 2 / sigpred[:, None] ** 3).sum(dim=1)
    T, m, N = float((gi * sigpred).sum()), float(delta.mean()), len(io)
    dd = (gi * sg - T / N) / m
    assert abs(float((delta * dd).sum())) <= 1e-9 * float((delta * dd).abs().sum())            # scale invariance
    _, _, zh, _ = O.nlik_forward(net, x.iobs, x.sigiobs)
    assert util.rel_err(float((dd * torch.sigmoid(zh)).sum()), float(g[-1][0])) < 1e-10       # the head's bias gradient
