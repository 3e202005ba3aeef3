"""Host-side logic of careless_amd that needs no GPU: the input-tuple contract, the flat parameter layout, sharding,
plugin classes, and that libcareless_hip.so loads and exports every symbol include/careless_hip.h declares.  CPU only."""
import os
import re

import numpy as np
import pytest
import torch

from careless_amd import _lib
from careless_amd.engine import make_layout, make_shard
from careless_amd.models.base import BaseModel
from careless_amd.models.likelihoods.mono import NormalLikelihood, StudentTLikelihood
from careless_amd.models.merging.surrogate_posteriors import TruncatedNormal
from careless_amd.models.merging.variational import VariationalMergingModel
from careless_amd.models.priors.wilson import WilsonPrior
from careless_amd.models.scaling.image import HybridImageScaler, ImageScaler
from careless_amd.models.scaling.nn import MLPScaler
from careless_amd.workloads import bytes_per_obs, flops_per_obs, make_workload, reference_inputs
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --- input contract (reference tests/models/test_base_model.py:6-28) -----------------------------------------
def test_base_model_contract():
    assert BaseModel.input_index == {"refl_id": 0, "image_id": 1, "file_id": 2, "metadata": 3, "intensities": 4,
                                     "uncertainties": 5, "wavelength": 6, "harmonic_id": 7}
    data = util.make_problem(N=50, R=8)[0]
    mono = reference_inputs(data)
    assert not BaseModel.is_laue(mono)
    laue = mono + (np.ones((50, 1), np.float32), np.zeros((50, 1), np.int64))
    assert BaseModel.is_laue(laue)
    for name, idx in BaseModel.input_index.items():
        assert BaseModel.get_name_by_index(idx) == name
        assert BaseModel.get_index_by_name(name) == idx
        assert BaseModel.get_input_by_name(laue, name) is laue[idx]
    assert BaseModel.get_metadata(mono).shape == (50, 5) and BaseModel.get_metadata(mono).dtype == np.float32
    assert BaseModel.get_refl_id(mono).dtype == np.int64 and BaseModel.get_refl_id(mono).shape == (50, 1)
    with pytest.raises(ValueError):
        BaseModel.get_index_by_name("nope")
    with pytest.raises(ValueError):
        BaseModel.get_name_by_index(99)
    with pytest.raises(ValueError):
        BaseModel.get_harmonic_id(mono)
    batched = tuple(a[None] for a in mono)          # a leading batch axis of 1 is squeezed (base.py:79-80)
    assert BaseModel.get_metadata(batched).shape == (50, 5)


# --- flat layout / sharding ---------------------------------------------------------------------------------------
def test_flat_layout_matches_scaler_and_library():
    lay = make_layout(R=100, d=21, w=64, L=5, n_img=9)
    mlp = MLPScaler(5, 64)
    assert lay.P == mlp.param_count(21) == 21 * 64 + 64 + 4 * (64 * 64 + 64) + 2 * 64 + 2
    assert lay.n == 200 + lay.P + 9
    assert lay.seg_off[0] == 0 and lay.seg_off[-1] == lay.n and len(lay.seg_owner) == len(lay.seg_off) - 1
    assert lay.seg_owner[:2] == ["q", "q"] and set(lay.seg_owner[2:]) == {"scaler"}
    assert np.all(np.diff(lay.seg_off) > 0)
    lib = _lib.get_lib()
    assert int(lib.cl_mlp_param_count(21, 64, 5)) == lay.P
    assert [int(lib.cl_mlp_max_layers(w)) for w in (10, 15, 16, 17, 32, 33, 64, 65)] == [20, 20, 20, 10, 10, 5, 5, 0]      # (16: its own instance since round 5)
    assert [int(lib.cl_mlp_meta_rows(d)) for d in (1, 4, 5, 21, 64)] == [4, 4, 8, 24, 64]


def test_shards_partition_observations_and_reflections():
    for N, R, W in [(1000, 31, 1), (1001, 31, 2), (999, 7, 4), (12345, 400, 8)]:
        sh = [make_shard(N, R, r, W) for r in range(W)]
        assert sh[0].start == 0 and sh[-1].stop == N and sh[0].kl_begin == 0 and sh[-1].kl_end == R
        for a, b in zip(sh[:-1], sh[1:]):
            assert a.stop == b.start and a.kl_end == b.kl_begin
        assert max(s.stop - s.start for s in sh) - min(s.stop - s.start for s in sh) <= W
    with pytest.raises(ValueError):
        make_shard(10, 3, 2, 2)


# --- plugin classes -----------------------------------------------------------------------------------------------
def test_scaler_parameter_views_and_identity_init():
    s = MLPScaler(3, 8)
    s.build(5)
    ws = s.weights
    assert [tuple(w.shape) for w in ws] == [(5, 8), (8,), (8, 8), (8,), (8, 8), (8,), (8, 2), (2,)]
    assert torch.equal(ws[0], torch.eye(5, 8)) and torch.equal(ws[6], torch.eye(8, 2)) and float(ws[1].abs().sum()) == 0.0
    ws[2][1, 3] = 7.0                                # views: Keras (in,out) element lands at W^T[out][in] of the flat buffer
    off = s.layer_slices()[1][0]
    assert float(s.flat[off + 3 * 8 + 1]) == 7.0
    with pytest.raises(ValueError):
        MLPScaler(2, 4, scale_bijector="tanh")
    with pytest.raises(ValueError):
        s.build(6)


def test_image_scaler_pins_first_image():
    im = ImageScaler(4)
    assert im.scales.tolist() == [1.0, 1.0, 1.0, 1.0] and im._scales.numel() == 3
    im._scales[:] = torch.tensor([2.0, 3.0, 4.0])
    ids = np.array([[0], [1], [3], [3]])
    inputs = (ids, ids, ids, np.zeros((4, 2), np.float32), np.zeros((4, 1), np.float32), np.ones((4, 1), np.float32))
    assert im(inputs).tolist() == [1.0, 2.0, 4.0, 4.0]


def test_wilson_prior_and_truncated_normal_host_protocol():
    from scipy import stats
    c = np.array([True, False, False])
    eps = np.array([1.0, 2.0, 1.0])
    p = WilsonPrior(c, eps, 1.0)
    E = np.array([0.5, 1.0, 2.0])
    ref = np.where(c, stats.halfnorm.logpdf(E, scale=np.sqrt(eps)), stats.weibull_min.logpdf(E, 2.0, scale=np.sqrt(eps)))
    assert np.allclose(p.log_prob(E), ref, rtol=1e-6)
    q = TruncatedNormal.from_loc_and_scale(p.mean(), p.stddev(), low=(1e-32 * ~c).astype(np.float32))
    assert len(q.trainable_variables) == 2 and q.trainable_variables[0].shape == (3,)      # reference test_truncated_normal.py:15-17
    assert np.allclose(q.loc.numpy(), p.mean(), rtol=1e-6) and np.allclose(q.scale.numpy(), p.stddev(), rtol=1e-6)
    loc, scale = q.loc.numpy().astype(float), q.scale.numpy().astype(float)
    a = (q.low.numpy() - loc) / scale
    m4 = stats.truncnorm.moment(4, a, np.inf, loc, scale)
    assert np.allclose(q.moment_4(method="scipy"), m4, rtol=1e-5)                          # reference test_truncated_normal.py:29-42
    if not torch.cuda.is_available():           # mean / stddev / moment_4('tf') are `cl_tn_moments`: no CPU path (tests/test_gpu_parity.py has them)
        from careless_amd._lib import CarelessHipError
        for f in (q.mean, q.stddev, lambda: q.moment_4(method="tf")):
            with pytest.raises(CarelessHipError):
                f()
    with pytest.raises(ValueError):
        q.moment_4(method="nope")
    q.trainable = False
    assert q.trainable_variables == []


def test_likelihood_objects_match_scipy():
    from scipy import stats
    data = util.make_problem(N=40, R=8)[0]
    inputs = reference_inputs(data)
    x = np.asarray(data["iobs"]) + 3.0
    assert np.allclose(NormalLikelihood()(inputs).log_prob(x), stats.norm.logpdf(x, data["iobs"], data["sigiobs"]), rtol=1e-5)
    assert np.allclose(StudentTLikelihood(4.0)(inputs).log_prob(x), stats.t.logpdf(x, 4.0, data["iobs"], data["sigiobs"]), rtol=1e-5)


def test_workload_bookkeeping():
    assert flops_per_obs(5, 64, 5) == 100992 and flops_per_obs(21, 64, 5) == 107136
    assert bytes_per_obs(5, 1) == 44 and bytes_per_obs(21, 8) == 164
    model, inputs, data, spec = make_workload("mono_1M_normal_5x64_S1", N=2000)
    assert spec["d"] == 5 and spec["R"] == 62 and inputs[3].shape == (2000, 5) and inputs[0].dtype == np.int64
    assert isinstance(model.scaling_model, HybridImageScaler) and model.mc_sample_size == 1
    assert np.all(np.diff(inputs[1][:, 0]) >= 0)                                          # image ids sorted
    assert set(np.unique(inputs[0][:, 0])) == set(range(62))                              # every reflection observed


# --- the C-ABI library -----------------------------------------------------------------------------------------------
def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "careless_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(cl_[a-z0-9_]+)\s*\(", hdr))
    assert {"cl_tn_forward", "cl_tn_backward", "cl_elbo_mono_fwd_bwd", "cl_mlp_forward", "cl_adam_step"} <= declared
    lib = _lib.get_lib()
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/careless_hip.h but not exported"
        assert name in _lib.EXPORTS, f"{name} not bound in careless_amd/_lib.py"
    assert lib.cl_version().startswith(b"careless_hip")


def test_compute_entry_points_fail_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    data, cfg, params, x, u_f, eta = util.make_problem(N=64, R=8, L=2, w=8, S=1)
    model = util.build_model(data, cfg, params, 2, 8)
    with pytest.raises(_lib.CarelessHipError):
        model.train_model(reference_inputs(data), 1, progress=False)
    with pytest.raises(_lib.CarelessHipError):
        model.surrogate_posterior.sample(2)
    with pytest.raises(_lib.CarelessHipError):
        model.scaling_model(reference_inputs(data))


def test_unsupported_plugins_are_rejected_not_emulated():
    class Odd:
        pass
    data, cfg, params, x, u_f, eta = util.make_problem(N=64, R=8, L=2, w=8, S=1)
    model = util.build_model(data, cfg, params, 2, 8)
    model.likelihood = Odd()
    with pytest.raises((NotImplementedError, _lib.CarelessHipError)):
        model.train_model(reference_inputs(data), 1, progress=False)


def test_double_wilson_prior_host_matches_oracle_and_validates_r():
    from careless_amd.models.priors.wilson import DoubleWilsonPrior
    from oracle import elbo_oracle as O
    data, cfg, params, x, u_f, eta = util.make_problem(N=200, R=40, S=2, double_wilson=True)
    out = O.elbo_forward(params, x, cfg, torch.as_tensor(u_f, dtype=torch.float64), torch.as_tensor(eta, dtype=torch.float64))
    prior = DoubleWilsonPrior(data["centric"], data["multiplicity"], data["parent_ids"], data["root"], data["asu_ids"], data["dw_r"])
    ref = O.double_wilson_log_prob(out["z_f"], x.centric, x.multiplicity, x.sigma, x.parent_ids, x.root, x.asu_ids, x.dw_r)
    assert np.allclose(prior.log_prob(out["z_f"].numpy()), ref.numpy(), rtol=1e-5, atol=1e-5)
    assert (data["parent_ids"] == -1).any()
    with pytest.raises(ValueError):                       # reference io/manager.py:415-419 (test_cli.py:92-110)
        DoubleWilsonPrior(data["centric"], data["multiplicity"], data["parent_ids"], data["root"], data["asu_ids"], [0.0, 1.0])


def test_laue_likelihood_convolve_known_answer():
    """reference tests/models/likelihoods/test_laue.py:11-36: convolve(iobs[hid] / count[hid]) reproduces iobs on the slots"""
    from careless_amd.models.likelihoods import laue
    from scipy import stats
    data = util.make_problem(N=120, R=16, laue=True)[0]
    inputs = util.reference_inputs(data)
    assert BaseModel.is_laue(inputs) and len(inputs) == 8
    hid = data["harmonic_id"]
    G = data["n_groups"]
    fake = (data["iobs"][hid] / np.bincount(hid)[hid]).astype(np.float32)
    lk = laue.NormalLikelihood()(inputs)
    conv = lk.convolve(fake)
    assert np.allclose(conv[:G], data["iobs"][:G], rtol=1e-5) and np.all(conv[G:] == 0)
    lp = lk.log_prob(fake)
    assert np.allclose(lp[:G], stats.norm.logpdf(data["iobs"][:G], data["iobs"][:G], data["sigiobs"][:G]), rtol=1e-5)
    assert np.allclose(lp[G:], stats.norm.logpdf(0.0, 1.0, 1.0))          # the padded-slot constant (formatter.py:637-640)
    assert np.allclose(lk.convolve(np.stack([fake] * 3)), conv[None, :])   # batched (reference :33-36)
    lt = laue.StudentTLikelihood(4.0)(inputs).log_prob(fake)
    assert np.allclose(lt[:G], stats.t.logpdf(data["iobs"][:G], 4.0, data["iobs"][:G], data["sigiobs"][:G]), rtol=1e-5)


def test_get_results_needs_the_hip_library_and_a_gpu():
    """F / SigF / <F^4> of the output step are `cl_tn_moments` (tests/test_output_step.py holds them against scipy on the GPU): on a
    machine without one the call fails loudly instead of computing the moments some other way."""
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_output_step.py::test_get_results_matches_scipy_moments covers the call")
    from careless_amd._lib import CarelessHipError
    from careless_amd.results import get_results
    data, cfg, params, x, u_f, eta = util.make_problem(N=120, R=30, S=1)
    model = util.build_model(data, cfg, params, 2, 32)
    with pytest.raises(CarelessHipError):
        get_results(model.surrogate_posterior, util.reference_inputs(data))


def test_ev11_host_likelihood_matches_scipy():
    """reference likelihoods/mono.py:39-73: scale = Sdfac sqrt(sig^2 + SdB softplus(x) + Sdadd softplus(x)^2)"""
    from scipy import stats
    from careless_amd.models.likelihoods.mono import NormalEv11Likelihood, StudentTEv11Likelihood
    data = util.make_problem(N=50, R=8)[0]
    inputs = reference_inputs(data)
    x = np.asarray(data["iobs"], dtype=np.float64) + 2.0
    lk = NormalEv11Likelihood()
    assert abs(lk.Sdfac - 1.0) < 1e-6 and abs(lk.Sdadd - 1.0) < 1e-6 and abs(lk.SdB - 1.0) < 1e-6 and len(lk.trainable_variables) == 1
    sp = np.logaddexp(0, x)
    sc = np.sqrt(np.asarray(data["sigiobs"], dtype=np.float64) ** 2 + sp + sp * sp)
    assert np.allclose(lk(inputs).log_prob(x), stats.norm.logpdf(x, data["iobs"], sc), rtol=1e-5, atol=1e-5)
    lt = StudentTEv11Likelihood(4.0)
    assert np.allclose(lt(inputs).log_prob(x), stats.t.logpdf(x, 4.0, data["iobs"], sc), rtol=1e-5, atol=1e-5)


def test_pack_by_image_and_pack_laue_layouts():
    """Host-side packing of the observation axis for the per-image-layer and single-pass Laue kernels (pure numpy)."""
    from careless_amd.engine import GRANULE, TILE, pack_by_image, pack_laue
    rng = np.random.default_rng(0)
    img = rng.integers(0, 7, size=1000)
    pos, n_pad, tile_img, row_map = pack_by_image(img)
    assert n_pad % TILE == 0 and len(np.unique(pos)) == 1000 and np.all(tile_img[pos // TILE] == img)
    assert np.all(row_map[pos] == np.arange(1000)) and (row_map >= 0).sum() == 1000
    for by_image in (False, True):
        sizes = rng.choice([1, 2, 3, 5, 16], p=[.7, .15, .05, .05, .05], size=300)
        hid = np.repeat(np.arange(300), sizes)
        gimg = np.sort(rng.integers(0, 4, size=300))
        img = gimg[hid]
        perm = rng.permutation(len(hid))
        hid, img = hid[perm], img[perm]
        pos, n_pad, gmeta, tile_gmax, row_map, tile_img = pack_laue(hid, img, by_image)
        assert len(np.unique(pos)) == len(hid) and pos.max() < n_pad and n_pad % TILE == 0
        for g in range(300):                       # members consecutive, inside one 16-row granule, member index / size recorded
            p = np.sort(pos[hid == g])
            assert np.all(np.diff(p) == 1) and p[0] // GRANULE == p[-1] // GRANULE
            assert list(gmeta[p] & 0xff) == list(range(len(p))) and np.all(gmeta[p] >> 8 == len(p))
        assert np.all(row_map[pos] == np.arange(len(hid))) and (gmeta[row_map < 0] == 0).all()
        assert np.all(tile_gmax[pos // TILE] >= (gmeta[pos] >> 8)) and tile_gmax.max() == 16
        if by_image:
            assert np.all(tile_img[pos // TILE] == img)
        else:
            assert tile_img is None
    assert pack_laue(np.zeros(17, int), np.zeros(17, int), False) is None      # a group larger than a wave: two-pass path


def test_kernel_name_follows_the_librarys_routing():
    """`cl_mlp_kernel_name` is printed by the code that selects the instance: it runs `cl_launch_mlp`'s own dispatch with a name sink,
    and the leaf that would launch prints its template parameters instead (bench.py labels its roofline row with it): the
    CLI-default scaler runs lane-per-observation up to 31 metadata columns and any number of MC samples, other depths / widths 11-15
    on the narrow kernel, everything else on the 16- / 32- / 64-wide fused instances.  Host function: no GPU needed."""
    import ctypes as C
    import itertools
    from careless_amd import _lib
    lib = _lib.get_lib()
    # the family of the name of every route ("elbo_mlp_kernel<" for the others)
    family = {_lib.CL_ROUTE_NONE: "(unsupported)", _lib.CL_ROUTE_LANE: "elbo_lane_kernel<", _lib.CL_ROUTE_LANE_IMGL: "elbo_lane_kernel<",
              _lib.CL_ROUTE_LANE_BLOCK: "elbo_lane_kernel<", _lib.CL_ROUTE_NARROW: "elbo_narrow_kernel<"}

    def name(mode=0, **kw):
        a = _lib.MlpArgs()
        for k, v in kw.items():
            setattr(a, k, v)
        buf = C.create_string_buffer(128)
        n = lib.cl_mlp_kernel_name(C.byref(a), mode, buf, 128)
        assert n == len(buf.value)
        r = _lib.mlp_route(lib, mode, **kw)
        assert buf.value.decode().startswith(family.get(r, "elbo_mlp_kernel<")), (r, buf.value)
        return buf.value.decode()

    def route(mode=0, **kw):
        return _lib.mlp_route(lib, mode, **kw)

    # (last argument: the instance with / without the optional inputs and outputs -- injected noise, ipred_out, Ev11)
    assert name(d=5, w=10, L=20, S=1) == "elbo_lane_kernel<10, 8, false, false>"
    assert name(d=5, w=10, L=20, S=1, eta=1) == "elbo_lane_kernel<10, 8, false, true>"
    assert name(d=12, w=7, L=20, S=3) == "elbo_lane_kernel<8, 15, false, false>"
    assert name(d=21, w=10, L=20, S=8) == "elbo_lane_kernel<10, 0, false, false>"   # positional encodings: rows of an LDS buffer
    assert name(d=31, w=4, L=20, S=40, row_map=1) == "elbo_lane_kernel<4, 0, true, true>"
    assert name(d=32, w=10, L=20, S=1).startswith("elbo_mlp_kernel<16, 32, 20, 0")
    assert name(d=5, w=13, L=12, S=8) == "elbo_narrow_kernel<2, 4, 8, false>"
    # other depths than the default at widths 7 .. 10 (round 6): the lane kernel compiled for that depth, widest instance
    assert name(d=5, w=10, L=12, S=1) == "elbo_lane_kernel<10, 15, false, false, false, 0, 12>"
    assert name(d=12, w=7, L=2, S=3, eta=1) == "elbo_lane_kernel<8, 15, false, true, false, 0, 2>"
    assert name(d=6, w=9, L=19, S=1, row_map=1) == "elbo_lane_kernel<10, 15, true, true, false, 0, 19>"
    assert name(d=5, w=6, L=12, S=1) == "elbo_lane_kernel<8, 15, false, false, false, 0, 12>"
    assert name(d=5, w=4, L=12, S=1).startswith("elbo_narrow_kernel<")                 # narrower than 5: the narrow kernel's two-step instance
    assert name(d=21, w=10, L=12, S=1).startswith("elbo_mlp_kernel<16, 32, 20, 0")     # (more than 15 columns without the engine's peeled first layer)
    assert name(d=5, w=10, L=1, S=1).startswith("elbo_narrow_kernel<")
    # widths 11 and 12 with the metadata in registers (round 6): the twelve-wide instances; on 16 .. 31 columns the next kernel down
    assert name(d=5, w=12, L=20, S=1) == "elbo_lane_kernel<12, 8, false, false>"
    assert name(d=12, w=11, L=14, S=2, row_map=1) == "elbo_lane_kernel<12, 15, true, true, false, 0, 14>"
    assert name(d=21, w=12, L=20, S=1).startswith("elbo_mlp_kernel<16, 32, 20, 0")
    # per-image layers (packed by image): the lane kernel's instances at the default depth and (round 6) at 2 .. 19 layers of width 5 .. 10
    imgl = dict(n_imgl=2, row_map=1, imgl=1, d_imgl=1, tile_img=1, n_images=7, use_img=0)
    assert name(d=5, w=10, L=20, S=2, **imgl) == "elbo_lane_kernel<10, 8, true, false, false, 2> (image layers)"
    assert name(d=10, w=10, L=20, S=2, dZ0_out=1, **imgl) == "elbo_lane_kernel<10, 15, true, false, true, 2> (image layers)"
    assert name(d=5, w=10, L=10, S=2, **imgl) == "elbo_lane_kernel<10, 15, true, false, false, 2, 10> (image layers)"
    assert name(d=7, w=7, L=3, S=1, ev11=1, **dict(imgl, n_imgl=1)) == "elbo_lane_kernel<10, 15, true, true, false, 1, 3> (image layers)"
    assert name(d=5, w=4, L=10, S=2, **imgl).startswith("elbo_mlp_kernel<16, 8, 24, 0, image layers")
    assert name(d=5, w=10, L=20, S=2, **dict(imgl, n_imgl=3)) == "elbo_lane_kernel<10, 15, true, false, false, 3> (image layers)"     # (three: the default depth only)
    assert name(d=5, w=10, L=12, S=2, **dict(imgl, n_imgl=3)) == "elbo_lane_kernel<10, 15, true, false, false, 3, 12> (image layers)"
    assert name(d=8, w=9, L=12, S=2, dZ0_out=1, **dict(imgl, n_imgl=3)) == "elbo_lane_kernel<10, 15, true, true, false, 3, 12> (image layers)"
    assert name(d=5, w=10, L=20, S=2, **dict(imgl, n_imgl=4)).startswith("elbo_mlp_kernel<16, 8, 24, 0, image layers")
    # width <= 15 on more than 32 columns: the training launch takes the 32-wide instance (the 16-wide one is withdrawn), the forward-only launch keeps it
    assert name(d=36, w=11, L=2, S=2, **imgl) == "elbo_mlp_kernel<32, 64, 5, 0, image layers, KS=4>"
    assert name(d=50, w=13, L=8, S=2, **dict(imgl, n_imgl=1)) == "elbo_mlp_kernel<32, 64, 10, 0, image layers, KS=4>"
    assert name(d=36, w=11, L=2, S=2, mode=1, **imgl) == "elbo_mlp_kernel<16, 64, 24, 1, image layers, KS=4>"
    # ... in deterministic mode (round 6): the lane instances only
    assert name(d=5, w=10, L=20, S=2, dzf_obs=1, **imgl) == "elbo_lane_kernel<10, 8, true, true, false, 2> (image layers) (deterministic stores)"
    assert name(d=5, w=10, L=7, S=2, dzf_obs=1, **imgl) == "elbo_lane_kernel<10, 15, true, true, false, 2, 7> (image layers) (deterministic stores)"
    assert name(d=5, w=32, L=2, S=2, dzf_obs=1, **imgl) == "(unsupported)"
    assert name(d=21, w=64, L=5, S=8) == "elbo_mlp_kernel<64, 32, 5, 0, KS=4>"
    assert name(d=21, w=64, L=5, S=8, mode=1) == "elbo_mlp_kernel<64, 32, 5, 1, KS=4>"
    assert name(d=5, w=10, L=20, S=1, act_out=1, mode=1) == "elbo_lane_kernel<10, 8, false, false, false, 0, 20, 1>"      # (a block launch: every parameter, the mode last)
    assert lib.cl_mlp_kernel_name(None, 0, C.create_string_buffer(8), 8) < 0
    # the route beside the name (cl_mlp_route: the launcher cl_launch_mlp hands the launch to)
    assert route(d=5, w=10, L=20, S=1) == route(d=31, w=4, L=20, S=40, row_map=1) == route(d=6, w=9, L=19, S=1, row_map=1) == _lib.CL_ROUTE_LANE
    assert route(d=5, w=13, L=12, S=8) == route(d=5, w=4, L=12, S=1) == route(d=5, w=10, L=1, S=1) == _lib.CL_ROUTE_NARROW
    assert route(d=32, w=10, L=20, S=1) == route(d=21, w=64, L=5, S=8) == route(d=21, w=64, L=5, S=8, mode=1) == _lib.CL_ROUTE_MLP
    assert route(d=5, w=10, L=20, S=2, **imgl) == route(d=5, w=10, L=7, S=2, dzf_obs=1, **imgl) == _lib.CL_ROUTE_LANE_IMGL
    assert route(d=5, w=4, L=10, S=2, **imgl) == route(d=36, w=11, L=2, S=2, **imgl) == _lib.CL_ROUTE_MLP_IMGL
    assert route(d=5, w=10, L=20, S=1, act_out=1, mode=1) == _lib.CL_ROUTE_LANE_BLOCK
    assert route(d=5, w=14, L=20, S=1, act_out=1, mode=1) == route(d=14, w=14, L=4, S=1, dH_ext=1, dX_out=1, mode=2) == _lib.CL_ROUTE_MLP_CHAIN
    assert route(d=40, w=20, L=10, S=1, row_map=1) == _lib.CL_ROUTE_MLP_PACKED
    assert route(d=40, w=20, L=10, S=1, dzf_obs=1) == _lib.CL_ROUTE_MLP_DET
    assert route(d=40, w=20, L=10, S=1, dzf_obs=1, row_map=1) == _lib.CL_ROUTE_MLP_PACKED_DET
    assert route(d=10, w=10, L=10, S=1, dzf_obs=1, dX_out=1) == _lib.CL_ROUTE_MLP_CHAIN_DET
    assert route(d=5, w=32, L=2, S=2, dzf_obs=1, **imgl) == _lib.CL_ROUTE_NONE
    assert lib.cl_mlp_route(None, 0) < 0 and route(d=5, w=10, L=20, S=1, mode=3) < 0
    # no route -- "(unsupported)" -- where the call returns -2: wider than 64, deeper than the instance, dZ_0 out off the default scaler's kernels
    assert name(d=5, w=65, L=2, S=1) == name(d=5, w=10, L=25, S=1) == name(d=36, w=10, L=20, S=2, mode=2, **imgl) == "(unsupported)"
    assert name(d=5, w=13, L=30, S=1, dZ0_out=1) == name(d=21, w=64, L=5, S=8, dZ0_out=1) == "(unsupported)"
    # ... and over a grid of shapes, optional buffers and modes: the name's family follows the route, "(unsupported)" iff no route
    flags = ("row_map", "gmeta", "dZ0_out", "act_out", "dH_ext", "dX_out", "dO_ext", "dzf_obs", "ev11")
    seen = set()
    for L, w, d, K, mode, f in itertools.product((1, 2, 12, 19, 20, 24), (4, 10, 12, 15, 16, 32, 64, 65), (5, 12, 21, 36, 65), (0, 2, 3), (0, 1, 2),
                                                (None,) + flags):
        kw = dict(dict(imgl, n_imgl=K) if K else {}, d=d, w=w, L=L, S=2)
        if f:
            kw[f] = 1
        name(mode, **kw)
        seen.add(route(mode, **kw))
    assert seen == set(range(_lib.CL_ROUTE_MLP_CHAIN_DET + 1)) - {_lib.CL_ROUTE_MLP_PACKED_DET, _lib.CL_ROUTE_MLP_CHAIN_DET}   # (two flags each: above)


def test_lane_instance_table_matches_the_record():
    """Which instance the lane kernel's launch layer selects, as data: `scripts/lane_table.py` walks widths, columns and depths on both sides
    of every threshold that layer tests, in every layout, with every optional buffer that picks another form, and the two launches of a
    layer block (31 416 launches), and asks the library for route and name.  tests/golden/lane_instances.json is that record taken on
    the library BEFORE the launch layer was rewritten: every entry equals it.  The one exception are the names of the block launches
    (CL_ROUTE_LANE_BLOCK), which until then carried the label of a chain instance that does not run: their route is the record's, their
    name follows the rule the launch layer implements -- the record holds the names since, so that a later change shows.  Host only."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("lane_table", os.path.join(ROOT, "scripts", "lane_table.py"))
    lane_table = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lane_table)
    assert not [k for k in os.environ if k.startswith(lane_table.SWITCHES)]
    with open(os.path.join(ROOT, "tests", "golden", "lane_instances.json")) as f:
        want = lane_table.decode(json.load(f))
    got = lane_table.table(_lib.get_lib())
    assert len(got) == len(want) == 31416
    differ = [(mode, kw, g, w_) for (mode, kw), g, w_ in zip(lane_table.walk(), got, want) if g != w_]
    assert not differ, (len(differ), differ[:5])
    blocks = 0
    for (mode, kw), (route, name) in zip(lane_table.walk(), got):
        if route != _lib.CL_ROUTE_LANE_BLOCK:
            continue
        blocks += 1
        W = 8 if kw["w"] <= 8 else (10 if kw["w"] <= 10 else 12)
        D = 8 if kw["L"] == 20 and kw["d"] <= 8 else 15
        assert name == f"elbo_lane_kernel<{W}, {D}, false, false, false, 0, {kw['L']}, {mode}>", (mode, kw, name)
    assert blocks > 0


def test_mlp_instance_table_matches_the_record():
    """What the scaler launch layer (csrc/mlp_launch.hip) and the units of csrc/elbo_mlp.hip under it answer, as data: `scripts/mlp_table.py`
    walks widths 8 .. 65, columns 8 .. 65 and depths 1 .. 25 on both sides of every threshold `mlp_geom`, `epi_plain` and `mlp_route`
    test, in every layout, with the options that pick another route, instance or epilogue, and the forward-only / external-gradient
    launches (29 160 launch descriptions), and asks the library for route, epilogue, return code (`cl_mlp_check`, grid 2) and name.
    tests/golden/mlp_instances.json is that record taken on the library BEFORE the layer moved out of the kernel file and the names of
    the seven units moved to the leaf that launches: every entry equals it.  The record reaches every route of elbo_mlp.hip and both plain
    epilogues.  Host only."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("mlp_table", os.path.join(ROOT, "scripts", "mlp_table.py"))
    mlp_table = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mlp_table)
    assert not [k for k in os.environ if k.startswith(mlp_table.SWITCHES)]
    with open(os.path.join(ROOT, "tests", "golden", "mlp_instances.json")) as f:
        want = mlp_table.decode(json.load(f))
    got = mlp_table.table(_lib.get_lib())
    assert len(got) == len(want) == mlp_table.ENTRIES == 29160
    differ = [(mode, kw, g, w_) for (mode, kw), g, w_ in zip(mlp_table.walk(), got, want) if g != w_]
    assert not differ, (len(differ), differ[:5])
    assert {r for r, _, _, _ in want} >= set(range(_lib.CL_ROUTE_MLP, _lib.CL_ROUTE_MLP_CHAIN_DET + 1))
    assert {e for _, e, _, _ in want} >= {_lib.CL_EPI_PLAIN_NORMAL, _lib.CL_EPI_PLAIN_STUDENTT}
    for route, _, _, name in want:          # (the name's family follows the route: a unit of elbo_mlp.hip prints elbo_mlp_kernel<...>)
        assert name.startswith("elbo_mlp_kernel<") == (route >= _lib.CL_ROUTE_MLP), (route, name)


def test_one_argument_check_answers_for_every_route():
    """`cl_mlp_check`: the return code a scaler launch would give, without the launch -- the entry checks of the call, the route, and
    `mlp_check`, the one table of argument checks every route shares (csrc/mlp_launch.hip).  For each of the twelve routes an accepted
    launch and a rejected one per clause that applies to it, with the exact code; precedence: -1 tile / grid, -2 no route, the route's
    -1 clauses, the -4 bounds.  Pointer fields are only tested against NULL and nothing is launched: holds with or without a GPU."""
    import ctypes as C
    from careless_amd import _lib
    lib = _lib.get_lib()
    mode_base = {0: dict(refl_id=1, iobs=1, sig=1, z_f=1, dz_f=1, partials=1, scalars=1), 1: dict(loc_out=1, sig_out=1), 2: dict(dO_ext=1, partials=1)}
    drop = object()

    def check(route, code, mode=0, grid=4, **kw):
        f = dict(mode_base[mode], meta_t=1, mlp=1, n_obs=256, n_pad=256, S=2, R=50)
        f.update(kw)
        f = {k: v for k, v in f.items() if v is not drop}
        assert _lib.mlp_route(lib, mode, **f) == route, (route, mode, kw)
        assert lib.cl_mlp_check(C.byref(_lib.MlpArgs(**f)), mode, grid) == code, (route, code, mode, kw)

    BIG_S = 1 << 22                     # n_pad * S * 4 = 2^32 at n_pad = 256: the per-(observation, sample) arrays
    BIG_R = 1 << 29                     # R * S * 4 = 2^32 at S = 2: z_f / dz_f
    BIG_N = 128 << 20                   # n_pad * 8 metadata rows * 4 = 2^32 (a multiple of the tile; R * S and n_pad * S stay below)
    big_n = dict(n_obs=BIG_N, n_pad=BIG_N, S=1)
    imgl = dict(n_imgl=2, row_map=1, imgl=1, d_imgl=1, tile_img=1, n_images=7, use_img=0)
    det = dict(dzf_obs=1, nll_part=1)
    lane, narrow, mlp = dict(d=5, w=10, L=20), dict(d=5, w=13, L=12), dict(d=40, w=20, L=10)

    assert lib.cl_mlp_check(None, 0, 4) < 0
    assert lib.cl_mlp_check(C.byref(_lib.MlpArgs(meta_t=1, mlp=1, n_obs=256, n_pad=256, d=5, w=10, L=20)), 3, 4) == -1       # no such mode
    # the entry checks and tile / grid validity come first: -1 whatever the route, CL_ROUTE_NONE included
    check(_lib.CL_ROUTE_LANE, -1, z_f=drop, **lane)
    check(_lib.CL_ROUTE_LANE, -1, n_pad=300, **lane)
    check(_lib.CL_ROUTE_LANE, -1, n_obs=0, **lane)
    check(_lib.CL_ROUTE_LANE, -1, grid=0, **lane)
    check(_lib.CL_ROUTE_NONE, -1, grid=0, d=5, w=65, L=2)
    check(_lib.CL_ROUTE_NONE, -2, d=5, w=65, L=2)
    check(_lib.CL_ROUTE_NONE, -2, S=BIG_S, d=5, w=65, L=2)
    check(_lib.CL_ROUTE_NONE, -2, ev11=1, **det, **lane)             # (the Evans-2011 gradients need their per-wave slots: no route)
    # the lane and the narrow kernel: plain and packed layout, deterministic stores
    for route, shape in ((_lib.CL_ROUTE_LANE, lane), (_lib.CL_ROUTE_NARROW, narrow)):
        check(route, 0, **shape)
        check(route, 0, grid=1000, **shape)                        # (a grid larger than the tiles is clamped, not refused)
        check(route, 0, row_map=1, gmeta=1, tile_gmax=1, eta=1, **shape)
        check(route, 0, use_img=1, image_id=1, img=1, d_img=1, dimg_obs=1, ev11=1, ev11_part=1, **det, **shape)
        check(route, -1, row_map=1, n_obs=200, **shape)
        check(route, -1, row_map=1, gmeta=1, **shape)
        check(route, -1, dzf_obs=1, **shape)                       # no nll_part
        check(route, -1, use_img=1, image_id=1, img=1, d_img=1, **det, **shape)       # no dimg_obs
        check(route, -4, **big_n, **shape)
        check(route, -4, R=BIG_R, **shape)
        check(route, 0, S=BIG_S, R=1, **shape)                     # plain layout, atomics: no array of n_pad * S elements is addressed
        check(route, 0, S=BIG_S, R=1, row_map=1, **shape)
        check(route, -4, S=BIG_S, R=1, row_map=1, eta=1, **shape)
        check(route, -4, S=BIG_S, R=1, row_map=1, ipred_out=1, **shape)
        check(route, -4, S=BIG_S, R=1, **det, **shape)
        check(route, -1, S=BIG_S, R=1, dzf_obs=1, **shape)         # precedence: a bound crossed AND nll_part missing -> -1
        check(route, -1, R=BIG_R, dzf_obs=1, **shape)
        check(route, -1, R=BIG_R, row_map=1, n_obs=200, **shape)    # ... the same for a packed-layout clause
    # ... with per-image layers
    check(_lib.CL_ROUTE_LANE_IMGL, 0, eta=1, **lane, **imgl)
    check(_lib.CL_ROUTE_LANE_IMGL, 0, **det, **lane, **imgl)
    check(_lib.CL_ROUTE_LANE_IMGL, -1, n_obs=200, **lane, **imgl)
    check(_lib.CL_ROUTE_LANE_IMGL, -1, dzf_obs=1, **lane, **imgl)
    check(_lib.CL_ROUTE_LANE_IMGL, -4, **big_n, **lane, **imgl)
    check(_lib.CL_ROUTE_LANE_IMGL, -4, R=BIG_R, **lane, **imgl)
    check(_lib.CL_ROUTE_LANE_IMGL, 0, S=BIG_S, R=1, **lane, **imgl)
    check(_lib.CL_ROUTE_LANE_IMGL, -4, S=BIG_S, R=1, ipred_out=1, **lane, **imgl)
    check(_lib.CL_ROUTE_LANE_IMGL, -4, S=BIG_S, R=1, **det, **lane, **imgl)
    check(_lib.CL_ROUTE_LANE_IMGL, -1, S=BIG_S, R=1, dzf_obs=1, **lane, **imgl)
    # ... a head-less layer block: forward (act_out) and backward (dH_ext); it reads no reflection, so R * S is no bound of it
    check(_lib.CL_ROUTE_LANE_BLOCK, 0, mode=1, act_out=1, loc_out=drop, sig_out=drop, **lane)
    check(_lib.CL_ROUTE_LANE_BLOCK, 0, mode=2, dH_ext=1, dO_ext=drop, **lane)
    check(_lib.CL_ROUTE_LANE_BLOCK, 0, mode=2, dH_ext=1, dO_ext=drop, R=BIG_R, **lane)
    check(_lib.CL_ROUTE_LANE_BLOCK, -1, mode=1, grid=0, act_out=1, loc_out=drop, sig_out=drop, **lane)
    check(_lib.CL_ROUTE_LANE_BLOCK, -4, mode=1, act_out=1, loc_out=drop, sig_out=drop, **big_n, **lane)
    # the 16- / 32- / 64-wide units: plain layout
    for mode in (0, 1, 2):
        check(_lib.CL_ROUTE_MLP, 0, mode=mode, **mlp)
        check(_lib.CL_ROUTE_MLP, -1, mode=mode, n_pad=300, **mlp)
        check(_lib.CL_ROUTE_MLP, -4, mode=mode, R=BIG_R, **mlp)
        check(_lib.CL_ROUTE_MLP, -4, mode=mode, **big_n, **dict(mlp, d=5))
    check(_lib.CL_ROUTE_MLP, 0, S=BIG_S, R=1, eta=1, **mlp)
    # ... packed layout
    check(_lib.CL_ROUTE_MLP_PACKED, 0, row_map=1, gmeta=1, tile_gmax=1, ipred_out=1, **mlp)
    check(_lib.CL_ROUTE_MLP_PACKED, 0, mode=1, row_map=1, **mlp)
    check(_lib.CL_ROUTE_MLP_PACKED, -1, row_map=1, n_obs=200, **mlp)
    check(_lib.CL_ROUTE_MLP_PACKED, -1, row_map=1, n_imgl=-1, **mlp)
    check(_lib.CL_ROUTE_MLP_PACKED, -1, row_map=1, gmeta=1, **mlp)
    check(_lib.CL_ROUTE_MLP_PACKED, -1, mode=1, row_map=1, gmeta=1, tile_gmax=1, **mlp)      # group sizes: the full step only
    check(_lib.CL_ROUTE_MLP_PACKED, 0, S=BIG_S, R=1, row_map=1, **mlp)
    check(_lib.CL_ROUTE_MLP_PACKED, -4, S=BIG_S, R=1, row_map=1, eta=1, **mlp)
    check(_lib.CL_ROUTE_MLP_PACKED, -4, R=BIG_R, row_map=1, **mlp)
    check(_lib.CL_ROUTE_MLP_PACKED, -4, row_map=1, **big_n, **dict(mlp, d=5))
    # ... per-image layers
    wide_imgl = dict(imgl, **dict(mlp, L=4))
    check(_lib.CL_ROUTE_MLP_IMGL, 0, gmeta=1, tile_gmax=1, **wide_imgl)
    check(_lib.CL_ROUTE_MLP_IMGL, 0, mode=1, **dict(wide_imgl, d_imgl=0))
    check(_lib.CL_ROUTE_MLP_IMGL, -1, **dict(wide_imgl, row_map=0))
    check(_lib.CL_ROUTE_MLP_IMGL, -1, n_obs=200, **wide_imgl)
    for missing in (dict(imgl=0), dict(tile_img=0), dict(n_images=0), dict(use_img=1, image_id=1, img=1, d_img=1), dict(d_imgl=0)):
        check(_lib.CL_ROUTE_MLP_IMGL, -1, **dict(wide_imgl, **missing))
    check(_lib.CL_ROUTE_MLP_IMGL, -1, gmeta=1, **wide_imgl)
    check(_lib.CL_ROUTE_MLP_IMGL, -1, mode=1, gmeta=1, tile_gmax=1, **wide_imgl)
    check(_lib.CL_ROUTE_MLP_IMGL, -4, S=BIG_S, R=1, ipred_out=1, **wide_imgl)
    check(_lib.CL_ROUTE_MLP_IMGL, -4, R=BIG_R, **wide_imgl)
    check(_lib.CL_ROUTE_MLP_IMGL, -4, **big_n, **dict(wide_imgl, d=5))
    # ... a block of a layer-block chain: activations leave the forward launch, the gradient enters the backward one
    chain = dict(d=5, w=14, L=20)
    check(_lib.CL_ROUTE_MLP_CHAIN, 0, mode=1, act_out=1, loc_out=drop, sig_out=drop, **chain)
    check(_lib.CL_ROUTE_MLP_CHAIN, 0, mode=2, dH_ext=1, dX_out=1, dO_ext=drop, **chain)
    check(_lib.CL_ROUTE_MLP_CHAIN, 0, dX_out=1, **chain)
    check(_lib.CL_ROUTE_MLP_CHAIN, -1, mode=0, act_out=1, **chain)
    check(_lib.CL_ROUTE_MLP_CHAIN, -1, mode=2, act_out=1, **chain)
    check(_lib.CL_ROUTE_MLP_CHAIN, -1, mode=0, dH_ext=1, **chain)
    check(_lib.CL_ROUTE_MLP_CHAIN, -1, mode=1, dH_ext=1, **chain)
    check(_lib.CL_ROUTE_MLP_CHAIN, -4, dX_out=1, R=BIG_R, **chain)
    check(_lib.CL_ROUTE_MLP_CHAIN, -4, dX_out=1, **big_n, **chain)
    # ... the deterministic compilations: every store target, and the per-(observation, sample) records below 4 GiB
    for route, kw in ((_lib.CL_ROUTE_MLP_DET, mlp), (_lib.CL_ROUTE_MLP_PACKED_DET, dict(mlp, row_map=1)), (_lib.CL_ROUTE_MLP_CHAIN_DET, dict(d=10, w=10, L=10, dX_out=1))):
        check(route, 0, **det, **kw)
        check(route, 0, use_img=1, image_id=1, img=1, d_img=1, dimg_obs=1, ev11=1, ev11_part=1, **det, **kw)
        check(route, -1, dzf_obs=1, **kw)
        check(route, -1, use_img=1, image_id=1, img=1, d_img=1, **det, **kw)
        check(route, -4, S=BIG_S, R=1, **det, **kw)
        check(route, -1, S=BIG_S, R=1, dzf_obs=1, **kw)            # precedence again
        check(route, -4, R=BIG_R, **det, **kw)
        check(route, -4, **det, **big_n, **dict(kw, d=5) if route != _lib.CL_ROUTE_MLP_CHAIN_DET else dict(kw, d=5, w=14, L=20))
    check(_lib.CL_ROUTE_MLP_PACKED_DET, -2, n_obs=200, **det, **dict(mlp, row_map=1))     # (this unit has always answered -2 to padding rows)
    check(_lib.CL_ROUTE_MLP_PACKED_DET, -1, gmeta=1, **det, **dict(mlp, row_map=1))
    check(_lib.CL_ROUTE_MLP_PACKED_DET, 0, gmeta=1, tile_gmax=1, **det, **dict(mlp, row_map=1))


def test_scaler_plan_follows_the_routing_tables():
    """`plan_scaler` (host side, no GPU): the peel / chain / layer-by-layer plan of every row of tests/test_routing.py's tables, from the
    library's routes alone -- and the shapes where a launch of the plan would have no route."""
    import subprocess
    import sys
    from careless_amd.engine import plan_scaler
    from tests.test_routing import IMGL_TABLE, TABLE
    lib = _lib.get_lib()
    for L, w, d, frag, peel, blocks, wide in TABLE:
        p = plan_scaler(lib, d, w, L)
        assert (p.peel, None if p.blocks is None else len(p.blocks), p.wide) == (peel, blocks, wide), (L, w, d, p)
        assert p.route == (_lib.CL_ROUTE_NONE if wide else (_lib.CL_ROUTE_LANE if frag.startswith("elbo_lane") else p.route))
    for L, w, d, K, laue, frag, peel in IMGL_TABLE:
        if laue:            # (the Laue generator's own metadata columns)
            d = BaseModel.get_metadata(reference_inputs(util.make_problem(N=600, R=30, L=L, w=w, S=1, laue=True, image_layers=K, n_images=5)[0])).shape[1]
        p = plan_scaler(lib, d, w, L, K, laue=laue)
        assert (p.peel, p.blocks, p.wide) == (peel, None, frag.startswith("wide")), (L, w, d, K, p)
        assert (p.route == _lib.CL_ROUTE_LANE_IMGL) == frag.startswith("elbo_lane")
    # two-pass Laue, `--image-layers 2`, 20 x 10 on more than 32 columns: cl_mlp_backward_ext has no route there (the 32-wide instance holds
    # 10 layers) -- layer by layer; single pass, the same shape runs the lane kernel behind the peeled layer
    assert plan_scaler(lib, 36, 10, 20, 2, laue=True, two_pass=True).wide
    assert plan_scaler(lib, 36, 10, 20, 2, laue=True, gmax=17).wide
    p = plan_scaler(lib, 36, 10, 20, 2, laue=True)
    assert p.peel and not p.wide and p.route == _lib.CL_ROUTE_LANE_IMGL
    # 24 x 12 with the per-depth lane instances switched off: the last block is no lane launch, the chain stays on the 16-wide kernel
    # (a subprocess: the library reads its switches once per process)
    code = ("from careless_amd import _lib; from careless_amd.engine import plan_scaler; "
            "p = plan_scaler(_lib.get_lib(), 5, 12, 24); print(p.chain_lane, [b.l1 - b.l0 for b in p.blocks])")
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CARELESS_HIP_LANE_DEPTHS="0"), cwd=ROOT, capture_output=True,
                         text=True, check=True).stdout.split()
    assert out == ["False", "[12,", "12]"]
    p = plan_scaler(lib, 5, 12, 24)
    assert p.chain_lane and [b.l1 - b.l0 for b in p.blocks] == [5, 19]


def test_wide_path_envelope_queries():
    """Host functions of the layer-by-layer path (no GPU needed): which shapes take the recomputed first layer, the head's backward pass
    fused into the top layer's kernels and the square-layer kernel's envelope, how many partials the fused dgrad + first-layer weight
    gradient writes, the row pitch of the activation buffers."""
    lib = _lib.get_lib()
    assert [lib.cl_wide_ld(w) for w in (1, 4, 70, 128, 129)] == [4, 4, 72, 128, 132] and lib.cl_wide_ld(0) == 0
    # first layer recomputed: at most 15 metadata columns, hidden width at most 128
    assert lib.cl_wide_pre_supported(5, 128) == 1 and lib.cl_wide_pre_supported(15, 65) == 1
    assert lib.cl_wide_pre_supported(16, 128) == 0 and lib.cl_wide_pre_supported(5, 129) == 0 and lib.cl_wide_pre_supported(0, 64) == 0
    # fused head backward: square layers of 5 .. 8 sixteen-column blocks on both sides (widths 65 .. 128, same block count)
    assert lib.cl_wide_head_bwd_supported(128, 128) == 1 and lib.cl_wide_head_bwd_supported(65, 80) == 1 and lib.cl_wide_head_bwd_supported(96, 90) == 1
    assert lib.cl_wide_head_bwd_supported(64, 64) == 0 and lib.cl_wide_head_bwd_supported(129, 129) == 0 and lib.cl_wide_head_bwd_supported(96, 128) == 0
    # one partial per workgroup of the streaming kernel: eight 16-row blocks per workgroup, two workgroups per CU at most
    assert lib.cl_wide_dgrad_wgrad0_parts(0) == 0 and lib.cl_wide_dgrad_wgrad0_parts(1) == 1 and lib.cl_wide_dgrad_wgrad0_parts(16 * 8 * 3 + 1) == 4
    big = lib.cl_wide_dgrad_wgrad0_parts(10_000_000)
    assert big % 2 == 0 and 2 <= big <= 4096 and lib.cl_wide_dgrad_wgrad0_parts(100_000_000) == big
    # weight-gradient splits: at least 512 observations each, at most 512 of them
    assert lib.cl_wide_wgrad_splits(1) == 1 and lib.cl_wide_wgrad_splits(513) == 2 and lib.cl_wide_wgrad_splits(10_000_000) == 512
    # the new entry points refuse missing buffers before touching a device
    assert lib.cl_slot_rows(None, None) == -1
    assert lib.cl_wide_dense_dgrad_head(None, 128, None, None, None, None, 100, 128, 128, None, 128, 0.01, None, 128, None, None) == -1
    assert lib.cl_wide_dense_wgrad_head(None, 128, None, None, None, 0.01, None, 128, 100, 128, 128, None, None, 1, None, None) == -1
    assert lib.cl_wide_dense_dgrad_pre_wgrad0(None, 128, None, 100, 128, 128, None, 8, 5, None, None, 0.01, None, None, None) == -1


def test_wide_entry_points_answer_without_a_launch():
    """The -2 (shape outside the kernel's envelope) and -1 (bad layout) answers of the layer-by-layer entry points that are given before
    anything is launched or dereferenced: the pointers below are made-up addresses.  That is safe only while each of these checks stays
    ahead of the launch in csrc/wide_gemm.hip (every call below was read against it: all return before hipLaunchKernelGGL) -- whoever
    reorders an entry check must keep it so, or this test launches on a bogus pointer where a device is present."""
    lib = _lib.get_lib()
    p, off = 0x10000, 0x10004                        # 16-byte aligned / 4 bytes off
    # the top layer with the head in its epilogue: layers up to 128 x 128
    for n_in, n_out in ((129, 64), (64, 129)):
        assert lib.cl_wide_dense_forward_head(p, 132, p, p, 100, n_in, n_out, 0.01, p, 132, p, 0, 1e-7, p, p, None, None, None) == -2
    # the head's backward pass inside the top layer's dgrad: the square-layer envelope (65 .. 128, same number of 16-column blocks)
    for n_out, n_in in ((96, 128), (64, 64), (129, 129), (128, 60)):
        assert lib.cl_wide_dense_dgrad_head(p, 132, p, p, p, p, 100, n_out, n_in, p, 132, 0.01, p, 132, None, None) == -2
    # the recomputed first layer takes at most 15 metadata columns
    assert lib.cl_wide_dense_wgrad_pre(p, 128, p, 16, 16, p, p, 0.01, 100, 128, 128, p, 1, None, None) == -2
    assert lib.cl_wide_dense_wgrad_pre(p, 128, off, 16, 15, p, p, 0.01, 100, 128, 128, p, 1, None, None) == -1      # (X0 off 16-byte alignment)
    # the head's backward pass reads H and writes dZ as float4: pitch a multiple of 4, 16-byte aligned, width at most 1024
    assert lib.cl_wide_head_backward(p, 128, p, p, 100, 128, 0, 1e-7, 0.01, off, 128, p, 1, None, None) == -1
    assert lib.cl_wide_head_backward(off, 128, p, p, 100, 128, 0, 1e-7, 0.01, p, 128, p, 1, None, None) == -1
    assert lib.cl_wide_head_backward(p, 128, p, p, 100, 126, 0, 1e-7, 0.01, p, 126, p, 1, None, None) == -1
    assert lib.cl_wide_head_backward(p, 1028, p, p, 100, 1025, 0, 1e-7, 0.01, p, 1028, p, 1, None, None) == -2
    _wide_rejections(lib)


def _wide_rejections(lib):
    """Every launching cl_wide_* entry point, one rejecting call per clause its checks distinguish: a missing pointer, the row-count
    bounds (n = 0; n = 2^31 where the entry point bounds it -- cl_wide_head_forward, cl_wide_image_forward / _dgrad and the _tiles pair
    do not, so that call is NOT made for them: it would launch), a pitch below the width, every -2 envelope edge, every alignment /
    pitch-multiple clause, and which of -1 and -2 answers when both apply.  Per entry point: its parameter names in C order, a call the
    library would ACCEPT (never made), and (expected answer, what to change in it) pairs."""
    import ctypes as C
    p, off, big = 0x10000, 0x10004, 1 << 31

    def rejects(name, params, base, cases):
        fn, params = getattr(lib, name), params.split()
        assert sorted(params) == sorted(base), name
        for want, over in cases:
            assert set(over) <= set(base), (name, over)
            a = dict(base, **over)
            got = fn(*[a[k] for k in params])
            assert got == want, (name, over, got, want)

    def nulls(*names):
        return [(-1, {k: None}) for k in names]

    row = [(-1, dict(n=0)), (-1, dict(n=-5)), (-1, dict(n=big))]
    com = dict(n=100, leak=0.01, stop=None, st=None)

    rejects("cl_wide_dense_forward", "X ldx Wt b n n_in n_out leak act Y ldy stop st",
            dict(com, X=p, ldx=128, Wt=p, b=p, n_in=128, n_out=128, act=1, Y=p, ldy=128),
            nulls("X", "Wt", "b", "Y") + row + [(-1, dict(n_in=0)), (-1, dict(n_out=0)), (-1, dict(ldx=127)), (-1, dict(ldy=127)),
                                              (-1, dict(n_in=200, n_out=200, ldx=200, ldy=199)), (-1, dict(n_in=200, ldx=199))])
    fh = dict(com, X=p, ldx=128, Wt=p, b=p, n_in=128, n_out=128, Y=p, ldy=128, head=p, bij=0, eps=1e-7, loc=p, sig=p, dsd=None)
    fh_cases = (nulls("X", "Wt", "b", "Y", "head", "loc", "sig") + row +
                [(-1, dict(n_in=0)), (-1, dict(n_out=0)), (-1, dict(ldx=127)), (-1, dict(ldy=127)),
                 (-2, dict(n_in=129, ldx=132)), (-2, dict(n_out=129, ldy=132)), (-2, dict(n_in=129, n_out=129, ldx=132, ldy=132)),
                 (-1, dict(n_in=129, ldx=132, X=None)), (-1, dict(n_out=129, ldy=128)), (-1, dict(n_in=129, ldx=132, n=0))])
    rejects("cl_wide_dense_forward_head", "X ldx Wt b n n_in n_out leak Y ldy head bij eps loc sig dsd stop st", fh, fh_cases)

    # ... with the slot likelihood: the host reads the argument block, so a real (zeroed, then filled with made-up addresses) one
    blocks = []

    def lik(**over):
        a = _lib.LaueArgs()
        blocks.append(a)
        for k in ("refl_id", "iobs", "sig", "z_f", "dz_f", "dO", "scalars"):
            setattr(a, k, p)
        a.S, a.n_obs = 4, 100
        for k, v in over.items():
            setattr(a, k, v)
        return C.pointer(a)

    fl = dict(fh, lik=lik())
    rejects("cl_wide_dense_forward_head_lik", "X ldx Wt b n n_in n_out leak Y ldy head bij eps loc sig dsd lik stop st", fl,
            fh_cases + [(-1, dict(lik=None)), (-2, dict(n_in=129, ldx=132, lik=lik(S=0)))] +         # the shared check comes first
            # what the fused epilogue declines: harmonics, injected noise, predictions out, Evans-2011 terms, the deterministic stores
            [(-2, dict(lik=lik(**{k: p}))) for k in ("harmonic_id", "eta", "ipred_out", "ev11", "dzf_obs", "nll_part")] +
            [(-2, dict(lik=lik(eta=p, refl_id=None)))] +                                            # (declined before the block is judged)
            [(-1, dict(lik=lik(**{k: None}))) for k in ("refl_id", "iobs", "sig", "z_f", "dz_f", "dO", "scalars")] +
            [(-1, dict(lik=lik(S=0))), (-1, dict(lik=lik(n_obs=99))), (-1, dict(lik=lik(use_img=1))),
             (-1, dict(lik=lik(use_img=1, image_id=p, img=p))), (-1, dict(lik=lik(use_img=1, image_id=p, d_img=p))),
             (-1, dict(lik=lik(use_img=1, img=p, d_img=p))), (-1, dict(lik=lik(S=0), n_in=64, ldx=64))] +
            # the square-layer kernel's envelope: 5 .. 8 blocks, the same on both sides, pitches multiples of 4 inside the blocks, aligned
            [(-2, dict(n_in=64, ldx=64)), (-2, dict(n_out=64, ldy=64)), (-2, dict(n_in=64, n_out=64, ldx=64, ldy=64)),
             (-2, dict(n_in=96, ldx=96)), (-2, dict(n_in=100, n_out=100, ldx=101, ldy=100)), (-2, dict(n_in=100, n_out=100, ldx=100, ldy=102)),
             (-2, dict(n_in=100, n_out=100, ldx=116, ldy=100)), (-2, dict(n_in=100, n_out=100, ldx=100, ldy=116)),
             (-2, dict(ldx=132)), (-2, dict(ldy=132)), (-2, dict(X=off)), (-2, dict(Y=off))])

    w100 = dict(n_out=100, n_in=100, ldt=100, ldo=100, ldh=100)     # (seven blocks a side: row buffers of 100 .. 112 floats)
    dh = dict(com, Htop=p, ldt=128, head=p, dO=p, dsd=p, Wt=p, n_out=128, n_in=128, Hprev=p, ldh=128, dX=p, ldo=128)
    rejects("cl_wide_dense_dgrad_head", "Htop ldt head dO dsd Wt n n_out n_in Hprev ldh leak dX ldo stop st", dh,
            nulls("Htop", "head", "dO", "dsd", "Wt", "dX") + row +
            [(-1, dict(n_in=0)), (-1, dict(n_out=0)), (-1, dict(ldt=127)), (-1, dict(ldo=127)), (-1, dict(n_out=129, ldt=128)),
             (-2, dict(n_out=129, ldt=132)), (-2, dict(n_out=64)), (-2, dict(n_out=64, n_in=64)), (-2, dict(n_out=96)), (-2, dict(n_in=96)),
             (-1, dict(n_out=64, n_in=64, dX=None)),
             (-2, dict(w100, ldt=101)), (-2, dict(w100, ldo=102)), (-2, dict(w100, ldh=106)), (-2, dict(w100, ldo=116)), (-2, dict(w100, ldt=116)),
             (-2, dict(w100, ldh=116)), (-2, dict(ldt=132)), (-2, dict(ldo=132)), (-2, dict(ldh=132)), (-2, dict(Htop=off)), (-2, dict(dX=off)),
             (-2, dict(Hprev=off)), (-2, dict(ldh=126))])

    rejects("cl_wide_dense_dgrad", "dZ lddz Wt n n_out n_in Hprev ldh leak dX ldo stop st",
            dict(com, dZ=p, lddz=128, Wt=p, n_out=128, n_in=128, Hprev=p, ldh=128, dX=p, ldo=128),
            nulls("dZ", "Wt", "dX") + row + [(-1, dict(n_in=0)), (-1, dict(n_out=0)), (-1, dict(lddz=127)), (-1, dict(ldo=127)),
                                            (-1, dict(n_out=200, lddz=199)), (-1, dict(n_in=200, ldo=199))])

    # the recomputed first layer (pre_check): pointers, then the envelope (1 .. 15 metadata columns, width 1 .. 128), then the metadata's layout
    pre = dict(X0=p, ldx0=8, n_in0=5, Wt0=p, b0=p)

    def pre_cases(width):
        return (nulls("X0", "Wt0", "b0") +
                [(-2, dict(n_in0=16, ldx0=16)), (-2, dict(n_in0=0)), (-2, {width: 129}), (-2, {width: 0}), (-1, dict(n_in0=16, ldx0=16, X0=None)),
                 (-1, dict(ldx0=4)), (-1, dict(n_in0=6, ldx0=7)), (-1, dict(ldx0=20)), (-1, dict(X0=off)), (-2, dict(n_in0=16, ldx0=4, X0=off))])

    rejects("cl_wide_dense2_forward", "X0 ldx0 n_in0 Wt0 b0 Wt1 b1 n w0 w1 leak Y ldy head bij eps loc sig stop st",
            dict(com, **pre, Wt1=p, b1=p, w0=128, w1=128, Y=p, ldy=128, head=p, bij=0, eps=1e-7, loc=p, sig=p),
            pre_cases("w0") + nulls("Wt1", "b1", "Y", "loc", "sig") + row +
            [(-1, dict(w1=0)), (-1, dict(ldy=127)), (-2, dict(w1=129, ldy=132)), (-1, dict(w1=129, ldy=128)), (-1, dict(w1=129, ldy=132, Y=None)),
             (-2, dict(w1=129, ldy=132, loc=None)), (-2, dict(n_in0=16, ldx0=16, Y=None)), (-2, dict(w0=129, n=0))])
    rejects("cl_wide_dense_dgrad_pre", "dZ lddz Wt n n_out n_in X0 ldx0 n_in0 Wt0 b0 leak dX ldo stop st",
            dict(com, **pre, dZ=p, lddz=128, Wt=p, n_out=128, n_in=128, dX=p, ldo=128),
            pre_cases("n_in") + nulls("dZ", "Wt", "dX") + row +
            [(-1, dict(n_out=0)), (-1, dict(lddz=127)), (-1, dict(ldo=127)), (-2, dict(n_out=129, lddz=132)), (-1, dict(n_out=129, lddz=128)),
             (-1, dict(n_out=129, lddz=132, dX=None)), (-2, dict(n_in0=16, ldx0=16, dX=None))])
    rejects("cl_wide_dense_dgrad_pre_wgrad0", "dZ lddz Wt n n_out n_in X0 ldx0 n_in0 Wt0 b0 leak partials stop st",
            dict(com, **pre, dZ=p, lddz=128, Wt=p, n_out=128, n_in=128, partials=p),
            pre_cases("n_in") + nulls("dZ", "Wt", "partials") + row +
            [(-1, dict(n_out=0)), (-1, dict(lddz=127)), (-2, dict(n_out=129, lddz=132)), (-1, dict(n_out=129, lddz=128)),
             (-1, dict(n_out=129, lddz=132, partials=None)),
             # the square-layer envelope; the rows of dZ are read at the width of BOTH sides of the layer: the pitch covers n_in too
             (-2, dict(n_out=64, n_in=64, lddz=64)), (-2, dict(n_out=64)), (-2, dict(n_in=64)), (-2, dict(n_out=96)), (-2, dict(n_in=96)),
             (-2, dict(n_out=100, n_in=110, lddz=104)), (-2, dict(n_out=100, n_in=110, lddz=108)), (-2, dict(n_out=100, n_in=100, lddz=101)),
             (-2, dict(n_out=100, n_in=100, lddz=116)), (-2, dict(lddz=132)), (-2, dict(dZ=off))])
    rejects("cl_wide_dense_wgrad_pre", "dZ lddz X0 ldx0 n_in0 Wt0 b0 leak n n_out n_in partials nsplit stop st",
            dict(com, **pre, dZ=p, lddz=128, n_out=128, n_in=128, partials=p, nsplit=1),
            pre_cases("n_in") + nulls("dZ", "partials") + row +
            [(-1, dict(n_out=0)), (-1, dict(nsplit=0)), (-1, dict(lddz=127)), (-2, dict(n_out=129, lddz=132)), (-1, dict(n_out=129, lddz=128)),
             (-1, dict(n_out=129, lddz=132, nsplit=0)), (-2, dict(n_in=129, dZ=None))])

    rejects("cl_wide_dense_wgrad", "dZ lddz H ldh n n_out n_in partials nsplit stop st",
            dict(n=100, stop=None, st=None, dZ=p, lddz=128, H=p, ldh=128, n_out=128, n_in=128, partials=p, nsplit=1),
            nulls("dZ", "H", "partials") + row + [(-1, dict(n_in=0)), (-1, dict(n_out=0)), (-1, dict(nsplit=0)), (-1, dict(lddz=127)), (-1, dict(ldh=127))])
    rejects("cl_wide_dense_wgrad_head", "Htop ldt head dO dsd leak H ldh n n_out n_in partials hpart nsplit stop st",
            dict(com, Htop=p, ldt=128, head=p, dO=p, dsd=p, H=p, ldh=128, n_out=128, n_in=128, partials=p, hpart=p, nsplit=1),
            nulls("Htop", "head", "dO", "dsd", "H", "partials", "hpart") + row +
            [(-1, dict(n_in=0)), (-1, dict(n_out=0)), (-1, dict(nsplit=0)), (-1, dict(ldt=127)), (-1, dict(ldh=127)),
             (-2, dict(n_out=129, ldt=132)), (-2, dict(n_out=64)), (-2, dict(n_out=64, n_in=64)), (-2, dict(n_in=96)),
             (-1, dict(n_out=64, n_in=64, nsplit=0)), (-1, dict(dO=off)), (-1, dict(dsd=off)), (-2, dict(n_in=96, dO=off))])

    # per-image layers: the grouped streaming kernel holds widths up to 128 and says so (-2) whatever else is wrong with the call
    imf = dict(com, X=p, ldx=128, W=p, b=p, seg=p, n_groups=3, w=128, Y=p, ldy=128)
    rejects("cl_wide_image_forward", "X ldx W b seg n_groups n w leak Y ldy stop st", imf,
            nulls("X", "W", "b", "seg", "Y") + [(-1, dict(n=0)), (-1, dict(n_groups=0)), (-1, dict(w=0)), (-1, dict(ldx=127)), (-1, dict(ldy=127)),
                                               (-2, dict(w=129, ldx=132, ldy=132)), (-2, dict(w=129)), (-2, dict(w=129, X=None)), (-2, dict(w=129, n=0))])
    imd = dict(com, dZ=p, lddz=128, W=p, seg=p, n_groups=3, w=128, Hprev=p, ldh=128, dX=p, ldo=128)
    rejects("cl_wide_image_dgrad", "dZ lddz W seg n_groups n w Hprev ldh leak dX ldo stop st", imd,
            nulls("dZ", "W", "seg", "dX") + [(-1, dict(n=0)), (-1, dict(n_groups=0)), (-1, dict(w=0)), (-1, dict(lddz=127)), (-1, dict(ldo=127)),
                                            (-2, dict(w=129, lddz=132, ldo=132)), (-2, dict(w=129)), (-2, dict(w=129, dZ=None)), (-2, dict(w=129, n=0))])
    tf = dict(leak=0.01, stop=None, st=None, X=p, ldx=256, W=p, b=p, seg=p, tiles=p, n_tiles=4, w=256, Y=p, ldy=256)
    rejects("cl_wide_image_forward_tiles", "X ldx W b seg tiles n_tiles w leak Y ldy stop st", tf,
            nulls("X", "W", "b", "seg", "tiles", "Y") + [(-1, dict(n_tiles=0)), (-1, dict(w=0)), (-1, dict(ldx=255)), (-1, dict(ldy=255))])
    td = dict(leak=0.01, stop=None, st=None, dZ=p, lddz=256, W=p, seg=p, tiles=p, n_tiles=4, w=256, Hprev=p, ldh=256, dX=p, ldo=256)
    rejects("cl_wide_image_dgrad_tiles", "dZ lddz W seg tiles n_tiles w Hprev ldh leak dX ldo stop st", td,
            nulls("dZ", "W", "seg", "tiles", "dX") + [(-1, dict(n_tiles=0)), (-1, dict(w=0)), (-1, dict(lddz=255)), (-1, dict(ldo=255))])
    rejects("cl_wide_image_wgrad", "dZ lddz H ldh seg n_groups n w dW db stop st",
            dict(n=100, stop=None, st=None, dZ=p, lddz=128, H=p, ldh=128, seg=p, n_groups=3, w=128, dW=p, db=p),
            nulls("dZ", "H", "seg", "dW", "db") + row + [(-1, dict(n_groups=0)), (-1, dict(w=0)), (-1, dict(lddz=127)), (-1, dict(ldh=127))])

    rejects("cl_wide_head_forward", "H ldh Wo n w bij eps loc sig stop st",
            dict(n=100, stop=None, st=None, H=p, ldh=128, Wo=p, w=128, bij=0, eps=1e-7, loc=p, sig=p),
            nulls("H", "Wo", "loc", "sig") + [(-1, dict(n=0)), (-1, dict(w=0)), (-1, dict(ldh=127))])
    rejects("cl_wide_head_backward", "H ldh Wo dO n w bij eps leak dZ lddz partials nblocks stop st",
            dict(com, H=p, ldh=128, Wo=p, dO=p, w=128, bij=0, eps=1e-7, dZ=p, lddz=128, partials=p, nblocks=1),
            nulls("H", "Wo", "dO", "dZ", "partials") + row +
            [(-1, dict(w=0)), (-1, dict(nblocks=0)), (-1, dict(ldh=127)), (-1, dict(lddz=127)), (-1, dict(w=126, ldh=126)), (-1, dict(w=126, lddz=126)),
             (-1, dict(H=off)), (-1, dict(dZ=off)), (-2, dict(w=1025, ldh=1028, lddz=1028)), (-1, dict(w=1025, ldh=1028, lddz=1028, H=off)),
             (-1, dict(w=1025, ldh=1028, lddz=1024))])


def test_round6_entry_points_host_side():
    """`cl_frozen_rows` / `cl_chain_dx` (round 6): workspace queries and argument checks answer without a device."""
    import ctypes as C
    lib = _lib.get_lib()
    # two edge records per 64-row wave, S floats each; at most CL_LAUE_LIK_MAX_BLOCKS workgroups of 256 rows
    assert lib.cl_frozen_edge_floats(0, 3) == 0 and lib.cl_frozen_edge_floats(1, 3) == 6 and lib.cl_frozen_edge_floats(64, 1) == 2
    assert lib.cl_frozen_edge_floats(65, 8) == 32 and lib.cl_frozen_edge_floats(10_000_000, 8) == 2 * 156250 * 8
    assert lib.cl_frozen_grid(1) == 1 and lib.cl_frozen_grid(257) == 2 and lib.cl_frozen_grid(10_000_000) == _lib.CL_LAUE_LIK_MAX_BLOCKS
    assert int(lib.cl_abi_sizeof(b"cl_frozen_args")) == C.sizeof(_lib.FrozenArgs)
    assert lib.cl_frozen_rows(None, None) == -1
    fa = _lib.FrozenArgs()
    fa.n, fa.S = 100, 2
    assert lib.cl_frozen_rows(C.byref(fa), None) == -1                    # no buffers
    fa.gmeta = 1                                                          # (harmonic groups, first call: still no buffers)
    assert lib.cl_frozen_rows(C.byref(fa), None) == -1
    assert lib.cl_chain_dx(None, None, 10, 128, 10, 10, None, None, None) == -1
    assert lib.cl_chain_dx(1, 1, 10, 128, 16, 10, 1, None, None) == -2    # widths beyond 15
    assert lib.cl_chain_dx(1, 1, 200, 128, 10, 10, 1, None, None) == -1   # n_pad < n_obs


# --- `cl_frozen_rows`: three forms behind one entry point (csrc/elbo_frozen.hip: frozen_check) -------------------------------------------------
_FP = 0x10000          # a made-up device address: every call below returns before anything is launched or dereferenced
_F_ROWS = dict(refl_id=_FP, loc=_FP, sigma=_FP, iobs=_FP, sig=_FP, z_f=_FP, dz_f=_FP, scalars=_FP, edge_rid=_FP, edge_val=_FP)      # monochromatic rows
_F_GROUPS = dict(refl_id=_FP, loc=_FP, sigma=_FP, iobs=_FP, sig=_FP, z_f=_FP, scalars=_FP, gmeta=_FP, gbuf=_FP)                     # harmonic groups, first call
_F_SUMS = dict(refl_id=_FP, gbuf=_FP, dz_f=_FP, edge_rid=_FP, edge_val=_FP)                                                         # ... second call: per-reflection sums
_BIG_N, _BIG_R = (1 << 31) - 64, 1 << 30


def test_cl_frozen_rows_rejections():
    """Per form: a call the library would ACCEPT (never made: it would launch), and one rejecting call per clause its checks distinguish --
    a missing pointer, n / S not positive, the likelihood (the two forms that evaluate one), Evans-2011 raw parameters without a place
    for their gradient, the 32-bit bounds (-4), and which of -1 and -4 answers when both apply."""
    import ctypes as C
    lib = _lib.get_lib()

    def call(base, **over):
        a = _lib.FrozenArgs()
        for k, v in dict(dict(base, n=100, S=2, R=50, lik_kind=_lib.CL_LIK_NORMAL), **over).items():
            setattr(a, k, v)
        return lib.cl_frozen_rows(C.byref(a), None)

    for name, base in (("rows", _F_ROWS), ("groups", _F_GROUPS), ("sums", _F_SUMS)):
        lik, edges = base is not _F_SUMS, base is not _F_GROUPS
        cases = [(-1, {k: None}) for k in base]                          # (a NULL gmeta / gbuf names another form, which misses its own buffers)
        cases += [(-1, dict(n=0)), (-1, dict(n=-3)), (-1, dict(S=0)), (-1, dict(ev11=_FP)), (-1, dict(ev11=_FP, nll_part=_FP)),
                  (-4, dict(n=_BIG_N)), (-4, dict(n=_BIG_N, ev11=_FP)), (-1, dict(n=_BIG_N, refl_id=None)), (-1, dict(n=_BIG_N, S=0))]
        if edges:
            cases += [(-4, dict(R=_BIG_R)), (-1, dict(R=_BIG_R, dz_f=None)), (-4, dict(R=_BIG_R, ev11=_FP))]
        else:           # no edges, no bound on R: the clause behind it answers
            cases += [(-1, dict(R=_BIG_R, ev11=_FP))]
        if lik:
            cases += [(-1, dict(lik_kind=3)), (-1, dict(lik_kind=-1)), (-1, dict(lik_kind=3, n=_BIG_N))]
            for k in ("ev11", "d_ev11", "ev11_part"):                    # Laplace beside an Evans-2011 buffer; the check comes before the bounds
                cases += [(-1, {"lik_kind": _lib.CL_LIK_LAPLACE, k: _FP}), (-1, {"lik_kind": _lib.CL_LIK_LAPLACE, k: _FP, "n": _BIG_N})]
        else:           # no likelihood check: neither an unknown kind nor Laplace beside Evans-2011 buffers is answered -1 by it
            cases += [(-4, dict(lik_kind=3, n=_BIG_N)), (-4, dict(lik_kind=_lib.CL_LIK_LAPLACE, ev11=_FP, d_ev11=_FP, n=_BIG_N))]
        for want, over in cases:
            assert set(over) <= set(f for f, _ in _lib.FrozenArgs._fields_), over
            got = call(base, **over)
            assert got == want, (name, over, got, want)


# --- the scaler's flat layouts and the row-chunk walk, each written once (nn.dense_layout, image.image_layer_layout, wide.image_chunks) ------
def test_dense_layout_is_what_the_library_the_scaler_the_flat_layout_and_the_chain_plan_count():
    from careless_amd.engine import chain_plan
    from careless_amd.models.scaling.nn import dense_layout
    lib = _lib.get_lib()
    for d in (1, 5, 37, 70):
        for w in (3, 10, 16, 64, 96):
            for L in (1, 2, 13, 24):
                layers, head = dense_layout(d, w, L)
                P = head + 2 * w + 2
                assert P == int(lib.cl_mlp_param_count(d, w, L)) == MLPScaler(L, w).param_count(d)
                assert [f for _, _, f in layers] == [d] + [w] * (L - 1) and layers[0][0] == 0
                for (ow, ob, f), nxt in zip(layers, [l[0] for l in layers[1:]] + [head]):       # kernel, bias, next kernel: no gap
                    assert ob == ow + w * f and nxt == ob + w
                slices = MLPScaler(L, w).layer_slices(d)
                assert slices == [(ow, w, f, ob) for ow, ob, f in layers] + [(head, 2, w, head + 2 * w)]
                lay = make_layout(R=11, d=d, w=w, L=L, n_img=0)
                bounds = [x for _, o, _, ob in slices for x in (ob, ob + o)]              # the end of every kernel and of every bias
                assert lay.P == P and lay.seg_off == [0, 11, 22] + [22 + x for x in bounds]
                for m in (3, 10):
                    for last in (0, 20):
                        blocks, at = chain_plan(d, w, L, m, last=last), 0
                        for b in blocks:                                                   # the blocks tile [0, P)
                            assert b.off == at and b.P > 0 and b.d_in == (d if b.l0 == 0 else w)
                            assert b.off == (layers[b.l0][0]) and b.final == (b is blocks[-1])
                            at += b.P
                        assert at == P and blocks[0].l0 == 0 and blocks[-1].l1 == L
                        assert all(a.l1 == b.l0 for a, b in zip(blocks[:-1], blocks[1:]))


def test_image_layer_layout_tiles_the_per_image_block():
    from careless_amd.models.scaling.image import NeuralImageScaler, image_layer_layout
    for K in (1, 3):
        for M in (1, 7):
            for w in (5, 72):
                layers, total = image_layer_layout(K, M, w)
                at = 0
                for ow, ob in layers:                       # kernels [M][w][w], then biases [M][w], layer after layer
                    assert ow == at and ob == ow + M * w * w
                    at = ob + M * w
                assert at == total == K * M * (w * w + w) and len(layers) == K
                s = NeuralImageScaler(K, M, 2, w)
                s.build(4)
                assert s.flat.numel() == total and [tuple(t.shape) for t in s.image_weights] == [(M, w, w), (M, w)] * K
                assert all(torch.equal(t, torch.eye(w).expand(M, w, w)) for t in s.image_weights[0::2])
                lay = make_layout(R=3, d=4, w=w, L=2, n_img=0, imgl=(K, M))
                assert lay.n_imgl == total and lay.seg_off[-2 * K - 1:] == [lay.off_imgl] + [lay.off_imgl + x for ow, ob in layers for x in (ob, ob + M * w)]


def test_image_chunks_keep_whole_images_and_cover_every_row_once():
    from careless_amd.wide import image_chunks
    rng = np.random.default_rng(5)
    counts = [np.array([20, 0, 280, 0])] + [rng.integers(0, 200, size=rng.integers(1, 12)) * (rng.random(1) < 2) for _ in range(10)]
    for k, c in enumerate(counts):
        if k:
            c = np.where(rng.random(len(c)) < 0.3, 0, c)                    # empty images, also in front and at the end
            c[rng.integers(len(c))] = 150                                  # (at least one row; an image longer than 128)
        seg = np.concatenate([[0], np.cumsum(c)]).astype(np.int64)
        for chunk in (128, 384):
            out = image_chunks(seg, chunk)
            assert [a for a, _, _, _ in out] == [0] + [b for _, b, _, _ in out[:-1]] and out[-1][1] == seg[-1]      # every row in exactly one chunk
            for a, b, m0, rel in out:
                m1 = m0 + len(rel) - 1
                assert b > a and rel.dtype == np.int32                                                   # no chunk is empty
                assert seg[m0] == a and seg[m1] == b and np.array_equal(rel, seg[m0:m1 + 1] - a)       # whole images: no image is split
                assert b - a <= max(chunk, int(np.max(np.diff(rel))))                                  # at most the chunk, or its single long image
                assert b - a <= chunk or np.count_nonzero(np.diff(rel)) == 1
    assert [(a, b, m0, rel.tolist()) for a, b, m0, rel in image_chunks(np.array([0, 20, 20, 300, 300]), 128)] == \
        [(0, 20, 0, [0, 20, 20]), (20, 300, 2, [0, 280])]


# --- the engine's state: the table of the flat vector, binding, the workspace carve, the two refusals (host logic of ElboEngine.__init__) ------
def test_flat_layout_table_gives_every_offset():
    from careless_amd.engine import FLAT_GROUPS
    from careless_amd.models.scaling.image import image_layer_layout
    from careless_amd.models.scaling.nn import dense_slices
    assert FLAT_GROUPS == ("q_loc", "q_scale", "mlp", "img", "imgl", "ev11", "dwr")
    for L, w, d in ((2, 32, 5), (20, 10, 5)):
        slices = dense_slices(d, w, L)
        P = slices[-1][3] + 2
        for R in (1, 3, 100):
            for n_img in (0, 9):
                for imgl in (None, (2, 7)):
                    for n_ev11 in (0, 3):
                        for n_dwr in (0, 4):
                            lay = make_layout(R=R, d=d, w=w, L=L, n_img=n_img, n_ev11=n_ev11, n_dwr=n_dwr, imgl=imgl)
                            n_imgl = 0 if imgl is None else imgl[0] * imgl[1] * (w * w + w)
                            assert [g[0] for g in lay.groups] == list(FLAT_GROUPS)
                            assert [g[2] for g in lay.groups] == [R, R, P, n_img, n_imgl, n_ev11, n_dwr]
                            at = 0
                            for name, off, cnt in lay.groups:            # contiguous, in the stated order
                                assert off == at == lay.off(name) and cnt >= 0
                                at += cnt
                            assert at == lay.n == 2 * R + P + n_img + n_imgl + n_ev11 + n_dwr
                            # the closed forms the properties restated before the table
                            assert (lay.P, lay.n_img, lay.n_imgl, lay.n_ev11, lay.n_dwr) == (P, n_img, n_imgl, n_ev11, n_dwr)
                            assert lay.off_mlp == 2 * R
                            assert lay.off_img == 2 * R + P
                            assert lay.off_imgl == 2 * R + P + n_img
                            assert lay.off_ev11 == 2 * R + P + n_img + n_imgl
                            assert lay.off_dwr == 2 * R + P + n_img + n_imgl + n_ev11
                            flat = torch.arange(lay.n)
                            for name, off, cnt in lay.groups:
                                assert lay.view(flat, name).tolist() == list(range(off, off + cnt))
                            # seg_off: the tensors of every group, as before
                            seg = [0, R, 2 * R] + [2 * R + x for _, o, _, ob in slices for x in (ob, ob + o)]
                            seg += [lay.off_img + n_img] if n_img else []
                            if imgl is not None:
                                seg += [lay.off_imgl + x for ow, ob in image_layer_layout(imgl[0], imgl[1], w)[0] for x in (ob, ob + imgl[1] * w)]
                            seg += [lay.off_ev11 + k + 1 for k in range(n_ev11)] + ([lay.off_dwr + n_dwr] if n_dwr else [])
                            assert lay.seg_off == seg and seg[-1] == lay.n
                            assert lay.seg_owner == ["q", "q"] + ["scaler"] * (len(seg) - 3 - n_ev11 - (1 if n_dwr else 0)) + ["likelihood"] * n_ev11 + \
                                ["prior"] * (1 if n_dwr else 0)
    from careless_amd.engine import FlatLayout
    lay = FlatLayout(R=4, P=10, n_img=2, seg_off=[], seg_owner=[])          # (the keywords bench.py's tests construct one with)
    assert (lay.n, lay.off_mlp, lay.off_img, lay.off_imgl, lay.off_ev11, lay.off_dwr) == (20, 8, 18, 20, 20, 20)


def test_bind_flat_turns_plugin_tensors_into_views_of_the_flat_vector():
    from types import SimpleNamespace as NS
    from careless_amd.engine import bind_flat, split_flat
    from careless_amd.models.scaling.image import NeuralImageScaler
    from careless_amd.models.scaling.nn import dense_slices
    R, d, w, L, K, M = 5, 4, 6, 2, 2, 3
    rng = torch.Generator().manual_seed(3)
    rand = lambda n: torch.rand(n, generator=rng)
    for with_img, with_imgl, ev11, n_dwr in ((True, False, True, 2), (False, True, False, 0), (False, False, False, 0), (True, True, True, 3)):
        slices = dense_slices(d, w, L)
        lay = make_layout(R=R, d=d, w=w, L=L, n_img=7 if with_img else 0, n_ev11=3 if ev11 else 0, n_dwr=n_dwr, imgl=(K, M) if with_imgl else None)
        q = NS(loc_raw=rand(R), scale_raw=rand(R))
        mlp = NS(flat=rand(lay.P))
        img = NS(_scales=rand(7)) if with_img else None
        imgl = NS(flat=rand(lay.n_imgl)) if with_imgl else None
        lik = NS(raw=rand(3)) if ev11 else NS(raw=None)
        prior = NS(r_raw=rand(n_dwr)) if n_dwr else NS(r_raw=None)
        bindings = [("q_loc", q, "loc_raw"), ("q_scale", q, "scale_raw"), ("mlp", mlp, "flat"), ("img", img, "_scales"), ("imgl", imgl, "flat"),
                    ("ev11", lik, "raw"), ("dwr", prior, "r_raw")]
        assert [b[0] for b in bindings] == [g[0] for g in lay.groups]
        before = {g: getattr(h, a).clone() for g, h, a in bindings if h is not None and getattr(h, a) is not None}
        flat = torch.full((lay.n,), float("nan"))
        bind_flat(flat, lay, q, mlp, img, imgl, lik, prior)
        assert not torch.isnan(flat).any()                                 # every element was written
        for (group, holder, attr), (name, off, cnt) in zip(bindings, lay.groups):
            if cnt == 0:
                assert group not in before or before[group].numel() == 0   # nothing to bind: the holder is left alone
                continue
            t = getattr(holder, attr)
            assert t.data_ptr() == flat.data_ptr() + 4 * off and t.numel() == cnt and t.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
            assert torch.equal(t, before[group])                           # its original values
            flat[off:off + cnt] += 1.0                                     # a write through the flat vector is seen by the plugin
            assert torch.equal(getattr(holder, attr), before[group] + 1.0)
        # the per-tensor views cover [0, n) exactly once, in order
        views = split_flat(flat, lay, slices, NeuralImageScaler(K, M, L, w).layer_views if with_imgl else None)
        marks = torch.zeros(lay.n, dtype=torch.int64)
        for v in views:
            assert v.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
            off = (v.data_ptr() - flat.data_ptr()) // 4
            marks[off:off + v.numel()] += 1
        assert torch.equal(marks, torch.ones(lay.n, dtype=torch.int64))
        # ... tensor by tensor as `seg_off` cuts the vector (the three Evans-2011 scalars come as one view)
        inner = [lay.off_ev11 + k for k in (1, 2)] if ev11 else []
        assert [v.numel() for v in views] == np.diff([x for x in lay.seg_off if x not in inner]).tolist()
        assert [tuple(v.shape) for v in views[2:2 + 2 * len(slices)]] == [s for _, o, i, _ in slices for s in ((i, o), (o,))]


# (R, S, n, nseg, owner) -> (dz_f, grads, msg, msg_norm, scalars, seg_sq, own_scratch, ws_step, total): offsets and counts in floats, taken from the
# arithmetic ElboEngine.__init__ held inline before `carve_workspace`
WORKSPACE_TABLE = {
    (1, 1, 9, 5, False): ((0, 1), (4, 9), (6, 15), (17, 4), (24, 8), (32, 10), (42, 10), (4, 48), 52),
    (1, 1, 9, 5, True): ((0, 1), (6, 9), (8, 15), (19, 4), (24, 8), (32, 10), (42, 10), (4, 48), 52),
    (3, 3, 1100, 9, True): ((0, 9), (14, 1100), (20, 1102), (1118, 4), (1124, 8), (1132, 18), (1150, 10), (12, 1148), 1160),
    (5, 8, 2251, 8, False): ((0, 40), (40, 2251), (50, 2249), (2295, 4), (2300, 8), (2308, 16), (2324, 10), (40, 2294), 2334),
    (41, 3, 500, 12, True): ((0, 123), (126, 500), (208, 426), (630, 4), (636, 8), (644, 24), (668, 10), (124, 554), 678),
    (41, 1, 500, 12, False): ((0, 41), (44, 500), (126, 426), (548, 4), (552, 8), (560, 24), (584, 10), (44, 550), 594),
    (2, 3, 71, 6, True): ((0, 6), (8, 71), (12, 75), (83, 4), (88, 8), (96, 12), (108, 10), (8, 110), 118),
    (100, 8, 4567, 15, False): ((0, 800), (800, 4567), (1000, 4375), (5371, 4), (5376, 8), (5384, 30), (5414, 10), (800, 4624), 5424),
}


def test_workspace_carve():
    from careless_amd.engine import carve_workspace
    names = ("dz_f", "grads", "msg", "msg_norm", "scalars", "seg_sq", "own_scratch", "ws_step")
    for key, want in WORKSPACE_TABLE.items():
        c = carve_workspace(*key)
        assert tuple(getattr(c, k) for k in names) + (c.total,) == want, key
    for R in (1, 2, 3, 5, 41):
        for S in (1, 3, 8):
            for owner in (False, True):
                for P, nseg in ((7, 4), (3472, 44)):
                    n = 2 * R + P
                    c = carve_workspace(R, S, n, nseg, owner)
                    assert c.aligned and c.owner == owner
                    assert (c.msg if owner else c.grads)[0] % 4 == 0 and c.ws_step[0] % 4 == 0        # the all-reduced buffer, ws_step: 16-byte boundaries
                    assert all(getattr(c, k)[0] % 2 == 0 for k in ("scalars", "seg_sq", "own_scratch"))                 # doubles on 8-byte boundaries
                    assert (c.dz_f, c.grads[1], c.scalars[1], c.seg_sq[1], c.own_scratch[1], c.msg_norm[1]) == ((0, R * S), n, 8, 2 * nseg, 10, 4)
                    # the regions follow each other without overlap (four floats of slack in front of the norm terms) and end at the total
                    slack = (c.grads[0] + n, 4)
                    regions = [c.dz_f, c.grads, slack, c.msg_norm, c.scalars, c.seg_sq, c.own_scratch]
                    for (a, na), (b, _) in zip(regions[:-1], regions[1:]):
                        assert a + na <= b
                    assert slack[0] + 4 == c.msg_norm[0]
                    assert c.own_scratch[0] + c.own_scratch[1] == c.total
                    # the two spans: the message is the gradient behind a and b, the slack and the norm terms; a step clears everything from the
                    # gradient's padding on
                    assert c.msg == (c.grads[0] + 2 * R, n + 8 - 2 * R) and c.msg[0] + c.msg[1] == c.msg_norm[0] + 4
                    assert c.dz_f[1] <= c.ws_step[0] <= c.grads[0] and c.ws_step[0] + c.ws_step[1] == c.total


def test_deterministic_refusal_clause_by_clause():
    from careless_amd.engine import ScalerPlan, chain_plan, check_deterministic
    LANE, IMGL, NONE = _lib.CL_ROUTE_LANE, _lib.CL_ROUTE_LANE_IMGL, _lib.CL_ROUTE_NONE
    plain = ScalerPlan(False, False, None, False, LANE)
    wide = ScalerPlan(True, False, None, False, NONE)
    chain = ScalerPlan(False, False, chain_plan(5, 10, 24, 20), False, LANE)
    ok = dict(plan=plain, laue=False, two_pass=False, imgl=False, S=1, dw_trainable=False)
    accepted = [{}, dict(laue=True), dict(S=3), dict(plan=wide, S=4), dict(plan=wide, S=64), dict(plan=chain), dict(plan=ScalerPlan(False, True, None, False, LANE)),
                dict(plan=ScalerPlan(False, False, None, False, IMGL), imgl=True), dict(plan=ScalerPlan(False, False, None, False, NONE))]
    for over in accepted:
        assert check_deterministic(**dict(ok, **over)) is None, over
    refused = [dict(two_pass=True), dict(laue=True, two_pass=True),                  # the two-pass Laue path
               dict(plan=wide, laue=True), dict(plan=wide, S=3), dict(plan=wide, S=128),      # wide: monochromatic, a sample count that divides 64
               dict(plan=ScalerPlan(False, False, None, False, NONE), imgl=True), dict(plan=wide, S=4, imgl=True),      # per-image layers without a route
               dict(plan=chain, laue=True),                                          # a chain on Laue data
               dict(dw_trainable=True)]                                              # a trainable double-Wilson r
    for over in refused:
        with pytest.raises(NotImplementedError, match="deterministic mode covers monochromatic and single-pass Laue data.*keep their float atomics"):
            check_deterministic(**dict(ok, **over))


def test_owner_shard_decision_clause_by_clause():
    from careless_amd.engine import wants_owner_shard
    from careless_amd.models.priors.empirical import NormalReferencePrior
    wilson = WilsonPrior(np.zeros(6, dtype=bool), np.ones(6), 1.0)
    ref = NormalReferencePrior(np.ones(6), np.ones(6), np.ones(6, dtype=bool))
    ok = dict(want=True, prior=wilson, world=2, owner_given=False, laue=False, double_wilson=False, wide=False, imgl=False, deterministic=False)
    assert wants_owner_shard(**ok) is True and wants_owner_shard(**dict(ok, world=8)) is True
    for over in (dict(want=False), dict(world=1), dict(owner_given=True), dict(laue=True), dict(double_wilson=True), dict(wide=True), dict(imgl=True),
                 dict(deterministic=True)):
        assert wants_owner_shard(**dict(ok, **over)) is False, over
    # the split is Wilson-only: asked for on several ranks, or given, it refuses another prior -- also where it would keep the row split
    for over in ({}, dict(laue=True), dict(owner_given=True), dict(want=False, owner_given=True), dict(world=1, owner_given=True)):
        with pytest.raises(NotImplementedError, match="reflection-owner split runs the Wilson prior only, not NormalReferencePrior"):
            wants_owner_shard(**dict(ok, prior=ref, **over))
    for over in (dict(want=False), dict(world=1)):                        # not asked for, nobody to split with: the prior is not looked at
        assert wants_owner_shard(**dict(ok, prior=ref, **over)) is False


def test_switch_model_attribute_then_environment_then_default(monkeypatch):
    from types import SimpleNamespace as NS
    from careless_amd.engine import switch
    env = "CARELESS_HIP_TEST_SWITCH"
    monkeypatch.delenv(env, raising=False)
    assert switch(NS(), "x", env) is False and switch(NS(), "x", env, default=True) is True and switch(NS(x=None), "x", env) is False
    assert switch(NS(x=True), "x", env) is True and switch(NS(x=False), "x", env, default=True) is False and switch(NS(), None, env) is False
    monkeypatch.setenv(env, "1")
    assert switch(NS(), "x", env) is True and switch(NS(x=None), "x", env) is True and switch(NS(), None, env) is True
    assert switch(NS(x=False), "x", env) is False                          # the attribute wins ...
    assert switch(NS(x=False), "x", env, env_adds=True) is True             # ... unless the variable may add (`deterministic`)
    monkeypatch.setenv(env, "0")
    assert switch(NS(), "x", env, default=True) is False and switch(NS(x=True), "x", env, default=True) is True
    assert switch(NS(x=True), "x", env, env_adds=True) is True and switch(NS(), "x", env) is False
    monkeypatch.setenv(env, "yes")                                          # only "1" switches on, only "0" off
    assert switch(NS(), "x", env) is False and switch(NS(), "x", env, default=True) is True


# --- the engine's modules: one route decision, host modules that need no engine ------------------------------
ENGINE_MODULES = ("flat", "plan", "fused", "slots", "det", "nlik")
# every name another file of the repository imports from, or reads on, careless_amd.engine
ENGINE_EXPORTS = ("ElboEngine", "ObsChunks", "ObsData", "make_shard", "owner_bounds", "owner_shard", "laue_group_shard", "launch_row_limit",
                  "debug_noise", "tn_sample", "tn_moments", "predict_moments", "scaler_forward", "_forward_layers", "require_gpu", "_stream",
                  "FORWARD_CHUNK_BYTES", "plan_scaler", "chain_plan", "ScalerPlan", "check_deterministic", "wants_owner_shard", "switch",
                  "check_neural_likelihood", "posterior_kind", "prior_kind", "reference_prior_arrays", "REFPRIOR_KINDS", "make_layout",
                  "FLAT_GROUPS", "FlatLayout", "bind_flat", "split_flat", "carve_workspace", "GRANULE", "TILE", "pack_by_image", "pack_laue")


def test_data_term_route_precedence():
    """frozen before wide, before chain, before two-pass (Laue rows not packed for the single-pass kernels), before peel, before fused --
    over every combination of the six arguments."""
    from itertools import product
    from careless_amd.frozen import FrozenForm
    from careless_amd.plan import Route, data_term_route
    assert [r.name for r in Route] == ["FROZEN", "WIDE", "CHAIN", "TWO_PASS", "PEEL", "FUSED"]
    n = 0
    for form, wide, chained, laue, fused_laue, peel in product((None, *FrozenForm), *[(False, True)] * 5):
        table = ((form is not None, Route.FROZEN), (wide, Route.WIDE), (chained, Route.CHAIN), (laue and not fused_laue, Route.TWO_PASS),
                 (peel, Route.PEEL), (True, Route.FUSED))
        want = next(route for holds, route in table if holds)
        assert data_term_route(form, wide, chained, laue, fused_laue, peel) is want, (form, wide, chained, laue, fused_laue, peel)
        n += 1
    assert n == 4 * 32
    # the precedence that is easy to get wrong: the plan says `peel`, `pack_laue` declined to pack the rows -- no peeled launch
    assert data_term_route(None, False, False, True, False, True) is Route.TWO_PASS
    assert data_term_route(None, False, False, True, True, True) is Route.PEEL
    assert data_term_route(None, False, True, True, False, True) is Route.CHAIN
    assert data_term_route(FrozenForm.SLOTS, True, True, True, False, True) is Route.FROZEN


def test_engine_modules_do_not_import_the_engine():
    """`careless_amd.flat` and `careless_amd.plan` -- and the four mixin modules -- import without `careless_amd.engine`: imported afresh
    with the engine taken out of `sys.modules`, none brings it back; and none names it in an import statement, a function's own included."""
    import ast
    import importlib
    import sys
    import careless_amd
    names = ["careless_amd." + m for m in ENGINE_MODULES]
    for m in ENGINE_MODULES:
        tree = ast.parse(open(os.path.join(ROOT, "careless_amd", m + ".py")).read())
        for node in ast.walk(tree):
            if isinstance(node, ast.Import):
                assert not any(a.name.startswith("careless_amd.engine") for a in node.names), (m, node.lineno)
            elif isinstance(node, ast.ImportFrom):
                assert not (node.module or "").startswith("careless_amd.engine"), (m, node.lineno)
                assert not (node.module == "careless_amd" and any(a.name == "engine" for a in node.names)), (m, node.lineno)
    saved = {n: sys.modules.pop(n) for n in names + ["careless_amd.engine"] if n in sys.modules}
    attrs = {n: getattr(careless_amd, n) for n in ENGINE_MODULES + ("engine",) if hasattr(careless_amd, n)}
    try:
        for n in names:
            importlib.import_module(n)
            assert "careless_amd.engine" not in sys.modules, n
    finally:
        for n in names:
            sys.modules.pop(n, None)
        sys.modules.update(saved)
        for n, mod in attrs.items():
            setattr(careless_amd, n, mod)


def test_engine_keeps_its_names():
    """`careless_amd.engine` exposes every name other files import from it, as the object its new home defines; `ElboEngine` keeps the class
    flags tests flip and the methods tests and scripts call."""
    from careless_amd import det, engine, flat, frozen, fused, nlik, plan, slots, wide
    missing = [n for n in ENGINE_EXPORTS if not hasattr(engine, n)]
    assert not missing, missing
    for mod in (flat, plan):
        for n in ENGINE_EXPORTS:
            assert not hasattr(mod, n) or getattr(mod, n) is getattr(engine, n), (mod.__name__, n)
    E = engine.ElboEngine
    assert [c for c in (fused.FusedPath, wide.WidePath, frozen.FrozenPath, slots.SlotPath, det.DetPath, nlik.NlikPath) if not issubclass(E, c)] == []
    for flag in ("SLOT_ROWS_ONE_LAUNCH", "FROZEN_LAUE_PACKED", "FROZEN_SORTED_ROWS", "FUSE_PRE", "FUSE_WG0", "FUSE_HEADB", "FUSE_LIK"):
        assert getattr(E, flag) is True, flag
    assert E.local_only is False
    for method in ("_mlp_args", "_block_args", "_nlik_args", "_data_term", "_data_term_launch", "_noise_to_device", "_likelihood_args",
                   "training_launch", "kernel_name", "_slot_args", "_slot_likelihood", "_laue_pad_slots", "_laue_passes", "_sig", "_det_parts",
                   "_det_attach", "_det_reduce", "_peel_bufs", "_peel_args", "_peel_reduce", "_fused_step_launch", "_data_term_chain",
                   "_nlik_attach", "_nlik_forward", "_nlik_backward", "_step_fields", "_shard_rows", "_param_ptr", "_grad_ptr", "_tn_args",
                   "_q_launch", "_ref_prior", "forward_backward", "optimizer_step", "evaluate_nll", "make_obs"):
        assert callable(getattr(E, method, None)), method
