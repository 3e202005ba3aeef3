"""What holds tests/ref_mlp.py -- the fp64 reference, the bounds and the case list of tests/test_mlp_kernels_gpu.py -- without a GPU:

  * the reference against oracle/elbo_oracle.py: the scaler's outputs against O.mlp_forward / O.scale_bijector, the NLL and the gradients of the
    scaler, the image scales and the Evans-2011 triple against O.elbo_value_and_grads (the KL does not reach them), dz_f through the oracle's own graph;
  * an fp32 emulation of the launch (numpy float32 in any summation order -- the fp32 MFMA is an fmaf chain, DESIGN 4.1 -- with the scalar
    math of the host build of csrc/cl_math.h) stays inside a QUARTER of every bound on the inputs of every GPU case;
  * every wrong kernel of ref_mlp.MUTANTS misses at least one bound on a case of the list (the factor is printed);
  * no case holds a pre-activation inside its own propagated rounding bound, every layer of every case takes both LeakyReLU branches on a tenth
    of its units at least, no reference gradient entry is exactly zero unless it is structurally zero;
  * the names the case list produces (cl_mlp_kernel_name + cl_mlp_epilogue, no device needed) are exactly the instances enumerated from the
    rules of mlp_geom / mlp_route restated in ref_mlp.enumerate_instances: an instance added later without a case fails here.
"""
import numpy as np
import pytest
import torch

from oracle import elbo_oracle as O
from tests import ref_mlp as RM
from tests import ref_rows as RR
from tests import ref_wide as RW

T = RR.T


@pytest.fixture(scope="module")
def hm():
    lib = RR.host_lib()
    if lib is None:
        pytest.skip("no host compiler")
    return lib


def all_cases():
    return RM.cases() + RM.stop_cases()


# ---- the reference against the oracle -------------------------------------------------------------------------------------------------------
ORACLE_CASES = [RM.case("plain", 0, 17, 9, 3, n=200, S=3, lik="normal", img="sorted"), RM.case("plain", 0, 8, 6, 20, n=150, S=5, lik="studentt", bij="softplus", img="unsorted"),
                RM.case("plain", 0, 64, 33, 5, n=130, S=2, lik="normal", ev11=True, img="sorted"), RM.case("plain", 0, 16, 1, 2, n=140, S=4, lik="laplace"),
                RM.case("plain", 0, 1, 8, 1, n=129, S=1, lik="studentt", ev11=True)]


@pytest.mark.parametrize("c", ORACLE_CASES, ids=lambda c: c.id)
def test_reference_equals_the_oracle(c):
    x = RM.make_inputs(c, RM.case_seed(c))
    layers, head = RM.unpack(x.mlp, x.d, x.w, x.L)
    ws = [T(Wt.T) for Wt, _ in layers] + [T(head[:2 * x.w].reshape(2, x.w).T)]
    bs = [T(b) for _, b in layers] + [T(head[2 * x.w:])]
    out = O.mlp_forward(T(x.X), ws, bs, RM.LEAK)
    sig = O.scale_bijector(out[:, 1], c.bij, float(x.eps))
    assert np.allclose(x.fw.loc[0], out[:, 0].numpy(), rtol=1e-12, atol=1e-13) and np.allclose(x.fw.sig[0], sig.numpy(), rtol=1e-12, atol=1e-13)
    lap = c.lik == "laplace"
    cfg = O.ElboConfig(mc_samples=x.S, likelihood=c.lik, dof=float(x.dof), scale_bijector=c.bij, epsilon=float(x.eps), scale_shift=float(x.shift),
                       use_image_scales=x.img is not None, ev11=c.ev11, leakiness=RM.LEAK)
    rng = np.random.default_rng(5)
    p = O.ElboParams(T(rng.normal(0.0, 0.3, x.R)), T(np.log(rng.uniform(0.05, 0.3, x.R))), ws, bs, img_raw=T(x.img) if x.img is not None else None,
                     ev11_raw=T(x.ev11) if c.ev11 else None)
    image_id = x.image_id if x.img is not None else np.zeros(x.n, np.int32)
    inp = O.ElboInputs(torch.as_tensor(x.refl_id.astype(np.int64)), torch.as_tensor(image_id.astype(np.int64)), T(x.X), T(x.iobs), T(x.sig),
                       torch.zeros(x.R, dtype=torch.bool), T(np.ones(x.R)), T(np.full(x.R, 1e-32)), sigma=T(1.0))
    u_f, eta = T(rng.uniform(0.05, 0.95, (x.S, x.R))), T(x.eta.T)
    res, grads = O.elbo_value_and_grads(p, inp, cfg, u_f, eta)
    x.z_f = res["z_f"].numpy().T.copy()                               # the oracle's own amplitudes, in fp64
    x.w_ll = 1.0 / x.S                                                # (the oracle's weight: the device gets its fp32 rounding)
    ref = RM.reference(x)
    rr = ref.rows
    assert abs(rr.nll - float(res["nll"])) <= 1e-10 * rr.M_nll
    flat = np.concatenate([np.concatenate([grads[2 + 2 * l].numpy().T.ravel(), grads[3 + 2 * l].numpy()]) for l in range(x.L + 1)])
    assert flat.shape == ref.grad.shape and np.all(np.abs(ref.grad - flat) <= 1e-10 * ref.M_grad)
    assert np.all(ref.M_grad * (1 + 1e-12) >= np.abs(ref.grad))
    k = 2 + 2 * (x.L + 1)
    if x.img is not None:
        assert np.all(np.abs(rr.d_img - grads[k].numpy()) <= 1e-10 * np.maximum(rr.M_img, 1e-300))
        k += 1
    if c.ev11:
        assert np.all(np.abs(rr.d_ev11 - grads[k].numpy()) <= 1e-10 * rr.M_ev11)
    # the workgroups' partial sums and NLL parts add up to the whole
    assert np.allclose(sum(v for v, _ in ref.part), ref.grad, rtol=1e-9, atol=1e-12 * np.max(ref.M_grad))
    assert abs(sum(q.nll for q in ref.parts) - rr.nll) <= 1e-10 * rr.M_nll
    if not lap:                                                       # dz_f and dX through the oracle's own graph
        q = p.clone(requires_grad=True)
        meta = inp.metadata.clone().requires_grad_(True)
        fw = O.elbo_forward(q, O.ElboInputs(**{**inp.__dict__, "metadata": meta}), cfg, u_f, eta)
        dz, dm = torch.autograd.grad(fw["nll"], [fw["z_f"], meta])
        assert np.all(np.abs(rr.dz - dz.numpy().T) <= 1e-10 * rr.M_dz)
        assert np.all(np.abs(ref.b.dX - dm.numpy()) <= 1e-10 * ref.b.MX)
    # the records of the deterministic mode add up to dz_f and d_img
    tot = np.zeros_like(rr.dz)
    np.add.at(tot, x.refl_id, rr.gbuf)
    assert np.all(np.abs(tot - rr.dz) <= 1e-10 * rr.M_dz)
    if x.img is not None:
        tot = np.zeros(x.n_images)
        np.add.at(tot, x.image_id, ref.dimg_row)
        assert np.all(np.abs(tot[1:] - rr.d_img) <= 1e-10 * np.maximum(rr.M_img, 1e-300))


def test_external_gradient_and_chain_references_compose_to_the_whole_scaler():
    """mode 2 from dO_ext = the full step's dO reproduces its scaler gradient; a two-block chain (head-less block, then the last block on its
    activations) composed by hand reproduces the whole scaler's loc / sigma, gradient and dX"""
    c = RM.case("plain", 0, 13, 18, 4, n=150, S=3, img="sorted")
    x, ref = RM.reference_for(c)
    x2 = RM.make_inputs(RM.case("plain", 2, 13, 18, 4, n=150), x.seed)
    assert np.array_equal(x2.mlp, x.mlp)
    x2.dO = ref.rows.dO                                               # (fp64: the same numbers)
    r2 = RM.reference(x2)
    assert np.allclose(r2.grad, ref.grad, rtol=1e-12, atol=1e-14 * np.max(ref.M_grad))
    # blocks: layers 0 .. 1 head-less, layers 2 .. 3 with the head
    layers, head = RM.unpack(x.mlp, x.d, x.w, x.L)
    flat = lambda ls, h=None: np.concatenate([np.concatenate([W.ravel(), b]) for W, b in ls] + ([h] if h is not None else []))
    f1 = RM.forward(x.X, flat(layers[:2]), x.d, x.w, 2, False, x.bij_kind, float(x.eps))
    f2 = RM.forward(f1.H[-1], flat(layers[2:], head), x.w, x.w, 2, True, x.bij_kind, float(x.eps))
    assert np.allclose(f2.loc[0], x.fw.loc[0], rtol=1e-13) and np.allclose(f2.sig[0], x.fw.sig[0], rtol=1e-13)
    assert np.all(f2.E[-1] <= x.fw.E[-1] * (1 + 1e-9))                # (the second block alone starts from exact inputs)


# ---- the case list -------------------------------------------------------------------------------------------------------------------------
def test_case_list_covers_the_enumerated_instances_exactly():
    want = RM.enumerate_instances()
    got = {}
    for c in all_cases():
        route, name, epi, inst = RM.query(c)
        assert "elbo_mlp_kernel" in name and "image layers" not in name, (c.id, name)
        assert RM.UNIT_TAG[c.unit] + ", KS=" in name, (c.id, name)
        got.setdefault(inst, c.id)
        assert inst == RM.expected_instance(c) == getattr(c, "instance", inst), (c.id, inst, RM.expected_instance(c))      # every case: the restated rules name its instance
    assert set(got) == set(want), (sorted(set(want) - set(got)), sorted(set(got) - set(want)))
    # every rim value of the issue's shape list is somewhere in the list
    ws, ds, Ls, Ss = ({getattr(c, k) for c in all_cases()} for k in ("w", "d", "L", "S"))
    assert {1, 8, 9, 12, 13, 15, 16, 17, 31, 32, 33, 64} <= ws and {1, 6, 8, 9, 32, 33, 50, 64} <= ds and {1, 2, 5, 10, 20} <= Ls and {1, 3, 4, 5, 8, 9, 12} <= Ss
    assert {c.n for c in all_cases()} >= {3, 128, 293, 677} and {c.grid for c in all_cases()} >= {1, 2, 7}


def test_every_case_passes_the_entry_check_and_no_case_sets_a_switch():
    import ctypes
    import os
    from careless_amd import _lib
    assert not [k for k in ("LANE", "NARROW", "LANE_W12", "LANE_DEPTHS", "LANE_BLOCKS", "EPI") if "CARELESS_HIP_" + k in os.environ]      # the routing switches
    lib = _lib.get_lib()
    for c in all_cases():
        a = _lib.MlpArgs(**RM.scalar_fields(c), **{k: 1 for k in RM.set_fields(c)})
        assert int(lib.cl_mlp_check(ctypes.byref(a), c.mode, c.grid)) == 0, c.id


def test_no_case_holds_a_near_zero_unit_and_every_case_is_alive():
    for c in all_cases():
        x, ref = RM.reference_for(c)
        assert ref.near == 0, (c.id, ref.near)
        f, act = x.fw, x.act
        if c.n < 64:                                                  # three rows are the first three of 64 drawn (ref_mlp.scaler_problem): liveness on all 64
            X64, mlp = RM.scaler_problem(x.seed, c.n, c.d, c.w, c.L, c.head, full=True)
            assert np.array_equal(mlp, x.mlp) and np.array_equal(X64[:c.n], x.X[x.act])
            f, act = RM.forward(X64, mlp, c.d, c.w, c.L, c.head, x.bij_kind, float(x.eps)), np.ones(64, bool)
            assert f.near == 0, (c.id, f.near)
        assert f.minpos >= 0.1, (c.id, f.minpos)                      # both branches on a tenth of every layer's units at least
        rms = [float(np.sqrt(np.mean(h[act] ** 2))) for h in f.H[1:]]
        assert 0.2 < min(rms) and max(rms) < 5.0, (c.id, rms)         # neither dying nor growing
        if c.mode == 0:                                               # no sample of the scale cancels: loc + sigma eta + shift keeps a third of its summands' size
            f = x.fw
            tq = f.loc[0][:, None] + f.sig[0][:, None] * RW.f64(x.eta_row) + float(x.shift)
            size = np.abs(f.loc[0])[:, None] + np.abs(f.sig[0][:, None] * RW.f64(x.eta_row)) + abs(float(x.shift))
            assert np.all(np.abs(tq[x.act]) >= size[x.act] / 3), c.id
        if c.mode == 1:
            continue
        assert np.all(ref.grad != 0.0) and np.all(ref.b.dX[x.act] != 0.0), c.id                       # (a padding position's are structurally zero)
        if c.mode == 0:
            rr = ref.rows
            has = np.bincount(x.refl_id[x.act], minlength=x.R) > 0
            assert np.all(rr.dz[has] != 0.0) and np.all(rr.dz[~has] == 0.0), c.id
            assert np.all(rr.gbuf[x.act] != 0.0), c.id
            if x.img is not None:                                     # an image without rows (and image 0, which is pinned) has no gradient
                present = np.zeros(len(x.img), bool)
                ids = np.unique(x.image_id[x.act])
                present[ids[ids > 0] - 1] = True
                assert np.all(rr.d_img[present] != 0.0) and np.all(rr.d_img[~present] == 0.0), c.id
            if c.ev11:
                assert np.all(rr.d_ev11 != 0.0), c.id


# ---- the emulation: inside a quarter of every bound; the wrong kernels: outside one ---------------------------------------------------------------
def test_fp32_emulation_stays_inside_a_quarter_of_every_bound(hm):
    worst = {}
    for c in all_cases():
        x, ref = RM.reference_for(c)
        pre = RM.preloads(x, ref) if c.mode != 1 else None
        r = RM.ratios(x, ref, pre, RM.emulate(x, hm, pre))
        for k, v in r.items():
            if v > worst.get(k, (0.0, ""))[0]:
                worst[k] = (v, c.id)
        assert all(v <= 0.25 for v in r.values()), (c.id, r)
    print("fp32 emulation, largest error / bound:", {k: f"{v:.2e} ({i})" for k, (v, i) in sorted(worst.items())})


MUTANT_CASES = {
    "rows_behind_n_obs_counted": RM.case("plain", 0, 17, 9, 2, S=3),
    "last_tile_left_out_of_wgrad": RM.case("plain", 2, 33, 6, 2),
    "wg1_partial_to_row_0": RM.case("plain", 2, 16, 8, 2),
    "bias_gradient_of_feature_15_dropped": RM.case("plain", 2, 15, 33, 2),
    "slope_at_zero_is_one": None,                                     # (its own test below: the case list holds no exact zero)
    "head_rows_swapped_in_backward": RM.case("plain", 2, 64, 8, 2),
    "image_0_not_pinned": RM.case("plain", 0, 64, 18, 2, S=3, img="sorted"),
    "shift_outside_image_scale": RM.case("plain", 0, 32, 9, 2, S=3, img="sorted", bij="softplus"),
    "second_sample_dropped": RM.case("plain", 0, 64, 8, 2, S=5),
    "eta_read_as_S_n": RM.case("plain", 0, 64, 8, 2, S=3),
    "obs_offset_left_out_of_noise_key": RM.case("plain", 0, 64, 8, 2, S=3, noise="philox"),
    "w_ll_lost": RM.case("plain", 0, 16, 6, 2, S=4, lik="laplace"),
    "dX_without_first_layer_mask": RM.case("chain", 2, 31, 18, 2, head=False, dX=True),
    "act_out_row_major": RM.case("chain", 1, 13, 33, 2, head=False),
    "group_sum_over_tile_gmax": RM.case("packed", 0, 64, 8, 2, S=3, groups=True),
    "det_slot_not_times_S": RM.case("det", 0, 31, 18, 2, S=4, det_slot=True),
}


@pytest.mark.parametrize("mutant", RM.MUTANTS)
def test_every_wrong_kernel_misses_a_bound(mutant, hm):
    c = MUTANT_CASES[mutant]
    if c is None:
        c = RM.case("plain", 2, 16, 8, 1, n=40)
        x = RM.make_inputs(c, 0)
        # a unit at EXACTLY zero: the row's metadata and the unit's bias zeroed (the derivative there is the leak)
        x.X[3] = 0.0
        x.meta_t[:, 3] = 0.0
        x.mlp[x.w * x.d + 5] = 0.0
        x.fw = RM.forward(x.X, x.mlp, x.d, x.w, x.L, True, x.bij_kind, float(x.eps))
        assert x.fw.Z[0][3, 5] == 0.0
        ref = RM.reference(x)
    else:
        x, ref = RM.reference_for(c)
    pre = RM.preloads(x, ref) if c.mode != 1 else None
    shifted = np.roll(x.eta, 1, axis=0) if c.mode == 0 else None      # (another key: another row's normals)
    good = RM.ratios(x, ref, pre, RM.emulate(x, hm, pre))
    assert all(v <= 0.25 for v in good.values()), (mutant, good)
    bad = RM.ratios(x, ref, pre, RM.emulate(x, hm, pre, mutant=mutant, eta_shifted=shifted))
    over = {k: v for k, v in bad.items() if not v <= 1.0}
    print(f"{mutant}: outside its bound by", {k: f"{v:.3g}" for k, v in over.items()})
    assert over, (mutant, bad)
