"""What holds tests/ref_lane.py -- the restated launch layer of csrc/elbo_lane.hip / csrc/elbo_narrow.hip and the case list of
tests/test_lane_kernels_gpu.py -- without a GPU:

  * the names the case list produces (cl_mlp_kernel_name on the built library) are exactly the enumerated covered set; none is a per-image-layer
    name; covered and uncovered sets together are what the library names over a sweep of (w, d, L, flags) through these routes: an instance added
    later without a case fails here;
  * every case passes cl_mlp_check, runs the route and the instance the restated rules give, and sets no routing switch;
  * the reference against oracle/elbo_oracle.py at 1e-10 M on the new shapes (20 layers at width <= 12, up to 31 columns);
  * no case holds a pre-activation inside its own propagated rounding bound, every layer of every case takes both LeakyReLU branches;
  * an fp32 emulation of every launch (dZ0_out included) stays inside a QUARTER of every bound on the inputs of every GPU case;
  * every wrong variant misses at least one bound (the smallest ratio over its bounds missed is printed);
  * every option of the list changes at least one output of the reference.
"""
import copy
import ctypes
import itertools
import os

import numpy as np
import pytest

from careless_amd import _lib
from tests import ref_lane as RL
from tests import ref_mlp as RM
from tests import ref_rows as RR
from tests import test_ref_mlp as TR


@pytest.fixture(scope="module")
def hm():
    lib = RR.host_lib()
    if lib is None:
        pytest.skip("no host compiler")
    return lib


def all_cases():
    return RL.cases() + RL.stop_cases()


ROUTE = {"lane": _lib.CL_ROUTE_LANE, "narrow": _lib.CL_ROUTE_NARROW, "lane_block": _lib.CL_ROUTE_LANE_BLOCK}


# ---- the case list against the enumerated sets and the library ---------------------------------------------------------------------------------
def test_case_list_covers_the_enumerated_instances_exactly():
    want, skip = RL.enumerate_lane_instances(), RL.enumerate_uncovered()
    assert not set(want) & skip
    assert len(want) == 18 * (3 * 4 + 3 * 2) + (9 * 4 + 4 * 2 + 4 * 3) + 6          # per depth 2 .. 19; the default depth: registers, blocks, LDS rows; narrow
    got, det = set(), set()
    for c in all_cases():
        route, name, chk = RL.query(c)
        assert chk == 0 and route == ROUTE[RL.route(c)], (c.id, route, chk)
        assert name == RL.expected_instance(c) == getattr(c, "instance", name), (c.id, name, RL.expected_instance(c))
        assert "image layers" not in name and name.replace(RL.DET_TAG, "") not in skip, (c.id, name)
        (det if name.endswith(RL.DET_TAG) else got).add(name.replace(RL.DET_TAG, ""))
    assert got == set(want), (sorted(set(want) - got), sorted(got - set(want)))
    full = {k for k, v in want.items() if v[4][0] and not v[6]}         # the deterministic stores: every full instance
    assert det == full, sorted(full - det)
    # the borders of the shape list
    cs = [c for c in all_cases() if RL.route(c) != "narrow"]
    assert {c.w for c in cs} >= set(range(3, 13)) | {1} and {c.d for c in cs} >= {1, 8, 9, 15, 16, 17, 30, 31} and {c.L for c in cs} >= set(range(2, 21))
    nar = [c for c in all_cases() if RL.route(c) == "narrow"]
    assert {max(c.w, c.d) for c in nar} >= {8, 9, 12, 13, 15} and {c.L for c in nar} >= {1, 19, 20} and any(c.w < c.d for c in nar) and any(c.w > c.d for c in nar)
    assert {c.S for c in all_cases()} >= {1, 2, 3, 4, 5, 8, 9, 12, 16, 17} and {c.n for c in all_cases()} >= {3, 32, 33, 64, 65, 128, 256, 257, RL.N_INST}
    assert RL.route(RL.lcase(4, 9, 7)) == "narrow" and RL.route(RL.lcase(5, 9, 7)) == "lane" and RL.route(RL.lcase(12, 9, 20)) == "narrow" and RL.route(RL.lcase(12, 8, 20)) == "lane"
    assert RL.route(RL.lcase(10, 32, 20)) is None and RL.route(RL.lcase(13, 16, 20)) is None and RL.route(RL.lcase(11, 16, 20)) is None


def test_covered_and_uncovered_sets_are_what_the_library_names_over_a_sweep():
    lib, buf, names = _lib.get_lib(), ctypes.create_string_buffer(256), set()
    routes = (_lib.CL_ROUTE_LANE, _lib.CL_ROUTE_LANE_IMGL, _lib.CL_ROUTE_LANE_BLOCK, _lib.CL_ROUTE_NARROW)
    flags = [dict(), dict(eta=1), dict(dZ0_out=1), dict(eta=1, dZ0_out=1), dict(row_map=1), dict(row_map=1, dZ0_out=1), dict(row_map=1, gmeta=1, tile_gmax=1)]
    imgl = [dict(row_map=1, n_imgl=k, imgl=1, d_imgl=1, tile_img=1, n_images=3, **f) for k in (1, 2, 3) for f in (dict(), dict(eta=1), dict(dZ0_out=1))]
    for w, d, L in itertools.product(range(1, 17), range(1, 34), range(1, 22)):
        base = dict(n_obs=256, n_pad=256, d=d, w=w, L=L, S=2, R=64, leak=RM.LEAK, lik_kind=RR.KINDS["normal"], dof=RM.DOF, bij_kind=0)
        for f in flags + imgl:
            a = _lib.MlpArgs(**base, **f)
            if int(lib.cl_mlp_route(ctypes.byref(a), 0)) in routes:
                lib.cl_mlp_kernel_name(ctypes.byref(a), 0, buf, 256)
                names.add(buf.value.decode())
        for mode, f in ((1, dict(act_out=1)), (2, dict(dH_ext=1, partials=1))):
            a = _lib.MlpArgs(**base, **f)
            if int(lib.cl_mlp_route(ctypes.byref(a), mode)) in routes:
                lib.cl_mlp_kernel_name(ctypes.byref(a), mode, buf, 256)
                names.add(buf.value.decode())
    want = set(RL.enumerate_lane_instances()) | RL.enumerate_uncovered()
    assert names == want, (sorted(want - names)[:8], sorted(names - want)[:8])


def test_no_case_sets_a_switch():
    assert not [k for k in os.environ if k.startswith("CARELESS_HIP_")]


# ---- the reference against the oracle on the new shapes ------------------------------------------------------------------------------------------
ORACLE_CASES = [RL.lcase(10, 15, 20, n=150, S=3, img="sorted"), RL.lcase(12, 8, 20, n=140, S=9, lik="studentt", bij="softplus", img="unsorted"),
                RL.lcase(9, 31, 20, n=130, S=2, ev11=True), RL.lcase(4, 16, 20, n=129, S=4), RL.lcase(13, 9, 20, n=131, S=2, lik="studentt", ev11=True)]


@pytest.mark.parametrize("c", ORACLE_CASES, ids=lambda c: c.id)
def test_reference_equals_the_oracle(c):
    TR.test_reference_equals_the_oracle(c)


def test_dz0_of_the_reference_is_the_gradient_of_the_peeled_composition():
    """dZ_0 X^T and its row sums are layer 0's gradient (what cl_peel_backward makes of dZ0_out), W_1^T dZ_1 is dL/d(activations of a first block)
    (what cl_chain_dx makes of it): the reference's own pieces, at 1e-10 M"""
    c = RL.lcase(10, 17, 20, n=150, S=3, dz0=True)
    x, ref = RM.reference_for(c)
    dz, mz = ref.b.dZ[0], ref.b.MZ[0]
    P0 = x.w * x.d
    assert np.all(np.abs((dz.T @ RM.RW.f64(x.X)).ravel() - ref.grad[:P0]) <= 1e-10 * ref.M_grad[:P0])
    assert np.all(np.abs(dz.sum(0) - ref.grad[P0:P0 + x.w]) <= 1e-10 * ref.M_grad[P0:P0 + x.w])
    assert np.all(np.abs(dz) <= mz * (1 + 1e-12)) and np.all(dz != 0.0)
    W1 = RM.RW.f64(x.fw.layers[1][0])
    assert np.allclose((ref.b.dZ[1] @ W1) * x.fw.slope[0], dz, rtol=1e-12, atol=0)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------------
def test_no_case_holds_a_near_zero_unit_and_every_case_is_alive():
    for c in all_cases():
        x, ref = RM.reference_for(c)
        assert ref.near == 0, (c.id, ref.near)
        if c.n >= 64:
            assert x.fw.minpos >= 0.1, (c.id, x.fw.minpos)
        if c.mode != 1:
            assert np.all(ref.grad != 0.0), c.id
        if c.dz0:
            assert np.all(ref.b.dZ[0][x.act] != 0.0), c.id


# ---- the emulation: inside a quarter of every bound; the wrong kernels: outside one ---------------------------------------------------------------
def test_fp32_emulation_stays_inside_a_quarter_of_every_bound(hm):
    worst = {}
    for c in all_cases():
        x, ref = RM.reference_for(c)
        pre = RM.preloads(x, ref) if c.mode != 1 else None
        r = RM.ratios(x, ref, pre, RM.emulate(x, hm, pre))
        assert not c.dz0 or "dZ0_out" in r
        for k, v in r.items():
            if v > worst.get(k, (0.0, ""))[0]:
                worst[k] = (v, c.id)
        assert all(v <= 0.25 for v in r.values()), (c.id, r)
    print("fp32 emulation, largest error / bound:", {k: f"{v:.2e} ({i})" for k, (v, i) in sorted(worst.items())})


def _dz0_observation_major(x, got):
    flat = np.zeros(got.dz0.size, RM.F32)
    v = got.dz0[:x.w, :x.np_].T.ravel()
    flat[:v.size] = v
    got.dz0 = flat.reshape(got.dz0.shape)


def _ev11_stride_4(x, got):
    p = got.ev11_part.reshape(-1, RM.EV11_WAVES, 3)
    q = np.zeros_like(p).reshape(-1, 3)
    for g in range(p.shape[0]):
        q[4 * g:4 * g + 4] += p[g, :4]                                  # (a later workgroup's store lands on an earlier one's slots 4 .. 7)
    got.ev11_part = q.ravel()


def _bias_from_column_w(x, got):
    """the bias gradient is the ones column (block 15) of a layer's weight-gradient accumulator.  Column w instead is: layer 0, metadata column w
    (d > w) -- another tensor's numbers; a hidden layer, input feature w -- a padding feature, whose activation is LeakyReLU(0) = 0: zeros ARE
    what that defect stores"""
    sl = dict(RM.tensor_slices(x))
    for l in range(x.L):
        k = x.d if l == 0 else x.w
        dW = got.partials[:, sl[f"dW{l}"]].reshape(-1, x.w, k)
        got.partials[:, sl[f"db{l}"]] = dW[:, :, x.w] if k > x.w else 0.0
    got.grad = None


def _second_block_one_column_off(x, got):
    d, w = x.d, x.w
    for g in range(got.partials.shape[0]):
        W = got.partials[g, :w * d].reshape(w, d)
        W[:, 15:] = np.roll(W[:, 15:], 1, axis=1)
    got.grad = None


def _col15_from_the_ones_row(x):
    x.X = x.X.copy()
    x.X[:, 15] = 1.0


def _narrow_ks_from_w(x):
    """the metadata layer takes max(w, d) / 4 k-steps; from w alone the steps behind it are not loaded (a step that is not `have` is zeroed:
    prefetch of elbo_narrow.hip) -- at w = 4, d = 9 ONE column, the ninth"""
    x.X = x.X.copy()
    x.X[:, 4 * (2 if x.w <= 8 else 3):] = 0.0


def _narrow_feature_as_its_own_slot(x, got):
    """the narrow kernel keeps feature f in slot ((f & 3) << 2) | (f >> 2) (a 4 x 4 transpose of 0 .. 15); a flush that takes the slot number for
    the feature stores every weight-gradient entry of the transposed pair (zeros where that pair is no feature)"""
    p = [((f & 3) << 2) | (f >> 2) for f in range(16)]
    sl = dict(RM.tensor_slices(x))
    for l in range(x.L):
        k = x.d if l == 0 else x.w
        dW = got.partials[:, sl[f"dW{l}"]].reshape(-1, x.w, k).copy()
        db = got.partials[:, sl[f"db{l}"]].copy()
        wrong, wb = np.zeros_like(dW), np.zeros_like(db)
        for fo in range(x.w):
            if p[fo] < x.w:
                wb[:, fo] = db[:, p[fo]]
                for fi in range(k):
                    if fi < 16 and p[fi] < k:
                        wrong[:, fo, fi] = dW[:, p[fo], p[fi]]
        got.partials[:, sl[f"dW{l}"]], got.partials[:, sl[f"db{l}"]] = wrong.reshape(len(dW), -1), wb
    got.grad = None


# mutant -> (case, emulate's mutant or None, a change of the inputs the emulation sees or None, a change of its result or None)
MUTANTS = {
    "rows_behind_n_obs_counted": (RL.lcase(10, 9, 20, S=3), "rows_behind_n_obs_counted", None, None),
    "second_wave_tile_skipped": (RL.lcase(8, 15, 20, S=3), "second_wave_tile_skipped", None, None),
    "metadata_column_15_read_from_the_ones_row": (RL.lcase(10, 17, 20, S=3), None, _col15_from_the_ones_row, None),
    "second_input_block_weight_gradient_one_column_off": (RL.lcase(10, 31, 20, S=3), None, None, _second_block_one_column_off),
    "bias_gradient_from_column_w": (RL.lcase(9, 15, 19, S=3), None, None, _bias_from_column_w),
    "head_wgrad_from_one_wave": (RL.lcase(10, 8, 20, S=3), "head_wgrad_from_one_wave", None, None),
    "ninth_sample_dropped": (RL.lcase(10, 15, 20, S=9), "ninth_sample_dropped", None, None),
    "tile_shares_a_reflection_by_store": (RL.lcase(10, 15, 20, S=3), "tile_shares_a_reflection_by_store", None, None),
    "dz0_without_first_slope": (RL.lcase(10, 15, 20, S=3, dz0=True), "dz0_without_first_slope", None, None),
    "dz0_observation_major": (RL.lcase(6, 8, 20, S=3, dz0=True), None, None, _dz0_observation_major),
    "narrow_ks_from_w_alone": (RL.lcase(4, 9, 3, S=3), None, _narrow_ks_from_w, None),
    "narrow_feature_taken_as_its_own_slot": (RL.lcase(13, 9, 20, S=3), None, None, _narrow_feature_as_its_own_slot),
    "dH_ext_read_behind_n_obs": (RL.lcase(10, 9, 20, mode=2, n=5 * 64 + 37), "dH_ext_read_behind_n_obs", None, None),
    "ev11_part_slot_stride_4": (RL.lcase(10, 15, 20, S=3, det=True, ev11=True), None, None, _ev11_stride_4),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_every_wrong_variant_misses_a_bound(mutant, hm):
    import copy
    c, em, change_in, change_out = MUTANTS[mutant]
    x, ref = RM.reference_for(c)
    pre = RM.preloads(x, ref)
    good = RM.ratios(x, ref, pre, RM.emulate(x, hm, pre))
    assert all(v <= 0.25 for v in good.values()), (mutant, good)
    assert RL.route(c) in ("lane", "narrow", "lane_block") and RL.query(c)[2] == 0, c.id
    xm = copy.copy(x)
    if change_in:
        change_in(xm)
    got = RM.emulate(xm, hm, pre, mutant=em)
    if change_out:
        change_out(x, got)
    bad = RM.ratios(x, ref, pre, got)
    over = {k: v for k, v in bad.items() if not v <= 1.0}
    print(f"{mutant}: outside its bound by", {k: f"{v:.3g}" for k, v in over.items()}, "smallest", min(over.values(), default=None))
    assert over, (mutant, bad)


# ---- liveness of the options ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt", [dict(S=9), dict(lik="studentt"), dict(bij="softplus"), dict(img="sorted"), dict(img="unsorted"), dict(ev11=True)])
def test_every_option_changes_an_output_of_the_reference(opt):
    base = RL.lcase(10, 15, 20, n=200, S=3)
    x0, r0 = RM.reference_for(base)
    x1, r1 = RM.reference_for(RL.lcase(10, 15, 20, n=200, **{**dict(S=3), **opt}))
    assert r0.rows.nll != r1.rows.nll and (r0.grad.shape != r1.grad.shape or np.any(r0.grad != r1.grad))


def test_every_option_that_adds_or_moves_an_output_is_alive(hm):
    """the options that leave the NLL and the gradient as they are: each one adds an output that the comparison then holds, or moves one --
    seen on the emulation's result through ref_mlp.ratios, the comparison of the GPU tests"""
    def outs(**kw):
        c = RL.lcase(10, 8, 20, n=200, S=3, **kw)
        x, ref = RM.reference_for(c)
        pre = RM.preloads(x, ref)
        return c, x, ref, pre, RM.emulate(x, hm, pre)
    c0, x0, ref0, pre0, g0 = outs()
    for kw, key in ((dict(ipred=True), "ipred_out"), (dict(dz0=True), "dZ0_out"), (dict(det=True), "dzf_obs")):
        c, x, ref, pre, g = outs(**kw)
        r = RM.ratios(x, ref, pre, g)
        assert key in r and key not in RM.ratios(x0, ref0, pre0, g0) and RM.set_fields(c) > RM.set_fields(c0), kw
    # ipred_out and dZ0_out are not constants: rows differ, no element is zero
    c, x, ref, pre, g = outs(ipred=True, dz0=True)
    assert np.all(ref.rows.ipred[x.act] != 0.0) and np.ptp(ref.rows.ipred) > 0 and np.all(ref.b.dZ[0] != 0.0)
    # det_slot moves every record: the same records in the caller's order miss the bound
    c, x, ref, pre, g = outs(det=True, det_slot=True)
    assert not np.array_equal(x.det_slot, np.arange(x.n))
    xs = copy.copy(x)
    xs.det_slot = None
    assert RM.ratios(xs, ref, pre, g)["dzf_obs"] > 1.0 and RM.ratios(x, ref, pre, g)["dzf_obs"] <= 0.25
    # noise_row moves the key of every position's normals (the GPU test draws them at cl_debug_noise's rows noise_row - obs_offset): a permutation
    c, x, ref, pre, g = outs(packed=True, noise="philox", noise_row=True)
    assert not np.array_equal(x.noise_row[x.act] - x.obs_offset, x.krow[x.act]) and "noise_row" in RM.set_fields(c)
    # harmonic groups: members of a group share one observation and one density of the SUM of their predictions
    c, x, ref, pre, g = outs(packed=True, groups=True)
    c1, x1, ref1, pre1, g1 = outs(packed=True)
    assert x.slot is not None and np.any(np.bincount(np.asarray(x.slot)[x.act]) > 1) and int(x.count.sum()) < int(x.act.sum()) == int(x1.count.sum())
    xg = copy.copy(x)
    xg.slot, xg.count = None, x.act.copy()
    assert abs(RM.reference(xg).rows.nll - ref.rows.nll) > RM.RTOL_LOSS * max(ref.rows.M_nll, 1.0)


# ---- the peeled first layer and the chain step ---------------------------------------------------------------------------------------------------
def test_peel_emulations_stay_inside_their_bounds():
    """each call in its own accumulation order: the fmaf chain of cl_peel_forward / cl_chain_dx, the tile sums of cl_peel_backward on one and on
    three workgroups.  A quarter of every derived and every RTOL bound, cl_chain_dx at every w_out included (its operands make the chain exact:
    ref_lane.chain_problem).  The ONE bar that is a single rounding, the tail's sum of two stored numbers, no fp32 evaluation meets at a quarter:
    the emulation has to hold it, and its ratio is printed."""
    worst = {}
    for s in RL.peel_shapes():
        p = RL.peel_problem(*s)
        assert RL.peel_supported(p.d, p.w, p.L)
        r = RL.peel_forward_ratios(p, *RL.peel_forward_emulate(p))
        for nparts in (1, 3):
            r.update({f"{k}, {nparts} part(s)": v for k, v in RL.peel_backward_ratios(p, RL.peel_backward_emulate(p, nparts=nparts)).items()})
        assert all(v <= (1.0 if k.startswith("tail") else 0.25) for k, v in r.items()), (p.id, r)
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in r.items()}
    for s in RL.CHAIN_SHAPES:
        q = RL.chain_problem(*s)
        r = RL.chain_ratios(q, RL.chain_emulate(q))
        assert all(v <= 0.25 for v in r.values()), (q.id, r)
        worst["cl_chain_dx"] = max(worst.get("cl_chain_dx", 0.0), r["dx_t"])
    print("peel emulations, largest error / bound:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert {p[1] for p in RL.peel_shapes()} >= {15, 16, 17, 37, 63, 64, 79} and {p[2] for p in RL.peel_shapes()} == set(RL.PEEL_NS) and {p[0] for p in RL.peel_shapes()} == set(RL.PEEL_WS)


@pytest.mark.parametrize("mutant", RL.PEEL_MUTANTS + ("W_not_transposed",))
def test_every_wrong_peel_variant_misses_a_bound(mutant):
    if mutant == "W_not_transposed":
        q = RL.chain_problem(10, 7, 257)
        bad = RL.chain_ratios(q, RL.chain_emulate(q, mutant))
    else:
        p = RL.peel_problem(10, 37, 257, 3)
        bad = RL.peel_backward_ratios(p, RL.peel_backward_emulate(p, mutant))
    over = {k: v for k, v in bad.items() if not v <= 1.0}
    print(f"{mutant}: outside its bound by", {k: f"{v:.3g}" for k, v in over.items()})
    assert over, (mutant, bad)


def test_peeled_composition_of_the_reference_is_the_unpeeled_scaler():
    """LeakyReLU(I u + 0) on u = W_0 x + b_0 is the first activation: the peeled scaler's forward pass on u_t equals the whole scaler's, in fp64"""
    c = RM.case("plain", 0, 10, 37, 20, n=150, S=3)
    x, ref = RM.reference_for(c)
    p = RL.peel_problem(10, 37, 150, 20)
    u = RM.RW.f64(x.X) @ RM.RW.f64(x.mlp[:370]).reshape(10, 37).T + RM.RW.f64(x.mlp[370:380])
    mlp_peel = np.concatenate([np.eye(10).ravel(), np.zeros(10), RM.RW.f64(x.mlp[380:])])
    f = RM.forward(u, mlp_peel, 10, 10, 20, True, x.bij_kind, float(x.eps))
    assert np.allclose(f.loc[0], x.fw.loc[0], rtol=1e-12, atol=0) and np.allclose(f.sig[0], x.fw.sig[0], rtol=1e-12, atol=0)
    assert p.mlp_peel.size == RM.param_count(10, 10, 20) and np.array_equal(p.mlp_peel[:100].reshape(10, 10), np.eye(10, dtype=np.float32))
