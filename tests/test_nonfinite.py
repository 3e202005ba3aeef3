"""The reference's contract for a step that meets a NaN or an Inf (careless/models/merging/variational.py:205-209, 271-274), held on every
kernel route a training step can take: the global gradient norm is taken BEFORE anything is sanitised (so it is non-finite), the
non-finite gradient entries are then zeroed one by one and that step's Adam update is still applied, the step is recorded and the loop
breaks.  In this package that rests on every fused kernel carrying a NaN from ONE poisoned observation to the gradient entries that
observation touches -- and to no others --, to the norm (csrc/elbo_step.hip) and to the `stop_flag` every later launch reads; the fused
scaler units are compiled with -fno-honor-nans (careless_amd/build.py), under which the compiler may fold a select or compare that sees
a NaN, so nothing but a test holds it.

One float cell of the inputs is poisoned (never an id column: no address depends on a poisoned value) and the engine is compared with
the fp64 oracle, which implements the contract (oracle/elbo_oracle.py: train_step):

  A  one forward + backward on injected noise: the non-finite MASK of every gradient tensor equals the oracle's -- a finite entry where
     the oracle has NaN is a NaN folded away (a silently wrong last update), a non-finite entry where the oracle is finite is a NaN that
     leaked across a reflection, image or harmonic-group border (those parameters would miss their last update) --, and with the
     non-finite entries zeroed on both sides (the gradient the reference applies) every tensor is within RTOL_GRAD;
  B  `train_model(inputs, 4)` against ONE oracle step: one history record, a non-finite "Grad Norm", every parameter finite and equal
     to the oracle's after the sanitised Adam step -- steps 2 .. 4 were skipped on the device by every launch of the route.

The shapes are the finite twins of cases that already run (tests/test_gpu_parity.py, test_routing.py, test_frozen_scaler.py), with
their keyword dictionaries: no launch geometry is new.  Every case asserts its route first; the closing test holds the matrix to every
`CL_ROUTE_*` of include/careless_hip.h.  The CPU part shows on the oracle alone that the comparison is not vacuous."""
import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np
import pytest
import torch

from careless_amd import _lib
from oracle import elbo_oracle as O
from tests import test_frozen_scaler as F
from tests import test_gpu_parity as P
from tests import test_routing as T
from tests import util

gpu = pytest.mark.gpu


@dataclass(frozen=True)
class Case:
    kw: dict
    route: str                      # plan.route: the name of the CL_ROUTE_* value behind the prefix
    frag: str = ""                  # a fragment of kernel_name()
    peel: bool = False
    blocks: Optional[int] = None    # launches of a chained scaler
    block_routes: tuple = ()        # ... and the routes of the blocks in front of the last one
    wide: bool = False              # layer by layer
    det: bool = False               # model.deterministic
    frozen: bool = False            # scaling_model.trainable = False, fast path on
    single_pass: Optional[bool] = None      # Laue data: harmonic group sums inside the fused kernel
    primary: bool = False           # the extended poisons and the ragged-last-tile row
    seed: int = 7                   # make_problem's seed: the first one whose draw meets the two conditions of `_oracle_grads`


def _routing(L, w, d):
    """The keyword dictionary test_routing.py runs a row of its table with."""
    assert any(r[:3] == (L, w, d) for r in T.TABLE), (L, w, d)
    return dict(N=300, R=30, d0=d, L=L, w=w, S=1, perturb=0.02)


def _param(fn, arg, ident):
    """The keyword dictionary behind one id of a parametrised test of the suite."""
    for m in fn.pytestmark:
        if m.name == "parametrize" and m.args[0] == arg:
            return dict(m.args[1][list(m.kwargs["ids"]).index(ident)])
    raise KeyError(ident)


_det = lambda ident: _param(P.test_deterministic_mode_matches_oracle_and_repeats_bit_for_bit, "kw", ident)
_shard = lambda ident: _param(P.test_rank_shards_sum_to_full_batch_on_gpu, "kw", ident)

MATRIX = {
    # the lane kernel (csrc/elbo_lane.hip)
    "lane_20x10_d5_S1": Case(P.CASES["cli_default_20x10_S1"], "LANE", "elbo_lane_kernel<10, 8, false, ", primary=True),
    "lane_20x10_d21_lds_rows_S8": Case(P.CASES["lane_20x10_d21_S8_studentt"], "LANE", "elbo_lane_kernel<10, 0, false, "),
    "lane_20x10_sample_batches_S12": Case(P.CASES["lane_20x10_S12"], "LANE", "elbo_lane_kernel<10, 8, false, "),
    "lane_per_depth_unit_10x10": Case(_routing(10, 10, 5), "LANE", "elbo_lane_kernel<10, 15, false, false, false, 0, 10>", seed=8),
    "lane_twelve_wide_20x12": Case(_routing(20, 12, 5), "LANE", "elbo_lane_kernel<12, 8, false, "),
    "lane_laue_single_pass_20x10": Case(P.CASES["lane_laue_single_pass_20x10_S2"], "LANE", "elbo_lane_kernel<10, 8, true, ", single_pass=True),
    "lane_image_layers1_20x10": Case(P.CASES["lane_image_layers1_20x10_many_images"], "LANE_IMGL", "false, 1> (image layers)", seed=9),
    "lane_image_layers2_20x10": Case(P.CASES["image_layers2_on_the_cli_default_20x10"], "LANE_IMGL", "false, 2> (image layers)", seed=8),
    "lane_image_layers3_20x10_d21_peeled": Case(P.CASES["lane_image_layers3_20x10_posenc_d21_peeled"], "LANE_IMGL", "3> (image layers)", peel=True, seed=10),
    # the peeled first layer (csrc/elbo_peel.hip) in front of the lane and of the narrow kernel
    "peel_lane_20x10_d37": Case(P.CASES["peel_20x10_d37_S1"], "LANE", "elbo_lane_kernel<10, 15, false, false, true", peel=True, seed=8),
    # (7 x 12 on 21 columns has run on the lane kernel's twelve-wide depth-7 instance since round 6; the narrow kernel keeps one layer and Laue data)
    "peel_lane_twelve_wide_7x12_d21": Case(P.CASES["peel_narrow_7x12_d21_S2"], "LANE", "elbo_lane_kernel<12, 15, false, false, true, 0, 7>", peel=True, seed=9),
    "peel_narrow_1x9_d16": Case(P.CASES["peel_narrow_1x9_d16"], "NARROW", "elbo_narrow_kernel<", peel=True),
    "peel_narrow_laue_single_pass_5x10_d22_ev11": Case(P.CASES["peel_narrow_laue_single_pass_5x10_d22_ev11"], "NARROW", "elbo_narrow_kernel<", peel=True,
                                                       single_pass=True, seed=8),
    # the narrow kernel (csrc/elbo_narrow.hip)
    "narrow_20x13": Case(_routing(20, 13, 5), "NARROW", "elbo_narrow_kernel<2, 4, 8", primary=True),
    "narrow_9x4": Case(P.CASES["narrow_9x4_d6_S2"], "NARROW", "elbo_narrow_kernel<2, 2, 8"),
    # csrc/elbo_mlp.hip: the 16-, 32- and 64-wide instances, the packed layout, per-image layers
    "mlp16_10x16": Case(_routing(10, 16, 5), "MLP", "elbo_mlp_kernel<16, 8, 20, 0"),
    "mlp16_7x15_d40": Case(_routing(7, 15, 40), "MLP", "elbo_mlp_kernel<16, 64, 20, 0"),
    "mlp32_2x32": Case(P.CASES["mlp2x32_normal_img_S3"], "MLP", "elbo_mlp_kernel<32, "),
    "mlp64_5x64_posenc_studentt_S8": Case(P.CASES["mlp5x64_studentt_posenc_S8"], "MLP", "elbo_mlp_kernel<64, 32, 5, 0", primary=True, seed=32),
    "mlp_packed_laue_single_pass_2x32": Case(P.CASES["laue_2x32_normal_S3"], "MLP_PACKED", ", packed", single_pass=True),
    "mlp_image_layers1_2x32": Case(P.CASES["image_layers1_2x32_S3"], "MLP_IMGL", ", image layers", primary=True),
    "mlp_image_layers2_3x64_S8": Case(P.CASES["image_layers2_3x64_S8_studentt"], "MLP_IMGL", "elbo_mlp_kernel<64, ", seed=41),
    "mlp_image_layers1_8x13_d50": Case(P.CASES["image_layers1_8x13_d50_S3_studentt"], "MLP_IMGL", "elbo_mlp_kernel<32, 64, 10, 0, image layers", seed=8),
    # chains of layer blocks
    "chain_12x64": Case(P.CASES["deep_12x64_studentt_S4"], "MLP_CHAIN", "elbo_mlp_kernel<64, ", blocks=3, block_routes=("MLP_CHAIN",), seed=152),
    "chain_24x14": Case(_routing(24, 14, 5), "MLP_CHAIN", "elbo_mlp_kernel<16, 32, 20, 0, chain", blocks=2, block_routes=("MLP_CHAIN",)),
    "chain_24x10_lane_block": Case(P.CASES["deep_24x10_d12_studentt_S3"], "LANE", "elbo_lane_kernel<10, 15, false, false, true", blocks=2,
                                   block_routes=("LANE_BLOCK",)),
    "chain_26x12": Case(P.CASES["deep_26x12_d9_S2"], "LANE", "elbo_lane_kernel<12, 15, false, false, true, 0, 19>", blocks=2, block_routes=("LANE_BLOCK",)),
    # layer by layer (csrc/wide_gemm.hip)
    "wide_3x96": Case(P.CASES["wide_3x96_studentt_S3"], "NONE", "wide_sq_kernel", wide=True, seed=8),
    "wide_metadata_d70_2x32": Case(P.CASES["wide_metadata_d70_2x32"], "NONE", "wide_gemm_kernel", wide=True),
    "wide_image_layers1_2x96": Case(P.CASES["wide_image_layers1_2x96_S3"], "NONE", "wide_", wide=True, seed=11),
    "wide_laue_two_pass_image_layers2_d36": Case(P.CASES["laue_two_pass_image_layers2_20x10_d36"], "NONE", "wide_gemm_kernel", wide=True, single_pass=False),
    # two-pass Laue (csrc/elbo_laue.hip)
    "laue_two_pass_2x32": Case(P.CASES["laue_two_pass_2x32_S3"], "MLP", "elbo_mlp_kernel<32, ", single_pass=False),
    "laue_group_of_more_than_16_rows": Case(P.CASES["laue_groups_over_16_rows_fall_back"], "MLP", "elbo_mlp_kernel<32, ", single_pass=False, seed=24),     # (the poisoned row sits in a small group of a data set whose largest group has 27 rows: 90 % of q stays finite)
    # other model features
    "double_wilson_2x32": Case(P.CASES["double_wilson_2x32_S3"], "MLP", "elbo_mlp_kernel<32, "),
    "double_wilson_trainable_r": Case(P.CASES["double_wilson_trainable_r_S4"], "MLP", "elbo_mlp_kernel<32, "),
    "ev11_normal_2x32": Case(P.CASES["ev11_normal_2x32_S3"], "MLP", "elbo_mlp_kernel<32, "),
    "ev11_studentt_5x64_S8": Case(P.CASES["ev11_studentt_5x64_S8"], "MLP", "elbo_mlp_kernel<64, ", seed=9),
    "klweight_4x48": Case(P.CASES["mlp4x48_klweight_S4"], "MLP", "elbo_mlp_kernel<64, ", seed=9),
    # deterministic mode: the plain, packed and chain-last-block compilations of elbo_mlp.hip, the lane kernel's per-image-layer stores
    "det_mlp_5x64": Case(_det("mono_5x64"), "MLP_DET", ", deterministic", det=True, seed=21),
    "det_packed_laue_5x64": Case(_det("laue_5x64_S3"), "MLP_PACKED_DET", ", packed deterministic", det=True, single_pass=True),
    "det_chain_12x64": Case(_det("deep_12x64_S3"), "MLP_CHAIN_DET", ", chain deterministic", det=True, blocks=3, block_routes=("MLP_CHAIN",), seed=207),
    "det_lane_image_layers2_20x10": Case(_det("image_layers2_lane_20x10"), "LANE_IMGL", "2> (image layers) (deterministic stores)", det=True),
    # a frozen scaler (csrc/elbo_frozen.hip): sorted rows, the two-call form for harmonic groups, per-image layers
    "frozen_mono_20x10": Case(F.CASES["cli_default_20x10_S3"], "LANE", "elbo_lane_kernel<10, 8, ", frozen=True),
    "frozen_laue_two_call_form_2x32": Case(F.CASES["laue_2x32_S2"], "MLP_PACKED", ", packed", frozen=True, single_pass=True),
    "frozen_image_layers1_2x32": Case(F.CASES["image_layers1_2x32"], "MLP_IMGL", ", image layers", frozen=True),
}
SHARD_CASES = {"mono_2x32": _shard("mono"), "cli_default_20x10": _shard("cli_default_20x10")}

# poison: (float column, value).  The core set runs on every route, the extended one on the primary shapes.  (No large finite values:
# they overflow fp32 and not fp64, the two masks would legitimately differ.)
CORE = {"metadata_nan": ("metadata", np.nan), "sigiobs_nan": ("sigiobs", np.nan)}
EXTENDED = {"metadata_inf": ("metadata", np.inf), "iobs_nan": ("iobs", np.nan), "sigiobs_zero": ("sigiobs", 0.0)}
POISONS = {**CORE, **EXTENDED}

PARAMS = [(c, p, "inner") for c in MATRIX for p in CORE]
PARAMS += [(c, p, "inner") for c in MATRIX if MATRIX[c].primary for p in EXTENDED]
PARAMS += [(c, p, "last") for c in MATRIX if MATRIX[c].primary for p in POISONS]
IDS = [f"{c}-{p}-{r}" for c, p, r in PARAMS]


# ---- the problem, its poisoned row and what the oracle makes of it ---------------------------------------------------------------------
def _groups(data):
    """Per row: the rows that share its likelihood term (its harmonic group; monochromatic data: the row alone)."""
    hid = data.get("harmonic_id")
    return np.arange(len(data["refl_id"])) if hid is None else np.asarray(hid)


def _pick_row(data, where):
    """The poisoned row, chosen from the data: `last` is row N - 1 (the ragged last tile); `inner` a row of an image with index >= 1 (the
    gradient of a TRAINABLE image scale / of an image's own layers is hit) -- for Laue data one whose harmonic group touches as few
    reflections as any (a group poisons every reflection it holds; most of q must stay finite and comparable) --, the middle one of those."""
    N = len(data["refl_id"])
    if where == "last":
        return N - 1
    cand = np.nonzero(np.asarray(data["image_id"]) >= 1)[0]
    if "harmonic_id" in data:
        g, rid = _groups(data), np.asarray(data["refl_id"])
        n_refl = np.array([len(set(rid[g == g[r]])) for r in cand])
        cand = cand[n_refl == n_refl.min()]
    return int(cand[len(cand) // 2])


def _problem(name, poison, where):
    case = MATRIX[name] if isinstance(name, str) else name
    kw = dict(case.kw, seed=case.seed)
    opts = {k: kw.pop(k, None) for k in ("two_pass", "regroup", "shuffle_rows", "grid")}
    assert not opts["shuffle_rows"]
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    if opts["regroup"]:
        data = P._regroup_laue(data, opts["regroup"])
    data = dict(data)
    row = _pick_row(data, where)
    column, value = POISONS[poison]
    a = np.array(data[column], dtype=np.float32, copy=True)
    if column == "metadata":
        a[row, row % a.shape[1]] = value
    else:
        a[_groups(data)[row]] = value             # (Laue: Iobs / SigIobs live in the slot of the row's harmonic group)
    data[column] = a
    g = _groups(data)
    hit = dict(row=row, refl=sorted(set(np.asarray(data["refl_id"])[g == g[row]].tolist())), image=int(np.asarray(data["image_id"])[row]))
    return case, kw, opts, data, cfg, params, u_f, eta, hit


def _f64(a):
    return torch.as_tensor(a, dtype=torch.float64)


def _oracle_grads(data, cfg, params, u_f, eta):
    near = []
    out, grads = O.elbo_value_and_grads(params, O.inputs_from_numpy(data), cfg, _f64(u_f), _f64(eta), near=near)
    # no LeakyReLU pre-activation within fp32 rounding of zero: the engine's branches are the oracle's (no forced-branch resolution here).
    # (An infinite pre-activation of the poisoned row -- |z| = inf under a bound of inf -- is listed with a NaN ratio: not a branch in doubt.)
    near = [t for t in near if np.isfinite(t[0])]
    assert not near, sorted(near)[:5]
    # ... and no sampled amplitude next to its truncation bound: z = loc + scale e carries an absolute fp32 error of ~ eps32 |loc| ~ 1e-7, the
    # Wilson density has a log z term, so a sample's KL term carries 1e-7 / z -- at z >= 1e-2 a tenth of RTOL_LOSS, at z = 2e-4 (a uniform of
    # 3e-5) five times RTOL_LOSS, in any fp32 implementation and with or without the poison.  A property of the noise draw: the seed's.
    assert float(out["z_f"].min()) >= 1e-2, float(out["z_f"].min())
    return out, [g.numpy() for g in grads]


def _oracle_step(data, cfg, params, u_f, eta):
    p = params.clone()
    rec = O.train_step(p, O.inputs_from_numpy(data), cfg, O.AdamState.zeros_like(p.tensors()), _f64(u_f), _f64(eta))
    return rec, [t.numpy() for t in p.tensors()]


def _tensor_names(params):
    names = ["q_loc_raw", "q_scale_raw"]
    for l in range(len(params.mlp_w)):
        names += [f"W_{l}", f"b_{l}"]
    if params.img_raw is not None:
        names.append("image_scales")
    for k in range(len(params.imgl_w or [])):
        names += [f"image_W_{k}", f"image_b_{k}"]
    if params.ev11_raw is not None:
        names.append("ev11")
    if params.dw_r_raw is not None:
        names.append("dw_r")
    return names


def _zeroed(a):
    return np.where(np.isfinite(a), a, 0.0)


# ---- CPU part: the oracle alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,poison,where", PARAMS, ids=IDS)
def test_oracle_mask_of_a_poisoned_observation_is_sharp(name, poison, where):
    """What the GPU tests compare against is informative: the norm is non-finite and the parameters after the step are finite; the poisoned
    reflection(s) are non-finite in both q tensors and every Dense tensor is non-finite throughout, while at least 90 % of each q tensor
    -- and, where per-image tensors exist, at least one whole image -- stay finite."""
    case, kw, opts, data, cfg, params, u_f, eta, hit = _problem(name, poison, where)
    out, grads = _oracle_grads(data, cfg, params, u_f, eta)
    rec, after = _oracle_step(data, cfg, params, u_f, eta)
    names = _tensor_names(params)
    assert len(names) == len(grads)
    assert not np.isfinite(rec["Grad Norm"]) and not np.isfinite(rec["loss"]) and np.isfinite(rec["F KLDiv"])
    for n, t0, t in zip(names, params.tensors(), after):
        # (logit(0) = -inf of the root ASU's double-Wilson r is what the reference holds before the step as well)
        assert np.array_equal(np.isfinite(t), np.isfinite(t0.numpy())) and (n == "dw_r" or np.isfinite(t).all()), n
    for n, g in zip(names, grads):
        fin = np.isfinite(g)
        if n.startswith("q_"):
            assert not fin[hit["refl"]].any() and fin.mean() >= 0.9, (n, hit, fin.mean())
        elif n.startswith(("W_", "b_")):
            assert not fin.any(), n
        elif n == "image_scales":                  # (image 0's scale is the fixed 1: image.py:23-25)
            assert hit["image"] >= 1 and not fin[hit["image"] - 1] and fin.sum() == fin.size - 1, (n, hit, fin)
        elif n.startswith("image_"):
            per_image = fin.reshape(fin.shape[0], -1)
            assert not per_image[hit["image"]].any() and per_image.all(axis=1).any(), (n, per_image.mean(axis=1))
        elif n == "ev11":
            assert not fin.any()
        elif n == "dw_r":
            assert fin.all()                       # (the prior's own parameter: the KL term does not see the observations)


def _plan(case):
    """The plan `ElboEngine` makes for the case, from the library's routes alone (host functions: no GPU)."""
    from careless_amd.engine import plan_scaler
    _, kw, opts, data, cfg, *_ = _problem(case, "metadata_nan", "inner")
    gmax = int(np.bincount(np.asarray(data["harmonic_id"])).max()) if cfg.laue else 1
    return plan_scaler(_lib.get_lib(), np.asarray(data["metadata"]).shape[1], kw["w"], kw["L"], cfg.image_layers, laue=cfg.laue,
                       two_pass=bool(opts["two_pass"]), gmax=gmax, ev11=cfg.ev11, deterministic=case.det)


def _route(name):
    return getattr(_lib, "CL_ROUTE_" + name)


def _block_routes(plan, real=None):
    """Routes of the launches of a chain's blocks in front of the last one: forward (activations out), backward (external gradient in)."""
    lib, out = _lib.get_lib(), set()
    for k, b in enumerate(plan.blocks[:-1]):
        if real is not None:
            eng, ma, obs = real
            fwd, bwd = eng._block_args(ma, obs, k), eng._block_args(ma, obs, k)
            fwd.act_out, bwd.dH_ext, bwd.dX_out = 1, 1, (1 if k > 0 else None)
            out |= {lib.cl_mlp_route(C.byref(fwd), 1), lib.cl_mlp_route(C.byref(bwd), 2)}
        else:
            proto = dict(d=b.d_in, w=plan.blocks[-1].d_in, L=b.l1 - b.l0, S=1, refl_id=1, meta_t=1, iobs=1, sig=1, mlp=1, z_f=1, dz_f=1, partials=1,
                         scalars=1, stop_flag=1)
            out |= {_lib.mlp_route(lib, 1, act_out=1, **proto), _lib.mlp_route(lib, 2, dH_ext=1, **(dict(proto, dX_out=1) if k > 0 else proto))}
    return out


@pytest.mark.parametrize("name", list(MATRIX))
def test_matrix_case_plans_the_route_it_names(name):
    case, plan = MATRIX[name], _plan(MATRIX[name])
    assert (plan.route, plan.peel, plan.wide, None if plan.blocks is None else len(plan.blocks)) == (_route(case.route), case.peel, case.wide, case.blocks)
    if case.blocks:
        assert _block_routes(plan) == {_route(r) for r in case.block_routes}


def test_matrix_covers_every_route_of_the_library():
    """A route added to include/careless_hip.h later gets a non-finite case too: the routes the matrix plans (block routes of chained plans
    included) are every CL_ROUTE_* value but CL_ROUTE_NONE.  (The GPU tests hold each engine to the plan collected here.)"""
    every = {v for k, v in vars(_lib).items() if k.startswith("CL_ROUTE_")}
    seen = set()
    for case in MATRIX.values():
        plan = _plan(case)
        seen.add(plan.route)
        if plan.blocks:
            seen |= _block_routes(plan)
    assert seen - {_lib.CL_ROUTE_NONE} == every - {_lib.CL_ROUTE_NONE}, sorted(every - seen)
    assert any(MATRIX[c].wide for c in MATRIX)          # (CL_ROUTE_NONE in a plan: layer by layer)


# ---- GPU part --------------------------------------------------------------------------------------------------------------------------------
def _model(case, kw, opts, data, cfg, params):
    model = util.build_model(data, cfg, params, kw["L"], kw["w"])
    model.laue_two_pass = bool(opts["two_pass"])
    model.kernel_grid = opts["grid"]
    if case.det:
        model.deterministic = True
    if case.frozen:
        model.scaling_model.trainable = False
        model.frozen_scaler_fast_path = True
    return model


def _assert_route(eng, case):
    """The engine runs the kernel the case is in the matrix for -- a case that has drifted off it must fail, not pass vacuously."""
    plan = _plan(case)
    assert eng.plan == plan and plan.route == _route(case.route), (eng.plan, plan)
    assert (bool(eng.peel), bool(eng.wide), None if eng.blocks is None else len(eng.blocks)) == (case.peel, case.wide, case.blocks)
    assert bool(eng.deterministic) == case.det
    if case.frozen:                  # (no scaler launch in the step: the sampling / likelihood kernels of csrc/elbo_frozen.hip on the engine's frozen layout)
        assert eng.scaler_frozen and eng._frozen_layout and eng.frozen_fast
        return
    assert case.frag in eng.kernel_name(), eng.kernel_name()
    if not eng.wide:
        ma, mode = eng.training_launch()
        assert eng.lib.cl_mlp_route(C.byref(ma), mode) == plan.route
        if case.blocks:
            obs = eng.obs.children[0] if hasattr(eng.obs, "children") else eng.obs
            assert _block_routes(plan, (eng, eng._mlp_args(0, None, None, obs), obs)) == {_route(r) for r in case.block_routes}
    if case.single_pass is not None:
        assert bool(eng.obs.fused_laue) == case.single_pass


def _assert_masks_and_values(names, g_hip, g_ref, what=""):
    for n, a, b in zip(names, g_hip, g_ref):
        fa, fb = np.isfinite(a), np.isfinite(b)
        folded, leaked = np.argwhere(~fb & fa), np.argwhere(fb & ~fa)
        assert not len(folded) and not len(leaked), (f"{what}{n}: {len(folded)} finite where the oracle is non-finite (first {folded[:4].tolist()}), "
                                                     f"{len(leaked)} non-finite where the oracle is finite (first {leaked[:4].tolist()}) of {a.size}")
    for n, a, b in zip(names, g_hip, g_ref):
        assert util.rel_err(_zeroed(a), _zeroed(b)) < P.RTOL_GRAD, (what + n, util.rel_err(_zeroed(a), _zeroed(b)))


@gpu
@pytest.mark.parametrize("name,poison,where", PARAMS, ids=IDS)
def test_gradient_masks_and_values_match_oracle(name, poison, where):
    """Test A of the module's docstring."""
    case, kw, opts, data, cfg, params, u_f, eta, hit = _problem(name, poison, where)
    model = _model(case, kw, opts, data, cfg, params)
    inputs = util.reference_inputs(data)
    eng = model.engine(inputs)
    _assert_route(eng, case)
    out, grads = _oracle_grads(data, cfg, params, u_f, eta)
    model(inputs, u_f=u_f, eta=eta)
    torch.cuda.synchronize()
    if case.frozen:
        assert getattr(eng.obs, "frozen_sorted", None) is not None           # (sorted rows / the two-call form: csrc/elbo_frozen.hip)
    terms = eng.loss_terms()
    g_hip = [g.cpu().numpy() for g in eng.grad_tensors()]
    names = _tensor_names(params)
    assert len(g_hip) == len(grads) == len(names)
    if case.frozen:                  # the scaler's gradient is not computed (trainable variables only): q's two tensors lead both lists
        names, g_hip, grads = names[:2], g_hip[:2], grads[:2]
    _assert_masks_and_values(names, g_hip, grads)
    kl = float(out["kl"])
    assert abs(terms["kl"] - kl) <= P.RTOL_LOSS * max(abs(kl), 1.0), (terms, kl)
    for k in ("nll", "loss"):
        assert not np.isfinite(float(out[k])) and not np.isfinite(terms[k]), (k, terms, float(out[k]))


@gpu
@pytest.mark.parametrize("name,poison,where", PARAMS, ids=IDS)
def test_training_stops_after_the_sanitised_step(name, poison, where):
    """Test B of the module's docstring: four steps asked for, one applied (every launch of steps 2 .. 4 honours `stop_flag`)."""
    case, kw, opts, data, cfg, params, u_f, eta, hit = _problem(name, poison, where)
    model = _model(case, kw, opts, data, cfg, params)
    inputs = util.reference_inputs(data)
    _assert_route(model.engine(inputs), case)
    rec, after = _oracle_step(data, cfg, params, u_f, eta)
    hist = model.train_model(inputs, 4, progress=False, noise=lambda i: (u_f, eta))
    eng = model._engine
    assert len(hist["loss"]) == 1 and not np.isfinite(hist["Grad Norm"][0]) and not np.isfinite(rec["Grad Norm"])
    assert abs(hist["F KLDiv"][0] - rec["F KLDiv"]) <= 1e-4 * max(abs(rec["F KLDiv"]), 1.0), (hist["F KLDiv"], rec["F KLDiv"])
    names, got = _tensor_names(params), [t.cpu().numpy() for t in eng.param_tensors()]
    assert len(names) == len(got) == len(after)
    if case.frozen:                  # (the oracle has no frozen scaler; q's Adam update does not depend on the other tensors')
        names, got, after = names[:2], got[:2], after[:2]
    for n, a, b in zip(names, got, after):
        fin = np.isfinite(b)         # everything but logit(0) of the root ASU's double-Wilson r: the CPU part
        assert np.array_equal(np.isfinite(a), fin) and np.array_equal(a[~fin], b[~fin].astype(np.float32)), n
        assert util.rel_err(a[fin], b[fin]) < 2e-4, (n, util.rel_err(a[fin], b[fin]))


@gpu
@pytest.mark.parametrize("where", ["inner", "last"])
@pytest.mark.parametrize("poison", list(CORE))
@pytest.mark.parametrize("name", list(SHARD_CASES))
def test_rank_shard_without_the_poisoned_row_stays_finite(name, poison, where):
    """The two rank shards of a 2-rank world on one GPU (all-reduce skipped, as test_rank_shards_sum_to_full_batch_on_gpu runs them): the
    shard that does not hold the poisoned row has an all-finite gradient, the sum of both has the oracle's mask and, zeroed, its values."""
    from careless_amd.engine import ElboEngine, make_shard
    kw = SHARD_CASES[name]
    case = Case(kw, "LANE" if kw["w"] == 10 else "MLP")
    case, kw, opts, data, cfg, params, u_f, eta, hit = _problem(case, poison, where)
    out, grads = _oracle_grads(data, cfg, params, u_f, eta)
    inputs = util.reference_inputs(data)
    parts, clean = [], 0
    for r in range(2):
        eng = ElboEngine(util.build_model(data, cfg, params, kw["L"], kw["w"]), inputs, seed=99, shard=make_shard(kw["N"], kw["R"], r, 2))
        assert eng.plan.route == _route(case.route) and not eng.owner
        eng.local_only = True
        du, de = eng._noise_to_device(u_f, eta)
        eng.forward_backward(0, du, de)
        torch.cuda.synchronize()
        g = [t.cpu().numpy() for t in eng.grad_tensors()]
        if not (eng.shard.start <= hit["row"] < eng.shard.stop):
            clean += 1
            assert all(np.isfinite(t).all() for t in g) and np.isfinite(eng.loss_terms()["nll"])
        else:
            assert not np.isfinite(eng.loss_terms()["nll"])
        parts.append(g)
    assert clean == 1
    _assert_masks_and_values(_tensor_names(params), [a + b for a, b in zip(*parts)], grads, "sum of the shards: ")
