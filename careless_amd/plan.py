"""What an engine decides before it owns a byte of device memory (split out of careless_amd/engine.py): which launches run the scaler
(`plan_scaler`, `chain_plan`), which plugin objects it runs and which it refuses (`prior_kind`, `posterior_kind`,
`check_neural_likelihood`, `check_deterministic`), how it shards (`wants_owner_shard`), its on / off switches (`switch`) -- and, per step
and per `ObsData`, THE route of the data term (`data_term_route`).  Host logic: functions of plain values and plugin objects; the
library is asked for routes and sizes only, nothing here needs a device.  The module reads no engine attribute and attaches nothing to
an `ObsData`; `ElboEngine._plan` stores `plan_scaler`'s answer as `self.plan`.
"""
from __future__ import annotations

import enum
import os
from dataclasses import dataclass
from typing import List, Optional

from careless_amd import _lib
from careless_amd.models.scaling.nn import dense_layout
from careless_amd.obs import GRANULE

REFPRIOR_KINDS = {"normal": _lib.CL_REFPRIOR_NORMAL, "laplace": _lib.CL_REFPRIOR_LAPLACE, "studentt": _lib.CL_REFPRIOR_STUDENTT,
                  "rice_woolfson": _lib.CL_REFPRIOR_RICE_WOOLFSON}       # ReferencePrior.engine_kind -> cl_refprior_args.kind
SPRIOR_KINDS = {"normal": _lib.CL_SPRIOR_NORMAL, "laplace": _lib.CL_SPRIOR_LAPLACE, "studentt": _lib.CL_SPRIOR_STUDENTT}       # ScalePrior.engine_kind -> cl_sprior_args.kind
BIJ_KINDS = {"exp": _lib.CL_BIJ_EXP, "softplus": _lib.CL_BIJ_SOFTPLUS}       # MetadataScaler.scale_bijector -> cl_mlp_args.bij_kind


class Route(enum.Enum):
    """The routes of one `ObsData`'s data term, in the order `data_term_route` asks for them."""
    FROZEN = 1        # behind a frozen scaler: no scaler launch at all (careless_amd/frozen.py)
    WIDE = 2          # layer by layer on the GEMM kernels (careless_amd/wide.py)
    CHAIN = 3         # a chain of layer blocks (`FusedPath._data_term_chain`)
    TWO_PASS = 4      # Laue rows the fused kernel does not take as harmonic groups, any rows under a scale prior: scaler forward, slot likelihood, scaler backward
    PEEL = 5          # the fused launch behind a peeled first layer
    FUSED = 6         # the fused launch on the scaler itself


def data_term_route(frozen_form, wide: bool, chained: bool, laue: bool, fused_laue: bool, peel: bool, scale_prior: bool = False) -> Route:
    """THE route decision, the precedence written once: a frozen scaler's form (`FrozenPath._frozen_form`, not None) before the plan's
    `wide`, before its chain of blocks (`chained`), before the two-pass Laue path -- `laue` data whose observation image is not packed
    for the single-pass kernels (`fused_laue`), and any data under a scale prior (`scale_prior`: its KL term sits between the two passes,
    careless_amd/sprior.py) --, before the plan's `peel`, before the plain fused launch.  Two-pass before peel: the plan may say `peel`
    for a scaler whose rows `pack_laue` then declines to pack; the two-pass path has no peeled launch."""
    if frozen_form is not None:
        return Route.FROZEN
    if wide:
        return Route.WIDE
    if chained:
        return Route.CHAIN
    if (laue and not fused_laue) or scale_prior:
        return Route.TWO_PASS
    return Route.PEEL if peel else Route.FUSED


@dataclass
class LayerBlock:
    """One launch of a chained scaler: Dense layers [l0, l1) of the stack; the last block also carries the Dense(2) head."""
    l0: int
    l1: int
    d_in: int          # width of the block's input: the metadata width for the first block, the hidden width for the others
    off: int           # offset of the block's parameters inside the scaler's flat W^T layout
    P: int             # number of parameters of the block (what its gradient partials hold)
    final: bool


def chain_plan(d: int, w: int, L: int, max_layers: int, last: int = 0) -> List[LayerBlock]:
    """Split a scaler of L Dense layers into the fewest, evenly sized blocks of at most `max_layers` layers (one block = one
    launch of the fused kernel, include/careless_hip.h: act_out / dH_ext / dX_out).  `last` > 0: the last block has exactly that many
    layers (round 6: 20 of them on the default scaler's lane kernel), the layers in front of it are split evenly."""
    if last > 0 and L > last:
        K = -(-(L - last) // max_layers)
        sizes = [(L - last) // K + (1 if i < (L - last) % K else 0) for i in range(K)] + [last]
        K += 1
    else:
        K = -(-L // max_layers)
        sizes = [L // K + (1 if i < L % K else 0) for i in range(K)]
    layers, head = dense_layout(d, w, L)
    off_of = lambda l: layers[l][0] if l < L else head
    blocks, l0 = [], 0
    for k, n in enumerate(sizes):
        l1 = l0 + n
        final = k == K - 1
        P = off_of(l1) - off_of(l0) + (2 * w + 2 if final else 0)
        blocks.append(LayerBlock(l0, l1, d if k == 0 else w, off_of(l0), P, final))
        l0 = l1
    return blocks


@dataclass
class ScalerPlan:
    wide: bool                             # layer by layer (careless_amd/wide.py): no fused launch holds the scaler
    peel: bool                             # the first Dense layer runs in front of the training launch (csrc/elbo_peel.hip)
    blocks: Optional[List[LayerBlock]]     # a chain of layer blocks: deeper than one launch holds
    chain_lane: bool                       # ... whose last block runs on the lane kernel (dZ_0 out, then cl_chain_dx)
    route: int                             # cl_mlp_route of the training launch (`ElboEngine.training_launch`); CL_ROUTE_NONE when wide


def plan_scaler(lib, d: int, w: int, L: int, K: int = 0, laue: bool = False, two_pass: bool = False, gmax: int = 1, ev11: bool = False,
                deterministic: bool = False, lik_kind: int = 0, scale_prior: bool = False) -> ScalerPlan:
    """How `ElboEngine` runs L Dense layers of width w on d columns with K per-image layers (`gmax`: the largest harmonic group): the plan
    chooses the launches -- peel the first layer, cut a deep scaler into blocks, go layer by layer --, the library's routes decide.
    `scale_prior`: the engine has a scale prior, whose KL term sits between a forward and a backward launch: monochromatic rows take the
    two-pass launches as well, a chain's last block its two-pass form (no lane kernel: that one is a full step)."""
    NONE, LANE, NARROW, LANE_IMGL = _lib.CL_ROUTE_NONE, _lib.CL_ROUTE_LANE, _lib.CL_ROUTE_NARROW, _lib.CL_ROUTE_LANE_IMGL
    proto = dict(d=d, w=w, L=L, S=1, refl_id=1, meta_t=1, iobs=1, sig=1, mlp=1, z_f=1, dz_f=1, partials=1, scalars=1, stop_flag=1,
                 ev11=int(ev11), d_ev11=int(ev11), lik_kind=lik_kind)      # (the lane and the narrow kernel refuse CL_LIK_LAPLACE: the routes say so)
    det = dict(dzf_obs=1, dimg_obs=1, nll_part=1, det_slot=1, ev11_part=int(ev11)) if deterministic else {}
    route = lambda mode, **kw: _lib.mlp_route(lib, mode, **{**proto, **kw})
    if w > 64 or d > 64:        # a layer's activations no longer fit a wave's registers next to the weight-gradient blocks
        return ScalerPlan(True, False, None, False, NONE)
    max_plain = int(lib.cl_mlp_max_layers(w))
    if K == 0 and L > max_plain:
        # a chain of layer blocks, activations exchanged through HBM.  The LAST 20 layers (widths 11, 12: 19, the deepest twelve-wide instance
        # without spilled registers) and the head on the lane kernel where it takes them, dZ_0 out, `cl_chain_dx` turns it into the gradient
        # of the block's input (round 6: 24 x 10 at 4 M observations 3.13 -> 1.4 ms per step).  Laue data: the two-pass path.
        last = 19 if w in (11, 12) else 20
        chain_lane = not laue and not scale_prior and route(0, d=w, L=last, dZ0_out=1) == LANE
        blocks = chain_plan(d, w, L, min(max_plain, last) if chain_lane else max_plain, last=last if chain_lane else 0)
        last_block = dict(d=w, L=blocks[-1].l1 - blocks[-1].l0, **({"dZ0_out": 1} if chain_lane else {"dX_out": 1}))
        return ScalerPlan(False, False, blocks, chain_lane, route(0, **last_block, **det))
    # Laue rows the fused kernel cannot take as harmonic groups: the two-pass path, cl_mlp_forward + cl_mlp_backward_ext on the scaler itself
    two_pass = (laue and (two_pass or gmax > GRANULE)) or scale_prior
    layout = dict(dict(row_map=1, tile_img=1, imgl=1, d_imgl=1, n_imgl=K, n_images=1) if K else {},
                  **(dict(row_map=1, gmeta=1, tile_gmax=1) if laue and not two_pass else {}))
    unpeeled, peeled = route(0, **layout), route(0, **layout, d=w, dZ0_out=1)
    if K:       # (the lane kernel's per-image-layer instances behind the peeled layer)
        peel = unpeeled != LANE_IMGL and peeled == LANE_IMGL
    else:
        # more columns than the lane / narrow kernel holds: cl_peel_forward computes the first layer's pre-activations, the fused kernel runs
        # on them (w "metadata columns") with an identity first layer and hands back dZ_0 for cl_peel_backward.  (Widths 13 .. 15
        # are no faster on the narrow kernel than on elbo_mlp.hip's 16-wide instance: profiles/r5_envelope.txt, 20 x 15 on 37 columns 2.02 vs 2.19 ms.)
        peel = unpeeled not in (LANE, NARROW) and peeled in (LANE, NARROW) and w <= 12
    peel = peel and bool(lib.cl_peel_supported(d, w, L))
    train = dict(layout, d=w, dZ0_out=1) if peel else layout          # (the two-pass path has no peeled launch)
    launches = [route(1, **layout, loc_out=1, sig_out=1), route(2, **layout, dO_ext=1)] if two_pass else [route(0, **train)]
    if NONE in launches:
        return ScalerPlan(True, False, None, False, NONE)
    return ScalerPlan(False, peel, None, False, launches[-1] if two_pass else route(0, **train, **det))


def prior_kind(prior, owner: bool = False) -> int:
    """CL_PRIOR_* under which the engine runs `prior` (`owner`: on a reflection-owner split); NotImplementedError for what it does not
    run.  Host logic: needs no device."""
    from careless_amd.models.priors.empirical import ReferencePrior
    from careless_amd.models.priors.wilson import DoubleWilsonPrior, WilsonPrior
    if isinstance(prior, ReferencePrior):
        if prior.base_dist is None or prior.engine_kind not in REFPRIOR_KINDS:
            raise NotImplementedError(f"prior {type(prior).__name__} has no base distribution the HIP engine evaluates (use one of its subclasses: "
                                      "Normal-, Laplace-, StudentT- or RiceWoolfsonReferencePrior)")
        if owner:
            raise NotImplementedError(f"the reflection-owner split runs the Wilson prior only, not {type(prior).__name__}: use the row split")
        return _lib.CL_PRIOR_REFERENCE
    if isinstance(prior, DoubleWilsonPrior):
        return _lib.CL_PRIOR_DOUBLE_WILSON
    if isinstance(prior, WilsonPrior):
        return _lib.CL_PRIOR_WILSON
    raise NotImplementedError(f"prior {type(prior).__name__} is not supported by the HIP engine yet")


def posterior_kind(q) -> str:
    """The surrogate posteriors the engine samples: "truncated_normal" (cl_tn_forward / _backward) or "rice_woolfson" (cl_rw_forward /
    _backward: the trainable class of `RiceWoolfson.from_loc_and_scale`); NotImplementedError for anything else -- the host-side
    `RiceWoolfson(loc, scale, centric)` of the reference priors included."""
    from careless_amd.models.merging.surrogate_posteriors import TrainableRiceWoolfson, TruncatedNormal
    if isinstance(q, TruncatedNormal):
        return "truncated_normal"
    if isinstance(q, TrainableRiceWoolfson):
        return "rice_woolfson"
    raise NotImplementedError(f"surrogate posterior {type(q).__name__} is not supported by the HIP engine")


def check_neural_likelihood(lik, laue: bool, world: int = 1, lib=None) -> bool:
    """Is `lik` a neural likelihood (`NeuralNormalLikelihood`: an error model learned from the data, csrc/elbo_nlik.hip)?  NotImplementedError
    for what the engine does not run it on: Laue data (the reference has no Laue form), the Evans-2011 error model beside it (the
    reference has no such class), more than one rank (the mean of delta over all rows would take two more collectives per step: DESIGN 7),
    a network the kernels do not hold.  Host logic: needs no device (`lib`: the loaded library, for `cl_nlik_supports`)."""
    if not getattr(lik, "neural", False):
        return False
    name = type(lik).__name__
    if laue:
        raise NotImplementedError(f"likelihood {name}: the neural likelihood is monochromatic only (the reference has no Laue form)")
    if getattr(lik, "ev11", False):
        raise NotImplementedError(f"likelihood {name}: a neural likelihood and the Evans-2011 error model are mutually exclusive (the reference has no such class)")
    if world > 1:
        raise NotImplementedError(f"likelihood {name}: the neural likelihood runs on one rank (its mean over all rows would need two more "
                                  f"collectives per step); got a shard of {world} ranks")
    lib = _lib.get_lib() if lib is None else lib
    if not lib.cl_nlik_supports(int(lik.n_layers), int(lik.width)):
        raise NotImplementedError(f"likelihood {name}({lik.n_layers}, {lik.width}): the HIP kernels hold 1 .. 4 hidden layers of width 1 .. 32")
    return True


def check_scale_prior(scale_prior, scale_kl_weight):
    """The scale prior the engine runs (`models/priors/scale.py`), or None without one.  As the reference executes it (careless/models/
    merging/variational.py:156-163): a prior beside `scale_kl_weight=None` reaches `add_kl_div(..., weight=None)` and fails in
    `add_loss(None * kl_div)` -- a TypeError here too; with a weight, the term is added with weight 1 and reduction 'mean' WHATEVER the
    weight's value (only that it is not None is read).  NotImplementedError for anything that is not one of the three families whose density
    the library evaluates.  Host logic: needs no device."""
    if scale_prior is None:
        return None
    from careless_amd.models.priors.scale import ScalePrior
    if not isinstance(scale_prior, ScalePrior) or scale_prior.engine_kind not in SPRIOR_KINDS:
        raise NotImplementedError(f"scale_prior {type(scale_prior).__name__} is not supported by the HIP engine: use NormalScalePrior, "
                                  "LaplaceScalePrior or StudentTScalePrior (careless_amd.models.priors.scale)")
    if scale_kl_weight is None:
        raise TypeError("unsupported operand type(s) for *: 'NoneType' and 'Tensor': a scale_prior with scale_kl_weight=None fails in the "
                        "reference as well (careless/models/merging/variational.py:160-161 call add_kl_div with weight=None); pass any "
                        "scale_kl_weight -- its value is not used, the term has weight 1")
    return scale_prior


def check_scale_prior_route(wide: bool, owner: bool, deterministic: bool = False, laue: bool = False, imgl: bool = False, S: int = 1) -> None:
    """NotImplementedError for the routes a scale prior's KL term has no launch on.  It sits between cl_mlp_forward and
    cl_mlp_backward_ext of the two-pass launches (careless_amd/sprior.py): the layer-by-layer route of scalers wider than 64 (`wide`) has
    neither, and the reflection-owner split (`owner`) cuts rows by reflection where the term is a mean over rows.  `deterministic`: the
    mode takes the route where `cl_slot_rows` has its store form -- monochromatic rows (not `laue`), no per-image layers (`imgl`), `S`
    dividing 64.  Host logic: needs no device."""
    if wide:
        raise NotImplementedError("scale_prior: the layer-by-layer route (scaler width or metadata width beyond 64) has no two-pass launches "
                                  "for the term to sit between; it runs on scalers the fused kernels hold")
    if owner:
        raise NotImplementedError("scale_prior: the reflection-owner split is not supported (the term is a mean over rows); use the row split")
    if deterministic and (laue or imgl or 64 % S != 0):
        raise NotImplementedError("scale_prior: deterministic mode covers monochromatic rows without per-image layers and a sample count that divides "
                                  "64 (the store form of cl_slot_rows: a row's samples inside one wave); the Laue slot kernels keep their float atomics")


def switch(model, attr: Optional[str], env: str, default: bool = False, env_adds: bool = False) -> bool:
    """One on / off switch of the engine: `model.<attr>` where it is set (not None), else the environment variable `env` ("1" on, "0"
    off), else `default`.  `env_adds`: the variable also switches on what the attribute leaves off (`deterministic`)."""
    want = getattr(model, attr, None) if attr is not None else None
    if want is None or (env_adds and not want):
        env = os.environ.get(env, "")
        want = (env != "0") if default else (env == "1")
    return bool(want)


def check_deterministic(plan: ScalerPlan, laue: bool, two_pass: bool, imgl: bool, S: int, dw_trainable: bool) -> None:
    """NotImplementedError for what the deterministic mode does not cover, of a scaler run by `plan` on `laue` data (`two_pass`: asked for
    by the model) with per-image layers (`imgl`), S samples and a trainable double-Wilson r (`dw_trainable`).  Host logic: needs no device."""
    # (wide scalers: monochromatic rows only -- they are their own slots and one kernel holds every float atomic of the path --, with a
    #  sample count that divides 64, so that a row's samples sit inside one wave)
    wide_det_ok = plan.wide and not laue and 64 % S == 0
    # (per-image layers: where the training launch has a route with the deterministic stores -- the lane kernel's instances, one wave per image)
    imgl_det_ok = plan.route != _lib.CL_ROUTE_NONE
    if two_pass or (plan.wide and not wide_det_ok) or (imgl and not imgl_det_ok) or (plan.blocks is not None and laue) or dw_trainable:
        raise NotImplementedError("deterministic mode covers monochromatic and single-pass Laue data, the Wilson and the double-Wilson prior "
                                  "(fixed r), Normal / Student-T likelihoods with or without the Evans-2011 error model, the Laplace likelihood, scalers of any depth up to "
                                  "width 64, up to three per-image layers on 2 .. 20 Dense layers of width 5 .. 10 (two on 19; the default scaler's kernels) and, "
                                  "for monochromatic data with a sample count that divides 64, scalers wider than 64; the two-pass "
                                  "Laue path (also under a chained scaler), a trainable double-Wilson r and every other shape with per-image layers "
                                  "keep their float atomics")


def wants_owner_shard(want: bool, prior, world: int, owner_given: bool, laue: bool, double_wilson: bool, wide: bool, imgl: bool,
                      deterministic: bool) -> bool:
    """Does an engine asked for the reflection-owner split (`want`) on `world` ranks cut its rows by reflection (`owner_shard`)?  Not on one
    rank, not when its shard already is an owner's (`owner_given`), not for Laue data (a harmonic group mixes reflections), the
    double-Wilson prior (a child's parent may live on another rank), wide scalers, per-image layers or the deterministic mode: they keep
    the row split.  NotImplementedError where the split is asked for or given and the prior is not one it runs.  Host logic: needs no device."""
    if owner_given or (want and world > 1):
        prior_kind(prior, owner=True)                # (the reflection-owner split is Wilson-only: raises for a reference prior)
    return bool(want and world > 1 and not laue and not double_wilson and not wide and not imgl and not deterministic and not owner_given)


def reference_prior_arrays(prior, R: int) -> dict:
    """What `cl_ref_prior` takes from an empirical reference prior, expanded to all R reflections (host arrays); ValueError where the
    prior's lengths do not match R or a Student-t prior has no positive dof."""
    out = dict(kind=REFPRIOR_KINDS[prior.engine_kind], dof=float(prior.dof), loc=prior.loc_full(R), scale=prior.scale_full(R),
               observed=prior.observed_mask(R), centric=prior.centric_full(R))
    if out["kind"] == _lib.CL_REFPRIOR_STUDENTT and not out["dof"] > 0.0:
        raise ValueError(f"{type(prior).__name__} needs dof > 0 (got {prior.dof})")
    return out
