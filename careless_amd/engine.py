"""Host side of the MI355X ELBO engine: turns the plugin objects of a `VariationalMergingModel` plus the reference's
`inputs` tuple into device buffers, and enqueues one ELBO training step as a fixed sequence of C-ABI calls.

What one step replaces in the reference: `train_step_with_gradient_norm` (careless/models/merging/variational.py:185-224)
= forward (`call`, :141-183), `tape.gradient`, `tf.linalg.global_norm`, non-finite sanitise, Adam.

Step schedule (all on one HIP stream, no host synchronisation):
    cl_tn_forward (clears the step's accumulators on its way) -> [cl_nlik_forward: neural likelihood] -> cl_elbo_mono_fwd_bwd
    -> [cl_nlik_backward: neural likelihood] -> [cl_ref_prior: empirical reference priors]
    -> cl_tn_backward (carries cl_reduce_partials)        (a Rice-Woolfson posterior: cl_rw_forward / cl_rw_backward in their place)
    -> [cl_owner_qnorm + all-reduce, data-parallel only: the flat gradient (row split) or its tail + 4 norm terms (reflection-owner
    split)] -> [cl_grad_sqnorm: clip modes only] -> cl_adam_step -> cl_step_finalize

HBM layout owned by the engine (see include/careless_hip.h):
    params / m / v / grads : one flat fp32 vector  [ q_loc_raw (R) | q_scale_raw (R) | scaler W^T layout (P) | image scales (M-1) | ... ]
    workspace              : [ dz_f (R*S) | grads (n) + message tail | scalars (4 doubles) | per-tensor norms | owner-mode scratch ]
    observation shard      : refl_id i32, image_id i32, meta_t [d][n_pad], iobs, sig [, noise_row]   (immutable)
PyTorch is used for device memory, streams and torch.distributed only.

Round 4: the observation layouts and the data-parallel splits live in careless_amd/obs.py, the layer-by-layer path of scalers wider
than 64 in careless_amd/wide.py, the data term of a step behind a frozen scaler in careless_amd/frozen.py (mixins of `ElboEngine`); this file keeps the flat parameter layout, the step schedule and the helpers
behind the plugin protocol methods.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from functools import cached_property
from itertools import accumulate
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from careless_amd import _lib
from careless_amd._lib import AdamArgs, DetArgs, LaueArgs, MlpArgs, NlikArgs, RefPriorArgs, RwArgs, TnArgs, check, ptr
from careless_amd.frozen import FrozenPath
from careless_amd.models.base import BaseModel
from careless_amd.models.scaling.image import image_layer_layout
from careless_amd.models.scaling.nn import dense_layout, dense_slices
# (re-exported: the tests, bench.py and scripts import the sharding / layout names from here)
from careless_amd.obs import (GRANULE, ObsChunks, ObsData, Shard, _EmptyObs, _ShardRows, _np, _tiles, image_order, laue_group_shard,  # noqa: F401
                              launch_row_limit, make_shard, meta_by_image, meta_feature_major, meta_row_major, owner_bounds, owner_shard,
                              pack_by_image, pack_laue)
from careless_amd.wide import WidePath, WideShape, hidden_forward, row_chunks

TILE = _lib.CL_MLP_TILE
REFPRIOR_KINDS = {"normal": _lib.CL_REFPRIOR_NORMAL, "laplace": _lib.CL_REFPRIOR_LAPLACE, "studentt": _lib.CL_REFPRIOR_STUDENTT,
                  "rice_woolfson": _lib.CL_REFPRIOR_RICE_WOOLFSON}       # ReferencePrior.engine_kind -> cl_refprior_args.kind
BIJ_KINDS = {"exp": _lib.CL_BIJ_EXP, "softplus": _lib.CL_BIJ_SOFTPLUS}       # MetadataScaler.scale_bijector -> cl_mlp_args.bij_kind
FORWARD_CHUNK_BYTES = 256 << 20       # `scaler_forward`, layer by layer: bytes of its two alternating hidden buffers; sizes the row chunk
HISTORY_KEYS = ("loss", "F KLDiv", "NLL", "Grad Norm")


def require_gpu(what: str) -> torch.device:
    """The product has no CPU path: every compute entry point calls this first."""
    _lib.get_lib()
    if not torch.cuda.is_available():
        raise _lib.CarelessHipError(f"{what} needs an AMD GPU (gfx950); careless_amd has no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _copy_args(ma: MlpArgs) -> MlpArgs:
    a = MlpArgs()
    C.memmove(C.byref(a), C.byref(ma), C.sizeof(MlpArgs))
    return a


def scaler_fields(a: MlpArgs, mlp, d: int, pmlp: int, imgl=None, pimgl=None, tile_img=None, row_map=None) -> MlpArgs:
    """The scaler's own fields of `cl_mlp_args`, filled in one place for the training step (`ElboEngine._mlp_args`) and the forward-only
    path (`scaler_forward`): the Dense stack at `pmlp`, the per-image layers `imgl` at `pimgl`, and what a packed layout adds (`a.n_pad` is set)."""
    a.mlp = pmlp
    a.d, a.w, a.L, a.leak = d, mlp.width, mlp.n_layers, mlp.leakiness
    a.bij_kind, a.eps = BIJ_KINDS[mlp.scale_bijector], mlp.epsilon
    if row_map is not None:
        a.n_obs, a.row_map = a.n_pad, ptr(row_map)       # packed: validity is per row (row_map / refl_id = -1)
    if imgl is not None:
        a.imgl, a.n_imgl, a.n_images, a.tile_img = pimgl, imgl.n_image_layers, imgl.max_images, ptr(tile_img)
    return a


def block_fields(a: MlpArgs, b: "LayerBlock", pmlp: int, x: int) -> MlpArgs:
    """`a` turned into the launch of block `b` of a chain: its slice of the parameters at `pmlp`, its input `x` (metadata or the previous block's output)."""
    a.mlp = pmlp + 4 * b.off
    a.d, a.L, a.meta_t = b.d_in, b.l1 - b.l0, x
    return a


# ------------------------------------------------------------------------------------------------------------
# layout of the flat parameter vector
# ------------------------------------------------------------------------------------------------------------
FLAT_GROUPS = ("q_loc", "q_scale", "mlp", "img", "imgl", "ev11", "dwr")      # the groups of the flat vector, in storage order


@dataclass
class FlatLayout:
    """The flat parameter vector (`groups`).  The group "ev11" holds the likelihood's trainable floats: the three scalars of the Evans-2011
    error model, or the network of a neural likelihood (`lik_dense`, its Dense slices) -- never both."""
    R: int
    P: int
    n_img: int                 # M - 1 trainable image scales (0 when image scales are off)
    seg_off: List[int]         # tensor boundaries (Keras trainable-variable granularity) for per-tensor clipnorm
    seg_owner: List[str]       # "q" | "scaler" | "likelihood" per tensor (for --freeze-*)
    n_ev11: int = 0            # the likelihood's trainable floats: 3 with the Evans-2011 error model, P_lik with a neural likelihood
    n_dwr: int = 0             # number of ASUs with --optimize-double-wilson-r
    n_imgl: int = 0            # floats of the per-image layers (NeuralImageScaler: `image_layer_layout`)
    lik_dense: Optional[list] = None      # a neural likelihood's Dense slices [(kernel offset, out, in, bias offset)] inside its group

    @cached_property
    def groups(self) -> Tuple[Tuple[str, int, int], ...]:
        """THE table of the flat vector: (name, offset, count) of its groups in storage order; an absent group has count 0.  Every
        offset below, `n`, the binding of the plugin objects (`bind_flat`) and the per-tensor split (`split_flat`) come from it."""
        counts = (self.R, self.R, self.P, self.n_img, self.n_imgl, self.n_ev11, self.n_dwr)
        return tuple(zip(FLAT_GROUPS, accumulate(counts, initial=0), counts))

    @cached_property
    def _span(self) -> Dict[str, Tuple[int, int]]:
        return {name: (off, cnt) for name, off, cnt in self.groups}

    def off(self, group: str) -> int:
        return self._span[group][0]

    def view(self, flat: torch.Tensor, group: str) -> torch.Tensor:
        off, cnt = self._span[group]
        return flat[off:off + cnt]

    n = property(lambda self: sum(self.groups[-1][1:]))
    off_mlp = property(lambda self: self.off("mlp"))
    off_img = property(lambda self: self.off("img"))
    off_imgl = property(lambda self: self.off("imgl"))
    off_ev11 = property(lambda self: self.off("ev11"))
    off_dwr = property(lambda self: self.off("dwr"))


def make_layout(R: int, d: int, w: int, L: int, n_img: int, n_ev11: int = 0, n_dwr: int = 0, imgl=None, lik_dense=None) -> FlatLayout:
    """`imgl` = (K, M): K per-image layers over M images (NeuralImageScaler).  `lik_dense`: the Dense slices of a neural likelihood's
    network (`NeuralLikelihood.layer_slices`) -- the likelihood's group then holds the network, one segment per kernel and per bias."""
    if lik_dense is not None and n_ev11:
        raise NotImplementedError("a neural likelihood and the Evans-2011 error model are mutually exclusive (the reference has no such class)")
    seg, owner = [0, R, 2 * R], ["q", "q"]
    for _, out, _, ob in dense_slices(d, w, L):       # kernel and bias of every Dense layer, then of the head
        seg += [2 * R + ob, 2 * R + ob + out]; owner += ["scaler", "scaler"]
    off = seg[-1]
    P = off - 2 * R
    if n_img > 0:
        off += n_img; seg.append(off); owner.append("scaler")
    n_imgl = 0
    if imgl is not None:
        K, M = imgl
        blocks, n_imgl = image_layer_layout(K, M, w)
        for ow, ob in blocks:                # ImageLayer kernel (M, w, w) and bias (M, w) (image.py:76-88)
            seg += [off + ob, off + ob + M * w]; owner += ["scaler", "scaler"]
        off += n_imgl
    for _ in range(n_ev11):              # Sdfac, Sdadd, SdB: three scalar variables (mono.py:42-44)
        off += 1; seg.append(off); owner.append("likelihood")
    if lik_dense is not None:            # kernel and bias of every Dense layer of the likelihood's network, then of its head (mono.py:79-92)
        for _, out, _, ob in lik_dense:
            seg += [off + ob, off + ob + out]; owner += ["likelihood", "likelihood"]
        n_ev11 = seg[-1] - off
        off = seg[-1]
    if n_dwr > 0:                        # the double-Wilson r vector (wilson.py:105-110)
        off += n_dwr; seg.append(off); owner.append("prior")
    return FlatLayout(R, P, n_img, seg, owner, n_ev11, n_dwr, n_imgl, None if lik_dense is None else list(lik_dense))


def bind_flat(flat: torch.Tensor, lay: FlatLayout, q, mlp, img=None, imgl=None, lik=None, prior=None) -> None:
    """The plugin objects become views into `flat`: the tensor that holds each group of `lay` is copied into it and the plugin attribute
    rebound to that slice, in one loop over (group, holder, attribute).  (A group whose count is 0 is passed over: its holder may be
    None.)  Any device: needs no engine."""
    for group, holder, attr in (("q_loc", q, "loc_raw"), ("q_scale", q, "scale_raw"), ("mlp", mlp, "flat"), ("img", img, "_scales"),
                                ("imgl", imgl, "flat"), ("ev11", lik, "raw"), ("dwr", prior, "r_raw")):
        view = lay.view(flat, group)
        if view.numel() > 0:
            view[:] = getattr(holder, attr).to(flat.device)
            setattr(holder, attr, view)


def split_flat(g: torch.Tensor, lay: FlatLayout, dense, imgl_views=None) -> List[torch.Tensor]:
    """`g`, a vector laid out like the parameters, per trainable tensor in the oracle's order and Keras shapes: the groups of `lay` in
    order, the Dense stack by `dense` (`MetadataScaler.layer_slices`) as kernel (in, out) and bias per layer, the per-image block by
    `imgl_views` (`NeuralImageScaler.layer_views`), a neural likelihood's network by `lay.lik_dense` like the Dense stack."""
    out = []
    for name, off, cnt in lay.groups:
        v = g[off:off + cnt]
        if name == "mlp":
            for ow, o, i, ob in dense:
                out += [v[ow:ow + o * i].view(o, i).t(), v[ob:ob + o]]
        elif name == "imgl" and cnt > 0:
            out += imgl_views(v)
        elif name == "ev11" and cnt > 0 and lay.lik_dense is not None:
            for ow, o, i, ob in lay.lik_dense:
                out += [v[ow:ow + o * i].view(o, i).t(), v[ob:ob + o]]
        elif cnt > 0:
            out.append(v)
    return out


@dataclass(frozen=True)
class Workspace:
    """The step workspace in floats, as (offset, count) per region (`carve_workspace`).  `dz_f`, `grads`, the four floats of slack behind
    them, `msg_norm`, `scalars` (4 doubles), `seg_sq` (nseg doubles) and `own_scratch` (5 doubles) follow each other without overlap;
    `msg` (what an owner-mode step all-reduces: the gradient behind a and b, the slack, the norm terms) and `ws_step` (what such a step
    clears: everything from the gradient's padding on) are spans over them."""
    owner: bool
    dz_f: Tuple[int, int]
    grads: Tuple[int, int]
    msg: Tuple[int, int]
    msg_norm: Tuple[int, int]
    scalars: Tuple[int, int]
    seg_sq: Tuple[int, int]
    own_scratch: Tuple[int, int]
    ws_step: Tuple[int, int]
    total: int

    @property
    def aligned(self) -> bool:
        """In a 16-byte aligned allocation the buffer a data-parallel step all-reduces -- the flat gradient (row split) or the message
        (reflection-owner split) -- and `ws_step` start on 16-byte boundaries, the doubles on 8-byte ones."""
        reduced = self.msg if self.owner else self.grads
        return reduced[0] % 4 == 0 and self.ws_step[0] % 4 == 0 and all(r[0] % 2 == 0 for r in (self.scalars, self.seg_sq, self.own_scratch))


def carve_workspace(R: int, S: int, n: int, nseg: int, owner: bool) -> Workspace:
    """Offsets of the step workspace for R reflections, S samples, n parameters in nseg tensors.  The buffer a step all-reduces starts on
    a 16-byte boundary: the flat gradient (row split), or -- reflection-owner split -- what lies behind a and b in it (two floats of
    padding in front of the gradient when 2 R is not a multiple of four)."""
    pad = (-2 * R) % 4 if owner else 0
    g = (R * S + 3) // 4 * 4 + pad
    sc = (g + n + 8 + 3) // 4 * 4           # 4 floats of slack, then the 4 norm terms of the owner-mode message; 16-byte aligned
    seg = sc + 8                            # 4 doubles = 8 floats
    own = seg + 2 * nseg                    # owner mode: 4 double accumulators + the block ticket of cl_owner_qnorm
    total = own + 10
    return Workspace(owner, dz_f=(0, R * S), grads=(g, n), msg=(g + 2 * R, n + 8 - 2 * R), msg_norm=(g + n + 4, 4), scalars=(sc, 8),
                     seg_sq=(seg, 2 * nseg), own_scratch=(own, 10), ws_step=(g - pad, total - (g - pad)), total=total)


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
                deterministic: bool = False, lik_kind: int = 0) -> ScalerPlan:
    """How `ElboEngine` runs L Dense layers of width w on d columns with K per-image layers (`gmax`: the largest harmonic group): the plan
    chooses the launches -- peel the first layer, cut a deep scaler into blocks, go layer by layer --, the library's routes decide."""
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
        chain_lane = not laue and route(0, d=w, L=last, dZ0_out=1) == LANE
        blocks = chain_plan(d, w, L, min(max_plain, last) if chain_lane else max_plain, last=last if chain_lane else 0)
        last_block = dict(d=w, L=blocks[-1].l1 - blocks[-1].l0, **({"dZ0_out": 1} if chain_lane else {"dX_out": 1}))
        return ScalerPlan(False, False, blocks, chain_lane, route(0, **last_block, **det))
    # Laue rows the fused kernel cannot take as harmonic groups: the two-pass path, cl_mlp_forward + cl_mlp_backward_ext on the scaler itself
    two_pass = laue and (two_pass or gmax > GRANULE)
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


@dataclass
class DetBuffers:
    """Deterministic mode, per observation set (`ObsData.det`, `ElboEngine._det_attach`): the per-observation stores of the kernels and the
    sort orders `cl_det_reduce` walks."""
    slot: Optional[torch.Tensor]        # position of every observation in reflection order (cl_mlp_args.det_slot); None past the 32-bit byte offset
    dzf: torch.Tensor                   # amplitude gradient per (observation, sample)
    dimg: torch.Tensor                  # image-scale term per observation
    nll: torch.Tensor                   # NLL per workgroup: `grid` slots per piece, then the slot / padded-slot likelihood launch's
    refl: Tuple[torch.Tensor, torch.Tensor]     # (permutation, segment starts) by reflection
    img: Tuple[torch.Tensor, torch.Tensor]      # ... by image
    M: int                              # number of images
    pieces: int                         # launches the set is cut into
    grid: int                           # workgroups of one of them
    ev11: Optional[torch.Tensor] = None         # Evans-2011 gradients: three floats per wave of every launch


@dataclass
class NlikBuffers:
    """A neural likelihood, per observation set (`ObsData.nlik` / `ObsChunks.nlik`, `ElboEngine._nlik_attach`): the set's rows in the
    caller's order -- the mean of delta couples them all, also where `ObsChunks` cuts the set into pieces."""
    n: int
    iobs: torch.Tensor                  # [n] raw Iobs, SigIobs in the caller's row order
    sigiobs: torch.Tensor
    sigpred: torch.Tensor               # [n + TILE]: cl_nlik_forward's output; the tail keeps the 1.0 of a plain layout's padding rows
    ws: torch.Tensor                    # cl_nlik_workspace_bytes
    ipred: Optional[torch.Tensor] = None        # [n][S]: the data term's ipred_out when the caller brings none
    image_key: Optional[tuple] = None   # what `image` / `pos` were built for: per piece, the layout's own order or a frozen scaler's sorted rows
    image: Optional[torch.Tensor] = None        # the pieces' sig-shaped images, one behind the other (None: every piece reads sigpred itself)
    pos: Optional[torch.Tensor] = None  # int32 [n]: position of row i in `image`


@dataclass
class PeelBuffers:
    """A peeled first layer, per observation set (`ObsData.peel`, `ElboEngine._peel_bufs`), feature-major like meta_t."""
    u: torch.Tensor                     # the layer's pre-activations
    dz0: torch.Tensor                   # their gradient
    parts: torch.Tensor                 # weight-gradient partials of cl_peel_backward
    nparts: int


# ------------------------------------------------------------------------------------------------------------
# the engine
# ------------------------------------------------------------------------------------------------------------
class ElboEngine(WidePath, FrozenPath):
    SLOT_ROWS_ONE_LAUNCH = True      # rows that are their own slot: predict + log-prob + gradient in one `cl_slot_rows` launch (tests flip it)
    local_only = False               # test hook: a rank shard on one device, the per-rank partial gradient stays in place (no collective call)
    force_allreduce = False          # CARELESS_FORCE_DIST=1: a one-rank run makes every collective call of the multi-GPU step

    def __init__(self, model, inputs, seed: int = 1234, shard: Optional[Shard] = None, process_group=None,
                 grid: Optional[int] = None):
        self.device = require_gpu("ElboEngine")
        self.lib = _lib.get_lib()
        self.model = model
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.process_group = process_group
        self.peel_params = self.peel_grad = None    # the peeled scaler's parameters and reduced gradient (`_peel_bufs`)
        self._wide = None                           # work buffers of the layer-by-layer path (`_wide_setup`)
        self._pending_reduce = None                 # a partial reduction left to the step's cl_tn_backward launch (`_data_term`)
        self._grid_arg = grid
        if switch(model, None, "CARELESS_FORCE_DIST"):         # (no model attribute: `force_allreduce` is set on the engine)
            import torch.distributed as dist
            self.force_allreduce = dist.is_available() and dist.is_initialized()
        self._read_plugins(model, inputs)
        check_neural_likelihood(self.lik, self.laue, shard.world if shard is not None else 1, self.lib)
        self._reflection_constants()
        two_pass = self._plan(inputs)
        if self.deterministic:
            check_deterministic(self.plan, self.laue, two_pass, self.imgl is not None, self.S, self.dw_trainable)
        self._bind_parameters()
        self._decide_shard(inputs, shard)
        # A frozen scaling model (`--freeze-scales`; the half-dataset trainings of `--merge-half-datasets`, reference careless.py:102-128):
        # its output (loc, sigma) per observation does not change from step to step, so a step needs neither its forward nor its backward
        # pass -- only the sampling / likelihood part (careless_amd/frozen.py).  An engine built around a frozen scaler lays its observations
        # out for that (`_frozen_layout_kw`).
        self.frozen_fast = switch(model, "frozen_scaler_fast_path", "CARELESS_HIP_FROZEN_FAST", default=True)
        self._frozen_layout = self._frozen_layout_kw() is not None
        self._frozen_epoch = 0
        self.scaler_frozen = False
        self.obs = self._build_obs(inputs, self.shard.start, self.shard.stop, grid, self.laue_groups, rows=self.shard.rows if self.owner else None)
        self._build_workspace()
        self.refresh_config()

    def _read_plugins(self, model, inputs):
        """The plugin objects the engine runs -- `q, prior, lik, mlp, img, imgl` -- or NotImplementedError / ValueError for those it does
        not; the sizes `R, N_total, d, S` and what the objects alone decide (`laue`, `ev11`, `double_wilson`, `dw_trainable`, `deterministic`)."""
        from careless_amd.models.likelihoods.mono import LocationScaleLikelihood
        from careless_amd.models.priors.wilson import DoubleWilsonPrior
        from careless_amd.models.scaling.image import HybridImageScaler, NeuralImageScaler
        from careless_amd.models.scaling.nn import MetadataScaler

        q, prior, lik, scaler = model.surrogate_posterior, model.prior, model.likelihood, model.scaling_model
        # the Rice-Woolfson posterior (cl_rw_forward / cl_rw_backward in place of cl_tn_*): nothing behind z_f / dz_f knows which one sampled
        self.rw = posterior_kind(q) == "rice_woolfson"
        self.ref_prior = prior_kind(prior) == _lib.CL_PRIOR_REFERENCE
        from careless_amd.models.likelihoods.laue import LaueBase
        self.laue = BaseModel.is_laue(inputs)
        self.neural = check_neural_likelihood(lik, self.laue, lib=self.lib)
        if self.laue != isinstance(lik, LaueBase):
            raise ValueError("Laue inputs (8-tuple with harmonic_id) need a careless_amd.models.likelihoods.laue likelihood, "
                             "monochromatic inputs a careless_amd.models.likelihoods.mono one")
        if not isinstance(lik, (LocationScaleLikelihood, LaueBase)) or lik.kind not in ("normal", "studentt", "laplace"):
            raise NotImplementedError(f"likelihood {type(lik).__name__} is not supported by the HIP engine yet")
        if lik.kind == "laplace" and getattr(lik, "ev11", False):
            raise NotImplementedError(f"likelihood {type(lik).__name__}: the Evans-2011 error model has no Laplace form (the reference has no such class)")
        imgl = None
        if isinstance(scaler, HybridImageScaler):
            mlp, img = scaler.mlp_scaler, scaler.image_scaler
        elif isinstance(scaler, NeuralImageScaler):
            mlp, img, imgl = scaler.metadata_scaler, None, scaler
        elif isinstance(scaler, MetadataScaler):
            mlp, img = scaler, None
        else:
            raise NotImplementedError(f"scaling model {type(scaler).__name__} is not supported by the HIP engine yet")
        if model.scale_prior is not None:
            raise NotImplementedError("scale_prior is never enabled by the reference CLI and is not supported")
        self.q, self.prior, self.lik, self.mlp, self.img, self.imgl = q, prior, lik, mlp, img, imgl
        self.R = int(q.loc_raw.numel())
        self.N_total = int(_np(BaseModel.get_refl_id(inputs)).reshape(-1).shape[0])
        self.d = int(_np(BaseModel.get_metadata(inputs)).reshape(self.N_total, -1).shape[1])
        self.S = int(model.mc_sample_size)
        if self.S < 1:
            raise ValueError("mc_sample_size must be >= 1")
        self.ev11 = bool(getattr(lik, "ev11", False))
        self.double_wilson = isinstance(prior, DoubleWilsonPrior)
        self.dw_trainable = self.double_wilson and prior.r_raw is not None
        # Deterministic mode (`model.deterministic = True` or CARELESS_HIP_DETERMINISTIC=1): no float atomics anywhere in the step --
        # per-observation stores + fixed-order sums (cl_det_reduce) -- so two runs give bit-identical gradients and parameters
        self.deterministic = switch(model, "deterministic", "CARELESS_HIP_DETERMINISTIC", env_adds=True)

    def _reflection_constants(self):
        """Per-reflection constants of the posterior and the prior, uploaded once."""
        q, prior, dev = self.q, self.prior, self.device
        self.low = q.low.to(dev, torch.float32).contiguous()
        self.q_centric = None
        if self.rw:                      # the posterior's own family flag (the prior's `centric` is NULL under a reference prior)
            if q.centric.size != self.R:
                raise ValueError("RiceWoolfson.centric does not match the number of reflections")
            self.q_centric = torch.as_tensor(q.centric.astype(np.uint8), device=dev)
        if self.ref_prior:
            # an empirical reference prior (models/priors/empirical.py): its arrays expanded to all reflections, uploaded once; the Wilson
            # arrays stay NULL (`_tn_args`) -- cl_ref_prior evaluates the density in front of the step's cl_tn_backward
            self.centric = self.es = None
            up = lambda a: None if a is None else torch.as_tensor(a, device=dev)
            self.ref = {k: (up(v) if isinstance(v, np.ndarray) else v) for k, v in reference_prior_arrays(prior, self.R).items()}
        else:
            self.centric = torch.as_tensor(prior.centric.astype(np.uint8), device=dev)
            self.es = torch.as_tensor(prior.eps_sigma, device=dev)
            if self.centric.numel() != self.R or self.es.numel() != self.R:
                raise ValueError("prior and surrogate posterior disagree on the number of reflections")
        if self.double_wilson:
            if prior.reflids.size != self.R or (prior.reflids >= self.R).any():
                raise ValueError("DoubleWilsonPrior.reflids does not match the surrogate posterior")
            self.parent_ids = torch.as_tensor(prior.reflids.astype(np.int32), device=dev)
            self.root = torch.as_tensor(prior.root.astype(np.uint8), device=dev)
            self.dw_r = torch.as_tensor(prior.r_per_reflection, device=dev)
            self.dw_children = None         # deterministic mode: the children of every reflection as a CSR list
            if self.deterministic:
                # parents pull their children's terms in list order instead of children scattering with atomics (cl_dw_prior_forward)
                par = np.asarray(prior.reflids).astype(np.int64)
                kids = np.nonzero(par >= 0)[0]
                kids = kids[np.argsort(par[kids], kind="stable")]
                seg = np.concatenate([[0], np.cumsum(np.bincount(par[kids], minlength=self.R))]).astype(np.int32)
                self.dw_children = (torch.as_tensor(seg, device=dev), torch.as_tensor(kids.astype(np.int32) if len(kids) else np.zeros(1, np.int32), device=dev))
            if self.dw_trainable:
                self.asu_ids = torch.as_tensor(prior.asu_ids.astype(np.int32), device=dev)

    def _plan(self, inputs) -> bool:
        """`self.plan`: how the scaler runs (`plan_scaler`), under its old names too; the answer: the model asks for the two-pass Laue path."""
        mlp, imgl = self.mlp, self.imgl
        mlp.build(self.d)
        self.w, self.L = mlp.width, mlp.n_layers
        two_pass = self.laue and bool(getattr(self.model, "laue_two_pass", False))
        gmax = int(np.bincount(_np(BaseModel.get_harmonic_id(inputs)).reshape(-1).astype(np.int64)).max()) if self.laue else 1
        self.plan = plan_scaler(self.lib, self.d, self.w, self.L, imgl.n_image_layers if imgl is not None else 0, laue=self.laue,
                                two_pass=two_pass, gmax=gmax, ev11=self.ev11, deterministic=self.deterministic,
                                lik_kind=_lib.CL_LIK_LAPLACE if self.lik.kind == "laplace" else 0)
        self.wide, self.peel, self.blocks, self.chain_lane = self.plan.wide, self.plan.peel, self.plan.blocks, self.plan.chain_lane
        if imgl is not None:
            imgl.build(self.d)
        return two_pass

    def _bind_parameters(self):
        """The flat parameter vector and Adam's moments; the plugin objects become views into the parameters (`bind_flat`)."""
        mlp, img, imgl, dev = self.mlp, self.img, self.imgl, self.device
        if self.neural:
            self.lik.build()
        self.layout = lay = make_layout(self.R, self.d, self.w, self.L, img.max_images - 1 if img is not None else 0, 3 if self.ev11 else 0,
                                        int(self.prior.r_raw.numel()) if self.dw_trainable else 0,
                                        imgl=(imgl.n_image_layers, imgl.max_images) if imgl is not None else None,
                                        lik_dense=self.lik.layer_slices() if self.neural else None)
        assert not self.neural or lay.n_ev11 == self.lik.param_count() == int(self.lib.cl_nlik_param_count(self.lik.n_layers, self.lik.width))
        assert lay.P == mlp.param_count(self.d) == int(self.lib.cl_mlp_param_count(self.d, self.w, self.L))
        self.params = torch.empty(lay.n, dtype=torch.float32, device=dev)
        bind_flat(self.params, lay, self.q, mlp, img, imgl, self.lik, self.prior)
        self.q.low = self.low
        self.adam_m = torch.zeros_like(self.params)
        self.adam_v = torch.zeros_like(self.params)
        self.t = 0                                  # optimizer iterations
        self.seg_off = torch.as_tensor(np.asarray(lay.seg_off, dtype=np.int32), device=dev)
        self.nseg = len(lay.seg_off) - 1

    def _decide_shard(self, inputs, shard: Optional[Shard]):
        """`self.shard`: the one given, else all rows -- or, asked for, this rank's reflections and their rows; `self.laue_groups`."""
        self.shard = shard if shard is not None else make_shard(self.N_total, self.R)
        self.laue_groups = None
        if self.laue and self.shard.world > 1:
            self.laue_groups = laue_group_shard(_np(BaseModel.get_harmonic_id(inputs)).reshape(-1), self.shard.rank, self.shard.world)
        # Reflection-owner sharding: with more than one rank, monochromatic data and the Wilson prior, a rank takes a
        # RANGE OF REFLECTIONS and every observation of theirs instead of a range of rows.  Sampling q(F), its KL, its gradient and
        # its Adam update are then local to the owner (1 / world of the replicated work of the row split), and the step's all-reduce
        # carries the scaler's gradient and four norm terms instead of 2 R floats.  Laue data (a harmonic group mixes reflections),
        # the double-Wilson prior (a child's parent may live on another rank), per-image layers, wide scalers and the deterministic
        # mode keep the row split.  OPT-IN (`model.owner_shard = True` or CARELESS_HIP_OWNER_SHARD=1) since round 5: the split has been
        # verified on one device and over gloo (parity suite, shard-sum tests) but has never met RCCL on a multi-GPU node, and on one
        # device its compute side is worth <= 1 % at eight ranks; the row split stays the default until
        # `scripts/scale_curve.sh` has measured both on a node.
        if wants_owner_shard(switch(self.model, "owner_shard", "CARELESS_HIP_OWNER_SHARD"), self.prior, self.shard.world, bool(self.shard.owner),
                             self.laue, self.double_wilson, self.wide, self.imgl is not None, self.deterministic):
            osh = owner_shard(_np(BaseModel.get_refl_id(inputs)).reshape(-1), self.R, self.shard.rank, self.shard.world)
            if osh is not None:
                self.shard = osh
        self.owner = bool(self.shard.owner)

    def _build_workspace(self):
        """The step workspace (`carve_workspace`) and the small per-step buffers beside it."""
        dev, RS = self.device, self.R * self.S
        carve = carve_workspace(self.R, self.S, self.layout.n, self.nseg, self.owner)
        self.ws = torch.zeros(carve.total, dtype=torch.float32, device=dev)
        assert carve.aligned and self.ws.data_ptr() % 16 == 0
        part = lambda region: self.ws[region[0]:region[0] + region[1]]
        self.dz_f, self.grads = part(carve.dz_f), part(carve.grads)
        self.scalars, self.seg_sq, self.own_scratch = (part(r).view(torch.float64) for r in (carve.scalars, carve.seg_sq, carve.own_scratch))
        self.msg_norm = part(carve.msg_norm)         # [raw, sanitised, sanitised a, sanitised b]
        self.msg = part(carve.msg)                   # what an owner-mode step all-reduces
        self.ws_step = part(carve.ws_step)           # owner mode zeroes this (16-byte aligned) and its own slice of dz_f per step
        self.norm_part = torch.zeros(2 * 1024, dtype=torch.float64, device=dev)                  # per-workgroup norm sums of cl_adam_step (<= 1024 workgroups)
        self.kl_part = torch.zeros((self.R + 255) // 256, dtype=torch.float64, device=dev)      # per-workgroup KL sums of cl_tn_forward
        self.kl_part_dw = torch.zeros_like(self.kl_part) if (self.double_wilson or self.ref_prior) else None    # ... and of cl_dw_prior_forward / cl_ref_prior
        self.z_f = torch.empty(RS, dtype=torch.float32, device=dev)
        self.stop_flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.frozen = torch.zeros(self.nseg, dtype=torch.uint8, device=dev)
        self.history_buf: Optional[torch.Tensor] = None
        self._keep = None

    def _build_obs(self, inputs, start, stop, grid, laue_groups, rows=None):
        """Device image of rows [start, stop) of `inputs`: one `ObsData`, or -- plain layout only -- as many pieces as the 4-GiB
        bound of a launch asks for (`ObsChunks`)."""
        kw = dict(grid=grid, n_refl=self.R, n_images=self._max_images(), laue_groups=laue_groups, pack_images=self.imgl is not None and not self.wide,
                  sort_images=self.imgl is not None and self.wide,
                  laue_single_pass=not getattr(self.model, "laue_two_pass", False) and self.blocks is None and not self.wide, wide=self.wide)
        kw.update((self._frozen_layout and self._frozen_layout_kw()) or {})
        n_total = int(_np(BaseModel.get_refl_id(inputs)).reshape(-1).shape[0])
        stop = n_total if stop is None else stop
        per = launch_row_limit(self.d, self.S if self.deterministic else 0)
        if rows is not None:
            start, stop = 0, len(rows)
        whole = self.laue or self.imgl is not None or self.wide or stop - start <= per
        bounds = [(start, stop)] if whole else [(a, min(stop, a + per)) for a in range(start, stop, per)]
        pieces = []
        for a, b in bounds:
            pieces.append(ObsData(self.lib, inputs, a, b, self.S, self.layout.P, self.device, rows=None if rows is None else rows[a:b], host_inputs=inputs, **kw))
            kw["n_refl"] = kw["n_images"] = None          # (the id ranges were checked over the whole input by the first piece)
            pieces[-1].partials = pieces[0].partials      # launches are serialised on one stream: one partial buffer
        o = pieces[0]
        if len(pieces) > 1:
            o = ObsChunks(pieces)
            if rows is not None:
                o.rows = np.asarray(rows, dtype=np.int64)
        if self.deterministic:
            self._det_attach(o, pieces)
        if self.neural:
            self._nlik_attach(o, pieces, inputs)
        if self.blocks is not None:
            o.alloc_chain(self.lib, self.blocks, self.w, self.device, self.chain_lane)
        return o

    def _det_attach(self, obs, pieces):
        """Buffers of the deterministic mode for one observation set: the per-observation stores of the fused kernel and the sort
        orders (by reflection, by image; stable, so sums run in row order) that `cl_det_reduce` walks."""
        dev = self.device
        if pieces[0].row_map is not None:
            # packed layout (single-pass Laue; per-image layers, round 6): the kernels store by the caller's local row (row_map), so the ids go back to that order
            p0 = pieces[0]
            if self.laue and not p0.fused_laue:
                raise NotImplementedError("deterministic mode: harmonic groups of more than 16 rows take the two-pass Laue path, which keeps its float atomics")
            rm = p0.row_map.cpu().numpy()
            ok = rm >= 0
            rid, img = np.zeros(p0.N, dtype=np.int64), np.zeros(p0.N, dtype=np.int64)
            rid[rm[ok]] = p0.refl_id.cpu().numpy()[ok]
            img[rm[ok]] = p0.image_id.cpu().numpy()[ok]
        else:
            rid = torch.cat([p.refl_id[: p.N] for p in pieces]).cpu().numpy()
            img = torch.cat([p.image_id[: p.N] for p in pieces]).cpu().numpy()
        n = len(rid)

        def order(ids, nbins):
            perm = np.argsort(ids, kind="stable").astype(np.int32)
            seg = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=nbins))]).astype(np.int32)
            return torch.as_tensor(perm, device=dev), torch.as_tensor(seg, device=dev)
        M = self._max_images() or 1
        # slot[i] = position of observation i in the reflection-sorted order: the kernels store its record THERE (cl_mlp_args.det_slot),
        # so that the per-reflection sums read contiguous records instead of gathering ~30 random ones each
        perm_r, seg_r = order(rid, self.R)
        slot = None
        if 4 * n * self.S < (1 << 32):          # (the kernels address a record with a 32-bit byte offset from the buffer's start)
            slot = torch.empty(n, dtype=torch.int32, device=dev)
            slot[perm_r.long()] = torch.arange(n, dtype=torch.int32, device=dev)
        obs.det = DetBuffers(slot=slot, dzf=torch.zeros(n * self.S, dtype=torch.float32, device=dev), dimg=torch.zeros(n, dtype=torch.float32, device=dev),
                             nll=torch.zeros(len(pieces) * pieces[0].grid + (_lib.CL_LAUE_LIK_MAX_BLOCKS if (self.laue or self.wide) else 0),
                                             dtype=torch.float64, device=dev),
                             refl=(perm_r, seg_r), img=order(img, M), M=M, pieces=len(pieces), grid=pieces[0].grid)
        if self.ev11:
            # Evans-2011 gradients: one slot of three floats per wave of every launch (the fused launches' CL_EV11_WAVES per workgroup, then
            # four per workgroup of the slot / padded-slot likelihood launch), summed in slot order by cl_det_reduce
            obs.det.ev11 = torch.zeros(3 * (_lib.CL_EV11_WAVES * len(pieces) * pieces[0].grid + 4 * _lib.CL_LAUE_LIK_MAX_BLOCKS), dtype=torch.float32, device=dev)
        for k, p in enumerate(pieces):
            p.det_parent, p.det_index = obs, k

    # -- neural likelihood (csrc/elbo_nlik.hip) ------------------------------------------------------------------
    def _nlik_attach(self, obs, pieces, inputs):
        """Buffers of the neural likelihood for one observation set: Iobs / SigIobs of all its rows in the order the set's eta and ipred_out
        are in -- the caller's rows, whatever order a packed layout stores them in; the image order of the wide path's sorted layout, whose
        eta / ipred_out follow `obs.rows` (`_noise_to_device`, `VariationalMergingModel.call`) --, sigpred and the kernels' workspace."""
        dev, lik = self.device, self.lik
        rows = np.concatenate([np.asarray(p.rows, dtype=np.int64) if p.rows is not None else np.arange(p.start, p.start + p.N, dtype=np.int64)
                               for p in pieces])
        col = lambda a: torch.as_tensor(np.ascontiguousarray(_np(a).reshape(-1)[rows].astype(np.float32)), device=dev)
        n = int(len(rows))
        nbytes = int(self.lib.cl_nlik_workspace_bytes(n, lik.n_layers, lik.width))
        sigpred = torch.ones(n + TILE, dtype=torch.float32, device=dev)
        obs.nlik = NlikBuffers(n, col(BaseModel.get_intensities(inputs)), col(BaseModel.get_uncertainties(inputs)), sigpred,
                               torch.zeros((nbytes + 3) // 4, dtype=torch.float32, device=dev))
        assert obs.nlik.ws.data_ptr() % 16 == 0
        for p in pieces:
            p.sig_now = None                # this step's sigpred in the order the piece's launches read sig (`_nlik_image`, `_sig`)

    def _nlik_image(self, obs, pieces, forms):
        """`nlik.image` / `nlik.pos` of the set for the forms its pieces' data terms take now, and every piece's `sig_now`: the sig-shaped
        array in the order its launch reads.  The pos map of a piece: none where sig is stored in the order of ipred_out (the plain layout;
        the wide path's image-sorted one, whose ipred_out is in that order too), the inverse of `row_map` (packed by image) or of a frozen
        scaler's sort by reflection (`SortedRows.key` - start)."""
        from careless_amd.frozen import FrozenForm
        nb = obs.nlik
        key = tuple(("sorted", self._frozen_epoch) if f is FrozenForm.SORTED_ROWS else "layout" for f in forms)
        if nb.image_key == key:
            return
        dev, owns, poss = self.device, [], []
        for p, f in zip(pieces, forms):
            pos = None
            if f is FrozenForm.SORTED_ROWS:
                fz = self._sorted_rows(p)
                own, src, dst = fz.sig, fz.key.long() - int(p.start), None
            elif p.row_map is not None:
                own, dst = p.sig, torch.nonzero(p.row_map >= 0).flatten()
                src = p.row_map.long().index_select(0, dst)
            else:
                own, src = p.sig, None
            if src is not None:
                pos = torch.empty(p.N, dtype=torch.int64, device=dev)
                pos[src] = torch.arange(p.N, dtype=torch.int64, device=dev) if dst is None else dst
                assert int(src.numel()) == p.N and int(pos.min()) >= 0 and int(pos.max()) < int(own.numel())
            owns.append(own); poss.append(pos)
        if all(q is None for q in poss):
            nb.image = nb.pos = None
            for p in pieces:
                p.sig_now = nb.sigpred[p.row0:]                     # (a piece's padding rows: the next piece's rows, or the tail of ones)
        else:
            offs = list(accumulate([int(o.numel()) for o in owns], initial=0))
            nb.image = torch.cat([o.clone() for o in owns])         # padding positions keep the layout's own 1.0
            nb.pos = torch.cat([(torch.arange(p.N, dtype=torch.int64, device=dev) if q is None else q) + off
                                for p, q, off in zip(pieces, poss, offs)]).to(torch.int32).contiguous()
            for p, a, b in zip(pieces, offs, offs[1:]):
                p.sig_now = nb.image[a:b]
        nb.image_key = key

    def _nlik_args(self, obs) -> NlikArgs:
        nb, lik = obs.nlik, self.lik
        a = NlikArgs()
        a.iobs, a.sigiobs, a.net = ptr(nb.iobs), ptr(nb.sigiobs), self._param_ptr("ev11")
        a.L, a.w, a.leak, a.n = lik.n_layers, lik.width, lik.leakiness, nb.n
        a.sigpred, a.pos, a.sig_image, a.workspace = ptr(nb.sigpred), ptr(nb.pos), ptr(nb.image), ptr(nb.ws)
        a.stop_flag = ptr(self.stop_flag)
        return a

    def _nlik_forward(self, obs, injected: bool, st):
        """sigpred of all rows of the set -- the mean of delta is over the whole set, also when it is cut into pieces -- in the caller's order
        and in the order every piece's data term reads (`_sig`)."""
        pieces = obs.children if isinstance(obs, ObsChunks) else [obs]
        self._nlik_image(obs, pieces, [self._frozen_form(p, injected=injected) for p in pieces])
        check(self.lib.cl_nlik_forward(C.byref(self._nlik_args(obs)), st), "cl_nlik_forward")

    def _nlik_backward(self, obs, ipred_out, st):
        """The network's gradient from the step's predictions (`ipred_out`, [n][S] in the caller's order) into the likelihood's slice of
        the flat gradient."""
        a = self._nlik_args(obs)
        a.ipred, a.S, a.w_ll, a.d_net = ptr(ipred_out), self.S, self._w_ll(obs), self._grad_ptr("ev11")
        check(self.lib.cl_nlik_backward(C.byref(a), st), "cl_nlik_backward")

    def _nlik_ipred(self, obs) -> torch.Tensor:
        nb = obs.nlik
        if nb.ipred is None:
            nb.ipred = torch.empty(nb.n * self.S, dtype=torch.float32, device=self.device)
        return nb.ipred

    def _sig(self, obs: ObsData, own: torch.Tensor) -> torch.Tensor:
        """THE hand-over of the likelihood's sigma to a data-term launch (`_mlp_args`, `_slot_args`, `_frozen_rows`): `own`, the observation
        image's SigIobs in the order the launch reads -- or, under a neural likelihood, this step's sigpred in the same order
        (`_nlik_forward` set `obs.sig_now`; before the first step -- a routing question -- there is none and the pointer is not read)."""
        if not self.neural or getattr(obs, "sig_now", None) is None:
            return own
        assert obs.sig_now.numel() >= own.numel()
        return obs.sig_now

    def _max_images(self):
        if self.img is not None:
            return self.img.max_images
        return self.imgl.max_images if self.imgl is not None else None

    def _param_ptr(self, group: str, el: int = 0) -> int:       # device address of element `el` of a group (`FlatLayout.groups`) of the parameters
        return self.params.data_ptr() + 4 * (self.layout.off(group) + el)

    def _grad_ptr(self, group: str, el: int = 0) -> int:        # ... of the flat gradient
        return self.grads.data_ptr() + 4 * (self.layout.off(group) + el)

    # the training shard's sizes under their old names (bench.py, tests, scripts/stamps*.py)
    N = property(lambda self: self.obs.N)
    n_pad = property(lambda self: self.obs.n_pad)
    grid = property(lambda self: self.obs.grid)

    # ------------------------------------------------------------------------------------------------------
    def refresh_config(self):
        """(Re)read the knobs that may change between train_model calls: trainable flags, kl weight, optimizer."""
        m = self.model
        fr = np.zeros(self.nseg, dtype=np.uint8)
        for k, owner in enumerate(self.layout.seg_owner):
            if owner == "q" and not self.q.trainable:
                fr[k] = 1
            if owner == "scaler" and not m.scaling_model.trainable:
                fr[k] = 1
            if owner == "likelihood" and not getattr(self.lik, "trainable", True):
                fr[k] = 1
        self.any_frozen = bool(fr.any())
        self.frozen.copy_(torch.as_tensor(fr))
        self.scaler_frozen = not m.scaling_model.trainable
        self._frozen_epoch += 1                          # (loc, sigma) of a frozen scaler are taken again at every train_model call
        if self._frozen_layout and self._frozen_layout_kw() is None:
            # the scaler was frozen when the engine laid its observations out and is trainable now: the fused kernels' layouts again
            self._frozen_layout = False
            first = self.obs.children[0] if isinstance(self.obs, ObsChunks) else self.obs
            self.obs = self._build_obs(first.host_inputs, self.shard.start, self.shard.stop, self._grid_arg, self.laue_groups,
                                       rows=self.shard.rows if self.owner else None)
        opt = m.optimizer
        self.opt = opt
        S, N, R = self.S, self.N_total, self.R
        if m.kl_weight is None:                         # variational.py:172-174
            self.w_ll, self.w_kl, self.kl_mult = 1.0 / S, 1.0 / S, 1.0
        else:                                           # variational.py:175-177
            self.w_ll, self.w_kl, self.kl_mult = 1.0 / (S * N), 1.0 / (S * R), float(m.kl_weight)
        if self.lik.kind == "studentt":
            nu = float(self.lik.dof)
            self.lik_kind, self.dof = _lib.CL_LIK_STUDENTT, nu
            self.lik_const = math.lgamma(0.5 * (nu + 1.0)) - math.lgamma(0.5 * nu) - 0.5 * math.log(nu * math.pi)
        elif self.lik.kind == "laplace":                # (neither dof nor lik_const is read)
            self.lik_kind, self.dof, self.lik_const = _lib.CL_LIK_LAPLACE, 0.0, 0.0
        else:
            self.lik_kind, self.dof, self.lik_const = _lib.CL_LIK_NORMAL, 0.0, 0.0
        self.bij_kind = BIJ_KINDS[self.mlp.scale_bijector]

    # ------------------------------------------------------------------------------------------------------
    def _tn_args(self, step: int, u_f) -> TnArgs:
        a = TnArgs()
        a.q_loc_raw, a.q_scale_raw = self._param_ptr("q_loc"), self._param_ptr("q_scale")
        a.low = ptr(self.low); a.centric = ptr(self.centric); a.es = ptr(self.es)
        a.R, a.S = self.R, self.S
        a.high, a.eps = self.q.high, self.q.scale_shift
        a.w_kl, a.kl_grad_mult = self.w_kl, self.kl_mult
        a.kl_begin, a.kl_end = self.shard.kl_begin, self.shard.kl_end
        if self.owner:
            a.r_begin, a.r_end = self.shard.kl_begin, self.shard.kl_end      # the reflections this rank owns: nobody else touches them
        a.u_f = ptr(u_f)
        a.seed, a.step = self.seed, step & 0xFFFFFFFF
        a.z_f = ptr(self.z_f); a.dz_f = ptr(self.dz_f)
        a.d_loc_raw, a.d_scale_raw = self._grad_ptr("q_loc"), self._grad_ptr("q_scale")
        a.scalars = ptr(self.scalars)
        a.stop_flag = ptr(self.stop_flag)
        if self.ref_prior:
            a.prior_kind = _lib.CL_PRIOR_REFERENCE               # (no Wilson term in cl_tn_forward / _backward: centric and es stay NULL)
        if self.double_wilson:
            a.prior_kind = _lib.CL_PRIOR_DOUBLE_WILSON
            a.parent_ids, a.root, a.dw_r = ptr(self.parent_ids), ptr(self.root), ptr(self.dw_r)
            a.dz_f_out = ptr(self.dz_f)
            if self.dw_children is not None:
                a.dw_child_seg, a.dw_child_ids = ptr(self.dw_children[0]), ptr(self.dw_children[1])
            if self.dw_trainable:
                a.dw_r_raw, a.d_dw_r_raw = self._param_ptr("dwr"), self._grad_ptr("dwr")
                a.asu_ids, a.n_asu = ptr(self.asu_ids), self.layout.n_dwr
        return a

    def _q_launch(self, which: str, tn: TnArgs, st):
        """`cl_tn_<which>` -- or, under the Rice-Woolfson posterior, `cl_rw_<which>` on the same argument fill (u_f: the injected normals)."""
        if not self.rw:
            check(getattr(self.lib, "cl_tn_" + which)(C.byref(tn), st), "cl_tn_" + which)
            return
        a = RwArgs()
        a.tn = tn
        a.q_centric, a.n_f = ptr(self.q_centric), tn.u_f
        a.tn.u_f = None
        check(getattr(self.lib, "cl_rw_" + which)(C.byref(a), st), "cl_rw_" + which)

    def _step_fields(self, a, obs: ObsData, step: int):
        """The per-step constants `cl_mlp_args`, `cl_laue_args` and `cl_frozen_args` name alike, on whichever of the three `a` is."""
        a.R, a.S = self.R, self.S
        a.z_f, a.dz_f = ptr(self.z_f), ptr(self.dz_f)
        a.lik_kind, a.dof, a.lik_const = self.lik_kind, self.dof, self.lik_const
        a.shift = self.mlp.scale_multiplier or 0.0
        a.w_ll = self._w_ll(obs)
        a.seed, a.step = self.seed, step & 0xFFFFFFFF
        a.scalars, a.stop_flag = ptr(self.scalars), ptr(self.stop_flag)
        if self.ev11:
            a.ev11, a.d_ev11 = self._param_ptr("ev11"), self._grad_ptr("ev11")
        return a

    def _shard_rows(self, obs: ObsData, t) -> Optional[int]:
        """Pointer to the rows of `obs` inside a per-(row, sample) array of its whole shard (eta, ipred_out): a piece of a chunked shard starts at row0."""
        return None if t is None else t.data_ptr() + 4 * self.S * obs.row0

    def _det_parts(self, obs: ObsData, k: int):
        """(nll_part, ev11_part) of part k of the shard `obs` belongs to (deterministic mode): the fused launches of its pieces store into parts
        0 .. pieces - 1 -- det.grid NLL slots, CL_EV11_WAVES Evans-2011 slots of three floats per workgroup --, the slot / padded-slot
        likelihood launch behind them (k = det.pieces)."""
        det = obs.det_parent.det
        return (det.nll.data_ptr() + 8 * det.grid * k,
                det.ev11.data_ptr() + 4 * 3 * _lib.CL_EV11_WAVES * det.grid * k if self.ev11 else None)

    def _mlp_args(self, step: int, eta, ipred_out=None, obs: Optional[ObsData] = None) -> MlpArgs:
        lay = self.layout
        obs = self.obs if obs is None else obs
        a = self._step_fields(MlpArgs(), obs, step)
        a.refl_id = ptr(obs.refl_id); a.image_id = ptr(obs.image_id); a.meta_t = ptr(obs.meta_t)
        a.iobs = ptr(obs.iobs); a.sig = ptr(self._sig(obs, obs.sig))
        a.n_obs, a.n_pad = obs.N, obs.n_pad
        a.obs_offset = obs.start
        if obs.fused_laue:
            a.gmeta, a.tile_gmax = ptr(obs.gmeta), ptr(obs.tile_gmax)
        a.noise_row = ptr(obs.noise_row)
        scaler_fields(a, self.mlp, self.d, self._param_ptr("mlp"), self.imgl, self._param_ptr("imgl"), obs.tile_img, obs.row_map)
        if self.imgl is not None:
            a.d_imgl = self._grad_ptr("imgl")
        a.use_img = 1 if lay.n_img > 0 else 0
        a.img = self._param_ptr("img") if lay.n_img > 0 else None
        a.eta, a.ipred_out = self._shard_rows(obs, eta), self._shard_rows(obs, ipred_out)
        a.d_img = self._grad_ptr("img") if lay.n_img > 0 else None
        a.partials = ptr(obs.partials)
        if self.deterministic:
            det = obs.det_parent.det
            if det.slot is not None:
                a.dzf_obs = det.dzf.data_ptr()                  # (records by slot: positions inside the whole shard, not the piece)
                a.det_slot = det.slot.data_ptr() + 4 * obs.row0
            else:
                a.dzf_obs = det.dzf.data_ptr() + 4 * self.S * obs.row0
            a.dimg_obs = det.dimg.data_ptr() + 4 * obs.row0
            a.nll_part, a.ev11_part = self._det_parts(obs, obs.det_index)
        return a

    def _likelihood_args(self, ma: MlpArgs, obs: ObsData, mode: int = 0):
        """From `_mlp_args` of `obs`: (arguments, mode) of the scaler launch that computes the likelihood -- the launch `plan.route` is the
        route of: the last block of a chain with its dZ_0 (lane kernel) or dX out, the backward launch of the two-pass Laue path (mode 2,
        dL/d(loc, sigma) in), the launch behind a peeled first layer, else the fused launch on the scaler itself.  The data term launches
        with it, `training_launch` asks about it."""
        if self.blocks is not None:
            K = len(self.blocks)
            ma = self._block_args(ma, obs, K - 1)
            if self.chain_lane:
                ma.dZ0_out = ptr(obs.chain_dz0)       # dZ_0 of the block's first layer; `cl_chain_dx` turns it into the gradient of the block's input
            else:
                ma.dX_out = ptr(obs.chain_dact[K - 2])
        elif self.laue and not obs.fused_laue:
            mode = 2 if mode == 0 else mode
            ma.dO_ext = ptr(obs.laue_dO)
        elif self.peel and mode == 0:
            ma = self._peel_args(ma, obs)
        return ma, mode

    def kernel_name(self, mode: int = 0) -> str:
        """Name of the kernel instance the scaler launches of this engine run (`cl_mlp_kernel_name`: the library's own routing):
        what a rocprofv3 kernel trace lists for the dominant kernel."""
        if self.wide:
            sq = 65 <= self.w <= 128 and self.d <= 128          # (square layers of the streaming kernel's widths: cl_wide_head_bwd_supported's range)
            return (("wide_sq_kernel + wide_gemm_kernel" if sq else "wide_gemm_kernel (+ wide_stream_kernel)") +
                    (" (slot likelihood: deterministic stores)" if self.deterministic else ""))
        ma, mode = self.training_launch(mode)
        buf = C.create_string_buffer(128)
        check(min(0, self.lib.cl_mlp_kernel_name(C.byref(ma), mode, buf, 128)), "cl_mlp_kernel_name")
        return buf.value.decode()

    def training_launch(self, mode: int = 0):         # (arguments, mode) of the launch kernel_name names; plan.route is its cl_mlp_route
        obs = self.obs.children[0] if isinstance(self.obs, ObsChunks) else self.obs
        return self._likelihood_args(self._mlp_args(0, None, None, obs), obs, mode)

    def _w_ll(self, obs: ObsData) -> float:
        """Weight of one log-likelihood term: sum / S, or with `kl_weight` the mean over the S x N terms of the observation set
        the model is called on (reference variational.py:172-177) -- the validation set's own N for `NLL_val` (:257-260)."""
        return 1.0 / self.S if self.model.kl_weight is None else 1.0 / (self.S * obs.N_total)

    def _noise_to_device(self, u_f, eta, obs: Optional[ObsData] = None):
        """Injected noise arrives in the reference's (S, R) / (S, N_total) orientation; device layout is [R][S] / [N][S].  Under the
        Rice-Woolfson posterior `u_f` carries the standard normals n1, n2 as (2, S, R); device layout [2][R][S]."""
        obs = self.obs if obs is None else obs
        du = de = None
        if u_f is not None and self.rw:
            u = torch.as_tensor(_np(u_f), dtype=torch.float32).reshape(2, self.S, self.R)
            du = u.permute(0, 2, 1).contiguous().to(self.device)
        elif u_f is not None:
            u = torch.as_tensor(_np(u_f), dtype=torch.float32).reshape(self.S, self.R)
            du = u.t().contiguous().to(self.device)
        if eta is not None:
            e = torch.as_tensor(_np(eta), dtype=torch.float32).reshape(self.S, obs.N_total)
            if obs.rows is not None:
                de = e[:, torch.as_tensor(obs.rows)].t().contiguous().to(self.device)
            else:
                de = e[:, obs.start:obs.start + obs.N].t().contiguous().to(self.device)
        return du, de

    # ------------------------------------------------------------------------------------------------------
    def forward_backward(self, step: int, u_f=None, eta=None, ipred_out=None):
        """Enqueue the loss + gradient part of a step (everything up to, not including, the optimizer)."""
        lib, st = self.lib, _stream()
        tn = self._tn_args(step, u_f)
        tn.kl_part = ptr(self.kl_part)       # the forward launch stores its workgroups' KL sums, the backward launch of this step adds them up
        if self.double_wilson or self.ref_prior:
            tn.kl_part_dw = ptr(self.kl_part_dw)
        # the step's accumulators are cleared by the forward launch itself (no memset launch in front of it): the flat gradient and
        # the scalars by all its threads, the dz_f rows of the reflections it samples by their threads
        n_own = (self.shard.kl_end - self.shard.kl_begin) if self.owner else self.R
        if self.ws_step.numel() <= max(1 << 20, 64 * n_own * self.S):
            tn.zero_ptr, tn.zero_n, tn.zero_dzf = self.ws_step.data_ptr(), int(self.ws_step.numel()), ptr(self.dz_f)
        else:                                # (per-image layers over many images: a gradient vector far longer than the launch: memset)
            self._zero_step()
        self._q_launch("forward", tn, st)
        if self.double_wilson:
            check(lib.cl_dw_prior_forward(C.byref(tn), st), "cl_dw_prior_forward")
        self._pending_reduce = None
        dist_on = (self.shard.world > 1 and not self.local_only) or self.force_allreduce
        # Row split, two-piece message (`model.split_message = True` / CARELESS_HIP_SPLIT_MESSAGE=1; measured in DESIGN 5.2): everything
        # behind a and b in the flat gradient -- the scaler's, the image scales', Ev11's part -- is final once the fused kernel and the
        # partial reduction are through, so its all-reduce starts then (asynchronously, on the communicator's stream) and runs beside
        # cl_tn_backward; a's and b's gradient follows when that kernel is done.  (Not with a trainable double-Wilson r: its gradient
        # sits in the tail and comes out of cl_tn_backward.)
        split = dist_on and not self.owner and not self.dw_trainable and switch(self.model, "split_message", "CARELESS_HIP_SPLIT_MESSAGE")
        self._data_term(self.obs, step, eta, ipred_out, st, defer_reduce=not split, train=True)
        tail_work = None
        if split:
            import torch.distributed as dist
            tail_work = dist.all_reduce(self.grads[2 * self.R:], op=dist.ReduceOp.SUM, group=self.process_group, async_op=True)
        if self._pending_reduce is not None:
            # ... and the reduction of the fused kernel's per-workgroup scaler-gradient partials rides in extra workgroups of the
            # backward launch (independent work: one launch instead of two)
            tn.red_partials, tn.red_nparts, tn.red_P, tn.red_out = self._pending_reduce
            self._pending_reduce = None
        if self.ref_prior:
            # behind EVERY data-term launch, directly in front of cl_tn_backward: the frozen-scaler step stores dz_f (a term added before it
            # would be lost), every other route adds to it -- added last the prior's term is right on all of them
            self._ref_prior(tn, st)
        self._q_launch("backward", tn, st)
        if self.owner:
            # this rank's share of |d a|^2 + |d b|^2 into the message, next to the scaler's gradient
            check(lib.cl_owner_qnorm(ptr(self.grads), self.R, self.shard.kl_begin, self.shard.kl_end, ptr(self.msg_norm),
                                     ptr(self.own_scratch), ptr(self.stop_flag), st), "cl_owner_qnorm")
        if split:
            from careless_amd.distributed import allreduce_flat_
            allreduce_flat_(self.grads[: 2 * self.R], self.process_group)
            tail_work.wait()         # (the current stream waits for the first piece; the host does not block)
        elif dist_on:
            self._allreduce()        # local_only: a test hook that leaves the per-rank partial gradient in place
        self._keep = (u_f, eta, ipred_out)

    def _ref_prior(self, tn: TnArgs, st):
        """The empirical reference prior's share of the step (`cl_ref_prior`): -w log p of the step's samples into the KL -- per-workgroup
        sums in kl_part_dw, which the step's cl_tn_backward adds up -- and -w kl_weight dlog p / dz onto dz_f, for the observed reflections
        whose KL this rank owns."""
        ref = self.ref
        a = RefPriorArgs()
        a.z_f, a.dz_f = tn.z_f, ptr(self.dz_f)
        a.loc, a.scale, a.observed, a.centric = ptr(ref["loc"]), ptr(ref["scale"]), ptr(ref["observed"]), ptr(ref["centric"])
        a.kind, a.dof = ref["kind"], ref["dof"]
        a.R, a.S = self.R, self.S
        a.w_kl, a.kl_grad_mult = tn.w_kl, tn.kl_grad_mult
        a.kl_begin, a.kl_end = tn.kl_begin, tn.kl_end
        a.kl_part, a.scalars, a.stop_flag = tn.kl_part_dw, tn.scalars, tn.stop_flag
        check(self.lib.cl_ref_prior(C.byref(a), st), "cl_ref_prior")

    def _zero_step(self):
        """Clear the step's accumulators: dz_f, the flat gradient, the scalars.  An owner-mode rank only ever touches the dz_f rows and
        the q gradients of its own reflections (those gradients are rewritten, not accumulated, by nobody else): it clears its slice
        of dz_f and everything from the gradients on."""
        if not self.owner:
            self.ws.zero_()
            return
        r0, r1 = self.shard.kl_begin, self.shard.kl_end
        self.dz_f[r0 * self.S:r1 * self.S].zero_()
        self.ws_step.zero_()

    def _det_reduce(self, obs, st):
        det, lay = obs.det, self.layout
        a = DetArgs()
        # (records stored in reflection order -- det_slot -- need no gather list)
        a.dzf_obs, a.perm_refl, a.seg_refl = ptr(det.dzf), (None if det.slot is not None else ptr(det.refl[0])), ptr(det.refl[1])
        a.R, a.S, a.dz_f = self.R, self.S, ptr(self.dz_f)
        if lay.n_img > 0:
            a.dimg_obs, a.perm_img, a.seg_img = ptr(det.dimg), ptr(det.img[0]), ptr(det.img[1])
            a.n_images, a.d_img = det.M, self._grad_ptr("img")
        a.nll_part, a.nparts, a.scalars = ptr(det.nll), int(det.nll.numel()), ptr(self.scalars)
        a.stop_flag = ptr(self.stop_flag)
        if self.ev11:
            a.ev11_part, a.n_ev11, a.d_ev11 = ptr(det.ev11), int(det.ev11.numel()) // 3, self._grad_ptr("ev11")
        check(self.lib.cl_det_reduce(C.byref(a), st), "cl_det_reduce")

    def _data_term(self, obs, step: int, eta, ipred_out, st, defer_reduce: bool = False, train: bool = False):
        """NLL of `obs` into scalars[NLL] and its gradient into dz_f / the flat gradient (scaler + image scales): one launch sequence per
        piece of the set, then -- deterministic mode -- the fixed-order sums over the whole set.  `defer_reduce`: a single fused launch
        leaves its partial reduction to the caller (`self._pending_reduce`: forward_backward hands it to the step's cl_tn_backward launch).
        A neural likelihood: cl_nlik_forward over the whole set in front (the pieces then read sigpred for SigIobs: `_sig`, and write their
        predictions), and -- `train`: a training step -- cl_nlik_backward behind."""
        if obs.empty:
            return
        chunked = isinstance(obs, ObsChunks)
        if self.neural:
            ipred_out = self._nlik_ipred(obs) if ipred_out is None else ipred_out
            self._nlik_forward(obs, True, st)
        for piece in (obs.children if chunked else [obs]):
            self._data_term_launch(piece, step, eta, ipred_out, st, defer_reduce and not chunked)
        if self.deterministic:
            self._det_reduce(obs, st)
        if self.neural and train and getattr(self.lik, "trainable", True):
            self._nlik_backward(obs, ipred_out, st)

    def _data_term_launch(self, obs: ObsData, step: int, eta, ipred_out, st, defer_reduce: bool):
        """The data term of one `ObsData`: exactly one path, then the reduction of the weight-gradient partials that goes with it."""
        lib, lay = self.lib, self.layout
        form = self._frozen_form(obs, injected=eta is not None or ipred_out is not None)
        if form is not None:
            self._data_term_frozen(form, obs, step, eta, ipred_out, st)       # (no scaler gradient: nothing to reduce)
            return
        if self.wide:
            self._data_term_wide(obs, step, eta, ipred_out, st)               # (reduces layer by layer)
            return
        ma = self._mlp_args(step, eta, ipred_out, obs)
        if self.blocks is not None:
            self._data_term_chain(ma, obs, step, eta, ipred_out, st)          # (reduces block by block)
            return
        a, mode = self._likelihood_args(ma, obs)
        if mode == 2:
            self._laue_passes(a, obs, step, eta, ipred_out, st)
        else:
            # (deterministic mode: every workgroup of the launch STORES its NLL slot, det.grid slots per piece -- nothing to clear;
            #  the slots a short last piece leaves unwritten were zero-initialised and are never touched)
            self._fused_step_launch(a, obs, st)
            if obs.fused_laue:
                # single pass: the harmonic group sums happen inside the fused kernel; the padded slots (no rows, iconv = 0,
                # reference formatter.py:637-640 / laue.py:24) only add their constant -- and, with Ev11, its gradient
                self._laue_pad_slots(a, obs, st)
        if self.peel and mode == 0:
            self._peel_reduce(obs, st, a.n_obs)
        elif defer_reduce and not self.deterministic:
            self._pending_reduce = (ptr(obs.partials), obs.grid, lay.P, self._grad_ptr("mlp"))
        else:
            check(lib.cl_reduce_partials(ptr(obs.partials), obs.grid, lay.P, self._grad_ptr("mlp"), ptr(self.stop_flag), st), "cl_reduce_partials")

    def _laue_pad_slots(self, ma, obs: ObsData, st):
        """The padded slots of a packed Laue observation set (no rows, iconv = 0: reference formatter.py:637-640 / laue.py:24) add their
        constant to the NLL -- and, with Ev11, its gradient -- through one small `cl_laue_likelihood` launch.  `ma`: the arguments of the
        rows' own launch (`cl_mlp_args` or `cl_frozen_args`: its w_ll, ev11, d_ev11).  (Of the per-step constants this launch reads the
        likelihood's alone: the other shared fields stay zero.)"""
        lib = self.lib
        npad = int(obs.pad_iobs.numel())
        if npad <= 0:
            return
        nslot = 1 if obs.pad_uniform else npad                  # all padded slots alike: one slot, weight x their number
        obs.pad_iconv[: nslot * self.S].zero_()
        la = LaueArgs()
        la.iobs, la.sig, la.iconv = ptr(obs.pad_iobs), ptr(obs.pad_sig), ptr(obs.pad_iconv)
        la.n_obs, la.S = nslot, self.S
        la.lik_kind, la.dof, la.lik_const = self.lik_kind, self.dof, self.lik_const
        la.w_ll = ma.w_ll * (npad if obs.pad_uniform else 1)
        la.scalars, la.stop_flag = ptr(self.scalars), ptr(self.stop_flag)
        la.ev11, la.d_ev11 = ma.ev11, ma.d_ev11
        if self.deterministic:      # the padded slots' workgroups store their NLL behind the fused launch's parts
            la.nll_part, la.ev11_part = self._det_parts(obs, obs.det_parent.det.pieces)
        check(lib.cl_laue_likelihood(C.byref(la), st), "cl_laue_likelihood")

    def _peel_bufs(self, obs: ObsData):
        """Buffers of the peeled first layer for one observation set: its pre-activations and dZ_0 (feature-major, like meta_t), the
        weight-gradient partials; per engine: the peeled scaler's parameters and reduced gradient."""
        if obs.peel is None:
            rows = int(self.lib.cl_mlp_meta_rows(self.w))
            nparts = int(self.lib.cl_peel_parts(obs.n_pad))     # (packed layouts: every row of the padded axis may be a real one)
            obs.peel = PeelBuffers(u=torch.zeros(rows * obs.n_pad, dtype=torch.float32, device=self.device),
                                   dz0=torch.zeros(rows * obs.n_pad, dtype=torch.float32, device=self.device),
                                   parts=torch.empty(nparts * (self.w * self.d + self.w), dtype=torch.float32, device=self.device), nparts=nparts)
        if self.peel_params is None:
            Pp = int(self.lib.cl_mlp_param_count(self.w, self.w, self.L))
            self.peel_params = torch.zeros(Pp, dtype=torch.float32, device=self.device)
            self.peel_grad = torch.zeros(Pp, dtype=torch.float32, device=self.device)
        return obs.peel

    def _peel_args(self, ma: MlpArgs, obs: ObsData) -> MlpArgs:
        """The fused launch behind the peeled first layer: the layer's pre-activations as metadata, identity first layer, dZ_0 out."""
        pb = self._peel_bufs(obs)
        a = _copy_args(ma)
        a.meta_t, a.d, a.mlp, a.dZ0_out = ptr(pb.u), self.w, ptr(self.peel_params), ptr(pb.dz0)
        return a

    def _fused_step_launch(self, a: MlpArgs, obs: ObsData, st):
        """cl_elbo_mono_fwd_bwd on `_likelihood_args`' arguments, behind cl_peel_forward when the first layer is peeled (self.peel)."""
        if self.peel:
            check(self.lib.cl_peel_forward(ptr(obs.meta_t), a.n_obs, obs.n_pad, self.d, self.w, self.L, self._param_ptr("mlp"), ptr(obs.peel.u),
                                           ptr(self.peel_params), ptr(self.peel_grad), int(self.peel_grad.numel()), ptr(self.stop_flag), st), "cl_peel_forward")
        check(self.lib.cl_elbo_mono_fwd_bwd(C.byref(a), obs.grid, st), "cl_elbo_mono_fwd_bwd")

    def _peel_reduce(self, obs: ObsData, st, n_obs: int):
        """Gradient of a step with a peeled first layer: the launch's partials -> the peeled scaler's gradient; layer 0's own gradient
        from dZ_0 and the metadata, everything behind it copied over (cl_peel_backward)."""
        pb = obs.peel
        check(self.lib.cl_reduce_partials(ptr(obs.partials), obs.grid, int(self.peel_grad.numel()), ptr(self.peel_grad), ptr(self.stop_flag), st),
              "cl_reduce_partials")
        check(self.lib.cl_peel_backward(ptr(obs.meta_t), n_obs, obs.n_pad, self.d, self.w, self.L, ptr(pb.dz0), ptr(self.peel_grad),
                                        self._grad_ptr("mlp"), ptr(pb.parts), pb.nparts, ptr(self.stop_flag), st), "cl_peel_backward")

    def _block_args(self, ma: MlpArgs, obs: ObsData, k: int) -> MlpArgs:
        """Arguments of block k of the chain: its slice of the parameters, its input (metadata or the previous block's output)."""
        return block_fields(_copy_args(ma), self.blocks[k], self._param_ptr("mlp"), ptr(obs.meta_t) if k == 0 else ptr(obs.chain_act[k - 1]))

    def _data_term_chain(self, ma: MlpArgs, obs: ObsData, step: int, eta, ipred_out, st):
        """Scaler deeper than one launch: forward through the head-less blocks (activations to HBM), the last block does the
        likelihood and its own backward (recomputing its forward), then the blocks are walked back, each recomputing its
        forward from its stored input.  8 P_mm flops per observation instead of 6, plus 2 x 8 w bytes per block boundary."""
        lib, K = self.lib, len(self.blocks)
        gptr = lambda k: self._grad_ptr("mlp", self.blocks[k].off)
        for k in range(K - 1):
            a = self._block_args(ma, obs, k)
            a.act_out = ptr(obs.chain_act[k])
            check(lib.cl_mlp_forward(C.byref(a), obs.grid, st), "cl_mlp_forward")
        a, _ = self._likelihood_args(ma, obs)
        if self.laue:
            a.dO_ext = ptr(obs.laue_dO)
            self._laue_passes(a, obs, step, eta, ipred_out, st)
        else:
            check(lib.cl_elbo_mono_fwd_bwd(C.byref(a), obs.grid, st), "cl_elbo_mono_fwd_bwd")
            if self.chain_lane:     # the last block on the lane kernel handed back dZ_0 of its first layer: dX = W_0^T dZ_0
                check(lib.cl_chain_dx(ptr(obs.chain_dz0), a.mlp, a.n_obs, obs.n_pad, self.w, self.w, ptr(obs.chain_dact[K - 2]), ptr(self.stop_flag), st), "cl_chain_dx")
        check(lib.cl_reduce_partials(ptr(obs.partials), obs.grid, self.blocks[K - 1].P, gptr(K - 1), ptr(self.stop_flag), st),
              "cl_reduce_partials")
        for k in range(K - 2, -1, -1):
            a = self._block_args(ma, obs, k)
            a.dH_ext = ptr(obs.chain_dact[k])
            a.dX_out = ptr(obs.chain_dact[k - 1]) if k > 0 else None
            check(lib.cl_mlp_backward_ext(C.byref(a), obs.grid, st), "cl_mlp_backward_ext")
            check(lib.cl_reduce_partials(ptr(obs.partials), obs.grid, self.blocks[k].P, gptr(k), ptr(self.stop_flag), st),
                  "cl_reduce_partials")

    def evaluate_nll(self, obs: ObsData, key: int, u_f=None, eta=None) -> float:
        """NLL of another observation set under the current parameters with fresh Monte-Carlo noise -- what
        `model.test_on_batch(validation_data)` reports as "NLL" (reference variational.py:257-260).  `u_f` (S, R) / `eta`
        (S, N_val) inject the noise (parity tests).  Uses the step workspace (call it between steps); synchronises."""
        lib, st = self.lib, _stream()
        u_f, eta = self._noise_to_device(u_f, eta, obs)
        self._zero_step()
        tn = self._tn_args(key, u_f)
        self._q_launch("forward", tn, st)
        self._data_term(obs, key, eta, None, st)
        if self.owner and self.shard.world > 1 and not self.local_only:
            # an owner-mode rank holds the validation rows of ITS reflections (make_obs): the set's NLL is the sum over the ranks
            import torch.distributed as dist
            t = self.scalars[0:1].clone()
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.process_group)
            return float(t.item())
        torch.cuda.synchronize()
        return float(self.scalars[0].item())

    def make_obs(self, inputs) -> ObsData:
        """Device image of another observation set (validation data) for `evaluate_nll`."""
        if BaseModel.is_laue(inputs) != self.laue:
            raise ValueError("validation data and training data differ in kind (mono / Laue)")
        rows = None
        if self.owner:
            # validation rows follow their reflections' owner (only the owner samples them); a rank none of whose reflections occurs
            # in the set launches nothing and contributes 0 to the sum
            rid = _np(BaseModel.get_refl_id(inputs)).reshape(-1)
            rows = np.nonzero((rid >= self.shard.kl_begin) & (rid < self.shard.kl_end))[0]
            if len(rows) == 0:
                return _EmptyObs(int(len(rid)))
        o = self._build_obs(inputs, 0, None, None, None, rows=rows)
        if o.d != self.d:
            raise ValueError("validation metadata width differs from the training data")
        return o

    def _laue_passes(self, ma: MlpArgs, obs: ObsData, step: int, eta, ipred_out, st):
        """Harmonic deconvolution (reference likelihoods/laue.py:9-47): scaler forward, predict + group sums, likelihood on
        the slots, gradient broadcast back to the rows, scaler backward from dL/d(loc, sigma).  `ma`: the backward launch's arguments
        (`dO_ext` set: `_likelihood_args`); the forward launch runs on a copy without it."""
        lib = self.lib
        ma.loc_out, ma.sig_out = ptr(obs.laue_loc), ptr(obs.laue_sig)
        fwd = _copy_args(ma)
        fwd.dO_ext = None
        check(lib.cl_mlp_forward(C.byref(fwd), obs.grid, st), "cl_mlp_forward")
        self._slot_likelihood(ma, obs, step, eta, ipred_out, st)
        check(lib.cl_mlp_backward_ext(C.byref(ma), obs.grid, st), "cl_mlp_backward_ext")

    def _slot_args(self, ma: MlpArgs, obs: ObsData, step: int, eta, ipred_out, a: int = 0, n: Optional[int] = None) -> LaueArgs:
        """Arguments of the slot likelihood kernels for the rows [a, a + n) of `obs` (default: all of them)."""
        la = self._step_fields(LaueArgs(), obs, step)
        n = obs.N - a if n is None else n
        off = lambda t, size: None if t is None else t.data_ptr() + size * a
        la.refl_id, la.image_id, la.harmonic_id = off(obs.refl_id, 4), off(obs.image_id, 4), off(obs.harmonic_id, 4)
        la.loc, la.sigma, la.iobs, la.sig = off(obs.laue_loc, 4), off(obs.laue_sig, 4), off(obs.iobs, 4), off(self._sig(obs, obs.sig), 4)
        la.n_obs, la.obs_offset = n, obs.start + a
        la.img, la.use_img, la.d_img = ma.img, ma.use_img, ma.d_img
        la.eta, la.ipred_out = off(eta, 4 * self.S), off(ipred_out, 4 * self.S)
        la.iconv, la.dO = off(obs.laue_iconv, 4 * self.S), off(obs.laue_dO, 8)
        la.row_index = off(obs.row_index, 8)
        return la

    def _slot_likelihood(self, ma: MlpArgs, obs: ObsData, step: int, eta, ipred_out, st, frozen: bool = False):
        """From (loc, sigma) per row in obs.laue_loc / laue_sig: sample, predict, group sums, slot likelihood (NLL into the
        scalars), its gradient back on the rows -> dz_f, d(image scales), obs.laue_dO = dL/d(loc, sigma) per row."""
        lib = self.lib
        if obs.harmonic_id is not None:
            obs.laue_iconv.zero_()          # (group sums accumulate by atomics; rows that are their own slot -- harmonic_id None -- store)
        la = self._slot_args(ma, obs, step, eta, ipred_out)
        if self.deterministic and obs.harmonic_id is None:
            # no float atomics: the amplitude gradient of every (row, sample) and the image-scale term of every row are stored (records in
            # reflection order: det_slot), every workgroup stores its NLL; cl_det_reduce sums them in a fixed order after the backward pass
            det = obs.det_parent.det
            la.dzf_obs, la.dimg_obs, la.det_slot = ptr(det.dzf), ptr(det.dimg), ptr(det.slot)
            la.nll_part, la.ev11_part = self._det_parts(obs, det.pieces)
            check(lib.cl_slot_rows(C.byref(la), st), "cl_slot_rows")
            return
        if obs.harmonic_id is None and self.SLOT_ROWS_ONE_LAUNCH:
            # every row its own slot (monochromatic data on the layer-by-layer path): one launch, no round trip through iconv
            check(lib.cl_slot_rows(C.byref(la), st), "cl_slot_rows")
            return
        check(lib.cl_laue_predict(C.byref(la), st), "cl_laue_predict")
        check(lib.cl_laue_likelihood(C.byref(la), st), "cl_laue_likelihood")
        if frozen:
            la.dO = None                # nobody takes dL/d(loc, sigma) of a frozen scaler: amplitude gradients only (no clearing, no row sums)
        check(lib.cl_laue_backward(C.byref(la), st), "cl_laue_backward")

    def _allreduce(self):
        from careless_amd.distributed import allreduce_flat_
        # row split: the whole flat gradient (2 R + P + ... floats); reflection-owner split: the scaler's part and the norm terms
        allreduce_flat_(self.msg if self.owner else self.grads, self.process_group)

    def sync_owned(self):
        """Reflection-owner mode: every rank has updated a and b of its own reflections only; after training all ranks need all of
        them (the output step, saved weights, a later `train_model` call).  One sum all-reduce of a vector that is zero outside the
        rank's own ranges -- once per training run, not per step.  Adam's moments stay with the owner (ownership is fixed for the
        engine's lifetime)."""
        if not self.owner or self.shard.world <= 1 or self.local_only:
            return
        import torch.distributed as dist
        if not dist.is_initialized():
            return
        from careless_amd.distributed import gather_owned_
        gather_owned_(self.params, self.R, self.shard.kl_begin, self.shard.kl_end, self.process_group)

    def optimizer_step(self, step_index: int):
        lib, st, opt = self.lib, _stream(), self.opt
        n = self.layout.n
        clipnorm = float(opt.clipnorm or 0.0)
        use_seg = clipnorm > 0.0
        # the clip modes that need the norm BEFORE the update get their own pass; otherwise the norm rides inside the Adam kernel
        norm_first = use_seg or float(opt.global_clipnorm or 0.0) > 0.0
        if norm_first:
            check(lib.cl_grad_sqnorm(ptr(self.grads), n, ptr(self.seg_off), self.nseg, ptr(self.seg_sq) if use_seg else None,
                                     ptr(self.scalars), ptr(self.frozen) if self.any_frozen else None, ptr(self.stop_flag), st), "cl_grad_sqnorm")
            if self.owner:
                # the pass above saw this rank's own q gradients (the others' entries are zero here) and the all-reduced tail: trade
                # the own share (cl_owner_qnorm's double accumulators) for the sum over the ranks that came back in the message
                tot, own = self.msg_norm.double(), self.own_scratch
                self.scalars[2] += tot[0] - own[0]
                self.scalars[3] += tot[1] - own[1]
                if use_seg:
                    self.seg_sq[0] += tot[2] - own[2]
                    self.seg_sq[1] += tot[3] - own[3]
        self.t += 1
        t = self.t
        a = AdamArgs()
        a.p = ptr(self.params); a.g = ptr(self.grads); a.m = ptr(self.adam_m); a.v = ptr(self.adam_v)
        a.n = n
        a.alpha = opt.learning_rate * math.sqrt(1.0 - opt.beta_2 ** t) / (1.0 - opt.beta_1 ** t)
        a.beta1, a.beta2, a.adam_eps = opt.beta_1, opt.beta_2, opt.epsilon
        # tf_keras applies the FIRST active clip mode only -- clipnorm, else global_clipnorm, else clipvalue
        # (`_BaseOptimizer._clip_gradients` [3P-recall]; oracle.clip_grads): the kernel sees one mode
        a.global_clipnorm = 0.0 if clipnorm > 0.0 else float(opt.global_clipnorm or 0.0)
        a.clipnorm = clipnorm
        a.clipvalue = 0.0 if (clipnorm > 0.0 or a.global_clipnorm > 0.0) else float(opt.clipvalue or 0.0)
        a.seg_off, a.nseg = ptr(self.seg_off), self.nseg
        a.seg_sq = ptr(self.seg_sq)
        a.frozen = ptr(self.frozen) if self.any_frozen else None
        a.scalars = ptr(self.scalars)
        a.stop_flag = ptr(self.stop_flag)
        a.norm_out = None if norm_first else ptr(self.scalars)
        if self.owner:
            # update what this rank owns -- a and b of its reflections -- and the replicated tail; the norm fused into the call covers
            # the tail, the q part over all ranks arrives in the message
            r0, r1, R = self.shard.kl_begin, self.shard.kl_end, self.R
            a.n_ranges = 3
            a.range_begin[0], a.range_end[0] = r0, r1
            a.range_begin[1], a.range_end[1] = R + r0, R + r1
            a.range_begin[2], a.range_end[2] = 2 * R, n
            a.norm_skip_ranges = 2
            a.norm_extra = None if norm_first else ptr(self.msg_norm)
        n_part = 0
        if not norm_first:
            # the norm fused into the update leaves one pair of sums per workgroup; cl_step_finalize adds them up
            a.norm_part = ptr(self.norm_part)
            n_part = int(lib.cl_adam_grid(C.byref(a)))
        check(lib.cl_adam_step(C.byref(a), st), "cl_adam_step")
        check(lib.cl_step_finalize(ptr(self.scalars), self.kl_mult, ptr(self.history_buf), step_index,
                                   ptr(self.stop_flag), ptr(self.norm_part) if n_part else None, n_part, st), "cl_step_finalize")

    def alloc_history(self, steps: int):
        self.history_buf = torch.zeros(max(1, steps) * _lib.CL_HIST_STRIDE, dtype=torch.float64, device=self.device)
        self.stop_flag.zero_()
        self._hist_reduced = False
        self.rdw_hist = (torch.zeros(max(1, steps), self.layout.n_dwr, dtype=torch.float32, device=self.device)
                         if self.dw_trainable else None)

    def train_step(self, step_index: int, u_f=None, eta=None):
        """One full ELBO step; `step_index` indexes the history buffer, the noise key is the optimizer iteration."""
        if self.dw_trainable:           # the "rDW_i" metrics are the values used in this step's forward pass (wilson.py:173-174)
            self.rdw_hist[step_index] = torch.sigmoid(self.layout.view(self.params, "dwr"))
        self.forward_backward(self.t, u_f, eta)
        self.optimizer_step(step_index)

    def read_history(self, steps: int) -> Dict[str, List[float]]:
        """Synchronise and convert the device history to the reference's dict of lists (variational.py:262-268).
        Steps after the first non-finite gradient norm were skipped on the device and are dropped, which reproduces
        the reference's early `break` (:271-274)."""
        if self.shard.world > 1 and not self.local_only and not self._hist_reduced:
            self._hist_reduced = True
            # the records hold this rank's partial NLL / KL: summed over the ranks once, in fp64 (careless_amd/distributed.py)
            from careless_amd.distributed import allreduce_history_
            allreduce_history_(self.history_buf, _lib.CL_HIST_STRIDE, self.kl_mult, self.process_group)
        h = self.history_buf.view(-1, _lib.CL_HIST_STRIDE)[:steps].cpu().numpy()
        keep = h[:, 4] == 0.0
        h = h[keep]
        out = {"Grad Norm": h[:, 3].tolist()}
        out["loss"] = h[:, 0].tolist()
        out["F KLDiv"] = h[:, 1].tolist()
        out["NLL"] = h[:, 2].tolist()
        if self.dw_trainable:
            r = self.rdw_hist[:steps].cpu().numpy()[keep]
            for i in range(r.shape[1]):
                out[f"rDW_{i}"] = r[:, i].tolist()
        return out

    # -- accessors used by tests -----------------------------------------------------------------------------
    def loss_terms(self) -> Dict[str, float]:
        s = self.scalars.cpu().numpy()
        return {"nll": float(s[0]), "kl": float(s[1]), "loss": float(s[0] + self.kl_mult * s[1])}

    def grad_tensors(self) -> List[torch.Tensor]:
        """Gradients split per trainable tensor, in the oracle's order and Keras shapes
        [q_loc_raw, q_scale_raw, W_0 (in,out), b_0, ..., W_o, b_o, image scales, per-image layers, Ev11 | the neural likelihood's
        network (Keras shapes), double-Wilson r]."""
        return self._split(self.grads)

    def param_tensors(self) -> List[torch.Tensor]:
        """The trainable tensors themselves, same order and shapes as `grad_tensors`."""
        return self._split(self.params)

    def _split(self, g: torch.Tensor) -> List[torch.Tensor]:
        return split_flat(g, self.layout, self.mlp.layer_slices(self.d), self.imgl.layer_views if self.imgl is not None else None)


# ------------------------------------------------------------------------------------------------------------
# stand-alone helpers behind the plugin protocol methods
# ------------------------------------------------------------------------------------------------------------
def tn_sample(q, n: int, seed=None, u_f=None) -> torch.Tensor:
    """`TruncatedNormal.sample(n)` -> (n, R) via `cl_tn_forward` (Philox noise unless `u_f` (n,R) is injected); a trainable Rice-Woolfson
    posterior: via `cl_rw_forward`, `u_f` then (2, n, R) standard normals."""
    rw = getattr(q, "posterior_kind", None) == "rice_woolfson"
    dev = require_gpu("RiceWoolfson.sample" if rw else "TruncatedNormal.sample")
    lib = _lib.get_lib()
    R = q.loc_raw.numel()
    loc_raw = q.loc_raw.to(dev, torch.float32).contiguous()
    scale_raw = q.scale_raw.to(dev, torch.float32).contiguous()
    low = q.low.to(dev, torch.float32).contiguous()
    centric = torch.zeros(R, dtype=torch.uint8, device=dev)
    es = torch.ones(R, dtype=torch.float32, device=dev)
    z = torch.empty(R * n, dtype=torch.float32, device=dev)
    sc = torch.zeros(_lib.CL_SC_COUNT, dtype=torch.float64, device=dev)
    du = None
    if u_f is not None and rw:
        du = torch.as_tensor(_np(u_f), dtype=torch.float32).reshape(2, n, R).permute(0, 2, 1).contiguous().to(dev)
    elif u_f is not None:
        du = torch.as_tensor(_np(u_f), dtype=torch.float32).reshape(n, R).t().contiguous().to(dev)
    a = TnArgs()
    a.q_loc_raw, a.q_scale_raw, a.low, a.centric, a.es = ptr(loc_raw), ptr(scale_raw), ptr(low), ptr(centric), ptr(es)
    a.R, a.S = R, n
    a.high, a.eps = q.high, q.scale_shift
    a.w_kl, a.kl_grad_mult = 0.0, 0.0
    a.kl_begin, a.kl_end = 0, 0
    a.u_f = ptr(du)
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    a.seed, a.step = int(seed) & 0xFFFFFFFFFFFFFFFF, 0
    a.z_f, a.scalars = ptr(z), ptr(sc)
    if rw:
        qc = torch.as_tensor(q.centric.astype(np.uint8), device=dev)
        ra = RwArgs()
        ra.tn = a
        ra.q_centric, ra.n_f = ptr(qc), ptr(du)
        ra.tn.u_f = None
        check(lib.cl_rw_forward(C.byref(ra), _stream()), "cl_rw_forward")
    else:
        check(lib.cl_tn_forward(C.byref(a), _stream()), "cl_tn_forward")
    return z.view(R, n).t()


def tn_moments(q, high_m4=np.inf, want=("mean", "std", "m4")):
    """Moments of the truncated-normal posterior for the output step via `cl_tn_moments` (reference surrogate_posteriors.py:23-27,
    55-102; consumed at io/manager.py:188-197): dict with `mean`, `std` (fp32 torch tensors on the device) and `m4` (fp64).
    `high_m4` is the upper bound of the fourth moment (the reference's `moment_4(high=np.inf)` default); mean / std use q.high.
    A trainable Rice-Woolfson posterior: the same dict via `cl_rw_moments` (no bounds)."""
    rw = getattr(q, "posterior_kind", None) == "rice_woolfson"
    dev = require_gpu("RiceWoolfson moments" if rw else "TruncatedNormal moments")
    lib = _lib.get_lib()
    R = q.loc_raw.numel()
    loc_raw = q.loc_raw.to(dev, torch.float32).contiguous()
    scale_raw = q.scale_raw.to(dev, torch.float32).contiguous()
    low = q.low.to(dev, torch.float32).contiguous()
    out = {}
    if "mean" in want:
        out["mean"] = torch.empty(R, dtype=torch.float32, device=dev)
    if "std" in want:
        out["std"] = torch.empty(R, dtype=torch.float32, device=dev)
    if "m4" in want:
        out["m4"] = torch.empty(R, dtype=torch.float64, device=dev)
    if rw:
        qc = torch.as_tensor(q.centric.astype(np.uint8), device=dev)
        check(lib.cl_rw_moments(ptr(loc_raw), ptr(scale_raw), ptr(qc), R, float(q.scale_shift), ptr(out.get("mean")), ptr(out.get("std")),
                                ptr(out.get("m4")), _stream()), "cl_rw_moments")
        return out
    hi4 = float("inf") if high_m4 is None else float(high_m4)
    check(lib.cl_tn_moments(ptr(loc_raw), ptr(scale_raw), ptr(low), R, float(q.high), hi4, float(q.scale_shift),
                            ptr(out.get("mean")), ptr(out.get("std")), ptr(out.get("m4")), _stream()), "cl_tn_moments")
    return out


def predict_moments(scale_mean, scale_std, refl_id, mom):
    """E[I] and var[I] of every observation (fp64 numpy arrays) via `cl_predict_moments` (reference variational.py:80-121) from the scale's
    moments per row (device tensors), the rows' reflection ids and `tn_moments(q)`."""
    dev = require_gpu("prediction_mean_stddev")
    lib = _lib.get_lib()
    sm = scale_mean.to(dev, torch.float32).contiguous().reshape(-1)
    ss = scale_std.to(dev, torch.float32).contiguous().reshape(-1)
    n = int(sm.numel())
    rid = torch.as_tensor(_np(refl_id).reshape(-1).astype(np.int32), device=dev)
    if int(rid.numel()) != n or int(ss.numel()) != n:
        raise ValueError("scale moments and refl_id differ in length")
    iexp = torch.empty(n, dtype=torch.float64, device=dev)
    ivar = torch.empty(n, dtype=torch.float64, device=dev)
    check(lib.cl_predict_moments(ptr(sm), ptr(ss), ptr(rid), n, ptr(mom["mean"]), ptr(mom["std"]), ptr(mom["m4"]), int(mom["mean"].numel()),
                                 ptr(iexp), ptr(ivar), _stream()), "cl_predict_moments")
    return iexp.cpu().numpy(), ivar.cpu().numpy()


def scaler_forward(mlp, metadata, imgl=None, image_id=None):
    """loc, sigma of the scaler's Normal for every row of `metadata`, forward only; `imgl` + `image_id` add the per-image layers of a
    `NeuralImageScaler`.  One question to `cl_mlp_route`, then one of three routes: the fused `cl_mlp_forward` on the whole scaler, a chain
    of layer blocks where a Dense-only scaler is deeper than one launch holds (`chain_plan`), or layer by layer (`_forward_layers`)."""
    dev = require_gpu("MLPScaler.call")
    lib, st = _lib.get_lib(), _stream()
    md = _np(metadata).astype(np.float32)
    md = md.reshape(md.shape[0], -1) if md.ndim > 1 else md.reshape(-1, 1)
    (N, d), w, L = md.shape, mlp.width, mlp.n_layers
    for net in (mlp,) if imgl is None else (mlp, imgl):
        net.build(d)
        if net.flat.device != dev:
            net.flat = net.flat.to(dev)
    ids = None if imgl is None else _np(image_id).reshape(-1).astype(np.int64)
    if imgl is not None and (ids.size != N or (ids.size and (ids.min() < 0 or ids.max() >= imgl.max_images))):
        raise ValueError("image_id does not match the metadata / exceeds max_images")
    packed = dict(row_map=1, tile_img=1, imgl=1, n_imgl=imgl.n_image_layers, n_images=imgl.max_images) if imgl is not None else {}
    fwd = _lib.mlp_route(lib, 1, d=d, w=w, L=L, S=1, meta_t=1, mlp=1, loc_out=1, sig_out=1, **packed)
    loc, sig = (torch.empty(N, dtype=torch.float32, device=dev) for _ in range(2))
    if fwd == _lib.CL_ROUTE_NONE and (imgl is not None or w > 64 or d > 64):
        return _forward_layers(lib, mlp, md, imgl, ids, loc, sig, dev, st)
    a, tile_img, row_map = MlpArgs(), None, None
    if imgl is not None:
        meta_t, _, n_pad, tile_img, row_map = meta_by_image(md, ids, int(lib.cl_mlp_meta_rows(d)))
        tile_img, row_map = torch.as_tensor(tile_img, device=dev), torch.as_tensor(row_map, device=dev)
    else:
        n_pad = _tiles(N)
        meta_t = meta_feature_major(md, int(lib.cl_mlp_meta_rows(d)), n_pad, slice(0, N))
    a.n_obs, a.n_pad, a.S, a.R, a.loc_out, a.sig_out = N, n_pad, 1, 1, ptr(loc), ptr(sig)
    scaler_fields(a, mlp, d, ptr(mlp.flat), imgl, ptr(imgl.flat) if imgl is not None else None, tile_img, row_map)
    grid = min(max(1, int(lib.cl_mlp_default_grid())), n_pad // TILE)
    # one launch holds the scaler, or a chain of blocks, the activations between them in feature-major buffers (ElboEngine._data_term_chain)
    blocks = [LayerBlock(0, L, d, 0, 0, True)] if fwd != _lib.CL_ROUTE_NONE else chain_plan(d, w, L, int(lib.cl_mlp_max_layers(w)))
    act_rows = int(lib.cl_mlp_meta_rows(w)) if len(blocks) > 1 else 0
    xs = [torch.as_tensor(meta_t, device=dev)]
    for b in blocks:
        block_fields(a, b, ptr(mlp.flat), ptr(xs[-1]))
        if not b.final:
            xs.append(torch.zeros(act_rows, n_pad, dtype=torch.float32, device=dev))
        a.act_out = None if b.final else ptr(xs[-1])
        check(lib.cl_mlp_forward(C.byref(a), grid, st), "cl_mlp_forward")
    return loc, sig


def _forward_layers(lib, mlp, md, imgl, ids, loc, sig, dev, st):
    """`scaler_forward` on a scaler no fused launch holds: the layer-by-layer GEMM kernels (ElboEngine._data_term_wide), forward only, in
    row chunks of whole images (rows sorted by image: the per-image layers run grouped), the metadata uploaded chunk by chunk."""
    (N, d), w, L = md.shape, mlp.width, mlp.n_layers
    sh = WideShape(d, w, L, imgl.n_image_layers if imgl is not None else 0, imgl.max_images if imgl is not None else 0, mlp.leakiness)
    perm, seg = image_order(ids, sh.M) if imgl is not None else (None, None)
    ld0, ldw = int(lib.cl_wide_ld(d)), int(lib.cl_wide_ld(w))
    rm = meta_row_major(md if perm is None else md[perm], ld0)
    chunks, tiles, rows = row_chunks(N, seg, max(128, min(N, (FORWARD_CHUNK_BYTES // (8 * max(ld0, ldw))) // 128 * 128)), w, dev)
    x = torch.zeros(rows * ld0, dtype=torch.float32, device=dev)
    hb = [torch.zeros(rows * ldw, dtype=torch.float32, device=dev) for _ in range(2)]
    for ch in chunks:
        x.view(rows, ld0)[: ch.b - ch.a] = torch.as_tensor(rm[ch.a:ch.b], device=dev)
        hs = hidden_forward(lib, ptr(mlp.flat), ptr(imgl.flat) if imgl is not None else None, sh, (x.data_ptr(), ld0),
                            [hb[l & 1].data_ptr() for l in range(L + sh.K)], ldw, ch, tiles and tiles[ch.a], None, st)
        check(lib.cl_wide_head_forward(*hs[-1], ptr(mlp.flat) + 4 * dense_layout(d, w, L)[1], ch.b - ch.a, w, BIJ_KINDS[mlp.scale_bijector], mlp.epsilon,
                                       loc.data_ptr() + 4 * ch.a, sig.data_ptr() + 4 * ch.a, None, st), "cl_wide_head_forward")
    if perm is not None:                    # back to the caller's row order
        inv = torch.as_tensor(perm, device=dev)
        loc[inv], sig[inv] = loc.clone(), sig.clone()
    return loc, sig


def debug_noise(seed: int, step: int, S: int, n: int, offset: int = 0, kind: int = 1) -> torch.Tensor:
    """The noise the kernels draw for (seed, step): kind 0 = q(F) uniforms [n][S], kind 1 = scale normals [n][S], kind 2 = the normal
    pairs (n1, n2) of the Rice-Woolfson posterior [n][S][2]."""
    dev = require_gpu("debug_noise")
    out = torch.empty(n * S * (2 if kind == 2 else 1), dtype=torch.float32, device=dev)
    check(_lib.get_lib().cl_debug_noise(int(seed) & 0xFFFFFFFFFFFFFFFF, step, S, n, offset, kind, ptr(out), _stream()),
          "cl_debug_noise")
    return out.view(n, S, 2) if kind == 2 else out.view(n, S)

