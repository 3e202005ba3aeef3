"""Host side of the MI355X ELBO engine: turns the plugin objects of a `VariationalMergingModel` plus the reference's
`inputs` tuple into device buffers, and enqueues one ELBO training step as a fixed sequence of C-ABI calls.

What one step replaces in the reference: `train_step_with_gradient_norm` (careless/models/merging/variational.py:185-224)
= forward (`call`, :141-183), `tape.gradient`, `tf.linalg.global_norm`, non-finite sanitise, Adam.

Step schedule (all on one HIP stream, no host synchronisation):
    cl_tn_forward (clears the step's accumulators on its way) -> [cl_nlik_forward: neural likelihood] -> cl_elbo_mono_fwd_bwd
    (a scale prior: cl_mlp_forward -> cl_slot_rows -> cl_scale_kl -> cl_mlp_backward_ext in its place, careless_amd/sprior.py)
    -> [cl_nlik_backward: neural likelihood] -> [cl_ref_prior: empirical reference priors]
    -> cl_tn_backward (carries cl_reduce_partials)        (a Rice-Woolfson posterior: cl_rw_forward / cl_rw_backward in their place)
    -> [cl_owner_qnorm + all-reduce, data-parallel only: the flat gradient (row split) or its tail + 4 norm terms (reflection-owner
    split)] -> [cl_grad_sqnorm: clip modes only] -> cl_adam_step -> cl_step_finalize -> [cl_scale_kl_record: a scale prior]

HBM layout owned by the engine (see include/careless_hip.h):
    params / m / v / grads : one flat fp32 vector  [ q_loc_raw (R) | q_scale_raw (R) | scaler W^T layout (P) | image scales (M-1) | ... ]
    workspace              : [ dz_f (R*S) | grads (n) + message tail | scalars (4 doubles) | per-tensor norms | owner-mode scratch ]
    observation shard      : refl_id i32, image_id i32, meta_t [d][n_pad], iobs, sig [, noise_row]   (immutable)
PyTorch is used for device memory, streams and torch.distributed only.

What lives where (one role per module; every class below is a mixin of `ElboEngine`, none of the modules imports this one):
    obs.py      the observation layouts and the data-parallel splits
    flat.py     the flat parameter vector and the step workspace
    plan.py     every decision taken without a device, and THE route of a piece's data term (`data_term_route`)
    fused.py    `FusedPath`: the fused scaler launches (plain, peeled, two-pass Laue, chain) and their argument fill
    wide.py     `WidePath`: scalers wider than 64, layer by layer
    frozen.py   `FrozenPath`: the data term behind a frozen scaler
    slots.py    `SlotPath`: the slot likelihood those three routes share
    det.py      `DetPath`: deterministic mode's buffers and fixed-order sums
    nlik.py     `NlikPath`: the neural likelihood's buffers and launches
    sprior.py   `SpriorPath`: the scale prior's KL term between the two-pass launches, its value and its history column
This file keeps the engine itself -- the constructor's named steps, the posterior launches, the step schedule (`forward_backward`,
`_data_term`, the route question `_route`), the optimizer, the history, the validation NLL -- and the stand-alone helpers behind the
plugin protocol methods.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional

import numpy as np
import torch

from careless_amd import _lib
from careless_amd._lib import AdamArgs, MlpArgs, RefPriorArgs, RwArgs, TnArgs, check, ptr
from careless_amd.models.base import BaseModel
from careless_amd.models.scaling.nn import dense_layout
# (re-exported, here and below: the tests, bench.py, the scripts and the plugin classes import these names from this module)
from careless_amd.obs import (GRANULE, ObsChunks, ObsData, Shard, _EmptyObs, _ShardRows, _np, _tiles, image_order, laue_group_shard,  # noqa: F401
                              launch_row_limit, make_shard, meta_by_image, meta_feature_major, meta_row_major, owner_bounds, owner_shard,
                              pack_by_image, pack_laue)
from careless_amd.flat import FLAT_GROUPS, FlatLayout, Workspace, bind_flat, carve_workspace, make_layout, split_flat  # noqa: F401
from careless_amd.plan import (BIJ_KINDS, REFPRIOR_KINDS, LayerBlock, Route, ScalerPlan, chain_plan, check_deterministic,  # noqa: F401
                               check_neural_likelihood, check_scale_prior, check_scale_prior_route, data_term_route, plan_scaler,
                               posterior_kind, prior_kind, reference_prior_arrays, switch, wants_owner_shard)
from careless_amd.det import DetBuffers, DetPath  # noqa: F401
from careless_amd.frozen import FrozenPath
from careless_amd.fused import FusedPath, PeelBuffers, _copy_args, block_fields, scaler_fields  # noqa: F401
from careless_amd.nlik import NlikBuffers, NlikPath  # noqa: F401
from careless_amd.slots import SlotPath
from careless_amd.sprior import SCALE_KL_KEY, SpriorBuffers, SpriorPath  # noqa: F401
from careless_amd.wide import WidePath, WideShape, hidden_forward, row_chunks

TILE = _lib.CL_MLP_TILE
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


# ------------------------------------------------------------------------------------------------------------
# the engine
# ------------------------------------------------------------------------------------------------------------
class ElboEngine(FusedPath, WidePath, FrozenPath, SlotPath, DetPath, NlikPath, SpriorPath):
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
        if self.sprior is not None:
            check_scale_prior_route(self.wide, self.owner, self.deterministic, self.laue, self.imgl is not None, self.S)
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
        self._sprior_setup()
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
        # the KL term on the scale distribution ("Σ KLDiv", reference variational.py:156-163): None without a scale prior
        self.sprior = check_scale_prior(model.scale_prior, model.scale_kl_weight)
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
        # (Laue data under a scale prior take the two-pass path: the prior's term sits between its launches)
        two_pass = self.two_pass = self.laue and (bool(getattr(self.model, "laue_two_pass", False)) or self.sprior is not None)
        gmax = int(np.bincount(_np(BaseModel.get_harmonic_id(inputs)).reshape(-1).astype(np.int64)).max()) if self.laue else 1
        self.plan = plan_scaler(self.lib, self.d, self.w, self.L, imgl.n_image_layers if imgl is not None else 0, laue=self.laue,
                                two_pass=two_pass, gmax=gmax, ev11=self.ev11, deterministic=self.deterministic,
                                lik_kind=_lib.CL_LIK_LAPLACE if self.lik.kind == "laplace" else 0, scale_prior=self.sprior is not None)
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
                  laue_single_pass=not getattr(self.model, "laue_two_pass", False) and self.blocks is None and not self.wide and self.sprior is None,
                  wide=self.wide, slot_buffers=self.sprior is not None)
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
        self._sprior_live, self._sprior_first = True, True
        self._data_term(self.obs, step, eta, ipred_out, st, defer_reduce=not split, train=True)
        self._sprior_live = False
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

    def _route(self, obs: ObsData, form=None, wide: bool = False, chained: Optional[bool] = None) -> Route:
        """THE route question (`plan.data_term_route`) for `obs` on this engine's plan.  `_data_term_launch` puts it whole -- `form`, the
        frozen scaler's answer for the step, and the plan's `wide`.  Left at their defaults the answer is the route of the fused scaler
        launch alone, which the frozen and the layer-by-layer route do not have (`_likelihood_args` behind `training_launch`);
        `chained=False`: of a chain's last block taken by itself."""
        return data_term_route(form, wide, self.blocks is not None if chained is None else chained, self.laue, obs.fused_laue, self.peel,
                               scale_prior=self.sprior is not None)

    def _data_term_launch(self, obs: ObsData, step: int, eta, ipred_out, st, defer_reduce: bool):
        """The data term of one `ObsData`: the route question, then the route's method -- each ends with the reduction of the
        weight-gradient partials that goes with it (`defer_reduce`: the two routes of a single reduction may leave it to the caller)."""
        form = self._frozen_form(obs, injected=eta is not None or ipred_out is not None)
        route = self._route(obs, form, self.wide)
        if route is Route.FROZEN:
            self._data_term_frozen(form, obs, step, eta, ipred_out, st)       # (no scaler gradient: nothing to reduce)
        elif route is Route.WIDE:
            self._data_term_wide(obs, step, eta, ipred_out, st)               # (reduces layer by layer)
        elif route is Route.CHAIN:
            self._data_term_chain(obs, step, eta, ipred_out, st)              # (reduces block by block)
        elif route is Route.TWO_PASS:
            self._data_term_two_pass(obs, step, eta, ipred_out, st, defer_reduce)
        elif route is Route.PEEL:
            self._data_term_peel(obs, step, eta, ipred_out, st)               # (`_peel_reduce`)
        else:
            self._data_term_fused(obs, step, eta, ipred_out, st, defer_reduce)

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
        self._scale_kl_record(step_index, st)

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
            allreduce_history_(self.history_buf, _lib.CL_HIST_STRIDE, self.kl_mult, self.process_group, scale_kl=self.sprior is not None)
        h = self.history_buf.view(-1, _lib.CL_HIST_STRIDE)[:steps].cpu().numpy()
        keep = h[:, 4] == 0.0
        h = h[keep]
        out = {"Grad Norm": h[:, 3].tolist()}
        out["loss"] = h[:, 0].tolist()
        out["F KLDiv"] = h[:, 1].tolist()
        out["NLL"] = h[:, 2].tolist()
        if self.sprior is not None:
            out[SCALE_KL_KEY] = h[:, _lib.CL_HIST_SCALE_KL].tolist()
        if self.dw_trainable:
            r = self.rdw_hist[:steps].cpu().numpy()[keep]
            for i in range(r.shape[1]):
                out[f"rDW_{i}"] = r[:, i].tolist()
        return out

    # -- accessors used by tests -----------------------------------------------------------------------------
    def loss_terms(self) -> Dict[str, float]:
        s = self.scalars.cpu().numpy()
        if self.sprior is not None:         # (+ Σ KLDiv with weight 1, whatever kl_weight is)
            skl = self.scale_kl_value()
            return {"nll": float(s[0]), "kl": float(s[1]), "scale_kl": skl, "loss": float(s[0] + self.kl_mult * s[1] + skl)}
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

