"""The data term on the fused scaler kernels -- `cl_elbo_mono_fwd_bwd`, `cl_mlp_forward`, `cl_mlp_backward_ext` --, as a mixin of
`ElboEngine` next to `WidePath` and `FrozenPath` (split out of careless_amd/engine.py): the one fill of `cl_mlp_args`, and the four routes
of `plan.data_term_route` that launch these kernels, each a method that ends with its own reduction of the weight-gradient partials:
    FUSED      `_data_term_fused`      one launch on the scaler itself (single-pass Laue: + the padded slots), `_reduce_or_defer`
    PEEL       `_data_term_peel`       cl_peel_forward, the same launch on the first layer's pre-activations, `_peel_reduce`
    TWO_PASS   `_data_term_two_pass`   `_laue_passes`: scaler forward, the slot likelihood (careless_amd/slots.py), scaler backward, `_reduce_or_defer`
    CHAIN      `_data_term_chain`      forward block by block, the last block like FUSED or TWO_PASS, backward and reduction block by block

What the module decides: nothing about the route -- `ElboEngine._route` asks `data_term_route` once per piece and `_likelihood_args`
takes its branch from that answer (`training_launch`: from the same question, put for the engine's first piece) -- and one thing about
the reduction: hand it to the step's `cl_tn_backward` launch (`self._pending_reduce`) or run `cl_reduce_partials` now (`_reduce_or_defer`).
Reads of the engine: `lib, device, layout, mlp, imgl, d, w, L, S, blocks, chain_lane, deterministic, stop_flag`, `_route`, `_step_fields`,
`_shard_rows`, `_param_ptr`, `_grad_ptr`, `_sig`, `_det_parts`, `_slot_likelihood`, `_laue_pad_slots`, `_scale_kl`; it sets `peel_params`, `peel_grad`
and `_pending_reduce`.
Reads of an `ObsData`: the row arrays, `partials`, `grid`, the chain's `chain_act / chain_dact / chain_dz0`, the two-pass buffers
`laue_loc / laue_sig / laue_dO`, `det_parent.det`.  Attaches: `obs.peel` (`PeelBuffers`).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import torch

from careless_amd._lib import MlpArgs, check, ptr
from careless_amd.obs import ObsChunks, ObsData
from careless_amd.plan import BIJ_KINDS, LayerBlock, Route


def _copy_args(ma: MlpArgs) -> MlpArgs:
    a = MlpArgs()
    C.memmove(C.byref(a), C.byref(ma), C.sizeof(MlpArgs))
    return a


def scaler_fields(a: MlpArgs, mlp, d: int, pmlp: int, imgl=None, pimgl=None, tile_img=None, row_map=None) -> MlpArgs:
    """The scaler's own fields of `cl_mlp_args`, filled in one place for the training step (`FusedPath._mlp_args`) and the forward-only
    path (`scaler_forward`): the Dense stack at `pmlp`, the per-image layers `imgl` at `pimgl`, and what a packed layout adds (`a.n_pad` is set)."""
    a.mlp = pmlp
    a.d, a.w, a.L, a.leak = d, mlp.width, mlp.n_layers, mlp.leakiness
    a.bij_kind, a.eps = BIJ_KINDS[mlp.scale_bijector], mlp.epsilon
    if row_map is not None:
        a.n_obs, a.row_map = a.n_pad, ptr(row_map)       # packed: validity is per row (row_map / refl_id = -1)
    if imgl is not None:
        a.imgl, a.n_imgl, a.n_images, a.tile_img = pimgl, imgl.n_image_layers, imgl.max_images, ptr(tile_img)
    return a


def block_fields(a: MlpArgs, b: LayerBlock, pmlp: int, x: int) -> MlpArgs:
    """`a` turned into the launch of block `b` of a chain: its slice of the parameters at `pmlp`, its input `x` (metadata or the previous block's output)."""
    a.mlp = pmlp + 4 * b.off
    a.d, a.L, a.meta_t = b.d_in, b.l1 - b.l0, x
    return a


@dataclass
class PeelBuffers:
    """A peeled first layer, per observation set (`ObsData.peel`, `FusedPath._peel_bufs`), feature-major like meta_t."""
    u: torch.Tensor                     # the layer's pre-activations
    dz0: torch.Tensor                   # their gradient
    parts: torch.Tensor                 # weight-gradient partials of cl_peel_backward
    nparts: int


class FusedPath:
    # -- the argument fill ---------------------------------------------------------------------------------------------------
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

    def _likelihood_args(self, ma: MlpArgs, obs: ObsData, mode: int = 0, route: Optional[Route] = None):
        """From `_mlp_args` of `obs`: (arguments, mode) of the scaler launch that computes the likelihood on `route` (default: the route of
        `obs` as a fused launch takes it, `_route(obs)`) -- the launch `plan.route` is the route of: the last block of a chain with its
        dZ_0 (lane kernel) or dX out, the backward launch of the two-pass Laue path (mode 2, dL/d(loc, sigma) in), the launch behind a
        peeled first layer, else the fused launch on the scaler itself.  The data term launches with it, `training_launch` asks about it
        (with a `mode` of its own: the forward-only launch has no peeled form)."""
        route = self._route(obs) if route is None else route
        if route is Route.CHAIN:
            K = len(self.blocks)
            ma = self._block_args(ma, obs, K - 1)
            if self.chain_lane:
                ma.dZ0_out = ptr(obs.chain_dz0)       # dZ_0 of the block's first layer; `cl_chain_dx` turns it into the gradient of the block's input
            else:
                ma.dX_out = ptr(obs.chain_dact[K - 2])
        elif route is Route.TWO_PASS:
            mode = 2 if mode == 0 else mode
            ma.dO_ext = ptr(obs.laue_dO)
            if self.deterministic:          # (as `_laue_passes`: the two scaler launches carry no store targets)
                ma.dzf_obs = ma.dimg_obs = ma.nll_part = ma.det_slot = ma.ev11_part = None
        elif route is Route.PEEL and mode == 0:
            ma = self._peel_args(ma, obs)
        return ma, mode

    def training_launch(self, mode: int = 0):         # (arguments, mode) of the launch kernel_name names; plan.route is its cl_mlp_route
        obs = self.obs.children[0] if isinstance(self.obs, ObsChunks) else self.obs
        return self._likelihood_args(self._mlp_args(0, None, None, obs), obs, mode)

    # -- one launch: FUSED, PEEL -----------------------------------------------------------------------------------------------
    def _reduce_or_defer(self, obs: ObsData, st, defer: bool):
        """The weight-gradient partials of the one launch that holds the whole scaler into the flat gradient: now, or -- `defer`, and not in
        deterministic mode, whose cl_det_reduce follows the data term -- in extra workgroups of the step's cl_tn_backward launch
        (`self._pending_reduce`: `forward_backward` hands it over)."""
        P = self.layout.P
        if defer and not self.deterministic:
            self._pending_reduce = (ptr(obs.partials), obs.grid, P, self._grad_ptr("mlp"))
        else:
            check(self.lib.cl_reduce_partials(ptr(obs.partials), obs.grid, P, self._grad_ptr("mlp"), ptr(self.stop_flag), st), "cl_reduce_partials")

    def _fused_step(self, route: Route, obs: ObsData, step: int, eta, ipred_out, st) -> MlpArgs:
        """The launch of `route` (FUSED or PEEL) and what rides behind it; returns its arguments."""
        a, _ = self._likelihood_args(self._mlp_args(step, eta, ipred_out, obs), obs, route=route)
        # (deterministic mode: every workgroup of the launch STORES its NLL slot, det.grid slots per piece -- nothing to clear;
        #  the slots a short last piece leaves unwritten were zero-initialised and are never touched)
        self._fused_step_launch(a, obs, st, route is Route.PEEL)
        if obs.fused_laue:
            # single pass: the harmonic group sums happen inside the fused kernel; the padded slots (no rows, iconv = 0,
            # reference formatter.py:637-640 / laue.py:24) only add their constant -- and, with Ev11, its gradient
            self._laue_pad_slots(a, obs, st)
        return a

    def _data_term_fused(self, obs: ObsData, step: int, eta, ipred_out, st, defer_reduce: bool):
        self._fused_step(Route.FUSED, obs, step, eta, ipred_out, st)
        self._reduce_or_defer(obs, st, defer_reduce)

    def _data_term_peel(self, obs: ObsData, step: int, eta, ipred_out, st):
        a = self._fused_step(Route.PEEL, obs, step, eta, ipred_out, st)
        self._peel_reduce(obs, st, a.n_obs)

    def _fused_step_launch(self, a: MlpArgs, obs: ObsData, st, peel: bool):
        """cl_elbo_mono_fwd_bwd on `_likelihood_args`' arguments, behind cl_peel_forward when the first layer is peeled."""
        if peel:
            check(self.lib.cl_peel_forward(ptr(obs.meta_t), a.n_obs, obs.n_pad, self.d, self.w, self.L, self._param_ptr("mlp"), ptr(obs.peel.u),
                                           ptr(self.peel_params), ptr(self.peel_grad), int(self.peel_grad.numel()), ptr(self.stop_flag), st), "cl_peel_forward")
        check(self.lib.cl_elbo_mono_fwd_bwd(C.byref(a), obs.grid, st), "cl_elbo_mono_fwd_bwd")

    # -- the peeled first layer (csrc/elbo_peel.hip) ---------------------------------------------------------------------------
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

    def _peel_reduce(self, obs: ObsData, st, n_obs: int):
        """Gradient of a step with a peeled first layer: the launch's partials -> the peeled scaler's gradient; layer 0's own gradient
        from dZ_0 and the metadata, everything behind it copied over (cl_peel_backward)."""
        pb = obs.peel
        check(self.lib.cl_reduce_partials(ptr(obs.partials), obs.grid, int(self.peel_grad.numel()), ptr(self.peel_grad), ptr(self.stop_flag), st),
              "cl_reduce_partials")
        check(self.lib.cl_peel_backward(ptr(obs.meta_t), n_obs, obs.n_pad, self.d, self.w, self.L, ptr(pb.dz0), ptr(self.peel_grad),
                                        self._grad_ptr("mlp"), ptr(pb.parts), pb.nparts, ptr(self.stop_flag), st), "cl_peel_backward")

    # -- two launches around the slot likelihood: TWO_PASS ---------------------------------------------------------------------
    def _data_term_two_pass(self, obs: ObsData, step: int, eta, ipred_out, st, defer_reduce: bool):
        a, _ = self._likelihood_args(self._mlp_args(step, eta, ipred_out, obs), obs, route=Route.TWO_PASS)
        self._laue_passes(a, obs, step, eta, ipred_out, st)
        self._reduce_or_defer(obs, st, defer_reduce)

    def _laue_passes(self, ma: MlpArgs, obs: ObsData, step: int, eta, ipred_out, st):
        """Harmonic deconvolution (reference likelihoods/laue.py:9-47): scaler forward, predict + group sums, likelihood on
        the slots, gradient broadcast back to the rows, scaler backward from dL/d(loc, sigma).  Under a scale prior monochromatic rows
        come here as well (every row its own slot: `cl_slot_rows`).  `ma`: the backward launch's arguments
        (`dO_ext` set: `_likelihood_args`); the forward launch runs on a copy without it."""
        lib = self.lib
        if self.deterministic:
            # (monochromatic rows under a scale prior: neither scaler launch holds a float atomic -- the stores are the slot likelihood's -- and
            #  a launch that carries the store targets is a full step to `cl_mlp_route`)
            ma.dzf_obs = ma.dimg_obs = ma.nll_part = ma.det_slot = ma.ev11_part = None
        ma.loc_out, ma.sig_out = ptr(obs.laue_loc), ptr(obs.laue_sig)
        fwd = _copy_args(ma)
        fwd.dO_ext = None
        check(lib.cl_mlp_forward(C.byref(fwd), obs.grid, st), "cl_mlp_forward")
        self._slot_likelihood(ma, obs, step, eta, ipred_out, st)
        self._scale_kl(ma, obs, step, eta, st)          # a scale prior's KL term adds to dL/d(loc, sigma) (careless_amd/sprior.py); else nothing
        check(lib.cl_mlp_backward_ext(C.byref(ma), obs.grid, st), "cl_mlp_backward_ext")

    # -- a chain of layer blocks: CHAIN ----------------------------------------------------------------------------------------
    def _block_args(self, ma: MlpArgs, obs: ObsData, k: int) -> MlpArgs:
        """Arguments of block k of the chain: its slice of the parameters, its input (metadata or the previous block's output)."""
        return block_fields(_copy_args(ma), self.blocks[k], self._param_ptr("mlp"), ptr(obs.meta_t) if k == 0 else ptr(obs.chain_act[k - 1]))

    def _data_term_chain(self, obs: ObsData, step: int, eta, ipred_out, st):
        """Scaler deeper than one launch: forward through the head-less blocks (activations to HBM), the last block does the
        likelihood and its own backward (recomputing its forward), then the blocks are walked back, each recomputing its
        forward from its stored input.  8 P_mm flops per observation instead of 6, plus 2 x 8 w bytes per block boundary."""
        lib, K = self.lib, len(self.blocks)
        ma = self._mlp_args(step, eta, ipred_out, obs)
        gptr = lambda k: self._grad_ptr("mlp", self.blocks[k].off)
        for k in range(K - 1):
            a = self._block_args(ma, obs, k)
            a.act_out = ptr(obs.chain_act[k])
            check(lib.cl_mlp_forward(C.byref(a), obs.grid, st), "cl_mlp_forward")
        a, _ = self._likelihood_args(ma, obs, route=Route.CHAIN)
        if self._route(obs, chained=False) is Route.TWO_PASS:       # the last block taken by itself: Laue rows go through the slot likelihood
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
