"""The scale prior's KL term, "Σ KLDiv" (`VariationalMergingModel(..., scale_prior=...)`; csrc/elbo_sprior.hip), as a mixin of `ElboEngine`
next to `NlikPath`.  An engine with a scale prior sends EVERY piece down the two-pass launches (`plan.data_term_route(scale_prior=True)`):
    cl_mlp_forward (loc, sigma out) -> the slot likelihood (careless_amd/slots.py: dO = dL/d(loc, sigma)) -> cl_scale_kl (dO +=) ->
    cl_mlp_backward_ext
and `FusedPath._laue_passes` calls `_scale_kl` between the two -- on monochromatic rows (`cl_slot_rows`), on two-pass Laue rows, and in the
two-pass form of a chain's last block alike.  No fused kernel is touched.

What the module decides: the form of the term (`scale_kl_form`: analytic where TFP has a KL registered -- a bare Normal scale distribution
against a Normal prior --, else on the step's samples), and where the value goes: one double on the device (`SpriorBuffers.value`), summed
over the pieces of a step in launch order, which `cl_scale_kl_record` copies into the step's history record behind `cl_step_finalize`.
Whether a prior is one the engine runs and which routes refuse it is decided before (`plan.check_scale_prior`, `plan.check_scale_prior_route`).
Reads of the engine: `device, lib, sprior, mlp, img, layout, S, seed, deterministic, stop_flag, history_buf`, `_param_ptr`, `_grad_ptr`, `_shard_rows`.
Reads of an `ObsData`: `N, N_total, start, image_id, slot_rows, row_index, laue_loc, laue_sig, laue_dO`; it attaches nothing.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch

from careless_amd import _lib
from careless_amd._lib import SpriorArgs, check, ptr
from careless_amd.obs import ObsData
from careless_amd.plan import SPRIOR_KINDS

SCALE_KL_KEY = "Σ KLDiv"        # the metric's name (reference variational.py:162)


def scale_kl_form(kind: str, has_shift: bool, image_scales: bool) -> int:
    """CL_SPRIOR_ANALYTIC where `scale_dist.kl_divergence(scale_prior)` exists in TFP -- a bare tfd.Normal (no tfb.Shift: scaling/nn.py:84-87,
    no tfb.Scale: scaling/image.py:60-63) against a Normal prior --, else CL_SPRIOR_SAMPLE (reference variational.py:123-139)."""
    return _lib.CL_SPRIOR_ANALYTIC if (kind == "normal" and not has_shift and not image_scales) else _lib.CL_SPRIOR_SAMPLE


@dataclass
class SpriorBuffers:
    """A scale prior, per engine: the launches of a step run one after the other on one stream and share these."""
    part: torch.Tensor          # fp64 [cl_scale_kl_grid]: the workgroups' partials of one launch
    value: torch.Tensor         # fp64 [1]: the step's term, summed over its pieces in launch order
    form: int


class SpriorPath:
    _sprior_live = False        # inside the data term of a training step (`forward_backward`): validation sets take no term
    _sprior_first = True        # the step's next cl_scale_kl launch is its first: it stores the value, later ones add

    def _sprior_setup(self):
        """Buffers of the term (`self.sprior_buf`), sized for the largest launch."""
        self.sprior_buf = None
        if self.sprior is None:
            return
        has_shift = self.mlp.scale_multiplier is not None
        form = scale_kl_form(self.sprior.engine_kind, has_shift, self.layout.n_img > 0)
        grid = int(self.lib.cl_scale_kl_grid(max(1, self.N_total)))
        self.sprior_buf = SpriorBuffers(torch.zeros(grid, dtype=torch.float64, device=self.device),
                                        torch.zeros(1, dtype=torch.float64, device=self.device), form)

    def _scale_kl(self, ma, obs: ObsData, step: int, eta, st):
        """`cl_scale_kl` on the rows of `obs`: behind the slot likelihood, in front of cl_mlp_backward_ext (`ma`: that launch's arguments)."""
        if self.sprior is None or not self._sprior_live:
            return
        sb, sp = self.sprior_buf, self.sprior
        a = SpriorArgs()
        a.loc, a.sigma, a.dO = ptr(obs.laue_loc), ptr(obs.laue_sig), ptr(obs.laue_dO)
        rows = getattr(obs, "slot_rows", None)
        image_id = rows["image_id"] if rows else obs.image_id       # (rows in the caller's order, as loc / sigma / dO are)
        a.image_id, a.img, a.use_img, a.d_img = ptr(image_id), ma.img, ma.use_img, ma.d_img
        if self.deterministic and ma.use_img:           # no float atomic: the row's term joins the slot likelihood's record, cl_det_reduce sums per image
            a.dimg_obs = obs.det_parent.det.dimg.data_ptr() + 4 * obs.row0
        a.shift, a.has_shift = ma.shift, int(self.mlp.scale_multiplier is not None)
        a.kind, a.p_loc, a.p_scale, a.p_df = SPRIOR_KINDS[sp.engine_kind], sp.loc, sp.scale, sp.df
        a.form = sb.form
        a.n, a.obs_offset, a.row_index = obs.N, obs.start, ptr(obs.row_index)
        a.S, a.eta = self.S, self._shard_rows(obs, eta)
        a.seed, a.step = self.seed, step & 0xFFFFFFFF
        a.weight = 1.0 / obs.N_total                    # the mean over the rows of the set the model is called on, all ranks' rows
        a.kl_part, a.value, a.accumulate = ptr(sb.part), ptr(sb.value), int(not self._sprior_first)
        a.stop_flag = ptr(self.stop_flag)
        check(self.lib.cl_scale_kl(C.byref(a), st), "cl_scale_kl")
        self._sprior_first = False

    def _scale_kl_record(self, step_index: int, st):
        """The step's term into its history record (the sixth double) and its loss: a one-thread launch behind `cl_step_finalize`."""
        if self.sprior is not None:
            check(self.lib.cl_scale_kl_record(ptr(self.sprior_buf.value), ptr(self.history_buf), step_index, st), "cl_scale_kl_record")

    def scale_kl_value(self) -> float:
        """Σ KLDiv of the last `forward_backward` (this rank's rows; synchronises)."""
        return float(self.sprior_buf.value.item()) if self.sprior is not None else 0.0
