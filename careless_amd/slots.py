"""The slot likelihood (csrc/elbo_laue.hip), as a mixin of `ElboEngine` (split out of careless_amd/engine.py): from (loc, sigma) per row in
`obs.laue_loc / laue_sig` -- whoever computed them -- sample the scale, predict, sum the rows of a slot (a harmonic group; a monochromatic
row is its own slot), the slot's log-prob into the NLL, its gradient back on the rows: dz_f, d(image scales), dL/d(loc, sigma).  No scaler
launch happens here.  Three routes share it: the two-pass Laue path (`FusedPath._laue_passes`), the layer-by-layer path
(`WidePath._data_term_wide`: its row chunks also through `_slot_args`) and the slot form of a frozen scaler
(`FrozenPath._data_term_frozen`); the padded slots of a packed Laue set (`_laue_pad_slots`) ride behind the single-pass fused launch and
the harmonic-group form of a frozen scaler.

What the module decides: which of the slot kernels run -- rows that are their own slot in one `cl_slot_rows` launch (always in
deterministic mode; else while `SLOT_ROWS_ONE_LAUNCH`), otherwise `cl_laue_predict`, `cl_laue_likelihood`, `cl_laue_backward`.
Reads of the engine: `lib, S, deterministic, lik_kind, dof, lik_const, scalars, stop_flag`, `_step_fields`, `_shard_rows`, `_sig`, `_det_parts`, `_det_slot_parts`.
Reads of an `ObsData`: the row arrays, `laue_loc, laue_sig, laue_iconv, laue_dO, row_index, harmonic_id, slot_rows`, the padded slots' `pad_*`, and
`det_parent.det`; it attaches nothing.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

from careless_amd._lib import LaueArgs, MlpArgs, check, ptr
from careless_amd.obs import ObsData


class SlotPath:
    SLOT_ROWS_ONE_LAUNCH = True      # rows that are their own slot: predict + log-prob + gradient in one `cl_slot_rows` launch (tests flip it)

    def _slot_args(self, ma: MlpArgs, obs: ObsData, step: int, eta, ipred_out, a: int = 0, n: Optional[int] = None) -> LaueArgs:
        """Arguments of the slot likelihood kernels for the rows [a, a + n) of `obs` (default: all of them)."""
        la = self._step_fields(LaueArgs(), obs, step)
        n = obs.N - a if n is None else n
        off = lambda t, size: None if t is None else t.data_ptr() + size * a
        rows = getattr(obs, "slot_rows", None) or {}       # packed monochromatic rows under a scale prior: the row arrays in the caller's order
        col = lambda k: rows[k] if k in rows else getattr(obs, k)
        sig = self._sig(obs, obs.sig)
        if rows:            # (a neural likelihood's sigpred is in that order itself)
            sig = obs.nlik.sigpred if self.neural else rows["sig"]
        la.refl_id, la.image_id, la.harmonic_id = off(col("refl_id"), 4), off(col("image_id"), 4), off(obs.harmonic_id, 4)
        la.loc, la.sigma, la.iobs, la.sig = off(obs.laue_loc, 4), off(obs.laue_sig, 4), off(col("iobs"), 4), off(sig, 4)
        la.n_obs, la.obs_offset = n, obs.start + a
        la.img, la.use_img, la.d_img = ma.img, ma.use_img, ma.d_img
        # (eta / ipred_out are the whole shard's: a piece of a chunked shard starts at its row0, `_shard_rows`)
        rows = lambda t: None if t is None else self._shard_rows(obs, t) + 4 * self.S * a
        la.eta, la.ipred_out = rows(eta), rows(ipred_out)
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
            det = obs.det_parent.det           # (a piece of a chunked shard -- a scale prior's route -- stores at its row0 inside the shard's records)
            if det.slot is not None:
                la.dzf_obs, la.det_slot = ptr(det.dzf), det.slot.data_ptr() + 4 * obs.row0
            else:
                la.dzf_obs = det.dzf.data_ptr() + 4 * self.S * obs.row0
            la.dimg_obs = det.dimg.data_ptr() + 4 * obs.row0
            la.nll_part, la.ev11_part = self._det_slot_parts(obs)
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
