"""The data term of a step whose scaling model is frozen (`--freeze-scales`; the half-dataset trainings of `--merge-half-datasets`,
reference careless/careless.py:48-50, 102-128 -- as many steps again as the main training), as a mixin of `ElboEngine` next to
`WidePath` (split out of careless_amd/engine.py).  The scaler's output (loc, sigma) per observation is a constant of the training, so a step
needs neither its forward nor its backward pass: (loc, sigma) of every row once per `train_model` call -- any scaler the package runs,
through `scaler_forward` -- then per step only what depends on the sampled amplitudes: sample the scale, predict, log-prob and its
gradient to dz_f (and the Evans-2011 terms).  The scaler's own gradient is not computed at all: the reference takes gradients of
`trainable_variables` only (variational.py:201), so its "Grad Norm" does not see it either.

Two decisions, each written once:
    layout time   `_frozen_layout_kw`: does the engine lay its observations out for a frozen scaler (plain rows in the caller's order: no
                  packing by image), and which `_build_obs` keywords that changes;
    step time     `_frozen_form`: which form a step's data term takes on one `ObsData` -- none (the fused / wide / chain step), rows sorted
                  by reflection (`cl_frozen_rows`, csrc/elbo_frozen.hip), harmonic groups (the two-call form of `cl_frozen_rows`), or
                  round 5's slot kernels (`SlotPath._slot_likelihood`, careless_amd/slots.py).
The per-training state of the two `cl_frozen_rows` forms is one record each (`SortedRows`, `GroupRows`) at `obs.frozen_sorted`; the slot
form reads `obs.laue_*` through `_slot_args` like the two-pass Laue path.  Defined elsewhere and used here: `_slot_likelihood` and
`_laue_pad_slots` (slots.py), `_mlp_args` (fused.py), `_sig` (nlik.py), `_step_fields` / `_shard_rows` (engine.py).  The index arithmetic of both records is in two functions of
torch tensors (`sorted_row_order`, `group_row_order`) that run on any device without an engine.
"""
from __future__ import annotations

import ctypes as C
import enum
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from careless_amd._lib import FrozenArgs, check, ptr
from careless_amd.models.base import BaseModel
from careless_amd.obs import ObsData, _np


class FrozenForm(enum.Enum):
    SORTED_ROWS = 1       # monochromatic rows sorted by reflection: one `cl_frozen_rows` call
    GROUPS = 2            # harmonic groups in the packed order of the single-pass kernels: `cl_frozen_rows` twice
    SLOTS = 3             # the slot kernels on rows in the caller's order (round 5; deterministic mode, plain Laue rows, the reference paths)


def _key32(key: torch.Tensor) -> torch.Tensor:
    """The noise key of every row as the kernels read it (int32): the global row number.  One that does not fit would draw other noise
    and index eta / ipred_out below zero, silently."""
    if key.numel() and int(key.max()) >= 1 << 31:
        raise ValueError(f"a frozen-scaler shard reaches global row {int(key.max())}: the kernels key a row's noise by its 32-bit global row "
                         "number (< 2^31) -- shard the data further")
    return key.to(torch.int32).contiguous()


def sorted_row_order(refl_id: torch.Tensor, start: int, row_index: Optional[torch.Tensor] = None):
    """Monochromatic rows for `cl_frozen_rows`: (order, key) -- the stable order by reflection of the rows `refl_id` and the int32 noise key
    of every SORTED row: its global row, row_index[i] when the rows are not the contiguous range from `start`."""
    order = torch.argsort(refl_id, stable=True)
    return order, _key32(row_index.index_select(0, order) if row_index is not None else order + int(start))


def group_row_order(refl_id: torch.Tensor, row_map: torch.Tensor, start: int, noise_row: Optional[torch.Tensor] = None):
    """Harmonic groups in the packed order (`refl_id`, `row_map` over the n_pad positions; padding row_map = -1, rows without a reflection
    refl_id = -1) for the two calls of `cl_frozen_rows`: (rmc, key, src, dst, refl_sorted, n2) -- the caller's local row of every position
    clamped to 0 on padding, the int32 noise key of every position (`noise_row` where the shard brings one), `src` the n2 active positions
    in stable reflection order, `dst` its inverse (the position of a row in that order, -1 elsewhere), and the reflections of `src`."""
    rmc = row_map.long().clamp(min=0)
    key = noise_row if noise_row is not None else _key32(rmc + int(start))
    active = torch.nonzero((row_map >= 0) & (refl_id >= 0)).flatten()
    src = active.index_select(0, torch.argsort(refl_id.index_select(0, active), stable=True))
    n2 = int(src.numel())
    dst = torch.full((int(refl_id.numel()),), -1, dtype=torch.int32, device=refl_id.device)
    dst[src] = torch.arange(n2, dtype=torch.int32, device=refl_id.device)
    return rmc, key, src, dst, refl_id.index_select(0, src).to(torch.int32).contiguous(), n2


@dataclass
class SortedRows:
    """Per-training state of `FrozenForm.SORTED_ROWS`: the row arrays of `cl_frozen_args` in reflection order and the edge workspace."""
    epoch: int                          # the `train_model` call it was built in
    rows_loc: torch.Tensor              # (loc, sigma) it was built from, in the caller's row order
    rows_sigma: torch.Tensor
    refl: torch.Tensor
    loc: torch.Tensor
    sigma: torch.Tensor
    aim: Optional[torch.Tensor]
    iobs: torch.Tensor
    sig: torch.Tensor
    key: torch.Tensor
    edge_rid: torch.Tensor
    edge_val: torch.Tensor


@dataclass
class GroupRows:
    """Per-training state of `FrozenForm.GROUPS`: per packed position (loc, sigma), image scale and noise key; the first call's scatter map
    `dst`; the second call's reflections, its `n2` rows of gradients `gbuf` and edge workspace."""
    epoch: int
    rows_loc: torch.Tensor
    rows_sigma: torch.Tensor
    loc: torch.Tensor
    sigma: torch.Tensor
    aim: Optional[torch.Tensor]
    key: torch.Tensor
    dst: torch.Tensor
    refl_sorted: torch.Tensor
    n2: int
    gbuf: torch.Tensor
    edge_rid: torch.Tensor
    edge_val: torch.Tensor


class FrozenPath:
    FROZEN_LAUE_PACKED = True        # harmonic groups: packed order + the two-call form of `cl_frozen_rows` (tests flip it to compare with the three slot launches)
    FROZEN_SORTED_ROWS = True        # monochromatic rows: sorted by reflection, `cl_frozen_rows` (round 6; tests flip it to compare with `cl_slot_rows`)

    def _frozen_layout_kw(self) -> Optional[dict]:
        """Layout time.  None unless the engine lays its observations out for a frozen scaler (the short cut is on, the scaler is frozen
        now, and the data are not deterministic-mode Laue data, which keep the fused step); else the `_build_obs` keywords that changes:
        plain rows (the scaler's output is a constant: no tile / image constraint) -- except Laue data, which keep the packed order of the
        single-pass kernels (a group inside a 16-row granule) for `cl_frozen_rows`' group sums.  `self._frozen_layout` holds the answer the
        observations were last laid out under."""
        if not self.frozen_fast or self.model.scaling_model.trainable or (self.deterministic and self.laue) or self.sprior is not None:
            return None             # (a scale prior: its KL term needs the scaler's launches around it, careless_amd/sprior.py)
        return dict(pack_images=False, sort_images=False,
                    laue_single_pass=bool(self.laue and self.FROZEN_LAUE_PACKED and not getattr(self.model, "laue_two_pass", False)))

    def _frozen_form(self, obs: ObsData, injected: bool = False) -> Optional[FrozenForm]:
        """Step time.  None: the scaler trains, the short cut is off, or the sampling / likelihood kernels do not take this observation image
        as it is -- they want rows in the caller's order (not packed or sorted by image) or harmonic groups in the packed order an engine built
        around a frozen scaler keeps.  `injected`: the step brings eta or asks for ipred_out."""
        if not (self.scaler_frozen and self.frozen_fast) or obs.host_inputs is None or self.sprior is not None:
            return None
        if obs.fused_laue:
            ok = self._frozen_layout and self.FROZEN_LAUE_PACKED and not self.deterministic and obs.tile_img is None
            return FrozenForm.GROUPS if ok else None
        if obs.row_map is not None or obs.perm is not None or (self.imgl is not None and not self._frozen_layout) or (self.deterministic and obs.laue):
            return None
        # (injected noise on rows that are not a contiguous range: the slot kernels index it by local row)
        keyed = injected and (obs.rows is not None or obs.row_index is not None)
        if obs.harmonic_id is None and not self.deterministic and self.FROZEN_SORTED_ROWS and not keyed:
            return FrozenForm.SORTED_ROWS
        return FrozenForm.SLOTS

    def _data_term_frozen(self, form: FrozenForm, obs: ObsData, step: int, eta, ipred_out, st):
        """The data term of one `ObsData` in the form `_frozen_form` answered."""
        if form is FrozenForm.GROUPS:
            self._frozen_laue(obs, step, eta, ipred_out, st)
        elif form is FrozenForm.SORTED_ROWS:
            self._frozen_rows(obs, step, eta, ipred_out, st)
        else:
            self._frozen_slots(obs)
            self._slot_likelihood(self._mlp_args(step, eta, ipred_out, obs), obs, step, eta, ipred_out, st, frozen=True)

    def _frozen_locsig(self, obs: ObsData):
        """(loc, sigma) of every row of `obs` in the caller's order, taken once per `train_model` call whichever forms its steps take."""
        fz = obs.frozen_sorted
        if fz is not None and fz.epoch == self._frozen_epoch:
            return fz.rows_loc, fz.rows_sigma
        if obs.locsig_epoch == self._frozen_epoch:
            return obs.laue_loc, obs.laue_sig
        from careless_amd.engine import scaler_forward
        sl = obs.rows if obs.rows is not None else slice(obs.start, obs.start + obs.N)
        md = _np(BaseModel.get_metadata(obs.host_inputs))
        md = md.reshape(md.shape[0], -1)[sl]
        ids = _np(BaseModel.get_image_id(obs.host_inputs)).reshape(-1)[sl] if self.imgl is not None else None
        return scaler_forward(self.mlp, md, self.imgl, ids)

    def _row_index(self, obs: ObsData) -> Optional[torch.Tensor]:
        """The global row of every stored row on the device (int64); None: rows start .. start + N - 1."""
        if obs.row_index is not None or obs.rows is None:
            return obs.row_index
        return torch.as_tensor(np.asarray(obs.rows, dtype=np.int64), device=self.device)

    def _frozen_slots(self, obs: ObsData):
        """The slot form's state: what `_slot_args` reads from `obs` -- (loc, sigma) of this `train_model` call, the noise key of every row,
        and the two buffers the entry points want a pointer for (nobody takes dL/d(loc, sigma) of a frozen scaler; rows that are their own
        slot never touch iconv)."""
        if obs.locsig_epoch != self._frozen_epoch:
            obs.laue_loc, obs.laue_sig = self._frozen_locsig(obs)
            obs.locsig_epoch = self._frozen_epoch
        obs.row_index = self._row_index(obs)
        if obs.laue_dO is None:
            obs.laue_dO = torch.empty(obs.N * 2, dtype=torch.float32, device=self.device)
        if obs.laue_iconv is None:
            obs.laue_iconv = torch.empty(obs.N * self.S if obs.harmonic_id is not None else 4, dtype=torch.float32, device=self.device)

    def _row_image_scales(self, image_id: torch.Tensor) -> Optional[torch.Tensor]:
        """The image scale of every row of `image_id` (image 0 is pinned to 1: image.py:23-25); None without image scales."""
        lay = self.layout
        if lay.n_img <= 0:
            return None
        scales = torch.cat([torch.ones(1, dtype=torch.float32, device=self.device), self.params[lay.off_img: lay.off_img + lay.n_img].detach()])
        return scales.index_select(0, image_id)

    def _edge_buffers(self, n: int):
        """(edge_rid, edge_val) of a `cl_frozen_rows` launch over n sorted rows, at the sizes the header documents: both forms that write
        edges (ROWS, SUMS) stay inside 2 * ceil(n / 64) ints and `cl_frozen_edge_floats` floats (tests/test_rows_kernels_gpu.py runs them on
        guarded workspaces of exactly these sizes)"""
        return (torch.empty(2 * ((n + 63) // 64), dtype=torch.int32, device=self.device),
                torch.empty(max(int(self.lib.cl_frozen_edge_floats(n, self.S)), 1), dtype=torch.float32, device=self.device))

    def _sorted_rows(self, obs: ObsData) -> SortedRows:
        """`obs.frozen_sorted` of the sorted-rows form, built once per `train_model` call: the rows sorted by reflection -- the scaler's
        output is a constant, so no layout constraint binds their order -- with (loc, sigma), the image scale and the global row number
        (the noise key) of every row beside them."""
        fz = obs.frozen_sorted
        if fz is None or fz.epoch != self._frozen_epoch:
            loc, sigma = self._frozen_locsig(obs)
            rid = obs.refl_id[: obs.N]
            ri = self._row_index(obs)
            order, key = sorted_row_order(rid, obs.start, None if ri is None else ri[: obs.N])
            take = lambda t: t[: obs.N].index_select(0, order).contiguous()
            aim = self._row_image_scales(obs.image_id[: obs.N].long())
            fz = obs.frozen_sorted = SortedRows(self._frozen_epoch, loc, sigma, take(rid).to(torch.int32), take(loc), take(sigma),
                                                None if aim is None else take(aim), take(obs.iobs), take(obs.sig), key, *self._edge_buffers(obs.N))
        return fz

    def _group_rows(self, obs: ObsData) -> GroupRows:
        """`obs.frozen_sorted` of the harmonic-group form, built once per `train_model` call.  The first call writes a row's gradients at its
        position in reflection order (`dst`: a 4 S-byte store per row), the second reads them front to back."""
        fz = obs.frozen_sorted
        if fz is None or fz.epoch != self._frozen_epoch:
            loc, sigma = self._frozen_locsig(obs)
            rmc, key, _, dst, refl_sorted, n2 = group_row_order(obs.refl_id, obs.row_map, obs.start, obs.noise_row)
            fz = obs.frozen_sorted = GroupRows(self._frozen_epoch, loc, sigma, loc.index_select(0, rmc).contiguous(), sigma.index_select(0, rmc).contiguous(),
                                               self._row_image_scales(obs.image_id.long().clamp(min=0)), key, dst, refl_sorted, n2,
                                               torch.zeros(max(n2, 1) * self.S, dtype=torch.float32, device=self.device), *self._edge_buffers(n2))
        return fz

    def _frozen_args(self, fz, obs: ObsData, step: int, eta, ipred_out) -> FrozenArgs:
        """What the row-per-thread launches of `cl_frozen_rows` share: (loc, sigma), image scale and noise key of every row from the
        record `fz`, the step's constants, the set's rows of eta / ipred_out.  The caller adds the row arrays, `n` and the fields of
        its form (`edge_*` and `accumulate`, or `gmeta` / `gbuf` / `src`)."""
        fa = self._step_fields(FrozenArgs(), obs, step)
        fa.loc, fa.sigma, fa.aim, fa.key = ptr(fz.loc), ptr(fz.sigma), ptr(fz.aim), ptr(fz.key)
        fa.obs_offset = int(obs.start)
        fa.eta, fa.ipred_out = self._shard_rows(obs, eta), self._shard_rows(obs, ipred_out)
        return fa

    def _frozen_rows(self, obs: ObsData, step: int, eta, ipred_out, st):
        """Monochromatic rows (round 6, `cl_frozen_rows`): per step one row-per-thread launch over the sorted rows that sums the amplitude
        gradients of a reflection's rows inside the wave and stores them (no float atomics into dz_f), plus the small launch for the runs
        that cross a wave border.  The image scales are part of the frozen scaling model: their gradient is not computed either."""
        fz = self._sorted_rows(obs)
        fa = self._frozen_args(fz, obs, step, eta, ipred_out)
        fa.refl_id, fa.iobs, fa.sig, fa.n = ptr(fz.refl), ptr(fz.iobs), ptr(self._sig(obs, fz.sig)), int(obs.N)
        # (several launches into one dz_f -- the pieces of a chunked shard -- and the double-Wilson prior, whose dlog p / dz is in dz_f
        #  before the data term: add with atomics instead of storing)
        fa.accumulate = 1 if (obs.is_piece or self.double_wilson) else 0
        fa.edge_rid, fa.edge_val = ptr(fz.edge_rid), ptr(fz.edge_val)
        check(self.lib.cl_frozen_rows(C.byref(fa), st), "cl_frozen_rows")

    def _frozen_laue(self, obs: ObsData, step: int, eta, ipred_out, st):
        """Harmonic groups (round 6): `cl_frozen_rows` twice -- in the packed order of the single-pass kernels the group sums, the
        likelihood and every row's amplitude gradient (stored per row: the rows of a group belong to different reflections), then the same
        rows in reflection order, gathered and summed per reflection like monochromatic rows -- and the padded slots' constant."""
        if obs.noise_row is not None and (eta is not None or ipred_out is not None):
            raise NotImplementedError("injected noise / ipred_out on a shard of harmonic groups behind a frozen scaler (a parity-test input: "
                                      "set model.frozen_scaler_fast_path = False)")
        fz = self._group_rows(obs)
        fa = self._frozen_args(fz, obs, step, eta, ipred_out)
        fa.refl_id, fa.iobs, fa.sig, fa.n = ptr(obs.refl_id), ptr(obs.iobs), ptr(obs.sig), int(obs.n_pad)
        fa.gmeta, fa.gbuf, fa.src = ptr(obs.gmeta), ptr(fz.gbuf), ptr(fz.dst)
        check(self.lib.cl_frozen_rows(C.byref(fa), st), "cl_frozen_rows (harmonic groups)")
        if fz.n2 > 0:               # (the second call reads the first one's gradients and nothing else of the step: a handful of fields)
            fb = FrozenArgs()
            fb.refl_id, fb.gbuf = ptr(fz.refl_sorted), ptr(fz.gbuf)
            fb.n, fb.R, fb.S = fz.n2, self.R, self.S
            fb.dz_f, fb.stop_flag = ptr(self.dz_f), ptr(self.stop_flag)
            fb.accumulate = 1 if (obs.is_piece or self.double_wilson) else 0
            fb.edge_rid, fb.edge_val = ptr(fz.edge_rid), ptr(fz.edge_val)
            check(self.lib.cl_frozen_rows(C.byref(fb), st), "cl_frozen_rows (per-reflection sums)")
        self._laue_pad_slots(fa, obs, st)
