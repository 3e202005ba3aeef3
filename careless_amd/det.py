"""Deterministic mode (`model.deterministic = True` / CARELESS_HIP_DETERMINISTIC=1; csrc/elbo_det.hip), as a mixin of `ElboEngine` (split out
of careless_amd/engine.py): no float atomics in the data term -- every launch stores per observation and per workgroup, `cl_det_reduce`
sums the stores in a fixed order once per observation set.

What the module owns: the per-observation-set buffers (`DetBuffers`), where each launch of a set stores inside them (`_det_parts`), and
the closing reduction (`_det_reduce`).  Whether the mode is on and what it refuses is decided before (`plan.check_deterministic`,
`ElboEngine._read_plugins`); the launches fill their `dzf_obs / dimg_obs / det_slot / nll_part / ev11_part` fields themselves (`_mlp_args`,
`_slot_likelihood`, `_laue_pad_slots`) from what is attached here.
Reads of the engine: `device, lib, R, S, laue, wide, ev11, sprior, layout, dz_f, scalars, stop_flag`, `_max_images`, `_grad_ptr`.
Attaches: `obs.det` on the set (`ObsData` or `ObsChunks`), `det_parent` / `det_index` on each of its pieces.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from careless_amd import _lib
from careless_amd._lib import DetArgs, check, ptr
from careless_amd.obs import ObsData


@dataclass
class DetBuffers:
    """Deterministic mode, per observation set (`ObsData.det`, `DetPath._det_attach`): the per-observation stores of the kernels and the
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


class DetPath:
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
        # (the slot likelihood's launches: one on the whole set -- Laue, wide --, or one per piece: monochromatic rows under a scale prior)
        sprior = getattr(self, "sprior", None) is not None
        slot_launches = len(pieces) if sprior else (1 if (self.laue or self.wide) else 0)
        obs.det = DetBuffers(slot=slot, dzf=torch.zeros(n * self.S, dtype=torch.float32, device=dev), dimg=torch.zeros(n, dtype=torch.float32, device=dev),
                             nll=torch.zeros(len(pieces) * pieces[0].grid + _lib.CL_LAUE_LIK_MAX_BLOCKS * slot_launches,
                                             dtype=torch.float64, device=dev),
                             refl=(perm_r, seg_r), img=order(img, M), M=M, pieces=len(pieces), grid=pieces[0].grid)
        if self.ev11:
            # Evans-2011 gradients: one slot of three floats per wave of every launch (the fused launches' CL_EV11_WAVES per workgroup, then
            # four per workgroup of the slot / padded-slot likelihood launch), summed in slot order by cl_det_reduce
            obs.det.ev11 = torch.zeros(3 * (_lib.CL_EV11_WAVES * len(pieces) * pieces[0].grid + 4 * _lib.CL_LAUE_LIK_MAX_BLOCKS * max(1, slot_launches)),
                                       dtype=torch.float32, device=dev)
        for k, p in enumerate(pieces):
            p.det_parent, p.det_index = obs, k

    def _det_parts(self, obs: ObsData, k: int):
        """(nll_part, ev11_part) of part k of the shard `obs` belongs to (deterministic mode): the fused launches of its pieces store into parts
        0 .. pieces - 1 -- det.grid NLL slots, CL_EV11_WAVES Evans-2011 slots of three floats per workgroup --, the slot / padded-slot
        likelihood launch behind them (k = det.pieces)."""
        det = obs.det_parent.det
        return (det.nll.data_ptr() + 8 * det.grid * k,
                det.ev11.data_ptr() + 4 * 3 * _lib.CL_EV11_WAVES * det.grid * k if self.ev11 else None)

    def _det_slot_parts(self, obs: ObsData):
        """(nll_part, ev11_part) of the slot likelihood's launch on `obs`: behind the fused launches' parts (`_det_parts(obs, det.pieces)`), and -- a
        piece of a chunked shard, which has a slot launch of its own under a scale prior -- behind the slot parts of the pieces in front of it."""
        nll, ev11 = self._det_parts(obs, obs.det_parent.det.pieces)
        k = obs.det_index if obs.is_piece else 0
        return nll + 8 * _lib.CL_LAUE_LIK_MAX_BLOCKS * k, None if ev11 is None else ev11 + 4 * 3 * 4 * _lib.CL_LAUE_LIK_MAX_BLOCKS * k

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
