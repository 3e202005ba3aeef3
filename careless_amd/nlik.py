"""The neural likelihood (`NeuralNormalLikelihood`: an error model learned from the data; csrc/elbo_nlik.hip), as a mixin of `ElboEngine`
(split out of careless_amd/engine.py).  Its network runs over ALL rows of an observation set in front of the data term (`cl_nlik_forward`:
the mean of delta couples the rows, also where `ObsChunks` cuts the set into pieces) and takes its gradient from the step's predictions
behind it (`cl_nlik_backward`); in between every data-term launch reads this step's sigpred where it would read SigIobs.

What the module owns: the per-set buffers (`NlikBuffers`), the order in which sigpred is handed to each piece's launch (`_nlik_image`:
the layout's own order, or a frozen scaler's rows sorted by reflection), and THE hand-over itself (`_sig`).  Whether a likelihood is a
neural one and what the engine refuses it on is decided before (`plan.check_neural_likelihood`); `ElboEngine._data_term` places the two
launches around the pieces' data terms.
Reads of the engine: `device, lib, lik, neural, S, stop_flag, _frozen_epoch`, `_param_ptr`, `_grad_ptr`, `_w_ll`, `_frozen_form`,
`_sorted_rows`.
Attaches: `obs.nlik` on the set (`ObsData` or `ObsChunks`), `sig_now` on each of its pieces.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from itertools import accumulate
from typing import Optional

import numpy as np
import torch

from careless_amd._lib import NlikArgs, check, ptr
from careless_amd.frozen import FrozenForm
from careless_amd.models.base import BaseModel
from careless_amd.obs import TILE, ObsChunks, ObsData, _np


@dataclass
class NlikBuffers:
    """A neural likelihood, per observation set (`ObsData.nlik` / `ObsChunks.nlik`, `NlikPath._nlik_attach`): the set's rows in the
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


class NlikPath:
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
