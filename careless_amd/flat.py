"""The flat fp32 vector that holds every trainable float of an engine, and the step workspace beside it (split out of
careless_amd/engine.py).  Host logic: nothing here asks for a device or the library.

What the module decides: the storage order of the parameter groups (`FLAT_GROUPS`, `FlatLayout.groups`), the tensor boundaries inside them
for per-tensor clipping and `--freeze-*` (`make_layout`), how the plugin objects are bound to and split out of such a vector (`bind_flat`,
`split_flat`), and the offsets of the step workspace (`carve_workspace`).  `ElboEngine._bind_parameters` / `_build_workspace` allocate
what is laid out here; the module reads no engine attribute and attaches nothing to an `ObsData`.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import cached_property
from itertools import accumulate
from typing import Dict, List, Optional, Tuple

import torch

from careless_amd.models.scaling.image import image_layer_layout
from careless_amd.models.scaling.nn import dense_slices

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
