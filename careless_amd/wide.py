"""Scalers wider than the fused kernels hold (hidden or metadata width > 64, or more hidden layers with per-image layers than one
fused launch takes): the layer-by-layer path of the engine on the GEMM kernels of csrc/wide_gemm.hip, as a mixin of `ElboEngine`
(split out of careless_amd/engine.py in round 4).  Reference: `MetadataScaler.call` (careless/models/scaling/nn.py:55-68, 92-120),
`ImageLayer` (scaling/image.py:66-125) and the tape gradient of both (models/merging/variational.py:197-202).
Defined elsewhere and used here: the likelihood between the forward and the backward pass is `SlotPath._slot_likelihood` / `_slot_args`
(careless_amd/slots.py) on (loc, sigma) per row; `_mlp_args` (fused.py) supplies the image-scale fields; `_param_ptr` / `_grad_ptr` (engine.py).
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

from careless_amd._lib import check, ptr
from careless_amd.models.scaling.image import image_layer_layout
from careless_amd.models.scaling.nn import dense_layout
from careless_amd.obs import ObsData


def image_tiles(rel_seg: np.ndarray, device) -> torch.Tensor:
    """(group, first row) pairs covering every group's rows in 128-row pieces: the x-blocks of cl_wide_image_forward_tiles /
    _dgrad_tiles (per-image layers wider than 128).  `rel_seg` = the groups' row starts relative to the call's first row."""
    rel = np.asarray(rel_seg, dtype=np.int64)
    n = np.maximum(0, -(-(rel[1:] - rel[:-1]) // 128))                      # pieces per group
    g = np.repeat(np.arange(len(n)), n)
    first = np.repeat(np.concatenate([[0], np.cumsum(n)[:-1]]), n)
    row = rel[:-1][g] + 128 * (np.arange(int(n.sum())) - first)
    return torch.as_tensor(np.stack([g, row], axis=1).astype(np.int32).reshape(-1), device=device)


# The Dense(2) head of one row chunk, for the top layer's epilogue: the head's offset in the scaler's flat layout, the device pointers of the
# chunk's loc / sigma rows and of its d sigma / d raw rows (None unless the head's backward pass is fused into the top layer's backward)
WideHead = namedtuple("WideHead", "off loc sig dsd")
# A scaler as the layer-by-layer launches see it: d columns, L Dense layers of width w, K per-image layers over M images, LeakyReLU slope
WideShape = namedtuple("WideShape", "d w L K M leak")
# One row chunk [a, b): its first image and the device array of its images' row starts relative to a (0, None without per-image layers)
RowChunk = namedtuple("RowChunk", "a b m0 seg")


def image_chunks(img_seg, chunk: int):
    """Whole images per row chunk: [(a, b, first image, row starts of the chunk's images relative to a)] from `img_seg`, the first row of
    every image of rows sorted by image.  Images are taken while they fit `chunk` rows; an image longer than that gets a chunk of its
    own; empty images in front of a chunk are skipped (those inside or behind one ride along as empty groups)."""
    seg, M = np.asarray(img_seg, dtype=np.int64), len(img_seg) - 1
    out, m0 = [], 0
    while m0 < M:
        m1 = m0 + 1
        while m1 < M and seg[m1 + 1] - seg[m0] <= chunk:
            m1 += 1
        if seg[m1] > seg[m0]:
            out.append((int(seg[m0]), int(seg[m1]), m0, (seg[m0:m1 + 1] - seg[m0]).astype(np.int32)))
        m0 = m1
    return out


def row_chunks(N: int, img_seg, chunk: int, w: int, device):
    """The `RowChunk`s of N rows for the layer-by-layer launches -- `chunk` rows each, or whole images (`image_chunks`) when `img_seg` is
    given --, the tile list of every chunk by its first row (`image_tiles`, made here, once: per-image layers wider than 128; else None),
    and the rows the work buffers need: `chunk`, or the longest chunk of whole images."""
    if img_seg is None:
        return [RowChunk(a, min(N, a + chunk), 0, None) for a in range(0, N, chunk)], None, chunk
    walk = image_chunks(img_seg, chunk)
    tiles = {a: image_tiles(rel, device) for a, _, _, rel in walk} if w > 128 else None
    return [RowChunk(a, b, m0, torch.as_tensor(rel, device=device)) for a, b, m0, rel in walk], tiles, max(b - a for a, b, _, _ in walk)


def imgl_ptrs(base: int, sh: WideShape, k: int, m0: int):
    """Device pointers of (kernel, bias) of image m0 in per-image layer k of the per-image block at `base` (parameters or gradients)."""
    ow, ob = image_layer_layout(sh.K, sh.M, sh.w)[0][k]
    return base + 4 * (ow + m0 * sh.w * sh.w), base + 4 * (ob + m0 * sh.w)


def hidden_forward(lib, pmlp: int, pimgl, sh: WideShape, src, dsts, ldw: int, ch: RowChunk, tiles, sf, st, layers=None):
    """The unfused hidden-layer launches of one row chunk, the one place that issues them: of the L + K hidden layers those in `layers` (a
    range; default all) -- a Dense layer through cl_wide_dense_forward, a per-image layer (image.py:116-125) through cl_wide_image_forward,
    or _tiles above width 128.  `pmlp` / `pimgl`: device pointers of the scaler's flat parameters and of its per-image block; `src`: the
    (pointer, ld) of the first of these layers' input; `dsts[l]`: where layer l's output goes (row pitch `ldw`); `tiles`: the chunk's tile
    list; `sf`: the stop flag.
    Returns the (pointer, ld) of every output."""
    dense, n, hs = dense_layout(sh.d, sh.w, sh.L)[0], ch.b - ch.a, [src]
    for l in (range(sh.L + sh.K) if layers is None else layers):
        if l < sh.L:
            ow, ob, fan_in = dense[l]
            check(lib.cl_wide_dense_forward(*hs[-1], pmlp + 4 * ow, pmlp + 4 * ob, n, fan_in, sh.w, sh.leak, 1, dsts[l], ldw, sf, st), "cl_wide_dense_forward")
        elif sh.w > 128:                # wider than the grouped streaming kernel holds: the tiled kernel over the chunk's list of row pieces
            check(lib.cl_wide_image_forward_tiles(*hs[-1], *imgl_ptrs(pimgl, sh, l - sh.L, ch.m0), ptr(ch.seg), ptr(tiles), tiles.numel() // 2,
                                                  sh.w, sh.leak, dsts[l], ldw, sf, st), "cl_wide_image_forward_tiles")
        else:
            check(lib.cl_wide_image_forward(*hs[-1], *imgl_ptrs(pimgl, sh, l - sh.L, ch.m0), ptr(ch.seg), ch.seg.numel() - 1, n, sh.w, sh.leak,
                                            dsts[l], ldw, sf, st), "cl_wide_image_forward")
        hs.append((dsts[l], ldw))
    return hs[1:]


@dataclass
class WideBuffers:
    """Work buffers of the layer-by-layer path, per engine (`WidePath._wide_setup`; the row buffers by `_wide_buffers`)."""
    ldw: int                                        # row pitch of a hidden layer's activations
    chunk: int                                      # rows of a chunk
    nh: int                                         # hidden layers, Dense + per-image
    rows: int = 0                                   # rows the buffers below hold
    acts: List[torch.Tensor] = field(default_factory=list)      # one activation buffer per hidden layer (two at least)
    dz: List[torch.Tensor] = field(default_factory=list)        # two alternating gradient buffers
    nsplit: int = 0                                 # weight-gradient partials of `rows` rows
    nblk: int = 0                                   # ... of the head's backward pass
    wpart: Optional[torch.Tensor] = None
    hpart: Optional[torch.Tensor] = None


class WidePath:
    # -- scalers wider than 64 ---------------------------------------------------------------------------------------------
    WIDE_BUDGET = 4 << 30     # bytes of activation storage a row chunk may take ((L + 2) buffers of chunk x ld floats), and never more
                              # than a quarter of the free device memory: longer chunks = fewer launches and a better-balanced last round of row blocks

    def _wide_setup(self):
        """Work buffers of the unfused path (csrc/wide_gemm.hip): one activation buffer per hidden layer (Dense + per-image) + two
        gradient buffers of `chunk` rows, the per-layer weight-gradient partials.  The chunk is sized from the layer count and
        width so the buffers stay inside WIDE_BUDGET (and, with it, inside the device memory next to the shard)."""
        if self._wide is not None:
            return self._wide
        lib, dev = self.lib, self.device
        ldw = int(lib.cl_wide_ld(self.w))
        nh = self.L + (self.imgl.n_image_layers if self.imgl is not None else 0)
        per_row = 4 * (nh + 2) * ldw
        free = torch.cuda.mem_get_info(dev)[0]
        budget = min(self.WIDE_BUDGET, max(free // 4, 64 << 20))
        chunk = max(128, min(budget // per_row, 1 << 21) // 128 * 128)
        self._wide = WideBuffers(ldw=ldw, chunk=chunk, nh=nh)
        self._wide_buffers(chunk)
        return self._wide

    def _wide_buffers(self, rows: int):
        """(Re)allocate the row buffers for chunks of up to `rows` rows (an image larger than the default chunk needs its own size)."""
        W, lib, dev = self._wide, self.lib, self.device
        if rows <= W.rows:
            return
        ldw = W.ldw
        W.acts = [torch.zeros(rows * ldw, dtype=torch.float32, device=dev) for _ in range(max(2, W.nh))]
        W.dz = [torch.zeros(rows * ldw, dtype=torch.float32, device=dev) for _ in range(2)]
        W.nsplit, W.nblk = int(lib.cl_wide_wgrad_splits(rows)), int(lib.cl_wide_head_blocks(rows))
        pmax = max(self.w * self.d + self.w, self.w * self.w + self.w)
        # (the fused dgrad + first-layer weight gradient writes one partial per workgroup: more of them, each smaller)
        W.wpart = torch.empty(max(W.nsplit * pmax, int(lib.cl_wide_dgrad_wgrad0_parts(rows)) * (self.w * self.d + self.w)),
                                 dtype=torch.float32, device=dev)
        W.hpart = torch.empty(W.nblk * (2 * self.w + 2), dtype=torch.float32, device=dev)
        W.rows = rows

    def _wide_chunks(self, obs: ObsData):
        """Row chunks [a, b) of `obs` for the layer-by-layer path.  With per-image layers a chunk holds whole images (their rows are
        consecutive: ObsData sort_images) and carries (first image, device array of the images' row starts relative to a)."""
        if obs.wide_chunks is not None:
            return obs.wide_chunks
        W = self._wide_setup()
        obs.wide_chunks, obs.wide_tiles, rows = row_chunks(obs.N, obs.img_seg if self.imgl is not None else None, W.chunk, self.w, self.device)
        self._wide_buffers(rows)
        return obs.wide_chunks

    def _wide_shape(self) -> WideShape:
        K, M = (self.imgl.n_image_layers, self.imgl.max_images) if self.imgl is not None else (0, 0)
        return WideShape(self.d, self.w, self.L, K, M, self.mlp.leakiness)

    def _imgl_ptrs(self, at, k: int, m0: int):
        """Device pointers of (kernel, bias) of image m0 in per-image layer k of the parameters or the gradient (`at`: `_param_ptr` / `_grad_ptr`)."""
        return imgl_ptrs(at("imgl"), self._wide_shape(), k, m0)

    WIDE_KEEP_BUDGET = 64 << 30     # bytes of activations of a whole observation set the forward pass may keep for the backward pass
    # The fusions of round 4, each with the separate launches it replaced still behind it (the fallback of shapes outside the fused
    # kernels' envelopes).  Class attributes, not environment switches: the A/Bs are closed (NOTEBOOK.md), one parity test flips them
    # to hold the fused step against the separate launches (tests/test_gpu_parity.py).
    FUSE_PRE = True          # first Dense layer recomputed instead of stored (cl_wide_dense2_forward / _dgrad_pre / _wgrad_pre)
    FUSE_WG0 = True          # first layer's weight gradient inside the second layer's dgrad (cl_wide_dense_dgrad_pre_wgrad0)
    FUSE_HEADB = True        # the Dense(2) head's backward pass inside the top layer's weight gradient and dgrad
    FUSE_LIK = True          # the slot likelihood in the top layer's forward epilogue (cl_wide_dense_forward_head_lik)

    def _wide_pre(self) -> bool:
        """The first Dense layer is recomputed instead of stored (cl_wide_dense2_forward / _dgrad_pre / _wgrad_pre): at least two Dense
        layers, at most 15 metadata columns, hidden width up to 128."""
        return self.FUSE_PRE and self.L >= 2 and bool(self.lib.cl_wide_pre_supported(self.d, self.w))

    def _wide_head_bwd(self) -> bool:
        """The Dense(2) head's backward pass runs inside the top Dense layer's weight gradient and dgrad (cl_wide_dense_wgrad_head /
        _dgrad_head) instead of a launch of its own that writes dZ_L: Dense-only scalers whose top layer is a square one of the streaming
        kernel's widths and not the layer fed by the recomputed first one."""
        return (self.FUSE_HEADB and self.imgl is None and self.L >= 2 and not (self._wide_pre() and self.L == 2) and
                bool(self.lib.cl_wide_head_bwd_supported(self.w, self.w)))

    def _wide_keep_all(self, obs: ObsData):
        """Per-layer activation buffers over ALL rows of `obs` (list of tensors), or None when they do not fit: then the backward pass
        recomputes each chunk's forward into the chunk-sized buffers."""
        W = self._wide_setup()
        need = 4 * (W.nh - (1 if self._wide_pre() else 0)) * W.ldw * obs.N
        if obs.wide_full is not None:
            return obs.wide_full
        free = torch.cuda.mem_get_info(self.device)[0]
        if need > min(self.WIDE_KEEP_BUDGET, free // 4):
            return None
        # (with the first layer recomputed its output has no buffer)
        obs.wide_full = [None if (l == 0 and self._wide_pre()) else torch.zeros(obs.N * W.ldw, dtype=torch.float32, device=self.device)
                         for l in range(W.nh)]
        return obs.wide_full

    def _wide_forward(self, obs: ObsData, chunk, keep: bool, st, full=None, head=None, lik=None):
        """Hidden layers on one row chunk of `obs`: layer l's output lands in acts[l] when `keep` (else two buffers alternate), or
        in the chunk's rows of the whole-set buffers `full`.  Returns the (buffer, ld) pairs of h_0 .. h_(L + K), whether `head` (a WideHead)
        rode in the top layer's epilogue and whether the slot likelihood `lik` did too."""
        a, n = chunk.a, chunk.b - chunk.a
        lib, W, sh = self.lib, self._wide_setup(), self._wide_shape()
        ldw, base = W.ldw, self._param_ptr("mlp")
        layers, _ = dense_layout(self.d, self.w, self.L)
        sf, leak = ptr(self.stop_flag), self.mlp.leakiness
        dsts = [None if t is None else t.data_ptr() + 4 * a * ldw for t in full] if full is not None else \
            [W.acts[l if keep else l & 1].data_ptr() for l in range(self.L + sh.K)]
        unfused = lambda src, l0, l1: hidden_forward(lib, base, self._param_ptr("imgl"), sh, src, dsts, ldw, chunk, obs.wide_tiles and obs.wide_tiles[a],
                                                     sf, st, range(l0, l1))
        hs = [(obs.meta_rm.data_ptr() + 4 * a * obs.meta_ld, obs.meta_ld)]
        head_fused = lik_fused = False
        first = 0
        if self._wide_pre():
            # h_0 is never stored: layer 1's launch makes it from the metadata
            (ow0, ob0, d0), (ow, ob, _), first = layers[0], layers[1], 2
            head_fused = head is not None and self.L == 2 and self.imgl is None
            hd = head if head_fused else WideHead(0, None, None, None)
            check(lib.cl_wide_dense2_forward(*hs[0], d0, base + 4 * ow0, base + 4 * ob0, base + 4 * ow, base + 4 * ob, n, self.w, self.w,
                                             leak, dsts[1], ldw, (base + 4 * hd.off) if head_fused else None, self.bij_kind, self.mlp.epsilon,
                                             hd.loc, hd.sig, sf, st), "cl_wide_dense2_forward")
            hs += [(None, ldw), (dsts[1], ldw)]
        ow, ob, fan_in = layers[-1]
        if not (head is not None and self.L > first and self.imgl is None and fan_in <= 128 and self.w <= 128):
            return hs + unfused(hs[-1], first, self.L + sh.K), head_fused, lik_fused
        # the top layer carries the Dense(2) head in its epilogue: (loc, sigma) come out of the same pass
        hs += unfused(hs[-1], first, self.L - 1)
        top = (*hs[-1], base + 4 * ow, base + 4 * ob, n, fan_in, self.w, leak, dsts[self.L - 1], ldw,
               base + 4 * head.off, self.bij_kind, self.mlp.epsilon, head.loc, head.sig, head.dsd)
        rc = -2
        if lik is not None:
            # ... and the slot likelihood of the chunk's rows too: (loc, sigma) never wait in memory for a launch of their own
            rc = lib.cl_wide_dense_forward_head_lik(*top, C.byref(lik), sf, st)
            if rc != -2:
                check(rc, "cl_wide_dense_forward_head_lik")
                lik_fused = True
        if rc == -2:
            check(lib.cl_wide_dense_forward_head(*top, sf, st), "cl_wide_dense_forward_head")
        return hs + [(dsts[self.L - 1], ldw)], True, lik_fused

    def _data_term_wide(self, obs: ObsData, step: int, eta, ipred_out, st):
        """Hidden / metadata width > 64 (or more hidden layers with per-image layers than one fused launch holds): unfused scaler on
        the GEMM kernels of csrc/wide_gemm.hip.  Forward (row chunks; the top layer carries the Dense(2) head) -> (loc, sigma) per row ->
        the slot likelihood (one launch when every row is its own slot, the three Laue launches otherwise) -> dL/d(loc, sigma) -> per
        chunk: forward again unless the activations were kept, then _wide_backward_chunk.  6 (activations kept) or 8 P_mm flops per
        observation; every product in exact fp32."""
        lib = self.lib
        chunks = self._wide_chunks(obs)
        ma = self._mlp_args(step, eta, ipred_out, obs)
        _, off_head = dense_layout(self.d, self.w, self.L)
        pbase = self._param_ptr("mlp")
        # The activations of ALL rows are kept by the forward pass when they fit (WIDE_KEEP_BUDGET, a quarter of the free memory at
        # most: 15 GB for 10 M rows of a 3 x 128 scaler on a 288-GB device) and the backward pass starts from them -- 6 P_mm flops per
        # observation.  Otherwise the buffers hold one chunk at a time and each chunk's forward is recomputed when its turn in the
        # backward pass comes (8 P_mm).
        full = self._wide_keep_all(obs)
        kept, lik_fused = [], []
        headb = self._wide_head_bwd()
        if headb and obs.wide_dsd is None:
            obs.wide_dsd = torch.empty(obs.N, dtype=torch.float32, device=self.device)
        # The slot likelihood rides in the top layer's forward epilogue when a production step asks for nothing else of it (rows that are
        # their own slot, in-kernel noise, no predictions out, no Evans-2011 terms, not the deterministic mode); the library decides by
        # shape (-2), the same for every chunk
        want_lik = (self.FUSE_LIK and obs.harmonic_id is None and eta is None and ipred_out is None and not self.ev11 and not self.deterministic)
        for ch in chunks:
            a, b = ch.a, ch.b
            loc, sig = obs.laue_loc.data_ptr() + 4 * a, obs.laue_sig.data_ptr() + 4 * a
            head = WideHead(off_head, loc, sig, obs.wide_dsd.data_ptr() + 4 * a if headb else None)
            lik = self._slot_args(ma, obs, step, None, None, a, b - a) if want_lik else None
            hs, head_fused, lf = self._wide_forward(obs, ch, full is not None, st, full=full, head=head, lik=lik)
            kept.append(hs)
            lik_fused.append(lf)
            if not head_fused:
                check(lib.cl_wide_head_forward(*hs[-1], pbase + 4 * off_head, b - a, self.w, self.bij_kind, self.mlp.epsilon, loc, sig,
                                               ptr(self.stop_flag), st), "cl_wide_head_forward")
        if not all(lik_fused):
            assert not any(lik_fused)
            self._slot_likelihood(ma, obs, step, eta, ipred_out, st)
        for ic, ch in enumerate(chunks):
            self._wide_backward_chunk(obs, ch, kept[ic] if full is not None else self._wide_forward(obs, ch, True, st)[0], headb, st)

    def _wide_backward_chunk(self, obs: ObsData, chunk, hs, headb: bool, st):
        """The backward pass of one row chunk from its activations `hs` (_wide_forward) and the rows' dL/d(loc, sigma): the head's backward
        pass inside the top Dense layer's weight gradient and dgrad (`headb`; its own launch outside their envelope), then weight gradient
        and dgrad layer by layer, top down -- the per-image layers, then the Dense layers, the first one's weight gradient inside the
        second one's dgrad when the first layer is recomputed."""
        a, b, m0, seg = chunk
        n = b - a
        lib, W = self.lib, self._wide_setup()
        layers, off_head = dense_layout(self.d, self.w, self.L)
        pbase, gbase = self._param_ptr("mlp"), self._grad_ptr("mlp")
        sf, leak, w, ldw = ptr(self.stop_flag), self.mlp.leakiness, self.w, W.ldw
        dz, dzn = W.dz
        nsplit = min(W.nsplit, int(lib.cl_wide_wgrad_splits(n)))

        def reduce(parts, nparts, size, off):
            check(lib.cl_reduce_partials(ptr(parts), nparts, size, gbase + 4 * off, sf, st), "cl_reduce_partials")

        if headb:
            # the head's backward pass rides on the top layer's two backward kernels: dZ_L is made from h_L where they read it
            l = self.L - 1
            ow, ob, fan_in = layers[l]
            hd = (*hs[-1], pbase + 4 * off_head, obs.laue_dO.data_ptr() + 8 * a, obs.wide_dsd.data_ptr() + 4 * a)
            check(lib.cl_wide_dense_wgrad_head(*hd, leak, *hs[l], n, w, fan_in, ptr(W.wpart), ptr(W.hpart), nsplit, sf, st), "cl_wide_dense_wgrad_head")
            reduce(W.wpart, nsplit, w * fan_in + w, ow)
            reduce(W.hpart, nsplit, 2 * w + 2, off_head)
            check(lib.cl_wide_dense_dgrad_head(*hd, pbase + 4 * ow, n, w, fan_in, *hs[l], leak, ptr(dz), ldw, sf, st), "cl_wide_dense_dgrad_head")
        else:
            nblk = min(W.nblk, int(lib.cl_wide_head_blocks(n)))
            check(lib.cl_wide_head_backward(*hs[-1], pbase + 4 * off_head, obs.laue_dO.data_ptr() + 8 * a, n, w, self.bij_kind,
                                            self.mlp.epsilon, leak, ptr(dz), ldw, ptr(W.hpart), nblk, sf, st), "cl_wide_head_backward")
            reduce(W.hpart, nblk, 2 * w + 2, off_head)
        K = self.imgl.n_image_layers if self.imgl is not None else 0
        for k in range(K - 1, -1, -1):          # per-image layers: each image's gradient is written once (its rows sit in one chunk)
            l = self.L + k
            gw, gb = self._imgl_ptrs(self._grad_ptr, k, m0)
            wk, _ = self._imgl_ptrs(self._param_ptr, k, m0)
            check(lib.cl_wide_image_wgrad(ptr(dz), ldw, *hs[l], ptr(seg), seg.numel() - 1, n, w, gw, gb, sf, st), "cl_wide_image_wgrad")
            if w > 128:
                tl = obs.wide_tiles[a]
                check(lib.cl_wide_image_dgrad_tiles(ptr(dz), ldw, wk, ptr(seg), ptr(tl), tl.numel() // 2, w, *hs[l], leak, ptr(dzn), ldw, sf, st),
                      "cl_wide_image_dgrad_tiles")
            else:
                check(lib.cl_wide_image_dgrad(ptr(dz), ldw, wk, ptr(seg), seg.numel() - 1, n, w, *hs[l], leak, ptr(dzn), ldw, sf, st), "cl_wide_image_dgrad")
            dz, dzn = dzn, dz
        pre = self._wide_pre()
        for l in range(self.L - (2 if headb else 1), -1, -1):
            ow, ob, fan_in = layers[l]
            if pre and l == 1:
                # the layer's input h_0 is recomputed from the metadata: as the weight gradient's operand and as the dgrad's mask
                ow0, ob0, d0 = layers[0]
                x0 = (*hs[0], d0, pbase + 4 * ow0, pbase + 4 * ob0)
                check(lib.cl_wide_dense_wgrad_pre(ptr(dz), ldw, *x0, leak, n, w, fan_in, ptr(W.wpart), nsplit, sf, st), "cl_wide_dense_wgrad_pre")
                reduce(W.wpart, nsplit, w * fan_in + w, ow)
                # layer 1's dgrad with layer 0's weight gradient taken where dZ_0 is produced (it is never stored) ...
                rc = -2 if not self.FUSE_WG0 else \
                    lib.cl_wide_dense_dgrad_pre_wgrad0(ptr(dz), ldw, pbase + 4 * ow, n, w, fan_in, *x0, leak, ptr(W.wpart), sf, st)
                if rc != -2:
                    check(rc, "cl_wide_dense_dgrad_pre_wgrad0")
                    reduce(W.wpart, int(lib.cl_wide_dgrad_wgrad0_parts(n)), w * d0 + w, ow0)
                    break
                # ... or, outside that kernel's envelope, the two launches
                check(lib.cl_wide_dense_dgrad_pre(ptr(dz), ldw, pbase + 4 * ow, n, w, fan_in, *x0, leak, ptr(dzn), ldw, sf, st), "cl_wide_dense_dgrad_pre")
                dz, dzn = dzn, dz
                continue
            check(lib.cl_wide_dense_wgrad(ptr(dz), ldw, *hs[l], n, w, fan_in, ptr(W.wpart), nsplit, sf, st), "cl_wide_dense_wgrad")
            reduce(W.wpart, nsplit, w * fan_in + w, ow)
            if l > 0:
                check(lib.cl_wide_dense_dgrad(ptr(dz), ldw, pbase + 4 * ow, n, w, fan_in, *hs[l], leak, ptr(dzn), ldw, sf, st), "cl_wide_dense_dgrad")
                dz, dzn = dzn, dz

