"""Device images of observation sets and the data-parallel splits of the observation axis (host side, numpy + torch tensors):
`Shard` / `make_shard` / `owner_shard` / `laue_group_shard` (who takes which rows), `pack_by_image` / `pack_laue` (the packed orders
of the per-image-layer and single-pass Laue kernels), `meta_feature_major` / `meta_by_image` / `meta_row_major` / `image_order` (the
metadata images and the order by image, from plain arrays: the layouts and the forward-only scaler path share them), `select_rows` ->
`lay_out` (`layout_plain` / `_by_image` / `_laue` / `_wide` fill a host `Layout`) -> `ObsData` (one launch's arrays in HBM: selection, layout, upload), `ObsChunks` (a shard cut into several
launches), `launch_row_limit`.  Split out of careless_amd/engine.py in round 4; the engine re-exports every name.

What the arrays replace in the reference: the `inputs` tuple of `BaseModel.input_index` order (careless/models/base.py:22-121) as
`formatter.py:354-400, 599-653` builds it -- the engine narrows the ids to int32 and stores the metadata feature-major.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, NamedTuple, Optional

import numpy as np
import torch

from careless_amd import _lib
from careless_amd.models.base import BaseModel

TILE = _lib.CL_MLP_TILE


def _np(x) -> np.ndarray:
    if torch.is_tensor(x):
        return x.detach().cpu().numpy()
    return np.asarray(x)


# ------------------------------------------------------------------------------------------------------------
# data-parallel sharding of the observation axis
# ------------------------------------------------------------------------------------------------------------
@dataclass
class Shard:
    rank: int
    world: int
    start: int        # first global observation of this rank
    stop: int
    kl_begin: int     # reflections whose KL term this rank owns
    kl_end: int
    owner: bool = False          # reflection-owner sharding: the rank holds EVERY observation of reflections [kl_begin, kl_end) and
    rows: Optional[np.ndarray] = None   # nothing else (`rows`: their global row numbers, ascending); start / stop are then 0 / len(rows)


def make_shard(n_obs: int, n_refl: int, rank: int = 0, world: int = 1) -> Shard:
    """Contiguous, near-equal split of the observations; the KL over the R reflections is split the same way so it
    is counted exactly once after the gradient all-reduce."""
    if not (0 <= rank < world):
        raise ValueError(f"rank {rank} outside world of size {world}")
    from careless_amd.distributed import check_world
    check_world(n_obs, world)
    per = (n_obs + world - 1) // world
    if (world - 1) * per >= n_obs:          # ceil-sized chunks would leave the last ranks empty: floor-sized, remainder spread
        base, extra = divmod(n_obs, world)
        start = rank * base + min(rank, extra)
        stop = start + base + (1 if rank < extra else 0)
        rper = (n_refl + world - 1) // world
        return Shard(rank, world, start, stop, min(rank * rper, n_refl), min((rank + 1) * rper, n_refl))
    start, stop = min(rank * per, n_obs), min((rank + 1) * per, n_obs)
    rper = (n_refl + world - 1) // world
    return Shard(rank, world, start, stop, min(rank * rper, n_refl), min((rank + 1) * rper, n_refl))


def owner_bounds(refl_id: np.ndarray, n_refl: int, world: int) -> Optional[np.ndarray]:
    """Reflection ranges of a reflection-owner split: world + 1 boundaries in [0, n_refl] such that the ranges hold about the same
    number of OBSERVATIONS (the work) and every rank gets at least one reflection with at least one observation.  None when no such
    split exists (fewer observed reflections than ranks) -- the same answer on every rank, which then all use the row split."""
    counts = np.bincount(np.asarray(refl_id).reshape(-1).astype(np.int64), minlength=n_refl)
    cum = np.concatenate([[0], np.cumsum(counts)])
    n = int(cum[-1])
    b = np.array([int(np.searchsorted(cum, n * r / world, side="left")) for r in range(world)] + [n_refl], dtype=np.int64)
    b[0] = 0
    b = np.clip(b, 0, n_refl)
    if np.any(np.diff(b) <= 0) or np.any(np.diff(cum[b]) <= 0):
        return None
    return b


def owner_shard(refl_id: np.ndarray, n_refl: int, rank: int, world: int) -> Optional[Shard]:
    """The shard of `rank` in a reflection-owner split: reflections [r0, r1) and every observation of theirs.  All the
    terms of the loss that touch q(F_h) of an owned reflection -- its KL, its observations' likelihoods -- are then local: no other
    rank samples it, adds to its gradient or updates it, and the step's all-reduce carries the scaler's gradient only."""
    b = owner_bounds(refl_id, n_refl, world)
    if b is None:
        return None
    r0, r1 = int(b[rank]), int(b[rank + 1])
    rid = np.asarray(refl_id).reshape(-1)
    rows = np.nonzero((rid >= r0) & (rid < r1))[0]
    return Shard(rank, world, 0, int(len(rows)), r0, r1, True, rows)


def laue_group_shard(harmonic_id: np.ndarray, rank: int, world: int):
    """Laue shards must keep every harmonic group on one rank (the invariant the reference enforces for its train/test split,
    careless/io/manager.py:317-324).  Groups [g0, g1) go to `rank`, balanced by row count; the padded slots [G, N) are dealt out so
    that every rank has exactly as many slots as rows.  Returns (g0, g1, pad0, pad1)."""
    hid = np.asarray(harmonic_id).astype(np.int64)
    N = len(hid)
    G = int(hid.max()) + 1
    counts = np.bincount(hid, minlength=G)
    cum = np.concatenate([[0], np.cumsum(counts)])
    bounds = [int(np.searchsorted(cum, N * r / world, side="left")) for r in range(world)] + [G]
    bounds = np.clip(bounds, 0, G)
    if G < world or np.any(np.diff(bounds) <= 0):      # same test on every rank: all raise together, none waits in the collective
        raise ValueError(f"cannot shard {G} harmonic groups over {world} ranks: every rank needs at least one whole group")
    g0, g1 = int(bounds[rank]), int(bounds[rank + 1])
    pads = [int(cum[bounds[r + 1]] - cum[bounds[r]]) - int(bounds[r + 1] - bounds[r]) for r in range(world)]
    pad0 = G + int(sum(pads[:rank]))
    return g0, g1, pad0, pad0 + pads[rank]


# ------------------------------------------------------------------------------------------------------------
# device image of one set of observations (the training shard, or a validation set)
# ------------------------------------------------------------------------------------------------------------
def pack_by_image(image_id: np.ndarray):
    """Packed observation order of the per-image-layer kernel: rows grouped by image, every image padded to whole tiles.
    Returns (pos, n_pad, tile_img, row_map): pos[i] = packed position of row i; row_map[p] = row of packed position p or -1."""
    image_id = np.asarray(image_id).astype(np.int64)
    order = np.argsort(image_id, kind="stable")
    ids, counts = np.unique(image_id, return_counts=True)
    tiles = (counts + TILE - 1) // TILE
    base = np.concatenate([[0], np.cumsum(tiles)[:-1]]) * TILE          # first packed position of each image
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])              # first sorted row of each image
    within = np.arange(len(image_id)) - np.repeat(first, counts)
    pos = np.empty(len(image_id), dtype=np.int64)
    pos[order] = np.repeat(base, counts) + within
    n_pad = int(tiles.sum()) * TILE
    row_map = np.full(n_pad, -1, dtype=np.int32)
    row_map[pos] = np.arange(len(image_id), dtype=np.int32)
    tile_img = np.repeat(ids, tiles).astype(np.int32)
    return pos, n_pad, tile_img, row_map


GRANULE = 16      # observations of one wave of the fused kernel


def pack_laue(harmonic_id: np.ndarray, image_id: np.ndarray, by_image: bool):
    """Packed order of the single-pass Laue kernel: the rows of a harmonic group are consecutive and inside one 16-row granule.
    Groups are laid out class by class (all groups of s rows of an image are contiguous: floor(16 / s) of them per granule, s rows
    apart, the rest of the granule padding -- triplets fill 15 of 16 rows, where padding them to four rows would fill 12), classes
    aligned to granules, images aligned to tiles when `by_image` (per-image layers).
    Returns (pos, n_pad, gmeta, tile_gmax, row_map, tile_img) or None when a group has more than 16 rows."""
    hid = np.asarray(harmonic_id).astype(np.int64)
    img = np.asarray(image_id).astype(np.int64)
    n = len(hid)
    order = np.argsort(hid, kind="stable")
    gid, first, size = np.unique(hid[order], return_index=True, return_counts=True)
    if size.max() > GRANULE:
        return None
    member = np.arange(n) - np.repeat(first, size)                       # member index of every sorted row
    gimg = img[order][first] if by_image else np.zeros(len(gid), dtype=np.int64)
    cls = size.astype(np.int64)                                          # class = exact group size
    per = GRANULE // cls                                                 # groups of that class per granule
    # regions = (image, class) pairs in sorted order; groups ranked inside their region
    key = gimg * 32 + cls
    gorder = np.argsort(key, kind="stable")
    rkey, rfirst, rcount = np.unique(key[gorder], return_index=True, return_counts=True)
    rcls = rkey % 32
    rimg = rkey // 32
    rrows = -(-rcount // (GRANULE // rcls)) * GRANULE                    # rows of a region: whole granules
    # image blocks aligned to tiles when the tiles must be single-image
    if by_image:
        ids, ifirst = np.unique(rimg, return_index=True)
        irows = np.add.reduceat(rrows, ifirst)
        irows = -(-irows // TILE) * TILE
        ibase = np.concatenate([[0], np.cumsum(irows)[:-1]])
        within = np.cumsum(rrows) - rrows - np.repeat((np.cumsum(rrows) - rrows)[ifirst], np.diff(np.concatenate([ifirst, [len(rimg)]])))
        rbase = np.repeat(ibase, np.diff(np.concatenate([ifirst, [len(rimg)]]))) + within
        n_pad = int(irows.sum())
        tile_img = np.repeat(ids, irows // TILE).astype(np.int32)
    else:
        rbase = np.cumsum(rrows) - rrows
        n_pad = int(-(-int(rrows.sum()) // TILE) * TILE)
        tile_img = None
    grank = np.empty(len(gid), dtype=np.int64)                           # rank of a group inside its region
    grank[gorder] = np.arange(len(gid)) - np.repeat(rfirst, rcount)
    gregion = np.empty(len(gid), dtype=np.int64)
    gregion[gorder] = np.repeat(np.arange(len(rkey)), rcount)
    gstart = rbase[gregion] + (grank // per) * GRANULE + (grank % per) * cls      # packed position of member 0
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.repeat(gstart, size) + member
    gmeta = np.zeros(n_pad, dtype=np.int32)
    gmeta[pos[order]] = (member | (np.repeat(size, size) << 8)).astype(np.int32)
    row_map = np.full(n_pad, -1, dtype=np.int32)
    row_map[pos] = np.arange(n, dtype=np.int32)
    tile_gmax = np.zeros(n_pad // TILE, dtype=np.int32)
    np.maximum.at(tile_gmax, pos[order] // TILE, np.repeat(size, size).astype(np.int32))
    return pos, n_pad, gmeta, tile_gmax, row_map, tile_img


class _ShardRows:
    """`x[sl]` of a (possibly memory-mapped) 2-D array as float32: the conversion happens on the selected rows only."""

    def __init__(self, a: np.ndarray, sl):
        self.a, self.shape = a, a.shape

    def __getitem__(self, sl) -> np.ndarray:
        return np.asarray(self.a[sl], dtype=np.float32)


class Selection(NamedTuple):
    """What `select_rows` answers: which rows of the caller's arrays a launch holds, and their small columns."""
    sl: object                          # the rows inside the caller's arrays: a slice or an int64 index array
    rows: Optional[np.ndarray]          # their global row numbers when they are not a contiguous range (ascending), else None
    start: int
    N: int
    N_total: int
    refl_id: np.ndarray                 # int32 [N]
    image_id: np.ndarray                # int32 [N]
    metadata: _ShardRows                # metadata[sl] -> float32 [N][d], converted on demand
    iobs: np.ndarray                    # fp32 per slot (mono: a row is its own slot; a group shard: its groups, then its share of the padded slots)
    sig: np.ndarray
    harmonic_id: Optional[np.ndarray]   # int64 [N], local to the shard (its first group is 0); None: monochromatic data


def select_rows(inputs, start, stop, laue_groups=None, rows=None, n_refl=None, n_images=None) -> Selection:
    """Row selection: a contiguous range, the explicit row list of a reflection-owner shard, or the harmonic groups
    `laue_groups = (g0, g1, pad0, pad1)` of `laue_group_shard`.  Every range check of the inputs is made here, before anything indexes
    with an id.  Views of the caller's arrays (possibly memory-mapped files shared by the ranks of a node): only this shard's rows are
    ever copied / converted -- a rank of an 8-GPU job does not hold eight copies' worth of the 50 M-observation problem."""
    refl_all = _np(BaseModel.get_refl_id(inputs)).reshape(-1)
    image_all = _np(BaseModel.get_image_id(inputs)).reshape(-1)
    meta_all = _np(BaseModel.get_metadata(inputs))
    meta_all = meta_all.reshape(len(refl_all), -1)
    iobs_all = _np(BaseModel.get_intensities(inputs)).reshape(-1)
    sig_all = _np(BaseModel.get_uncertainties(inputs)).reshape(-1)
    n_total = int(len(refl_all))
    laue = BaseModel.is_laue(inputs)
    hid_all = _np(BaseModel.get_harmonic_id(inputs)).reshape(-1).astype(np.int64) if laue else None
    g0 = 0
    if laue and laue_groups is not None:
        g0, g1, pad0, pad1 = laue_groups
        rows = np.nonzero((hid_all >= g0) & (hid_all < g1))[0]
        # per-slot arrays of this shard: its own groups first, then its share of the padded slots (formatter.py:637-640)
        slots = np.concatenate([np.arange(g0, g1), np.arange(pad0, pad1)])
        assert len(slots) == len(rows)
    elif rows is not None:
        # monochromatic rows that are not a contiguous range (reflection-owner shard): stored in ascending row order; the global
        # row numbers key the in-kernel noise (noise_row) and pick the columns of injected noise
        if laue:
            raise ValueError("explicit rows are for monochromatic data (Laue shards go by harmonic group)")
        rows = np.asarray(rows, dtype=np.int64)
        slots = rows
    else:
        slots = slice(start, n_total if stop is None else stop)
    if rows is not None:
        sl, start, n = rows, 0, len(rows)
    else:
        sl, n = slots, slots.stop - start
    iobs, sig = iobs_all[slots].astype(np.float32), sig_all[slots].astype(np.float32)
    if n <= 0:
        raise ValueError("empty observation shard")
    if n_refl is not None and refl_all.size and (refl_all.min() < 0 or refl_all.max() >= n_refl):
        raise ValueError("refl_id outside the range of the surrogate posterior")
    if n_images is not None and image_all.size and image_all.max() >= n_images:
        raise ValueError("image_id exceeds ImageScaler.max_images")
    if laue and hid_all.size and (hid_all.min() < 0 or hid_all.max() >= n_total):
        raise ValueError("harmonic_id outside [0, N)")
    return Selection(sl, rows, int(start), int(n), n_total, refl_all[sl].astype(np.int32), image_all[sl].astype(np.int32),
                     _ShardRows(meta_all, sl), iobs, sig, hid_all[sl] - g0 if laue else None)


@dataclass
class Layout:
    """What the layout step answers: the host image of one launch's arrays in the order the kernels read them (numpy arrays and scalars; `ObsData` uploads
    it and lets it go).  None: the layout has no such array."""
    n_pad: int
    meta_t: np.ndarray                         # fp32 [meta_rows][n_pad], feature-major ((4, 4) of zeros in the wide layout)
    refl_id: np.ndarray                        # int32; padding -1
    image_id: np.ndarray                       # int32; padding 0
    iobs: np.ndarray                           # fp32 per stored row (packed mono / single-pass Laue; padding 0) or per slot
    sig: np.ndarray                            # ... padding 1
    rows: Optional[np.ndarray] = None          # int64: global row of every stored row when that is not start + its position
    row_index: Optional[np.ndarray] = None     # ... the copy the slot kernels and the wide path read on the device
    harmonic_id: Optional[np.ndarray] = None   # int32 per stored row: the slot kernels' group ids (two-pass Laue, wide Laue)
    row_map: Optional[np.ndarray] = None       # int32 [n_pad]: the caller's local row of a packed position, -1 on padding
    tile_img: Optional[np.ndarray] = None      # int32 per tile: its image (by image)
    gmeta: Optional[np.ndarray] = None         # int32 [n_pad]: member | size << 8 (single-pass Laue)
    tile_gmax: Optional[np.ndarray] = None     # int32 per tile: its largest group
    noise_row: Optional[np.ndarray] = None     # int32 [n_pad]: the global row that keys the in-kernel noise
    pad_iobs: Optional[np.ndarray] = None      # fp32: the padded slots' own arrays (single-pass Laue)
    pad_sig: Optional[np.ndarray] = None
    pad_uniform: bool = False
    fused_laue: bool = False
    meta_rm: Optional[np.ndarray] = None       # fp32 [N][meta_ld], row-major (wide)
    meta_ld: int = 0
    perm: Optional[np.ndarray] = None          # int64: stored position -> the caller's local row (wide, sorted by image)
    img_seg: Optional[np.ndarray] = None       # int64 [n_images + 1]: first stored row of every image

    ARRAYS = ("meta_t", "refl_id", "image_id", "iobs", "sig", "row_index", "harmonic_id", "row_map", "tile_img", "gmeta", "tile_gmax",
              "noise_row", "pad_iobs", "pad_sig", "meta_rm")          # what lives on the device; rows / perm / img_seg stay on the host


def _tiles(n: int) -> int:
    return ((n + TILE - 1) // TILE) * TILE


def _scatter(v: np.ndarray, pos, n_pad: int, fill) -> np.ndarray:
    """`v` at the positions `pos` of an array of n_pad entries, `fill` elsewhere"""
    out = np.full(n_pad, fill, dtype=v.dtype)
    out[pos] = v
    return out


def meta_feature_major(md: np.ndarray, meta_rows: int, n_pad: int, pos) -> np.ndarray:
    """The feature-major metadata image [meta_rows][n_pad] of the rows `md` [N][d], row i at column pos[i], written once: rows
    d .. meta_rows - 1 and the padding columns are zero."""
    meta_t = np.zeros((meta_rows, n_pad), dtype=np.float32)
    meta_t[:md.shape[1], pos] = md.T
    return meta_t


def meta_by_image(md: np.ndarray, image_id: np.ndarray, meta_rows: int):
    """The feature-major image of `md` in the packed order of `pack_by_image`: (meta_t, pos, n_pad, tile_img, row_map)."""
    pos, n_pad, tile_img, row_map = pack_by_image(image_id)
    return meta_feature_major(md, meta_rows, n_pad, pos), pos, n_pad, tile_img, row_map


def meta_row_major(md: np.ndarray, meta_ld: int) -> np.ndarray:
    """The row-major metadata image [N][meta_ld] of the layer-by-layer path: the features, zero padding behind them."""
    rm = np.zeros((md.shape[0], meta_ld), dtype=np.float32)
    rm[:, :md.shape[1]] = md
    return rm


def image_order(image_id: np.ndarray, n_images: int):
    """Rows grouped by image for the grouped GEMM kernels: (perm, img_seg) -- the stable order by image (stored position -> row) and the
    first stored row of every image, int64 [n_images + 1]."""
    seg = np.concatenate([[0], np.cumsum(np.bincount(image_id, minlength=n_images))]).astype(np.int64)
    return np.argsort(image_id, kind="stable"), seg


def _slot_ids(s: Selection) -> dict:
    """What the slot kernels of the two-pass Laue path read per row: the group id and -- a shard of groups -- the global row."""
    if s.harmonic_id is None:
        return {}
    return dict(harmonic_id=s.harmonic_id.astype(np.int32), row_index=s.rows)


def layout_plain(s: Selection, meta_rows: int) -> Layout:
    """Rows in the caller's order, padded to whole tiles at the end."""
    n_pad = _tiles(s.N)
    noise_row = None
    if s.rows is not None and s.harmonic_id is None:      # (every plain-layout kernel reads the per-row noise key when it is given)
        noise_row = _scatter(s.rows.astype(np.int32), slice(0, s.N), n_pad, 0)
    return Layout(n_pad, meta_feature_major(s.metadata[s.sl], meta_rows, n_pad, slice(0, s.N)), s.refl_id, s.image_id, s.iobs, s.sig, rows=s.rows, noise_row=noise_row,
                  **_slot_ids(s))


def layout_by_image(s: Selection, meta_rows: int) -> Layout:
    """Per-image layers: rows grouped by image, every image padded to whole tiles (`pack_by_image`)."""
    meta_t, pos, n_pad, tile_img, row_map = meta_by_image(s.metadata[s.sl], s.image_id, meta_rows)
    rid, img, iobs, sig = s.refl_id, s.image_id, s.iobs, s.sig
    if s.harmonic_id is None:           # the mono likelihood runs inside the fused kernel: its inputs are packed too
        rid, img = _scatter(rid, pos, n_pad, -1), _scatter(img, pos, n_pad, 0)
        iobs, sig = _scatter(iobs, pos, n_pad, 0.0), _scatter(sig, pos, n_pad, 1.0)
    return Layout(n_pad, meta_t, rid, img, iobs, sig, rows=s.rows, row_map=row_map, tile_img=tile_img, **_slot_ids(s))


def layout_laue(s: Selection, meta_rows: int, lp) -> Layout:
    """Single-pass Laue (`lp`: what `pack_laue` answered): everything the fused kernel streams is packed so that a harmonic group sits
    in one wave; the group's observed intensity is replicated on its member rows; the padded slots keep their own small arrays."""
    pos, n_pad, gmeta, tile_gmax, row_map, tile_img = lp
    hid = s.harmonic_id
    G = int(hid.max()) + 1
    # the formatter pads every empty slot with the same (1.0, 1.0) (reference io/formatter.py:637-640): their terms are one term times
    # their number -- the engine then launches the slot kernel on ONE slot with the weight multiplied (round 5: 29 us per step at 5 M rows)
    pi, ps = s.iobs[G:], s.sig[G:]
    return Layout(n_pad, meta_feature_major(s.metadata[s.sl], meta_rows, n_pad, pos), _scatter(s.refl_id, pos, n_pad, -1), _scatter(s.image_id, pos, n_pad, 0),
                  _scatter(s.iobs[hid], pos, n_pad, 0.0), _scatter(s.sig[hid], pos, n_pad, 1.0), rows=s.rows, row_index=s.rows,
                  row_map=row_map, tile_img=tile_img, gmeta=gmeta, tile_gmax=tile_gmax,
                  # a shard of whole harmonic groups: rows are not a contiguous range
                  noise_row=_scatter(s.rows.astype(np.int32), pos, n_pad, 0) if s.rows is not None else None,
                  pad_iobs=pi, pad_sig=ps, pad_uniform=bool(len(pi) > 1 and np.all(pi == pi[0]) and np.all(ps == ps[0])), fused_laue=True)


def layout_wide(s: Selection, meta_ld: int, sort_images: bool = False, n_images=None) -> Layout:
    """Scaler wider than the fused kernel holds: layer-by-layer GEMMs on the row-major metadata [rows][ld] (the features, zero padding
    to a multiple of four; ElboEngine._data_term_wide).  Monochromatic rows are their own "harmonic group" (harmonic_id NULL): the slot
    kernels then ARE the mono likelihood."""
    rm = meta_row_major(s.metadata[s.sl], meta_ld)
    lay = Layout(_tiles(s.N), np.zeros((4, 4), dtype=np.float32), s.refl_id, s.image_id, s.iobs, s.sig, rows=s.rows, meta_rm=rm, meta_ld=meta_ld,
                 **_slot_ids(s))
    if sort_images:
        # per-image layers on this path: the rows of an image must be consecutive (grouped GEMM kernels); everything per row
        # is stored in image order, `perm` maps the local order back to the caller's
        perm, lay.img_seg = image_order(s.image_id, int(n_images or (s.image_id.max() + 1)))
        lay.perm = perm
        lay.refl_id, lay.image_id, lay.meta_rm = s.refl_id[perm], s.image_id[perm], rm[perm]
        if s.harmonic_id is None:                   # (mono: a row is its own slot; Laue keeps iobs / sig per slot)
            lay.iobs, lay.sig = s.iobs[perm], s.sig[perm]
        else:
            lay.harmonic_id = lay.harmonic_id[perm]
        # global rows in the stored (image) order: the noise key of every row, and which columns of an injected eta are its
        lay.rows = lay.row_index = (s.rows if s.rows is not None else np.arange(s.start, s.start + s.N))[perm]
    return lay


def lay_out(s: Selection, size, pack_images=False, laue_single_pass=True, wide=False, sort_images=False, n_images=None) -> Layout:
    """The precedence between the four layouts: single-pass Laue when it is asked for and every harmonic group fits a wave (`pack_laue`
    answers None when one does not: those data take the two-pass path on one of the other layouts), else by image, else wide, else plain.
    `size(name)`: the library's `cl_mlp_meta_rows` / `cl_wide_ld` of this metadata width; the layout chosen asks for the one it needs."""
    lp = pack_laue(s.harmonic_id, s.image_id, by_image=pack_images) if (s.harmonic_id is not None and laue_single_pass) else None
    if lp is not None:
        return layout_laue(s, size("cl_mlp_meta_rows"), lp)
    if pack_images:
        return layout_by_image(s, size("cl_mlp_meta_rows"))
    if wide:
        return layout_wide(s, size("cl_wide_ld"), sort_images, n_images)
    return layout_plain(s, size("cl_mlp_meta_rows"))


class ObsData:
    """refl_id / image_id int32 [N], meta_t fp32 [rows][n_pad], iobs / sig fp32 [N], optional harmonic_id + Laue work
    buffers, and the per-launch workspace of the fused kernel (grid, gradient partials).  With `pack_images` (per-image
    layers) the arrays the fused kernel streams are in the packed order of `pack_by_image`."""

    def __init__(self, lib, inputs, start: int, stop: int, S: int, P: int, device, grid=None, n_refl=None, n_images=None,
                 laue_groups=None, pack_images: bool = False, laue_single_pass: bool = True, wide: bool = False, sort_images: bool = False,
                 rows: Optional[np.ndarray] = None, host_inputs=None, slot_buffers: bool = False):
        # 1. the library's answers for this metadata width, asked when a step needs one (a launch trace shows the queries too)
        size = lambda name: int(getattr(lib, name)(self.d))
        # 2. which rows
        s = select_rows(inputs, start, stop, laue_groups, rows, n_refl, n_images)
        self.start, self.N, self.N_total, self.d = s.start, s.N, s.N_total, int(s.metadata.shape[1])
        self.laue = s.harmonic_id is not None
        self.empty = False
        # 3. in which order
        lay = lay_out(s, size, pack_images, laue_single_pass, wide, sort_images, n_images)
        # 4. onto the device (rows: the explicit row list when the stored rows are not a contiguous range; perm, img_seg: the wide path's image order)
        self.n_pad, self.pad_uniform, self.fused_laue, self.meta_ld = lay.n_pad, lay.pad_uniform, lay.fused_laue, lay.meta_ld
        self.rows, self.perm, self.img_seg = lay.rows, lay.perm, lay.img_seg
        for name in Layout.ARRAYS:
            v = getattr(lay, name)
            setattr(self, name, None if v is None else torch.as_tensor(np.ascontiguousarray(v), device=device))
        # (monochromatic rows packed by image on the two-pass launches: the scaler launches write loc / sigma and read dL/d(loc, sigma) by the
        #  caller's local row -- row_map --, so the slot kernels between them get the row arrays in that order: `slot_rows`, on those sets only)
        if slot_buffers and not self.laue and self.row_map is not None:
            self.slot_rows = {k: torch.as_tensor(np.ascontiguousarray(getattr(s, k)), device=device) for k in ("refl_id", "image_id", "iobs", "sig")}
        # 5. work buffers: the slot kernels' (two-pass Laue, wide), the padded slots', the fused kernel's gradient partials
        slots = wide or (self.laue and not self.fused_laue) or slot_buffers       # (slot_buffers: monochromatic rows on the two-pass launches, a scale prior)
        self.laue_loc = torch.empty(self.N, dtype=torch.float32, device=device) if slots else None
        self.laue_sig = torch.empty(self.N, dtype=torch.float32, device=device) if slots else None
        self.laue_iconv = torch.empty(self.N * S, dtype=torch.float32, device=device) if slots else None
        self.laue_dO = torch.empty(self.N * 2, dtype=torch.float32, device=device) if slots else None
        self.pad_iconv = torch.zeros(max(1, len(lay.pad_iobs) * S), dtype=torch.float32, device=device) if self.fused_laue else None
        g = int(grid) if grid is not None else max(1, int(lib.cl_mlp_default_grid()))
        self.grid = min(g, self.n_pad // TILE)
        self.partials = torch.empty(0 if wide else self.grid * P, dtype=torch.float32, device=device)
        # what the engine attaches later (careless_amd/engine.py, wide.py); None / 0 / False until then
        self.host_inputs = host_inputs        # the caller's inputs (a reference: the frozen-scaler path reads the rows' metadata once per training)
        self.row0, self.is_piece = 0, False   # piece of a chunked shard (`ObsChunks`): its first row inside the shard's eta / ipred arrays
        self.det = self.det_parent = None     # deterministic mode: the shard's buffers (on the set `cl_det_reduce` runs on), the set a piece stores into
        self.det_index = 0                    # ... and the piece's part of its NLL / Evans-2011 slots
        self.peel = None                      # buffers of a peeled first layer
        self.frozen_sorted = self.locsig_epoch = None         # frozen scaler: the per-training row arrays, the `train_model` call (loc, sigma) are of
        self.chain_act = self.chain_dact = self.chain_dz0 = None      # chained scaler: activations / their gradients at the block boundaries, dZ_0 of a lane-kernel last block
        self.wide_chunks = self.wide_tiles = self.wide_full = self.wide_dsd = None     # layer-by-layer path: row chunks, tile lists, kept activations, d sigma / d raw

    def alloc_chain(self, lib, blocks, w, device, lane: bool = False):
        """Buffers of a chained scaler; `lane`: the last block runs on the lane kernel, which hands back dZ_0 of its first layer."""
        rows = int(lib.cl_mlp_meta_rows(w))
        n = len(blocks) - 1
        self.chain_act = [torch.zeros(rows, self.n_pad, dtype=torch.float32, device=device) for _ in range(n)]
        self.chain_dact = [torch.zeros(rows, self.n_pad, dtype=torch.float32, device=device) for _ in range(n)]
        self.chain_dz0 = torch.zeros_like(self.chain_dact[-1]) if lane else None      # (a buffer of the last boundary's shape)


class ObsChunks:
    """A shard whose metadata image does not fit one launch of the fused kernels (their per-lane offsets are 32-bit: a launch
    addresses < 4 GiB of metadata; 50 M observations with positional encodings are 4.8 GB): consecutive `ObsData` pieces that are
    launched one after the other.  The reference is full-batch at any N (careless/models/merging/variational.py:255-256) and so is
    this: the weight-gradient partials reduce per launch into the same gradient, NLL and dz_f accumulate, the noise is keyed by
    the global row.  Only the plain observation layout is cut (packed layouts keep whole groups / images per launch)."""

    def __init__(self, children: List[ObsData]):
        self.children = children
        c0 = children[0]
        self.start, self.N, self.N_total, self.d = c0.start, sum(c.N for c in children), c0.N_total, c0.d
        self.n_pad, self.grid, self.partials = sum(c.n_pad for c in children), c0.grid, c0.partials
        self.laue, self.fused_laue, self.rows, self.row_map, self.perm, self.empty = False, False, None, None, None, False
        self.det = None                             # deterministic mode: the shard's buffers (ElboEngine._det_attach)
        row0 = 0
        for c in children:
            c.row0, c.is_piece = row0, True         # first row of the piece inside the shard's eta / ipred arrays; several launches share dz_f
            row0 += c.N

    def alloc_chain(self, lib, blocks, w, device, lane: bool = False):
        c0 = self.children[0]
        c0.alloc_chain(lib, blocks, w, device, lane)                 # the pieces run one after the other: one set of buffers
        for c in self.children[1:]:
            c.chain_act, c.chain_dact = c0.chain_act, c0.chain_dact
            c.chain_dz0 = torch.zeros_like(c0.chain_dz0) if lane else None


class _EmptyObs:
    """An owner-mode rank's share of a validation set in which none of its reflections occurs: nothing to launch."""

    def __init__(self, n_total: int):
        self.N, self.N_total, self.rows, self.empty = 0, n_total, np.zeros(0, dtype=np.int64), True


def launch_row_limit(d: int, S: int = 0) -> int:
    """Most rows of the plain layout one launch takes: 4 * cl_mlp_meta_rows(d) * n_pad bytes of metadata must stay below 4 GiB
    (include/careless_hip.h: return code -4), and -- `S` given: launches that address per-(row, sample) arrays with 32-bit lane
    offsets (the deterministic mode's dzf_obs) -- 4 * S * n_pad bytes as well.  CARELESS_HIP_MAX_LAUNCH_BYTES lowers the bound
    (tests of the chunked path)."""
    import os
    lim = int(os.environ.get("CARELESS_HIP_MAX_LAUNCH_BYTES", str((1 << 32) - (1 << 24))))
    per_row = 4 * max((d + 3) // 4 * 4, int(S))
    return max(TILE, lim // per_row // TILE * TILE)


