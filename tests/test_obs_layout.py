"""The host code under `ObsData` (careless_amd/obs.py: row selection, the four observation layouts, the upload), without a device and
without the library: `scripts/obs_table.py` builds every layout with `device="cpu"` and a stand-in for the library's three size queries.

* the record: the table of that script equals tests/golden/obs_layouts.json, taken before the constructor was split into its steps;
* properties that hold for any correct layout, stated against the INPUTS (so they do not inherit a mistake of the record);
* every `ValueError` of the selection, by the smallest input that raises it;
* on a device: the same objects built there equal the ones built on the host, tensor for tensor (the upload decides nothing).
"""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from careless_amd.engine import ObsData, laue_group_shard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("obs_table", os.path.join(ROOT, "scripts", "obs_table.py"))
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)

CASES = T.cases()
# which layout each case must come out in (from the request and the data, DESIGN 3: single-pass Laue > by image > wide > plain)
KIND = {"plain": "plain", "plain_range": "plain", "plain_rows": "plain", "by_image": "by_image", "by_image_interleaved": "by_image",
        "wide": "wide", "wide_sorted_4": "wide", "wide_sorted_none": "wide", "wide_sorted_interleaved": "wide", "wide_sorted_range": "wide",
        "laue": "fused", "laue_by_image": "fused", "laue_by_image_interleaved": "fused", "laue_pad_changed": "fused", "laue_one_pad": "fused",
        "laue_group_of_17": "plain", "laue_two_pass": "plain", "laue_wide": "wide", "laue_wide_sorted": "wide",
        "laue_wide_sorted_interleaved": "wide", "laue_shard": "fused", "laue_shard_two_pass": "plain"}
TILE, GRANULE = 128, 16


def test_the_case_list_is_the_one_the_layouts_were_recorded_on():
    assert set(CASES) == set(KIND) and len(CASES) == 22


def test_layout_table_matches_the_record():
    """Every attribute of every case: name, kind, dtype, shape and SHA-1 of the bytes (work buffers: dtype and shape), `repr` of the rest."""
    with open(os.path.join(ROOT, "tests", "golden", "obs_layouts.json")) as f:
        want = json.load(f)
    got = T.table()
    assert set(got) == set(want)
    for name in want:
        assert set(got[name]) == set(want[name]), name
        differ = {k: (got[name][k], want[name][k]) for k in want[name] if got[name][k] != want[name][k]}
        assert not differ, (name, differ)


def _t(x):
    return None if x is None else x.numpy()


@pytest.mark.parametrize("name", sorted(CASES))
def test_layout_properties(name):
    kw_in, start, stop, kw = CASES[name]
    inputs, o = T.build(CASES[name])
    kind = KIND[name]
    refl, image, meta, iobs_all, sig_all = (np.asarray(inputs[k]) for k in (0, 1, 3, 4, 5))
    refl, image, iobs_all, sig_all = refl.reshape(-1), image.reshape(-1), iobs_all.reshape(-1), sig_all.reshape(-1)
    laue = len(inputs) > 7
    d = meta.shape[1]
    # the global rows the object must hold, in the caller's order, and -- Laue -- their groups and the slots' arrays
    hid = g0 = None
    if laue:
        hid = np.asarray(inputs[7]).reshape(-1)
        G = int(hid.max()) + 1
    if kw.get("laue_groups") is not None:
        g0, g1, pad0, pad1 = kw["laue_groups"]
        sel = np.nonzero((hid >= g0) & (hid < g1))[0]
        slot_iobs, slot_sig = np.concatenate([iobs_all[g0:g1], iobs_all[pad0:pad1]]), np.concatenate([sig_all[g0:g1], sig_all[pad0:pad1]])
        pads = (iobs_all[pad0:pad1], sig_all[pad0:pad1])
    elif kw.get("rows") is not None:
        sel = np.asarray(kw["rows"])
    else:
        sel = np.arange(start, T.N if stop is None else stop)
        slot_iobs, slot_sig = iobs_all[sel], sig_all[sel]
        if laue:
            pads = (iobs_all[G:], sig_all[G:])
    n = len(sel)
    explicit = kw.get("rows") is not None or g0 is not None
    assert (o.N, o.N_total, o.d, o.laue, o.fused_laue) == (n, T.N, d, laue, kind == "fused")
    assert o.start == (0 if explicit else start)
    assert o.grid == min(T.GRID, o.n_pad // TILE) and o.partials.shape == (0 if kind == "wide" else o.grid * T.P,)

    # ---- where local row i is stored ---------------------------------------------------------------------------------
    if kind in ("by_image", "fused"):
        row_map = _t(o.row_map)
        assert row_map.shape == (o.n_pad,) and o.n_pad % TILE == 0
        real = row_map >= 0
        assert np.array_equal(np.sort(row_map[real]), np.arange(n)) and np.all(row_map[~real] == -1)      # a bijection onto 0 .. N - 1
        pos = np.empty(n, dtype=np.int64)
        pos[row_map[real]] = np.nonzero(real)[0]
    else:
        assert o.row_map is None and o.n_pad == (n + TILE - 1) // TILE * TILE
        real = np.arange(o.n_pad) < n
        if kw.get("sort_images"):
            perm = o.perm
            assert np.array_equal(np.sort(perm), np.arange(n))                                            # a permutation
            pos = np.argsort(perm)                                                                        # stored k holds local row perm[k]
        else:
            assert o.perm is None
            pos = np.arange(n)

    # ---- the metadata: the caller's rows at the real positions, zeros everywhere else ------------------------------------
    if kind == "wide":
        rm = _t(o.meta_rm)
        assert rm.shape == (n, (d + 3) & ~3) and o.meta_ld == rm.shape[1] and rm.dtype == np.float32
        assert np.array_equal(rm[pos, :d], meta[sel].astype(np.float32)) and not rm[:, d:].any()
        assert o.meta_t.shape == (4, 4) and not _t(o.meta_t).any()
    else:
        mt = _t(o.meta_t)
        assert mt.shape == ((d + 3) & ~3, o.n_pad) and mt.dtype == np.float32 and o.meta_rm is None and o.meta_ld == 0
        assert np.array_equal(mt[:d, pos].T, meta[sel].astype(np.float32))
        assert not mt[d:].any() and not mt[:, ~real].any()

    # ---- ids, intensities ------------------------------------------------------------------------------------------------
    rid, img, io, sg = _t(o.refl_id), _t(o.image_id), _t(o.iobs), _t(o.sig)
    assert rid.dtype == img.dtype == np.int32 and io.dtype == sg.dtype == np.float32
    assert np.array_equal(rid[pos], refl[sel]) and np.array_equal(img[pos], image[sel])
    if kind == "fused" or (kind == "by_image" and not laue):
        assert rid.shape == io.shape == (o.n_pad,)
        assert np.all(rid[~real] == -1) and np.all(io[~real] == 0.0) and np.all(sg[~real] == 1.0)       # padding rows
    else:
        assert rid.shape == (n,)
    if kind == "fused":
        # every member row carries its slot's observation; the slots behind the last group are the padded slots' own arrays
        assert np.array_equal(io[pos], iobs_all[hid[sel]]) and np.array_equal(sg[pos], sig_all[hid[sel]])
        assert np.array_equal(_t(o.pad_iobs), pads[0]) and np.array_equal(_t(o.pad_sig), pads[1])
        assert o.pad_iconv.shape == (max(1, len(pads[0]) * T.S),) and not _t(o.pad_iconv).any()
        uniform = len(pads[0]) > 1 and len(set(pads[0].tolist())) == 1 and len(set(pads[1].tolist())) == 1
        assert o.pad_uniform is uniform
        assert uniform == (name not in ("laue_pad_changed", "laue_one_pad"))
        assert o.harmonic_id is None and o.laue_loc is None
        # no group crosses a multiple of 16; its rows are consecutive; gmeta = member | size << 8; tile_gmax = the tile's largest group
        gmeta, gmax = _t(o.gmeta), np.zeros(o.n_pad // TILE, dtype=np.int64)
        assert not gmeta[~real].any()
        for g in np.unique(hid[sel]):
            p = np.sort(pos[hid[sel] == g])
            assert p[0] // GRANULE == p[-1] // GRANULE and np.array_equal(p, np.arange(p[0], p[0] + len(p))), g
            assert np.array_equal(gmeta[p], np.arange(len(p)) | (len(p) << 8)), g
            gmax[p[0] // TILE] = max(gmax[p[0] // TILE], len(p))
        assert np.array_equal(_t(o.tile_gmax), gmax)
    else:
        assert o.pad_iobs is None and o.pad_sig is None and o.pad_iconv is None and o.pad_uniform is False and o.gmeta is None and o.tile_gmax is None
        if laue:           # two-pass and wide Laue: intensities per slot, group ids (local to the shard) per stored row
            assert np.array_equal(io, slot_iobs) and np.array_equal(sg, slot_sig)
            assert np.array_equal(_t(o.harmonic_id)[pos], hid[sel] - (g0 or 0)) and o.harmonic_id.dtype == torch.int32
        else:              # monochromatic: a row is its own slot
            assert np.array_equal(io[pos], iobs_all[sel]) and np.array_equal(sg[pos], sig_all[sel]) and o.harmonic_id is None
    slot_buffers = kind == "wide" or (laue and kind != "fused")
    for buf, size in (("laue_loc", n), ("laue_sig", n), ("laue_iconv", n * T.S), ("laue_dO", 2 * n)):
        assert (getattr(o, buf).shape == (size,)) if slot_buffers else (getattr(o, buf) is None), buf

    # ---- by image (mono or single-pass Laue): a tile holds one image and tile_img names it -------------------------------
    if kw.get("pack_images"):
        tile_img = _t(o.tile_img)
        assert tile_img.shape == (o.n_pad // TILE,) and tile_img.dtype == np.int32
        assert np.array_equal(tile_img[pos // TILE], image[sel])
    else:
        assert o.tile_img is None

    # ---- wide, sorted by image -----------------------------------------------------------------------------------------
    if kw.get("sort_images"):
        assert np.all(np.diff(img) >= 0)
        n_img = kw.get("n_images") or int(image[sel].max()) + 1
        assert o.img_seg.dtype == np.int64 and np.array_equal(o.img_seg, [int((img < k).sum()) for k in range(n_img + 1)])
        assert np.array_equal(o.rows, sel[o.perm]) and o.rows.dtype == np.int64
        assert np.array_equal(_t(o.row_index), o.rows) and o.row_index.dtype == torch.int64
    else:
        assert o.img_seg is None
        # ---- rows that are not a contiguous range: their global numbers ------------------------------------------------
        if explicit:
            assert np.array_equal(o.rows, sel) and o.rows.dtype == np.int64
        else:
            assert o.rows is None
        if laue and explicit:
            assert np.array_equal(_t(o.row_index), sel)
        else:
            assert o.row_index is None
    if explicit and not (laue and kind != "fused"):
        nr = _t(o.noise_row)
        assert nr.shape == (o.n_pad,) and nr.dtype == np.int32 and np.array_equal(nr[pos], sel) and not nr[~real].any()
    else:
        assert o.noise_row is None


def test_the_laue_cases_put_a_group_across_a_granule_in_the_callers_order():
    """... so that the packed order has something to repair."""
    hid = np.asarray(T.make_inputs(laue=True)[7]).reshape(-1)
    sizes = np.bincount(hid)
    assert set(sizes.tolist()) == {1, 2, 3}
    rows = [np.nonzero(hid == g)[0] for g in range(len(sizes))]
    assert any(r[0] // GRANULE != r[-1] // GRANULE for r in rows)
    assert np.bincount(np.asarray(T.make_inputs(laue=True, big=17)[7]).reshape(-1)).max() == 17


def _tiny(n=2, laue=False, **cols):
    """`n` rows, one metadata column; `cols` replace a column"""
    c = dict(refl_id=np.zeros(n, np.int64), image_id=np.zeros(n, np.int64), file_id=np.zeros(n, np.int64), metadata=np.ones(n, np.float32),
             intensities=np.ones(n, np.float32), uncertainties=np.ones(n, np.float32))
    if laue:
        c.update(wavelength=np.ones(n, np.float32), harmonic_id=np.arange(n, dtype=np.int64))
    c.update({k: np.asarray(v) for k, v in cols.items()})
    return tuple(v.reshape(n, 1) for v in c.values())


def _obs(inputs, start=0, stop=None, **kw):
    return ObsData(T.StubLib(), inputs, start, stop, T.S, T.P, "cpu", grid=T.GRID, **kw)


@pytest.mark.parametrize("what, make, message", [
    ("explicit rows on Laue data", lambda: _obs(_tiny(1, laue=True), rows=np.array([0])), "explicit rows are for monochromatic data (Laue shards go by harmonic group)"),
    ("empty range", lambda: _obs(_tiny(1), 0, 0), "empty observation shard"),
    ("empty row list", lambda: _obs(_tiny(1), rows=np.zeros(0, np.int64)), "empty observation shard"),
    ("refl_id == n_refl", lambda: _obs(_tiny(1, refl_id=[1]), n_refl=1), "refl_id outside the range of the surrogate posterior"),
    ("refl_id < 0", lambda: _obs(_tiny(1, refl_id=[-1]), n_refl=1), "refl_id outside the range of the surrogate posterior"),
    ("image_id == n_images", lambda: _obs(_tiny(1, image_id=[1]), n_images=1), "image_id exceeds ImageScaler.max_images"),
    ("harmonic_id == N, single pass", lambda: _obs(_tiny(1, laue=True, harmonic_id=[1])), "harmonic_id outside [0, N)"),
    ("harmonic_id == N, two pass", lambda: _obs(_tiny(1, laue=True, harmonic_id=[1]), laue_single_pass=False), "harmonic_id outside [0, N)"),
    ("harmonic_id < 0", lambda: _obs(_tiny(1, laue=True, harmonic_id=[-1])), "harmonic_id outside [0, N)"),
    ("harmonic_id == N of 300 rows, single pass", lambda: _obs(_tiny(300, laue=True, harmonic_id=np.r_[np.arange(299), 300])), "harmonic_id outside [0, N)"),
])
def test_selection_errors(what, make, message):
    """The five `ValueError`s of the row selection, each by the smallest input that raises it (one row).  An id >= N used to reach
    `pack_laue` on the single-pass path and die there with numpy's IndexError; the range check now runs before anything indexes."""
    with pytest.raises(ValueError) as e:
        make()
    assert str(e.value) == message, what


def test_selection_errors_keep_their_order():
    """empty shard, then refl_id, then image_id, then harmonic_id"""
    bad = _tiny(1, laue=True, refl_id=[5], image_id=[5], harmonic_id=[5])
    for kw, message in ((dict(stop=0, n_refl=1, n_images=1), "empty observation shard"), (dict(n_refl=1, n_images=1), "refl_id outside the range of the surrogate posterior"),
                        (dict(n_images=1), "image_id exceeds ImageScaler.max_images"), ({}, "harmonic_id outside [0, N)")):
        with pytest.raises(ValueError) as e:
            _obs(bad, **kw)
        assert str(e.value) == message


def test_smallest_valid_inputs_build():
    """... so the error cases fail for their reason and not for their size."""
    assert _obs(_tiny(1), n_refl=1, n_images=1).n_pad == TILE
    assert _obs(_tiny(1, laue=True)).fused_laue
    o = _obs(_tiny(4, laue=True, harmonic_id=[0, 0, 1, 1]), laue_groups=laue_group_shard(np.array([0, 0, 1, 1]), 1, 2))
    assert o.N == 2 and o.rows.tolist() == [2, 3] and o.noise_row[:2].tolist() == [2, 3]


def test_host_inputs_is_a_constructor_argument():
    inputs = _tiny(1)
    assert _obs(inputs).host_inputs is None and _obs(inputs, host_inputs=inputs).host_inputs is inputs


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
def test_device_image_equals_host_image():
    """`ObsData` built on the device against `ObsData` built with device="cpu", same library (the real one): every attribute equal,
    tensor for tensor, every tensor where it was asked to be.  Nothing is launched."""
    from careless_amd import _lib
    lib = _lib.get_lib()
    for name, case in CASES.items():
        host, dev = T.build(case, lib, "cpu")[1], T.build(case, lib, "cuda")[1]
        assert T.describe(dev) == T.describe(host), name
        for k, v in vars(dev).items():
            if torch.is_tensor(v):
                assert v.is_cuda and not getattr(host, k).is_cuda, (name, k)
                if k not in T.UNINITIALISED:
                    assert torch.equal(v.cpu(), getattr(host, k)), (name, k)
