"""What does `ObsData` put into each of its arrays, in every observation layout?  (Host only: no GPU, no library.)

    python scripts/obs_table.py OUT.json
    python scripts/obs_table.py --time plain|by_image|laue       (one big construction in this process: seconds, peak resident MB)

What a change of the host code under `ObsData` (careless_amd/obs.py: row selection, the four layouts, the upload) has to show: record
the table on the parent and on the change and compare.  The constructor is run with `device="cpu"` and a three-method stand-in for the
library's queries (`cl_mlp_meta_rows`, `cl_wide_ld`: `(d + 3) & ~3`; the grid is given), on the smallest inputs at which each layout can
still go wrong: 300 rows (three 128-row tiles, the last one ragged) of 4 images of unequal size, 20 reflections, d = 5 (8 metadata
rows: the zero rows show) or d = 70 (wide, pitch 72).  tests/golden/obs_layouts.json is this record; tests/test_obs_layout.py
recomputes it and holds the layouts to properties stated against the inputs.

The file: per case, per attribute of the object (all of `vars(obj)` but `host_inputs`): arrays and tensors as [kind, dtype, shape,
SHA-1 of the bytes], the uninitialised work buffers as [kind, dtype, shape], everything else as its `repr`.
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S, P, GRID, N_REFL, N = 3, 77, 8, 20, 300
IMAGE_ROWS = (130, 37, 101, 32)                  # 2 + 1 + 1 + 1 tiles by image, 3 tiles plain
UNINITIALISED = ("laue_loc", "laue_sig", "laue_iconv", "laue_dO", "partials")      # torch.empty: dtype and shape only


class StubLib:
    """The three integers the layout code asks the library for."""

    def __init__(self, grid: int = GRID):
        self.grid = grid

    def cl_mlp_meta_rows(self, d):
        return (int(d) + 3) & ~3

    def cl_wide_ld(self, d):
        return (int(d) + 3) & ~3

    def cl_mlp_default_grid(self):
        return self.grid


def group_sizes(rng, image_rows, big=None, singles=False):
    """Sizes of the harmonic groups, image by image (no group spans two images): 1..3 rows; `big`: the first group has that many;
    `singles`: one pair, every other row on its own (exactly one padded slot)."""
    sizes = []
    for k, n in enumerate(image_rows):
        left = n
        if k == 0 and big:
            sizes.append(big)
            left -= big
        if k == 0 and singles:
            sizes.append(2)
            left -= 2
        while left:
            s = 1 if singles else min(left, int(rng.integers(1, 4)))
            sizes.append(s)
            left -= s
    return np.asarray(sizes, dtype=np.int64)


def make_inputs(d=5, laue=False, shuffle_images=False, big=None, singles=False, pad_change=False, seed=7):
    """The `inputs` tuple (BaseModel.input_index order, every column 2-D) of 300 rows.  Laue: `harmonic_id` labels the groups in a
    shuffled order (a shard of a label range is no row range), intensities / uncertainties are per slot: the groups' own, then the
    formatter's (1, 1) fill on the padded slots."""
    rng = np.random.default_rng(seed)
    image = np.repeat(np.arange(len(IMAGE_ROWS)), IMAGE_ROWS).astype(np.int64)
    if shuffle_images:
        image = image[rng.permutation(N)]
    refl = rng.integers(0, N_REFL, N).astype(np.int64)
    meta = rng.standard_normal((N, d)).astype(np.float32)
    iobs = rng.gamma(2.0, 50.0, N).astype(np.float32)
    sig = (1.0 + rng.random(N) * 5.0).astype(np.float32)
    col = lambda v: v.reshape(-1, 1)
    out = [col(refl), col(image), col(np.zeros(N, dtype=np.int64)), meta, col(iobs), col(sig)]
    if laue:
        sizes = group_sizes(rng, IMAGE_ROWS, big=big, singles=singles)
        G = len(sizes)
        first = np.cumsum(sizes) - sizes
        if not (big or singles):
            assert set(sizes.tolist()) == {1, 2, 3} and np.any(first // 16 != (first + sizes - 1) // 16)     # a group straddles a granule
        label = rng.permutation(G)
        hid = np.repeat(label, sizes)
        if shuffle_images:                       # rows of image k in the caller's order take the k-th block of group ids
            hid = hid[np.argsort(np.argsort(image, kind="stable"), kind="stable")]
        iobs[G:], sig[G:] = 1.0, 1.0
        if pad_change:
            iobs[G + 1] = 2.0
        out += [col(rng.random(N).astype(np.float32) + 1.0), col(hid.astype(np.int64))]
    return tuple(out)


def cases():
    """name -> (make_inputs arguments, ObsData arguments: start, stop, keywords)"""
    from careless_amd.obs import laue_group_shard
    shard = lambda: laue_group_shard(make_inputs(laue=True)[7].reshape(-1), 1, 2)
    L = dict(laue=True)
    return {
        "plain": ({}, 0, None, {}),
        "plain_range": ({}, 100, 260, {}),
        "plain_rows": ({}, 0, None, dict(rows=np.arange(3, N, 2))),
        "by_image": ({}, 0, None, dict(pack_images=True)),
        "by_image_interleaved": (dict(shuffle_images=True), 0, None, dict(pack_images=True)),
        "wide": (dict(d=70), 0, None, dict(wide=True)),
        "wide_sorted_4": (dict(d=70), 0, None, dict(wide=True, sort_images=True, n_images=4)),
        "wide_sorted_none": (dict(d=70), 0, None, dict(wide=True, sort_images=True)),
        "wide_sorted_interleaved": (dict(d=70, shuffle_images=True), 0, None, dict(wide=True, sort_images=True, n_images=4)),
        "wide_sorted_range": (dict(d=70, shuffle_images=True), 100, 260, dict(wide=True, sort_images=True)),
        "laue": (L, 0, None, {}),
        "laue_by_image": (L, 0, None, dict(pack_images=True)),
        "laue_by_image_interleaved": (dict(L, shuffle_images=True), 0, None, dict(pack_images=True)),
        "laue_pad_changed": (dict(L, pad_change=True), 0, None, {}),
        "laue_one_pad": (dict(L, singles=True), 0, None, {}),
        "laue_group_of_17": (dict(L, big=17), 0, None, {}),
        "laue_two_pass": (L, 0, None, dict(laue_single_pass=False)),
        "laue_wide": (dict(L, d=70), 0, None, dict(wide=True, laue_single_pass=False)),
        "laue_wide_sorted": (dict(L, d=70), 0, None, dict(wide=True, sort_images=True, laue_single_pass=False)),
        "laue_wide_sorted_interleaved": (dict(L, d=70, shuffle_images=True), 0, None, dict(wide=True, sort_images=True, laue_single_pass=False)),
        "laue_shard": (L, 0, None, dict(laue_groups=shard())),
        "laue_shard_two_pass": (L, 0, None, dict(laue_groups=shard(), laue_single_pass=False)),
    }


def build(case, lib=None, device="cpu"):
    """(inputs, ObsData) of one entry of `cases()`"""
    from careless_amd.obs import ObsData
    kw_in, start, stop, kw = case
    inputs = make_inputs(**kw_in)
    return inputs, ObsData(lib or StubLib(), inputs, start, stop, S, P, device, grid=GRID, n_refl=N_REFL, **kw)


def describe(obj) -> dict:
    import torch
    out = {}
    for name, v in sorted(vars(obj).items()):
        if name == "host_inputs":
            continue
        if torch.is_tensor(v) or isinstance(v, np.ndarray):
            a = v.detach().cpu().numpy() if torch.is_tensor(v) else v
            out[name] = ["tensor" if torch.is_tensor(v) else "ndarray", str(a.dtype), list(a.shape)]
            if name not in UNINITIALISED:
                out[name].append(hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest())
        else:
            out[name] = repr(v)
    return out


def table(lib=None, device="cpu") -> dict:
    return {name: describe(build(case, lib, device)[1]) for name, case in cases().items()}


def time_case(which: str) -> int:
    """One construction at a size where its time and memory show: 4 M plain rows at d = 21, the same packed by image, 2 M single-pass
    Laue rows.  Run it in a fresh process per observation (peak resident memory is the process's)."""
    import resource
    import time
    from careless_amd.obs import ObsData
    rng = np.random.default_rng(0)
    n, d = (2_000_000, 21) if which == "laue" else (4_000_000, 21)
    col = lambda v: v.reshape(-1, 1)
    image = np.sort(rng.integers(0, 2000, n)).astype(np.int64)
    inputs = [col(rng.integers(0, 100_000, n).astype(np.int64)), col(image), col(np.zeros(n, dtype=np.int64)),
              rng.standard_normal((n, d)).astype(np.float32), col(rng.random(n).astype(np.float32)), col(rng.random(n).astype(np.float32) + 1.0)]
    if which == "laue":
        hid = np.repeat(np.arange(n // 2), 2).astype(np.int64)           # pairs
        inputs += [col(np.ones(n, dtype=np.float32)), col(hid)]
    kw = dict(pack_images=True) if which == "by_image" else {}
    t0 = time.perf_counter()
    o = ObsData(StubLib(256), tuple(inputs), 0, None, 4, 1000, "cpu", grid=256, n_refl=100_000, **kw)
    dt = time.perf_counter() - t0
    print(json.dumps({"case": which, "n_pad": o.n_pad, "seconds": round(dt, 4), "peak_rss_mb": round(resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024.0, 1)}))
    return 0


def main(argv) -> int:
    if len(argv) == 3 and argv[1] == "--time" and argv[2] in ("plain", "by_image", "laue"):
        return time_case(argv[2])
    if len(argv) != 2:
        print(__doc__)
        return 2
    rec = table()
    with open(argv[1], "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(rec)} cases, {sum(len(v) for v in rec.values())} attributes")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
