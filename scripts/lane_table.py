"""Which kernel instance does the library select for which scaler launch?  (Host only: no GPU, nothing is launched.)

    python scripts/lane_table.py OUT.json

What a change of the lane kernel's selection code (the launch layer at the end of csrc/elbo_lane.hip) has to show: record the table on
the parent and on the change (`CARELESS_HIP_LIB` selects the library) and compare.  `cl_mlp_route` and `cl_mlp_kernel_name` are asked on
made-up non-null pointers over a grid that straddles every threshold that code tests -- widths 4 / 6 / 8 / 10 / 12, columns 8 / 15 / 31,
depths 18 / 19 / 20 -- in every observation layout, with every optional buffer that picks another form of an instance, and for the two
launches of a head-less layer block.  tests/golden/lane_instances.json is this record; tests/test_host_logic.py walks the same grid.

The file: `pairs` = the distinct [route, name], `rows` = for every entry of `walk()`, in its order, the index of its pair.
"""
from __future__ import annotations

import ctypes as C
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWITCHES = ("CARELESS_HIP_LANE", "CARELESS_HIP_NARROW", "CARELESS_HIP_EPI")      # (prefixes) the A/B switches that move shapes between kernels
S = 2
DEPTHS = (1, 2, 3, 12, 18, 19, 20, 21)
WIDTHS = (1, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13)
COLUMNS = (1, 8, 9, 15, 16, 31, 32)
_IMGL = dict(row_map=1, tile_img=1, imgl=1, d_imgl=1, n_images=1)
LAYOUTS = {"plain": {}, "packed": dict(row_map=1, gmeta=1, tile_gmax=1),
           **{f"image_layers{K}": dict(_IMGL, n_imgl=K) for K in (1, 2, 3, 4)},
           "image_layers2_laue": dict(_IMGL, n_imgl=2, gmeta=1, tile_gmax=1)}
OPTIONS = {"none": {}, "eta": dict(eta=1), "ipred_out": dict(ipred_out=1), "ev11": dict(ev11=1, d_ev11=1), "dZ0_out": dict(dZ0_out=1),
           "deterministic": dict(dzf_obs=1, dimg_obs=1, nll_part=1, det_slot=1), "dZ0_out_eta": dict(dZ0_out=1, eta=1)}
BLOCKS = {1: dict(act_out=1), 2: dict(dH_ext=1, partials=1)}      # the launches of a head-less layer block: plain layout, no option


def walk():
    """(mode, cl_mlp_args fields) of every entry, in the order of the record"""
    for L, w, d in itertools.product(DEPTHS, WIDTHS, COLUMNS):
        shape = dict(L=L, w=w, d=d, S=S)
        for layout, option in itertools.product(LAYOUTS.values(), OPTIONS.values()):
            yield 0, {**shape, **layout, **option}
        for mode, fields in BLOCKS.items():
            yield mode, {**shape, **fields}


def table(lib):
    """[(route, name)] over walk()"""
    from careless_amd import _lib
    buf = C.create_string_buffer(160)
    out = []
    for mode, fields in walk():
        a = _lib.MlpArgs(**fields)
        n = lib.cl_mlp_kernel_name(C.byref(a), mode, buf, len(buf))
        assert 0 < n < len(buf), (mode, fields, n)
        out.append((int(lib.cl_mlp_route(C.byref(a), mode)), buf.value.decode()))
    return out


def encode(rows) -> dict:
    pairs = sorted(set(rows))
    index = {p: k for k, p in enumerate(pairs)}
    return {"pairs": [list(p) for p in pairs], "rows": [index[r] for r in rows]}


def decode(rec: dict):
    return [tuple(rec["pairs"][k]) for k in rec["rows"]]


def main(argv) -> int:
    if len(argv) != 2:
        print(__doc__)
        return 2
    set_ = sorted(k for k in os.environ if k.startswith(SWITCHES))
    if set_:
        print("refusing to record a table with A/B switches set: " + ", ".join(set_))
        return 1
    from careless_amd import _lib
    rows = table(_lib.get_lib())
    with open(argv[1], "w") as f:
        json.dump(encode(rows), f, separators=(",", ":"))
        f.write("\n")
    names = {p for p in set(rows)}
    print(f"{len(rows)} entries, {len(names)} distinct (route, name) pairs, {sum(1 for r, n in names if n.startswith('elbo_lane_kernel<'))} of them lane names")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
