"""Which route, epilogue, return code and instance does the library give a launch of the 16/32/64-wide kernel?  (Host only: no GPU.)

    python scripts/mlp_table.py OUT.json

The sibling of scripts/lane_table.py (whose grid stops at width 13 and 32 columns) for the scaler launch layer (csrc/mlp_launch.hip) and
the units of csrc/elbo_mlp.hip under it: `cl_mlp_route`, `cl_mlp_epilogue`, `cl_mlp_check` and `cl_mlp_kernel_name` are asked on made-up
non-null pointers over a grid that straddles every threshold `mlp_geom`, `epi_plain` and `mlp_route` test -- widths 8 .. 65, columns
8 .. 65, depths 1 .. 25 -- in every observation layout, with every option that picks another route, instance or epilogue, and for the
forward-only and external-gradient launches.  The check is asked with every pointer its entry wants, n_obs = n_pad = 256, grid 2.
tests/golden/mlp_instances.json is this record, taken before the launch layer moved out of the kernel file; tests/test_host_logic.py
walks the same grid.  The option x layout product is thinned (the options that only move the epilogue stay on the plain and the packed
layout), the thresholds are not.

The file, as lane_table's: `pairs` = the distinct [route, epilogue, check, name], `rows` = for every entry of `walk()` the index of its tuple.
"""
from __future__ import annotations

import ctypes as C
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from lane_table import SWITCHES, decode, encode  # noqa: E402,F401

WIDTHS = (8, 12, 13, 15, 16, 17, 32, 33, 64, 65)
COLUMNS = (8, 9, 32, 33, 64, 65)
DEPTHS = (1, 5, 6, 10, 11, 20, 21, 24, 25)       # (with K = 1 and K = 3 per-image layers: L + K on both sides of 5, 10 and 24)
NORMAL, STUDENTT, LAPLACE = 0, 1, 2
_IMGL = dict(row_map=1, tile_img=1, imgl=1, d_imgl=1, n_images=1)
_DET = dict(dzf_obs=1, dimg_obs=1, nll_part=1, det_slot=1)
OPTIONS = {"none": {}, "eta": dict(eta=1), "noise_row": dict(noise_row=1), "ipred_out": dict(ipred_out=1), "ev11": dict(ev11=1, d_ev11=1),
           "S8": dict(S=8), "S9": dict(S=9), "normal": dict(lik_kind=NORMAL), "studentt": dict(lik_kind=STUDENTT), "laplace": dict(lik_kind=LAPLACE),
           "dZ0_out": dict(dZ0_out=1), "deterministic": _DET, "deterministic_dX": dict(_DET, dX_out=1)}
_SOME = ("none", "eta", "ev11", "laplace", "dZ0_out", "deterministic")
# layout -> (its fields, the options of mode 0 it is walked with)
LAYOUTS = {"plain": ({}, tuple(OPTIONS)),
           "packed": (dict(row_map=1, gmeta=1, tile_gmax=1), _SOME + ("ipred_out", "S9", "deterministic_dX")),
           "image_layers1": (dict(_IMGL, n_imgl=1), _SOME), "image_layers3": (dict(_IMGL, n_imgl=3), _SOME),
           "image_layers2_laue": (dict(_IMGL, n_imgl=2, gmeta=1, tile_gmax=1), _SOME)}
LAUNCHES = {"loc_sig_out": dict(loc_out=1, sig_out=1), "act_out": dict(act_out=1), "dO_ext": dict(dO_ext=1), "dH_ext": dict(dH_ext=1),
            "dH_ext_dX": dict(dH_ext=1, dX_out=1)}
# what the entry check of a mode wants (cl_elbo_mono_fwd_bwd, cl_mlp_forward, cl_mlp_backward_ext)
ENTRY = {0: dict(refl_id=1, iobs=1, sig=1, z_f=1, dz_f=1, partials=1, scalars=1), 1: dict(loc_out=1, sig_out=1), 2: dict(dO_ext=1, partials=1)}
COMMON = dict(meta_t=1, mlp=1, n_obs=256, n_pad=256, S=2, R=50)
GRID = 2
ENTRIES = 29160


def walk():
    """(mode, cl_mlp_args fields) of every entry, in the order of the record"""
    for L, w, d in itertools.product(DEPTHS, WIDTHS, COLUMNS):
        shape = dict(COMMON, L=L, w=w, d=d)
        for layout, options in LAYOUTS.values():
            for o in options:
                yield 0, {**shape, **ENTRY[0], **layout, **OPTIONS[o]}
        for mode, launch in itertools.product((1, 2), LAUNCHES.values()):
            yield mode, {**shape, **ENTRY[mode], **launch}
        for layout in ("packed", "image_layers1"):           # the forward-only and the external-gradient launch of the packed layouts
            for mode in (1, 2):
                yield mode, {**shape, **ENTRY[mode], **LAYOUTS[layout][0]}


def table(lib):
    """[(route, epilogue, check, name)] over walk()"""
    from careless_amd import _lib
    buf = C.create_string_buffer(160)
    out = []
    for mode, fields in walk():
        a = _lib.MlpArgs(**fields)
        n = lib.cl_mlp_kernel_name(C.byref(a), mode, buf, len(buf))
        assert 0 < n < len(buf), (mode, fields, n)
        out.append((int(lib.cl_mlp_route(C.byref(a), mode)), int(lib.cl_mlp_epilogue(C.byref(a), mode)),
                    int(lib.cl_mlp_check(C.byref(a), mode, GRID)), buf.value.decode()))
    return out


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
    routes, epis, codes = ({r[k] for r in rows} for k in range(3))
    print(f"{len(rows)} entries, {len(set(rows))} distinct tuples; routes {sorted(routes)}, epilogues {sorted(epis)}, codes {sorted(codes)}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
