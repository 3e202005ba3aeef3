"""The fused scaler + likelihood kernel (csrc/elbo_mlp.hip) behind cl_elbo_mono_fwd_bwd (mode 0), cl_mlp_forward (mode 1) and
cl_mlp_backward_ext (mode 2), restated ONCE in fp64 from the contract (include/careless_hip.h: cl_mlp_args), with a bound or a summand size
beside every output element, the inputs and the generated case list of the direct kernel tests (tests/test_mlp_kernels_gpu.py), and an
fp32 emulation of the launch with its wrong variants (MUTANTS).  tests/test_ref_mlp.py checks all of it without a GPU.

Built from what exists: tests/ref_wide.py (Dense stack, head, bijector: gamma(m) sum |a||b|, the input's error carried to first order,
BIJ_RTOL behind the bijector) and tests/ref_rows.py (`reference`: densities, Evans-2011 terms, harmonic group sums, the summand size M).
The arrays are the fp32 arrays the device gets, in the device's layouts: meta_t feature-major [cl_mlp_meta_rows(d)][n_pad], mlp in the W^T
layout, z_f [R][S], eta [rows][S].  Nothing is specific to elbo_mlp.hip: the same argument block describes the launches of the lane and
narrow kernels.

Bounds (no new tolerance):
    loc_out, sig_out, act_out   the derived bound of ref_wide.  The error of a layer's input is carried through the LeakyReLU with the
                                unit's OWN slope: no case holds a pre-activation inside its bound (`near_zero` = 0 is asserted for every
                                case), so every unit's branch is certain and the first-order factor is the slope itself
    ipred_out                   RTOL_LOSS M per element;   NLL  RTOL_LOSS max(M, 1)
    every gradient entry and every deterministic record   RTOL_GRAD M + one fp32 rounding of the stored value, M the chain rule with every
                                summand replaced by its absolute value (|W|, |dO|, slopes; the residual as |ipred| + |iobs|: ref_rows); every
                                gradient tensor also RTOL_GRAD of its max-norm; nll_part, a record and an NLL, the tighter of the two bars
Accumulating outputs (dz_f, d_img, d_ev11, scalars, cl_reduce_partials' target) are preloaded at a tenth of their M.

Inputs.  The Dense stack is identity plus a perturbation, each unit's row rescaled so that its pre-activations have unit variance over the
case's rows (activations neither die nor grow over 20 layers), and each unit's bias puts the LeakyReLU's kink into the LARGEST GAP between
two neighbouring rows' pre-activations in the unit's second and third quartile: both branches are taken by a quarter of a unit's rows at
least, and no pre-activation lies near zero.  That is what makes the rule "no unit inside its own bound" reachable at all: with a kink at
a random place the worst-case bound of a 20-layer stack (2.6 per layer in the max-norm of |W|) puts hundreds of the 2 x 10^5
pre-activations of a 677-row case inside it, whatever the seed (NOTEBOOK).  Seeds are still searched (`case_seed`) and the count asserted.
"""
from __future__ import annotations

import copy
import ctypes
import math
from types import SimpleNamespace

import numpy as np

from tests import ref_rows as RR
from tests import ref_wide as RW
from tests.ref_q import fp

F32 = np.float32
U = RW.U
RTOL_LOSS, RTOL_GRAD = RR.RTOL_LOSS, RR.RTOL_GRAD
TILE = 128
EV11_WAVES = 8
LEAK = float(np.float32(0.01))          # the number the device gets
DOF = RR.DOF
SEED, STEP, OBS_OFFSET = 20263, 7, 3000
SENT = RR.SENT
UNITS = ("plain", "chain", "packed", "det", "packed_det", "chain_det")
UNIT_TAG = {"plain": "", "chain": ", chain", "packed": ", packed", "det": ", deterministic", "packed_det": ", packed deterministic",
            "chain_det": ", chain deterministic"}
EPI_NAMES = ("generic", "plain normal", "plain studentt")


def meta_rows(d):
    return (d + 3) & ~3


def param_count(d, w, L, head=True):
    return w * d + w + (L - 1) * (w * w + w) + (2 * w + 2 if head else 0)


def unpack(mlp, d, w, L, head=True):
    """[(Wt_l [w][in], b_l [w])], head [2 w + 2] or None from the flat W^T layout"""
    mlp = np.asarray(mlp)
    out, o = [], 0
    for l in range(L):
        k = d if l == 0 else w
        out.append((mlp[o:o + w * k].reshape(w, k), mlp[o + w * k:o + w * k + w]))
        o += w * k + w
    return out, (mlp[o:o + 2 * w + 2] if head else None)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
def case(unit, mode, w, d, L, n=5 * TILE + 37, grid=2, S=3, lik="normal", bij="exp", img="off", noise="eta", ipred=False, ev11=False, head=True,
         dX=False, det_slot=False, groups=False, noise_row=False, tag="", kernel="mlp", dz0=False):
    """One launch.  unit: one of UNITS; img: off / sorted (image borders inside a wave's 16 rows) / unsorted; noise: eta (injected) / philox
    (drawn in the kernel: the reference takes cl_debug_noise(kind = 1)); head False: a head-less block of a chain (act_out in mode 1, dH_ext in
    mode 2); dX: dX_out given; groups: gmeta / tile_gmax (packed units); n: the caller's rows (active rows of a packed layout).  kernel: whose
    launch geometry the case has (WAVES: elbo_mlp.hip's 128-row tiles, or the 64- / 32-row wave tiles of elbo_lane.hip / elbo_narrow.hip, strided
    over all waves of the launch: tests/ref_lane.py); dz0: dZ0_out given (those two kernels only)."""
    c = SimpleNamespace(unit=unit, mode=mode, w=w, d=d, L=L, n=n, grid=grid, S=S, lik=lik, bij=bij, img=img, noise=noise, ipred=ipred, ev11=ev11,
                        head=head, dX=dX, det_slot=det_slot, groups=groups, noise_row=noise_row, tag=tag, kernel=kernel, dz0=dz0)
    c.packed, c.det, c.chain = unit.startswith("packed"), unit.endswith("det"), unit.startswith("chain")
    assert unit in UNITS and (head or c.chain) and (not dX or c.chain) and (not groups or (c.packed and mode == 0)) and kernel in WAVES
    assert not dz0 or (kernel != "mlp" and mode == 0)
    assert not (lik == "laplace" and ev11) and (mode == 0 or not (ipred or ev11))
    c.id = (f"{unit}-m{mode}-{L}x{w}-d{d}-n{n}-g{grid}-S{S}-{lik}-{bij}" + ("" if img == "off" else f"-img{img}") + ("" if noise == "eta" else "-philox") +
            ("-ipred" if ipred else "") + ("-ev11" if ev11 else "") + ("" if head else "-nohead") + ("-dX" if dX else "") + ("-slot" if det_slot else "") +
            ("-groups" if groups else "") + ("-noiserow" if noise_row else "") + ("-dz0" if dz0 else "") + ("" if kernel == "mlp" else f"-{kernel}") +
            (f"-{tag}" if tag else ""))
    return c


def set_fields(c):
    """the pointer fields of cl_mlp_args the case sets (what the route, the epilogue and the check look at)"""
    f = {"meta_t", "mlp", "stop_flag"}
    if c.mode == 0:
        f |= {"refl_id", "iobs", "sig", "z_f", "partials", "scalars", "dz_f"}
        if c.img != "off":
            f |= {"image_id", "img", "d_img"}
        if c.noise == "eta":
            f.add("eta")
        if c.ipred:
            f.add("ipred_out")
        if c.ev11:
            f |= {"ev11", "ev11_part" if c.det else "d_ev11"}
        if c.det:
            f |= {"dzf_obs", "nll_part"} | ({"dimg_obs"} if c.img != "off" else set()) | ({"det_slot"} if c.det_slot else set())
    elif c.mode == 1:
        f |= {"loc_out", "sig_out"} if c.head else {"act_out"}
    else:
        f |= {"partials", "dO_ext" if c.head else "dH_ext"}
    if c.dX:
        f.add("dX_out")
    if c.dz0:
        f.add("dZ0_out")
    if c.packed:
        f.add("row_map")
        if c.groups:
            f |= {"gmeta", "tile_gmax"}
        if c.noise_row:
            f.add("noise_row")
    elif c.noise_row:
        f.add("noise_row")
    return f


def scalar_fields(c):
    """the scalar fields the route, the name and the entry check read (a packed layout of c.n active rows has at least that many positions)"""
    n_pad = (c.n + TILE - 1) // TILE * TILE
    return dict(n_obs=n_pad if c.packed else c.n, n_pad=n_pad, d=c.d, w=c.w, L=c.L, S=c.S, R=64, leak=LEAK, lik_kind=RR.KINDS[c.lik], dof=DOF,
                bij_kind=RW.BIJ_EXP if c.bij == "exp" else RW.BIJ_SOFTPLUS, use_img=int(c.img != "off"))


def query(c, lib=None):
    """(route, kernel name, epilogue, instance name) of the case from the library's own routing: no device needed"""
    from careless_amd import _lib
    lib = lib or _lib.get_lib()
    a = _lib.MlpArgs(**scalar_fields(c), **{k: 1 for k in set_fields(c)})
    buf = ctypes.create_string_buffer(256)
    lib.cl_mlp_kernel_name(ctypes.byref(a), c.mode, buf, 256)
    route, epi = int(lib.cl_mlp_route(ctypes.byref(a), c.mode)), int(lib.cl_mlp_epilogue(ctypes.byref(a), c.mode))
    name = buf.value.decode()
    return route, name, epi, instance_name(name, epi, c)


def instance_name(kernel_name, epi, c):
    """what names a compiled instance: the kernel's template arguments, the epilogue, and the Laplace instance of a full step (the generic
    epilogue with the kind compiled in: not a value of cl_epilogue)"""
    return f"{kernel_name} {EPI_NAMES[epi]}" + (" laplace" if c.mode == 0 and c.lik == "laplace" else "")


# width forms: (WP, LMAX, KS as a full step / an external-gradient launch runs it) -> hidden widths at the rim and inside it, depths
FORMS = {(16, 20, 2): ((1, 8), (1, 2, 20)), (16, 20, 3): ((9, 12), (1, 2, 20)), (16, 20, 4): ((13, 15), (1, 2, 20)), (16, 20, 5): ((16,), (1, 2, 20)),
         (32, 5, 4): ((17, 31, 32), (1, 2, 5)), (32, 10, 4): ((17, 31, 32), (6, 10)), (64, 5, 4): ((33, 64), (1, 2, 5))}
DPS = {8: (1, 6, 8), 32: (9, 18, 32), 64: (33, 50, 64)}
UNIT_MODES = {"plain": (0, 1, 2), "chain": (0, 1, 2), "packed": (0, 1, 2), "det": (0,), "packed_det": (0,), "chain_det": (0,)}


def enumerate_instances():
    """Every instance of elbo_mlp.hip outside the per-image-layer unit that direct arguments reach, from the rules of mlp_geom / mlp_route
    (csrc/cl_kernels.h, csrc/mlp_launch.hip) restated: {instance name: (unit, mode, WP, DP, LMAX, KS, variant)}.
      * seven width forms; the forward-only launch keeps all four k-steps at width <= 15 (KS = 4 for every such width);
      * three metadata capacities; three modes on the plain, chain and packed units, full steps only on the deterministic ones;
      * a full step has a Laplace instance beside the generic one; the 64-wide full step of the plain unit also the two plain epilogues;
      * a full step of width <= 15 on <= 15 metadata columns in the plain or packed layout (deterministic or not) belongs to the narrow and lane
        kernels unless it is a Laplace step: the generic instances <16, 8, ...> of those units are reached by no arguments (the chain units'
        are: dX_out keeps a launch off both kernels)."""
    out = {}
    for unit in UNITS:
        for mode in UNIT_MODES[unit]:
            for (WP, LMAX, KS) in FORMS:
                ks = 4 if (mode == 1 and WP == 16 and KS < 5) else KS
                for DP in DPS:
                    variants = ["generic"] + (["laplace"] if mode == 0 else [])
                    if unit == "plain" and mode == 0 and WP == 64:
                        variants += ["plain normal", "plain studentt"]
                    for v in variants:
                        if mode == 0 and unit in ("plain", "packed", "det", "packed_det") and WP == 16 and KS < 5 and DP == 8 and v != "laplace":
                            continue
                        epi = v if v.startswith("plain") else "generic"
                        name = f"elbo_mlp_kernel<{WP}, {DP}, {LMAX}, {mode}{UNIT_TAG[unit]}, KS={ks}> {epi}" + (" laplace" if v == "laplace" else "")
                        out.setdefault(name, (unit, mode, WP, DP, LMAX, ks, v))
    return out


def _variant_kw(v):
    # the plain epilogues want in-kernel noise, no ipred_out, S <= 8; the generic one of a Normal step anything else
    return {"generic": dict(lik="normal", noise="eta"), "laplace": dict(lik="laplace", noise="eta"), "plain normal": dict(lik="normal", noise="philox", S=5),
            "plain studentt": dict(lik="studentt", noise="philox", S=8)}[v]


def _unit_kw(unit, mode, k):
    """how a unit's launches of a mode are told apart (the k-th instance of the unit alternates the chain's forms)"""
    if unit == "chain":
        return {0: dict(dX=True), 1: dict(head=False), 2: (dict(head=False, dX=bool(k & 1)) if k % 3 else dict(dX=True))}[mode]
    if unit == "chain_det":
        return dict(dX=True)
    return {}


def _candidates(WP, LMAX, KS, DP):
    """shapes of a width form on a metadata capacity, the rim values first.  (Which of them reach the instance is the library's answer: a full step
    of width <= 15 that is not a Laplace step leaves the narrow and lane kernels by d >= 32, by widths 13 .. 15 on 16 .. 31 columns, or by dX_out.)"""
    ws, Ls = FORMS[(WP, LMAX, KS)]
    return [(w, d, L) for L in Ls for w in ws for d in DPS[DP] if L <= 2 or (d > 1 and w > 1)]      # (a stack behind ONE column or unit is a function of one number: its units are collinear, the
                                                                                                  # rescaled rows of the layers behind reach |W| row sums of 13 and the fp32 emulation 0.24 of a weight gradient's bound)


def instance_cases(lib=None):
    """one case per enumerated instance at n = 5 * 128 + 37 rows on two workgroups, the shape cycling through the form's rim values; the shape is
    accepted when the library names the wanted instance for it"""
    out, k = [], 0
    for name, (unit, mode, WP, DP, LMAX, ks, v) in enumerate_instances().items():
        forms = [f for f in FORMS if f[0] == WP and f[1] == LMAX and (f[2] == ks or (mode == 1 and WP == 16 and ks == 4 and f[2] < 5))]
        cands = [s for f in forms for s in _candidates(*f, DP)]
        kw = dict(_variant_kw(v) if mode == 0 else {}, **_unit_kw(unit, mode, k))
        if mode == 0:
            kw.update(img=("off", "sorted", "unsorted")[k % 3], bij=("exp", "softplus")[k % 2])
            if v == "generic":
                kw.update(S=(1, 3, 4, 9)[k % 4], lik=("normal", "studentt")[(k // 2) % 2], ipred=bool(k % 2))
            if unit.startswith("packed"):
                kw.update(groups=bool(k % 2))
        else:
            kw.update(bij=("exp", "softplus")[k % 2])
        for i in range(len(cands)):
            w, d, L = cands[(k + i) % len(cands)]
            c = case(unit, mode, w, d, L, **kw)
            if query(c, lib)[3] == name:
                c.instance = name
                out.append(c)
                break
        k += 1
    return out


def _like(c, **kw):
    f = dict(n=c.n, grid=c.grid, S=c.S, lik=c.lik, bij=c.bij, img=c.img, noise=c.noise, ipred=c.ipred, ev11=c.ev11, head=c.head, dX=c.dX, det_slot=c.det_slot,
             groups=c.groups, noise_row=c.noise_row, tag=c.tag, kernel=c.kernel, dz0=c.dz0)
    f.update(kw)
    return case(c.unit, c.mode, c.w, c.d, c.L, **f)


def extra_cases(lib=None):
    """once per (unit, width form), on a full step: n = 3, n = 128 exactly, one workgroup, a grid larger than the tile count; the forward-only and
    external-gradient launches of the form at n = 3 and under the larger grid"""
    out, seen, info = [], set(), enumerate_instances()
    for c0 in instance_cases(lib):
        unit, mode, WP, DP, LMAX, ks, v = info[c0.instance]
        key = (unit, mode, WP, LMAX, ks)
        if key in seen or v.startswith("plain"):
            continue
        seen.add(key)
        rows = ((3, 2, "n3"), (TILE, 1, "n128"), (5 * TILE + 37, 1, "g1"), (2 * TILE + 37, 7, "gbig")) if mode == 0 else ((3, 2, "n3"), (2 * TILE + 37, 7, "gbig"))
        out += [_like(c0, n=n, grid=grid, tag=tag) for n, grid, tag in rows]
    return out


def option_cases(lib=None):
    out = []
    # MC samples on every epilogue of the 64-wide plain unit; the batches beyond eight on the generic one
    for S in (1, 3, 4, 5, 8):
        out.append(case("plain", 0, 64, 18, 2, S=S, lik="normal", noise="philox", img="sorted", tag="opt"))
        out.append(case("plain", 0, 33, 6, 5, S=S, lik="studentt", noise="philox", bij="softplus", tag="opt"))
    for S in (1, 3, 4, 5, 8, 9, 12):
        out.append(case("plain", 0, 64, 33, 2, S=S, lik=("normal", "studentt", "laplace")[S % 3], ipred=True, img="unsorted", tag="opt"))
        out.append(case("plain", 0, 17, 9, 6, S=S, lik=("laplace", "normal", "studentt")[S % 3], noise="philox" if S % 2 else "eta", tag="opt"))
        out.append(case("plain", 0, 16, 8, 2, S=S, lik="studentt", bij="softplus", img="sorted", tag="opt"))
    # bijector and image scales on the plain epilogues (what else keeps a launch on them: the S sweep above, the stop flag in stop_cases)
    out.append(case("plain", 0, 64, 50, 5, S=8, lik="normal", noise="philox", bij="softplus", img="unsorted", tag="opt"))
    out.append(case("plain", 0, 33, 32, 2, S=4, lik="studentt", noise="philox", bij="exp", img="sorted", tag="opt"))
    # every option on the generic epilogue of every (unit, width form): the MC sample counts with likelihood, bijector, image scales, noise and
    # ipred_out cycling; the Evans-2011 buffers (d_ev11 on the atomic units, ev11_part per wave on the deterministic ones); det_slot on the
    # deterministic units; noise_row on the packed ones
    k = 0
    for unit, (WP, LMAX, KS), w, d, L, kw in _unit_forms():
        for S in (1, 3, 4, 5, 8, 9, 12):
            out.append(case(unit, 0, w, d, L, S=S, lik=("normal", "studentt", "laplace")[k % 3], bij=("exp", "softplus")[k % 2], img=("sorted", "off", "unsorted")[k % 3],
                            noise=("eta", "philox")[(k // 2) % 2], ipred=bool(k % 5 == 0), groups=unit.startswith("packed") and bool(k % 2), tag="opt", **kw))
            k += 1
        out.append(case(unit, 0, w, d, L, S=4, lik=("normal", "studentt")[k % 2], ev11=True, img=("sorted", "unsorted")[k % 2], ipred=bool(k % 3 == 0),
                        groups=unit.startswith("packed") and bool(k % 2), tag="opt", **kw))
        if unit.endswith("det"):
            out.append(case(unit, 0, w, d, L, S=(4, 5)[k % 2], det_slot=True, img=("unsorted", "sorted", "off")[k % 3], noise=("eta", "philox")[k % 2],
                            ev11=bool(k % 2), groups=unit.startswith("packed") and not k % 2, tag="opt", **kw))
        if unit.startswith("packed"):
            out.append(case(unit, 0, w, d, L, S=(3, 8)[k % 2], noise="philox", noise_row=True, groups=bool(k % 2), img=("off", "sorted")[k % 2],
                            det_slot=unit.endswith("det") and bool(k % 2), tag="opt"))
    return out


def _unit_forms():
    """(unit, width form, w, d, L, unit keywords) of every (unit, width form): the form's widest width, its second depth (LMAX 10: its first), d off
    a multiple of 4 -- 33 where a full step of width <= 15 has to stay off the narrow and lane kernels"""
    k = 0
    for unit in UNITS:
        kw = dict(dX=True) if unit.startswith("chain") else {}
        for form, (ws, Ls) in FORMS.items():
            WP, LMAX, KS = form
            d = 33 if (WP == 16 and KS < 5 and not unit.startswith("chain")) else (6, 18, 50)[k % 3]
            yield unit, form, ws[-1], d, (Ls[1] if Ls[0] <= 5 else Ls[0]), kw
            k += 1


def stop_cases():
    """a raised stop flag once per (unit, width form) on a full step with every optional output the unit has, on the two plain epilogues, and on
    the forward-only and external-gradient launches of the plain, chain and packed units"""
    out = []
    for k, (unit, form, w, d, L, kw) in enumerate(_unit_forms()):
        out.append(case(unit, 0, w, d, L, S=(3, 4)[k % 2], lik=("normal", "studentt")[k % 2], ev11=True, ipred=True, img=("sorted", "unsorted")[k % 2],
                        det_slot=unit.endswith("det") and bool(k % 2), groups=unit.startswith("packed") and bool(k % 2), tag="stop", **kw))
    out.append(case("plain", 0, 64, 8, 5, S=8, lik="normal", noise="philox", img="sorted", tag="stop"))
    out.append(case("plain", 0, 33, 18, 2, S=5, lik="studentt", noise="philox", img="unsorted", tag="stop"))
    out += [case("plain", 1, 16, 8, 2, tag="stop"), case("plain", 2, 31, 33, 6, tag="stop"), case("packed", 1, 12, 6, 2, tag="stop"), case("packed", 2, 64, 18, 5, tag="stop"),
            case("chain", 1, 15, 33, 2, head=False, tag="stop"), case("chain", 2, 33, 9, 2, head=False, dX=True, tag="stop"), case("chain", 2, 16, 50, 20, dX=True, tag="stop")]
    return out


def expected_instance(c):
    """the instance a case of this file's units must run, from the rules of mlp_geom / epi_plain (csrc/cl_kernels.h) restated: what every launch
    of the GPU tests and every case of the list is compared with (the library's answer is the other side)"""
    DP = 8 if c.d <= 8 else (32 if c.d <= 32 else 64)
    if c.w <= 15:
        WP, LMAX, KS = 16, 20, (4 if c.mode == 1 else (2 if c.w <= 8 else (3 if c.w <= 12 else 4)))
    elif c.w == 16:
        WP, LMAX, KS = 16, 20, 5
    elif c.w <= 32:
        WP, LMAX, KS = 32, (5 if c.L <= 5 else 10), 4
    else:
        WP, LMAX, KS = 64, 5, 4
    epi = "generic"
    if (c.unit == "plain" and WP == 64 and c.mode == 0 and c.noise == "philox" and not (c.noise_row or c.ipred or c.ev11) and c.S <= 8 and c.lik != "laplace"):
        epi = "plain " + c.lik
    return f"elbo_mlp_kernel<{WP}, {DP}, {LMAX}, {c.mode}{UNIT_TAG[c.unit]}, KS={KS}> {epi}" + (" laplace" if c.mode == 0 and c.lik == "laplace" else "")


_CASES = {}


def cases(lib=None):
    """the whole generated list (cached): instance cases, row borders, options"""
    if "all" not in _CASES:
        cs = instance_cases(lib) + extra_cases(lib) + option_cases(lib)
        ids = set()
        _CASES["all"] = [c for c in cs if not (c.id in ids or ids.add(c.id))]
    return _CASES["all"]


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def _kink(z, rng):
    """per unit the bias that puts zero into the largest gap between neighbouring rows' values in the unit's second and third quartile"""
    n, w = z.shape
    zs = np.sort(z, axis=0)
    if n == 1:
        return -(zs[0] - np.where(rng.random(w) < 0.5, 0.7, -0.7))
    lo, hi = int(0.25 * (n - 1)), max(int(0.25 * (n - 1)) + 1, int(math.ceil(0.75 * (n - 1))))
    gaps = zs[lo + 1:hi + 1] - zs[lo:hi]
    i = lo + np.argmax(gaps, axis=0)
    return -0.5 * (zs[i, np.arange(w)] + zs[i + 1, np.arange(w)])


def scaler_problem(seed, n, d, w, L, head=True, sig=None, X=None, full=False):
    """(X [n][d], flat mlp in the W^T layout): module docstring, "Inputs".  The perturbation is 0.3 / sqrt(fan-in) up to five layers, a third of it on
    deeper stacks, where the propagated bound at 0.3 reaches the kinks' gaps (20 x 16 on 677 rows: 30 pre-activations inside it)"""
    sig = (0.3 if L <= 5 else 0.1) if sig is None else sig
    rng = np.random.default_rng([31, seed, n, d, w, L])
    # (a case of fewer than 64 rows takes the first ones of 64: variances and gaps of three rows say little.)  The metadata are multiples of 2^-8,
    # the first layer's weights and biases of 2^-13 and 2^-10: its products and sums are exact in fp32 in any order, its error is the one rounding of
    # leak * z.  Against gamma(d + 4) of a d-column dot product, d = 1 .. 8, three or four honest roundings are a quarter of the bound
    # (NOTEBOOK: act_out of a one-layer block on 6 columns, 0.27)
    X = (np.round(RW.normals(rng, max(n, 64), d) * 256) / 256).astype(F32) if X is None else X
    H, flat = X.astype(np.float64), []
    n_all, n = n, len(X)
    for l in range(L):
        k = d if l == 0 else w
        W = np.eye(w, k) + sig * rng.standard_normal((w, k)) / math.sqrt(k)
        W += (np.abs(np.eye(w, k)).sum(1, keepdims=True) == 0) * rng.standard_normal((w, k)) / math.sqrt(k)      # (units past the identity's rows)
        z = H @ W.T
        sd = z.std(0) if n > 1 else np.abs(z[0])
        W = (W / np.where(sd > 0, sd, 1.0)[:, None]).astype(F32)
        if l == 0:
            W = (np.round(W * 8192) / 8192).astype(F32)
            W = np.where(W == 0, F32(1.0 / 8192), W)                      # (no gradient entry exactly zero by accident)
        b = _kink(H @ W.astype(np.float64).T, rng).astype(F32)
        if l == 0:
            b = (np.round(b * 1024) / 1024).astype(F32)
            b = np.where(b == 0, F32(1.0 / 1024), b)                      # (a padding position's pre-activation is the bias itself)
        flat += [W.ravel(), b]
        H = RW.lrelu(H @ W.astype(np.float64).T + b, LEAK)
    if head:
        # loc = 2.5 +- 1 at the most, sigma = f(-2.3 +- 0.4) <= 0.15: loc + sigma eta + shift never cancels.  Where it does (sigma ~ 0.4 loc: a
        # handful of the 677 S samples), the fp32 error of loc, 1e-6, is 1e-4 of the sample, and of every record that carries the sample as a
        # factor: the emulation reached 0.43 of the record's bound there (NOTEBOOK)
        Wo = rng.standard_normal((2, w)) / math.sqrt(w)
        Wo *= (np.array([1.0, 0.4]) / np.maximum(np.abs(H @ Wo.T).max(0), 1e-30))[:, None]
        flat += [Wo.astype(F32).ravel(), np.array([2.5, -2.3], F32)]
    return (X if full else X[:n_all]), np.concatenate(flat).astype(F32)      # full: all the rows the layers were scaled on (a case of n < 64)


def forward(X, mlp, d, w, L, head, bij_kind, eps):
    """fp64 forward with bounds: SimpleNamespace(H [L + 1] (H[0] = X), Z [L], E [L + 1] bounds of H, slope [L], near (count of pre-activations inside
    their bound), loc, sig, dsd as (value, bound))"""
    layers, hd = unpack(mlp, d, w, L, head)
    f = SimpleNamespace(H=[RW.f64(X)], E=[None], Z=[], slope=[], near=0, layers=layers, head=hd, minpos=1.0)
    for (Wt, b) in layers:
        y, bound, z = RW.dense_forward(f.H[-1], Wt, b, LEAK, 1, eX=f.E[-1])
        s = RW.slope(z, LEAK)
        f.near += int(np.count_nonzero(np.abs(z) <= bound))
        pos = float(np.mean(z > 0))
        f.minpos = min(f.minpos, pos, 1.0 - pos)
        f.H.append(y), f.Z.append(z), f.slope.append(s), f.E.append(bound * s)
    if head:
        hf = RW.head_forward(f.H[-1], hd, bij_kind, eps, eH=f.E[-1])
        f.loc, f.sig, f.dsd = hf["loc"], hf["sig"], hf["dsd"]
    return f


# (waves of a workgroup, rows of a wave's tile) of the kernel a case runs on
WAVES = {"mlp": (EV11_WAVES, 16), "lane": (4, 64), "narrow": (8, 32)}


def partition(c, npos, grid_eff, ntiles):
    """(workgroup, wave) of every position.  elbo_mlp.hip: 128-row tiles strided over the grid (the packed layout: one contiguous range of tiles
    per workgroup), wave = the tile's 16-row slice.  The lane and narrow kernels: wave tiles strided over ALL waves of the launch, in either layout."""
    pos = np.arange(npos)
    nw, wt = WAVES[c.kernel]
    if c.kernel != "mlp":
        gw = (pos // wt) % (grid_eff * nw)
        return gw // nw, gw % nw
    tile_of = pos // TILE
    wg_of = tile_of % grid_eff
    if c.packed:                                                        # tile t belongs to the g with g nt / G <= t < (g + 1) nt / G (integer division)
        begin = np.array([g * ntiles // grid_eff for g in range(grid_eff + 1)])
        wg_of = np.searchsorted(begin, tile_of, side="right") - 1
    return wg_of, (pos % TILE) // 16


def packed_layout(c, seed):
    """positions of a packed layout by the header's contract: groups of 1 .. 16 rows inside 16-row granules (ref_rows.groups_layout), padding
    positions with refl_id = -1, the whole padded to tiles; the caller's rows are a permutation of the active positions"""
    refl, gmeta, start, R = RR.groups_layout(c.n, seed)
    n_pad = (len(refl) + TILE - 1) // TILE * TILE
    pad = n_pad - len(refl)
    refl, gmeta, start = np.concatenate([refl, np.full(pad, -1, np.int32)]), np.concatenate([gmeta, np.zeros(pad, np.int32)]), np.concatenate([start, np.full(pad, -1, np.int64)])
    return refl, gmeta, start, R, n_pad


def make_inputs(c, seed=0):
    """the operands of a case as float32 / int32 arrays over POSITIONS (rows of meta_t: the caller's rows in the plain layout, packed positions in the
    packed one) and the scalars of the argument block"""
    rng = np.random.default_rng([32, seed, c.n, c.d, c.w, c.L, c.S])
    x = SimpleNamespace(case=c, seed=seed, d=c.d, w=c.w, L=c.L, S=c.S, head=c.head, kind=c.lik, dof=F32(DOF), lik_const=RR.lik_const(c.lik, DOF),
                        bij_kind=RW.BIJ_EXP if c.bij == "exp" else RW.BIJ_SOFTPLUS, eps=F32(1e-3), shift=F32(0.37 if c.bij == "softplus" else 0.0),
                        w_ll=F32(1.0 / c.S), obs_offset=OBS_OFFSET, grid=c.grid)
    if c.packed:
        x.refl_id, gmeta, start, x.R, x.n_pad = packed_layout(c, seed)
        x.np_ = x.n_pad                                               # positions
        x.act = x.refl_id >= 0
        x.row_map = np.full(x.np_, -1, np.int32)
        x.row_map[x.act] = rng.permutation(c.n).astype(np.int32)
        x.gmeta = gmeta if c.groups else None
        x.slot = np.where(x.act, start, np.arange(x.np_)) if c.groups else None
        x.count = x.act & ((gmeta & 0xff) == 0) if c.groups else x.act.copy()
        x.tile_gmax = (gmeta >> 8).reshape(-1, TILE).max(1).astype(np.int32) if c.groups else None
        x.n_obs = x.n_pad
    else:
        x.np_ = x.n_obs = c.n
        x.n_pad = (c.n + TILE - 1) // TILE * TILE
        x.R = max(2, c.n // 7 + 2)
        x.refl_id = rng.integers(0, x.R - 1, c.n).astype(np.int32)      # (reflection R - 1 has no rows)
        x.act = np.ones(c.n, bool)
        x.row_map, x.gmeta, x.slot, x.tile_gmax, x.count = None, None, None, None, x.act.copy()
    x.n = c.n                                                            # the caller's rows
    x.krow = np.where(x.act, x.row_map, 0).astype(np.int64) if c.packed else np.arange(c.n)
    Xa, x.mlp = scaler_problem(seed, int(x.act.sum()), c.d, c.w, c.L, c.head)
    x.X = np.zeros((x.np_, c.d), F32)
    x.X[x.act] = Xa                                                      # (padding positions: metadata 0)
    x.meta_t = np.zeros((meta_rows(c.d), x.n_pad), F32)
    x.meta_t[:c.d, :x.np_] = x.X.T
    x.fw = forward(x.X, x.mlp, c.d, c.w, c.L, c.head, x.bij_kind, float(x.eps))
    x.P = param_count(c.d, c.w, c.L, c.head)
    x.ntiles = x.n_pad // TILE
    x.grid_eff = min(c.grid, x.ntiles)
    # a workgroup's tiles: strided over the grid in the plain layout, ONE contiguous range in the packed one (image changes are then rare)
    wg_of, x.wave_of = partition(c, x.np_, x.grid_eff, x.ntiles)
    x.wg_of = wg_of
    x.wg_rows = [np.flatnonzero((wg_of == g) & x.act) for g in range(x.grid_eff)]
    if c.mode == 1:
        return x
    if c.mode == 2:
        if c.head:
            x.dO = np.zeros((c.n, 2), F32)
            x.dO[:] = RW.normals(rng, c.n, 2) * F32(0.7)
        else:
            x.dH = np.zeros((meta_rows(c.w), x.n_pad), F32)
            if c.kernel != "mlp":                                       # dH_ext is read below n_obs and in the rows < w only: numbers a launch must not use everywhere else
                x.dH[:] = F32(1e3)
            x.dH[:c.w, :x.np_] = (RW.normals(rng, c.w, x.np_) * F32(0.7)) * x.act
        x.grad_pre = None
        return x
    # ---- the likelihood's operands (mode 0) ----
    S, n = c.S, c.n
    x.z_f = (np.abs(rng.standard_normal((x.R, S))) + 0.3).astype(F32)
    x.eta = rng.standard_normal((n, S)).astype(F32)
    x.n_images = 1
    if c.img != "off":
        # image borders inside a wave's 16 rows (runs of 5 .. 11 rows), image 0 (pinned) among them; unsorted: a permutation of the same ids
        runs = rng.integers(5, 12, x.np_)
        ids = np.repeat(np.arange(len(runs)), runs)[:x.np_]
        x.image_id = (rng.permutation(ids) if c.img == "unsorted" else ids).astype(np.int32)
        x.n_images = int(ids.max()) + 2                                  # (the last image has no rows)
        x.img = (10 ** rng.uniform(-0.3, 0.3, x.n_images - 1)).astype(F32)
    else:
        x.image_id = x.img = None
    x.ev11 = np.array(RR.EV11_RAW, F32) if c.ev11 else None
    x.noise_row = (OBS_OFFSET + 17 + rng.permutation(x.np_)).astype(np.int32) if c.noise_row else None
    x.det_slot = None
    if c.det_slot:                                                       # the caller's reflection-sorted position of every row
        rid_rows = np.zeros(n, np.int64)
        rid_rows[x.krow[x.act]] = x.refl_id[x.act]
        order = np.argsort(rid_rows, kind="stable")
        x.det_slot = np.empty(n, np.int32)
        x.det_slot[order] = np.arange(n, dtype=np.int32)
    finish_likelihood(x, rng)
    return x


def finish_likelihood(x, rng=None):
    """iobs / sig from the fp64 prediction (no accidental fit: ref_rows.make_inputs), the preloads of the accumulating outputs from the summand sizes"""
    c = x.case
    rng = rng or np.random.default_rng([33, x.seed, c.n])
    x.eta_row = np.zeros((x.np_, c.S), F32)
    x.eta_row[x.act] = x.eta[x.krow[x.act]]
    xx = rows_view(x, iobs=np.zeros(x.np_, F32), sig=np.ones(x.np_, F32))
    ip = RR.reference(xx, values_only=True).iconv
    io = (ip[:, 0] * (1.0 + 0.4 * rng.standard_normal(x.np_)) + 0.2 * rng.standard_normal(x.np_)).astype(F32)
    io = np.where(np.any(np.abs(ip - io.astype(np.float64)[:, None]) < 1e-2 * (np.abs(ip) + np.abs(io.astype(np.float64))[:, None]), axis=1), io * F32(2), io)
    sg = ((0.1 * np.abs(io) + 0.1) * 10 ** rng.uniform(-0.5, 0.5, x.np_)).astype(F32)
    if x.slot is not None:
        io, sg = io[x.slot], sg[x.slot]                                  # the group's observation on every member row
    x.iobs, x.sig = np.where(x.act, io, F32(0)).astype(F32), np.where(x.act, sg, F32(1)).astype(F32)


def rows_view(x, iobs=None, sig=None):
    """the operands of ref_rows.reference over the positions: (loc, sigma) the fp64 scaler outputs"""
    return SimpleNamespace(n=x.np_, S=x.S, R=x.R, refl_id=x.refl_id, image_id=x.image_id, img=x.img, aim=None, slot=x.slot, count=x.count,
                           loc=x.fw.loc[0], sigma=x.fw.sig[0], iobs=x.iobs if iobs is None else iobs, sig=x.sig if sig is None else sig, z_f=x.z_f,
                           eta_row=x.eta_row, kind=x.kind, dof=x.dof, shift=x.shift, w_ll=x.w_ll, ev11=x.ev11, lik_const=x.lik_const)


def case_seed(c, tries=40):
    """the first seed whose case holds no pre-activation inside its own propagated rounding bound -- found from the reference alone"""
    for s in range(tries):
        n_act = c.n
        X, mlp = scaler_problem(s, n_act, c.d, c.w, c.L, c.head)
        if forward(X, mlp, c.d, c.w, c.L, c.head, 0, 1e-3).near == 0:
            return s
    raise AssertionError(f"{c.id}: no seed in [0, {tries}) without a pre-activation inside its rounding bound")


# ---- the fp64 reference ----------------------------------------------------------------------------------------------------------------------
def backward(x, g0=None, g1=None, M0=None, M1=None, dH=None, MH=None):
    """the Dense stack's backward pass per position: dZ [L], M_dZ [L] (the chain rule on absolute values), the head's (g0, g1); dX, M_dX"""
    f = x.fw
    b = SimpleNamespace(g0=g0, g1=g1, M0=M0, M1=M1)
    if dH is None:
        Wo = RW.f64(f.head)[:2 * x.w].reshape(2, x.w)
        dH = g0[:, None] * Wo[0] + g1[:, None] * Wo[1]
        MH = M0[:, None] * np.abs(Wo[0]) + M1[:, None] * np.abs(Wo[1])
    b.dZ, b.MZ = [None] * x.L, [None] * x.L
    for l in range(x.L - 1, -1, -1):
        b.dZ[l], b.MZ[l] = dH * f.slope[l], MH * f.slope[l]
        Wt = RW.f64(f.layers[l][0])
        dH, MH = b.dZ[l] @ Wt, b.MZ[l] @ np.abs(Wt)
    b.dX, b.MX = dH, MH
    return b


def param_grad(x, b, rows):
    """flat (gradient, M) of the scaler parameters over the positions `rows`, in the W^T layout"""
    f, g, M = x.fw, [], []
    for l in range(x.L):
        dz, mz, h = b.dZ[l][rows], b.MZ[l][rows], f.H[l][rows]
        g += [(dz.T @ h).ravel(), dz.sum(0)]
        M += [(mz.T @ np.abs(h)).ravel(), mz.sum(0)]
    if x.head:
        h = f.H[-1][rows]
        g += [b.g0[rows] @ h, b.g1[rows] @ h, [b.g0[rows].sum(), b.g1[rows].sum()]]
        M += [b.M0[rows] @ np.abs(h), b.M1[rows] @ np.abs(h), [b.M0[rows].sum(), b.M1[rows].sum()]]
    return np.concatenate([np.asarray(v, np.float64).ravel() for v in g]), np.concatenate([np.asarray(v, np.float64).ravel() for v in M])


def tensor_slices(x):
    """[(name, slice)] of the gradient tensors inside the flat scaler gradient"""
    out, o = [], 0
    for l in range(x.L):
        k = x.d if l == 0 else x.w
        out += [(f"dW{l}", slice(o, o + x.w * k)), (f"db{l}", slice(o + x.w * k, o + x.w * k + x.w))]
        o += x.w * k + x.w
    if x.head:
        out += [("dWo", slice(o, o + 2 * x.w)), ("dbo", slice(o + 2 * x.w, o + 2 * x.w + 2))]
    return out


def reference(x):
    """fp64 value and bound / summand size of every output of the case's launch (module docstring)"""
    c, f = x.case, x.fw
    r = SimpleNamespace(near=f.near)
    if c.mode == 1:
        return r
    if c.mode == 2:
        if c.head:
            dO = np.zeros((x.np_, 2))
            dO[x.act] = RW.f64(x.dO)[x.krow[x.act]]
            g1 = dO[:, 1] * f.dsd[0]
            r.b = backward(x, dO[:, 0], g1, np.abs(dO[:, 0]), np.abs(g1))
        else:
            dH = RW.f64(x.dH)[:x.w, :x.np_].T
            r.b = backward(x, dH=dH, MH=np.abs(dH))
    else:
        xx = rows_view(x)
        r.rows = RR.reference(xx)
        rr = r.rows
        g1, M1 = rr.dO[:, 1] * f.dsd[0], rr.M_dO[:, 1] * np.abs(f.dsd[0])
        r.b = backward(x, rr.dO[:, 0], g1, rr.M_dO[:, 0], M1)
        # the deterministic records: per (row, sample) the row's own share of dz_f (ref_rows: gbuf), per row dNLL / d(image scale)
        tq = f.loc[0][:, None] + f.sig[0][:, None] * RW.f64(x.eta_row) + float(x.shift)
        z = RW.f64(x.z_f)[np.where(x.act, x.refl_id, 0)]
        sl = np.arange(x.np_) if x.slot is None else np.asarray(x.slot, np.int64)
        a2 = x.act[:, None]
        r.dimg_row, r.M_dimg_row = (rr.dconv[sl] * tq * z * z * a2).sum(1), (rr.M_dconv[sl] * np.abs(tq) * z * z * a2).sum(1)
        r.parts = []
        for rows in x.wg_rows:                                           # a workgroup's NLL (and, per wave, its Evans-2011 terms): the counted rows masked
            sub = copy.copy(xx)
            m = np.zeros(x.np_, bool)
            m[rows] = True
            sub.count = xx.count & m
            r.parts.append(RR.reference(sub))
    r.grad, r.M_grad = param_grad(x, r.b, np.flatnonzero(x.act))
    r.part = [param_grad(x, r.b, rows) for rows in x.wg_rows]
    return r


def ev11_wave_reference(x, g, wv):
    """d_ev11 (value, M) of wave wv of workgroup g: the rows 16 wv .. 16 wv + 15 of each of its tiles"""
    xx = rows_view(x)
    m = np.zeros(x.np_, bool)
    rows = x.wg_rows[g]
    m[rows[x.wave_of[rows] == wv]] = True
    sub = copy.copy(xx)
    sub.count = xx.count & m
    if not sub.count.any():
        return np.zeros(3), np.zeros(3)
    rr = RR.reference(sub)
    return rr.d_ev11, rr.M_ev11


_REFS = {}


def reference_for(c):
    """(inputs, reference) of a case at its searched seed, computed once per process and shared (read-only)"""
    if c.id not in _REFS:
        x = make_inputs(c, case_seed(c))
        _REFS[c.id] = (x, reference(x))
    return _REFS[c.id]


def preloads(x, ref):
    """what the accumulating outputs hold in front of the launch: a tenth of the entry's summand size (a store in place of an add stays visible)"""
    rng = np.random.default_rng([34, x.seed, x.case.n])
    sgn = lambda shape: np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    load = lambda M: (np.where(M > 0.0, 0.1 * M, 0.75) * sgn(np.shape(M))).astype(F32)      # (an entry nothing is added to: a number whose bits an added 0.0 keeps)
    p = SimpleNamespace(grad=load(ref.M_grad))
    if x.case.mode == 0:
        rr = ref.rows
        p.dz, p.nll = load(rr.M_dz), 0.1 * rr.M_nll
        p.d_img = load(rr.M_img) if x.img is not None else None
        p.d_ev11 = load(rr.M_ev11) if x.ev11 is not None else None
    return p


# ---- bounds ----------------------------------------------------------------------------------------------------------------------------------
def ratios(x, ref, pre, got):
    """{quantity: largest error / bound} of a launch's result `got` (attributes as in `emulate`'s result; None / absent: not checked)"""
    c, f, out = x.case, x.fw, {}
    have = lambda k: getattr(got, k, None) is not None
    act_rows = x.krow[x.act]
    if have("loc"):
        out["loc_out"] = RR._worst(np.abs(RW.f64(got.loc)[act_rows] - f.loc[0][x.act]), f.loc[1][x.act])
        out["sig_out"] = RR._worst(np.abs(RW.f64(got.sig)[act_rows] - f.sig[0][x.act]), f.sig[1][x.act])
    if have("act"):
        out["act_out"] = RR._worst(np.abs(RW.f64(got.act)[:x.w, :x.np_].T - f.H[-1]), f.E[-1])
    wide = True
    if c.mode == 0:
        rr = ref.rows
        if have("nll"):
            out["nll"] = abs(got.nll - rr.nll) / (RTOL_LOSS * max(rr.M_nll, 1.0))
        if have("ipred"):
            out["ipred_out"] = RR._worst(np.abs(RW.f64(got.ipred)[act_rows] - rr.ipred[x.act]), RTOL_LOSS * rr.M_ipred[x.act])
        has_rows = np.bincount(x.refl_id[x.act], minlength=x.R) > 0
        if have("dz"):
            RR._grad(out, "dz_f", got.dz, rr.dz, rr.M_dz, pre.dz, wide, sel=has_rows)
            if not np.array_equal(np.asarray(got.dz)[~has_rows].view(np.uint32), pre.dz[~has_rows].view(np.uint32)):
                out["dz_f"] = np.inf                                    # a reflection without rows keeps its bits
        if have("d_img"):
            present = np.zeros(len(x.img), bool)
            ids = np.unique(x.image_id[x.act])
            present[ids[ids > 0] - 1] = True
            RR._grad(out, "d_img", got.d_img, rr.d_img, rr.M_img, pre.d_img, wide, sel=present)
            if not np.array_equal(np.asarray(got.d_img)[~present].view(np.uint32), pre.d_img[~present].view(np.uint32)):
                out["d_img"] = np.inf
        if have("d_ev11"):
            RR._grad(out, "d_ev11", got.d_ev11, rr.d_ev11, rr.M_ev11, pre.d_ev11, False)
        if have("dzf_obs"):                                             # records in the caller's row order, or at det_slot
            rec = np.asarray(got.dzf_obs)
            at = act_rows if x.det_slot is None else x.det_slot[act_rows]
            RR._grad(out, "dzf_obs", rec[at], rr.gbuf[x.act], rr.M_gbuf[x.act], None, wide)
        if have("dimg_obs"):
            RR._grad(out, "dimg_obs", np.asarray(got.dimg_obs)[act_rows], ref.dimg_row[x.act], ref.M_dimg_row[x.act], None, wide)
        if have("nll_part"):
            # a workgroup's NLL is an NLL and a deterministic record: the tighter of the two bars (RTOL_LOSS max(M, 1) above M = 1, the records' below)
            q = [abs(float(got.nll_part[g]) - p.nll) / min(RTOL_LOSS * max(p.M_nll, 1.0), RTOL_GRAD * p.M_nll + U * abs(p.nll)) if p.M_nll > 0.0 else
                 (0.0 if float(got.nll_part[g]) == 0.0 else np.inf) for g, p in enumerate(ref.parts[:x.grid_eff])]
            out["nll_part"] = max(q)                                    # (the slots behind the clamped grid: untouched, the harness's mask)
        if have("ev11_part"):
            worst = 0.0
            parts = np.asarray(got.ev11_part, np.float64).reshape(-1, 3)
            for g in range(x.grid_eff):
                for wv in range(EV11_WAVES):
                    v, M = ev11_wave_reference(x, g, wv)
                    o = {}
                    RR._grad(o, "e", parts[EV11_WAVES * g + wv], v, np.maximum(M, 1e-300), None, False)
                    worst = max(worst, o["e"])
            out["ev11_part"] = worst
    if have("partials"):
        parts = np.asarray(got.partials, np.float64).reshape(-1, x.P)
        worst = 0.0
        for g in range(x.grid_eff):
            v, M = ref.part[g]
            worst = max(worst, RR._worst_grad(np.abs(parts[g] - v), M, v))
        out["partials"] = worst
        tot = parts[:x.grid_eff].sum(0)
        out["partials sum"] = RR._worst_grad(np.abs(tot - ref.grad), ref.M_grad, ref.grad)
        for name, s in tensor_slices(x):
            if np.max(np.abs(ref.grad[s])) > 0.0:
                out["max-norm " + name[:2].rstrip("0123456789")] = max(out.get("max-norm " + name[:2].rstrip("0123456789"), 0.0),
                                                                       float(np.max(np.abs(tot[s] - ref.grad[s])) / np.max(np.abs(ref.grad[s])) / RTOL_GRAD))
    if have("grad"):                                                    # behind cl_reduce_partials, on top of the preload
        stored = RW.f64(pre.grad) + ref.grad
        out["reduced grad"] = RR._worst_grad(np.abs(RW.f64(got.grad) - stored), ref.M_grad, stored)
    if have("dz0"):                                                     # dL/d(pre-activations of layer 0), feature-major, every element below n_obs
        dz0 = RW.f64(got.dz0)[:x.w, :x.np_].T
        out["dZ0_out"] = RR._worst_grad(np.abs(dz0 - ref.b.dZ[0]), ref.b.MZ[0], ref.b.dZ[0])
    if have("dX"):
        dX = RW.f64(got.dX)[:x.d, :x.np_].T
        out["dX_out"] = RR._worst_grad(np.abs(dX - ref.b.dX), ref.b.MX, ref.b.dX)
        if np.max(np.abs(ref.b.dX)) > 0:
            out["max-norm dX"] = float(np.max(np.abs(dX - ref.b.dX)) / np.max(np.abs(ref.b.dX)) / RTOL_GRAD)
    return out


# ---- fp32 emulation ----------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("rows_behind_n_obs_counted", "last_tile_left_out_of_wgrad", "wg1_partial_to_row_0", "bias_gradient_of_feature_15_dropped", "slope_at_zero_is_one",
           "head_rows_swapped_in_backward", "image_0_not_pinned", "shift_outside_image_scale", "second_sample_dropped", "eta_read_as_S_n",
           "obs_offset_left_out_of_noise_key", "w_ll_lost", "dX_without_first_layer_mask", "act_out_row_major", "group_sum_over_tile_gmax",
           "det_slot_not_times_S")
# ... of the lane and narrow kernels' launches (tests/ref_lane.py, tests/test_ref_lane.py)
LANE_MUTANTS = ("rows_behind_n_obs_counted", "second_wave_tile_skipped", "ninth_sample_dropped", "head_wgrad_from_one_wave", "dz0_without_first_slope",
                "tile_shares_a_reflection_by_store", "dH_ext_read_behind_n_obs")


def _mm(a, b):
    return np.matmul(np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32))          # fp32 in numpy's (BLAS) order: any order is inside the bound


def _wg(x, npos, act):
    wg_of = x.wg_of if npos == x.np_ else partition(x.case, npos, x.grid_eff, x.ntiles)[0]      # (more positions: the plain layout's padding rows)
    return [np.flatnonzero((wg_of == g) & act) for g in range(x.grid_eff)]


def emulate(x, hm, pre, mutant=None, eta_shifted=None):
    """the launch in numpy float32 with the scalar functions of the host build of csrc/cl_math.h (tests/host_math_check.cpp); `mutant`: one of
    MUTANTS, a kernel that is wrong in one place.  eta_shifted: the normals a kernel that forgot obs_offset would draw (in-kernel noise)."""
    c, S, npos = x.case, x.S, x.np_
    layers, head = unpack(x.mlp, x.d, x.w, x.L, x.head)
    act = x.act.copy()
    X = x.X.copy()
    if mutant in ("rows_behind_n_obs_counted", "dH_ext_read_behind_n_obs") and not c.packed:      # the padding rows of the last tile take part (metadata 0)
        npos = x.n_pad
        X = np.zeros((npos, x.d), F32)
        X[:x.np_] = x.X
        act = np.ones(npos, bool)
    H, Z = [X], []
    for (Wt, b) in layers:
        z = _mm(H[-1], Wt.T) + b
        Z.append(z)
        H.append(np.where(z > 0, z, F32(LEAK) * z).astype(F32))
    slope = [np.where(z > 0, F32(1), F32(LEAK)) for z in Z]
    if mutant == "slope_at_zero_is_one":
        slope = [np.where(z >= 0, F32(1), F32(LEAK)) for z in Z]
    got = SimpleNamespace()
    krow = np.arange(npos) if not c.packed else x.krow
    if x.head:
        Wo, bo = head[:2 * x.w].reshape(2, x.w), head[2 * x.w:]
        raw = _mm(H[-1], Wo.T) + bo
        sig, dsd = np.empty(npos, F32), np.empty(npos, F32)
        hm.hm_bij(npos, fp(np.ascontiguousarray(raw[:, 1])), int(x.bij_kind), ctypes.c_float(float(x.eps)), fp(sig), fp(dsd))
        loc = np.ascontiguousarray(raw[:, 0])
    if c.mode == 1:
        if x.head:
            got.loc, got.sig = np.full(x.n, SENT, F32), np.full(x.n, SENT, F32)
            got.loc[krow[x.act]], got.sig[krow[x.act]] = loc[:x.np_][x.act], sig[:x.np_][x.act]
        else:
            got.act = np.zeros((meta_rows(x.w), x.n_pad), F32)
            if mutant == "act_out_row_major":
                flat = got.act.reshape(-1)
                hh = H[-1][:x.np_]
                flat[:hh.size] = hh.ravel()
            else:
                got.act[:x.w, :x.np_] = H[-1][:x.np_].T
        return got
    rid = np.zeros(npos, np.int64)
    rid[:x.np_] = np.where(x.act, x.refl_id, 0)
    if c.mode == 0:
        eta = np.zeros((npos, S), F32)
        src = x.eta if eta_shifted is None or mutant != "obs_offset_left_out_of_noise_key" else eta_shifted
        if mutant == "eta_read_as_S_n":
            src = np.ascontiguousarray(src.reshape(S, -1).T)
        eta[:x.np_][x.act] = src[x.krow[x.act]]
        zf = x.z_f[rid]
        aim = np.ones(npos, F32)
        imgid = np.zeros(npos, np.int64)
        if x.img is not None:
            imgid[:x.np_] = x.image_id
            table = np.concatenate([[F32(1)], x.img]).astype(F32)
            if mutant == "image_0_not_pinned":
                table = np.concatenate([x.img[:1], x.img]).astype(F32)
            aim = table[imgid]
        io, sg = np.zeros(npos, F32), np.ones(npos, F32)
        io[:x.np_], sg[:x.np_] = x.iobs, x.sig
        if mutant == "rows_behind_n_obs_counted":
            io[x.np_:], sg[x.np_:] = F32(0), F32(1)
        shift = F32(x.shift)
        if mutant == "shift_outside_image_scale":
            tq = loc[:, None] + sig[:, None] * eta
            zs = aim[:, None] * tq + shift
            tq = tq + shift
        else:
            tq = loc[:, None] + sig[:, None] * eta + shift
            zs = aim[:, None] * tq
        ipred = (zs * zf * zf * act[:, None]).astype(F32)
        tot, cnt = ipred, act.copy()
        if x.slot is not None:
            sl = np.asarray(x.slot, np.int64)
            tot = np.zeros_like(ipred)
            if mutant == "group_sum_over_tile_gmax":                   # every member adds tile_gmax lanes from its group's first one
                first = np.where(x.act, sl, np.arange(npos))
                gm = x.tile_gmax[np.arange(npos) // TILE]
                for m in range(int(gm.max())):
                    idx = np.minimum(first + m, npos - 1)
                    ok = (m < gm) & ((first + m) // 16 == first // 16)
                    tot += np.where(ok[:, None], ipred[idx], F32(0))
            else:
                np.add.at(tot, sl, ipred)
                tot = tot[sl]
            cnt = x.count
        w_ll = F32(1) if mutant == "w_ll_lost" else F32(x.w_ll)
        flat = lambda a: np.ascontiguousarray(np.broadcast_to(a, (npos, S)), F32).ravel()
        ll, dll, gf, ga, gb = RR.lik32(hm, x, tot.ravel(), flat(io[:, None]), flat(sg[:, None]), 1)
        ll, dll = ll.reshape(npos, S), dll.reshape(npos, S)
        live = act[:, None] & np.ones((1, S), bool)
        if mutant == "second_sample_dropped":                          # a lane's samples s and s + 4: the second one never evaluated
            live = live & (np.arange(S)[None, :] < 4)
        if mutant == "ninth_sample_dropped":                           # the lane kernel's batches of eight samples: the second batch one short
            live = live & (np.arange(S)[None, :] != 8)
        nll_rows = -(np.where(live & cnt[:, None], ll, F32(0)) * w_ll).astype(np.float64).sum(1)
        gi = np.where(live, -dll * w_ll, F32(0)).astype(F32)
        rec = (gi * zs * F32(2) * zf).astype(F32)
        dzs = gi * zf * zf
        dt = dzs * aim[:, None]
        pdl, pds, pda = dt.sum(1, dtype=F32), (dt * eta).sum(1, dtype=F32), (dzs * tq).sum(1, dtype=F32)
        g0, g1 = pdl, (pds * dsd).astype(F32)
        if c.ipred:
            got.ipred = np.full((x.n, S), SENT, F32)
            got.ipred[krow[:x.np_][x.act]] = ipred[:x.np_][x.act]
        wg = _wg(x, npos, act)
        got.nll_part = np.array([nll_rows[r].sum() for r in wg] + [0.0] * (c.grid - x.grid_eff))
        got.nll = float(got.nll_part.sum())
        if c.det:
            got.dzf_obs = np.full((x.n, S), SENT, F32)
            rows = x.krow[x.act]
            if x.det_slot is not None:
                if mutant == "det_slot_not_times_S":
                    flat_rec = got.dzf_obs.reshape(-1)
                    for i, r_ in zip(np.flatnonzero(x.act), rows):
                        flat_rec[x.det_slot[r_]:x.det_slot[r_] + S] = rec[i]
                else:
                    got.dzf_obs[x.det_slot[rows]] = rec[:x.np_][x.act]
            else:
                got.dzf_obs[rows] = rec[:x.np_][x.act]
            if x.img is not None:
                got.dimg_obs = np.full(x.n, SENT, F32)
                got.dimg_obs[rows] = pda[:x.np_][x.act]
        else:
            got.dz = pre.dz.copy()
            add = act
            if mutant == "tile_shares_a_reflection_by_store":          # the rows of one wave tile that share a reflection: the last one's record alone arrives
                key = (np.arange(npos) // WAVES[c.kernel][1]) * x.R + rid
                last = np.zeros(npos, bool)
                last[npos - 1 - np.unique(key[::-1], return_index=True)[1]] = True
                add = act & last
            np.add.at(got.dz, (rid[add][:, None], np.arange(S)[None, :]), rec[add])
            if x.img is not None:
                got.d_img = pre.d_img.copy()
                if mutant == "image_0_not_pinned":
                    np.add.at(got.d_img, np.maximum(imgid[act] - 1, 0), pda[act])
                else:
                    m = act & (imgid > 0)
                    np.add.at(got.d_img, imgid[m] - 1, pda[m])
        if x.ev11 is not None:
            sgm = RR.sigmoid32(hm, x.ev11)
            e = np.stack([-(np.where(live & cnt[:, None], v.reshape(npos, S), F32(0)) * w_ll).sum(1, dtype=F32) for v in (gf, ga, gb)], 1)      # Sdfac, Sdadd, SdB
            if c.det:
                wave_of = partition(c, npos, x.grid_eff, x.ntiles)[1]
                got.ev11_part = np.zeros((EV11_WAVES * c.grid, 3), F32)
                for g, r in enumerate(wg):
                    for wv in range(EV11_WAVES):
                        got.ev11_part[EV11_WAVES * g + wv] = e[r[wave_of[r] == wv]].sum(0, dtype=F32) * sgm
                got.ev11_part = got.ev11_part.ravel()
            else:
                got.d_ev11 = (pre.d_ev11 + e[act].sum(0, dtype=F32) * sgm).astype(F32)
    elif x.head:
        dO = np.zeros((npos, 2), F32)
        dO[:x.np_][x.act] = x.dO[x.krow[x.act]]
        g0, g1 = np.ascontiguousarray(dO[:, 0]), (dO[:, 1] * dsd).astype(F32)
        wg = _wg(x, npos, act)
    else:
        wg = _wg(x, npos, act)
    # ---- backward ----
    if x.head:
        if mutant == "head_rows_swapped_in_backward":
            dH = g0[:, None] * Wo[1] + g1[:, None] * Wo[0]
        else:
            dH = g0[:, None] * Wo[0] + g1[:, None] * Wo[1]
    else:
        dH = np.zeros((npos, x.w), F32)
        dH[:x.np_] = x.dH[:x.w, :x.np_].T
        if mutant == "dH_ext_read_behind_n_obs":                       # a block's backward launch that reads whole wave tiles of dH_ext
            dH[:] = x.dH[:x.w, :npos].T
    dZ = [None] * x.L
    for l in range(x.L - 1, -1, -1):
        dZ[l] = (dH * slope[l]).astype(F32)
        dH0 = dH                                                       # (behind the loop: dL/d(activations of layer 0))
        if l == 0 and mutant == "dX_without_first_layer_mask":
            dH = _mm(dH, layers[0][0])
        else:
            dH = _mm(dZ[l], layers[l][0])
    if c.dz0:
        got.dz0 = np.zeros((meta_rows(x.w), x.n_pad), F32)
        got.dz0[:x.w, :x.np_] = (dH0 if mutant == "dz0_without_first_slope" else dZ[0])[:x.np_].T
    if c.dX:
        got.dX = np.zeros((meta_rows(x.d), x.n_pad), F32)
        got.dX[:x.d, :x.np_] = dH[:x.np_].T
    parts = np.zeros((c.grid, x.P), F32)
    for g, rows in enumerate(wg):
        if mutant == "last_tile_left_out_of_wgrad" and len(rows):
            rows = rows[rows // TILE != (rows // TILE).max()] if len(np.unique(rows // TILE)) > 1 else rows[:0]
        hrows = rows
        if mutant in ("second_wave_tile_skipped", "head_wgrad_from_one_wave"):
            nw, wt = WAVES[c.kernel]
            if mutant == "second_wave_tile_skipped":                   # wave tiles are strided over all waves of the launch: every wave's second one
                rows = rows[(rows // wt) // (x.grid_eff * nw) != 1]
                hrows = rows
            else:                                                      # the head's per-wave sums: wave 0's alone
                hrows = rows[((rows // wt) % (x.grid_eff * nw)) % nw == 0]
        v = []
        for l in range(x.L):
            db = dZ[l][rows].sum(0, dtype=F32)
            if mutant == "bias_gradient_of_feature_15_dropped" and l > 0 and x.w <= 15:
                # padded feature 15 carries the WHOLE bias gradient of a hidden layer (column 15 of the dW^T accumulator): the quiet form of the
                # fault is one wave's column left out of the flush -- the rows 112 .. 127 of every tile
                db = dZ[l][rows[(rows % TILE) // 16 != 7]].sum(0, dtype=F32)
            v += [_mm(dZ[l][rows].T, H[l][rows]).ravel(), db]
        if x.head:
            v += [_mm(g0[hrows][None, :], H[-1][hrows]).ravel(), _mm(g1[hrows][None, :], H[-1][hrows]).ravel(), np.array([g0[hrows].sum(dtype=F32), g1[hrows].sum(dtype=F32)], F32)]
        row = 0 if (mutant == "wg1_partial_to_row_0" and g == 1) else g
        parts[row] = np.concatenate(v)
    got.partials = parts
    got.grad = (pre.grad + parts[:x.grid_eff].sum(0, dtype=F32)).astype(F32)
    return got
