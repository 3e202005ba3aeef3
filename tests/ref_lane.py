"""The launch layer of the lane-per-observation kernel (csrc/elbo_lane.hip) and the narrow kernel (csrc/elbo_narrow.hip) restated in Python from
their text, and the generated case list of the direct kernel tests (tests/test_lane_kernels_gpu.py).  Inputs, the fp64 reference, the bounds,
the preloads and the fp32 emulation are those of tests/ref_mlp.py, unchanged: a case of this file is a ref_mlp.case with `kernel` = "lane" or
"narrow" (the 64- / 32-row wave tiles strided over all waves of the launch: ref_mlp.partition) and, where asked, `dz0` (dZ0_out).

Restated (the library's cl_mlp_route / cl_mlp_kernel_name / cl_mlp_check are the OTHER side of every comparison):
    lane_supports, lane_block_supports, narrow_supports     cl_lane_supports, cl_lane_block_supports, cl_narrow_supports
    route                                                   the clauses of mlp_route that choose CL_ROUTE_LANE, _LANE_BLOCK and _NARROW
    lane_width, lane_form, lane_instance, narrow_instance   with_lane_width, launch_lane_form, launch_lane_reg / _rows / _block, launch_narrow_ks
Per-image layers (CL_ROUTE_LANE_IMGL) are not covered: the reference has no per-image layers and no packed-by-image layout.  Their instance names
are enumerated all the same (`enumerate_uncovered`), disjoint from the covered set, so that the gap is written down in code.
"""
from __future__ import annotations

import ctypes

import numpy as np

from tests import ref_mlp as RM
from tests import ref_rows as RR
from tests import ref_wide as RW

NL, WMAX, W12, DMAX_ALL, DMAX_LX, DEPTH_LO, DEPTH_WMIN = 20, 10, 12, 15, 31, 2, 5
IMGL_MAX, IMGL_MAX_NL, IMGL3_DEPTH_MAX = 2, 3, 18
N_INST = 17 * 64 + 37                                                  # eighteen 64-row wave tiles on eight waves: two take three, six two; the last ragged
DET_TAG = " (deterministic stores)"
TF = {False: "false", True: "true"}


# ---- the predicates ----------------------------------------------------------------------------------------------------------------------------
def wants_full(c):
    return c.noise == "eta" or c.ipred or c.ev11 or c.det


def depth_compiled(c):
    return c.L == NL or (DEPTH_LO <= c.L < NL and c.w >= DEPTH_WMIN)


def envelope(c, wmax, dmax):
    return 1 <= c.w <= wmax and 1 <= c.d <= dmax and depth_compiled(c) and not c.dX


def lane_supports(c):
    if c.lik == "laplace" or c.mode != 0 or not c.head:
        return False
    regs = 1 <= c.d <= DMAX_ALL
    if not (envelope(c, W12 if regs else WMAX, DMAX_LX) and c.S >= 1 and (c.packed or not c.groups)):
        return False
    if c.L != NL:
        return regs and not (c.dz0 and c.packed)
    if c.w > WMAX:
        return c.d <= 8
    return True                                                         # (the LDS rows of every width <= 10 on <= 31 columns fit the 160 KB: the sweep of test_ref_lane holds this to the library)


def narrow_supports(c):
    return (c.lik != "laplace" and c.mode == 0 and c.head and 1 <= c.w <= 15 and 1 <= c.d <= 15 and 1 <= c.L <= NL and not c.dX and (c.packed or not c.groups))


def lane_block_supports(c):
    if c.mode not in (1, 2) or c.head or c.det:
        return False
    return envelope(c, WMAX if c.L == NL else W12, DMAX_ALL) and c.w >= DEPTH_WMIN and not c.packed and not c.groups and not c.dz0


def route(c):
    """lane / lane_block / narrow, or None: another launcher's, or no route at all (`refused`)"""
    if c.mode == 0 and c.head and not c.dX:
        return "lane" if lane_supports(c) else ("narrow" if narrow_supports(c) else None)
    if not c.head and lane_block_supports(c):
        return "lane_block"
    return None


def refused(c):
    """dZ0_out off the kernels that store it: CL_ROUTE_NONE"""
    return c.dz0 and route(c) not in ("lane", "narrow")


# ---- the instances -----------------------------------------------------------------------------------------------------------------------------
def lane_width(w, widths):
    """the compile-time width that holds w: the smallest of the set"""
    return next(W for W in widths if w <= W)


def lane_name(W, DMAX, packed, full, dxo=False, NI=0, L=NL, mode=0):
    shown = 8 if mode else (7 if L != NL else (6 if NI else (5 if dxo else 4)))
    p = [str(W), str(DMAX), TF[packed], TF[full], TF[dxo], str(NI), str(L), str(mode)][:shown]
    return f"elbo_lane_kernel<{', '.join(p)}>" + (" (image layers)" if NI else "")


def lane_form(c, forms):
    """(FULL, DXO) of a unit that compiles `forms`: all (production, full, production + dZ_0), prod_full, full"""
    if forms == "full":
        return True, False
    full = wants_full(c) or (c.dz0 and forms != "all")
    if forms == "all" and c.dz0 and not full:
        return False, True
    return full, False


def lane_instance(c):
    if c.mode:                                                          # a head-less block
        W = lane_width(c.w, (8, 10, 12))
        return lane_name(W, 8 if (c.L == NL and c.d <= 8) else DMAX_ALL, False, False, L=c.L, mode=c.mode)
    if c.L != NL:
        W, DMAX, forms = lane_width(c.w, (8, 10, 12)), DMAX_ALL, "full" if c.packed else "all"
    elif c.d > DMAX_ALL:
        W, DMAX, forms = lane_width(c.w, (4, 6, 8, 10)), 0, "full" if c.packed else "prod_full"
    else:
        W, DMAX, forms = lane_width(c.w, (4, 6, 8, 10, 12)), (8 if c.d <= 8 else DMAX_ALL), "full" if c.packed else "all"
    full, dxo = lane_form(c, forms)
    return lane_name(W, DMAX, c.packed, full, dxo, L=c.L) + (DET_TAG if c.det else "")


def narrow_instance(c):
    m = max(c.w, c.d)
    return f"elbo_narrow_kernel<2, {2 if m <= 8 else (3 if m <= 12 else 4)}, 8, {TF[c.packed]}>" + (DET_TAG if c.det else "")


def expected_instance(c):
    r = route(c)
    return None if r is None else (narrow_instance(c) if r == "narrow" else lane_instance(c))


def enumerate_lane_instances():
    """{instance name: (kernel, W, DMAX or KS, packed, form, L, mode)} of every instance without per-image layers, from the rules above: the default
    depth (registers: 4 / 6 / 8 / 10 on 8 / 15 columns and 12 on 8, three plain forms, the packed full one; LDS rows: production and full, the packed
    full one; blocks of width 8 / 10), the depths 2 .. 19 (8 / 10 / 12 on 15 columns), the six narrow instances.  The deterministic stores are a
    run-time form of a full instance: no name of their own here, cases of their own in the list."""
    out = {}
    for L in range(DEPTH_LO, NL + 1):
        shapes = [(W, D) for W in (4, 6, 8, 10) for D in (8, 15)] + [(12, 8)] if L == NL else [(W, 15) for W in (8, 10, 12)]
        for W, D in shapes:
            for full, dxo in ((False, False), (True, False), (False, True)):
                out[lane_name(W, D, False, full, dxo, L=L)] = ("lane", W, D, False, (full, dxo), L, 0)
            out[lane_name(W, D, True, True, L=L)] = ("lane", W, D, True, (True, False), L, 0)
            if W >= 8 and not (L == NL and W > WMAX):
                for mode in (1, 2):
                    out[lane_name(W, D, False, False, L=L, mode=mode)] = ("lane", W, D, False, (False, False), L, mode)
        if L == NL:
            for W in (4, 6, 8, 10):
                for packed, forms in ((False, (False, True)), (True, (True,))):
                    for full in forms:
                        out[lane_name(W, 0, packed, full)] = ("lane", W, 0, packed, (full, False), L, 0)
    for KS in (2, 3, 4):
        for packed in (False, True):
            out[f"elbo_narrow_kernel<2, {KS}, 8, {TF[packed]}>"] = ("narrow", 0, KS, packed, (True, False), 0, 0)
    return out


def enumerate_uncovered():
    """the names of the per-image-layer instances (launch_lane_imgl_of): known, not covered"""
    out = set()
    for L in range(DEPTH_LO, NL + 1):
        for NI in (1, 2, 3):
            if NI == 3 and not (L == NL or L <= IMGL3_DEPTH_MAX):
                continue
            forms = ((False, False), (True, False), (False, True)) if NI <= IMGL_MAX else ((False, False), (True, False))
            for D in ((8, 15) if (L == NL and NI <= IMGL_MAX) else (15,)):
                out |= {lane_name(WMAX, D, True, full, dxo, NI=NI, L=L) for full, dxo in forms}
    return out


# ---- the case list -----------------------------------------------------------------------------------------------------------------------------
def query(c, lib=None):
    """(route, kernel name, cl_mlp_check) of the case's arguments from the library: no device needed"""
    from careless_amd import _lib
    lib = lib or _lib.get_lib()
    a = _lib.MlpArgs(**RM.scalar_fields(c), **{k: 1 for k in RM.set_fields(c)})
    buf = ctypes.create_string_buffer(256)
    lib.cl_mlp_kernel_name(ctypes.byref(a), c.mode, buf, 256)
    return int(lib.cl_mlp_route(ctypes.byref(a), c.mode)), buf.value.decode(), int(lib.cl_mlp_check(ctypes.byref(a), c.mode, c.grid))


def lcase(w, d, L, *, packed=False, det=False, mode=0, kernel=None, **kw):
    """a case on these kernels: the unit from (packed, det), a head-less chain block for a block launch, the kernel from the restated route"""
    if mode:
        c = RM.case("chain", mode, w, d, L, head=False, kernel="lane", **kw)
    else:
        kw.setdefault("n", N_INST)
        unit = ("packed" if packed else "") + ("_det" if det and packed else ("det" if det else "")) or "plain"
        c = RM.case(unit, 0, w, d, L, kernel="lane", **kw)
        c.kernel = kernel or {"lane": "lane", "narrow": "narrow"}.get(route(c), "lane")
        c.id = c.id.replace("-lane", "-" + c.kernel)
    return c


# shapes of an instance, the rim values first: hidden widths of a compile-time width, metadata columns of a capacity
W_OF = {4: (4, 1, 3), 6: (6, 5), 8: (8, 7), 10: (10, 9), 12: (12, 11)}
W_OF_DEPTH = {8: (8, 5, 7), 10: (10, 9), 12: (12, 11)}
D_OF = {8: (8, 1, 6), 15: (15, 9, 12), 0: (16, 31, 17, 30, 23)}
D_OF_DEPTH = (15, 9, 12, 1, 8)
# ONE column in front of a deep stack: every unit of every layer is a function of one number, the units are collinear, the rows rescaled to unit
# variance reach |W| row sums of 13 per layer (ref_mlp._candidates) and no seed keeps the pre-activations out of the propagated bound.  d = 1 is
# placed where the stack has up to D1_LMAX layers (the per-depth units' register instances, the narrow kernel); deeper stacks start at two columns
# in the instance cases.  With THREE rows seeds exist at 20 layers: extra_cases runs every <W, 8, ...> register instance on one column that way.
D1_LMAX = 3
# (w, d, L) the narrow kernel keeps, by (KS, packed): one layer; widths <= 4 off the default depth; widths 13 .. 15; 11 / 12 on 9 .. 15 columns at depth 20
NARROW_SHAPES = {(2, False): ((8, 3, 1), (3, 8, 2), (4, 7, 19), (2, 5, 10), (1, 1, 1)), (3, False): ((9, 4, 1), (4, 12, 3), (12, 11, 1), (3, 9, 19), (11, 9, 20), (12, 12, 20)),
                 (4, False): ((13, 6, 20), (15, 15, 2), (4, 13, 19), (14, 15, 1), (13, 12, 20), (11, 15, 20)),
                 (2, True): ((4, 8, 2), (8, 8, 1), (3, 2, 19)), (3, True): ((4, 9, 3), (9, 12, 1), (12, 4, 1), (12, 9, 20)), (4, True): ((13, 8, 20), (15, 13, 1), (4, 15, 19))}


def _form_kw(form, k, packed):
    """the options that put a launch on a form; what else a form allows cycles with k"""
    full, dxo = form
    if not full:                                                        # production: in-kernel noise, none of the optional buffers
        return dict(noise="philox", dz0=dxo, S=(1, 2, 3, 5, 8)[k % 5], lik=("normal", "studentt")[k % 2], bij=("exp", "softplus")[(k // 2) % 2],
                    img=("off", "sorted", "unsorted")[k % 3])
    why = k % 4                                                         # what asks for the full form: eta, ipred_out, the Evans-2011 buffers, or all of them
    return dict(noise="eta" if why in (0, 3) else "philox", ipred=why in (1, 3), ev11=why in (2, 3), dz0=bool(k % 2) and not packed,
                S=(1, 3, 4, 9)[k % 4], lik=("normal", "studentt")[(k // 2) % 2], bij=("exp", "softplus")[k % 2], img=("off", "sorted", "unsorted")[k % 3],
                groups=packed and bool(k % 2))


def instance_cases():
    """one case per enumerated instance and one more per full instance in its deterministic run-time form, at n = 17 * 64 + 37 rows on two
    workgroups, the shape cycling through the instance's rim values"""
    out, k = [], 0
    for name, (kern, W, D, packed, form, L, mode) in enumerate_lane_instances().items():
        for det in ((False, True) if (form[0] and not mode) else (False,)):
            if kern == "narrow":
                w, d, l = NARROW_SHAPES[(D, packed)][k % len(NARROW_SHAPES[(D, packed)])]
                if det:
                    w, d, l = NARROW_SHAPES[(D, packed)][(k + 1) % len(NARROW_SHAPES[(D, packed)])]
            else:
                ws = (W_OF if L == NL else W_OF_DEPTH)[W]
                ds = D_OF[D] if L == NL else D_OF_DEPTH
                w, d, l = ws[k % len(ws)], ds[k % len(ds)], L
                d = 2 if (d == 1 and l > D1_LMAX) else d
            if mode:
                c = lcase(max(w, DEPTH_WMIN), d, l, mode=mode, n=N_INST)
            else:
                kw = _form_kw(form, k, packed)
                if det:
                    kw.update(noise=("eta", "philox")[k % 2], det_slot=bool(k % 3 == 0), dz0=kw["dz0"] and l == NL)
                if l != NL and packed:
                    kw["dz0"] = False
                c = lcase(w, d, l, packed=packed, det=det, **kw)
            c.instance = name + (DET_TAG if det else "")
            out.append(c)
            k += 1
    return out


def _families():
    """(tag, w, d, L, packed): a full-form shape per (kernel, layout, metadata form)"""
    return [("reg", 10, 15, NL, False), ("reg", 10, 8, NL, True), ("rows", 10, 16, NL, False), ("rows", 9, 31, NL, True), ("depth", 12, 15, 7, False),
            ("depth", 5, 9, 19, True), ("w12", 11, 8, NL, False), ("narrow", 13, 9, 20, False), ("narrow", 4, 13, 3, True), ("narrow", 3, 2, 1, False)]


def extra_cases():
    """per (kernel, layout, metadata form): the row borders of the wave tile and the launch's geometry"""
    out = []
    for k, (tag, w, d, L, packed) in enumerate(_families()):
        nar = tag == "narrow"
        rows = [(3, 2, "n3"), (32 if nar else 64, 2, "t"), (33 if nar else 65, 2, "t1"), (128, 1, "n128"), (256, 2, "n256"), (257, 2, "n257"),
                (N_INST, 1, "g1"), (2 * 128 + 37, 7, "gbig")]
        for i, (n, grid, t) in enumerate(rows):
            det = bool((k + i) % 2)
            out.append(lcase(w, d, L, packed=packed, det=det, n=n, grid=grid, S=(3, 2)[i % 2], lik=("normal", "studentt")[i % 2], ev11=bool(i % 3 == 0),
                             img=("sorted", "off", "unsorted")[i % 3], ipred=bool(i % 2), dz0=not packed and bool(i % 2), tag=t))
    # ONE column at the default depth (D1_LMAX): three rows of the 64 drawn keep every unit out of its bound -- the single-column path of the
    # <4 / 6 / 8, 8, ...> register instances in the plain layout's three forms, and of a block.  Not at widths 10 and 12 (the emulation's weight
    # gradient reaches 1.5 and 0.26 of its bound: three rows of collinear units cancel), not in the packed layout (its 125 padding positions have
    # metadata 0: every pre-activation of theirs is inside the bound of a 20-layer stack): NOTEBOOK R25.1
    for k, w in enumerate((4, 5, 8)):
        out.append(lcase(w, 1, NL, n=3, noise="philox", S=(1, 3)[k % 2], dz0=bool(k % 2), tag="d1"))
        out.append(lcase(w, 1, NL, n=3, S=3, ipred=True, det=bool(k % 2), img="sorted", tag="d1"))
    out += [lcase(5, 1, NL, mode=1, n=3, tag="d1"), lcase(8, 1, NL, mode=2, n=3, tag="d1")]
    return out


def option_cases():
    out = []
    for k, (tag, w, d, L, packed) in enumerate(_families()):
        for i, S in enumerate((1, 2, 3, 4, 5, 8, 9, 12, 16, 17)):
            out.append(lcase(w, d, L, packed=packed, det=bool(i % 3 == 1), n=5 * 64 + 37, S=S, lik=("normal", "studentt")[(k + i) % 2], bij=("exp", "softplus")[i % 2],
                             img=("sorted", "unsorted", "off")[(k + i) % 3], noise=("eta", "philox")[(i // 2) % 2], ipred=bool(i % 4 == 0), ev11=bool(i % 5 == 2),
                             groups=packed and bool(i % 2), tag="opt"))
        out.append(lcase(w, d, L, packed=packed, det=True, n=5 * 64 + 37, S=4, ev11=True, det_slot=True, img="sorted", groups=packed, tag="opt"))
        if packed:                                                      # det_slot[row_map[position]]: the packed branch, without harmonic groups too
            out.append(lcase(w, d, L, packed=True, det=True, n=5 * 64 + 37, S=3, det_slot=True, img="unsorted", noise="philox", tag="opt"))
        out.append(lcase(w, d, L, packed=packed, n=5 * 64 + 37, S=5, ev11=True, img="unsorted", lik="studentt", bij="softplus", dz0=not packed or L == NL, tag="opt"))
        if packed:
            out.append(lcase(w, d, L, packed=True, det=bool(k % 2), n=5 * 64 + 37, S=3, noise="philox", noise_row=True, groups=True, ipred=True, tag="opt"))
    return out


def block_cases():
    """the head-less blocks' own borders: widths 5 | 8 | 9 | 10 | 12, columns 8 | 9 | 15, depths 2, 19, 20, the geometry of the extras"""
    out = []
    for mode in (1, 2):
        for (w, d, L) in ((5, 1, 2), (5, 2, 20), (8, 9, 20), (10, 15, 2), (12, 8, 19), (9, 15, 19)):
            for (n, grid, t) in ((3, 2, "n3"), (65, 2, "t1"), (128, 1, "n128"), (2 * 128 + 37, 7, "gbig")):
                out.append(lcase(w, d, L, mode=mode, n=n, grid=grid, tag=t))
    return out


def stop_cases():
    out = []
    for k, (tag, w, d, L, packed) in enumerate(_families()):
        out.append(lcase(w, d, L, packed=packed, det=bool(k % 2), n=5 * 64 + 37, S=(3, 4)[k % 2], ev11=True, ipred=True, img=("sorted", "unsorted")[k % 2],
                         det_slot=bool(k % 2), groups=packed, dz0=not packed or L == NL, tag="stop"))
    out += [lcase(10, 15, 20, noise="philox", n=5 * 64 + 37, tag="stop"), lcase(8, 8, 20, noise="philox", dz0=True, n=5 * 64 + 37, tag="stop"),
            lcase(10, 9, 20, mode=1, n=5 * 64 + 37, tag="stop"), lcase(12, 15, 6, mode=2, n=5 * 64 + 37, tag="stop")]
    return out


def refusal_cases():
    """(case, why): arguments that must leave these routes -- cl_mlp_check and the call answer -2 where no route is left"""
    mk = lambda *a, **kw: RM.case(*a, n=5 * 64 + 37, **kw)
    return [(mk("plain", 0, 10, 15, 20, lik="laplace", S=3), "Laplace: elbo_mlp.hip's instance, not refused"),
            (mk("chain", 0, 10, 15, 20, dX=True, S=3), "dX_out: the chain unit, not refused"),
            (mk("plain", 0, 10, 15, 20, lik="laplace", S=3, kernel="lane", dz0=True), "dZ0_out on a Laplace step"),
            (mk("plain", 0, 16, 8, 2, kernel="lane", dz0=True), "dZ0_out at width 16"),
            (mk("plain", 0, 10, 32, 20, kernel="lane", dz0=True), "dZ0_out on 32 columns"),
            (mk("chain", 0, 10, 15, 20, dX=True, kernel="lane", dz0=True), "dZ0_out beside dX_out"),
            (mk("packed", 0, 10, 9, 7, kernel="lane", dz0=True), "dZ0_out with row_map at a non-default depth")]


_CASES = {}


def cases():
    if "all" not in _CASES:
        cs = instance_cases() + extra_cases() + option_cases() + block_cases()
        ids = set()
        _CASES["all"] = [c for c in cs if not (c.id in ids or ids.add(c.id))]
    return _CASES["all"]


# ---- the peeled first layer and the chain step (csrc/elbo_peel.hip) -------------------------------------------------------------------------------
F32, U = np.float32, RW.U
PEEL_WS, PEEL_NS = (1, 4, 5, 10, 15), (3, 64, 257, 1125)
PEEL_DMAX = 79                                                         # cl_peel_supported: five 16-column blocks hold 79 columns and the ones


def peel_ds(w):
    return sorted({d for d in (w + 1, 15, 16, 17, 37, 63, 64, 79) if d > w})


def peel_supported(d, w, L):
    return 1 <= d <= PEEL_DMAX and 1 <= w <= 15 and L >= 1 and d > w


def peel_shapes():
    """(w, d, n, L): every (w, d) of the border lists with n cycling through its four values; every n at 10 x 37; the default depth once"""
    out = [(w, d, PEEL_NS[(i + j) % 4], 2 + (i + j) % 2) for i, w in enumerate(PEEL_WS) for j, d in enumerate(peel_ds(w))]
    out += [(10, 37, n, 3) for n in PEEL_NS] + [(10, 37, 257, 20), (15, 79, 1125, 1)]
    return sorted(set(out))


def peel_problem(w, d, n, L):
    """operands of cl_peel_forward / cl_peel_backward: the inputs of ref_mlp.scaler_problem, a dZ_0 that is zero behind n_obs (the contract of
    cl_mlp_args.dZ0_out), the peeled scaler's gradient and the preload of grad_mlp"""
    rng = np.random.default_rng([35, w, d, n, L])
    X, mlp = RM.scaler_problem(1, n, d, w, L)
    p = RM.SimpleNamespace(w=w, d=d, n=n, L=L, n_pad=(n + RM.TILE - 1) // RM.TILE * RM.TILE, mlp=mlp, id=f"{L}x{w}-d{d}-n{n}")
    p.X = np.zeros((p.n_pad, d), F32)
    p.X[:n] = X
    p.meta_t = np.zeros((RM.meta_rows(d), p.n_pad), F32)
    p.meta_t[:d] = p.X.T
    p.dz0 = np.zeros((RM.meta_rows(w), p.n_pad), F32)
    p.dz0[:w, :n] = RW.normals(rng, w, n) * F32(0.7)
    p.P, p.Pp, p.n0 = RM.param_count(d, w, L), RM.param_count(w, w, L), w * d + w
    p.grad_peel = RW.normals(rng, p.Pp)
    Wt, b = RW.f64(mlp[:w * d]).reshape(w, d), RW.f64(mlp[w * d:w * d + w])
    X64, dz = RW.f64(p.X), RW.f64(p.dz0[:w]).T
    p.u, p.u_bound = X64 @ Wt.T + b, RW.gamma(d + 1) * (np.abs(X64) @ np.abs(Wt).T + np.abs(b))
    p.mlp_peel = np.concatenate([np.eye(w, dtype=F32).ravel(), np.zeros(w, F32), mlp[p.n0:]])
    p.g0, p.M0 = np.concatenate([(dz.T @ X64).ravel(), dz.sum(0)]), np.concatenate([(np.abs(dz).T @ np.abs(X64)).ravel(), np.abs(dz).sum(0)])
    sgn = np.where(rng.random(p.P) < 0.5, -1.0, 1.0)
    p.pre = (np.concatenate([0.1 * p.M0, 0.3 * np.ones(p.P - p.n0)]) * sgn).astype(F32)
    p.tail = RW.f64(p.pre[p.n0:]) + RW.f64(p.grad_peel[w * w + w:])
    return p


def peel_forward_ratios(p, u_t, mlp_peel):
    """u_t over ALL n_pad columns against gamma(d + 1) sum |W||x| (the bias with the ones among the d + 1 products); the rest exact"""
    out = {"u_t": RR._worst(np.abs(RW.f64(u_t)[:p.w].T - p.u), p.u_bound)}
    out["u_t padding rows"] = 0.0 if np.all(u_t[p.w:] == 0.0) else np.inf
    out["mlp_peel"] = 0.0 if np.asarray(mlp_peel).tobytes() == p.mlp_peel.tobytes() else np.inf
    return out


def peel_backward_ratios(p, grad):
    stored = RW.f64(p.pre[:p.n0]) + p.g0
    return {"layer 0": RR._worst_grad(np.abs(RW.f64(grad[:p.n0]) - stored), p.M0, stored), "tail": RR._worst(np.abs(RW.f64(grad[p.n0:]) - p.tail), U * np.abs(p.tail))}


def _fma_chain(acc, A, x):
    """acc[k] = fmaf(A[k][c], x[c], acc[k]) over c ascending, in fp32 (the product is exact in fp64)"""
    acc = acc.astype(F32)
    for c in range(A.shape[1]):
        acc = (RW.f64(A[:, c]) * RW.f64(x[..., c, None]) + RW.f64(acc)).astype(F32)
    return acc


def peel_forward_emulate(p):
    Wt, b = p.mlp[:p.w * p.d].reshape(p.w, p.d), p.mlp[p.w * p.d:p.n0]
    u_t = np.zeros((RM.meta_rows(p.w), p.n_pad), F32)
    u_t[:p.w] = _fma_chain(np.broadcast_to(b, (p.n_pad, p.w)), Wt, p.X).T
    return u_t, p.mlp_peel.copy()


PEEL_MUTANTS = ("bias_gradient_over_a_non_zero_dz0_behind_n_obs", "block_index_dropped", "tail_from_the_unpeeled_offset")


def peel_backward_emulate(p, mutant=None, nparts=1):
    dz = p.dz0[:p.w].copy()
    if mutant == "bias_gradient_over_a_non_zero_dz0_behind_n_obs":      # what the step's kernel must never leave behind n_obs
        dz[:, p.n:] = F32(1e-3)
    parts = np.zeros((nparts, p.n0), F32)
    for g in range(nparts):                                            # 64-observation tiles strided over the workgroups' four waves
        cols = np.flatnonzero(((np.arange(p.n_pad) // 64) % (4 * nparts)) // 4 == g)
        dW = RM._mm(dz[:, cols], p.X[cols])
        if mutant == "block_index_dropped":
            wrong = np.zeros_like(dW)
            for c in range(p.d):
                wrong[:, c % 16] = dW[:, c]
            dW = wrong
        parts[g] = np.concatenate([dW.ravel(), dz[:, cols].sum(1, dtype=F32)])
    grad = p.pre.copy()
    grad[:p.n0] += parts.sum(0, dtype=F32)
    off = p.n0 if mutant == "tail_from_the_unpeeled_offset" else p.w * p.w + p.w
    src = np.concatenate([p.grad_peel, np.zeros(p.P, F32)])[off:off + p.P - p.n0]
    grad[p.n0:] += src
    return grad


def chain_problem(w_out, w_in, n):
    rng = np.random.default_rng([36, w_out, w_in, n])
    q = RM.SimpleNamespace(w_out=w_out, w_in=w_in, n=n, n_pad=(n + RM.TILE - 1) // RM.TILE * RM.TILE, id=f"{w_out}to{w_in}-n{n}")
    # gamma(w_out) of a chain of w_out products is w_out roundings: a chain that rounds at all uses up to half of it (random numbers: 0.12 .. 0.53 of
    # the bound at w_out = 4 .. 12, 0.99 at w_out = 1: NOTEBOOK R25.1).  As for the first layer of ref_mlp.scaler_problem the operands are multiples
    # of 2^-6 and 2^-8 below 4: products and sums of up to fifteen of them are exact in fp32 in any order, and a result that is off at all is outside
    q.Wt = (np.clip(np.round(RW.normals(rng, w_out, w_in) / F32(np.sqrt(w_in)) * 64), -255, 255) / 64).astype(F32)
    q.Wt = np.where(q.Wt == 0, F32(1.0 / 64), q.Wt)
    q.dz = (np.clip(np.round(RW.normals(rng, RM.meta_rows(w_out), q.n_pad) * 256), -1023, 1023) / 256).astype(F32)      # (behind n_obs and in the padding rows: numbers the call must not use)
    dz = RW.f64(q.dz[:w_out, :n]).T
    q.dx, q.bound = dz @ RW.f64(q.Wt), RW.gamma(w_out) * (np.abs(dz) @ np.abs(RW.f64(q.Wt)))
    return q


def chain_ratios(q, dx_t):
    out = {"dx_t": RR._worst(np.abs(RW.f64(dx_t)[:q.w_in, :q.n].T - q.dx), q.bound)}
    out["zeros"] = 0.0 if (np.all(dx_t[:, q.n:] == 0.0) and np.all(dx_t[q.w_in:] == 0.0)) else np.inf
    return out


def chain_emulate(q, mutant=None):
    Wt = q.Wt if mutant != "W_not_transposed" else np.ascontiguousarray(q.Wt.ravel().reshape(q.w_in, q.w_out).T)
    dx_t = np.zeros((RM.meta_rows(q.w_in), q.n_pad), F32)
    dx_t[:q.w_in, :q.n] = _fma_chain(np.zeros((q.n, q.w_in), F32), np.ascontiguousarray(Wt.T), q.dz[:q.w_out, :q.n].T).T
    return dx_t


CHAIN_SHAPES = [(10, 7, 3), (7, 10, 64), (15, 1, 257), (1, 15, 1125), (4, 5, 257), (12, 9, 1125), (15, 14, 257)]
