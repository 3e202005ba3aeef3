"""Every `cl_wide_*` entry point of csrc/wide_gemm.hip called directly, element by element against the fp64 references of
tests/ref_wide.py at their a-priori rounding bounds, on operands carved from one guarded allocation (ref_wide.Arena: guard rows
bit-identical after the call, every output element written, padding columns of outputs exactly zero, partial slots written).

Shape -> instance, from the dispatch in wide_gemm.hip (shapes are in -> out; N = output columns of the launch, K = contraction):
  launch_sq (sq_ok: ceil(N / 16) == ceil(K / 16) = NA >= 5, ld % 4 == 0, 16-byte aligned): `with_blocks<5>((s.N + 15) >> 4, ..)`, NA = 5 .. 7 by name, else 8
      65 -> 80: wide_sq_kernel<.., NA = 5>; 96 -> 96: NA = 6; 100 -> 112, 112 -> 100, 100 -> 100, 120 -> 120: NA = 7 (never run before);
      113 -> 128, 128 -> 113: NA = 8 with a ragged last block; PRE (dgrad_pre), WG0 (dgrad_pre_wgrad0), HEADB (dgrad_head) forms alike.
  launch_stream: `s.N <= 64 ? launch_stream_n<.., 4, .., PRE> : launch_stream_n<.., 8, .., PRE>` for the other layers up to 128 x 128:
      70 -> 96, 128 -> 65, 16 -> 128, 1 -> 65, 96 -> 70 (dgrad: N = 70), 32 -> 70: wide_stream_kernel<.., NAT = 8>; 70 -> 32, 128 -> 1, 3 -> 64: NAT = 4;
      any layer with ld % 4 != 0 or a pointer off 16-byte alignment: the same kernels on their scalar paths (vec == false).
  launch_gemm (a side beyond 128; every weight gradient): `if (g.N > 64) .. wide_gemm_kernel<.., 128> ..; .. wide_gemm_kernel<.., 64>`
      130 -> 96, 64 -> 129 (a tile of one column), 200 -> 300 (three column tiles, K > 128): BN = 128; 130 -> 32, 129 -> 64, 300 -> 1: BN = 64.
  launch_stream2: `with_blocks<1>(((s.pre.N0 > s.N1 ? s.pre.N0 : s.N1) + 15) >> 4, ..)`: 100, 120 -> wide_stream2_kernel<7>; 65 -> <5>; 128 -> <8>; 20 -> <2>.
  cl_wide_head_backward's ladder: `if (w <= 128) return launch(<1>); if (w <= 256) .. <2>; if (w <= 512) .. <4>; return launch(<8>)` (cl_launch_lds sets the dynamic-LDS attribute):
      65, 128 -> 1; 129, 256 -> 2; 300, 512 -> wide_head_backward_kernel<4>; 520, 1024 -> <8>.
  Rows: grids are min(ceil(n / 128), 2 CUs) workgroups of 8 waves, a wave per 16-row block: at n_long = 128 (2 CUs) + 128 * 3 + 5 some waves
  walk two blocks (the prefetch of "the wave's next block"), some one, and the last block is ragged.  Grouped kernels take
  min(groups, 2 CUs) workgroups: 2 CUs + 40 groups make some workgroups take a second group (`grp += gridDim.x`).

No tolerance here is a tuned number: every comparison is `|device - fp64| <= bound` per element with the bound ref_wide derives."""
import numpy as np
import pytest
import torch

from careless_amd import _lib as L
from careless_amd.wide import image_tiles
from tests import ref_wide as R

pytestmark = pytest.mark.gpu

LEAK = 0.01
EPS = 1e-7
DEV = "cuda"
ROWS = R.N_ROWS
GROUP_SIZES = [0, 1, 15, 16, 17, 200, 0, 3]


def lib():
    return L.get_lib()


def n_cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def n_long():
    return R.n_long(n_cus())


def ld_of(w, scalar=False):
    return w if scalar else int(lib().cl_wide_ld(w))


def run(a, fn, *args, want=0):
    """the call on stream 0, synchronised; the stop flag is the arena's `stop` operand when it has one"""
    code = int(getattr(lib(), fn)(*args, a.ptr("stop") if "stop" in a.ops else None, None))
    torch.cuda.synchronize()
    assert code == want, f"{fn} returned {code}, expected {want}"
    return code


def reduce_partials(a, name, nparts, P, out):
    code = int(lib().cl_reduce_partials(a.ptr(name), nparts, P, a.ptr(out), None, None))
    torch.cuda.synchronize()
    assert code == 0
    return a


def arena(stop):
    a = R.Arena(DEV)
    if stop:
        a.input("stop", np.array([1], np.int32))
    return a


def ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


# ---- cl_wide_dense_forward ----------------------------------------------------------------------------------------------------------------
FWD = [(65, 80, 0), (96, 96, 1), (100, 112, 0), (113, 128, 0),                       # square-layer kernel
       (70, 96, 1), (128, 65, 0), (16, 128, 0), (1, 65, 0),                            # stream, NAT 8
       (70, 32, 0), (128, 1, 0), (3, 64, 0),                                           # stream, NAT 4
       (130, 96, 0), (64, 129, 0), (200, 300, 0),                                      # tiled, BN 128
       (130, 32, 0), (129, 64, 0), (300, 1, 0)]                                        # tiled, BN 64
FWD_CASES = [(i, o, act, n) for (i, o, lg) in FWD for act in (0, 1) for n in ROWS] + [(i, o, act, -1) for (i, o, lg) in FWD if lg for act in (0, 1)]


def dense_forward(n, n_in, n_out, act, scalar=False, stop=False, seed=0):
    rng = np.random.default_rng(seed + 1000 * n_in + n_out)
    X, (Wt, b) = R.normals(rng, n, n_in), R.layer(rng, n_out, n_in)
    mis = 1 if scalar else 0
    a = arena(stop).input("X", X, ld_of(n_in, scalar), mis).input("Wt", Wt, misalign=mis).input("b", b).output("Y", n, n_out, ld_of(n_out, scalar), mis).build()
    run(a, "cl_wide_dense_forward", a.ptr("X"), a.ld("X"), a.ptr("Wt"), a.ptr("b"), n, n_in, n_out, LEAK, act, a.ptr("Y"), a.ld("Y"))
    if stop:
        return a.verify(untouched=True)
    a.verify()
    y, bound, _ = R.dense_forward(X, Wt, b, LEAK, act)
    R.assert_within(a.get("Y"), y, bound, f"dense_forward {n_in}->{n_out} act {act} n {n}", "cl_wide_dense_forward" + (" (scalar paths)" if scalar else ""))


@pytest.mark.parametrize("n_in,n_out,act,n", FWD_CASES, ids=ids(FWD_CASES))
def test_dense_forward(n_in, n_out, act, n):
    """Y = act(X Wt^T + b) on each of the three kernel families and both tile widths (module docstring: shape -> instance)"""
    dense_forward(n_long() if n < 0 else n, n_in, n_out, act)


# ---- cl_wide_dense_forward_head -----------------------------------------------------------------------------------------------------------
FH = [(100, 112, 0), (128, 128, 1), (70, 96, 0), (40, 20, 0)]
FH_CASES = [(i, o, kind, dsd, n) for (i, o, lg) in FH for kind in (0, 1) for dsd in (0, 1) for n in ROWS] + \
           [(i, o, kind, 1, -1) for (i, o, lg) in FH if lg for kind in (0, 1)]


def forward_head(n, n_in, n_out, kind, dsd, stop=False):
    rng = np.random.default_rng(7 + 1000 * n_in + n_out)
    X, (Wt, b), head = R.normals(rng, n, n_in), R.layer(rng, n_out, n_in), R.head_params(rng, n_out)
    a = arena(stop).input("X", X, ld_of(n_in)).input("Wt", Wt).input("b", b).input("head", head).output("Y", n, n_out, ld_of(n_out))
    a.output("loc", n, 1).output("sig", n, 1)
    if dsd:
        a.output("dsd", n, 1)
    a.build()
    run(a, "cl_wide_dense_forward_head", a.ptr("X"), a.ld("X"), a.ptr("Wt"), a.ptr("b"), n, n_in, n_out, LEAK, a.ptr("Y"), a.ld("Y"), a.ptr("head"), kind, EPS,
        a.ptr("loc"), a.ptr("sig"), a.ptr("dsd" if dsd else None))
    if stop:
        return a.verify(untouched=True)
    a.verify()
    ref = R.dense_forward_head(X, Wt, b, LEAK, head, kind, EPS)
    for k in ("Y", "loc", "sig") + (("dsd",) if dsd else ()):
        v, bd = ref[k]
        R.assert_within(a.get(k).reshape(v.shape), v, bd, f"forward_head {n_in}->{n_out} bij {kind} n {n}: {k}", "cl_wide_dense_forward_head")


@pytest.mark.parametrize("n_in,n_out,kind,dsd,n", FH_CASES, ids=ids(FH_CASES))
def test_dense_forward_head(n_in, n_out, kind, dsd, n):
    """the top layer with the Dense(2) head in its epilogue: 100 -> 112 wide_sq_kernel<.., 7>, 128 -> 128 <.., 8>, 70 -> 96 / 40 -> 20 the
    streaming kernel's head (NAT 8 / 4); both bijectors; dsig_draw_out NULL and set"""
    forward_head(n_long() if n < 0 else n, n_in, n_out, kind, dsd)


def forward_head_lik(n, n_in, n_out, S, stop=False):
    """cl_wide_dense_forward_head_lik: the same layer and head with the slot likelihood of the rows in the epilogue (LIK instances of
    wide_sq_kernel).  Y, loc, sigma, dsig_draw are compared with the reference; the likelihood's own outputs (dO, dz_f, d_img, the NLL)
    are accumulators here -- their values are held to the oracle by the whole-step cases of tests/test_gpu_parity.py -- and must be finite."""
    rng = np.random.default_rng(37 + 1000 * n_in + n_out)
    X, (Wt, b), head = R.normals(rng, n, n_in), R.layer(rng, n_out, n_in), R.head_params(rng, n_out)
    Rf, M = 23, 5
    refl, img_id = rng.integers(0, Rf, n).astype(np.int32), np.sort(rng.integers(0, M, n)).astype(np.int32)
    iobs, sg = (10.0 * np.abs(R.normals(rng, n))).astype(np.float32), (1.0 + np.abs(R.normals(rng, n))).astype(np.float32)
    z_f, img = (1.0 + np.abs(R.normals(rng, Rf, S))).astype(np.float32), (1.0 + 0.1 * R.normals(rng, M - 1)).astype(np.float32)
    a = arena(stop).input("X", X, ld_of(n_in)).input("Wt", Wt).input("b", b).input("head", head).output("Y", n, n_out, ld_of(n_out))
    a.output("loc", n, 1).output("sig", n, 1).output("dsd", n, 1)
    a.input("refl", refl).input("img_id", img_id).input("iobs", iobs).input("sg", sg).input("z_f", z_f.ravel()).input("img", img)
    a.accum("dO", 2 * n).accum("dz_f", Rf * S).accum("d_img", M - 1).accum("scalars", 2 * L.CL_SC_COUNT).build()
    la = L.LaueArgs(refl_id=a.ptr("refl"), image_id=a.ptr("img_id"), iobs=a.ptr("iobs"), sig=a.ptr("sg"), n_obs=n, obs_offset=0, img=a.ptr("img"), use_img=1,
                    z_f=a.ptr("z_f"), R=Rf, S=S, lik_kind=L.CL_LIK_NORMAL, dof=0.0, lik_const=0.0, shift=0.0, w_ll=1.0, seed=5, step=2,
                    dz_f=a.ptr("dz_f"), d_img=a.ptr("d_img"), dO=a.ptr("dO"), scalars=a.ptr("scalars"))
    import ctypes
    code = int(lib().cl_wide_dense_forward_head_lik(a.ptr("X"), a.ld("X"), a.ptr("Wt"), a.ptr("b"), n, n_in, n_out, LEAK, a.ptr("Y"), a.ld("Y"), a.ptr("head"),
                                                    R.BIJ_SOFTPLUS, EPS, a.ptr("loc"), a.ptr("sig"), a.ptr("dsd"), ctypes.byref(la),
                                                    a.ptr("stop") if stop else None, None))
    torch.cuda.synchronize()
    assert code == 0
    if stop:
        return a.verify(untouched=True)       # Y, loc, sigma, dO, dz_f, d_img and the scalars: nothing written, nothing added
    a.verify()
    ref = R.dense_forward_head(X, Wt, b, LEAK, head, R.BIJ_SOFTPLUS, EPS)
    for k in ("Y", "loc", "sig", "dsd"):
        v, bd = ref[k]
        R.assert_within(a.get(k).reshape(v.shape), v, bd, f"forward_head_lik {n_in}->{n_out} S {S} n {n}: {k}", "cl_wide_dense_forward_head_lik")
    for k in ("dO", "dz_f", "d_img"):
        assert np.all(np.isfinite(a.get(k))) and np.any(a.get(k) != 0.0), k
    nll = a.get("scalars").view(np.float64)[0, L.CL_SC_NLL]
    assert np.isfinite(nll) and nll != 0.0


FHL_CASES = [(100, 112, 3, 129), (100, 112, 4, 677), (128, 128, 4, -1)]


@pytest.mark.parametrize("n_in,n_out,S,n", FHL_CASES, ids=ids(FHL_CASES))
def test_dense_forward_head_lik(n_in, n_out, S, n):
    """wide_sq_kernel<false, EPI_BIAS_LRELU, 7 / 8, false, false, false, LIK>: the layer's and the head's outputs at the reference's bound with
    the likelihood epilogue running (S = 3: a row's samples straddle its four lanes unevenly; the long case: a wave's second block)"""
    forward_head_lik(n_long() if n < 0 else n, n_in, n_out, S)


@pytest.mark.parametrize("n_in,n_out", [(129, 64), (64, 129)])
def test_dense_forward_head_refuses_layers_past_128(n_in, n_out):
    a = R.Arena(DEV).input("x", np.zeros((4, 132), np.float32)).output("y", 4, 132).build()
    p = a.ptr("x")
    run(a, "cl_wide_dense_forward_head", p, 132, p, p, 4, n_in, n_out, LEAK, a.ptr("y"), 132, p, 0, EPS, a.ptr("y"), a.ptr("y"), None, want=-2)
    a.verify(untouched=True)


# ---- cl_wide_dense2_forward ---------------------------------------------------------------------------------------------------------------
D2 = [(100, 0), (120, 0), (65, 0), (128, 1), (20, 0)]
D2_CASES = [(d0, w, hd, n) for (w, lg) in D2 for d0 in R.D0S for hd in (0, 1) for n in ROWS] + [(d0, w, 1, -1) for (w, lg) in D2 if lg for d0 in R.D0S]


def dense2_forward(n, d0, w, hd, stop=False):
    X0, Wt0, b0, rng = R.pre_problem(11 + 100 * w + d0, n, d0, w)
    (Wt1, b1), head = R.layer(rng, w, w), R.head_params(rng, w)
    a = arena(stop).input("X0", X0, ld_of(d0)).input("Wt0", Wt0).input("b0", b0).input("Wt1", Wt1).input("b1", b1).input("head", head).output("Y", n, w, ld_of(w))
    if hd:
        a.output("loc", n, 1).output("sig", n, 1)
    a.build()
    kind = R.BIJ_SOFTPLUS if d0 == 8 else R.BIJ_EXP
    run(a, "cl_wide_dense2_forward", a.ptr("X0"), a.ld("X0"), d0, a.ptr("Wt0"), a.ptr("b0"), a.ptr("Wt1"), a.ptr("b1"), n, w, w, LEAK, a.ptr("Y"), a.ld("Y"),
        a.ptr("head" if hd else None), kind, EPS, a.ptr("loc" if hd else None), a.ptr("sig" if hd else None))
    if stop:
        return a.verify(untouched=True)
    a.verify()
    ref = R.dense2_forward(X0, Wt0, b0, Wt1, b1, LEAK, head if hd else None, kind, EPS)
    for k in ("Y",) + (("loc", "sig") if hd else ()):
        v, bd = ref[k]
        R.assert_within(a.get(k).reshape(v.shape), v, bd, f"dense2_forward d0 {d0} w {w} n {n}: {k}", "cl_wide_dense2_forward")


@pytest.mark.parametrize("d0,w,hd,n", D2_CASES, ids=ids(D2_CASES))
def test_dense2_forward(d0, w, hd, n):
    """layers 0 + 1 in one launch: wide_stream2_kernel<ceil(w / 16)> -- <7> at 100 and 120, <5> at 65, <8> at 128, <2> at 20; head NULL and set"""
    dense2_forward(n_long() if n < 0 else n, d0, w, hd)


# ---- cl_wide_dense_dgrad ------------------------------------------------------------------------------------------------------------------
DG = [(112, 100, 0), (128, 113, 1), (96, 70, 0), (32, 70, 0), (96, 130, 0), (300, 200, 0), (32, 130, 0)]      # in -> out of the product: n_out -> n_in
DG_CASES = [(no, ni, h, n) for (no, ni, lg) in DG for h in (0, 1) for n in ROWS] + [(no, ni, 1, -1) for (no, ni, lg) in DG if lg]


def dense_dgrad(n, n_out, n_in, with_h, scalar=False, stop=False):
    rng = np.random.default_rng(3 + 1000 * n_out + n_in)
    dZ, (Wt, _), H = R.normals(rng, n, n_out), R.layer(rng, n_out, n_in), R.with_zeros(rng, R.normals(rng, n, n_in))
    mis = 1 if scalar else 0
    a = arena(stop).input("dZ", dZ, ld_of(n_out, scalar), mis).input("Wt", Wt, misalign=mis).input("H", H, ld_of(n_in, scalar), mis)
    a.output("dX", n, n_in, ld_of(n_in, scalar), mis).build()
    run(a, "cl_wide_dense_dgrad", a.ptr("dZ"), a.ld("dZ"), a.ptr("Wt"), n, n_out, n_in, a.ptr("H" if with_h else None), a.ld("H"), LEAK, a.ptr("dX"), a.ld("dX"))
    if stop:
        return a.verify(untouched=True)
    a.verify()
    v, bd = R.dense_dgrad(dZ, Wt, H if with_h else None, LEAK)
    R.assert_within(a.get("dX"), v, bd, f"dense_dgrad {n_out}->{n_in} mask {with_h} n {n}", "cl_wide_dense_dgrad" + (" (scalar paths)" if scalar else ""))


@pytest.mark.parametrize("n_out,n_in,with_h,n", DG_CASES, ids=ids(DG_CASES))
def test_dense_dgrad(n_out, n_in, with_h, n):
    """dX = (dZ Wt) * LeakyReLU'(H), H with exact +0.0 / -0.0 entries: 112 -> 100 wide_sq_kernel<true, EPI_DLRELU, 7>, 128 -> 113 <.., 8> ragged,
    96 -> 70 and 32 -> 70 wide_stream_kernel NAT 8 (N = 70), 96 -> 130 and 300 -> 200 the tiled kernel BN 128, 32 -> 130 BN 128 over K = 32"""
    dense_dgrad(n_long() if n < 0 else n, n_out, n_in, with_h)


@pytest.mark.parametrize("n_in,n_out", [(70, 96), (130, 96)])
@pytest.mark.parametrize("n", ROWS)
def test_scalar_fallbacks_of_forward_and_dgrad(n, n_in, n_out):
    """ld = width (70, 130: no multiple of 4) and every base pointer 4 bytes off 16-byte alignment: `vec == false` in load_x / load_tile and
    the element-wise stores of wide_stream_kernel (70 -> 96) and wide_gemm_kernel (130 -> 96)"""
    dense_forward(n, n_in, n_out, 1, scalar=True)
    dense_dgrad(n, n_out, n_in, 1, scalar=True)


# ---- the recomputed first layer: cl_wide_dense_dgrad_pre, cl_wide_dense_dgrad_pre_wgrad0 --------------------------------------------------
PRE_CASES = [(d0, no, ni, n) for (no, ni) in R.PRE_DGRAD_LAYERS for d0 in R.D0S for n in ROWS] + [(d0, 120, 120, -1) for d0 in R.LONG_D0S]


def pre_operands(n, d0, n_out, n_in):
    X0, Wt0, b0, rng = R.pre_problem(R.pre_case_seed(n, d0, n_in), n, d0, n_in)
    assert R.near_zero(X0, Wt0, b0) == 0          # no mask element may take either branch: nothing is excluded below
    dZ, (Wt, _) = R.normals(rng, n, n_out), R.layer(rng, n_out, n_in)
    return X0, Wt0, b0, dZ, Wt


def dgrad_pre(n, d0, n_out, n_in, stop=False):
    X0, Wt0, b0, dZ, Wt = pre_operands(n, d0, n_out, n_in)
    a = arena(stop).input("dZ", dZ, ld_of(n_out)).input("Wt", Wt).input("X0", X0, ld_of(d0)).input("Wt0", Wt0).input("b0", b0).output("dX", n, n_in, ld_of(n_in)).build()
    run(a, "cl_wide_dense_dgrad_pre", a.ptr("dZ"), a.ld("dZ"), a.ptr("Wt"), n, n_out, n_in, a.ptr("X0"), a.ld("X0"), d0, a.ptr("Wt0"), a.ptr("b0"), LEAK,
        a.ptr("dX"), a.ld("dX"))
    if stop:
        return a.verify(untouched=True)
    a.verify()
    v, bd = R.dense_dgrad_pre(dZ, Wt, X0, Wt0, b0, LEAK)
    R.assert_within(a.get("dX"), v, bd, f"dgrad_pre d0 {d0} {n_out}->{n_in} n {n}", "cl_wide_dense_dgrad_pre")


def dgrad_pre_wgrad0(n, d0, n_out, n_in, stop=False):
    X0, Wt0, b0, dZ, Wt = pre_operands(n, d0, n_out, n_in)
    parts, P = int(lib().cl_wide_dgrad_wgrad0_parts(n)), n_in * d0 + n_in
    assert parts >= 1
    a = arena(stop).input("dZ", dZ, ld_of(n_out)).input("Wt", Wt).input("X0", X0, ld_of(d0)).input("Wt0", Wt0).input("b0", b0).partial("part", parts * P).accum("g", P).build()
    run(a, "cl_wide_dense_dgrad_pre_wgrad0", a.ptr("dZ"), a.ld("dZ"), a.ptr("Wt"), n, n_out, n_in, a.ptr("X0"), a.ld("X0"), d0, a.ptr("Wt0"), a.ptr("b0"), LEAK, a.ptr("part"))
    if stop:
        return a.verify(untouched=True)
    reduce_partials(a, "part", parts, P, "g").verify()
    v, bd = R.dense_dgrad_pre_wgrad0(dZ, Wt, X0, Wt0, b0, LEAK)
    R.assert_within(a.get("g").ravel(), v, bd, f"dgrad_pre_wgrad0 d0 {d0} {n_out}->{n_in} n {n}", "cl_wide_dense_dgrad_pre_wgrad0")


@pytest.mark.parametrize("d0,n_out,n_in,n", PRE_CASES, ids=ids(PRE_CASES))
def test_dense_dgrad_pre(d0, n_out, n_in, n):
    """layer 1's dgrad behind the recomputed mask: 100 -> 100 and 120 -> 120 wide_sq_kernel<true, EPI_DLRELU, 7, PRE>, 65 -> 80 (N = 65, K = 80) <.., 5, PRE>,
    96 -> 70 (N = 96, K = 70: block counts differ) wide_stream_kernel<true, EPI_DLRELU, 8, false, PRE>"""
    dgrad_pre(n_long() if n < 0 else n, d0, n_out, n_in)


@pytest.mark.parametrize("d0,n_out,n_in,n", [c for c in PRE_CASES if (c[1], c[2]) != (70, 96)], ids=ids([c for c in PRE_CASES if (c[1], c[2]) != (70, 96)]))
def test_dense_dgrad_pre_wgrad0(d0, n_out, n_in, n):
    """... with the first layer's weight gradient taken from the output block in registers (WG0 instances, NA = 7 and 5), every one of the
    cl_wide_dgrad_wgrad0_parts(n) partial slots written, summed by cl_reduce_partials.  The long cases run at d0 = 1 and 8 (at d0 = 8 the
    `xg` rows, the row clamp and the ones column at lane K0 do real work on a wave's second block); d0 = 15 has no seed without a
    pre-activation inside its bound at that row count (ref_wide.LONG_D0S).  A contraction over n rows carries gamma(n + 4): 3.9e-3 at
    n_long, above 1 / n -- the long case checks addressing, the guards and the partial slots; its power against a block of rows left out
    comes from test_wide_fused_backward_equals_the_separate_launches[rows66000_waves_walk_two_blocks] (tests/test_gpu_parity.py)"""
    dgrad_pre_wgrad0(n_long() if n < 0 else n, d0, n_out, n_in)


def test_dense_dgrad_pre_wgrad0_refuses_the_non_square_layer():
    X0, Wt0, b0, dZ, Wt = pre_operands(129, 8, 70, 96)
    a = R.Arena(DEV).input("dZ", dZ, ld_of(70)).input("Wt", Wt).input("X0", X0, ld_of(8)).input("Wt0", Wt0).input("b0", b0).partial("part", 4096).build()
    run(a, "cl_wide_dense_dgrad_pre_wgrad0", a.ptr("dZ"), a.ld("dZ"), a.ptr("Wt"), 129, 70, 96, a.ptr("X0"), a.ld("X0"), 8, a.ptr("Wt0"), a.ptr("b0"), LEAK, a.ptr("part"), want=-2)
    a.verify(untouched=True)


# ---- weight gradients ---------------------------------------------------------------------------------------------------------------------
WG_SQ = [(100, 100), (120, 120), (65, 80)]
WG_PLAIN = WG_SQ + [(300, 200), (32, 130), (129, 64), (1, 300)]
SPLITS = ("one", "auto", "three")


def n_split(which, n):
    return {"one": 1, "auto": int(lib().cl_wide_wgrad_splits(n)), "three": 3}[which]


def dense_wgrad(n, n_out, n_in, nsplit, ldh=None, stop=False):
    rng = np.random.default_rng(5 + 1000 * n_out + n_in)
    dZ, H = R.normals(rng, n, n_out), R.normals(rng, n, n_in)
    P = n_out * n_in + n_out
    a = arena(stop).input("dZ", dZ, ld_of(n_out)).input("H", H, ld_of(n_in) if ldh is None else ldh).partial("part", nsplit * P).accum("g", P).build()
    run(a, "cl_wide_dense_wgrad", a.ptr("dZ"), a.ld("dZ"), a.ptr("H"), a.ld("H"), n, n_out, n_in, a.ptr("part"), nsplit)
    if stop:
        return a.verify(untouched=True)
    reduce_partials(a, "part", nsplit, P, "g").verify()
    v, bd = R.dense_wgrad(dZ, H)
    R.assert_within(a.get("g").ravel(), v, bd, f"dense_wgrad ({n_out}, {n_in}) n {n} splits {nsplit}", "cl_wide_dense_wgrad")


@pytest.mark.parametrize("which", SPLITS)
@pytest.mark.parametrize("n", R.N_ROWS_WGRAD)
@pytest.mark.parametrize("n_out,n_in", WG_PLAIN, ids=ids(WG_PLAIN))
def test_dense_wgrad(n_out, n_in, n, which):
    """[dWt | db] over `nsplit` row ranges (n = 40 in three splits: the third range is empty and its slots are still written), summed by
    cl_reduce_partials: wide_gemm_kernel<true, true, EPI_WGRAD, 128> for n_in > 64 -- (300, 200): a 3 x 2 grid of tiles; (1, 300): one output
    unit, three column tiles -- and <.., 64> for (129, 64)"""
    dense_wgrad(n, n_out, n_in, n_split(which, n))


@pytest.mark.parametrize("n", R.N_ROWS_WGRAD)
def test_dense_wgrad_scalar_fallback(n):
    """(96, 70) with ldh = 70: the B operand's transposing loader on its element-wise path"""
    dense_wgrad(n, 96, 70, n_split("auto", n), ldh=70)


def dense_wgrad_pre(n, d0, n_out, n_in, nsplit, stop=False):
    X0, Wt0, b0, dZ, _ = pre_operands(n, d0, n_out, n_in)
    P = n_out * n_in + n_out
    a = arena(stop).input("dZ", dZ, ld_of(n_out)).input("X0", X0, ld_of(d0)).input("Wt0", Wt0).input("b0", b0).partial("part", nsplit * P).accum("g", P).build()
    run(a, "cl_wide_dense_wgrad_pre", a.ptr("dZ"), a.ld("dZ"), a.ptr("X0"), a.ld("X0"), d0, a.ptr("Wt0"), a.ptr("b0"), LEAK, n, n_out, n_in, a.ptr("part"), nsplit)
    if stop:
        return a.verify(untouched=True)
    reduce_partials(a, "part", nsplit, P, "g").verify()
    v, bd = R.dense_wgrad_pre(dZ, X0, Wt0, b0, LEAK)
    R.assert_within(a.get("g").ravel(), v, bd, f"dense_wgrad_pre d0 {d0} ({n_out}, {n_in}) n {n} splits {nsplit}", "cl_wide_dense_wgrad_pre")


@pytest.mark.parametrize("which", SPLITS)
@pytest.mark.parametrize("n", R.N_ROWS_WGRAD)
@pytest.mark.parametrize("d0", R.D0S)
@pytest.mark.parametrize("n_out,n_in", WG_SQ, ids=ids(WG_SQ))
def test_dense_wgrad_pre(n_out, n_in, d0, n, which):
    """layer 1's weight gradient, its input h_0 made by MFMAs while the tile is staged (wide_gemm_kernel<.., 128, false, PREM>)"""
    dense_wgrad_pre(n, d0, n_out, n_in, n_split(which, n))


def head_bwd_operands(rng, n, n_out):
    Htop = R.with_zeros(rng, R.normals(rng, n, n_out))
    return Htop, R.head_params(rng, n_out), R.normals(rng, n, 2), np.abs(R.normals(rng, n)) + np.float32(0.05)


def dense_wgrad_head(n, n_out, n_in, nsplit, stop=False):
    rng = np.random.default_rng(9 + 1000 * n_out + n_in)
    Htop, head, dO, dsd = head_bwd_operands(rng, n, n_out)
    H = R.normals(rng, n, n_in)
    P, PH = n_out * n_in + n_out, 2 * n_out + 2
    a = arena(stop).input("Htop", Htop, ld_of(n_out)).input("head", head).input("dO", dO).input("dsd", dsd.reshape(-1, 1)).input("H", H, ld_of(n_in))
    a.partial("part", nsplit * P).partial("hpart", nsplit * PH).accum("g", P).accum("gh", PH).build()
    run(a, "cl_wide_dense_wgrad_head", a.ptr("Htop"), a.ld("Htop"), a.ptr("head"), a.ptr("dO"), a.ptr("dsd"), LEAK, a.ptr("H"), a.ld("H"), n, n_out, n_in,
        a.ptr("part"), a.ptr("hpart"), nsplit)
    if stop:
        return a.verify(untouched=True)
    reduce_partials(a, "part", nsplit, P, "g")
    reduce_partials(a, "hpart", nsplit, PH, "gh").verify()
    ref = R.dense_wgrad_head(Htop, head, dO, dsd, LEAK, H)
    R.assert_within(a.get("g").ravel(), *ref["partials"], f"dense_wgrad_head ({n_out}, {n_in}) n {n} splits {nsplit}: layer", "cl_wide_dense_wgrad_head")
    R.assert_within(a.get("gh").ravel(), *ref["dhead"], f"dense_wgrad_head ({n_out}, {n_in}) n {n} splits {nsplit}: head", "cl_wide_dense_wgrad_head")


@pytest.mark.parametrize("which", SPLITS)
@pytest.mark.parametrize("n", R.N_ROWS_WGRAD)
@pytest.mark.parametrize("n_out,n_in", WG_SQ, ids=ids(WG_SQ))
def test_dense_wgrad_head(n_out, n_in, n, which):
    """the top layer's weight gradient with the head's backward pass made while the A tile is staged (HEADW), and the head's own partials"""
    dense_wgrad_head(n, n_out, n_in, n_split(which, n))


def dense_dgrad_head(n, n_out, n_in, stop=False):
    rng = np.random.default_rng(13 + 1000 * n_out + n_in)
    Htop, head, dO, dsd = head_bwd_operands(rng, n, n_out)
    (Wt, _), Hp = R.layer(rng, n_out, n_in), R.with_zeros(rng, R.normals(rng, n, n_in))
    a = arena(stop).input("Htop", Htop, ld_of(n_out)).input("head", head).input("dO", dO).input("dsd", dsd.reshape(-1, 1)).input("Wt", Wt).input("Hp", Hp, ld_of(n_in))
    a.output("dX", n, n_in, ld_of(n_in)).build()
    run(a, "cl_wide_dense_dgrad_head", a.ptr("Htop"), a.ld("Htop"), a.ptr("head"), a.ptr("dO"), a.ptr("dsd"), a.ptr("Wt"), n, n_out, n_in, a.ptr("Hp"), a.ld("Hp"), LEAK,
        a.ptr("dX"), a.ld("dX"))
    if stop:
        return a.verify(untouched=True)
    a.verify()
    v, bd = R.dense_dgrad_head(Htop, head, dO, dsd, Wt, Hp, LEAK)
    R.assert_within(a.get("dX"), v, bd, f"dense_dgrad_head {n_out}->{n_in} n {n}", "cl_wide_dense_dgrad_head")


DGH_CASES = [(no, ni, n) for (no, ni) in ((100, 100), (128, 113)) for n in ROWS] + [(128, 113, -1)]


@pytest.mark.parametrize("n_out,n_in,n", DGH_CASES, ids=ids(DGH_CASES))
def test_dense_dgrad_head(n_out, n_in, n):
    """the top layer's dgrad with dZ_L made from h_L on the way to the MFMAs: wide_sq_kernel<true, EPI_DLRELU, 7 / 8, false, false, HEADB>; the
    long row count makes the prefetch of the next block's (dO, dsig_draw) cross a block boundary inside a wave"""
    dense_dgrad_head(n_long() if n < 0 else n, n_out, n_in)


# ---- the Dense(2) head on its own ---------------------------------------------------------------------------------------------------------
HEAD_W = (65, 128, 129, 256, 300, 512, 520, 1024)


def head_forward(n, w, kind, stop=False):
    rng = np.random.default_rng(17 + w)
    H, head = R.normals(rng, n, w), R.head_params(rng, w)
    a = arena(stop).input("H", H, ld_of(w)).input("head", head).output("loc", n, 1).output("sig", n, 1).build()
    run(a, "cl_wide_head_forward", a.ptr("H"), a.ld("H"), a.ptr("head"), n, w, kind, EPS, a.ptr("loc"), a.ptr("sig"))
    if stop:
        return a.verify(untouched=True)
    a.verify()
    ref = R.head_forward(H, head, kind, EPS)
    for k in ("loc", "sig"):
        R.assert_within(a.get(k).ravel(), *ref[k], f"head_forward w {w} bij {kind} n {n}: {k}", "cl_wide_head_forward")


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("w", HEAD_W)
def test_head_forward(w, n, kind):
    head_forward(n, w, kind)


def head_backward(n, w, kind, nblocks, stop=False):
    rng = np.random.default_rng(19 + w)
    H, head, dO = R.with_zeros(rng, R.normals(rng, n, w)), R.head_params(rng, w), R.normals(rng, n, 2)
    P = 2 * w + 2
    a = arena(stop).input("H", H, ld_of(w)).input("head", head).input("dO", dO).output("dZ", n, w, ld_of(w)).partial("part", nblocks * P).accum("g", P).build()
    run(a, "cl_wide_head_backward", a.ptr("H"), a.ld("H"), a.ptr("head"), a.ptr("dO"), n, w, kind, EPS, LEAK, a.ptr("dZ"), a.ld("dZ"), a.ptr("part"), nblocks)
    if stop:
        return a.verify(untouched=True)
    reduce_partials(a, "part", nblocks, P, "g").verify()
    ref = R.head_backward(H, head, dO, kind, EPS, LEAK)
    R.assert_within(a.get("dZ"), *ref["dZ"], f"head_backward w {w} bij {kind} n {n} blocks {nblocks}: dZ", "cl_wide_head_backward")
    R.assert_within(a.get("g").ravel(), *ref["dhead"], f"head_backward w {w} bij {kind} n {n} blocks {nblocks}: head gradient", "cl_wide_head_backward")


@pytest.mark.parametrize("kind", [R.BIJ_EXP, R.BIJ_SOFTPLUS], ids=["exp", "softplus"])
@pytest.mark.parametrize("blocks", ("one", "auto", "seven"))
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("w", HEAD_W)
def test_head_backward(w, n, blocks, kind):
    """the instance ladder of cl_wide_head_backward: NP = 1 (65, 128), 2 (129, 256), 4 (300, 512), 8 (520, 1024: 8 * (2 w + 2) floats of dynamic LDS, past 64 KiB at 1024);
    blocks without rows (n = 1 in seven blocks) still write their partial slots"""
    nb = {"one": 1, "auto": int(lib().cl_wide_head_blocks(n)), "seven": 7}[blocks]
    head_backward(n, w, kind, nb)


def test_head_backward_refuses_width_1025():
    a = R.Arena(DEV).input("H", np.zeros((8, 1028), np.float32)).output("dZ", 8, 1028).partial("part", 4096).build()
    run(a, "cl_wide_head_backward", a.ptr("H"), 1028, a.ptr("H"), a.ptr("H"), 8, 1025, 0, EPS, LEAK, a.ptr("dZ"), 1028, a.ptr("part"), 1, want=-2)
    a.verify(untouched=True)


# ---- per-image (grouped) layers -----------------------------------------------------------------------------------------------------------
def group_operands(w, sizes, seed):
    rng = np.random.default_rng(seed + w)
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n, G = int(seg[-1]), len(sizes)
    W = (R.normals(rng, G, w, w) / np.float32(np.sqrt(w))).astype(np.float32)
    return rng, seg, n, G, W, R.normals(rng, G, w)


def many_group_sizes():
    return list(np.random.default_rng(1).integers(1, 4, size=2 * n_cus() + 40))


def image_forward(w, sizes, tiles=False, stop=False):
    rng, seg, n, G, W, b = group_operands(w, sizes, 23)
    X = R.normals(rng, n, w)
    a = arena(stop).input("X", X, ld_of(w)).input("W", W.reshape(G, -1)).input("b", b).input("seg", seg).output("Y", n, w, ld_of(w))
    if tiles:
        t = image_tiles(seg, "cpu").numpy()
        a.input("tiles", t).build()
        run(a, "cl_wide_image_forward_tiles", a.ptr("X"), a.ld("X"), a.ptr("W"), a.ptr("b"), a.ptr("seg"), a.ptr("tiles"), len(t) // 2, w, LEAK, a.ptr("Y"), a.ld("Y"))
    else:
        a.build()
        run(a, "cl_wide_image_forward", a.ptr("X"), a.ld("X"), a.ptr("W"), a.ptr("b"), a.ptr("seg"), G, n, w, LEAK, a.ptr("Y"), a.ld("Y"))
    if stop:
        return a.verify(untouched=True)
    a.verify()
    R.assert_within(a.get("Y"), *R.image_forward(X, W, b, seg, LEAK), f"image_forward w {w} groups {G}", "cl_wide_image_forward" + ("_tiles" if tiles else ""))


def image_dgrad(w, sizes, tiles=False, stop=False):
    rng, seg, n, G, W, _ = group_operands(w, sizes, 29)
    dZ, H = R.normals(rng, n, w), R.with_zeros(rng, R.normals(rng, n, w))
    a = arena(stop).input("dZ", dZ, ld_of(w)).input("W", W.reshape(G, -1)).input("seg", seg).input("H", H, ld_of(w)).output("dX", n, w, ld_of(w))
    if tiles:
        t = image_tiles(seg, "cpu").numpy()
        a.input("tiles", t).build()
        run(a, "cl_wide_image_dgrad_tiles", a.ptr("dZ"), a.ld("dZ"), a.ptr("W"), a.ptr("seg"), a.ptr("tiles"), len(t) // 2, w, a.ptr("H"), a.ld("H"), LEAK, a.ptr("dX"), a.ld("dX"))
    else:
        a.build()
        run(a, "cl_wide_image_dgrad", a.ptr("dZ"), a.ld("dZ"), a.ptr("W"), a.ptr("seg"), G, n, w, a.ptr("H"), a.ld("H"), LEAK, a.ptr("dX"), a.ld("dX"))
    if stop:
        return a.verify(untouched=True)
    a.verify()
    R.assert_within(a.get("dX"), *R.image_dgrad(dZ, W, seg, H, LEAK), f"image_dgrad w {w} groups {G}", "cl_wide_image_dgrad" + ("_tiles" if tiles else ""))


def image_wgrad(w, sizes, stop=False):
    rng, seg, n, G, _, _ = group_operands(w, sizes, 31)
    dZ, H = R.normals(rng, n, w), R.normals(rng, n, w)
    a = arena(stop).input("dZ", dZ, ld_of(w)).input("H", H, ld_of(w)).input("seg", seg).output("dW", G, w * w).output("db", G, w).build()
    run(a, "cl_wide_image_wgrad", a.ptr("dZ"), a.ld("dZ"), a.ptr("H"), a.ld("H"), a.ptr("seg"), G, n, w, a.ptr("dW"), a.ptr("db"))
    if stop:
        return a.verify(untouched=True)
    a.verify()
    (dW, bW), (db, bb) = R.image_wgrad(dZ, H, seg)
    for g in np.flatnonzero(np.diff(seg) == 0):
        assert not a.get("dW")[g].any() and not a.get("db")[g].any(), f"empty group {g}: gradients not zero"
    R.assert_within(a.get("dW").reshape(G, w, w), dW, bW, f"image_wgrad w {w} groups {G}: dW", "cl_wide_image_wgrad")
    R.assert_within(a.get("db"), db, bb, f"image_wgrad w {w} groups {G}: db", "cl_wide_image_wgrad")


@pytest.mark.parametrize("w", [20, 72, 128])
def test_image_layers(w):
    """per-image layers on wide_stream_kernel<.., NAT 4 (w = 20) / 8, GRP = true> and the grouped weight gradient (wide_gemm_kernel BN 64 / 128
    over `seg`), groups of 0, 1, 15, 16, 17, 200, 0 and 3 rows: an empty group's dW, db come out zero"""
    image_forward(w, GROUP_SIZES)
    image_dgrad(w, GROUP_SIZES)
    image_wgrad(w, GROUP_SIZES)


def test_image_layers_with_more_groups_than_workgroups():
    """2 CUs + 40 groups of 1 .. 3 rows at w = 72: the grid is 2 CUs workgroups, 40 of them take a second group (`grp += gridDim.x`, the
    __syncthreads() between groups before the weights are staged again)"""
    sizes = many_group_sizes()
    image_forward(72, sizes)
    image_dgrad(72, sizes)
    image_wgrad(72, sizes)


@pytest.mark.parametrize("w", [144, 260])
def test_image_layers_tiles(w):
    """per-image layers wider than 128 on the tiled kernel, one x-block per (group, 128-row piece) of careless_amd.wide.image_tiles
    (the 200-row group takes two); w = 260: three column tiles, the last of four columns"""
    image_forward(w, GROUP_SIZES, tiles=True)
    image_dgrad(w, GROUP_SIZES, tiles=True)
    image_wgrad(w, GROUP_SIZES)


# ---- a raised stop flag: nothing is written -----------------------------------------------------------------------------------------------
STOPPED = {
    "cl_wide_dense_forward_sq": lambda: dense_forward(129, 100, 112, 1, stop=True),
    "cl_wide_dense_forward_stream": lambda: dense_forward(129, 70, 96, 1, stop=True),
    "cl_wide_dense_forward_tiled": lambda: dense_forward(129, 130, 96, 1, stop=True),
    "cl_wide_dense_forward_head": lambda: forward_head(129, 100, 112, 0, 1, stop=True),
    "cl_wide_dense_forward_head_lik": lambda: forward_head_lik(129, 100, 112, 4, stop=True),
    "cl_wide_dense2_forward": lambda: dense2_forward(129, 8, 100, 1, stop=True),
    "cl_wide_dense_dgrad": lambda: dense_dgrad(129, 112, 100, 1, stop=True),
    "cl_wide_dense_dgrad_pre": lambda: dgrad_pre(129, 8, 100, 100, stop=True),
    "cl_wide_dense_dgrad_pre_wgrad0": lambda: dgrad_pre_wgrad0(129, 8, 100, 100, stop=True),
    "cl_wide_dense_dgrad_head": lambda: dense_dgrad_head(129, 100, 100, stop=True),
    "cl_wide_dense_wgrad": lambda: dense_wgrad(677, 100, 100, 2, stop=True),
    "cl_wide_dense_wgrad_pre": lambda: dense_wgrad_pre(677, 8, 100, 100, 2, stop=True),
    "cl_wide_dense_wgrad_head": lambda: dense_wgrad_head(677, 100, 100, 2, stop=True),
    "cl_wide_head_forward": lambda: head_forward(129, 300, 0, stop=True),
    "cl_wide_head_backward": lambda: head_backward(129, 300, 0, 2, stop=True),
    "cl_wide_image_forward": lambda: image_forward(72, GROUP_SIZES, stop=True),
    "cl_wide_image_dgrad": lambda: image_dgrad(72, GROUP_SIZES, stop=True),
    "cl_wide_image_wgrad": lambda: image_wgrad(72, GROUP_SIZES, stop=True),
    "cl_wide_image_forward_tiles": lambda: image_forward(144, GROUP_SIZES, tiles=True, stop=True),
    "cl_wide_image_dgrad_tiles": lambda: image_dgrad(144, GROUP_SIZES, tiles=True, stop=True),
}


@pytest.mark.parametrize("entry", list(STOPPED))
def test_a_raised_stop_flag_leaves_every_output_untouched(entry):
    STOPPED[entry]()
