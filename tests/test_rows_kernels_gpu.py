"""The row-level data-term kernels on the GPU, call by call through the C ABI the engine calls (careless_amd._lib: FrozenArgs, LaueArgs,
DetArgs): `cl_frozen_rows` in its three forms (ROWS; GROUPS then SUMS), `cl_laue_predict` -> `cl_laue_likelihood` -> `cl_laue_backward`,
`cl_slot_rows` (plain and deterministic mode, followed by `cl_det_reduce`) and `cl_det_reduce` alone, against the ONE fp64 reference of
tests/ref_rows.py with a bound per element.  The layouts are built by hand so that the borders the kernels branch on are where the case says (tests/ref_rows.py: ROW_LAYOUTS,
rows_features; groups_layout): runs of equal reflections ending at lane 63, crossing one wave border, running through whole waves across the
256-row chunk border, two chains back to back, a chain into the ragged last wave, rows without a reflection, reflections without rows, and
n = 2048 * 256 + 3 * 256 + 37 rows, above the grid cap, where a workgroup walks two chunks and prefetches the second; rows in the caller's
order with harmonic groups of 1 .. 40 rows and padded slots, S on every reduction path of cl_slot_rows and one, two and three rounds of its
loop, one / a few / more than four images per wave (tests/ref_rows.py: LGPU_CASES).

Every operand is carved from one guarded allocation (ref_step.Guarded: 256 guard bytes around each, a mask of what the header lets the call
write) that is verified after every call; workspaces have exactly the documented size (edge_rid 2 ceil(n / 64) ints, edge_val
cl_frozen_edge_floats, nll_part cl_frozen_grid(n) doubles, ev11_part 3 * 4 * cl_frozen_grid(n) floats); outputs are preloaded with a
sentinel where the call stores and with values where it adds.

Bounds (tests/ref_rows.py; all tolerances are the project's): ipred within RTOL_LOSS M per element, the NLL within RTOL_LOSS max(M, 1), every
entry of dz_f, gbuf and d_ev11 within RTOL_GRAD M + one fp32 rounding of the stored value, M the entry's summand size; on the wide family also
RTOL_GRAD of the max-norm; reflections without rows bit-unchanged; the edge records (ROWS, SUMS) equal to what the layout implies; cl_det_reduce exact on the dyadic inputs and within n u sum |x| on floats.
The cases, their inputs and what the fp32 emulation reaches on them: tests/ref_rows.py, tests/test_ref_rows.py.

Measured on an MI355X, the largest ratio to the bound over all cases (in brackets: the fp32 emulation on the host build, glibc's expf /
logf / log1pf, on the same inputs):
    cl_frozen_rows ROWS       dz_f 4.0e-3 [4.0e-3]   max-norm 5.1e-3 [5.1e-3]   ipred 1.9e-3 [2.4e-3]   NLL 9.3e-4 [9.5e-4]   d_ev11 7.1e-4 [4.3e-4]
    cl_frozen_rows GROUPS     gbuf 0.14 [0.14]   gbuf max-norm 8.6e-3 [8.6e-3]   dz_f after SUMS 8.8e-4 [1.9e-3]   max-norm 1.2e-2 [1.2e-2]   NLL 1.1e-3 [1.1e-3]
    cl_laue_*                 iconv 3.8e-3 [6.0e-3]   dNLL/diconv 5.9e-3 [5.4e-3]   dz_f 4.6e-3 [5.2e-3]   dO 5.8e-3 [5.1e-3]   d_img 1.8e-3 [1.8e-3]   NLL 9.3e-4 [9.3e-4]
    cl_slot_rows              dz_f 1.2e-2 [1.8e-2]   dO 6.1e-3 [6.1e-3]   dO max-norm 7.4e-2 [7.4e-2]   d_img 4.3e-3 [4.0e-3]   NLL 1.1e-3 [1.1e-3]
    cl_slot_rows + cl_det_reduce   dz_f 7.3e-3   dO 1.3e-3   d_img 7.7e-4   d_ev11 0 (beyond the store's rounding); two runs bit for bit (det_slot NULL
                              with perm_refl; with det_slot set and perm_refl NULL, the engine's form: inside the same bounds, emulation dz_f 1.2e-2)
    cl_det_reduce alone       0 on the dyadic inputs; 0.49 [0.49] of n u sum |x| on floats (d_img 7.7e-3, d_ev11 0.20); two runs bit for bit
    in-kernel Philox (S = 1, 8, 9, 13, 2) = cl_debug_noise(kind 1) gathered by key: the same bits as the dumped normals injected
Nothing is outside a bound, nothing within a factor 7 of one, no guard was touched: edge_rid needs its 2 ceil(n / 64) ints and no more.
"""
import copy
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from careless_amd import _lib
from tests import ref_rows as RR
from tests import ref_step

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda"
F32 = np.float32
SEED, STEP = 20261, 5
WORST = ref_step.WORST                 # (entry point, quantity) -> largest ratio to its bound this session (printed, not a gate)
KIND = {"normal": _lib.CL_LIK_NORMAL, "studentt": _lib.CL_LIK_STUDENTT, "laplace": _lib.CL_LIK_LAPLACE}


def record(entry, ratios, what):
    for k, v in ratios.items():
        WORST[(entry, k)] = max(WORST.get((entry, k), 0.0), v)
    print(f"{what}: " + " ".join(f"{k} {v:.2e}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (what, "error / bound", bad)


def report(prefix):
    print("largest error / bound so far:", {f"{k[0]} {k[1]}": f"{v:.2e}" for k, v in sorted(WORST.items()) if k[0].startswith(prefix)})


def edge_sizes(n, S):
    lib = _lib.get_lib()
    W = (n + 63) // 64
    assert int(lib.cl_frozen_edge_floats(n, S)) == 2 * W * S and int(lib.cl_frozen_grid(n)) == RR.frozen_grid(n)
    return 2 * W, 2 * W * S, RR.frozen_grid(n)


class FrozenRun:
    """The operands of one cl_frozen_rows case in a guarded allocation and the argument block(s) that point at them.  philox: eta NULL, the
    kernel draws (SEED, STEP)."""

    def __init__(self, x, stop=False, philox=False):
        c, n, S, R = x.case, x.n, x.S, x.R
        self.x, self.rows = x, x.entry == "rows"
        g = ref_step.Guarded(DEV).add("refl", x.refl_id).add("loc", x.loc).add("sigma", x.sigma).add("iobs", x.iobs).add("sig", x.sig).add("z_f", x.z_f)
        g.add("eta", x.eta).add("stop", np.array([1 if stop else 0], np.int32))
        if x.aim is not None:
            g.add("aim", x.aim)
        if x.key is not None:
            g.add("key", x.key)
        n_edge = n if self.rows else x.n2
        ne, nf, grid = edge_sizes(n_edge, S)
        self.grid = RR.frozen_grid(n)
        g.add("dz", x.dz_pre, np.repeat(x.has_rows[:, None], S, axis=1))
        g.add("edge_rid", np.full(ne, -77, np.int32), True).add("edge_val", np.full(nf, RR.SENT, F32), True)
        g.add("scalars", np.array([x.nll_pre, 1.25, 7.0, 6.0]), [c.nll == "atomic", False, False, False])
        if c.nll == "part":
            g.add("nll_part", np.zeros(self.grid), True)
        if c.ipred_out:
            m = np.zeros((n, S), bool)
            m[x.krow[x.act]] = True
            g.add("ipred", np.full((n, S), RR.SENT, F32), m)
        if c.ev11:
            g.add("ev11", x.ev11).add("d_ev11", x.ev_pre, c.ev11 == "atomic")
            g.add("ev11_part", np.zeros(3 * 4 * self.grid, F32), c.ev11 == "part")
        if not self.rows:
            g.add("gmeta", x.gmeta).add("dst", x.dst).add("order", x.order.astype(np.int32)).add("refl_sorted", x.refl_sorted)
            g.add("gbuf", np.full((x.n2 if c.src else n, S), RR.SENT, F32), True)
        self.g = g.build()
        A = _lib.FrozenArgs()
        A.refl_id, A.loc, A.sigma, A.iobs, A.sig, A.z_f = (g.ptr(k) for k in ("refl", "loc", "sigma", "iobs", "sig", "z_f"))
        A.aim, A.key = g.ptr("aim" if x.aim is not None else None), g.ptr("key" if x.key is not None else None)
        A.obs_offset, A.n, A.R, A.S = x.obs_offset, n, R, S
        A.lik_kind, A.dof, A.lik_const, A.shift, A.w_ll = KIND[x.kind], float(x.dof), float(x.lik_const), float(x.shift), float(x.w_ll)
        A.eta, A.seed, A.step = (None, SEED, STEP) if philox else (g.ptr("eta"), 0, 0)
        A.scalars, A.stop_flag = g.ptr("scalars"), g.ptr("stop")
        A.nll_part = g.ptr("nll_part" if c.nll == "part" else None)
        A.ipred_out = g.ptr("ipred" if c.ipred_out else None)
        if c.ev11:
            A.ev11 = g.ptr("ev11")
            A.d_ev11, A.ev11_part = (g.ptr("d_ev11"), None) if c.ev11 == "atomic" else (None, g.ptr("ev11_part"))
        self.A, self.B = A, None
        if self.rows:
            A.dz_f, A.accumulate, A.edge_rid, A.edge_val = g.ptr("dz"), c.accumulate, g.ptr("edge_rid"), g.ptr("edge_val")
        else:
            A.gmeta, A.gbuf, A.src = g.ptr("gmeta"), g.ptr("gbuf"), g.ptr("dst" if c.src else None)
            B = _lib.FrozenArgs()                                      # (the second call reads the first one's gradients and a handful of fields)
            B.refl_id, B.gbuf, B.src = g.ptr("refl_sorted"), g.ptr("gbuf"), g.ptr(None if c.src else "order")
            B.n, B.R, B.S, B.dz_f, B.stop_flag, B.accumulate = x.n2, R, S, g.ptr("dz"), g.ptr("stop"), c.accumulate
            B.edge_rid, B.edge_val = g.ptr("edge_rid"), g.ptr("edge_val")
            self.B = B

    def call(self, A=None, expect=0, untouched=False):
        ret = int(_lib.get_lib().cl_frozen_rows(C.byref(self.A if A is None else A), None))
        torch.cuda.synchronize()
        assert ret == expect, (self.x.case.id, ret, expect)
        self.g.verify(untouched=untouched)           # guards, inputs, reflections without rows, slots nobody owns: bit-identical; stopped / refused: everything
        return self

    def sequence(self, untouched=False):
        """ROWS: the call.  GROUPS then SUMS: gbuf is taken right behind the first call, which leaves dz_f and the edge workspace alone; the
        second call only reads gbuf."""
        self.call(untouched=untouched)
        if self.rows:
            return self
        self.gbuf_groups = self.g.get("gbuf").copy()
        assert not any(self.g.changed(k).any() for k in ("dz", "edge_rid", "edge_val")), self.x.case.id
        self.call(self.B, untouched=untouched)
        assert np.array_equal(self.g.get("gbuf").view(np.uint32), self.gbuf_groups.view(np.uint32)), self.x.case.id
        return self

    def result(self):
        g, x, c = self.g, self.x, self.x.case
        nll = float(g.get("nll_part").sum()) if c.nll == "part" else float(g.get("scalars")[_lib.CL_SC_NLL]) - x.nll_pre
        out = SimpleNamespace(dz=g.get("dz").copy(), nll=nll, ipred=g.get("ipred").copy() if c.ipred_out else None, d_ev11=None, gbuf=None,
                              edge_rid=g.get("edge_rid").copy(), parts=g.get("nll_part").copy() if c.nll == "part" else None)
        if c.ev11:
            out.d_ev11 = g.get("d_ev11").copy() if c.ev11 == "atomic" else g.get("ev11_part").astype(np.float64).reshape(-1, 3).sum(0)
        if not self.rows:
            out.gbuf = self.gbuf_groups if c.src else self.gbuf_groups[x.order]      # (what GROUPS left, before SUMS ran)
        return out


def check(run, ref, what=None):
    x, c = run.x, run.x.case
    got = run.result()
    what = what or c.id
    assert np.all(np.isfinite(got.dz[x.has_rows])) and np.all(got.dz[x.has_rows] != F32(RR.SENT)), what
    if c.ipred_out:
        assert np.all(got.ipred[x.krow[x.act]] != F32(RR.SENT)), what
    if not run.rows and not c.src:                                     # a padding position of gbuf in position order holds the zero the kernel stores
        assert np.all(run.gbuf_groups[~x.act] == 0.0), what
    record(f"cl_frozen_rows {x.entry}", RR.rows_ratios(x, ref, got), what)
    return got


def same_bits(a, b):
    ok = np.array_equal(a.dz.view(np.uint32), b.dz.view(np.uint32)) and np.array_equal(a.edge_rid, b.edge_rid)
    if a.parts is not None:
        ok = ok and a.parts.tobytes() == b.parts.tobytes()
    if a.gbuf is not None:
        ok = ok and np.array_equal(a.gbuf.view(np.uint32), b.gbuf.view(np.uint32))
    return ok


# ---- cl_frozen_rows: every case against the fp64 reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", RR.GPU_CASES, ids=lambda c: c.id)
def test_frozen_rows_match_fp64(c):
    x, ref = RR.reference_for(c)
    got = check(FrozenRun(x).sequence(), ref)
    if not c.accumulate:                                               # no atomic touches dz_f: a second run gives the same bits
        assert same_bits(got, FrozenRun(x).sequence().result()), c.id
    report("cl_frozen_rows")


@pytest.mark.parametrize("layout,S,key", [("through", 1, True), ("through", 8, True), ("back2back", 9, False), ("n641", 13, True), ("negwave", 2, True)])
def test_in_kernel_noise_is_cl_debug_noise_kind_1_gathered_by_key(layout, S, key):
    """eta NULL: the kernel draws the normals of (seed, step) keyed by the row's global number -- one Philox block and Box-Muller pair serving
    samples s and s + 4 of a batch of eight, a ragged second batch at S = 9 and 13, the instance of its own at S = 1.  The reference consumes
    cl_debug_noise(kind 1) of the same (seed, step, offset); the same normals injected give the same bits."""
    c = RR.case("rows", layout, S, key=key, nll="part", ipred_out=True)
    x = copy.copy(RR.make_inputs(c))
    dump = torch.empty(x.n * S, dtype=torch.float32, device=DEV)
    assert int(_lib.get_lib().cl_debug_noise(SEED, STEP, S, x.n, x.obs_offset, 1, dump.data_ptr(), None)) == 0
    torch.cuda.synchronize()
    x.eta = dump.cpu().numpy().reshape(x.n, S)
    x.eta_row = x.eta[x.krow]
    assert np.all(np.isfinite(x.eta)) and 0.5 < x.eta.std() < 1.5
    ref = RR.reference(x)
    drawn = check(FrozenRun(x, philox=True).sequence(), ref, what=f"{c.id}-philox")
    injected = check(FrozenRun(x).sequence(), ref, what=f"{c.id}-dumped-normals")
    assert same_bits(drawn, injected) and np.array_equal(drawn.ipred.view(np.uint32), injected.ipred.view(np.uint32)), c.id
    # another row's normals move the predictions by far more than their bound
    xw = copy.copy(x)
    xw.eta_row = np.roll(x.eta_row, 1, axis=0)
    moved = np.abs(RR.reference(xw, values_only=True).ipred - ref.ipred)[x.act] / (RR.RTOL_LOSS * ref.M_ipred[x.act] + 1e-300)
    assert np.median(moved) > 10.0, float(np.median(moved))


STOP_CASES = [RR.case("rows", "through", 8, ev11="atomic", ipred_out=True), RR.case("rows", "back2back", 1, nll="part", ev11="part", kind="studentt"),
              RR.case("groups", 65, 3, ev11="atomic", ipred_out=True)]


@pytest.mark.parametrize("c", STOP_CASES, ids=lambda c: c.id)
def test_a_raised_stop_flag_makes_every_call_write_nothing(c):
    FrozenRun(RR.make_inputs(c), stop=True).sequence(untouched=True)    # outputs AND workspaces


def test_refusals_on_real_buffers_return_their_code_and_write_nothing():
    x = RR.make_inputs(RR.case("rows", "through", 8, ev11="atomic"))
    run = FrozenRun(x)
    base = bytes(run.A)
    for fields, expect in ((dict(lik_kind=_lib.CL_LIK_LAPLACE), -1), (dict(d_ev11=None), -1), (dict(n=0), -1), (dict(S=0), -1), (dict(R=1 << 30), -4),
                           (dict(lik_kind=7), -1), (dict(n=(1 << 31) - 64), -4)):
        C.memmove(C.byref(run.A), base, len(base))
        for k, v in fields.items():
            setattr(run.A, k, v)
        run.call(expect=expect, untouched=True)
    xg = RR.make_inputs(RR.case("groups", 65, 3))
    rg = FrozenRun(xg)
    rg.A.gbuf = None
    rg.call(expect=-1, untouched=True)
    rg.B.R = 1 << 30
    rg.call(rg.B, expect=-4, untouched=True)


# ---- cl_det_reduce ----------------------------------------------------------------------------------------------------------------------------------
class DetRun:
    def __init__(self, x, stop=False):
        c = x.case
        self.x = x
        g = ref_step.Guarded(DEV).add("dzf_obs", x.dzf_obs).add("seg_refl", x.seg_refl).add("dz", x.dz_pre, True)
        if x.perm_refl is not None:
            g.add("perm_refl", x.perm_refl)
        g.add("dimg_obs", x.dimg_obs).add("perm_img", x.perm_img if len(x.perm_img) else np.zeros(1, np.int32)).add("seg_img", x.seg_img)
        k = x.n_images - 1
        g.add("d_img", x.img_pre, ([True] * k + [False] * (len(x.img_pre) - k)) if c.d_img else False)
        g.add("nll_part", x.nll_part).add("scalars", np.array([x.nll_pre, 1.25, 7.0, 6.0]), [True, False, False, False])
        g.add("ev11_part", x.ev11_part).add("d_ev11", x.ev_pre, x.n_ev11 > 0).add("stop", np.array([1 if stop else 0], np.int32))
        self.g = g.build()
        A = _lib.DetArgs()
        A.dzf_obs, A.perm_refl, A.seg_refl, A.R, A.S, A.dz_f = g.ptr("dzf_obs"), g.ptr("perm_refl" if x.perm_refl is not None else None), g.ptr("seg_refl"), x.R, x.S, g.ptr("dz")
        A.dimg_obs, A.perm_img, A.seg_img, A.n_images, A.d_img = g.ptr("dimg_obs"), g.ptr("perm_img"), g.ptr("seg_img"), x.n_images, g.ptr("d_img" if c.d_img else None)
        A.nll_part, A.nparts, A.scalars, A.stop_flag = g.ptr("nll_part"), x.nparts, g.ptr("scalars"), g.ptr("stop")
        if x.n_ev11:
            A.ev11_part, A.n_ev11, A.d_ev11 = g.ptr("ev11_part"), x.n_ev11, g.ptr("d_ev11")
        self.A = A

    def call(self, untouched=False):
        assert int(_lib.get_lib().cl_det_reduce(C.byref(self.A), None)) == 0
        torch.cuda.synchronize()
        self.g.verify(untouched=untouched)
        g = self.g
        return SimpleNamespace(dz=g.get("dz").copy(), d_img=g.get("d_img").copy(), nll=float(g.get("scalars")[0]), d_ev11=g.get("d_ev11").copy())


@pytest.mark.parametrize("c", RR.DET_CASES, ids=lambda c: c.id)
def test_det_reduce_alone(c):
    """Every output preloaded (the call adds).  On the dyadic inputs every fp32 sum is exact and the result must EQUAL the fp64 sum; on floats
    the a-priori fp32 bound; two runs bit for bit -- what the kernel exists for."""
    x = RR.det_inputs(c)
    ref = RR.det_reference(x)
    got = DetRun(x).call()
    r = RR.det_ratios(x, ref, got)
    record("cl_det_reduce" + ("" if c.dyadic else " floats"), r, c.id)
    if c.dyadic:
        assert all(v == 0.0 for v in r.values()), (c.id, r)
    again = DetRun(x).call()
    assert all(getattr(got, k).tobytes() == getattr(again, k).tobytes() for k in ("dz", "d_img", "d_ev11")) and got.nll == again.nll, c.id
    if not c.d_img:
        assert np.array_equal(got.d_img.view(np.uint32), x.img_pre.view(np.uint32))


def test_det_reduce_under_a_raised_stop_flag_writes_nothing():
    DetRun(RR.det_inputs(RR.det_case(17, 5, 6, 65, 257)), stop=True).call(untouched=True)


# ---- rows in the caller's order: cl_laue_predict -> cl_laue_likelihood -> cl_laue_backward, and cl_slot_rows -------------------------------------
class LaueRun:
    """The operands of one Laue / slot case in a guarded allocation and the cl_laue_args that point at them.  The masks are the union over the
    calls of the case; what a single call must leave alone beyond them is asserted after it (`quiet`)."""

    def __init__(self, x, stop=False, philox=None):
        c, n, S, R = x.case, x.n, x.S, x.R
        self.x, self.laue = x, x.entry == "laue"
        use_img = x.img is not None
        g = ref_step.Guarded(DEV).add("refl", x.refl_id).add("loc", x.loc).add("sigma", x.sigma).add("iobs", x.iobs).add("sig", x.sig).add("z_f", x.z_f)
        g.add("eta", x.eta).add("stop", np.array([1 if stop else 0], np.int32))
        if use_img:
            present = np.zeros(len(x.img), bool)
            present[np.unique(x.image_id[x.image_id > 0]) - 1] = True
            if c.det:
                present[:] = False
                present[:x.n_images - 1] = True
            g.add("image_id", x.image_id).add("img", x.img).add("d_img", x.img_pre, present if c.dO else False)
        if self.laue:
            g.add("harmonic", x.slot).add("iconv", np.zeros((n, S), F32), True)
        else:
            g.add("iconv", np.full(4, RR.SENT, F32))                  # (rows that are their own slot never touch it)
        g.add("dz", x.dz_pre, True if c.det else np.repeat(x.has_rows[:, None], S, axis=1))
        if c.dO:
            g.add("dO", np.full((n, 2), RR.SENT, F32), True)
        self.grid = min((n * S + 255) // 256, RR.CAP)
        g.add("scalars", np.array([x.nll_pre, 1.25, 7.0, 6.0]), [True if c.det else c.nll == "atomic", False, False, False])
        if c.nll == "part":
            g.add("nll_part", np.zeros(self.grid), True)
        if c.ipred_out:
            g.add("ipred", np.full((n, S), RR.SENT, F32), True)
        if c.ev11:
            g.add("ev11", x.ev11).add("d_ev11", x.ev_pre, c.ev11 == "atomic" or c.det).add("ev11_part", np.zeros(3 * 4 * self.grid, F32), c.ev11 == "part")
        if c.det:
            if x.det_slot is None:
                g.add("dzf_obs", np.full((n, S), RR.SENT, F32), True).add("perm_refl", x.perm_refl)
            else:                                                      # records nobody owns in front of and behind the observations' slots: not writable
                self.owned = np.zeros((n + RR.DET_LEAD + RR.DET_TAIL, S), bool)
                self.owned[x.det_slot] = True
                assert self.owned[RR.DET_LEAD:RR.DET_LEAD + n].all() and self.owned.sum() == n * S
                g.add("dzf_obs", np.full(self.owned.shape, RR.SENT, F32), self.owned).add("det_slot", x.det_slot)
            g.add("dimg_obs", np.full(n, RR.SENT, F32), use_img)
            g.add("seg_refl", x.seg_refl).add("perm_img", x.perm_img).add("seg_img", x.seg_img)
        if philox == "row_index":
            g.add("row_index", (x.obs_offset + np.arange(n, dtype=np.int64)).view(np.float64))      # (the bytes of the int64 list)
        self.g = g.build()
        A = _lib.LaueArgs()
        A.refl_id, A.loc, A.sigma, A.iobs, A.sig, A.z_f = (g.ptr(k) for k in ("refl", "loc", "sigma", "iobs", "sig", "z_f"))
        A.harmonic_id = g.ptr("harmonic" if self.laue else None)
        A.n_obs, A.R, A.S, A.obs_offset = n, R, S, 0 if philox == "row_index" else x.obs_offset
        A.use_img = int(use_img)
        if use_img:
            A.image_id, A.img, A.d_img = g.ptr("image_id"), g.ptr("img"), g.ptr("d_img")
        A.lik_kind, A.dof, A.lik_const, A.shift, A.w_ll = KIND[x.kind], float(x.dof), float(x.lik_const), float(x.shift), float(x.w_ll)
        A.eta, A.seed, A.step = (None, SEED, STEP) if philox else (g.ptr("eta"), 0, 0)
        A.row_index = g.ptr("row_index" if philox == "row_index" else None)
        A.iconv, A.dz_f, A.dO, A.scalars, A.stop_flag = g.ptr("iconv"), g.ptr("dz"), g.ptr("dO" if c.dO else None), g.ptr("scalars"), g.ptr("stop")
        A.ipred_out, A.nll_part = g.ptr("ipred" if c.ipred_out else None), g.ptr("nll_part" if c.nll == "part" else None)
        if c.ev11:
            A.ev11 = g.ptr("ev11")
            A.d_ev11, A.ev11_part = (g.ptr("d_ev11"), None) if c.ev11 == "atomic" else (None, g.ptr("ev11_part"))
        if c.det:
            A.dzf_obs, A.dimg_obs = g.ptr("dzf_obs"), g.ptr("dimg_obs" if use_img else None)
            A.det_slot = g.ptr("det_slot" if x.det_slot is not None else None)
        self.A = A

    def call(self, name, expect=0, untouched=False, quiet=()):
        before = self.g.download().copy() if quiet else None
        ret = int(getattr(_lib.get_lib(), name)(C.byref(self.A), None))
        torch.cuda.synchronize()
        assert ret == expect, (self.x.case.id, name, ret, expect)
        self.g.verify(untouched=untouched)
        for k in quiet:                                                # operands another call of the case may write: THIS call left their bytes alone
            o = self.g.ops.get(k)
            assert o is None or np.array_equal(before[o["start"]:o["start"] + o["nbytes"]], self.g.got[o["start"]:o["start"] + o["nbytes"]]), (self.x.case.id, name, k)
        return self

    def det_reduce(self):
        g, x, c = self.g, self.x, self.x.case
        D = _lib.DetArgs()
        D.dzf_obs, D.perm_refl, D.seg_refl, D.R, D.S, D.dz_f = g.ptr("dzf_obs"), g.ptr("perm_refl" if x.det_slot is None else None), g.ptr("seg_refl"), x.R, x.S, g.ptr("dz")
        if x.img is not None:
            D.dimg_obs, D.perm_img, D.seg_img, D.n_images, D.d_img = g.ptr("dimg_obs"), g.ptr("perm_img"), g.ptr("seg_img"), x.n_images, g.ptr("d_img")
        D.nll_part, D.nparts, D.scalars, D.stop_flag = g.ptr("nll_part"), self.grid, g.ptr("scalars"), g.ptr("stop")
        if c.ev11:
            D.ev11_part, D.n_ev11, D.d_ev11 = g.ptr("ev11_part"), 4 * self.grid, g.ptr("d_ev11")
        assert int(_lib.get_lib().cl_det_reduce(C.byref(D), None)) == 0
        torch.cuda.synchronize()
        g.verify()
        return self

    def nll(self):
        g, c = self.g, self.x.case
        if c.nll == "part" and not c.det:
            return float(g.get("nll_part").sum())
        return float(g.get("scalars")[_lib.CL_SC_NLL]) - self.x.nll_pre

    def result(self, **kw):
        g, x, c = self.g, self.x, self.x.case
        out = SimpleNamespace(nll=self.nll(), dz=g.get("dz").copy(), dO=g.get("dO").copy() if c.dO else None, d_img=g.get("d_img").copy() if x.img is not None else None,
                              ipred=g.get("ipred").copy() if c.ipred_out else None, d_ev11=None, **kw)
        if c.ev11:
            out.d_ev11 = g.get("d_ev11").copy() if (c.ev11 == "atomic" or c.det) else g.get("ev11_part").astype(np.float64).reshape(-1, 3).sum(0)
        return out


BACKWARD_ONLY = ("dz", "dO", "d_img")


def run_laue(x, **kw):
    """the three calls, with what each wrote taken right behind it"""
    run = LaueRun(x, **kw)
    run.call("cl_laue_predict", quiet=BACKWARD_ONLY + ("scalars", "d_ev11", "nll_part", "ev11_part"))
    iconv = run.g.get("iconv").copy()
    run.call("cl_laue_likelihood", quiet=BACKWARD_ONLY + ("ipred",))
    dconv = run.g.get("iconv").copy()
    run.call("cl_laue_backward", quiet=("iconv", "scalars", "d_ev11", "nll_part", "ev11_part", "ipred"))
    return run, run.result(iconv=iconv, dconv=dconv)


def run_slot(x, **kw):
    run = LaueRun(x, **kw)
    if x.case.det:
        run.call("cl_slot_rows", quiet=("dz", "d_img", "scalars", "d_ev11", "iconv"))
        wrote = run.g.changed("dzf_obs")
        assert (wrote.all() if x.det_slot is None else wrote[run.owned].all()) and run.g.changed("dO").all()
        run.det_reduce()
    else:
        run.call("cl_slot_rows", quiet=("iconv",))
    return run, run.result()


@pytest.mark.parametrize("c", RR.LGPU_CASES, ids=lambda c: c.id)
def test_laue_calls_and_slot_rows_match_fp64(c):
    x, ref = RR.lreference_for(c)
    run, got = (run_laue if x.entry == "laue" else run_slot)(x)
    if c.dO:
        assert np.all(got.dO != F32(RR.SENT)), c.id                    # the store path overwrites the sentinel, the atomic path clears it and adds
    record("cl_laue_*" if x.entry == "laue" else ("cl_slot_rows + cl_det_reduce" if c.det else "cl_slot_rows"), RR.laue_ratios(x, ref, got), c.id)
    if c.det:                                                          # the pair is reproducible: two runs, the same bits
        again = run_slot(x)[1]
        assert all(getattr(got, k) is None or getattr(got, k).tobytes() == getattr(again, k).tobytes() for k in ("dz", "dO", "d_img", "d_ev11")) and got.nll == again.nll, c.id
    report("cl_laue" if x.entry == "laue" else "cl_slot")


def test_laue_in_kernel_noise_by_obs_offset_and_by_row_index():
    """eta NULL: the normals of (seed, step) keyed by obs_offset + i, or by row_index[i] -- the same rows named both ways predict the same
    bits (the group sums behind them are float atomics: within the bounds, not bit for bit), and the reference on cl_debug_noise(kind 1) of
    that range holds the bounds"""
    c = RR.lcase("laue", 300, 5, img_run=30, ipred_out=True)
    x = copy.copy(RR.lreference_for(c)[0])
    dump = torch.empty(x.n * x.S, dtype=torch.float32, device=DEV)
    assert int(_lib.get_lib().cl_debug_noise(SEED, STEP, x.S, x.n, x.obs_offset, 1, dump.data_ptr(), None)) == 0
    torch.cuda.synchronize()
    x.eta = x.eta_row = dump.cpu().numpy().reshape(x.n, x.S)
    ref = RR.reference(x)
    by_offset = run_laue(x, philox="obs_offset")[1]
    by_index = run_laue(x, philox="row_index")[1]
    record("cl_laue_*", RR.laue_ratios(x, ref, by_offset), c.id + "-philox")
    record("cl_laue_*", RR.laue_ratios(x, ref, by_index), c.id + "-philox-row_index")
    assert by_offset.ipred.tobytes() == by_index.ipred.tobytes()


@pytest.mark.parametrize("c", [RR.lcase("laue", 300, 3, img_run=50, ev11="atomic", ipred_out=True), RR.lcase("slot", 300, 9, img_run=8, ev11="atomic", ipred_out=True),
                               RR.lcase("slot", 300, 4, img_run=24, det=True, nll="part", ev11="part")], ids=lambda c: c.id)
def test_laue_and_slot_calls_under_a_raised_stop_flag_write_nothing(c):
    x = RR.lreference_for(c)[0]
    run = LaueRun(x, stop=True)
    for name in (("cl_laue_predict", "cl_laue_likelihood", "cl_laue_backward") if x.entry == "laue" else ("cl_slot_rows",)):
        # where dO is filled by atomics (cl_laue_backward; cl_slot_rows when S does not divide 64) its clearing is a memset on the stream in
        # front of the launch: part of the call whatever the flag says.  Nobody reads dO of a stopped step; everything else keeps its bits.
        clears = name == "cl_laue_backward" or (name == "cl_slot_rows" and 64 % c.S != 0)
        run.call(name, untouched=not clears)
        if clears:
            assert not any(k in run.g.ops and run.g.changed(k).any() for k in ("dz", "d_img", "scalars", "d_ev11", "ipred", "iconv", "nll_part", "ev11_part"))
            assert np.all(run.g.get("dO") == 0.0)


def test_slot_rows_refusals_write_nothing():
    x = RR.lreference_for(RR.lcase("laue", 300, 3, img_run=50, ev11="atomic", ipred_out=True))[0]
    LaueRun(x).call("cl_slot_rows", expect=-2, untouched=True)            # harmonic_id set: rows that share slots need the three passes
    xs = RR.make_linputs(RR.lcase("slot", 300, 4, img_run=24, det=True, det_slot=True, nll="part"))
    xs.S, xs.w_ll = 3, F32(1.0 / 3)                                      # deterministic mode: S must divide 64 (the operands keep their S = 4 sizes)
    LaueRun(xs).call("cl_slot_rows", expect=-2, untouched=True)
