"""Every instance of the lane-per-observation kernel (csrc/elbo_lane.hip) and of the narrow kernel (csrc/elbo_narrow.hip) without per-image
layers, called directly through the C ABI (cl_elbo_mono_fwd_bwd, cl_mlp_forward, cl_mlp_backward_ext; cl_reduce_partials and cl_det_reduce behind
them) and held, launch by launch and element by element, to the ONE fp64 reference of tests/ref_mlp.py -- as tests/test_mlp_kernels_gpu.py does
for csrc/elbo_mlp.hip, with its harness (Run: one guarded allocation with a write mask, workspaces at their documented size, sentinels, preloads).

The case list is generated (tests/ref_lane.py): one case per instance name and one more per full instance in its deterministic run-time form at
n = 17 * 64 + 37 rows on two workgroups (eighteen 64-row wave tiles on eight waves, the last ragged; the narrow kernel's tile is 32 rows), the
shape cycling through the instance's rim values; per (kernel, layout, metadata form) the row borders (3, the tile and one more, 128 on one
workgroup, 256 | 257, 1125 on one workgroup, a clamped grid), the MC sample counts 1 .. 17, bijectors, image scales, ipred_out, the Evans-2011
buffers, det_slot, noise_row, harmonic groups, a raised stop flag; the head-less blocks (MODE 1 / 2) at their own borders.  Every launch asserts
cl_mlp_check == 0 and that cl_mlp_route / cl_mlp_kernel_name give the route and the instance of the launch rules RESTATED in ref_lane.

Three contracts of include/careless_hip.h are pinned here:
  * dZ0_out: every element below n_obs in rows < w holds dL/d(pre-activations of layer 0) (RTOL_GRAD M + one rounding); behind n_obs the kernel
    stores exact zeros up to the end of the wave tile (64 columns; 32 on the narrow kernel) and nothing behind that, nor in rows [w, meta_rows(w)):
    the caller clears the buffer once (cl_peel_backward reads every column up to n_pad);
  * ev11_part: the lane kernel has four waves and stores slots 0 .. 3 of a workgroup's CL_EV11_WAVES = 8; slots 4 .. 7 keep their bytes (the
    caller's zeros: cl_det_reduce adds all eight);
  * act_out of a lane block: whole 64-column wave tiles are stored; rows [w, meta_rows(w)) and the columns behind the last wave tile keep their bytes.

Total time of this file on an MI355X: 815 tests (some 1400 launches) in 12 s; the largest ratios met are in DESIGN section 2.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from careless_amd import _lib
from tests import ref_lane as RL
from tests import ref_mlp as RM
from tests import ref_step
from tests import test_mlp_kernels_gpu as TM

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda"
F32 = np.float32
WORST = {}
ROUTE = {"lane": _lib.CL_ROUTE_LANE, "narrow": _lib.CL_ROUTE_NARROW, "lane_block": _lib.CL_ROUTE_LANE_BLOCK}


def record(c, ratios, what=None):
    for k, v in ratios.items():
        key = (str(RL.route(c)), k)
        WORST[key] = max(WORST.get(key, 0.0), v)
    print(f"{what or c.id}: " + " ".join(f"{k} {v:.2e}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (what or c.id, "error / bound", bad)


class Run(TM.Run):
    """a launch on the lane or narrow kernel: whole wave tiles of act_out / dZ0_out, the kernel's own wave count, the restated launch rules"""

    def wave_tile(self):
        return RM.WAVES[self.c.kernel][1]

    def stored_columns(self):
        wt = self.wave_tile()
        return min((self.x.np_ + wt - 1) // wt * wt, self.x.n_pad)

    def act_mask(self, live):
        m = np.zeros((RM.meta_rows(self.x.w), self.x.n_pad), bool)
        m[:self.x.w] = live                                            # (the padding rows [w, meta_rows(w)) keep their bytes: the caller's zeros)
        return m

    def check_act(self, act):
        x = self.x
        assert np.all(act[:x.w, :x.np_] != F32(RM.SENT)) and np.all(np.isfinite(act[:x.w, :self.stored_columns()])), self.c.id      # (behind n_obs: the activations of zero metadata)

    def ev11_waves(self):
        return RM.WAVES[self.c.kernel][0]

    def more_operands(self, g):
        if self.c.dz0:
            x = self.x
            m = np.zeros((RM.meta_rows(x.w), x.n_pad), bool)
            m[:x.w, :self.stored_columns()] = True
            g.add("dZ0_out", np.full(m.shape, RM.SENT, F32), m)

    def more_args(self, A, opt):
        A.dZ0_out = opt("dZ0_out")

    def check_instance(self, route, inst):
        c = self.c
        name = inst[:-len(" generic")]
        assert inst.endswith(" generic") and route == ROUTE[RL.route(c)] and name == RL.expected_instance(c) == getattr(c, "instance", name), (c.id, route, inst, RL.expected_instance(c))

    def result(self):
        out, x = super().result(), self.x
        if self.c.dz0:
            dz0 = self.g.get("dZ0_out").copy()
            sent = F32(RM.SENT)
            # every element below n_obs written; exact zeros in the rest of the ragged wave tile; (the columns behind and the padding rows: the mask)
            assert np.all(dz0[:x.w, :x.np_] != sent) and np.all(dz0[:x.w, x.np_:self.stored_columns()] == 0.0), self.c.id
            assert np.all(dz0[x.w:] == sent) and np.all(dz0[:, self.stored_columns():] == sent), self.c.id
            out.dz0 = dz0
        return out


CASES = RL.cases()


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_launch_matches_fp64(c):
    x, ref = TM.inputs_of(c)
    run = Run(x, ref).launch()
    got = run.result()
    record(c, RM.ratios(x, ref, run.pre, got))
    if c.det:
        assert not any(run.g.changed(k).any() for k in ("dz_f", "d_img", "scalars", "d_ev11") if k in run.g.ops), c.id
        again = Run(x, ref).launch().result()
        assert all(getattr(got, k, None) is None or getattr(got, k).tobytes() == getattr(again, k).tobytes() for k in TM.SAME + ("dz0",)), c.id
        record(c, RM.ratios(x, ref, run.pre, run.det_reduce()), c.id + " + cl_det_reduce")


@pytest.mark.parametrize("c", RL.stop_cases(), ids=lambda c: c.id)
def test_a_raised_stop_flag_leaves_every_output_and_workspace_as_it_was(c):
    x, ref = RM.reference_for(c)
    Run(x, ref, stop=True).launch(untouched=True)


class RunSentinelSlots(Run):
    EV11_FILL = RM.SENT                                                # (no cl_det_reduce behind this launch: nothing adds the slots)


@pytest.mark.parametrize("packed", (False, True), ids=("plain", "packed"))
def test_the_lane_kernel_never_writes_the_wave_slots_4_to_7_of_ev11_part(packed):
    """with the sentinel in the slots the kernel has no wave for, "kept" is "never written" (a stored 0.0 would show); slots 0 .. 3 all written"""
    c = RL.lcase(10, 15, 20, packed=packed, det=True, ev11=True, S=3, n=5 * 64 + 37, groups=packed, tag="slots")
    x, ref = RM.reference_for(c)
    run = RunSentinelSlots(x, ref).launch()                            # (verify: every byte outside the mask -- slots 4 .. 7 -- as it was)
    part = run.g.get("ev11_part")
    assert RL.route(c) == "lane" and np.all(part[:x.grid_eff, 12:] == F32(RM.SENT)) and np.all(part[:x.grid_eff, :12] != F32(RM.SENT))


@pytest.mark.parametrize("c,why", RL.refusal_cases(), ids=lambda v: v.id if hasattr(v, "id") else None)
def test_arguments_off_these_routes_are_routed_elsewhere_or_refused_without_a_launch(c, why):
    x, ref = RM.reference_for(c)
    run = Run(x, ref)
    lib = _lib.get_lib()
    route, inst = run.instance()
    want = RL.route(c)
    if RL.refused(c):
        assert route == _lib.CL_ROUTE_NONE and int(lib.cl_mlp_check(C.byref(run.A), 0, c.grid)) == -2, (c.id, why, route)
        assert int(lib.cl_elbo_mono_fwd_bwd(C.byref(run.A), c.grid, None)) == -2, (c.id, why)
        torch.cuda.synchronize()
        run.g.verify(untouched=True)
    else:
        assert route == (ROUTE[want] if want else TM.ROUTE[c.unit]) and route != _lib.CL_ROUTE_LANE, (c.id, why, route, inst)


def test_two_block_chain_lane_block_then_lane_step_composes_to_the_whole_scaler():
    """layers 0 .. 2 as a head-less lane block (cl_mlp_forward, MODE 1), layers 3 .. 5 with the head on its activations as a lane full step with
    dZ0_out, cl_chain_dx (dL/d(block activations) = W_3^T dZ_3), then the lane block's backward (cl_mlp_backward_ext, MODE 2): the gradient of
    all six layers against the reference of the whole 6 x 10 scaler"""
    c = RM.case("plain", 0, 10, 9, 6, n=5 * 64 + 37, S=3, img="sorted", tag="whole-lane")
    x, ref = RM.reference_for(c)
    layers, head = RM.unpack(x.mlp, x.d, x.w, x.L)
    flat = lambda ls, h=None: np.concatenate([np.concatenate([W.ravel(), b]) for W, b in ls] + ([h] if h is not None else []))

    def block(cb, mlp, meta_t, **over):
        xb = copy.copy(x)
        xb.case, xb.mlp, xb.meta_t, xb.d, xb.L, xb.head = cb, mlp, meta_t, cb.d, cb.L, cb.head
        xb.P = RM.param_count(cb.d, cb.w, cb.L, cb.head)
        xb.wg_of, xb.wave_of = RM.partition(cb, x.np_, x.grid_eff, x.ntiles)
        xb.wg_rows = [np.flatnonzero(xb.wg_of == g) for g in range(x.grid_eff)]
        for k, v in over.items():
            setattr(xb, k, v)
        return xb

    n = c.n
    c1 = RL.lcase(10, 9, 3, mode=1, n=n)
    r1 = Run(block(c1, flat(layers[:3]), x.meta_t), ref, act_zero=True).launch()
    act = r1.result().act
    f1 = RM.forward(x.X, flat(layers[:3]), 9, 10, 3, False, x.bij_kind, float(x.eps))
    record(c1, {"act_out": RM.RR._worst(np.abs(RM.RW.f64(act)[:10, :n].T - f1.H[-1]), f1.E[-1])}, "lane block, forward")
    assert np.any(act[:10, n:r1.stored_columns()] != 0.0) and np.all(act[10:] == 0.0) and np.all(act[:, r1.stored_columns():] == 0.0)
    # (as it stands it is the next block's metadata: finite behind n_obs in the ragged wave tile, the caller's zeros elsewhere)
    c2 = RL.lcase(10, 10, 3, n=n, S=3, img="sorted", dz0=True)
    x2 = block(c2, flat(layers[3:], head), act)
    P1, P2 = RM.param_count(9, 10, 3, False), RM.param_count(10, 10, 3, True)
    ref2 = copy.copy(ref)
    ref2.M_grad, ref2.grad = ref.M_grad[P1:], ref.grad[P1:]
    ref2.part = [RM.param_grad(x, ref.b, rows) for rows in x2.wg_rows]
    ref2.part = [(v[P1:], M[P1:]) for v, M in ref2.part]
    r2 = Run(x2, ref2).launch()
    got2 = r2.result()
    dz3 = RM.RW.f64(got2.dz0)[:10, :n].T
    record(c2, {"dZ0_out": RM.RR._worst_grad(np.abs(dz3 - ref.b.dZ[3]), ref.b.MZ[3], ref.b.dZ[3])}, "lane step behind the block: dZ0_out")
    # cl_chain_dx: dx_t [meta_rows(10)][n_pad] = W_3^T dZ_3
    g = ref_step.Guarded(DEV).add("dz0", np.where(got2.dz0 == F32(RM.SENT), F32(0), got2.dz0)).add("Wt", np.ascontiguousarray(layers[3][0]))
    g.add("dx", np.full((RM.meta_rows(10), x.n_pad), RM.SENT, F32), True).add("stop", np.zeros(1, np.int32)).build()
    assert int(_lib.get_lib().cl_chain_dx(g.ptr("dz0"), g.ptr("Wt"), n, x.n_pad, 10, 10, g.ptr("dx"), g.ptr("stop"), None)) == 0
    torch.cuda.synchronize()
    g.verify()
    dH = g.get("dx").copy()
    want, Mw = ref.b.dZ[3] @ RM.RW.f64(layers[3][0]), ref.b.MZ[3] @ np.abs(RM.RW.f64(layers[3][0]))
    record(c2, {"cl_chain_dx": RM.RR._worst_grad(np.abs(RM.RW.f64(dH)[:10, :n].T - want), Mw, want)}, "cl_chain_dx")
    assert np.all(dH[:10, n:] == 0.0) and np.all(dH[10:] == 0.0)
    c3 = RL.lcase(10, 9, 3, mode=2, n=n)
    ref1 = copy.copy(ref)
    ref1.M_grad, ref1.grad = ref.M_grad[:P1], ref.grad[:P1]
    got1 = Run(block(c3, flat(layers[:3]), x.meta_t, dH=dH), ref1).launch().result()
    whole = RM.SimpleNamespace(partials=np.concatenate([got1.partials[:x.grid_eff], got2.partials[:x.grid_eff]], axis=1), dz=got2.dz, d_img=got2.d_img, nll=got2.nll)
    assert whole.partials.shape[1] == P1 + P2 == x.P
    xw = copy.copy(x)                                                  # the whole scaler's partials by the lane kernel's workgroups
    xw.wg_rows = x2.wg_rows
    refw = copy.copy(ref)
    refw.part = [RM.param_grad(x, ref.b, rows) for rows in x2.wg_rows]
    record(c, RM.ratios(xw, refw, r2.pre, whole), "lane block + lane step, backward")


def test_report():
    print("largest error / bound on this device:", {f"{k[0]}: {k[1]}": f"{v:.2e}" for k, v in sorted(WORST.items())})
