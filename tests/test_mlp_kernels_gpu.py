"""Every instance of the fused scaler + likelihood kernel (csrc/elbo_mlp.hip) outside the per-image-layer unit, called directly through the C ABI
(cl_elbo_mono_fwd_bwd, cl_mlp_forward, cl_mlp_backward_ext; cl_reduce_partials and cl_det_reduce behind them) and held, launch by launch and
element by element, to the ONE fp64 reference of tests/ref_mlp.py.

The case list is generated (ref_mlp.cases): one case per instance -- unit (plain, chain, packed, deterministic, packed deterministic, chain
deterministic) x width form (WP 16 with KS 2 / 3 / 4 / 5, WP 32 with LMAX 5 / 10, WP 64) x metadata capacity (DP 8 / 32 / 64) x mode x epilogue
(generic, its Laplace instance, and on the 64-wide plain unit the two plain epilogues) -- at n = 5 * 128 + 37 rows on two workgroups (three
tiles each, the last ragged); per (unit, width form) n = 3, n = 128, one workgroup and a grid larger than the tile count (the launch clamps
it: the rows of `partials` behind n_pad / 128 keep their bits); per (unit, width form) on the generic epilogue the options -- MC samples
1 .. 12 with likelihoods, bijectors, image scales (borders inside a wave's 16 rows, unsorted, none), injected / in-kernel noise at a non-zero
obs_offset and ipred_out cycling; d_ev11 / ev11_part; det_slot on the deterministic units; noise_row on the packed ones, with and without
harmonic groups of 1 .. 16 rows; a raised stop flag -- and on the two plain epilogues what keeps a launch on them.  act_out and dX_out are
stored for observations below n_obs only (include/careless_hip.h): the columns behind keep their bytes, the caller clears them.
Every case asserts cl_mlp_check == 0 in front of the launch and that
cl_mlp_route / cl_mlp_kernel_name / cl_mlp_epilogue name the instance the restated rules give for its arguments (ref_mlp.expected_instance).  tests/test_ref_mlp.py holds the list to the
enumerated set of instances, the reference to the oracle and the bounds to an fp32 emulation, without a GPU.

Every operand comes from one guarded allocation (ref_step.Guarded) with a mask of what the header lets the call write, verified after every
call; workspaces have exactly the documented size (partials [grid][P], nll_part [grid], ev11_part [3 * CL_EV11_WAVES * grid]); outputs a call
stores are preloaded with a sentinel and must all be written, outputs it adds to with a tenth of their summand size.

Bounds (tests/ref_mlp.py; no tolerance of this file's own): loc_out / sig_out / act_out within the derived rounding bound, ipred_out within
RTOL_LOSS M, the NLL within RTOL_LOSS max(M, 1), every gradient entry and deterministic record within RTOL_GRAD M + one rounding of the stored
value, every gradient tensor within RTOL_GRAD of its max-norm.  The largest ratios met on an MI355X are in DESIGN section 2.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from careless_amd import _lib
from tests import ref_mlp as RM
from tests import ref_step

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda"
F32 = np.float32
WORST = {}
ENTRY = ("cl_elbo_mono_fwd_bwd", "cl_mlp_forward", "cl_mlp_backward_ext")
ROUTE = {"plain": _lib.CL_ROUTE_MLP, "chain": _lib.CL_ROUTE_MLP_CHAIN, "packed": _lib.CL_ROUTE_MLP_PACKED, "det": _lib.CL_ROUTE_MLP_DET,
         "packed_det": _lib.CL_ROUTE_MLP_PACKED_DET, "chain_det": _lib.CL_ROUTE_MLP_CHAIN_DET}


def record(c, ratios, what=None):
    for k, v in ratios.items():
        key = (c.unit + (" plain epilogue" if getattr(c, "instance", "").find(" plain ") > 0 else ""), k)
        WORST[key] = max(WORST.get(key, 0.0), v)
    print(f"{what or c.id}: " + " ".join(f"{k} {v:.2e}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (what or c.id, "error / bound", bad)


def dump_noise(S, n, offset):
    out = torch.empty(n * S, dtype=torch.float32, device=DEV)
    assert int(_lib.get_lib().cl_debug_noise(RM.SEED, RM.STEP, S, n, offset, 1, out.data_ptr(), None)) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(n, S)


def inputs_of(c):
    """(inputs, reference): the shared ones, or -- in-kernel noise -- the case's inputs with cl_debug_noise(kind = 1) as its normals"""
    x, ref = RM.reference_for(c)
    if c.mode != 0 or c.noise == "eta":
        return x, ref
    x = copy.copy(x)
    if x.noise_row is not None:                                        # keys all over a range behind obs_offset: the row of every position
        dump = dump_noise(x.S, x.np_ + 17, x.obs_offset)
        x.eta = np.zeros((x.n, x.S), F32)
        x.eta[x.krow[x.act]] = dump[x.noise_row[x.act] - x.obs_offset]
    else:
        x.eta = dump_noise(x.S, x.n, x.obs_offset)
    assert np.all(np.isfinite(x.eta)) and (x.n * x.S < 50 or 0.5 < x.eta.std() < 1.5)
    RM.finish_likelihood(x)
    return x, RM.reference(x)


class Run:
    """the operands of one case in a guarded allocation and the cl_mlp_args that point at them.  (The hooks -- stored_columns, ev11_waves,
    more_operands, more_args, check_instance -- are what tests/test_lane_kernels_gpu.py replaces for the lane and narrow kernels.)"""

    def stored_columns(self):
        """columns of act_out / dX_out the launch may store: the observations below n_obs"""
        return self.x.np_

    def act_mask(self, live):
        """elements of act_out the launch may store: every row of the padded feature block (the padding rows: zeros) in the stored columns"""
        return np.broadcast_to(live, (RM.meta_rows(self.x.w), self.x.n_pad))

    def check_act(self, act):
        """data rows written, padding rows exactly zero, columns behind n_obs left alone (the mask)"""
        x = self.x
        assert np.all(act[:x.w, :x.np_] != F32(RM.SENT)) and np.all(act[x.w:, :x.np_] == 0.0), self.c.id

    EV11_FILL = 0.0                                                    # what the wave slots the kernel never stores hold: the caller's zeros (cl_det_reduce adds them)

    def ev11_waves(self):
        """wave slots of a workgroup's CL_EV11_WAVES in ev11_part that the kernel stores"""
        return RM.EV11_WAVES

    def more_operands(self, g):
        pass

    def more_args(self, A, opt):
        pass

    def check_instance(self, route, inst):
        c = self.c
        assert route == ROUTE[c.unit] and inst == RM.expected_instance(c) == getattr(c, "instance", inst), (c.id, route, inst, RM.expected_instance(c))

    def __init__(self, x, ref, stop=False, act_zero=False):
        c = x.case
        self.x, self.ref, self.c = x, ref, c
        self.pre = pre = RM.preloads(x, ref) if c.mode != 1 else None
        n, S, grid, P = x.n, x.S, c.grid, x.P
        live = np.zeros(x.n_pad, bool)
        live[:self.stored_columns()] = True
        g = ref_step.Guarded(DEV).add("meta_t", x.meta_t).add("mlp", x.mlp).add("stop", np.array([1 if stop else 0], np.int32))
        part_mask = np.zeros((grid, P), bool)
        part_mask[:x.grid_eff] = True                                  # the launch clamps the grid: the rows behind n_pad / 128 keep their bits
        if c.mode == 0:
            rid = np.full(x.n_obs, -1, np.int32)
            rid[:x.np_] = x.refl_id
            g.add("refl_id", rid).add("iobs", x.iobs).add("sig", x.sig).add("z_f", x.z_f).add("eta", x.eta)
            has_rows = np.bincount(x.refl_id[x.act], minlength=x.R) > 0
            g.add("dz_f", pre.dz, np.repeat(has_rows[:, None], S, axis=1))
            g.add("scalars", np.array([pre.nll, 1.25, 7.0, 6.0]), [True, False, False, False])
            if x.img is not None:
                present = np.zeros(len(x.img), bool)
                ids = np.unique(x.image_id[x.act])
                present[ids[ids > 0] - 1] = True
                g.add("image_id", x.image_id).add("img", x.img).add("d_img", pre.d_img, present)
            if c.ipred:
                g.add("ipred", np.full((n, S), RM.SENT, F32), True)
            if c.ev11:
                g.add("ev11", x.ev11).add("d_ev11", pre.d_ev11, True)
                if c.det:
                    m = np.zeros((grid, 3 * RM.EV11_WAVES), bool)
                    m[:x.grid_eff, :3 * self.ev11_waves()] = True
                    g.add("ev11_part", np.where(m | (np.arange(grid) >= x.grid_eff)[:, None], F32(RM.SENT), F32(self.EV11_FILL)), m)      # (slots the kernel has no wave for: the caller's zeros)
                    self.ev11_mask = m
            if c.det:
                g.add("dzf_obs", np.full((n, S), RM.SENT, F32), True).add("nll_part", np.full(grid, -7.5e300), np.arange(grid) < x.grid_eff)
                if x.img is not None:
                    g.add("dimg_obs", np.full(n, RM.SENT, F32), True)
                if x.det_slot is not None:
                    g.add("det_slot", x.det_slot)
        if c.mode == 1:
            if c.head:
                g.add("loc_out", np.full(n, RM.SENT, F32), True).add("sig_out", np.full(n, RM.SENT, F32), True)
            else:
                g.add("act_out", np.full((RM.meta_rows(x.w), x.n_pad), 0.0 if act_zero else RM.SENT, F32), self.act_mask(live))
        if c.mode == 2:
            g.add("dO_ext", x.dO) if c.head else g.add("dH_ext", x.dH)
        if c.mode != 1:
            g.add("partials", np.full((grid, P), RM.SENT, F32), part_mask).add("grad", pre.grad, True)
        if c.dX:
            g.add("dX_out", np.full((RM.meta_rows(x.d), x.n_pad), RM.SENT, F32), np.broadcast_to(live, (RM.meta_rows(x.d), x.n_pad)))
        if c.packed:
            g.add("row_map", x.row_map)
            if c.groups:
                g.add("gmeta", x.gmeta).add("tile_gmax", x.tile_gmax)
        if x.case.noise_row:
            g.add("noise_row", x.noise_row)
        self.more_operands(g)
        self.g = g.build()
        A = _lib.MlpArgs()
        A.meta_t, A.mlp, A.stop_flag = g.ptr("meta_t"), g.ptr("mlp"), g.ptr("stop")
        A.n_obs, A.n_pad, A.obs_offset, A.d, A.w, A.L, A.leak = x.n_obs, x.n_pad, x.obs_offset, x.d, x.w, x.L, RM.LEAK
        A.bij_kind, A.eps, A.shift = int(x.bij_kind), float(x.eps), float(x.shift)
        A.S, A.lik_kind, A.dof, A.lik_const, A.w_ll = S, RM.RR.KINDS[x.kind], float(x.dof), float(x.lik_const), float(x.w_ll)
        opt = lambda k: g.ptr(k if k in g.ops else None)
        if c.mode == 0:
            A.refl_id, A.iobs, A.sig, A.z_f, A.R = g.ptr("refl_id"), g.ptr("iobs"), g.ptr("sig"), g.ptr("z_f"), x.R
            A.dz_f, A.scalars = g.ptr("dz_f"), g.ptr("scalars")
            A.use_img, A.image_id, A.img, A.d_img = int(x.img is not None), opt("image_id"), opt("img"), opt("d_img")
            A.eta, A.seed, A.step = (g.ptr("eta"), 0, 0) if c.noise == "eta" else (None, RM.SEED, RM.STEP)
            A.ipred_out, A.ev11 = opt("ipred"), opt("ev11")
            A.d_ev11, A.ev11_part = (None, opt("ev11_part")) if c.det else (opt("d_ev11"), None)
            A.dzf_obs, A.dimg_obs, A.nll_part, A.det_slot = opt("dzf_obs"), opt("dimg_obs"), opt("nll_part"), opt("det_slot")
        A.loc_out, A.sig_out, A.act_out, A.dO_ext, A.dH_ext, A.dX_out = (opt(k) for k in ("loc_out", "sig_out", "act_out", "dO_ext", "dH_ext", "dX_out"))
        A.partials, A.row_map, A.gmeta, A.tile_gmax, A.noise_row = (opt(k) for k in ("partials", "row_map", "gmeta", "tile_gmax", "noise_row"))
        self.more_args(A, opt)
        self.A = A

    def instance(self):
        lib, buf = _lib.get_lib(), C.create_string_buffer(256)
        lib.cl_mlp_kernel_name(C.byref(self.A), self.c.mode, buf, 256)
        route, epi = int(lib.cl_mlp_route(C.byref(self.A), self.c.mode)), int(lib.cl_mlp_epilogue(C.byref(self.A), self.c.mode))
        return route, RM.instance_name(buf.value.decode(), epi, self.c)

    def launch(self, untouched=False):
        lib, c = _lib.get_lib(), self.c
        route, inst = self.instance()
        self.check_instance(route, inst)
        assert int(lib.cl_mlp_check(C.byref(self.A), c.mode, c.grid)) == 0, c.id
        ret = int(getattr(lib, ENTRY[c.mode])(C.byref(self.A), c.grid, None))
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:                                      # a device fault: nothing more is started on the GPU in this session
            pytest.exit(f"{c.id}: {e}", returncode=3)
        if ret > 0:
            pytest.exit(f"{c.id}: HIP error {ret} from the launch", returncode=3)
        assert ret == 0, (c.id, ret)
        if c.mode != 1 and not untouched:                              # the fixed-order sum of the workgroups' partials, on top of the preload
            assert int(lib.cl_reduce_partials(self.g.ptr("partials"), self.x.grid_eff, self.x.P, self.g.ptr("grad"), self.g.ptr("stop"), None)) == 0
            torch.cuda.synchronize()
        self.g.verify(untouched=untouched)
        return self

    def result(self):
        g, x, c = self.g, self.x, self.c
        get = lambda k: g.get(k).copy() if k in g.ops else None
        out = RM.SimpleNamespace(loc=get("loc_out"), sig=get("sig_out"), act=get("act_out"), ipred=get("ipred"), partials=get("partials"), grad=get("grad"),
                                 dX=get("dX_out"), dzf_obs=get("dzf_obs"), dimg_obs=get("dimg_obs"), nll_part=get("nll_part"), ev11_part=get("ev11_part"))
        sent = F32(RM.SENT)
        for k in ("loc", "sig", "ipred", "dzf_obs", "dimg_obs"):       # every element of a stored output was written
            assert getattr(out, k) is None or np.all(getattr(out, k) != sent), (c.id, k)
        if out.partials is not None:
            assert np.all(out.partials[:x.grid_eff] != sent), c.id
        if out.act is not None:
            self.check_act(out.act)
        if out.dX is not None:
            assert np.all(out.dX[:x.d, :x.np_] != sent) and np.all(out.dX[x.d:, :x.np_] == 0.0), c.id
        if out.ev11_part is not None:
            assert np.all(out.ev11_part[self.ev11_mask] != sent), c.id
            out.ev11_part = out.ev11_part[:x.grid_eff].ravel()
        if c.mode == 0 and not c.det:
            out.dz, out.d_img, out.d_ev11 = get("dz_f"), get("d_img"), get("d_ev11")
            out.nll = float(g.get("scalars")[0]) - self.pre.nll
        return out

    def det_reduce(self):
        """cl_det_reduce over the records: dz_f, d_img, the NLL and d_ev11 as the atomic units leave them"""
        g, x, c = self.g, self.x, self.c
        rid_rows, img_rows = np.zeros(x.n, np.int64), np.zeros(x.n, np.int64)
        rid_rows[x.krow[x.act]] = x.refl_id[x.act]
        D = _lib.DetArgs()
        extra = ref_step.Guarded(DEV)
        extra.add("seg_refl", np.concatenate([[0], np.cumsum(np.bincount(rid_rows, minlength=x.R))]).astype(np.int32))
        extra.add("perm_refl", np.argsort(rid_rows, kind="stable").astype(np.int32))
        if x.img is not None:
            img_rows[x.krow[x.act]] = x.image_id[x.act]
            extra.add("seg_img", np.concatenate([[0], np.cumsum(np.bincount(img_rows, minlength=x.n_images))]).astype(np.int32))
            extra.add("perm_img", np.argsort(img_rows, kind="stable").astype(np.int32))
        extra.build()
        D.dzf_obs, D.perm_refl, D.seg_refl, D.R, D.S, D.dz_f = g.ptr("dzf_obs"), None if x.det_slot is not None else extra.ptr("perm_refl"), extra.ptr("seg_refl"), x.R, x.S, g.ptr("dz_f")
        if x.img is not None:
            D.dimg_obs, D.perm_img, D.seg_img, D.n_images, D.d_img = g.ptr("dimg_obs"), extra.ptr("perm_img"), extra.ptr("seg_img"), x.n_images, g.ptr("d_img")
        D.nll_part, D.nparts, D.scalars, D.stop_flag = g.ptr("nll_part"), x.grid_eff, g.ptr("scalars"), g.ptr("stop")
        if c.ev11:
            D.ev11_part, D.n_ev11, D.d_ev11 = g.ptr("ev11_part"), RM.EV11_WAVES * x.grid_eff, g.ptr("d_ev11")
        assert int(_lib.get_lib().cl_det_reduce(C.byref(D), None)) == 0
        torch.cuda.synchronize()
        g.verify()
        extra.verify(untouched=True)
        get = lambda k: g.get(k).copy() if k in g.ops else None
        return RM.SimpleNamespace(dz=get("dz_f"), d_img=get("d_img"), d_ev11=get("d_ev11"), nll=float(g.get("scalars")[0]) - self.pre.nll)


SAME = ("partials", "grad", "dX", "dzf_obs", "dimg_obs", "nll_part", "ev11_part")


@pytest.mark.parametrize("c", RM.cases(), ids=lambda c: c.id)
def test_launch_matches_fp64(c):
    x, ref = inputs_of(c)
    run = Run(x, ref).launch()
    got = run.result()
    record(c, RM.ratios(x, ref, run.pre, got))
    if c.det:
        # the launch itself adds nowhere; no atomic, so a second run gives the same bits; the reduced sums hold the atomic units' bounds
        assert not any(run.g.changed(k).any() for k in ("dz_f", "d_img", "scalars", "d_ev11") if k in run.g.ops), c.id
        again = Run(x, ref).launch().result()
        assert all(getattr(got, k) is None or getattr(got, k).tobytes() == getattr(again, k).tobytes() for k in SAME), c.id
        record(c, RM.ratios(x, ref, run.pre, run.det_reduce()), c.id + " + cl_det_reduce")


STOP_CASES = RM.stop_cases()


@pytest.mark.parametrize("c", STOP_CASES, ids=lambda c: c.id)
def test_a_raised_stop_flag_leaves_every_output_and_workspace_as_it_was(c):
    x, ref = RM.reference_for(c)
    Run(x, ref, stop=True).launch(untouched=True)


def test_two_block_chain_composed_by_hand_is_the_whole_scaler():
    """layers 0 .. 2 as a head-less block (cl_mlp_forward with act_out), layers 3 .. 5 with the head on its activations (cl_mlp_forward;
    cl_elbo_mono_fwd_bwd with dX_out), then the first block's cl_mlp_backward_ext from dH_ext = that dX_out: loc / sigma and the gradient of all
    six layers against the reference of the 6 x 17 scaler"""
    c = RM.case("plain", 0, 17, 9, 6, S=3, img="sorted", tag="whole")
    x, ref = RM.reference_for(c)
    layers, head = RM.unpack(x.mlp, x.d, x.w, x.L)
    flat = lambda ls, h=None: np.concatenate([np.concatenate([W.ravel(), b]) for W, b in ls] + ([h] if h is not None else []))

    def block(cb, mlp, meta_t, **over):
        xb = copy.copy(x)
        xb.case, xb.mlp, xb.meta_t, xb.d, xb.L, xb.head = cb, mlp, meta_t, cb.d, cb.L, cb.head
        xb.P = RM.param_count(cb.d, cb.w, cb.L, cb.head)
        for k, v in over.items():
            setattr(xb, k, v)
        return xb

    c1 = RM.case("chain", 1, 17, 9, 3, head=False)
    r1 = Run(block(c1, flat(layers[:3]), x.meta_t), ref, act_zero=True).launch()
    act = r1.result().act                                              # [cl_mlp_meta_rows(17)][n_pad], rows behind n_obs zero: the next block's metadata
    c2f = RM.case("plain", 1, 17, 17, 3)
    fwd = Run(block(c2f, flat(layers[3:], head), act), ref).launch().result()
    record(c, RM.ratios(x, ref, None, RM.SimpleNamespace(loc=fwd.loc, sig=fwd.sig)), "two blocks, forward")
    c2 = RM.case("chain", 0, 17, 17, 3, S=3, img="sorted", dX=True)
    P1, P2 = RM.param_count(9, 17, 3, False), RM.param_count(17, 17, 3, True)
    ref2 = copy.copy(ref)
    ref2.M_grad, ref2.grad = ref.M_grad[P1:], ref.grad[P1:]
    r2 = Run(block(c2, flat(layers[3:], head), act), ref2).launch()
    got2 = r2.result()
    c3 = RM.case("chain", 2, 17, 9, 3, head=False)
    ref1 = copy.copy(ref)
    ref1.M_grad, ref1.grad = ref.M_grad[:P1], ref.grad[:P1]
    dH = got2.dX.copy()
    dH[:, x.n:] = 0.0
    got1 = Run(block(c3, flat(layers[:3]), x.meta_t, dH=dH), ref1).launch().result()
    whole = RM.SimpleNamespace(partials=np.concatenate([got1.partials[:x.grid_eff], got2.partials[:x.grid_eff]], axis=1), dz=got2.dz, d_img=got2.d_img, nll=got2.nll)
    assert whole.partials.shape[1] == P1 + P2 == x.P
    record(c, RM.ratios(x, ref, r2.pre, whole), "two blocks, backward")


def test_report():
    tot = {}
    for (unit, k), v in WORST.items():
        tot[k] = max(tot.get(k, 0.0), v)
    print("largest error / bound on this device, all units:", {k: f"{v:.2e}" for k, v in sorted(tot.items())})
    print("largest error / bound on this device:", {f"{k[0]}: {k[1]}": f"{v:.2e}" for k, v in sorted(WORST.items())})
