"""The peeled first layer and the chain step (csrc/elbo_peel.hip: cl_peel_forward, cl_peel_backward, cl_chain_dx) called directly and held to the
fp64 reference of tests/ref_lane.py, every operand in one guarded allocation with a write mask (ref_step.Guarded).

  cl_peel_forward   u_t within gamma(d + 1) sum |W||x| per element over ALL n_pad columns, its padding rows [w, cl_mlp_meta_rows(w)) exact
                    zeros; mlp_peel exact (identity, zero bias, the tail bit for bit); zero_ptr cleared; nothing else written
  cl_peel_backward  layer 0's entries within RTOL_GRAD M + one rounding on top of a preloaded grad_mlp, the tail within one rounding of the sum;
                    nparts = 1 and nparts = cl_peel_parts(n) both inside the bound; a repeat gives the same bits
  cl_chain_dx       an asymmetric Wt (w_out != w_in): within gamma(w_out) sum |W||dz|; zeros behind n_obs and in the padding rows
Shapes: w in {1, 4, 5, 10, 15} x d in {w + 1, 15, 16, 17, 37, 63, 64, 79} (every 16-column block count, the ones column first in a block at
d = 16, 64) with n cycling through {3, 64, 257, 1125}.  One composed step at 20 x 10 on 37 metadata columns -- cl_peel_forward, cl_elbo_mono_fwd_bwd
with dZ0_out on the lane kernel, cl_reduce_partials, cl_peel_backward -- against the reference gradient of the UNPEELED scaler, entry by entry.
Refusals and a raised stop flag on all three calls.
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
from tests.test_lane_kernels_gpu import Run

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda"
F32 = np.float32
SENT = F32(RM.SENT)


def sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                          # a device fault: nothing more is started on the GPU in this session
        pytest.exit(f"{what}: {e}", returncode=3)


def held(what, ratios):
    print(f"{what}: " + " ".join(f"{k} {v:.2e}" for k, v in ratios.items()))
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (what, "error / bound", bad)


def forward(p, stop=0, zero_n=5):
    g = ref_step.Guarded(DEV).add("meta_t", p.meta_t).add("mlp", p.mlp).add("stop", np.array([stop], np.int32))
    g.add("u_t", np.full((RM.meta_rows(p.w), p.n_pad), SENT, F32), True).add("mlp_peel", np.full(p.Pp, SENT, F32), True).add("zero", np.full(zero_n, 2.5, F32), True).build()
    ret = int(_lib.get_lib().cl_peel_forward(g.ptr("meta_t"), p.n, p.n_pad, p.d, p.w, p.L, g.ptr("mlp"), g.ptr("u_t"), g.ptr("mlp_peel"), g.ptr("zero"), zero_n, g.ptr("stop"), None))
    sync(p.id)
    assert ret == 0, (p.id, ret)
    g.verify(untouched=bool(stop))
    return g


def backward(p, nparts, stop=0):
    g = ref_step.Guarded(DEV).add("meta_t", p.meta_t).add("dz0", p.dz0).add("grad_peel", p.grad_peel).add("stop", np.array([stop], np.int32))
    g.add("grad_mlp", p.pre, True).add("partials", np.full((nparts, p.n0), SENT, F32), True).build()
    ret = int(_lib.get_lib().cl_peel_backward(g.ptr("meta_t"), p.n, p.n_pad, p.d, p.w, p.L, g.ptr("dz0"), g.ptr("grad_peel"), g.ptr("grad_mlp"), g.ptr("partials"), nparts,
                                              g.ptr("stop"), None))
    sync(p.id)
    assert ret == 0, (p.id, ret)
    g.verify(untouched=bool(stop))
    return g


@pytest.mark.parametrize("shape", RL.peel_shapes(), ids=lambda s: "{3}x{0}-d{1}-n{2}".format(*s))
def test_peel_forward_and_backward_match_fp64(shape):
    p = RL.peel_problem(*shape)
    assert int(_lib.get_lib().cl_peel_supported(p.d, p.w, p.L)) == 1 == int(RL.peel_supported(p.d, p.w, p.L))
    g = forward(p)
    assert np.all(g.get("zero") == 0.0) and np.all(g.get("u_t") != SENT), p.id
    held(p.id + " forward", RL.peel_forward_ratios(p, g.get("u_t"), g.get("mlp_peel")))
    nmax = int(_lib.get_lib().cl_peel_parts(p.n))
    assert nmax == min(2 * torch.cuda.get_device_properties(0).multi_processor_count, (p.n + 255) // 256)
    for nparts in sorted({1, nmax}):
        gb = backward(p, nparts)
        assert np.all(gb.get("partials") != SENT), p.id
        held(f"{p.id} backward, {nparts} part(s)", RL.peel_backward_ratios(p, gb.get("grad_mlp")))
        assert backward(p, nparts).get("grad_mlp").tobytes() == gb.get("grad_mlp").tobytes(), p.id


def chain(q, stop=0):
    g = ref_step.Guarded(DEV).add("dz", q.dz).add("Wt", q.Wt).add("stop", np.array([stop], np.int32)).add("dx", np.full((RM.meta_rows(q.w_in), q.n_pad), SENT, F32), True).build()
    ret = int(_lib.get_lib().cl_chain_dx(g.ptr("dz"), g.ptr("Wt"), q.n, q.n_pad, q.w_out, q.w_in, g.ptr("dx"), g.ptr("stop"), None))
    sync(q.id)
    assert ret == 0, (q.id, ret)
    g.verify(untouched=bool(stop))
    return g


@pytest.mark.parametrize("shape", RL.CHAIN_SHAPES, ids=lambda s: "{0}to{1}-n{2}".format(*s))
def test_chain_dx_matches_fp64(shape):
    q = RL.chain_problem(*shape)
    held(q.id, RL.chain_ratios(q, chain(q).get("dx")))


def test_a_raised_stop_flag_leaves_everything_as_it_was():
    p = RL.peel_problem(10, 37, 257, 3)
    forward(p, stop=1)
    backward(p, 1, stop=1)
    chain(RL.chain_problem(10, 7, 257), stop=1)


def test_refusals_launch_nothing():
    lib, p = _lib.get_lib(), RL.peel_problem(10, 37, 64, 2)
    for d, w, L in ((10, 10, 2), (9, 10, 2), (80, 10, 2), (79, 15, 1), (79, 16, 1), (17, 0, 2), (37, 10, 0), (79, 1, 20)):
        assert int(lib.cl_peel_supported(d, w, L)) == int(RL.peel_supported(d, w, L)), (d, w, L)
    g = ref_step.Guarded(DEV).add("meta_t", p.meta_t).add("mlp", p.mlp).add("dz0", p.dz0).add("grad_peel", p.grad_peel).add("u_t", np.full((12, p.n_pad), SENT, F32))
    g.add("mlp_peel", np.full(p.Pp, SENT, F32)).add("grad_mlp", p.pre).add("partials", np.full((2, p.n0), SENT, F32)).add("stop", np.zeros(1, np.int32)).build()
    P = g.ptr
    fwd = lambda d, w, n=p.n, n_pad=p.n_pad, zero_n=0: int(lib.cl_peel_forward(P("meta_t"), n, n_pad, d, w, 2, P("mlp"), P("u_t"), P("mlp_peel"), None, zero_n, P("stop"), None))
    bwd = lambda d, w, nparts=1, n=p.n, n_pad=p.n_pad: int(lib.cl_peel_backward(P("meta_t"), n, n_pad, d, w, 2, P("dz0"), P("grad_peel"), P("grad_mlp"), P("partials"), nparts, P("stop"), None))
    assert fwd(10, 10) == -2 and fwd(80, 10) == -2 and fwd(37, 16) == -2 and fwd(37, 10, n=0) == -1 and fwd(37, 10, n=p.n_pad + 1) == -1 and fwd(37, 10, zero_n=3) == -1
    assert bwd(10, 10) == -2 and bwd(80, 10) == -2 and bwd(37, 10, nparts=0) == -1 and bwd(37, 10, nparts=2) == -1 and bwd(37, 10, n=0) == -1
    assert int(lib.cl_peel_backward(P("meta_t"), 60, 96, 37, 10, 2, P("dz0"), P("grad_peel"), P("grad_mlp"), P("partials"), 1, P("stop"), None)) == -1      # n_pad no multiple of 64
    cdx = lambda wo, wi, n=p.n: int(lib.cl_chain_dx(P("dz0"), P("mlp"), n, p.n_pad, wo, wi, P("u_t"), P("stop"), None))
    assert cdx(16, 10) == -2 and cdx(10, 16) == -2 and cdx(0, 10) == -2 and cdx(10, 7, n=0) == -1 and cdx(10, 7, n=p.n_pad + 1) == -1
    assert int(lib.cl_chain_dx(None, P("mlp"), p.n, p.n_pad, 10, 7, P("u_t"), P("stop"), None)) == -1
    sync("refusals")
    g.verify(untouched=True)


def test_one_composed_step_is_the_gradient_of_the_unpeeled_scaler():
    """20 x 10 on 37 metadata columns"""
    w, d, L, n = 10, 37, 20, 5 * 64 + 37
    c = RM.case("plain", 0, w, d, L, n=n, S=3, img="sorted", tag="peeled")
    x, ref = RM.reference_for(c)
    assert ref.near == 0
    p = RM.SimpleNamespace(w=w, d=d, L=L, n=n, n_pad=x.n_pad, mlp=x.mlp, meta_t=x.meta_t, Pp=RM.param_count(w, w, L), id=c.id)
    gf = forward(p, zero_n=0)
    u_t, mlp_peel = gf.get("u_t").copy(), gf.get("mlp_peel").copy()
    c2 = RL.lcase(w, w, L, n=n, S=3, img="sorted", dz0=True)
    x2 = copy.copy(x)
    x2.case, x2.mlp, x2.meta_t, x2.d, x2.P = c2, mlp_peel, u_t, w, p.Pp
    x2.wg_of, x2.wave_of = RM.partition(c2, x.np_, x.grid_eff, x.ntiles)
    x2.wg_rows = [np.flatnonzero(x2.wg_of == g) for g in range(x.grid_eff)]
    n0, t0 = w * d + w, w * w + w
    ref2 = copy.copy(ref)                                              # (for the preloads: the summand sizes of the peeled scaler's gradient; its layer 0 is not compared)
    ref2.M_grad, ref2.grad = np.concatenate([np.ones(t0), ref.M_grad[n0:]]), np.concatenate([np.zeros(t0), ref.grad[n0:]])
    run = Run(x2, ref2).launch()
    got = run.result()
    dz0 = np.where(got.dz0 == SENT, F32(0), got.dz0)                   # the caller's cleared buffer with the launch's stores in it
    held("the step behind the peeled layer: dZ0_out", {"dZ0_out": RM.RR._worst_grad(np.abs(RM.RW.f64(dz0)[:w, :n].T - ref.b.dZ[0]), ref.b.MZ[0], ref.b.dZ[0])})
    pre = RM.preloads(x, ref).grad
    pb = RM.SimpleNamespace(w=w, d=d, L=L, n=n, n_pad=x.n_pad, meta_t=x.meta_t, dz0=dz0, grad_peel=got.grad, pre=pre, n0=n0, id=c.id)
    grad = backward(pb, 1).get("grad_mlp")
    stored = RM.RW.f64(pre) + ref.grad
    err = np.abs(RM.RW.f64(grad) - stored)
    err[n0:] = np.abs(RM.RW.f64(grad[n0:]) - (stored[n0:] + RM.RW.f64(run.pre.grad[t0:])))      # (the launch's own preload rides along in grad_peel: one more stored value, one more rounding)
    extra = np.concatenate([np.zeros(n0), RL.U * np.abs(RM.RW.f64(got.grad[t0:]))])
    held("composed step, every entry", {"grad": RM.RR._worst(np.maximum(err - RL.U * np.abs(stored) - extra, 0.0), RM.RTOL_GRAD * ref.M_grad)})
    for name, s in RM.tensor_slices(x):
        tot = RM.RW.f64(grad[s]) - RM.RW.f64(pre[s]) - (RM.RW.f64(run.pre.grad[t0:])[s.start - n0:s.stop - n0] if s.start >= n0 else 0.0)
        assert np.max(np.abs(tot - ref.grad[s])) <= RM.RTOL_GRAD * np.max(np.abs(ref.grad[s])) + 2 * RL.U * np.max(np.abs(stored[s])), name
