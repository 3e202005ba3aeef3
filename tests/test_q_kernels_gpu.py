"""The posterior and prior half of the step on the GPU: `cl_tn_forward`, `cl_dw_prior_forward`, `cl_tn_backward` and `cl_reduce_partials`
called directly through the C ABI the engine calls, on injected uniforms, against the fp64 reference of tests/ref_q.py (the oracle's
O.tn_* / O.wilson_log_prob / O.double_wilson_log_prob under autograd) -- at R up to 1100 (five workgroups of reflections), S in
{1, 3, 4, 5, 8, 9} (the Philox block is shared by four samples), with and without kl_part, an inner KL range, an owned range whose r_begin
is no multiple of 256, under the three prior kinds, fixed and trainable r, the atomic and the child-list form.

Every operand is carved from one guarded allocation (ref_step.Guarded: 256 guard bytes around each, a mask of what the contract lets a call
write) that is verified after every call; outputs are preloaded (a sentinel where a call stores, values or exact zeros where it adds).

Bounds (tests/ref_q.py: `ratios`; all tolerances are the project's): z_f within 1e-5 (loc + scale) per element; the KL within RTOL_LOSS
max(|KL|, 1); every entry of d_loc_raw / d_scale_raw / d_dw_r_raw and every dz_f element after the parents' scatter within RTOL_GRAD M + one
fp32 rounding of the stored sum, M the entry's summand size; on the wide family also RTOL_GRAD of the max-norm; entries outside the owned
range bit-unchanged.  The cases, their inputs and what the fp32 emulation reaches on them: tests/ref_q.py, tests/test_ref_q.py.

Measured on an MI355X, the largest ratio to the bound over all cases (in brackets: the fp32 emulation on the host build, glibc's
expf / erfcf / log1pf, on the same inputs):
    z_f                           wide 0.085 [0.10]      tiny scale 0.013 [0.012]     double Wilson 0.063 [0.071]
    KL                            wide 1.8e-3 [1.7e-3]   tiny scale 4.9e-4 [7e-5]     double Wilson 5.1e-3 [5.7e-3]    reference prior 1.3e-3 [5.7e-4]
    d_loc_raw, per entry          wide 0.13 [0.19]       tiny scale 4.9e-4 [4.8e-4]   double Wilson 0.056 [0.13]       reference prior 2.5e-3 [1.9e-3]
    d_scale_raw, per entry        wide 0.070 [0.070]     tiny scale 6.5e-4 [7.5e-4]   double Wilson 0.089 [0.17]       reference prior 2.5e-3 [2.4e-3]
    dz_f after the scatter        double Wilson 0.29 [0.13]        d_dw_r_raw 4.4e-3 [5.6e-3]
    max-norm, wide family         d_loc_raw 0.14 [0.12]  d_scale_raw 0.015 [0.009]    (mostly the store's rounding on top of the preloaded value)
    on the uniforms the kernels draw themselves (R = 1100, S = 3, owned range): d_loc_raw 0.36, everything else below 0.08
    reduction: 0 on the dyadic inputs (the bound set for it), 0.49 of the a-priori fp32 bound on floats; the two routes bit for bit
The device's transcendental functions sit where glibc's do: nothing is outside a bound, and nothing within a factor 2.5 of one.
"""
import copy
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from careless_amd import _lib
from tests import ref_q as Q
from tests import ref_step

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda"
F32 = np.float32
ZERO_NS = (36, 37, 4)                 # zero_n: a multiple of four, one float over, a lone f32x4
WORST = {}                            # (family / prior, quantity) -> largest ratio to its bound this session (printed, not a gate)
SEED, STEP = 20260, 7


class Run:
    """The operands of one case in a guarded allocation and the argument block that points at them."""

    def __init__(self, x, stop=False, seeded=False, red=None, fields=None):
        R, S, part = x.R, x.S, x.part
        self.x, self.dw, self.ref_kind = x, x.prior == "dw", x.prior == "reference"
        own2 = np.repeat(x.own[:, None], S, axis=1)
        self.zero_n = ZERO_NS[(R + S) % 3]
        g = ref_step.Guarded(DEV).add("a", x.a).add("b", x.b).add("low", x.low).add("centric", x.centric).add("es", x.es).add("u", x.u)
        g.add("z_f", np.full((R, S), Q.SENT, F32), own2)
        scat = np.zeros(R, bool)
        if self.dw:
            act = x.in_kl & (x.root == 0) & (x.par >= 0)
            scat[x.par[act]] = True
        g.add("dz", x.dz, np.repeat(scat[:, None], S, axis=1))
        g.add("dz_zero", np.full((R, S), 2.5, F32), own2 if part else False)
        g.add("d_a", x.pre[0], x.own).add("d_b", x.pre[1], x.own)
        g.add("kl_part", np.full(x.nb + 3, Q.SENT), ([True] * x.nb + [False] * 3) if part else False)
        if self.ref_kind:
            g.add("kl_part_dw", x.kl_part_dw_pre)
        else:
            g.add("kl_part_dw", np.full(x.nblk + 2, Q.SENT), ([True] * x.nblk + [False] * 2) if (part and self.dw) else False)
        g.add("zero", np.full(self.zero_n + 1, 5.5, F32), ([True] * self.zero_n + [False]) if part else False)
        g.add("scalars", np.array([1.25, x.kl_before, 7.0, 6.0]), [False, True, False, False])
        g.add("stop", np.array([1 if stop else 0], np.int32))
        if self.dw:
            g.add("par", x.par).add("root", x.root).add("dw_r", x.dw_r).add("r_raw", x.r_raw).add("asu", x.asu)
            g.add("d_r", x.pre_r, [False, True, True] if x.trainable else False)      # (the root ASU has no child)
            g.add("child_seg", x.child_seg).add("child_ids", x.child_ids)
        if red is not None:
            parts, pre = red
            g.add("red_parts", parts).add("red_out", pre, True).add("red_out2", pre, True)
        self.g = g.build()
        A = _lib.TnArgs()
        A.q_loc_raw, A.q_scale_raw, A.low = g.ptr("a"), g.ptr("b"), g.ptr("low")
        A.centric, A.es = (None, None) if self.ref_kind else (g.ptr("centric"), g.ptr("es"))
        A.R, A.S, A.high, A.eps, A.w_kl, A.kl_grad_mult = R, S, Q.HIGH, Q.EPS, float(x.w_kl), x.mult
        A.kl_begin, A.kl_end, A.r_begin, A.r_end = x.k0, x.k1, x.r0, x.r1
        A.u_f, A.seed, A.step = (None, SEED, STEP) if seeded else (g.ptr("u"), 0, 0)
        A.z_f, A.dz_f, A.d_loc_raw, A.d_scale_raw = g.ptr("z_f"), g.ptr("dz"), g.ptr("d_a"), g.ptr("d_b")
        A.scalars, A.stop_flag = g.ptr("scalars"), g.ptr("stop")
        if part:
            A.kl_part, A.kl_part_dw = g.ptr("kl_part"), g.ptr("kl_part_dw")
            A.zero_ptr, A.zero_n, A.zero_dzf = g.ptr("zero"), self.zero_n, g.ptr("dz_zero")
        A.prior_kind = {"wilson": _lib.CL_PRIOR_WILSON, "reference": _lib.CL_PRIOR_REFERENCE, "dw": _lib.CL_PRIOR_DOUBLE_WILSON}[x.prior]
        if self.dw:
            A.parent_ids, A.root, A.dz_f_out = g.ptr("par"), g.ptr("root"), g.ptr("dz")
            if x.trainable:
                A.dw_r_raw, A.asu_ids, A.d_dw_r_raw, A.n_asu = g.ptr("r_raw"), g.ptr("asu"), g.ptr("d_r"), 3
            else:
                A.dw_r = g.ptr("dw_r")
            if x.child_list:
                A.dw_child_seg, A.dw_child_ids = g.ptr("child_seg"), g.ptr("child_ids")
        if red is not None:
            A.red_partials, A.red_nparts, A.red_P, A.red_out = g.ptr("red_parts"), red[0].shape[0], red[0].shape[1], g.ptr("red_out")
        for k, v in (fields or {}).items():
            setattr(A, k, v)
        self.A = A

    def call(self, name, expect=0, untouched=False):
        ret = int(getattr(_lib.get_lib(), name)(C.byref(self.A), None))
        torch.cuda.synchronize()
        assert ret == expect, (self.x.case.id, name, ret, expect)
        self.g.verify(untouched=untouched)           # guards, inputs, rows outside the owned range, unused slots: bit-identical; refused / stopped: everything
        return self

    def sequence(self, untouched=False):
        self.call("cl_tn_forward", untouched=untouched)
        if self.dw:
            self.call("cl_dw_prior_forward", untouched=untouched)
        return self.call("cl_tn_backward", untouched=untouched)

    def result(self):
        g, x = self.g, self.x
        return SimpleNamespace(z=g.get("z_f").copy(), kl=float(g.get("scalars")[_lib.CL_SC_KL]) - x.kl_before, d=[g.get("d_a").copy(), g.get("d_b").copy()],
                                 dz=g.get("dz").copy(), d_r=g.get("d_r").copy() if self.dw else None, scalars=g.get("scalars").copy())


def check(run, ref, what=None):
    """the stores of the case's modes, then every bound"""
    g, x = run.g, run.x
    got = run.result()
    what = what or x.case.id
    assert np.all(got.z[~x.own] == F32(Q.SENT)) and np.all(np.isfinite(got.z[x.own])) and np.all(got.z[x.own] != F32(Q.SENT)), what
    if x.part:
        assert g.changed("kl_part")[:x.nb].all() and np.all(g.get("zero")[:run.zero_n] == 0.0) and np.all(g.get("dz_zero")[x.own] == 0.0), what
        assert not run.dw or g.changed("kl_part_dw")[:x.nblk].all(), what
    r = Q.ratios(x, ref, got)
    for k, v in r.items():
        key = (f"{x.family}/{x.prior}", k)
        WORST[key] = max(WORST.get(key, 0.0), v)
    print(f"{what}: " + " ".join(f"{k} {v:.2e}" for k, v in r.items()))
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, (what, "error / bound", bad)
    return got


def same_bits(a, b, part):
    ok = all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in ((a.z, b.z), (a.d[0], b.d[0]), (a.d[1], b.d[1]), (a.dz, b.dz)))
    return ok and (not part or a.scalars.tobytes() == b.scalars.tobytes())      # (without kl_part the KL is a double atomic per workgroup)


def report(prefix):
    print("largest error / bound so far:", {f"{k[0]} {k[1]}": f"{v:.2e}" for k, v in sorted(WORST.items()) if k[0].startswith(prefix)})


# ---- every case against the fp64 reference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", Q.GROUPS)
def test_direct_calls_match_fp64(group):
    cases = [c for c in Q.GPU_CASES if Q.group_of(c) == group]
    assert cases
    for c in cases:
        x, ref = Q.reference_for(c)
        got = check(Run(x).sequence(), ref)
        if c.child_list:                             # no atomic in the child-list form: a second run gives the same bits
            again = Run(x).sequence().result()
            assert same_bits(got, again, c.part), c.id
    report(group.rsplit("-R", 1)[0].replace("-", "/", 1))


def test_child_list_with_a_trainable_r_is_refused():
    x = Q.make_inputs(Q.case("dw", 513, 3, prior="dw", trainable=True))
    x.child_list = True
    Run(x).call("cl_tn_forward").call("cl_dw_prior_forward", expect=-2)


@pytest.mark.parametrize("kw", [dict(family="wide", R=1100, S=3, part=True, owned=True), dict(family="wide", R=513, S=4, inner=True),
                                dict(family="wide", R=513, S=4, prior="reference", part=True),
                                dict(family="dw", prior="dw", R=513, S=3, part=True, trainable=True), dict(family="dw", prior="dw", R=1100, S=1, child_list=True)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_a_raised_stop_flag_makes_every_call_write_nothing(kw):
    x = Q.make_inputs(Q.case(**kw))
    red = Q.reduce_inputs(33, 9)
    run = Run(x, stop=True, red=red).sequence(untouched=True)
    lib = _lib.get_lib()
    assert int(lib.cl_reduce_partials(run.g.ptr("red_parts"), 9, 33, run.g.ptr("red_out2"), run.g.ptr("stop"), None)) == 0
    torch.cuda.synchronize()
    run.g.verify(untouched=True)


# ---- in-kernel noise -----------------------------------------------------------------------------------------------------------------------------
def dump_uniforms(S, n, offset):
    out = torch.empty(n * S, dtype=torch.float32, device=DEV)
    assert int(_lib.get_lib().cl_debug_noise(SEED, STEP, S, n, offset, 0, out.data_ptr(), None)) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(n, S)


@pytest.mark.parametrize("R,S,owned", [(257, 5, False), (513, 9, True), (1100, 3, True), (1100, 8, False)])
def test_in_kernel_noise_is_cl_debug_noise_kind_0_at_the_global_index(R, S, owned):
    c = Q.case("wide", R, S, part=True, owned=owned)
    x = Q.make_inputs(c)
    u = dump_uniforms(S, R, 0)
    assert np.all((u.astype(np.float64) * 2.0 ** 23 - 0.5) % 1.0 == 0.0) and u.min() > 0.0 and u.max() < 1.0       # the device's grid
    if owned:
        assert np.array_equal(dump_uniforms(S, x.r1 - x.r0, x.r0), u[x.r0:x.r1])                                   # offset = the global index
    drawn = Run(x, seeded=True).sequence().result()
    xi = copy.copy(x)
    xi.u = u
    ref = Q.reference(xi)
    injected = check(Run(xi).sequence(), ref, what=f"{c.id}-dumped-uniforms")
    assert same_bits(drawn, injected, True), c.id                                                               # z_f, both increments, the KL
    # a wrong uniform (the neighbouring reflection's) moves z_f by far more than its bound
    xw = copy.copy(x)
    xw.u = np.roll(u, 1, axis=0)
    moved = np.abs(Q.reference(xw).z - ref.z) / (Q.Z_TOL * (x.loc + x.scale)[:, None])
    assert np.median(moved[x.own]) > 100.0, float(np.median(moved[x.own]))


# ---- the ride-along reduction ----------------------------------------------------------------------------------------------------------------------
def test_ride_along_reduction_and_cl_reduce_partials_agree_and_hold_the_sum_bound():
    """Through cl_tn_backward's red_* fields (the workgroups behind the reflections': blockIdx.x - nb_tn) and through cl_reduce_partials alone, on
    top of a preloaded output: the two routes bit for bit, both within ref_step.sum_bound(nparts, sum |part|) on the dyadic inputs (tests/ref_q.py:
    every fp32 sum exact) and within the a-priori fp32 bound on floats over six decades; the reflections' gradients do not notice the passengers."""
    lib = _lib.get_lib()
    bases = [Q.make_inputs(Q.case("wide", 257, 1)), Q.make_inputs(Q.case("wide", 513, 3, owned=True))]
    plain = [Run(x).call("cl_tn_backward").result() for x in bases]
    worst, n = 0.0, 0
    for P in Q.RED_P:
        for nparts in Q.RED_NPARTS:
            n += 1
            for dyadic in (True, False):
                parts, pre = Q.reduce_inputs(P, nparts, dyadic)
                ref, total = Q.reduce_reference(parts, pre)
                k = (n + int(dyadic)) % 2                      # both kinds of input behind both launches: two workgroups of reflections, all / an owned range
                run = Run(bases[k], red=(parts, pre)).call("cl_tn_backward")
                assert int(lib.cl_reduce_partials(run.g.ptr("red_parts"), nparts, P, run.g.ptr("red_out2"), run.g.ptr("stop"), None)) == 0
                torch.cuda.synchronize()
                run.g.verify()
                a, b = run.g.get("red_out").copy(), run.g.get("red_out2").copy()
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (P, nparts, dyadic)
                bound = (Q.reduce_bound if dyadic else Q.reduce_bound_fp32)(nparts, total)
                err = np.abs(a.astype(np.float64) - ref)
                assert np.all(err <= bound), (P, nparts, dyadic, float(np.max(err / bound)))
                worst = max(worst, float(np.max(err / bound)))
                got = run.result()
                assert all(np.array_equal(got.d[j].view(np.uint32), plain[k].d[j].view(np.uint32)) for j in (0, 1)), (P, nparts)
    print("reduction: largest error / bound", worst)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def _refusals(x, entries):
    """(entry point, fields to break, expected return) one at a time on a fresh, otherwise valid argument block: refused before any launch"""
    run = Run(x, red=Q.reduce_inputs(33, 9))
    base = bytes(run.A)
    for name, fields, expect in entries:
        C.memmove(C.byref(run.A), base, len(base))
        for k, v in fields.items():
            setattr(run.A, k, v(run) if callable(v) else v)
        ret = int(getattr(_lib.get_lib(), name)(C.byref(run.A), None))
        assert ret == expect, (name, sorted(fields), ret, expect)
    torch.cuda.synchronize()
    run.g.verify(untouched=True)
    return run


FWD, BWD, DWF = "cl_tn_forward", "cl_tn_backward", "cl_dw_prior_forward"


def test_refusals_of_the_posterior_calls_write_nothing():
    lib = _lib.get_lib()
    for name in (FWD, BWD, DWF):
        assert int(getattr(lib, name)(None, None)) == -1
    x = Q.make_inputs(Q.case("wide", 513, 3, part=True))
    R = x.R
    check_tn = [dict(q_loc_raw=None), dict(q_scale_raw=None), dict(low=None), dict(R=0), dict(S=0), dict(centric=None), dict(es=None),
                dict(prior_kind=3), dict(prior_kind=-1), dict(r_begin=-1, r_end=5), dict(r_begin=3, r_end=R + 1)]
    entries = [(name, f, -1) for f in check_tn for name in (FWD, BWD)]
    entries += [(FWD, f, -1) for f in (dict(z_f=None), dict(scalars=None), dict(zero_n=0), dict(zero_ptr=lambda r: r.g.ptr("zero") + 4), dict(kl_part=None))]
    entries += [(BWD, f, -1) for f in (dict(dz_f=None), dict(d_loc_raw=None), dict(d_scale_raw=None), dict(red_out=None), dict(red_nparts=0), dict(red_P=0))]
    entries += [(DWF, {}, -1)]                                       # not the double-Wilson prior
    run = _refusals(x, entries)
    g = run.g
    for args in ((None, 9, 33, g.ptr("red_out")), (g.ptr("red_parts"), 9, 33, None), (g.ptr("red_parts"), 0, 33, g.ptr("red_out")),
                 (g.ptr("red_parts"), 9, 0, g.ptr("red_out"))):
        assert int(lib.cl_reduce_partials(args[0], args[1], args[2], args[3], None, None)) == -1
    torch.cuda.synchronize()
    g.verify(untouched=True)


@pytest.mark.parametrize("trainable", [False, True])
def test_refusals_under_the_double_wilson_prior_write_nothing(trainable):
    x = Q.make_inputs(Q.case("dw", 513, 3, prior="dw", part=True, trainable=trainable))
    three = (FWD, BWD, DWF)
    entries = [(n, f, -1) for f in (dict(parent_ids=None), dict(root=None), dict(centric=None), dict(es=None), dict(low=None)) for n in three]
    entries += [(n, dict(r_begin=100, r_end=300), -2) for n in three]                 # an owned range: a child's parent may belong to another rank
    entries += [(n, (dict(asu_ids=None) if trainable else dict(dw_r=None)), -1) for n in three]
    entries += [(DWF, f, -1) for f in (dict(z_f=None), dict(dz_f_out=None), dict(scalars=None), dict(prior_kind=_lib.CL_PRIOR_WILSON),
                                       dict(dw_child_seg=lambda r: r.g.ptr("child_seg")), dict(dw_child_ids=lambda r: r.g.ptr("child_ids")))]
    both = dict(dw_child_seg=lambda r: r.g.ptr("child_seg"), dw_child_ids=lambda r: r.g.ptr("child_ids"))
    if trainable:
        entries += [(DWF, dict(d_dw_r_raw=None), -1), (DWF, dict(n_asu=0), -1), (DWF, both, -2)]      # the child-list form: fixed r only
    _refusals(x, entries)
