"""tests/ref_q.py checked without a GPU: the fp64 reference of the posterior / prior half of the step against the oracle composed by hand,
its summand sizes, the fp32 emulation (numpy float32 in the kernels' order, scalar functions from the host build of csrc/cl_math.h) inside a
quarter of every bound of tests/test_q_kernels_gpu.py on the inputs of every GPU case, and eleven wrong kernels ("mutants" of the emulation)
each outside a bound by 4 x or more on some GPU case's inputs: the inputs have the power to see them.

A quarter of a gradient bound: the kernel's own share, RTOL_GRAD M, is held to a quarter; the rounding of the store on top of the preloaded
value (u |stored sum|, the bound's second term) is used up to the full by ANY kernel and is allowed in full (ref_q._worst_grad).

Measured here (host build, glibc's expf / erfcf / log1pf), the largest ratio to each bound over the GPU cases' inputs:
    z_f error / (1e-5 (loc + scale))          wide 0.10, tiny scale 0.012, double Wilson 0.071
    KL error / (RTOL_LOSS max(|KL|, 1))       wide 1.7e-3, tiny scale 7e-5, double Wilson 5.7e-3
    gradient error / (RTOL_GRAD M)            wide 0.19 (d_loc_raw, R = 1100: error / M 3.8e-5), tiny scale 4.8e-4 / 7.5e-4 (error / M 1.5e-7),
                                              double Wilson 0.17 (d_scale_raw), dz_f 0.13, d_dw_r_raw 5.6e-3
    max-norm error / RTOL_GRAD, wide family   0.12
    reduction                                 0 on the dyadic inputs, 0.49 of the a-priori fp32 bound on floats
On the tiny-scale family the max-norm error of d_loc_raw is 0.07 .. 0.22 of the largest entry in this (in any) fp32 evaluation: M reaches 2.5e7
where the entries are O(1), the +-y / scale of dlog q / dz and dlog q / dloc cancel.  That family gets the element-wise bound only.
Every mutant is outside a bound by 195 x (the reference prior's parts counted over the owned workgroups) to 6e6 x.
"""
import numpy as np
import pytest
import torch

from oracle import elbo_oracle as O
from tests import ref_q as Q
from tests import ref_step

T = Q.T


@pytest.fixture(scope="module")
def hm():
    lib = Q.host_lib()
    if lib is None:
        pytest.skip("g++ not available")
    return lib


def test_tolerances_are_the_projects_own():
    from tests import test_gpu_parity as P
    assert (Q.RTOL_LOSS, Q.RTOL_GRAD) == (P.RTOL_LOSS, P.RTOL_GRAD)


def test_case_list_covers_what_the_kernels_branch_on():
    cs = Q.GPU_CASES
    assert len({c.id for c in cs}) == len(cs) and {c.R for c in cs} == set(Q.RS) and {c.S for c in cs} == {1, 3, 4, 5, 8, 9}
    big = [c for c in cs if c.R > 256]
    assert {c.S for c in big} == {1, 3, 4, 5, 8, 9}
    for prior in ("wilson", "reference", "dw"):
        sub = [c for c in big if c.prior == prior]
        assert {(c.part, c.inner) for c in sub} == {(p, i) for p in (False, True) for i in (False, True)}, prior
        assert {c.zeros for c in sub} == {False, True}
        assert (prior == "dw") or {c.owned for c in sub} == {False, True}
    dw = [c for c in big if c.prior == "dw"]
    assert {c.layout for c in dw if c.trainable} == {"cut", "b64", "inwave", "klwave"} and any(c.child_list for c in dw)
    assert any(c.family == "tiny" and c.owned and c.part for c in big) and any(c.S == 3 for c in big)
    assert 0.4 < np.mean([c.zeros for c in cs]) < 0.6


@pytest.mark.parametrize("family,trainable", [("wide", False), ("tiny", False), ("dw", False), ("dw", True)])
def test_reference_equals_the_oracle_composed_by_hand(family, trainable):
    """Unmasked inputs (no owned range, the whole KL range): z, KL and gradients from O.tn_* / O.wilson_log_prob / O.double_wilson_log_prob
    written out here, at 1e-12 (gradients: of their summand size, which bounds an fp64 evaluation's rounding as it does an fp32 one's);
    the chain rule over the reference's partial derivatives gives the same gradients; the summand sizes dominate the entries."""
    for R, S in ((257, 3), (600, 4)):
        prior = "dw" if family == "dw" else "wilson"
        x = Q.make_inputs(Q.case(family, R, S, prior=prior, trainable=trainable))
        ref = Q.reference(x)
        assert x.own.all() and x.in_kl.all()
        ta, tb = T(x.a).requires_grad_(True), T(x.b).requires_grad_(True)
        leaves = [ta, tb]
        loc, scale = O.tn_loc_scale(ta, tb, float(np.float32(Q.EPS)))
        low, high = T(x.low), T(float(np.float32(Q.HIGH)))
        z = O.tn_sample(loc, scale, low, high, T(x.u.T))
        lq = O.tn_log_prob(z, loc, scale, low, high)
        ct, one, es = torch.as_tensor(x.centric.astype(bool)), T(np.ones(R)), T(x.es)
        if prior == "wilson":
            lp = O.wilson_log_prob(z, ct, one, es)
        else:
            if trainable:
                raw = T(x.r_raw).requires_grad_(True)
                leaves.append(raw)
            r = torch.sigmoid(raw) if trainable else T(x.r_asu)
            lp = O.double_wilson_log_prob(z, ct, one, es, torch.as_tensor(x.par.astype(np.int64)), torch.as_tensor(x.root.astype(bool)),
                                          torch.as_tensor(x.asu.astype(np.int64)), r)
        wk = float(x.w_kl)
        kl = wk * (lq - lp).sum()
        g = torch.autograd.grad((T(x.dz.T) * z).sum() + x.mult * kl, leaves)
        assert np.max(np.abs(ref.z - z.detach().numpy().T) / ref.z) < 1e-12
        assert abs(ref.kl - float(kl.detach())) <= 1e-12 * max(abs(float(kl.detach())), 1.0)
        for k in (0, 1):
            assert np.all(np.abs(ref.g[k] - g[k].numpy()) <= 1e-12 * ref.M[k]), (family, R, S, k)
            assert np.all(ref.M[k] * (1.0 + 1e-12) >= np.abs(ref.g[k])) and np.all(ref.M[k] > 0.0)
        if trainable:
            assert np.all(np.abs(ref.g_r - g[2].numpy()) <= 1e-12 * np.maximum(ref.M_r, 1e-300)) and np.all(ref.M_r >= np.abs(ref.g_r))
            assert ref.M_r[0] == 0.0 and np.all(ref.M_r[1:] > 0.0)
        # the chain rule the kernel follows, over the reference's partial derivatives
        p, wg = ref.parts, wk * x.mult
        gz = x.dz.astype(np.float64) + p.c_sum + wg * (p.dq_dz - p.dp_dz)
        for k, (dzd, dqd, fac) in enumerate(((p.dz_dloc, p.dq_dloc, x.loc), (p.dz_dscale, p.dq_dscale, x.scale - float(np.float32(Q.EPS))))):
            chain = (gz * dzd + wg * dqd).sum(1) * fac
            assert np.all(np.abs(chain - ref.g[k]) <= 1e-12 * ref.M[k]), (family, R, S, k)
        assert np.all(np.abs(ref.dz_after - (x.dz + p.c_sum)) == 0.0) and np.all(ref.M_dz >= np.abs(ref.dz_after))


@pytest.mark.parametrize("group", Q.GROUPS)
def test_emulation_stays_inside_a_quarter_of_every_bound(hm, group):
    worst = {}
    for c in Q.GPU_CASES:
        if Q.group_of(c) != group:
            continue
        x, ref = Q.reference_for(c)
        r = Q.ratios(x, ref, Q.emulate(x, hm))
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= 0.25, (c.id, k, v)
    print(group, {k: f"{v:.2e}" for k, v in sorted(worst.items())})


TARGETS = {                       # mutant -> the GPU cases whose inputs must show it
    "last_kl_part": lambda c: c.part and c.R >= 513 and c.prior == "wilson",
    "no_r_begin": lambda c: c.owned and c.R >= 513,
    "scale_not_minus_eps": lambda c: c.family == "tiny",
    "no_kl_grad_mult": lambda c: c.S == 3 and c.R >= 513,
    "no_alpha_term": lambda c: c.family == "wide" and c.prior == "wilson" and c.R >= 513,
    "child_wilson_dz": lambda c: c.prior == "dw" and c.R >= 513,
    "scatter_sign": lambda c: c.prior == "dw" and c.R >= 513,
    "absent_parent_is_0": lambda c: c.prior == "dw" and c.R >= 513,
    "no_sigmoid_derivative": lambda c: c.prior == "dw" and c.trainable and c.R >= 513,
    "ref_part_dw_owned_count": lambda c: c.prior == "reference" and c.part and c.owned and c.R == 1100,
}


@pytest.mark.parametrize("mutant", Q.MUTANTS)
def test_every_mutant_is_outside_a_bound_by_four_times(hm, mutant):
    cases = [c for c in Q.GPU_CASES if TARGETS[mutant](c)][:4]
    assert cases
    best = (0.0, None, None)
    for c in cases:
        x, ref = Q.reference_for(c)
        r = Q.ratios(x, ref, Q.emulate(x, hm, mutant=mutant))
        k = max(r, key=r.get)
        best = max(best, (r[k], k, c.id))
    print(mutant, best)
    assert best[0] >= 4.0, (mutant, best)


def test_reduction_emulation_and_its_mutant():
    worst, mutant = 0.0, {}
    for P in Q.RED_P:
        for nparts in Q.RED_NPARTS:
            for dyadic in (True, False):
                parts, pre = Q.reduce_inputs(P, nparts, dyadic)
                ref, total = Q.reduce_reference(parts, pre)
                bound = (Q.reduce_bound if dyadic else Q.reduce_bound_fp32)(nparts, total)
                err = np.abs(Q.reduce_emulate(parts, pre).astype(np.float64) - ref)
                assert np.all(err <= bound), (P, nparts, dyadic, float(np.max(err / bound)))      # (a-priori: a lone rounding reaches it)
                if dyadic:
                    assert np.all(err == 0.0)                    # (the grid: every fp32 sum is exact)
                else:
                    worst = max(worst, float(np.max(err / bound)))
                m = np.abs(Q.reduce_emulate(parts, pre, mutant="no_chunk_tail").astype(np.float64) - ref)
                mutant[(P, nparts, dyadic)] = float(np.max(m / bound))
    print("fp32 reduction: error / bound", worst)
    # the mutant drops the rows a chunk's groups of eight leave over: nothing at 64 rows a chunk... every nparts of the list has such rows
    assert all(v >= 4.0 for v in mutant.values()), mutant
    assert Q.reduce_bound(67, 1.0) == ref_step.sum_bound(67, 1.0)
