"""The posterior and prior half of the step -- one cl_tn_forward [+ cl_dw_prior_forward] + cl_tn_backward sequence on injected uniforms, and
the ride-along reduction of cl_tn_backward / cl_reduce_partials -- restated in torch fp64 from the contract (include/careless_hip.h: the
comments on cl_tn_args), with a summand size M per gradient entry, the bounds the direct kernel tests hold the device to, the inputs of those
tests, and an fp32 emulation of the kernels' arithmetic through the host build of csrc/cl_math.h (tests/host_math_check.cpp).

`reference`: loc, scale = O.tn_loc_scale; z = O.tn_sample; KL = w_kl sum over the owned KL range of O.tn_log_prob - prior, the prior being
O.wilson_log_prob, O.double_wilson_log_prob or nothing (a reference prior's term is cl_ref_prior's); gradients by autograd of
    loss = sum dz_f z [owned rows] + w_kl kl_grad_mult sum_{in KL} (log q - log p)
with respect to the raw parameters (a = log loc, b = log(scale - eps), the pre-sigmoid r per ASU).  Every float of the argument block enters as
the float32 it is, widened.

The summand size M of a gradient entry is the same chain rule with every summand replaced by its absolute value:
    Mz[s]      = |data dz_f| + sum over children |w dlog p(child) / dz_parent| + w |dlog q / dz| + w |dlog p / dz|         (w = w_kl kl_grad_mult)
    M(loc raw) = loc   sum_s (Mz |dz / dloc|   + w |dlog q / dloc|)
    M(scale raw) = scale sum_s (Mz |dz / dscale| + w |dlog q / dscale|)
    M(r raw)   = sum over the ASU's children in the KL range, sum_s w |dlog p / dr| r (1 - r);    M(dz_f) = |dz_f| + sum over children |w dlog p / dz_parent|
An fp32 evaluation's rounding is proportional to M, not to the entry: at scale << loc the +-y / scale of dlog q / dz and dlog q / dloc cancel,
and the entry is 1e-7 of M.  Bounds (`ratios`): z_f 1e-5 (loc + scale) per element; KL RTOL_LOSS max(|KL|, 1); every gradient entry and every
dz_f element after the parents' scatter RTOL_GRAD M + one fp32 rounding of the stored sum; on the wide family also RTOL_GRAD of the max-norm;
entries outside the owned range bit-unchanged.

The ride-along reduction adds in fp32; the bound set for it, ref_step.sum_bound(nparts, sum |part|), is that of a DOUBLE sum.  The inputs
it is asserted on (`reduce_inputs`) therefore lie on a dyadic grid (k / 64, |k| <= 2^12, preloaded output included) on which every fp32 sum of
<= 67 terms is exact in any order: the bound then holds for a correct kernel and a dropped, doubled or misplaced term breaks it by ten orders.
"""
from __future__ import annotations

import ctypes
import itertools
import os
import shutil
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np
import torch

from oracle import elbo_oracle as O
from tests import ref_step

F32 = np.float32
EPS, HIGH = 1e-7, 1e10
RTOL_LOSS, RTOL_GRAD = 1e-4, 2e-4        # tests/test_gpu_parity.py's (asserted equal in tests/test_ref_q.py)
Z_TOL = 1e-5                             # tests/test_host_math.py::test_truncated_normal_element, the Rice-Woolfson z_f
U = ref_step.U
KL_BEFORE, SENT = 3.5, -7.25e30          # scalars[CL_SC_KL] before a call that ADDS; what a kl_part slot / z_f element holds before a call that STORES
R_RAW = (0.0, 2.0, 0.4)                  # pre-sigmoid r of the three ASUs (the first is root: its r is never read)
FAMILY_ID = {"wide": 1, "tiny": 2, "dw": 3}
HERE = os.path.dirname(os.path.abspath(__file__))


def T(v):
    return torch.as_tensor(np.asarray(v, dtype=np.float64))


# ---- cases and inputs ---------------------------------------------------------------------------------------------------------------------
def case(family, R, S, prior="wilson", part=False, inner=False, owned=False, trainable=False, layout="cut", child_list=False, zeros=False, seed=0):
    """One call sequence.  family: wide / tiny / dw (the inputs); prior: wilson / reference / dw; part: kl_part mode (with zero_ptr, zero_dzf);
    inner: a KL range inside [0, R); owned: an owned range with r_begin no multiple of 256; dw only: trainable r, the ASU layout, the child-list
    form; zeros: the buffers the calls add to hold exact zeros."""
    assert (prior == "dw") == (family == "dw") and not (owned and prior == "dw") and not (child_list and trainable)
    c = SimpleNamespace(family=family, R=R, S=S, prior=prior, part=part, inner=inner, owned=owned, trainable=trainable, layout=layout,
                        child_list=child_list, zeros=zeros, seed=seed)
    c.id = (f"{family}-{prior}-R{R}-S{S}" + ("-part" if part else "") + ("-inner" if inner else "") + ("-owned" if owned else "") +
            ("-trainable" if trainable else "") + (f"-{layout}" if layout != "cut" else "") + ("-childlist" if child_list else "") + ("-zeros" if zeros else ""))
    return c


def dw_layout(R, layout):
    """(c1, c2, kl_begin or None): three ASUs [0, c1) root, [c1, c2), [c2, R).  cut: 0.36 R and 0.67 R; b64: borders at multiples of 64 (a wave
    holds one ASU: the wave-reduced atomic); inwave: borders 17 and 41 lanes into a wave (two ASUs in a wave: the lane-by-lane atomics);
    klwave: borders at multiples of 64 and kl_begin five lanes into a wave of children (lane 0 inactive: the ASU of the first active lane)."""
    c1, c2 = int(round(0.36 * R)), int(round(0.67 * R))
    if layout == "cut":
        return c1, c2, None
    b1, b2 = max(64, c1 // 64 * 64), max(128, c2 // 64 * 64)
    if layout == "b64":
        return b1, b2, None
    if layout == "inwave":
        return b1 + 17, b2 + 41, None
    assert layout == "klwave"
    return b1, b2, b1 + 64 + 5


def make_inputs(c):
    """The float32 / integer operands of the calls of case c (seeded default_rng)."""
    R, S = c.R, c.S
    rng = np.random.default_rng([FAMILY_ID[c.family], R, S, c.seed])
    if c.family == "wide":
        ratio = 10 ** np.linspace(-3, 3, R)[rng.permutation(R)] if R > 1 else np.array([2.0])
        scale = 10 ** rng.uniform(-1.5, 1.5, R)
        loc = ratio * scale
    elif c.family == "tiny":
        scale, loc = 10 ** rng.uniform(-6.7, -3, R), 10 ** rng.uniform(-1, 1, R)
    else:
        loc = rng.uniform(0.5, 3, R)
        scale = loc / 10 ** rng.uniform(-0.5, 2.5, R)
    x = SimpleNamespace(case=c, R=R, S=S, family=c.family, prior=c.prior, part=c.part, trainable=c.trainable, child_list=c.child_list)
    x.a, x.b = np.log(loc).astype(F32), np.log(scale - EPS).astype(F32)
    x.loc, x.scale = np.exp(x.a.astype(np.float64)), np.exp(x.b.astype(np.float64)) + float(F32(EPS))
    x.centric = (rng.random(R) < 0.3).astype(np.uint8)
    x.low = np.where(rng.random(R) < 0.1, 0.0, 1e-32).astype(F32)
    x.u = ((rng.integers(0, 1 << 23, (R, S)) + 0.5) * 2.0 ** -23).astype(F32)                     # the device's grid: exact in fp32
    assert np.all((x.u.astype(np.float64) * 2.0 ** 23 - 0.5) % 1.0 == 0.0)
    if c.family == "dw":
        x.es = rng.choice([1.0, 2.0, 3.0], R).astype(F32)
    else:
        x.es = ((x.loc ** 2 + x.scale ** 2) * rng.uniform(0.5, 2.0, R)).astype(F32)
    dz = (rng.normal(size=(R, S)) / (x.loc + x.scale)[:, None]).astype(F32)                      # dL/dz of a loss of O(1) per reflection
    pre = rng.normal(size=(2, R)).astype(F32)
    x.dz, x.pre, x.kl_before = (np.zeros_like(dz), np.zeros_like(pre), 0.0) if c.zeros else (dz, pre, KL_BEFORE)
    if c.family == "dw":
        # (changed inputs: dz_f keeps the data term in the double-Wilson cases with zeroed accumulators.  A parent whose dz_f holds nothing but
        #  one child's w dlog p / dz_parent has M = |that term|, and the Rice derivative -nu / s^2 + z I1/I0 / s^2 cancels inside it: fp32 is
        #  off by up to 30 x the bound there, in any evaluation.  The data term is what the scatter adds to in a step.)
        x.dz = dz
    x.w_kl, x.mult = F32(1.0 / S), (0.5 if S == 3 else 1.0)
    x.k0, x.k1 = (R // 3, R - R // 4) if c.inner and R >= 4 else (0, R)
    x.r0, x.r1 = (R // 5, R - R // 6) if c.owned and R >= 6 else (0, 0)
    assert x.r1 <= x.r0 or x.r0 % 256 != 0
    x.nblk = (R + 255) // 256
    x.kl_part_dw_pre = np.arange(1.0, x.nblk + 1.0)                                                # what a cl_ref_prior in front of the backward call left
    if c.prior == "dw":
        c1, c2, kb = dw_layout(R, c.layout)
        assert 0 < c1 < c2 < R
        if kb is not None:
            x.k0, x.k1 = kb, R - 3
        x.asu = np.repeat(np.arange(3), [c1, c2 - c1, R - c2]).astype(np.int32)
        x.root = (x.asu == 0).astype(np.uint8)
        lo = np.array([0, 0, c1])[x.asu]
        hi = np.array([1, c1, c2])[x.asu]
        x.par = np.where((x.asu > 0) & (rng.random(R) >= 0.1), rng.integers(lo, hi), -1).astype(np.int32)   # a parent from the ASU before; one in ten absent
        x.r_raw = np.array(R_RAW, F32)
        x.r_asu = (1.0 / (1.0 + np.exp(-x.r_raw.astype(np.float64)))).astype(F32)
        x.dw_r = x.r_asu[x.asu]
        x.pre_r = np.zeros(3, F32) if c.zeros else rng.normal(size=3).astype(F32)
        order = np.argsort(x.par, kind="stable")
        order = order[x.par[order] >= 0]
        x.child_ids = order.astype(np.int32)                                                      # CSR: the children of p, ascending
        x.child_seg = np.searchsorted(x.par[order], np.arange(R + 1)).astype(np.int32)
        nshared = np.bincount(x.par[x.par >= 0], minlength=R)
        assert nshared.max() >= 2 and np.any((x.par >= 0) & (x.par // 256 != np.arange(R) // 256)) or R < 300
    idx = np.arange(R)
    x.own = np.ones(R, bool) if x.r1 <= x.r0 else (idx >= x.r0) & (idx < x.r1)
    x.in_kl = (idx >= x.k0) & (idx < x.k1) & x.own
    x.nb = (int(x.own.sum()) + 255) // 256
    return x


# ---- the fp64 reference ---------------------------------------------------------------------------------------------------------------------
def _prior(x, z, r):
    ct, one, es = torch.as_tensor(x.centric.astype(bool)), T(np.ones(x.R)), T(x.es)
    if x.prior == "reference":
        return torch.zeros_like(z)
    if x.prior == "wilson":
        return O.wilson_log_prob(z, ct, one, es)
    return O.double_wilson_log_prob(z, ct, one, es, torch.as_tensor(x.par.astype(np.int64)), torch.as_tensor(x.root.astype(bool)),
                                    torch.as_tensor(x.asu.astype(np.int64)), r)


def reference(x):
    """z (R, S), kl (the increment of scalars[CL_SC_KL], a reference prior's ride-along parts included in kl_part mode), g = [d_loc_raw, d_scale_raw]
    increments, M = their summand sizes, dz_after / M_dz (R, S), g_r / M_r (double Wilson), and the partial derivatives M is made of."""
    R, S = x.R, x.S
    eps, low, high, uT = float(F32(EPS)), T(x.low), T(float(F32(HIGH))), T(x.u.T)
    wk = float(x.w_kl)
    wg = wk * x.mult
    own, in_kl = T(x.own), T(x.in_kl)
    ta, tb = T(x.a).requires_grad_(True), T(x.b).requires_grad_(True)
    raw = T(x.r_raw).requires_grad_(True) if x.prior == "dw" and x.trainable else None
    r = None if x.prior != "dw" else (torch.sigmoid(raw) if raw is not None else T(x.r_asu))
    loc, scale = O.tn_loc_scale(ta, tb, eps)
    z = O.tn_sample(loc, scale, low, high, uT)
    lq = O.tn_log_prob(z, loc, scale, low, high)
    kl_e = ((lq - _prior(x, z, r)) * in_kl).sum()
    loss = (T(x.dz.T) * z * own).sum() + wg * kl_e
    g = torch.autograd.grad(loss, [ta, tb] + ([raw] if raw is not None else []))
    out = SimpleNamespace(z=z.detach().numpy().T.copy(), kl=wk * float(kl_e.detach()), g=[g[0].numpy(), g[1].numpy()])
    if x.prior == "reference" and x.part:
        out.kl += float(x.kl_part_dw_pre.sum())
    # the partial derivatives, element by element: leaves of shape (S, R)
    L, Sc = loc.detach().expand(S, R).clone().requires_grad_(True), scale.detach().expand(S, R).clone().requires_grad_(True)
    zz = O.tn_sample(L, Sc, low, high, uT)
    dz_dloc, dz_dscale = torch.autograd.grad(zz.sum(), [L, Sc])
    zd = zz.detach().clone().requires_grad_(True)
    dq_dz, dq_dloc, dq_dscale = torch.autograd.grad(O.tn_log_prob(zd, L, Sc, low, high).sum(), [zd, L, Sc])
    dp_dz, c_sum, c_abs = torch.zeros(S, R, dtype=torch.float64), torch.zeros(S, R, dtype=torch.float64), torch.zeros(S, R, dtype=torch.float64)
    if x.prior == "wilson":
        zw = zz.detach().clone().requires_grad_(True)
        dp_dz, = torch.autograd.grad(_prior(x, zw, None).sum(), zw)
    elif x.prior == "dw":
        # reflection h twice: as itself (column h) and as the carrier of ITS parent's sample (column R + h, a root), so that the derivative
        # with respect to the parent's sample comes out child by child; r as an (S, 2R) leaf (`r[...]`), so that d/dr does too
        par = torch.as_tensor(x.par.astype(np.int64))
        san = torch.where(par >= 0, par, torch.zeros_like(par))
        zA, zB = zz.detach().clone().requires_grad_(True), zz.detach()[:, san].clone().requires_grad_(True)
        rr = torch.cat([r.detach()[torch.as_tensor(x.asu.astype(np.int64))]] * 2).expand(S, 2 * R).clone().requires_grad_(True)
        ct, rt = torch.as_tensor(x.centric.astype(bool)), torch.as_tensor(x.root.astype(bool))
        lp = O.double_wilson_log_prob(torch.cat([zA, zB], 1), torch.cat([ct, ct]), T(np.ones(2 * R)), T(np.concatenate([x.es, x.es])),
                                      torch.cat([torch.where(par >= 0, R + torch.arange(R), par), torch.full((R,), -1)]),
                                      torch.cat([rt, torch.ones(R, dtype=torch.bool)]), Ellipsis, rr)
        dp_dz, dzp, dr = torch.autograd.grad(lp[:, :R].sum(), [zA, zB, rr])
        child = torch.as_tensor(x.in_kl & (x.root == 0))
        sc = torch.as_tensor(x.in_kl & (x.root == 0) & (x.par >= 0))
        c_sum.index_add_(1, san[sc], -wg * dzp[:, sc])
        c_abs.index_add_(1, san[sc], wg * dzp[:, sc].abs())
        rv = r.detach()[torch.as_tensor(x.asu.astype(np.int64))]
        m_r = (wg * dr[:, :R].abs().sum(0) * rv * (1.0 - rv) * child).numpy()
        out.M_r = np.bincount(x.asu, weights=m_r, minlength=3)
        out.g_r = g[2].numpy() if raw is not None else np.zeros(3)
        out.dr = dr[:, :R].numpy().T.copy()
    w_h = wg * in_kl
    dz_data = T(x.dz.T).abs() * own
    Mz = dz_data + c_abs + w_h * (dq_dz.abs() + dp_dz.abs())
    out.M = [(((Mz * dz_dloc.abs() + w_h * dq_dloc.abs()).sum(0)) * loc.detach()).numpy(),
             (((Mz * dz_dscale.abs() + w_h * dq_dscale.abs()).sum(0)) * scale.detach()).numpy()]
    out.dz_after, out.M_dz = (T(x.dz.T) + c_sum).numpy().T.copy(), (T(x.dz.T).abs() + c_abs).numpy().T.copy()
    out.parts = SimpleNamespace(**{k: v.numpy().T.copy() for k, v in dict(dz_dloc=dz_dloc, dz_dscale=dz_dscale, dq_dz=dq_dz, dq_dloc=dq_dloc,
                                                                         dq_dscale=dq_dscale, dp_dz=dp_dz, c_sum=c_sum).items()})
    return out


_REFS = {}


def reference_for(c):
    """(inputs, reference) of a case, computed once per process and shared (treat both as read-only)"""
    if c.id not in _REFS:
        x = make_inputs(c)
        _REFS[c.id] = (x, reference(x))
    return _REFS[c.id]


# ---- bounds -----------------------------------------------------------------------------------------------------------------------------------
def _worst(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err > 0.0, err / bound, 0.0)
    return float(np.max(q)) if q.size else 0.0


def _worst_grad(err, M, stored):
    """|error| <= RTOL_GRAD M + one fp32 rounding of the stored sum, as a ratio: the error BEYOND that rounding (u |stored|: the store may use
    all of it, whatever the kernel computes) over RTOL_GRAD M.  <= 1 is the bound; <= f says that the kernel's own share is within f of its."""
    return _worst(np.maximum(err - U * np.abs(stored), 0.0), RTOL_GRAD * M)


def ratios(x, ref, got):
    """{quantity: largest error / bound} of a result `got`: z (R, S), kl (the increment), d = [d_loc_raw, d_scale_raw] as STORED on top of x.pre,
    and under the double-Wilson prior dz (stored) and d_r (stored on top of x.pre_r; trainable r).  1 is the bound (gradients: `_worst_grad`); an entry
    outside the owned range that moved counts as inf."""
    own = x.own
    out = {"z_f": _worst(np.abs(got.z.astype(np.float64) - ref.z)[own], (Z_TOL * (x.loc + x.scale))[own, None] * np.ones((1, x.S))),
           "kl": abs(got.kl - ref.kl) / (RTOL_LOSS * max(abs(ref.kl), 1.0))}
    for k, name in enumerate(("d_loc_raw", "d_scale_raw")):
        pre = x.pre[k].astype(np.float64)
        inc = got.d[k].astype(np.float64) - pre
        err = np.abs(inc - ref.g[k])
        out[name] = _worst_grad(err[own], ref.M[k][own], (pre + ref.g[k])[own])
        if np.any(inc[~own] != 0.0):
            out[name] = np.inf
        if x.family == "wide":
            out[name + " max-norm"] = float(np.max(err[own]) / np.max(np.abs(ref.g[k][own])) / RTOL_GRAD)
    if x.prior == "dw":
        out["dz_f"] = _worst_grad(np.abs(got.dz.astype(np.float64) - ref.dz_after), ref.M_dz, ref.dz_after)
        if x.trainable:
            pre = x.pre_r.astype(np.float64)
            out["d_dw_r_raw"] = _worst_grad(np.abs(got.d_r.astype(np.float64) - pre - ref.g_r), ref.M_r, pre + ref.g_r)
    return out


# ---- fp32 emulation ---------------------------------------------------------------------------------------------------------------------------
_HM = []


def host_lib():
    """tests/host_math_check.cpp compiled with g++ (as tests/test_host_math.py does), or None without a compiler"""
    if not _HM:
        if shutil.which("g++") is None:
            _HM.append(None)
        else:
            so = os.path.join(tempfile.mkdtemp(prefix="cl_hmq_"), "libhm.so")
            subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "host_math_check.cpp")])
            _HM.append(ctypes.CDLL(so))
    return _HM[0]


fp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
MUTANTS = ("last_kl_part", "no_r_begin", "scale_not_minus_eps", "no_kl_grad_mult", "no_alpha_term", "child_wilson_dz", "scatter_sign",
           "absent_parent_is_0", "no_sigmoid_derivative", "ref_part_dw_owned_count")
REDUCE_MUTANTS = ("no_chunk_tail",)


def hm_tn(hm, x):
    """the (R, S, 10) outputs of hm_tn: z, log q, dz/dloc, dz/dscale, dlogq/dz, dlogq/dloc, dlogq/dscale, loc, scale, e"""
    n = x.R * x.S
    a, b, low = (np.ascontiguousarray(np.repeat(v, x.S)) for v in (x.a, x.b, x.low))
    u = np.ascontiguousarray(x.u.ravel())
    out = np.empty((n, 10), F32)
    hm.hm_tn(n, fp(a), fp(b), fp(low), ctypes.c_float(HIGH), ctypes.c_float(EPS), fp(u), fp(out))
    return out.reshape(x.R, x.S, 10)


def emulate(x, hm, mutant=None):
    """The call sequence in numpy float32 in the kernels' own order (a thread per reflection: the loop over s, then the factor), the scalar
    functions from the host build.  Returns what `ratios` takes.  `mutant`: one of MUTANTS, a kernel that is wrong in one place."""
    R, S, n = x.R, x.S, x.R * x.S
    o = hm_tn(hm, x)
    z, lq, dzl, dzs, dqz, dql, dqs, loc, scale = (np.ascontiguousarray(o[..., k]) for k in range(9))
    eps32, w32 = F32(EPS), F32(x.w_kl)
    wg = w32 if mutant == "no_kl_grad_mult" else w32 * F32(x.mult)
    ref_kind, dw = x.prior == "reference", x.prior == "dw"
    cen = np.ascontiguousarray(np.repeat(x.centric.astype(np.int32), S))
    es = np.ascontiguousarray(np.repeat(x.es, S))
    lpw, dlpw = np.zeros(n, F32), np.zeros(n, F32)
    if not ref_kind:
        hm.hm_wilson(n, fp(np.ascontiguousarray(z.ravel())), fp(cen), fp(es), fp(lpw), fp(dlpw))
    lpw, dlpw = lpw.reshape(R, S), dlpw.reshape(R, S)
    child = (x.root == 0) if dw else np.zeros(R, bool)
    # tn_forward_kernel: the KL of the reflections it takes, a double per thread, a part per workgroup
    lp = np.where((child | ref_kind)[:, None] if dw else ref_kind, F32(0), lpw)
    kl_h = np.where(x.in_kl, (lq - lp).astype(np.float64).sum(1), 0.0) * float(w32)
    first = x.r0 if x.r1 > x.r0 else 0
    blk = (np.arange(R) - first) // 256
    part = np.array([kl_h[x.own & (blk == i)].sum() for i in range(x.nb)])
    part_dw = x.kl_part_dw_pre.copy() if ref_kind else np.zeros(x.nblk)
    dz_after, d_r = x.dz.copy(), None
    dp = np.zeros((R, S), F32) if ref_kind else dlpw
    if dw:
        par = np.where(x.par < 0, 0, x.par) if mutant == "absent_parent_is_0" else x.par
        has = (par >= 0) & child
        zp = np.where(has[:, None], z[np.where(has, par, 0)], F32(0))
        r_h = x.dw_r
        if x.trainable:                                            # cl_sigmoid of the host build (hm_bij's derivative of softplus)
            sg, dsg = np.empty(3, F32), np.empty(3, F32)
            hm.hm_bij(3, fp(x.r_raw), 1, ctypes.c_float(EPS), fp(sg), fp(dsg))
            r_h = dsg[x.asu]
        lpd, dzd, dzpd, drd = (np.zeros(n, F32) for _ in range(4))
        hm.hm_dw(n, fp(np.ascontiguousarray(z.ravel())), fp(np.ascontiguousarray(zp.ravel())), fp(np.ascontiguousarray(np.repeat(has.astype(np.int32), S))),
                 fp(np.ascontiguousarray(np.repeat(r_h, S))), fp(cen), fp(es), fp(lpd), fp(dzd), fp(dzpd), fp(drd))
        lpd, dzd, dzpd, drd = (v.reshape(R, S) for v in (lpd, dzd, dzpd, drd))
        act = child & x.in_kl
        kd = np.where(act, -lpd.astype(np.float64).sum(1), 0.0) * float(w32)
        part_dw = np.array([kd[np.arange(R) // 256 == i].sum() for i in range(x.nblk)])
        gr = np.zeros(R, F32)
        for s in range(S):
            gr = gr - wg * drd[:, s]
        if x.trainable:
            if mutant != "no_sigmoid_derivative":
                gr = gr * (r_h * (F32(1) - r_h))
            d_r = x.pre_r.copy()
            np.add.at(d_r, x.asu[act], gr[act])
        sc = np.flatnonzero(act & has)
        sign = F32(1) if mutant == "scatter_sign" else F32(-1)
        for s in range(S):
            np.add.at(dz_after[:, s], par[sc], sign * wg * dzpd[sc, s])
        dp = np.where(child[:, None], dlpw if mutant == "child_wilson_dz" else dzd, dlpw)
    # tn_backward_kernel
    if x.part:
        kl = part[:x.nb - 1 if mutant == "last_kl_part" else x.nb].sum()
        if dw or ref_kind:
            kl += part_dw[:x.nb if mutant == "ref_part_dw_owned_count" else x.nblk].sum()
    else:
        kl = part.sum() + (part_dw.sum() if dw else 0.0)
    wkl = np.where(x.in_kl, wg, F32(0)).astype(F32)
    if mutant == "no_alpha_term":                                   # e - alpha dl - beta du without alpha dl; dl = 1 - dz/dloc (du = 0 at high = 1e10)
        alpha = (x.low - loc[:, 0]) / scale[:, 0]
        dzs = np.where(dzl != 0, dzs + alpha[:, None] * (F32(1) - dzl), dzs).astype(F32)
    gloc, gscale = np.zeros(R, F32), np.zeros(R, F32)
    for s in range(S):
        gz = dz_after[:, s] + wkl * (dqz[:, s] - dp[:, s])
        gloc = gloc + (gz * dzl[:, s] + wkl * dql[:, s])
        gscale = gscale + (gz * dzs[:, s] + wkl * dqs[:, s])
    inc = [gloc * loc[:, 0], gscale * (scale[:, 0] if mutant == "scale_not_minus_eps" else scale[:, 0] - eps32)]
    d = [x.pre[0].copy(), x.pre[1].copy()]
    rows = np.flatnonzero(x.own) - (first if mutant == "no_r_begin" else 0)      # (the mutant: the thread of reflection h works on h - r_begin)
    for k in range(2):
        d[k][rows] = d[k][rows] + inc[k][rows]
    assert all(v.dtype == F32 for v in (gloc, gscale, d[0], d[1], dz_after))
    return SimpleNamespace(z=np.where(x.own[:, None], z, F32(SENT)), kl=float(kl), d=d, dz=dz_after, d_r=d_r, part=part, part_dw=part_dw)


# ---- the ride-along reduction --------------------------------------------------------------------------------------------------------------------
RED_P, RED_NPARTS = (1, 31, 32, 33, 1000), (1, 7, 8, 9, 67)


def reduce_inputs(P, nparts, dyadic=True):
    """(partials [nparts][P], preloaded out [P]).  dyadic: k / 64 with |k| <= 2^12, so that every fp32 sum of the column is exact in any order
    (the module docstring); else 10^U(-3, 3) with random signs."""
    rng = np.random.default_rng([7, P, nparts, int(dyadic)])
    if dyadic:
        return (rng.integers(-4096, 4097, (nparts, P)) / 64.0).astype(F32), (rng.integers(-4096, 4097, P) / 64.0).astype(F32)
    return ((10 ** rng.uniform(-3, 3, (nparts, P))) * rng.choice([-1.0, 1.0], (nparts, P))).astype(F32), rng.normal(size=P).astype(F32)


def reduce_reference(parts, pre):
    """(out, sum |part| with the preloaded value among the parts) in fp64"""
    p = parts.astype(np.float64)
    return pre.astype(np.float64) + p.sum(0), np.abs(p).sum(0) + np.abs(pre.astype(np.float64))


def reduce_emulate(parts, pre, mutant=None):
    """cl_reduce_partials_block in float32: eight chunks of ceil(nparts / 8) rows, each summed in row order (groups of eight, then the tail
    loop), the chunk sums added in chunk order, then out += t"""
    nparts, P = parts.shape
    per = (nparts + 7) // 8
    t = np.zeros(P, F32)
    for c in range(8):
        g0, g1 = c * per, min(nparts, (c + 1) * per)
        s = np.zeros(P, F32)
        full = g0 + max(g1 - g0, 0) // 8 * 8
        for g in range(g0, g1 if mutant != "no_chunk_tail" else full):
            s = s + parts[g]
        t = t + s
    return pre + t


def reduce_bound(nparts, total):
    return ref_step.sum_bound(nparts, total)


def reduce_bound_fp32(nparts, total):
    """a-priori bound of ANY-order fp32 summation of nparts + 1 terms (Higham, Accuracy and Stability, (4.4)): n u sum |x|, first order"""
    return (nparts + 1) * U * total


# ---- the cases of the GPU tests ------------------------------------------------------------------------------------------------------------------
RS = (1, 255, 256, 257, 513, 1100)
S_OF = {1: (1, 4), 255: (3, 5), 256: (1, 8), 257: (3, 4, 9), 513: (1, 3, 5, 8), 1100: (1, 3, 4, 5, 8, 9)}     # every S at R > 256, S = 3 (kl_grad_mult 0.5) at four R
REF_RS = ((257, 3), (513, 4), (1100, 3), (1100, 9))
TINY_RS = ((257, 1), (513, 3), (1100, 5), (1100, 8))
DW_RS = ((255, 3), (256, 1), (257, 4), (513, 8), (513, 9), (1100, 1), (1100, 5))
DW_LAYOUT_RS = ((513, 3), (1100, 4))
ONOFF = (False, True)


def _cases():
    out = []
    for R in RS:
        for S in S_OF[R]:
            for part, inner, owned in itertools.product(ONOFF, ONOFF, ONOFF):
                if R == 1 and (inner or owned):
                    continue
                out.append(dict(family="wide", R=R, S=S, part=part, inner=inner, owned=owned))
    for R, S in REF_RS:
        for part, inner, owned in itertools.product(ONOFF, ONOFF, ONOFF):
            out.append(dict(family="wide", R=R, S=S, prior="reference", part=part, inner=inner, owned=owned))
    for R, S in TINY_RS:
        for part, owned in itertools.product(ONOFF, ONOFF):
            out.append(dict(family="tiny", R=R, S=S, part=part, inner=(S == 3), owned=owned))
    for R, S in DW_RS:
        for part, inner in itertools.product(ONOFF, ONOFF):
            for trainable, child_list in ((False, False), (False, True), (True, False)):
                if child_list and part == inner:                   # (the child-list form: kl_part alone and the inner range alone)
                    continue
                out.append(dict(family="dw", prior="dw", R=R, S=S, part=part, inner=inner, trainable=trainable, child_list=child_list))
    for layout in ("b64", "inwave", "klwave"):
        for R, S in DW_LAYOUT_RS:
            for part in ONOFF:
                out.append(dict(family="dw", prior="dw", R=R, S=S, part=part, trainable=True, layout=layout))
    return [case(zeros=(bin(i).count("1") % 2 == 1), **kw) for i, kw in enumerate(out)]      # half of them, not aligned with any of the switches


GPU_CASES = _cases()


def group_of(c):
    return f"{c.family}-{c.prior}-R{c.R}"


GROUPS = sorted({group_of(c) for c in GPU_CASES})
