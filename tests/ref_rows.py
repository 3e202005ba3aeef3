"""The row-level data-term kernels -- cl_frozen_rows in its three forms (csrc/elbo_frozen.hip, csrc/elbo_frozen_rows.h), cl_laue_predict /
cl_laue_likelihood / cl_laue_backward and cl_slot_rows (csrc/elbo_laue.hip), cl_det_reduce (csrc/elbo_det.hip) -- restated ONCE in torch
fp64 from the contract (include/careless_hip.h: the comments on cl_frozen_args, cl_laue_args, cl_det_args), with a summand size M beside
every output element, the bounds the direct kernel tests hold the device to (tests/test_rows_kernels_gpu.py), the inputs and the case list
of those tests, and an fp32 emulation of each kernel's arithmetic in the kernel's own order through the host build of csrc/cl_math.h
(tests/host_math_check.cpp).  tests/test_ref_rows.py checks all of it without a GPU.

`reference(x)` over plain arrays: rows i with refl_id, an image scale (image_id into [1, img], image 0 pinned to 1 and without a gradient, or
a scale per row), an optional slot map (harmonic_id, or the position of member 0 of a row's harmonic group), (loc, sigma), eta in the rows'
order:
    ipred[i][s] = aim_i (loc_i + sigma_i eta[i][s] + shift) z_f[refl_i][s]^2            0 on rows with refl_id < 0
    iconv       = O.laue_convolve(ipred, slot)                                           (ipred itself without a slot map)
    NLL         = -w_ll sum over the COUNTED slots and samples of log p(iconv | iobs, sig)
log p from O.normal_log_prob / O.studentt_log_prob / O.laplace_log_prob; under the Evans-2011 error model sig is the oracle's
(O.elbo_forward: sd[0] sqrt(sig^2 + sd[2] sp + sd[1] sp^2), sd = softplus(raw), sp = softplus(iconv); tests/test_ref_rows.py holds the whole
reference against O.elbo_value_and_grads).  Which slots count: every active row (monochromatic), every slot 0 .. n_obs - 1 (Laue: the slots
past the last group keep iconv = 0 and still count, elbo_laue.hip:1-6), member 0 of every group (the GROUPS form: the padded slots' constant
is another call's).  Gradients of the NLL by autograd: dz_f[R][S], d_img[M - 1], dO[n][2] = d / d(loc, sigma), d_ev11[3] (raw), dNLL / diconv,
and the row's own share of dz_f (the GROUPS form's gbuf).

The summand size M of an output element is the same chain rule with every summand replaced by its absolute value -- the residual inside the
likelihood's derivative included, so that an observation the prediction fits is not credited with its cancellation:
    M(ipred)  = |aim| (|loc| + |sigma eta| + |shift|) z^2                  M(iconv) = sum over the slot's rows
    M(dlogp / dx):  Normal (M(iconv) + |iobs|) / sig^2;  Student-t (nu + 1) (M(iconv) + |iobs|) / (sig^2 (nu + y^2));  Laplace sqrt2 / sig (its
                    derivative holds no residual, only its sign: no input of the fitted family is Laplace)
    Evans-2011 adds M(dlogp / dsig) |dsig / dx|,  M(dlogp / dsig) = (t |y| (M(iconv) + |iobs|) / sig + 1) / sig,  t = 1 or (nu + 1) / (nu + y^2)
    M(dz_f[r][s]) = sum over the rows of r of w_ll M(dlogp / dx) |aim tq 2 z|,   M(d_img), M(dO), M(d_ev11) likewise
    M(NLL) = w_ll sum over the counted (slot, sample) of |data term| + |log sig| + |constant| + |dlogp / dx| M(iconv)
Bounds (`*_ratios`; RTOL_LOSS, RTOL_GRAD are tests/test_gpu_parity.py's): ipred, iconv RTOL_LOSS M per element; NLL RTOL_LOSS max(M, 1); every
entry of dz_f, d_img, dO, d_ev11, dNLL / diconv and gbuf RTOL_GRAD M + u |stored value|; on the wide family also RTOL_GRAD of the tensor's
max-norm; the edge records of cl_frozen_rows, integers the layout fixes, exactly.  cl_det_reduce evaluates nothing: ref_step.sum_bound, the
bound of a DOUBLE sum, on dyadic inputs only, where every fp32 sum is exact (the result must equal the fp64 sum); the a-priori fp32 bound
n u sum |x| on floats (`det_bound`).

Two input families: `wide` (loc, iobs, z_f over decades, sig 1e-2 .. 1e3, sigma from 1e-3 loc to loc, 2 % exact zeros in loc, iobs, z_f; an
observation that a prediction happens to meet within 1 % is doubled: where a residual cancels, the entry's M is far above every entry of
the tensor and no fp32 evaluation holds the max-norm bar -- cancellation is the other family's subject, under the element-wise bound) and
`fitted` (iobs within three fp32 ulps of the fp64 prediction of sample 0 -- of every sample at S = 1).  In front of the calls that add with one
atomic per (row, sample) or per wave (the Laue calls, cl_slot_rows) dz_f and d_img hold a tenth of the entry's summand size (`lreference_for`
says why); cl_frozen_rows adds at most one atomic per run piece and keeps N(0, 1).

Cases: GPU_CASES (cl_frozen_rows: ROWS on ROW_LAYOUTS, GROUPS + SUMS on groups_layout), LGPU_CASES (the Laue calls and cl_slot_rows on rows in
the caller's order), DET_CASES (cl_det_reduce alone).  Emulations: emulate_rows, emulate_groups, emulate_laue, emulate_slot, emulate_det, each
with its wrong variants (`*_MUTANTS`).
"""
from __future__ import annotations

import ctypes
import math
from types import SimpleNamespace

import numpy as np
import torch

from oracle import elbo_oracle as O
from tests import ref_step
from tests.ref_q import host_lib, fp          # the host build of csrc/cl_math.h (tests/host_math_check.cpp)

F32 = np.float32
RTOL_LOSS, RTOL_GRAD = 1e-4, 2e-4            # tests/test_gpu_parity.py's (asserted equal in tests/test_ref_rows.py)
U = ref_step.U
SENT = -7.25e30                              # what an element holds before a call that STORES it
THROUGH = 1 << 30
FB, CAP = 256, 2048                          # rows of a chunk; CL_LAUE_LIK_MAX_BLOCKS
KINDS = {"normal": 0, "studentt": 1, "laplace": 2}
DOF = 7.5
EV11_RAW = (0.3, -1.2, -0.4)                 # raw Sdfac, Sdadd, SdB
OBS_OFFSET = 1000
N_BIG = CAP * FB + 3 * FB + 37               # above cl_frozen_grid's cap: some workgroup walks two chunks


def T(v):
    return torch.as_tensor(np.asarray(v, dtype=np.float64))


def lik_const(kind, dof):
    return F32(math.lgamma(0.5 * (dof + 1.0)) - math.lgamma(0.5 * dof) - 0.5 * math.log(dof * math.pi)) if kind == "studentt" else F32(0.0)


def frozen_grid(n):
    return max(1, min((n + FB - 1) // FB, CAP))


# ---- layouts ------------------------------------------------------------------------------------------------------------------------------
def runs_layout(runs, neg=0, skip=(), tail=0):
    """(refl_id ascending, R): `neg` leading rows of -1, then one run of equal reflections per entry of `runs`; the reflection numbers in `skip`
    have no rows, nor have the last `tail` reflections"""
    ids, r = [], 0
    for length in runs:
        while r in skip:
            r += 1
        ids.append(np.full(length, r, np.int32))
        r += 1
    return np.concatenate([np.full(neg, -1, np.int32)] + ids), r + tail


def random_runs(n, seed, hi=90):
    rng = np.random.default_rng([11, n, seed])
    runs, left = [], n
    while left > 0:
        k = int(min(left, rng.integers(1, hi)))
        runs.append(k)
        left -= k
    return runs


def big_runs():
    rng = np.random.default_rng(12)
    runs, left, big = [], N_BIG - 70000, False
    while left > 0:
        if not big and left < (N_BIG - 70000) // 2:
            runs.append(70000)
            big = True
        k = int(min(left, rng.integers(200, 400)))
        runs.append(k)
        left -= k
    return runs


ROW_LAYOUTS = {                       # name -> keyword arguments of runs_layout (rows_features names what each is there for)
    "ones": dict(runs=[1] * 70, tail=1),
    "lane63": dict(runs=[30, 34, 10]),                         # a run ends at lane 63, the next starts at lane 0: no chain
    "cross1": dict(runs=[50, 30, 5], skip=(1,)),               # a run crosses one wave border
    "through": dict(runs=[130, 250, 20], skip=(0, 2), tail=1),  # rows 130 .. 379: waves 3 and 4 are through-waves, across the chunk border at 256
    "lane0full": dict(runs=[20, 44, 84, 10]),                  # the third run starts at lane 0 of wave 1, fills it and goes on
    "back2back": dict(runs=[40, 60, 70, 10], tail=1),          # a chain ends mid-wave 1, the wave's last run starts the next one
    "raggedend": dict(runs=[60, 41]),                          # a chain that ends in the ragged last wave
    "R1": dict(runs=[257]),
    "negwave": dict(runs=[50, 30, 5], neg=64, tail=1),         # a whole wave of rows without a reflection
    "negmid": dict(runs=[50, 30], neg=20),                     # ... and their border mid-wave
    "n1": dict(runs=[1]),
    "n63": dict(runs=random_runs(63, 0, 30)),
    "n64": dict(runs=random_runs(64, 1, 30)),
    "n65": dict(runs=random_runs(65, 2, 30), tail=1),
    "n256": dict(runs=random_runs(256, 3)),
    "n257": dict(runs=random_runs(257, 4), skip=(2,)),
    "n641": dict(runs=random_runs(641, 5, 150), tail=1),
    "big": dict(runs=big_runs(), tail=1),
}


def wave_flags(refl_id):
    """The wave-border bookkeeping of frozen_rows_kernel from refl_id alone: per wave first_cp, last_cn, single, rec1 and the two edge_rid ints"""
    n = len(refl_id)
    W = (n + 63) // 64
    rid = np.full(W * 64, -1, np.int64)
    rid[:n] = refl_id
    rw = rid.reshape(W, 64)
    first, last = rw[:, 0], rw[:, 63]
    row0 = np.arange(W) * 64
    before = np.where(row0 > 0, rid[np.maximum(row0 - 1, 0)], -1)
    after = np.where(row0 + 64 < n, rid[np.minimum(row0 + 64, W * 64 - 1)], -1)
    first_cp = (first >= 0) & (first == before)
    last_cn = (last >= 0) & (last == after)
    single = first == last
    rec1 = last_cn & ~(single & first_cp)
    e0 = np.where(first_cp, first | np.where(single & last_cn, THROUGH, 0), -1)
    e1 = np.where(rec1, last, -1)
    return SimpleNamespace(W=W, rw=rw, first_cp=first_cp, last_cn=last_cn, single=single, rec1=rec1, e0=e0, e1=e1, after=after)


def rows_features(refl_id):
    """what a sorted layout places at the wave borders (names asserted over the case list in tests/test_ref_rows.py)"""
    n = len(refl_id)
    f = wave_flags(refl_id)
    out, W = set(), f.W
    rid = np.asarray(refl_id)
    runs = np.diff(np.flatnonzero(np.concatenate([[True], rid[1:] != rid[:-1], [True]])))
    if np.any(runs[rid[np.cumsum(runs) - 1] >= 0] == 1):
        out.add("run of one row")
    for w in range(W - 1):
        if f.rw[w, 63] >= 0 and not f.last_cn[w] and f.rw[w + 1, 0] >= 0:
            out.add("run ends at lane 63, next starts at lane 0")
    thr = f.first_cp & f.single & f.last_cn
    if f.last_cn.any():
        out.add("run crosses a wave border")
    for w in np.flatnonzero(thr):
        out.add("through-wave")
        if (w * 64) % FB == 0 or ((w + 1) * 64) % FB == 0:
            out.add("through-wave at a chunk border")
    if np.any(f.single & f.last_cn & ~f.first_cp):
        out.add("run starts at lane 0, fills its wave and goes on")
    if np.any(f.first_cp & ~f.single & f.rec1):
        out.add("two chains back to back")
    if n % 64 and f.first_cp[W - 1]:
        out.add("chain ends in the ragged last wave")
    if rid.min() >= 0 and rid.max() == 0 and n > 64:
        out.add("R = 1")
    neg = int(np.sum(rid < 0))
    if neg >= 64:
        out.add("a whole wave without a reflection")
    if neg % 64:
        out.add("refl_id < 0 ends mid-wave")
    if n > CAP * FB:
        out.add("above the grid cap")
    return out


GRANULE_PATTERNS = ([16], [5, 5, 3, 2], [3, 3, 3, 3, 3], [2] * 8, [1] * 16, [5, 1, 2], [16], [3, 5, 5], [1, 2, 3, 5])


def groups_layout(n2, seed):
    """Packed positions by the header's contract: groups of 1, 2, 3, 5 and 16 members, each inside a 16-row granule, padding positions with
    refl_id < 0; n2 active positions in all.  Returns (refl_id [n], gmeta [n], group start of every position [n] (-1 on padding), R)."""
    rng = np.random.default_rng([13, n2, seed])
    granules, total, k = [], 0, 0
    while total < n2:
        pat = list(GRANULE_PATTERNS[k % len(GRANULE_PATTERNS)])
        k += 1
        if total + sum(pat) > n2:
            pat = [1] * (n2 - total) if n2 - total <= 16 else [16]
        granules.append(pat)
        total += sum(pat)
    granules.insert(len(granules) // 2, [])                                   # a granule of padding alone
    n = 16 * len(granules)
    R = max(2, n2 // 90 + 3)                                                  # runs of ~90 rows in reflection order: chains and through-waves
    refl, gmeta, start = np.full(n, -1, np.int32), np.zeros(n, np.int32), np.full(n, -1, np.int64)
    for g, pat in enumerate(granules):
        p = 16 * g
        for size in pat:
            refl[p:p + size] = rng.choice(R - 1, size, replace=size > R - 1)      # (reflection R - 1 has no rows)
            gmeta[p:p + size] = np.arange(size) | (size << 8)
            start[p:p + size] = p
            p += size
    assert int(np.sum(refl >= 0)) == n2
    return refl, gmeta, start, R


# ---- cases --------------------------------------------------------------------------------------------------------------------------------
def case(entry, layout, S, family="wide", kind="normal", ev11=None, aim=True, key=True, accumulate=0, nll="atomic", ipred_out=False, src=True, seed=0):
    """One call (sequence).  entry: rows / groups; layout: a name of ROW_LAYOUTS, or n2 (groups); ev11: None / 'atomic' (d_ev11) / 'part'
    (ev11_part); aim, key, src: given or NULL; nll: 'atomic' (scalars) / 'part' (nll_part)."""
    assert not (kind == "laplace" and (ev11 or family == "fitted"))
    c = SimpleNamespace(entry=entry, layout=layout, S=S, family=family, kind=kind, ev11=ev11, aim=aim, key=key, accumulate=accumulate, nll=nll,
                        ipred_out=ipred_out, src=src, seed=seed)
    c.id = (f"{entry}-{layout}-S{S}-{family}-{kind}" + (f"-ev11{ev11}" if ev11 else "") + ("" if aim else "-noaim") + ("" if key else "-nokey") +
            ("-acc" if accumulate else "") + ("-nllpart" if nll == "part" else "") + ("-ipred" if ipred_out else "") + ("" if src else "-nosrc"))
    return c


def _draw(c, rng, n, R, S, rows_total):
    """the float operands of the wide family over n rows"""
    x = SimpleNamespace()
    x.loc = ref_step.decades(rng, n, -2, 2, zeros=0.02)
    x.sigma = (np.abs(x.loc.astype(np.float64)) * 10 ** rng.uniform(-3, 0, n) + (x.loc == 0) * 10 ** rng.uniform(-3, 0, n)).astype(F32)
    x.iobs = ref_step.decades(rng, n, -2, 5, zeros=0.02)
    x.sig = (10 ** rng.uniform(-2, 3, n)).astype(F32)
    x.z_f = ref_step.decades(rng, R * S, -1.5, 1.5, signed=False, zeros=0.02).reshape(R, S)
    x.aim = (10 ** rng.uniform(-0.5, 0.5, n)).astype(F32)
    x.eta = rng.standard_normal((rows_total, S)).astype(F32)
    return x


def make_inputs(c):
    """The operands of case c (seeded default_rng): a namespace of float32 / int32 arrays and the scalars of the argument block"""
    S = c.S
    if c.entry == "rows":
        refl, R = runs_layout(**ROW_LAYOUTS[c.layout])
        gmeta = start = None
    else:
        refl, gmeta, start, R = groups_layout(c.layout, c.seed)
    n = len(refl)
    rng = np.random.default_rng([21, n, S, KINDS[c.kind], c.seed, int(c.entry == "rows")])
    x = _draw(c, rng, n, R, S, n)
    x.case, x.entry, x.family, x.n, x.R, x.S, x.refl_id, x.gmeta, x.start = c, c.entry, c.family, n, R, S, refl, gmeta, start
    x.kind, x.dof, x.shift, x.w_ll = c.kind, F32(DOF), F32(0.37), F32(1.0 / S)
    x.lik_const = lik_const(c.kind, DOF)
    x.ev11 = np.array(EV11_RAW, F32) if c.ev11 else None
    x.image_id = x.img = None
    if not c.aim:
        x.aim = None
    x.obs_offset = OBS_OFFSET
    x.key = (OBS_OFFSET + rng.permutation(n)).astype(np.int32) if c.key else None
    x.krow = (x.key - OBS_OFFSET).astype(np.int64) if c.key else np.arange(n)            # a row's row of eta / ipred_out
    x.eta_row = x.eta[x.krow]
    x.act = refl >= 0
    if c.entry == "rows":
        x.slot, x.count = None, x.act.copy()
    else:
        x.slot = np.where(x.act, start, np.arange(n))                                   # the slot of a group: the position of its member 0
        x.count = x.act & ((gmeta & 0xff) == 0)
        x.iobs, x.sig = x.iobs[x.slot], x.sig[x.slot]                                   # replicated over the group
        act_pos = np.flatnonzero(x.act)
        order = act_pos[np.argsort(refl[act_pos], kind="stable")]                        # frozen.group_row_order: src, dst, refl_sorted
        x.n2, x.order, x.refl_sorted = len(order), order, refl[order].astype(np.int32)
        x.dst = np.full(n, -1, np.int32)
        x.dst[order] = np.arange(x.n2, dtype=np.int32)
    x.has_rows = np.bincount(refl[x.act], minlength=R) > 0
    x.dz_pre = rng.standard_normal((R, S)).astype(F32) if c.accumulate else np.full((R, S), SENT, F32)
    x.ev_pre = rng.standard_normal(3).astype(F32)
    x.nll_pre = 3.5
    ip = reference(x, values_only=True).iconv
    if c.family == "fitted":
        x.iobs = (ip[:, 0].astype(F32).astype(np.float64) * (1.0 + rng.integers(-3, 4, n) * 2.0 ** -23)).astype(F32)
    else:               # no ACCIDENTAL fit in the wide family (one in 10^2 .. 10^3 (row, sample) pairs is within 1 % otherwise): the fitted family's subject
        io = x.iobs.astype(np.float64)[:, None]
        x.iobs = np.where(np.any(np.abs(ip - io) < 1e-2 * (np.abs(ip) + np.abs(io)), axis=1), x.iobs * F32(2), x.iobs)
    if c.entry == "groups":
        x.iobs = x.iobs[x.slot]
    return x


# ---- the fp64 reference ---------------------------------------------------------------------------------------------------------------------
def _log_prob(kind, dof, v, io, sc):
    if kind == "normal":
        return O.normal_log_prob(v, io, sc)
    if kind == "studentt":
        return O.studentt_log_prob(v, float(dof), io, sc)
    return O.laplace_log_prob(v, io, sc)


def reference(x, values_only=False):
    """fp64 values and summand sizes (module docstring) of everything the four entry points write.  x: refl_id [n], image_id [n] + img [M - 1] or
    aim [n] or neither, slot [n] or None, count [n], loc, sigma, iobs, sig [n] (iobs / sig by SLOT), z_f [R][S], eta_row [n][S], kind, dof, shift,
    w_ll, ev11 [3] or None."""
    n, S, R = x.n, x.S, x.R
    rid = np.asarray(x.refl_id, np.int64)
    act = rid >= 0
    rc = torch.as_tensor(np.where(act, rid, 0))
    w, shift = float(x.w_ll), float(x.shift)
    loc, sigma, zf = T(x.loc).requires_grad_(True), T(x.sigma).requires_grad_(True), T(x.z_f).requires_grad_(True)
    leaves, names = [zf, loc, sigma], ["dz", "dloc", "dsigma"]
    if x.image_id is not None:
        img = T(x.img).requires_grad_(True)
        aim = O.image_scales(img)[torch.as_tensor(np.asarray(x.image_id, np.int64))]
        leaves, names = leaves + [img], names + ["d_img"]
    else:
        aim = T(x.aim) if x.aim is not None else torch.ones(n, dtype=torch.float64)
    eta = T(x.eta_row)
    tq = loc[:, None] + sigma[:, None] * eta + shift
    zr = zf[rc]
    ipred = aim[:, None] * tq * zr * zr * T(act)[:, None]
    slot = None if x.slot is None else torch.as_tensor(np.asarray(x.slot, np.int64))
    iconv = ipred if slot is None else O.laue_convolve(ipred.T, slot).T
    io, sg, cnt = T(x.iobs)[:, None], T(x.sig)[:, None], T(x.count)[:, None]
    if x.ev11 is not None:
        raw = T(x.ev11).requires_grad_(True)
        sd = torch.nn.functional.softplus(raw)
        sp = torch.nn.functional.softplus(iconv)
        sc = sd[0] * torch.sqrt(sg ** 2 + sd[2] * sp + sd[1] * sp * sp)
        leaves, names = leaves + [raw], names + ["d_ev11"]
    else:
        sc = sg.expand(n, S)
    ll = _log_prob(x.kind, x.dof, iconv, io, sc)
    nll = -(w * (ll * cnt).sum())
    out = SimpleNamespace(ipred=ipred.detach().numpy(), iconv=iconv.detach().numpy(), nll=float(nll.detach()))
    if values_only:
        return out
    g = dict(zip(names + ["dconv"], torch.autograd.grad(nll, leaves + [iconv], allow_unused=True)))
    g = {k: (v.numpy() if v is not None else None) for k, v in g.items()}
    out.dz, out.dconv, out.dO = g["dz"], g["dconv"], np.stack([g["dloc"], g["dsigma"]], 1)
    out.d_img, out.d_ev11 = g.get("d_img"), g.get("d_ev11")
    # summand sizes, in numpy from the values
    f = lambda t: t.detach().numpy()
    aim_, tq_, zr_, eta_, sc_, io_, cnt_ = f(aim)[:, None], f(tq), f(zr), f(eta), f(sc), f(io), f(cnt)
    a2 = act[:, None]
    absq = np.abs(x.loc.astype(np.float64))[:, None] + np.abs(x.sigma.astype(np.float64)[:, None] * eta_) + abs(shift)
    out.M_ipred = np.abs(aim_) * absq * zr_ * zr_ * a2
    sl = np.arange(n) if x.slot is None else np.asarray(x.slot, np.int64)
    out.M_iconv = np.zeros((n, S))
    np.add.at(out.M_iconv, sl, out.M_ipred)
    res = out.M_iconv + np.abs(io_)
    y = (out.iconv - io_) / sc_
    t = (float(x.dof) + 1.0) / (float(x.dof) + y * y) if x.kind == "studentt" else np.ones_like(y)
    Mx = math.sqrt(2.0) / sc_ if x.kind == "laplace" else t * res / sc_ ** 2
    Mdll = Mx
    if x.ev11 is not None:
        sd_, sp_ = f(sd), f(sp)
        rv = sc_ / sd_[0]
        Msc = (t * np.abs(y) * res / sc_ + 1.0) / sc_
        Mdll = Mx + Msc * sd_[0] * (sd_[2] + 2.0 * sd_[1] * sp_) * 0.5 / rv * 0.5 * (1.0 + np.tanh(0.5 * out.iconv))
        dsc = np.stack([rv, sd_[0] * sp_ * sp_ * 0.5 / rv, sd_[0] * sp_ * 0.5 / rv])                      # d sig / d(Sdfac, Sdadd, SdB): the raw order
        sgm = 1.0 / (1.0 + np.exp(-x.ev11.astype(np.float64)))
        out.M_ev11 = (w * cnt_ * Msc * dsc).sum((1, 2)) * sgm
    out.M_dconv = w * Mdll * cnt_
    Mrow = out.M_dconv[sl]
    out.M_gbuf = Mrow * np.abs(aim_ * tq_ * 2.0 * zr_) * a2
    out.gbuf = out.dconv[sl] * aim_ * tq_ * 2.0 * zr_ * a2
    out.M_dz = np.zeros((R, S))
    np.add.at(out.M_dz, np.where(act, rid, 0), out.M_gbuf)
    out.M_dO = np.stack([(Mrow * np.abs(aim_) * zr_ * zr_ * a2).sum(1), (Mrow * np.abs(aim_ * eta_) * zr_ * zr_ * a2).sum(1)], 1)
    if x.image_id is not None:
        out.M_img = np.zeros(len(x.img) + 1)
        np.add.at(out.M_img, np.asarray(x.image_id, np.int64), (Mrow * np.abs(tq_) * zr_ * zr_ * a2).sum(1))
        out.M_img = out.M_img[1:]
    const = {"normal": 0.5 * math.log(2.0 * math.pi), "studentt": abs(float(lik_const("studentt", float(x.dof)))), "laplace": 0.5 * math.log(2.0)}[x.kind]
    data = np.abs(f(ll) + np.log(sc_) + (const if x.kind != "studentt" else -float(lik_const("studentt", float(x.dof)))))
    out.M_nll = float((w * cnt_ * (data + np.abs(np.log(sc_)) + const + np.abs(out.dconv) / w * out.M_iconv)).sum())
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
    err, bound = np.asarray(err, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(err))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err > 0.0, err / bound, 0.0)
    q = np.where(np.isnan(err), np.inf, q)
    return float(np.max(q)) if q.size else 0.0


def _worst_grad(err, M, stored):
    """|error| <= RTOL_GRAD M + u |stored|, as the ratio of the error beyond the store's rounding to RTOL_GRAD M (ref_q._worst_grad)"""
    return _worst(np.maximum(np.abs(err) - U * np.abs(stored), 0.0), RTOL_GRAD * M)


def _grad(out, name, got, ref, M, pre, wide, sel=None):
    """one gradient tensor as STORED on top of `pre` (None: stored alone) into the ratios `out`"""
    got, ref, M = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(M, np.float64)
    stored = ref if pre is None else np.asarray(pre, np.float64) + ref
    err = np.abs(got - stored)
    if sel is not None:
        err, M, stored, ref = err[sel], M[sel], stored[sel], ref[sel]
    out[name] = _worst_grad(err, M, stored)
    if wide and err.size and np.max(np.abs(ref)) > 0.0:
        out[name + " max-norm"] = float(np.max(err) / np.max(np.abs(stored)) / RTOL_GRAD)


def rows_ratios(x, ref, got):
    """{quantity: largest error / bound} of a ROWS (or GROUPS + SUMS) result: got.dz (R, S) as stored, got.nll (the increment), optional got.ipred
    (rows of ipred_out, by caller row), got.d_ev11 (the increment's stored value on top of x.ev_pre, or the summed parts), got.gbuf (n2, S),
    got.edge_rid (the 2 ceil(n / 64) ints of the workspace after the call that sums the runs)."""
    wide, c = x.family == "wide", x.case
    out = {"nll": abs(got.nll - ref.nll) / (RTOL_LOSS * max(ref.M_nll, 1.0))}
    _grad(out, "dz_f", got.dz, ref.dz, ref.M_dz, x.dz_pre if c.accumulate else None, wide, sel=x.has_rows)
    if not c.accumulate and not np.array_equal(np.asarray(got.dz)[~x.has_rows].view(np.uint32), x.dz_pre[~x.has_rows].view(np.uint32)):
        out["dz_f"] = np.inf                                          # a reflection without rows keeps its bits
    if getattr(got, "ipred", None) is not None:
        rows = x.krow[x.act]
        out["ipred"] = _worst(np.abs(got.ipred[rows].astype(np.float64) - ref.ipred[x.act]), RTOL_LOSS * ref.M_ipred[x.act])
    if x.ev11 is not None:
        _grad(out, "d_ev11", got.d_ev11, ref.d_ev11, ref.M_ev11, x.ev_pre if c.ev11 == "atomic" else None, False)
    if getattr(got, "gbuf", None) is not None:
        _grad(out, "gbuf", got.gbuf, ref.gbuf[x.order], ref.M_gbuf[x.order], None, wide)
    if getattr(got, "edge_rid", None) is not None:
        # The edge records are integers the sorted layout fixes (csrc/elbo_frozen_rows.h: record 0 the first run's reflection where it continues
        # the previous wave's last one, with THROUGH where the wave is one run that goes on, else -1; record 1 the last run's reflection where it
        # STARTS in the wave and goes on, else -1): an exact bar.  A record that claims a chain where none is moves no total -- the edge launch
        # walks it and stores what the first launch would have -- but takes the store out of the launch that owns it.
        f = wave_flags(x.refl_id if x.entry == "rows" else x.refl_sorted)
        want = np.stack([f.e0, f.e1], 1).ravel()
        out["edge records"] = 0.0 if np.array_equal(np.asarray(got.edge_rid, np.int64), want) else np.inf
    return out


# ---- fp32 emulation: the likelihood forms -----------------------------------------------------------------------------------------------------
def _c(a, dt=F32):
    return np.ascontiguousarray(a, dtype=dt)


def lik32(hm, x, ip, io, sg, form):
    """(ll, dll, g_fac, g_add, g_b) of flat float32 arrays through the host build: form 3 = cl_lik_log_prob3 / cl_lik_laplace_log_prob2 (the
    frozen kernels), 1 = cl_lik_log_prob / cl_lik_laplace_log_prob (elbo_laue.hip); cl_lik_ev11 with an Evans-2011 triple"""
    ip, io, sg = _c(ip), _c(io), _c(sg)
    m = ip.size
    ll, dll = np.empty(m, F32), np.empty(m, F32)
    k, dof, lc = KINDS[x.kind], ctypes.c_float(float(x.dof)), ctypes.c_float(float(x.lik_const))
    if x.ev11 is not None:
        gf, gb, ga = np.empty(m, F32), np.empty(m, F32), np.empty(m, F32)
        hm.hm_lik_ev11(m, fp(ip), fp(io), fp(sg), k, dof, lc, fp(_c(x.ev11)), fp(ll), fp(dll), fp(gf), fp(gb), fp(ga))
        return ll, dll, gf, ga, gb
    if x.kind == "laplace":
        (hm.hm_lik_laplace2 if form == 3 else hm.hm_lik_laplace)(m, fp(ip), fp(io), fp(sg), fp(ll), fp(dll))
    else:
        (hm.hm_lik3 if form == 3 else hm.hm_lik)(m, fp(ip), fp(io), fp(sg), k, dof, lc, fp(ll), fp(dll))
    return ll, dll, None, None, None


def sigmoid32(hm, v):
    v, out = _c(v), np.empty(len(v), F32)
    hm.hm_sigmoid(len(v), fp(v), fp(out))
    return out


def butterfly(v, down=False):
    """the xor butterfly over the last axis (a power of two) in float32: what every lane holds after the steps.  Offsets 1, 2, 4, ... as the DPP
    sums take them (cl_wave_sum, cl_group_sum: a sum of two floats does not depend on their order, so the mirror and broadcast steps give the
    xor steps' values); down: the largest offset first, as the `for (off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off)` loops"""
    v = np.array(v, F32)
    lanes = np.arange(v.shape[-1])
    offs = [1 << k for k in range(int(v.shape[-1]).bit_length() - 1)]
    for off in (offs[::-1] if down else offs):
        v = v + v[..., lanes ^ off]
    return v


def suffix_runs(G, ids):
    """The six shuffle steps of the run totals: G (W, 64, ...) float32, ids (W, 64): a lane adds the lane `off` above it while that lane has
    the same id; the first lane of a run ends with the run's total."""
    G = np.array(G, F32)
    for k in range(6):
        off = 1 << k
        m = ids[:, :64 - off] == ids[:, off:]
        v = G[:, off:].copy()
        G[:, :64 - off] += np.where(m.reshape(m.shape + (1,) * (G.ndim - 2)), v, F32(0))
    return G


ROWS_MUTANTS = ("chain_stops_after_one_wave", "first_cp_ignored", "rid_after_at_lane_63", "rec1_total_to_dzf", "no_aim_in_dzf", "z_not_2z",
                "no_w_ll", "eta_by_sorted_position")
GROUPS_MUTANTS = ("every_member_counts_nll", "group_sum_over_gmax")


def _row_terms(x, hm, mutant=None, group=False):
    """per (row, sample) in float32: ipred, log p, the row's amplitude gradient g, and the Evans-2011 terms; frozen_rows_kernel /
    frozen_laue_body up to the sums"""
    n, S = x.n, x.S
    act = x.act
    rc = np.where(act, x.refl_id, 0)
    e = x.eta[np.arange(n)] if mutant == "eta_by_sorted_position" else x.eta_row
    e = np.where(act[:, None], e, F32(0))
    aim = x.aim if x.aim is not None else np.ones(n, F32)
    w = F32(1.0) if mutant == "no_w_ll" else x.w_ll
    tq = (x.loc[:, None] + x.sigma[:, None] * e) + x.shift
    zf = x.z_f[rc]
    ipred = np.where(act[:, None], ((aim[:, None] * tq) * zf) * zf, F32(0))
    lin = ipred
    if group:
        mem, cnt = (x.gmeta & 0xff), np.where(act, x.gmeta >> 8, 1)
        mem = np.where(act, mem, 0)
        W = (n + 63) // 64
        pad = np.zeros((W * 64, S), F32)
        pad[:n] = ipred
        pos = np.arange(n)
        cpad = np.ones(W * 64, np.int64)
        cpad[:n] = cnt
        gmax = cpad.reshape(W, 64).max(1)[pos // 64]
        lin = np.zeros((n, S), F32)
        for mm in range(16):
            v = pad[(pos // 64) * 64 + ((pos % 64 - mem + mm) & 63)]
            take = (mm < gmax) if mutant == "group_sum_over_gmax" else (mm < cnt)
            lin = lin + np.where(take[:, None], v, F32(0))
    rep = lambda a: np.repeat(a, S)
    ll, dll, gf, ga, gb = lik32(hm, x, lin.ravel(), rep(x.iobs), rep(x.sig), 3)
    ll, dll = ll.reshape(n, S), dll.reshape(n, S)
    g = (((-dll * w) * (F32(1) if mutant == "no_aim_in_dzf" else aim[:, None])) * tq) * (F32(1) if mutant == "z_not_2z" else F32(2)) * zf
    g = np.where(act[:, None], g, F32(0)).astype(F32)
    counted = act if (not group or mutant == "every_member_counts_nll") else x.count
    nll = float(-(ll.astype(np.float64)[counted] * float(w)).sum())
    ev = None
    if x.ev11 is not None:                                           # per thread over its samples, per wave (the butterfly), times sigmoid(raw), over the waves
        W = (n + 63) // 64
        acc = np.zeros((3, W * 64), F32)
        for s in range(S):
            for k, t in enumerate((gf, ga, gb)):
                acc[k, :n] = acc[k, :n] - np.where(counted, t.reshape(n, S)[:, s] * w, F32(0))
        wave = butterfly(acc.reshape(3, W, 64))[:, :, 63] * sigmoid32(hm, x.ev11)[:, None]
        ev = wave.astype(F32)                                        # (3, W): what ev11_part holds, wave by wave
    assert all(v.dtype == F32 for v in (tq, ipred, lin, g))
    return SimpleNamespace(ipred=ipred, g=g, nll=nll, ev=ev)


def sum_runs(refl_id, g, R, pre, accumulate, mutant=None):
    """frozen_rows_kernel's run totals and frozen_edges_kernel in float32: g (n, S) per sorted row -> dz (R, S) on top of `pre`"""
    n, S = g.shape
    f = wave_flags(refl_id)
    W = f.W
    G = np.zeros((W * 64, S), F32)
    G[:n] = g
    G = suffix_runs(G.reshape(W, 64, S), f.rw)
    if mutant == "rid_after_at_lane_63":                               # (rid_after = the wave's own last row)
        after = np.where(np.arange(W) * 64 + 64 < n, f.rw[:, 63], -1)
        f.last_cn = (f.rw[:, 63] >= 0) & (f.rw[:, 63] == after)
        f.rec1 = f.last_cn & ~(f.single & f.first_cp)
        f.e0 = np.where(f.first_cp, f.rw[:, 0] | np.where(f.single & f.last_cn, THROUGH, 0), -1)
        f.e1 = np.where(f.rec1, f.rw[:, 63], -1)
    if mutant == "first_cp_ignored":                                   # (every wave thinks its first run starts in it)
        f.first_cp = np.zeros(W, bool)
        f.rec1 = f.last_cn.copy()
        f.e0, f.e1 = np.full(W, -1), np.where(f.rec1, f.rw[:, 63], -1)
    first_cp, e0 = f.first_cp, f.e0
    lane = np.arange(64)[None, :]
    prev = np.concatenate([np.full((W, 1), -2), f.rw[:, :-1]], 1)
    head = (f.rw >= 0) & ((lane == 0) | (prev != f.rw))
    to_e0 = head & (lane == 0) & first_cp[:, None]
    to_e1 = head & ~to_e0 & (f.rw == f.rw[:, 63:64]) & f.rec1[:, None]
    dz = np.array(pre, F32)
    ev0, ev1 = np.zeros((W, S), F32), np.zeros((W, S), F32)             # (an edge record nobody wrote reads as 0 here; on the device it is stale)
    ev0[to_e0.any(1)] = G[to_e0]
    if mutant != "rec1_total_to_dzf":
        ev1[to_e1.any(1)] = G[to_e1]
        direct = head & ~to_e0 & ~to_e1
    else:
        direct = head & ~to_e0
    r_direct = f.rw[direct]
    if accumulate:
        np.add.at(dz, r_direct, G[direct])
    else:
        dz[r_direct] = G[direct]
    for w in np.flatnonzero(f.e1 >= 0):
        r, tot = int(f.e1[w]), ev1[w].copy()
        for j in range(w + 1, W):
            r0 = int(e0[j])
            if r0 < 0 or (r0 & ~THROUGH) != r:
                break
            tot = tot + ev0[j]
            if not (r0 & THROUGH) or mutant == "chain_stops_after_one_wave":
                break
        dz[r] = dz[r] + tot if accumulate else tot
    assert dz.dtype == F32
    return dz, np.stack([f.e0, f.e1], 1).ravel().astype(np.int32)          # ... and the 2 W ints the launch leaves in edge_rid


def emulate_rows(x, hm, mutant=None):
    """cl_frozen_rows, form ROWS, in numpy float32 in the kernel's order; returns what rows_ratios takes"""
    t = _row_terms(x, hm, mutant)
    dz, edge = sum_runs(x.refl_id, t.g, x.R, x.dz_pre, x.case.accumulate, mutant)
    ip = np.full((x.n, x.S), SENT, F32)
    ip[x.krow[x.act]] = t.ipred[x.act]
    return SimpleNamespace(dz=dz, nll=t.nll, ipred=ip, d_ev11=_ev_total(x, t.ev), edge_rid=edge)


def _ev_total(x, ev):
    if ev is None:
        return None
    tot = x.ev_pre.copy() if x.case.ev11 == "atomic" else np.zeros(3, F32)
    for w in range(ev.shape[1]):
        tot = tot + ev[:, w]
    return tot


def emulate_groups(x, hm, mutant=None):
    """cl_frozen_rows, form GROUPS then form SUMS: the group sums over the lanes, the likelihood on them, every row's gradient stored at
    gbuf[dst], then the run totals of gbuf in reflection order"""
    t = _row_terms(x, hm, mutant, group=True)
    gbuf = t.g[x.order]                                              # gbuf[dst[i]] = g[i]: row j of gbuf is position order[j]
    dz, edge = sum_runs(x.refl_sorted, gbuf, x.R, x.dz_pre, x.case.accumulate, mutant)
    ip = np.full((x.n, x.S), SENT, F32)
    ip[x.krow[x.act]] = t.ipred[x.act]
    return SimpleNamespace(dz=dz, nll=t.nll, ipred=ip, d_ev11=_ev_total(x, t.ev), gbuf=gbuf, edge_rid=edge)


# ---- cl_det_reduce ------------------------------------------------------------------------------------------------------------------------------
DET_MUTANTS = ("first_pass_only", "store_not_add")
DET_S = (1, 2, 3, 4, 5, 8, 9, 16, 17, 33)
DET_R = (1, 16, 17, 1100)
DET_NPARTS = (1, 63, 64, 65, 2048)
DET_NEV = (0, 4, 257)
DET_IMAGES = (1, 2, 6)
DET_REFL_ROWS = (0, 1, 15, 16, 17, 100)
DET_IMG_ROWS = (0, 63, 64, 65, 200)


def det_case(R, S, n_images, nparts, n_ev11, perm=True, dyadic=True, d_img=True):
    c = SimpleNamespace(R=R, S=S, n_images=n_images, nparts=nparts, n_ev11=n_ev11, perm=perm, dyadic=dyadic, d_img=d_img)
    c.id = f"det-R{R}-S{S}-M{n_images}-parts{nparts}-ev{n_ev11}" + ("" if perm else "-noperm") + ("" if dyadic else "-floats") + ("" if d_img else "-noimg")
    return c


def det_inputs(c):
    """Reflections of 0, 1, 15, 16, 17 and 100 rows (cycled), images of 0, 63, 64, 65 and 200 rows, every output preloaded.  dyadic: k / 64 with
    |k| <= 2^12, so that every fp32 sum of <= 2048 terms is exact in any order; else 10^U(-3, 3) with random signs."""
    rng = np.random.default_rng([31, c.R, c.S, c.n_images, c.nparts, c.n_ev11, int(c.perm), int(c.dyadic)])
    counts = np.array([DET_REFL_ROWS[(r + c.R) % len(DET_REFL_ROWS)] for r in range(c.R)])
    if c.R == 1:
        counts[:] = 100
    n = int(counts.sum())
    draw = (lambda *sh: (rng.integers(-4096, 4097, sh) / 64.0).astype(F32)) if c.dyadic else \
           (lambda *sh: (10 ** rng.uniform(-3, 3, sh) * rng.choice([-1.0, 1.0], sh)).astype(F32))
    x = SimpleNamespace(case=c, R=c.R, S=c.S, n=n, n_images=c.n_images, nparts=c.nparts, n_ev11=c.n_ev11)
    refl = np.repeat(np.arange(c.R), counts)
    x.seg_refl = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    if c.perm:                                                       # records in the caller's (shuffled) row order, perm_refl sorts them
        shuffle = rng.permutation(n)
        x.perm_refl = np.argsort(refl[shuffle], kind="stable").astype(np.int32)
    else:
        x.perm_refl = None
    x.dzf_obs = draw(max(n, 1), c.S)
    icounts = np.array([DET_IMG_ROWS[m % len(DET_IMG_ROWS)] for m in range(c.n_images)])
    icounts[0] = 7
    ni = int(icounts.sum())
    x.seg_img = np.concatenate([[0], np.cumsum(icounts)]).astype(np.int32)
    x.perm_img = rng.permutation(ni).astype(np.int32)
    x.dimg_obs = draw(max(ni, 1))
    x.nll_part = draw(c.nparts).astype(np.float64)
    x.ev11_part = draw(max(c.n_ev11, 1), 3)
    x.dz_pre, x.img_pre, x.ev_pre, x.nll_pre = draw(c.R, c.S), draw(max(c.n_images - 1, 1)), draw(3), float(draw(1)[0])
    return x


def det_reference(x):
    """fp64 sums and the sum of the summands' sizes (the preloaded value among them) of every output, and the number of terms"""
    S = x.S
    rec = x.dzf_obs.astype(np.float64)
    dz, Mdz, ndz = x.dz_pre.astype(np.float64).copy(), np.abs(x.dz_pre.astype(np.float64)), np.ones(x.R)
    for r in range(x.R):
        k = np.arange(x.seg_refl[r], x.seg_refl[r + 1])
        rows = x.perm_refl[k] if x.perm_refl is not None else k
        dz[r] += rec[rows].sum(0)
        Mdz[r] += np.abs(rec[rows]).sum(0)
        ndz[r] += len(k)
    out = SimpleNamespace(dz=dz, M_dz=Mdz, n_dz=np.repeat(ndz[:, None], S, 1))
    im = x.dimg_obs.astype(np.float64)
    out.d_img, out.M_img, out.n_img = x.img_pre.astype(np.float64).copy(), np.abs(x.img_pre.astype(np.float64)), np.ones(len(x.img_pre))
    for m in range(1, x.n_images):
        rows = x.perm_img[x.seg_img[m]:x.seg_img[m + 1]]
        out.d_img[m - 1] += im[rows].sum()
        out.M_img[m - 1] += np.abs(im[rows]).sum()
        out.n_img[m - 1] += len(rows)
    out.nll, out.M_nll = x.nll_pre + x.nll_part.sum(), abs(x.nll_pre) + np.abs(x.nll_part).sum()
    ev = x.ev11_part[:x.n_ev11].astype(np.float64)
    out.d_ev11, out.M_ev11 = x.ev_pre.astype(np.float64) + ev.sum(0), np.abs(x.ev_pre.astype(np.float64)) + np.abs(ev).sum(0)
    return out


def det_bound(x, n, total):
    # (ref_step.sum_bound bounds a DOUBLE sum and cl_det_reduce adds in fp32: it is right only where the fp32 sums are exact, the dyadic inputs)
    """ref_step.sum_bound on the dyadic inputs (every fp32 sum exact: the bound of a double sum holds), n u sum |x| on floats (Higham (4.4))"""
    return ref_step.sum_bound(n, total) if x.case.dyadic else np.asarray(n) * U * np.asarray(total)


def det_ratios(x, ref, got):
    out = {"dz_f": _worst(np.abs(got.dz.astype(np.float64) - ref.dz), det_bound(x, ref.n_dz, ref.M_dz)),
           "nll": abs(got.nll - ref.nll) / ref_step.sum_bound(x.nparts + 1, ref.M_nll)}
    if x.n_images > 1 and x.case.d_img:
        k = x.n_images - 1
        out["d_img"] = _worst(np.abs(got.d_img[:k].astype(np.float64) - ref.d_img[:k]), det_bound(x, ref.n_img[:k], ref.M_img[:k]))
    if x.n_ev11:
        out["d_ev11"] = _worst(np.abs(got.d_ev11.astype(np.float64) - ref.d_ev11), det_bound(x, x.n_ev11 + 1, ref.M_ev11))
    return out


def emulate_det(x, mutant=None):
    """det_refl_kernel / det_img_kernel / det_nll_kernel / det_ev11_kernel in float32 (the NLL in double), in their order of sums"""
    S, R = x.S, x.R
    Sp = 1 if S <= 1 else 2 if S <= 2 else 4 if S <= 4 else 8 if S <= 8 else 16
    nslot = 16 // Sp
    dz = x.dz_pre.copy()
    for r in range(R):
        k0, k1 = int(x.seg_refl[r]), int(x.seg_refl[r + 1])
        for s0 in range(0, S, 16):
            ns = min(Sp, S - s0)
            acc = np.zeros((nslot, Sp), F32)
            for slot in range(nslot):
                ks = np.arange(k0 + slot, k0 + slot + 1 if mutant == "first_pass_only" else k1, nslot)
                ks = ks[ks < k1]
                rows = x.perm_refl[ks] if x.perm_refl is not None else ks
                for row in rows:
                    acc[slot, :ns] = acc[slot, :ns] + x.dzf_obs[row, s0:s0 + ns]
            tot = butterfly(acc.T, down=True)[:, 0]                              # over the row slots (offsets 8 .. Sp of the 16 lanes)
            if mutant == "store_not_add":
                dz[r, s0:s0 + ns] = tot[:ns]
            else:
                dz[r, s0:s0 + ns] = dz[r, s0:s0 + ns] + tot[:ns]
    d_img = x.img_pre.copy()
    for m in range(1, x.n_images):
        acc = np.zeros(64, F32)
        rows = x.perm_img[x.seg_img[m]:x.seg_img[m + 1]]
        for j, row in enumerate(rows):
            acc[j % 64] = acc[j % 64] + x.dimg_obs[row]
        d_img[m - 1] = d_img[m - 1] + butterfly(acc, down=True)[0]
    acc = np.zeros(64)
    for k in range(x.nparts):
        acc[k % 64] += x.nll_part[k]
    off = 32
    while off:
        acc = acc + acc[np.arange(64) ^ off]
        off >>= 1
    ev = np.zeros((3, 64), F32)
    for k in range(x.n_ev11):
        ev[:, k % 64] = ev[:, k % 64] + x.ev11_part[k]
    d_ev = x.ev_pre + butterfly(ev, down=True)[:, 0]
    assert dz.dtype == F32 and d_img.dtype == F32 and d_ev.dtype == F32
    return SimpleNamespace(dz=dz, d_img=d_img, nll=x.nll_pre + acc[0], d_ev11=d_ev)


def _det_cases():
    out = []
    for k, S in enumerate(DET_S):                                    # every S at R = 17 and R = 1100 alternately, the other axes cycled
        out.append(det_case((17, 1100)[k % 2], S, DET_IMAGES[k % 3], DET_NPARTS[k % 5], DET_NEV[k % 3], perm=k % 2 == 0, dyadic=True, d_img=k % 4 != 3))
        out.append(det_case((1100, 17)[k % 2] if S <= 5 else 17, S, DET_IMAGES[(k + 1) % 3], DET_NPARTS[(k + 2) % 5], DET_NEV[(k + 1) % 3], perm=k % 2 == 1, dyadic=False))
    for k, R in enumerate(DET_R):
        out.append(det_case(R, (3, 8, 1, 5)[k], 6, DET_NPARTS[(k + 3) % 5], 257, perm=True, dyadic=k % 2 == 0))
    out.append(det_case(16, 4, 2, 2048, 4, perm=False, dyadic=True))
    out.append(det_case(17, 2, 6, 1, 0, perm=False, dyadic=False, d_img=False))
    seen, uniq = set(), []
    for c in out:
        if c.id not in seen:
            seen.add(c.id)
            uniq.append(c)
    return uniq


DET_CASES = _det_cases()


# ---- the cases of the GPU tests ------------------------------------------------------------------------------------------------------------------
ROWS_S = (1, 2, 8, 9, 13)
GROUPS_S = (1, 3, 9)
GROUPS_N2 = (64, 65, 641)


def _gpu_cases():
    r = lambda layout, S, **kw: case("rows", layout, S, **kw)
    out = [r("ones", 1), r("ones", 9, kind="studentt", nll="part"),
           r("lane63", 2, key=False), r("lane63", 8, family="fitted", accumulate=1),
           r("cross1", 8, aim=False), r("cross1", 1, kind="laplace", accumulate=1, nll="part"), r("cross1", 13, family="fitted", kind="studentt"),
           r("through", 1, kind="studentt", nll="part"), r("through", 9, accumulate=1, ev11="atomic"), r("through", 13, kind="laplace", ipred_out=True),
           r("through", 8, family="fitted", ev11="part", nll="part", key=False), r("through", 2, aim=False, ipred_out=True),
           r("lane0full", 8, kind="studentt", ev11="part", nll="part"), r("lane0full", 1, family="fitted"),
           r("back2back", 2, accumulate=1), r("back2back", 9, family="fitted", ipred_out=True), r("back2back", 1, kind="laplace", key=False),
           r("raggedend", 13, kind="studentt", ev11="atomic"), r("raggedend", 1, aim=False, key=False),
           r("R1", 1, family="fitted"), r("R1", 8, accumulate=1),
           r("negwave", 8, ipred_out=True), r("negwave", 1, kind="studentt", ev11="atomic"), r("negmid", 1, kind="laplace"), r("negmid", 9, nll="part"),
           r("n1", 1), r("n1", 13), r("n63", 2), r("n64", 8, kind="studentt"), r("n65", 9), r("n256", 1, nll="part"), r("n257", 13, accumulate=1),
           r("n641", 8, ev11="atomic"), r("n641", 1, family="fitted", kind="studentt"), r("n641", 2, kind="laplace", nll="part"),
           r("big", 1, nll="part"), r("big", 8, kind="studentt")]
    g = lambda n2, S, **kw: case("groups", n2, S, **kw)
    out += [g(64, 1), g(64, 9, src=False, kind="studentt"), g(65, 3, ev11="atomic"), g(65, 1, kind="laplace", src=False, accumulate=1),
            g(641, 9, family="fitted"), g(641, 3, kind="studentt", ev11="part", nll="part"), g(641, 1, aim=False, accumulate=1),
            g(641, 3, kind="laplace", ipred_out=True)]
    assert len({c.id for c in out}) == len(out)
    return out


GPU_CASES = _gpu_cases()


def emulate(x, hm, mutant=None):
    return (emulate_rows if x.entry == "rows" else emulate_groups)(x, hm, mutant)


# ---- cl_laue_predict / _likelihood / _backward and cl_slot_rows: rows in the caller's order ------------------------------------------------------
LAUE_S = (1, 3, 4, 5, 9, 64, 65)
SLOT_S = (1, 2, 4, 8, 16, 32, 64, 3, 5, 9, 65)
PAIRS_CAP = CAP * 256
LAUE_MUTANTS = ("padded_slots_not_counted", "harmonic_id_ignored_in_backward")
SLOT_MUTANTS = ("second_head_dO_dropped", "image_0_has_a_gradient", "no_lane_by_lane_tail", "det_slot_not_times_S")
DET_LEAD, DET_TAIL = 3, 5                    # records of dzf_obs in front of seg_refl[0] and behind seg_refl[R] that no observation owns (det_slot cases)


def lcase(entry, n, S, family="wide", kind="normal", ev11=None, img_run=0, dO=True, det=False, ipred_out=False, nll="atomic", det_slot=False):
    """entry: laue (the three calls) / slot (cl_slot_rows); img_run: rows per image (images 0, 1, 2, ... in row order; 0: use_img = 0); dO: given
    or NULL (cl_laue_backward); det: the deterministic mode of cl_slot_rows followed by cl_det_reduce -- det_slot NULL and perm_refl given, or
    (det_slot) det_slot[i] = the observation's position in reflection order and perm_refl NULL, the form the engine runs; ev11: None / 'atomic' /
    'part'"""
    assert not (kind == "laplace" and (ev11 or family == "fitted")) and not (det and 64 % S) and not (det_slot and not det)
    c = SimpleNamespace(entry=entry, n=n, S=S, family=family, kind=kind, ev11=ev11, img_run=img_run, dO=dO, det=det, ipred_out=ipred_out, nll=nll,
                        accumulate=1, layout=n, det_slot=det_slot)
    c.id = (f"{entry}-n{n}-S{S}-{family}-{kind}" + (f"-ev11{ev11}" if ev11 else "") + (f"-img{img_run}" if img_run else "-noimg") + ("" if dO else "-nodO") +
            ("-det" if det else "") + ("-detslot" if det_slot else "") + ("-ipred" if ipred_out else "") + ("-nllpart" if nll == "part" else ""))
    return c


def make_linputs(c):
    n, S = c.n, c.S
    rng = np.random.default_rng([22, n, S, KINDS[c.kind], c.img_run, int(c.entry == "laue")])
    R = max(2, min(n // 6 + 2, 4000))
    x = _draw(c, rng, n, R, S, n)
    x.case, x.entry, x.family, x.n, x.R, x.S = c, c.entry, c.family, n, R, S
    x.refl_id = rng.integers(0, R - 1, n).astype(np.int32)                             # (reflection R - 1 has no rows; every row has a reflection)
    x.kind, x.dof, x.shift, x.w_ll, x.lik_const = c.kind, F32(DOF), F32(0.37), F32(1.0 / S), lik_const(c.kind, DOF)
    x.ev11 = np.array(EV11_RAW, F32) if c.ev11 else None
    x.aim = None
    if c.img_run:
        x.image_id = (np.arange(n) // c.img_run).astype(np.int32)                      # image 0 present: its rows are pinned to scale 1
        x.img = (10 ** rng.uniform(-0.5, 0.5, int(x.image_id.max()) + 1)).astype(F32)   # (one more than the images with rows)
    else:
        x.image_id = x.img = None
    x.obs_offset, x.krow, x.eta_row, x.act = OBS_OFFSET, np.arange(n), x.eta, np.ones(n, bool)
    if c.entry == "laue":                                                             # groups of 1 .. 40 rows, unsorted; G < n: the slots G .. n - 1 are padded
        sizes, k = [], 0
        while sum(sizes) < n:
            sizes.append(min((1, 40, 2, 17, 5, 16, 33, 8)[k % 8], n - sum(sizes)))
            k += 1
        x.G = len(sizes)
        x.slot = np.repeat(rng.permutation(x.G), sizes)[rng.permutation(n)].astype(np.int32)
    else:
        x.slot, x.G = None, n
    x.count = np.ones(n, bool)
    x.has_rows = np.bincount(x.refl_id, minlength=R) > 0
    x.dz_pre, x.ev_pre, x.nll_pre = rng.standard_normal((R, S)).astype(F32), rng.standard_normal(3).astype(F32), 3.5
    x.img_pre = rng.standard_normal(len(x.img)).astype(F32) if c.img_run else None
    ip = reference(x, values_only=True).iconv
    if c.family == "fitted":
        x.iobs = (ip[:, 0].astype(F32).astype(np.float64) * (1.0 + rng.integers(-3, 4, n) * 2.0 ** -23)).astype(F32)
    else:
        io = x.iobs.astype(np.float64)[:, None]
        x.iobs = np.where(np.any(np.abs(ip - io) < 1e-2 * (np.abs(ip) + np.abs(io)), axis=1), x.iobs * F32(2), x.iobs)
    if c.det:                                                                         # cl_det_reduce's lists: observations by reflection / by image (stable)
        x.perm_refl = np.argsort(x.refl_id, kind="stable").astype(np.int32)
        x.seg_refl = np.concatenate([[0], np.cumsum(np.bincount(x.refl_id, minlength=R))]).astype(np.int32)
        x.det_slot = None
        if c.det_slot:      # records in reflection order between DET_LEAD and DET_TAIL records nobody owns; cl_det_reduce then reads them contiguously
            x.det_slot = np.empty(n, np.int32)
            x.det_slot[x.perm_refl] = DET_LEAD + np.arange(n, dtype=np.int32)
            x.seg_refl, x.perm_refl = (x.seg_refl + DET_LEAD).astype(np.int32), None
        im = x.image_id if c.img_run else np.zeros(n, np.int32)
        x.n_images = int(im.max()) + 2 if c.img_run else 1
        x.perm_img = np.argsort(im, kind="stable").astype(np.int32)
        x.seg_img = np.concatenate([[0], np.cumsum(np.bincount(im, minlength=x.n_images))]).astype(np.int32)
    return x


_LREFS = {}


def lreference_for(c):
    if c.id not in _LREFS:
        x = make_linputs(c)
        ref = reference(x)
        # What dz_f and d_img hold before calls that add with ONE ATOMIC PER (ROW, SAMPLE) or per wave: a tenth of the entry's summand size.  Every
        # atomic rounds at the size of the running total, so k atomics on top of a preloaded value p cost k u |p|, which the bound's one
        # rounding of the stored value does not cover when p is far above the entry's own summands; in a step dz_f holds zero or the prior's
        # term there.
        rng = np.random.default_rng([23, c.n, c.S])
        x.dz_pre = (0.1 * rng.standard_normal(ref.M_dz.shape) * ref.M_dz).astype(F32)
        if x.img is not None:
            x.img_pre = (0.1 * rng.standard_normal(ref.M_img.shape) * ref.M_img).astype(F32)
        _LREFS[c.id] = (x, ref)
    return _LREFS[c.id]


def laue_ratios(x, ref, got):
    """{quantity: largest error / bound}: got.iconv (after cl_laue_predict), got.dconv (dNLL / diconv in place, after cl_laue_likelihood), got.nll
    (the increment), got.dz / got.d_img as stored on top of the preloaded values, got.dO (stored), got.d_ev11, optional got.ipred"""
    wide, c = x.family == "wide", x.case
    out = {"nll": abs(got.nll - ref.nll) / (RTOL_LOSS * max(ref.M_nll, 1.0))}
    if getattr(got, "iconv", None) is not None:
        out["iconv"] = _worst(np.abs(got.iconv.astype(np.float64) - ref.iconv), RTOL_LOSS * ref.M_iconv)
    if getattr(got, "dconv", None) is not None:
        _grad(out, "dNLL/diconv", got.dconv, ref.dconv, ref.M_dconv, None, wide)
    if getattr(got, "ipred", None) is not None:
        out["ipred"] = _worst(np.abs(got.ipred.astype(np.float64) - ref.ipred), RTOL_LOSS * ref.M_ipred)
    _grad(out, "dz_f", got.dz, ref.dz, ref.M_dz, x.dz_pre, wide, sel=x.has_rows)
    same = (lambda a, b: np.array_equal(a, b)) if c.det else (lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32)))
    if not same(np.asarray(got.dz)[~x.has_rows], x.dz_pre[~x.has_rows]):                 # bit-unchanged (cl_det_reduce adds its zero: the value)
        out["dz_f"] = np.inf
    if c.dO:
        _grad(out, "dO", got.dO, ref.dO, ref.M_dO, None, wide)
        if c.img_run:
            _grad(out, "d_img", got.d_img, ref.d_img, ref.M_img, x.img_pre, wide)
    elif c.img_run and not np.array_equal(got.d_img.view(np.uint32), x.img_pre.view(np.uint32)):
        out["d_img"] = np.inf                                         # dO NULL: d_img keeps its bits
    if x.ev11 is not None:
        _grad(out, "d_ev11", got.d_ev11, ref.d_ev11, ref.M_ev11, x.ev_pre if (c.ev11 == "atomic" or c.det) else None, False)
    return out


def image_wave_sums(d_img, im, da, take, down, mutant=None):
    """The image-scale atomics of a launch, wave by wave: im, da, take (W, 64).  A wave whose taking lanes hold one image: one wave sum (down:
    the __shfl_xor loop of laue_backward_kernel; else cl_wave_sum); else cl_image_grad_segments: up to four images, one wave sum each in the
    order of their first lane, the rest lane by lane."""
    d_img = np.array(d_img, F32)
    W = im.shape[0]
    key = np.where(take, im, 0)
    kmax = key.max(1)
    kmin = np.where(take, im, np.iinfo(np.int32).max).min(1)
    one = take.any(1) & (kmin == kmax)
    v = butterfly(np.where(take, da, F32(0)), down=down)[:, 0]
    for w in np.flatnonzero(one):
        d_img[kmax[w] - 1] = d_img[kmax[w] - 1] + v[w]
    for w in np.flatnonzero(take.any(1) & ~one):
        t = take[w].copy()
        for _ in range(4):
            if not t.any():
                break
            m = im[w, np.argmax(t)]
            mine = t & (im[w] == m)
            d_img[m - 1] = d_img[m - 1] + butterfly(np.where(mine, da[w], F32(0)))[0]
            t &= ~mine
        if mutant != "no_lane_by_lane_tail":
            for lane in np.flatnonzero(t):
                d_img[im[w, lane] - 1] = d_img[im[w, lane] - 1] + da[w, lane]
    return d_img


def _pairs(x, mutant=None):
    """per (row, sample) in float32, flat in p = i S + s and padded to whole waves: what laue_predict / laue_backward / slot_rows compute alike"""
    n, S = x.n, x.S
    aim = np.ones(n, F32)
    if x.image_id is not None:
        aim = np.where(x.image_id > 0, x.img[np.maximum(x.image_id - 1, 0)], F32(1))
    tq = (x.loc[:, None] + x.sigma[:, None] * x.eta) + x.shift
    zf = x.z_f[x.refl_id]
    ipred = ((aim[:, None] * tq) * zf) * zf
    assert tq.dtype == F32 and ipred.dtype == F32
    return aim[:, None], tq, zf, ipred


def _waves(a, fill):
    a = np.asarray(a).ravel()
    W = (a.size + 63) // 64
    out = np.full(W * 64, fill, a.dtype)
    out[:a.size] = a
    return out.reshape(W, 64)


def _ev_waves(x, hm, gf, ga, gb, w):
    """the Evans-2011 terms of elbo_laue.hip: g -= gf w sigmoid(raw) per thread, the __shfl_xor butterfly per wave, the waves' shares"""
    sg = sigmoid32(hm, x.ev11)
    per = [butterfly(_waves(-((t * w) * sg[k]), F32(0)), down=True)[:, 0] for k, t in enumerate((gf, ga, gb))]
    return np.stack(per).astype(F32)


def _row_heads(x, i_flat, vals, straddle_mutant=False):
    """the segmented sums over the lanes of a row (suffix_runs) and the head lanes: (heads (W, 64) bool, sums (W, 64, k))"""
    ids = _waves(i_flat, -1)
    W = ids.shape[0]
    G = np.zeros((W * 64, vals.shape[1]), F32)
    G[:vals.shape[0]] = vals
    G = suffix_runs(G.reshape(W, 64, -1), ids)
    prev = np.concatenate([np.full((W, 1), -2), ids[:, :-1]], 1)
    head = (ids >= 0) & ((np.arange(64)[None, :] == 0) | (prev != ids))
    if straddle_mutant:                                              # a row that began in the previous wave: its second head adds nothing
        before = np.concatenate([[-2], ids[:-1, 63]])
        head &= ~((np.arange(64)[None, :] == 0) & (ids[:, 0] == before)[:, None])
    return ids, head, G


def emulate_laue(x, hm, mutant=None):
    """cl_laue_predict -> cl_laue_likelihood -> cl_laue_backward in float32; the atomics in row order"""
    n, S, c = x.n, x.S, x.case
    aim, tq, zf, ipred = _pairs(x)
    iconv = np.zeros((n, S), F32)
    np.add.at(iconv, x.slot, ipred)
    rep = lambda a: np.repeat(a, S)
    ll, dll, gf, ga, gb = lik32(hm, x, iconv.ravel(), rep(x.iobs), rep(x.sig), 1)
    counted = np.repeat(np.arange(n) < x.G, S) if mutant == "padded_slots_not_counted" else np.ones(n * S, bool)
    nll = float(-(ll.astype(np.float64)[counted] * float(x.w_ll)).sum())
    dconv = (-dll * x.w_ll).reshape(n, S)
    d_ev = None
    if x.ev11 is not None:
        ev = _ev_waves(x, hm, gf, ga, gb, x.w_ll)
        d_ev = x.ev_pre.copy() if c.ev11 == "atomic" else np.zeros(3, F32)
        for w in range(ev.shape[1]):
            d_ev = d_ev + ev[:, w]
    hid = np.arange(n) if mutant == "harmonic_id_ignored_in_backward" else x.slot
    gi = dconv[hid]
    dzs = (gi * zf) * zf
    dz = x.dz_pre.copy()
    np.add.at(dz, x.refl_id, (((gi * aim) * tq) * F32(2)) * zf)
    dt = dzs * aim
    out = SimpleNamespace(iconv=iconv, dconv=dconv, nll=nll, dz=dz, d_ev11=d_ev, ipred=ipred, dO=None, d_img=None if x.img is None else x.img_pre.copy())
    if c.dO:
        vals = np.stack([dt.ravel(), (dt * x.eta).ravel(), (dzs * tq).ravel()], 1)
        ids, head, G = _row_heads(x, np.repeat(np.arange(n), S), vals)
        dO = np.zeros((n, 2), F32)
        np.add.at(dO, ids[head], G[head][:, :2])
        out.dO = dO
        if x.img is not None:
            im = _waves(np.repeat(x.image_id, S), 0)
            out.d_img = image_wave_sums(x.img_pre, im, G[:, :, 2], head & (im > 0), down=True, mutant=mutant)
    return out


def emulate_slot(x, hm, mutant=None):
    """cl_slot_rows in float32: one pass per (row, sample), the row's sums by the path its S takes (the DPP group sum with stores for S = 1, 2,
    4, 8, 16; the shuffles with stores for 32 and 64; the shuffles with atomics onto a cleared dO otherwise).  det: what the deterministic mode
    stores for cl_det_reduce, then cl_det_reduce (emulate_det's order)."""
    n, S, c = x.n, x.S, x.case
    aim, tq, zf, ipred = _pairs(x)
    rep = lambda a: np.repeat(a, S)
    ll, dll, gf, ga, gb = lik32(hm, x, ipred.ravel(), rep(x.iobs), rep(x.sig), 1)
    nll = float(-(ll.astype(np.float64) * float(x.w_ll)).sum())
    gi = (-dll * x.w_ll).reshape(n, S)
    dzs = (gi * zf) * zf
    dzf = (((gi * aim) * tq) * F32(2)) * zf
    dt = dzs * aim
    vals = np.stack([dt.ravel(), (dt * x.eta).ravel(), (dzs * tq).ravel()], 1)
    store = 64 % S == 0
    if store and S <= 16:
        sums = butterfly(vals.reshape(n, S, 3).transpose(0, 2, 1))[:, :, 0]            # cl_group_sum over the S lanes of the row
        dO, da_row = sums[:, :2].copy(), sums[:, 2]
        ids = _waves(np.repeat(np.arange(n), S), -1)
        head = _waves(np.tile(np.arange(S) == 0, n), False)
        da = np.zeros(ids.shape, F32)
        da[head] = da_row
    else:
        ids, head, G = _row_heads(x, np.repeat(np.arange(n), S), vals, straddle_mutant=(mutant == "second_head_dO_dropped"))
        dO = np.zeros((n, 2), F32)
        if store:
            dO[ids[head]] = G[head][:, :2]
        else:
            np.add.at(dO, ids[head], G[head][:, :2])
        da = G[:, :, 2]
    out = SimpleNamespace(nll=nll, ipred=ipred, dO=dO, d_ev11=None, d_img=None if x.img is None else x.img_pre.copy())
    ev = _ev_waves(x, hm, gf, ga, gb, x.w_ll) if x.ev11 is not None else None
    if c.det:
        rec = dzf
        if x.det_slot is not None:                                    # dzf_obs[det_slot[i] * S + s], in the order of p = i S + s (a later store wins)
            rec = np.zeros((n + DET_LEAD + DET_TAIL) * S, F32)
            at = x.det_slot.astype(np.int64)[:, None] * (1 if mutant == "det_slot_not_times_S" else S) + np.arange(S)[None, :]
            rec[at.ravel()] = dzf.ravel()
            rec = rec.reshape(-1, S)
        d = SimpleNamespace(S=S, R=x.R, seg_refl=x.seg_refl, perm_refl=x.perm_refl, dzf_obs=rec, dz_pre=x.dz_pre, n_images=x.n_images, seg_img=x.seg_img,
                            perm_img=x.perm_img, dimg_obs=np.zeros(n, F32), img_pre=x.img_pre if x.img is not None else np.zeros(1, F32), nparts=1,
                            nll_part=np.array([nll]), nll_pre=x.nll_pre, n_ev11=0 if ev is None else ev.shape[1], ev11_part=None if ev is None else ev.T.copy(),
                            ev_pre=x.ev_pre)
        if x.img is not None:
            d.dimg_obs[ids[head]] = np.where(_waves(np.repeat(x.image_id, S), 0)[head] > 0, da[head], F32(0))
        r = emulate_det(d)
        out.dz, out.nll, out.d_ev11 = r.dz, r.nll - x.nll_pre, (r.d_ev11 if ev is not None else None)
        if x.img is not None:
            out.d_img = r.d_img
        return out
    dz = x.dz_pre.copy()
    np.add.at(dz, x.refl_id, dzf)
    out.dz = dz
    if ev is not None:
        out.d_ev11 = x.ev_pre.copy() if c.ev11 == "atomic" else np.zeros(3, F32)
        for w in range(ev.shape[1]):
            out.d_ev11 = out.d_ev11 + ev[:, w]
    if x.img is not None:
        im = _waves(np.repeat(x.image_id, S), 0)
        if mutant == "image_0_has_a_gradient":                        # (image 0's rows land in the first trainable scale)
            im = np.where(ids >= 0, np.maximum(im, 1), 0)
        out.d_img = image_wave_sums(x.img_pre, im, da, head & (im > 0), down=False, mutant=mutant)
    return out


def _lcases():
    L = lambda n, S, **kw: lcase("laue", n, S, **kw)
    out = [L(300, 1, img_run=8), L(300, 1, img_run=24, kind="studentt", ev11="atomic"), L(301, 3, img_run=40, ipred_out=True), L(257, 4, img_run=0),
           L(300, 5, img_run=30, dO=False), L(130, 9, img_run=1000, kind="laplace"), L(70, 64, img_run=3, family="fitted"), L(70, 65, img_run=2, kind="studentt"),
           L(300, 3, family="fitted", img_run=50, ev11="part", nll="part"), L(300, 9, img_run=8, dO=False, kind="studentt"),
           L(PAIRS_CAP // 4 + 28, 4, img_run=5000, nll="part")]
    s = lambda n, S, **kw: lcase("slot", n, S, **kw)
    out += [s(300, 1, img_run=8), s(300, 2, img_run=24, kind="studentt"), s(257, 4, img_run=0), s(300, 8, img_run=30, ev11="atomic", ipred_out=True),
            s(130, 16, img_run=2, kind="laplace"), s(70, 32, img_run=3), s(70, 64, img_run=1, family="fitted"), s(301, 3, img_run=9, kind="studentt", ev11="atomic"),
            s(300, 5, img_run=40, family="fitted"), s(130, 9, img_run=1000, kind="laplace", ipred_out=True), s(70, 65, img_run=2),
            s(PAIRS_CAP // 8 + 64, 8, img_run=5000, nll="part"), s(2 * PAIRS_CAP // 8 + 128, 8, img_run=7000, kind="studentt"),
            s(300, 1, img_run=8, det=True, nll="part"), s(300, 4, img_run=24, det=True, nll="part", kind="studentt", ev11="part"), s(257, 16, det=True, nll="part"),
            s(70, 64, img_run=3, det=True, nll="part", family="fitted"),
            s(300, 1, img_run=8, det=True, det_slot=True, nll="part"), s(301, 4, img_run=24, det=True, det_slot=True, nll="part", kind="studentt", ev11="part"),
            s(257, 16, det=True, det_slot=True, nll="part", family="fitted"), s(70, 64, img_run=3, det=True, det_slot=True, nll="part", kind="laplace"),
            s(2049 * 32, 8, img_run=5000, det=True, det_slot=True, nll="part")]
    assert len({c.id for c in out}) == len(out)
    return out


LGPU_CASES = _lcases()


def lemulate(x, hm, mutant=None):
    return (emulate_laue if x.entry == "laue" else emulate_slot)(x, hm, mutant)
