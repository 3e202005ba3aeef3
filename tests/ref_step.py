"""fp64 restatements of the optimizer half of the training step -- cl_grad_sqnorm, cl_owner_qnorm, cl_adam_step, cl_step_finalize
(csrc/elbo_step.hip) -- with an a-priori bound per element, the inputs of the direct kernel tests (tests/test_step_kernels.py), and the
guarded-buffer harness their device operands are carved from.

Written from the contract in include/careless_hip.h ("gradient norm, sanitise, clip, Adam") and the reference's
train_step_with_gradient_norm: norm of the raw gradients -> non-finite -> 0 -> clip -> tf_keras Adam.  Nothing here reads the kernel
text or calls oracle/elbo_oracle.py (tests/test_ref_step.py compares the two).  Every float of cl_adam_args (beta1, beta2, adam_eps,
alpha, the clip thresholds) enters as the float32 the struct carries, widened to fp64: 1 - beta is then exact in fp32 (Sterbenz) and the
reference tests the kernel, not the host's rounding of 0.999.

Order of the gradient's way into Adam: sanitise (non-finite -> 0) FIRST, then per-tensor clipnorm (g c / |t| only where |t| > c, |t| from
seg_sq), then global_clipnorm (g c / max(|g|, c), |g| from scalars[CL_SC_GNORM2_SANE]), then clipvalue.

The Adam bound.  u = 2^-24, tiny = 2^-126 (a subnormal fp32 result may flush), c1 = 1 - beta1, c2 = 1 - beta2:
    m' = m + (g - m) c1          b_m = u (2 |g - m| c1 + |m'|) + tiny               (subtract, multiply, add: the first two scaled by c1)
    v' = v + (g^2 - v) c2        b_v = u (3 g^2 c2 + 2 |v| c2 + |v'|) + tiny         (square, subtract, multiply, add)
    s  = m' alpha / (sqrt v' + eps): the interval of s over the four corners (m' +- b_m, max(v' +- b_v, 0)) -- s is monotone in both, and
         a derivative would blow up at v' -> 0, which is a real input -- plus 4 u |s| + tiny (multiply, root, add, divide)
    p' = p - s                   b_p = b_s + u |p'| + tiny
First order in u, valid for an fp32 evaluation with or without FMA contraction (a contraction only drops roundings).  A numpy fp32
evaluation reaches error / bound 0.99, 1.00, 1.00 (2e6 elements, 5 % exact zeros in each of g, m, v), so the GATE is twice these
expressions: room for the second-order terms, none for a wrong constant.  A norm-dependent clip multiplies g by a factor made of three
rounded operations (root -> float, divide, multiply): e_g = 3 u |g| per active mode, which enters b_m as e_g c1 and b_v as
2 |g| e_g c2.  clipvalue is exact.

The norm bound.  The square of a float is exact in double; a double sum of n non-negative terms in ANY order is within
(n - 1) 2^-53 of its exact value, relatively: (n + 8) 2^-53 * sum, the 8 for the block / wave / atomic combination steps, prior contents
and norm_extra.  References are long-double sums.  cl_owner_qnorm's four floats add u |sum| for the conversion.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
UD = 2.0 ** -53
GATE = 2.0
SC_NLL, SC_KL, SC_GNORM2, SC_GNORM2_SANE, SC_COUNT = 0, 1, 2, 3, 4
HIST_STRIDE = 8
F32 = np.float32


f64 = functools.partial(np.asarray, dtype=np.float64)        # numpy, where the oracle's f64 makes a tensor


# ---- launch shapes (quoted in tests/test_step_kernels.py) ------------------------------------------------------------------------------
def adam_grid(n, work=None, atomics=False):
    """workgroups of cl_adam_step: one per 1024 elements of work, at most 256 when the fused norm goes through atomics and n < 2^22, else 1024"""
    work = n if work is None else max(int(work), 1)
    cap = 1024 if (n >= (1 << 22) or not atomics) else 256
    return min((work + 1023) // 1024, cap)


def sqnorm_grid(n):
    return min((n + 255) // 256, 1024)


def owner_grid(nr):
    return max(1, min((2 * nr + 1023) // 1024, 64))


# ---- sums ---------------------------------------------------------------------------------------------------------------------------
def sumsq(x):
    """sum of squares of a float32 array beyond double precision (long double where it is wider than double, else math.fsum), as a float"""
    x = f64(x).ravel()
    sq = x * x                                                     # exact: 24-bit x 24-bit significands
    if np.finfo(np.longdouble).eps < 2.0 ** -60:
        return float(np.sum(sq.astype(np.longdouble)))
    return math.fsum(sq.tolist())


def sum_bound(n, total):
    return (n + 8) * UD * abs(total)


def norm_sums(x):
    """(class of the raw sum: 'nan' / 'inf' / 'finite', raw sum of the finite elements, sanitised sum, n) of a float32 array"""
    x = np.asarray(x, dtype=F32).ravel()
    fin = np.isfinite(x)
    cls = "finite" if fin.all() else ("nan" if np.isnan(x).any() else "inf")
    s = sumsq(np.where(fin, x, F32(0.0)))
    return cls, s, s, int(x.size)


def seg_index(seg_off, n):
    """tensor of every element: k with seg_off[k] <= i < seg_off[k + 1] (a zero-length tensor owns nothing)"""
    seg_off = np.asarray(seg_off, dtype=np.int64)
    assert seg_off[0] == 0 and seg_off[-1] == n and np.all(np.diff(seg_off) >= 0)
    return np.repeat(np.arange(len(seg_off) - 1), np.diff(seg_off))


def selection(n, ranges):
    """(indices a call updates, the number of the range each belongs to); no ranges: the whole vector"""
    if not ranges:
        return np.arange(n), np.zeros(n, dtype=np.int64)
    idx = np.concatenate([np.arange(b, e) for b, e in ranges]).astype(np.int64)
    rk = np.concatenate([np.full(e - b, k, dtype=np.int64) for k, (b, e) in enumerate(ranges)])
    return idx, rk


# ---- cl_grad_sqnorm ----------------------------------------------------------------------------------------------------------------
def grad_sqnorm(g, seg_off=None, frozen=None, want_seg=False):
    """what the call ADDS: raw / sanitised squared norm over the tensors that are not frozen, and per tensor (sanitised; a frozen
    tensor's slot is not touched).  Returns a namespace: cls, raw, sane, n, seg (values), seg_n (elements per tensor), seg_on (slots added to)"""
    g = np.asarray(g, dtype=F32)
    n = g.size
    on = np.ones(n, dtype=bool)
    if frozen is not None:
        on = np.asarray(frozen)[seg_index(seg_off, n)] == 0
    cls, raw, sane, cnt = norm_sums(g[on])
    out = SimpleNamespace(cls=cls, raw=raw, sane=sane, n=cnt, seg=None, seg_n=None, seg_on=None)
    if want_seg:
        nseg = len(seg_off) - 1
        out.seg, out.seg_n, out.seg_on = np.zeros(nseg), np.diff(np.asarray(seg_off, dtype=np.int64)), np.zeros(nseg, dtype=bool)
        for k in range(nseg):
            if out.seg_n[k] > 0 and (frozen is None or frozen[k] == 0):
                out.seg[k] = norm_sums(g[seg_off[k]:seg_off[k + 1]])[2]
                out.seg_on[k] = True
    return out


# ---- cl_owner_qnorm ----------------------------------------------------------------------------------------------------------------
def owner_qnorm(g, R, r0, r1):
    """{raw, sane, sane a, sane b} of g[r0:r1] and g[R + r0:R + r1]: cls, the four sums, n"""
    g = np.asarray(g, dtype=F32)
    a, b = g[r0:r1], g[R + r0:R + r1]
    cls, raw, _, _ = norm_sums(np.concatenate([a, b]))
    qa, qb = norm_sums(a)[2], norm_sums(b)[2]
    return SimpleNamespace(cls=cls, sums=np.array([raw, qa + qb, qa, qb]), n=2 * (r1 - r0))


# ---- sanitise, clip, Adam --------------------------------------------------------------------------------------------------------------
def sanitise(g):
    g = f64(g)
    return np.where(np.isfinite(g), g, 0.0)


def clip(g, seg=None, *, clipnorm=0.0, global_clipnorm=0.0, clipvalue=0.0, seg_sq=None, gnorm2_sane=None):
    """the SANITISED gradient through the clip modes in the contract's order; returns (g', rounded operations that scaled each element)"""
    x = f64(g)
    k = np.zeros(x.shape)
    if clipnorm > 0.0:
        nrm = np.sqrt(f64(seg_sq))[seg]
        hit = nrm > clipnorm
        x = np.where(hit, x * clipnorm / np.where(hit, nrm, 1.0), x)
        k = k + 3.0 * (hit | (np.abs(nrm - clipnorm) <= 4.0 * U * clipnorm))      # (a norm within a rounding of c: either branch, factor 1 - O(u))
    if global_clipnorm > 0.0:
        x = x * (global_clipnorm / max(math.sqrt(float(gnorm2_sane)), global_clipnorm))
        k = k + 3.0
    if clipvalue > 0.0:
        x = np.clip(x, -clipvalue, clipvalue)
    return x, k


def adam(p, g, m, v, kops, *, alpha, beta1, beta2, adam_eps):
    """tf_keras Adam.update_step on fp64 arrays (g already sanitised and clipped); returns {name: (value, bound)} for m, v, p"""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    c1, c2 = 1.0 - float(beta1), 1.0 - float(beta2)
    alpha, eps = float(alpha), float(adam_eps)
    m1 = m + (g - m) * c1
    v1 = v + (g * g - v) * c2
    eg = f64(kops) * U * np.abs(g)
    bm = U * (2.0 * np.abs(g - m) * c1 + np.abs(m1)) + eg * c1 + TINY
    bv = U * (3.0 * g * g * c2 + 2.0 * np.abs(v) * c2 + np.abs(v1)) + 2.0 * np.abs(g) * eg * c2 + TINY
    s = m1 * alpha / (np.sqrt(v1) + eps)
    bs = np.zeros_like(s)
    for mm in (m1 - bm, m1 + bm):
        for vv in (np.maximum(v1 - bv, 0.0), np.maximum(v1 + bv, 0.0)):
            np.maximum(bs, np.abs(mm * alpha / (np.sqrt(vv) + eps) - s), out=bs)
    bs += 4.0 * U * np.abs(s) + TINY
    p1 = p - s
    return {"m": (m1, bm), "v": (v1, bv), "p": (p1, bs + U * np.abs(p1) + TINY)}


def adam_step(c):
    """cl_adam_step on a case (adam_case below, or any namespace with its fields).  Returns a namespace:
    upd    [n] bool: elements the call updates (inside the ranges, tensor not frozen); everything else keeps its bits
    p, m, v  (value, bound) over all n elements; bound 0 and the input's value where not updated
    cls, raw, sane, n_norm   the fused norm's class and sums over the updated elements of ranges >= norm_skip_ranges, norm_extra included"""
    n = c.n
    idx, rk = selection(n, c.ranges)
    seg = None if c.seg_off is None else seg_index(c.seg_off, n)
    if c.frozen is not None:
        keep = np.asarray(c.frozen)[seg[idx]] == 0
        idx, rk = idx[keep], rk[keep]
    upd = np.zeros(n, dtype=bool)
    upd[idx] = True
    gs, kops = clip(sanitise(c.g[idx]), None if seg is None else seg[idx], clipnorm=float(c.clipnorm), global_clipnorm=float(c.global_clipnorm),
                    clipvalue=float(c.clipvalue), seg_sq=c.seg_sq, gnorm2_sane=None if c.scalars is None else c.scalars[SC_GNORM2_SANE])
    r = adam(c.p[idx], gs, c.m[idx], c.v[idx], kops, alpha=c.alpha, beta1=c.beta1, beta2=c.beta2, adam_eps=c.adam_eps)
    out = SimpleNamespace(upd=upd)
    for k, src in (("p", c.p), ("m", c.m), ("v", c.v)):
        val, bnd = f64(src).copy(), np.zeros(n)
        val[idx], bnd[idx] = r[k]
        setattr(out, k, (val, bnd))
    innorm = idx[rk >= c.norm_skip_ranges]
    out.cls, out.raw, out.sane, out.n_norm = norm_sums(c.g[innorm])
    if c.norm_extra is not None:
        ex = f64(c.norm_extra)
        out.raw, out.sane, out.n_norm = out.raw + ex[0], out.sane + ex[1], out.n_norm + 1
    return out


# ---- cl_step_finalize --------------------------------------------------------------------------------------------------------------
def finalize(scalars, klw, norm_part=None, flag=0):
    """(record[5], record bounds[5], scalars after, scalars bounds, flag after).  A raised flag: {0, 0, 0, 0, 1}, nothing else moves."""
    sc = f64(scalars).copy()
    bsc = np.zeros(SC_COUNT)
    if flag:
        return np.array([0.0, 0.0, 0.0, 0.0, 1.0]), np.zeros(5), sc, bsc, 1
    if norm_part is not None:
        part = f64(norm_part).reshape(-1, 2)
        for j, slot in ((0, SC_GNORM2), (1, SC_GNORM2_SANE)):
            col = part[:, j]
            fin = np.isfinite(col)
            add = float(np.sum(np.where(fin, col, 0.0).astype(np.longdouble))) if fin.all() else float(np.sum(col))
            bsc[slot] = (len(col) + 2) * UD * (abs(sc[slot]) + float(np.sum(np.abs(np.where(fin, col, 0.0)))))
            sc[slot] = sc[slot] + add
    nll, kl, gn2 = sc[SC_NLL], sc[SC_KL], sc[SC_GNORM2]
    klw = float(F32(klw))
    with np.errstate(invalid="ignore"):
        gn = math.sqrt(gn2) if gn2 >= 0.0 and math.isfinite(gn2) else (math.inf if gn2 == math.inf else math.nan)
    rec = np.array([nll + klw * kl, kl, nll, gn, 0.0])
    brec = np.zeros(5)
    brec[0] = 2.0 * UD * (abs(nll) + abs(klw * kl))
    if math.isfinite(gn) and gn > 0.0:
        brec[3] = UD * gn + 0.5 * bsc[SC_GNORM2] / gn
    return rec, brec, sc, bsc, int(not math.isfinite(gn))


# ---- comparison ----------------------------------------------------------------------------------------------------------------------
WORST = {}         # (entry point, output) -> largest error / bound seen (a record for the notebook, not a gate)


def outside(got, ref, bound, gate=1.0):
    """elements whose error exceeds gate * bound (a NaN counts as outside)"""
    err = np.abs(f64(got) - f64(ref))
    return ~(err <= gate * f64(bound))


def assert_within(got, ref, bound, what, entry, gate=1.0):
    got, ref, bound = np.atleast_1d(f64(got)), np.atleast_1d(f64(ref)), np.atleast_1d(f64(bound))
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0.0, err / bound, 0.0)
    worst = float(np.nanmax(ratio)) if ratio.size else 0.0
    bad = np.flatnonzero(outside(got, ref, bound, gate))
    assert bad.size == 0, (f"{entry}: {what}: {bad.size} of {err.size} elements outside {gate:g} x their bound, first at {bad[0]}: got {got[bad[0]]!r}, "
                           f"reference {ref[bad[0]]!r}, bound {bound[bad[0]]:.3g}; largest error / bound {worst:.3g}")
    key = (entry, what.split(":")[-1].strip())
    WORST[key] = max(WORST.get(key, 0.0), worst)
    return worst


def assert_norm(got, cls, ref, n, what, entry, prior=0.0, extra_rel=0.0):
    """a squared norm the device accumulated on top of `prior`: the class of a non-finite raw norm, else the double-sum bound"""
    got = float(got)
    if cls == "nan":
        assert math.isnan(got), f"{entry}: {what}: {got!r}, expected NaN"
    elif cls == "inf":
        assert got == math.inf, f"{entry}: {what}: {got!r}, expected +inf"
    else:
        assert math.isfinite(got), f"{entry}: {what}: {got!r}, expected a finite sum"
        tot = abs(prior) + abs(ref)
        assert_within(got, prior + ref, sum_bound(n, tot) + extra_rel * tot, what, entry)


def check_adam(c, ref, p, m, v, entry="cl_adam_step"):
    for k, got in (("m", m), ("v", v), ("p", p)):
        val, bnd = getattr(ref, k)
        assert np.all(np.isfinite(f64(got)[ref.upd])), f"{entry}: {c.name}: non-finite {k}"
        assert_within(got, val, bnd, f"{c.name}: {k}", entry, gate=GATE)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
LR, BETA1, BETA2, ADAM_EPS, T_STEP = 1e-3, F32(0.9), F32(0.999), F32(1e-7), 3
ALPHA = F32(LR * math.sqrt(1.0 - float(BETA2) ** T_STEP) / (1.0 - float(BETA1) ** T_STEP))     # the non-default step count t = 3


def decades(rng, n, lo, hi, signed=True, zeros=0.05):
    """10^U(lo, hi) with random signs and a fraction of exact zeros, as float32"""
    x = 10.0 ** rng.uniform(lo, hi, n)
    if signed:
        x = x * rng.choice([-1.0, 1.0], n)
    x[rng.random(n) < zeros] = 0.0
    return x.astype(F32)


def segments(n, nseg):
    """nseg tensor boundaries over n elements with a zero-length tensor and one-element tensors among them (n >= 2 nseg)"""
    sizes = np.ones(nseg, dtype=np.int64)
    sizes[1] = 0                                  # [1, 0, 1, ...]
    sizes[nseg // 2] = 0
    rest = n - int(sizes.sum())
    big = [k for k in range(nseg) if k % 3 == 0 and k not in (0, nseg - 1)]
    w = np.arange(1, len(big) + 1, dtype=np.float64)
    share = np.floor(rest * w / w.sum()).astype(np.int64)
    share[-1] += rest - int(share.sum())
    sizes[big] += share
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    assert off[-1] == n and sizes[0] == 1 and sizes[-1] == 1
    return off


NF = (F32(np.nan), F32(np.inf), F32(-np.inf))


def adam_case(name, n, seed=0, nseg=0, frozen=(), clip=None, some=True, nf=None, ranges=None, skip=0, extra=False, norm="atomic",
              nan_outside=False):
    """One call of cl_adam_step.  g, m over 10^-8 .. 10^4, v over 10^-16 .. 10^8, 5 % exact zeros each.
    frozen: tensor numbers (negative from the end) or 'allbut'; clip: 'clipnorm' / 'global' / 'value' or a '+'-joined pair, `some`: the threshold
    clips some tensors (elements) or none; nf: 'all' (NaN, +inf, -inf at the first and last element, both sides of a tensor boundary, inside a
    frozen tensor, outside the ranges), 'hidden' (only where they must not be seen), 'inf' (infinities only); norm: 'none' / 'atomic' / 'part'"""
    rng = np.random.default_rng(1000 + seed)
    c = SimpleNamespace(name=name, n=n, alpha=ALPHA, beta1=BETA1, beta2=BETA2, adam_eps=ADAM_EPS, clipnorm=F32(0), clipvalue=F32(0),
                        global_clipnorm=F32(0), seg_off=None, seg_sq=None, frozen=None, scalars=None, ranges=ranges, norm_skip_ranges=skip,
                        norm_extra=None, norm=norm)
    c.p = rng.standard_normal(n).astype(F32)
    c.g, c.m, c.v = decades(rng, n, -8, 4), decades(rng, n, -8, 4), decades(rng, n, -16, 8, signed=False)
    if nseg:
        c.seg_off = segments(n, nseg)
        sizes = np.diff(c.seg_off)
        if len(frozen) or frozen == "allbut":
            c.frozen = np.zeros(nseg, dtype=np.uint8)
            if frozen == "allbut":
                c.frozen[:] = 1
                c.frozen[int(np.argmax(sizes))] = 0
            else:
                c.frozen[list(frozen)] = 1
    idx, _ = selection(n, ranges)
    inr = np.zeros(n, dtype=bool)
    inr[idx] = True
    live = inr.copy()
    if c.frozen is not None:
        live &= c.frozen[seg_index(c.seg_off, n)] == 0
    if nf is not None:
        spots = []
        if nf in ("all", "inf"):
            lv = np.flatnonzero(live)
            spots += [lv[0], lv[-1]]
            if nseg:
                k = int(np.argmax(sizes * (np.arange(nseg) > 2)))          # both sides of the boundary in front of a large tensor
                spots += [c.seg_off[k] - 1, c.seg_off[k]]
        if nf in ("all", "hidden"):
            if c.frozen is not None:
                fz = np.flatnonzero(inr & ~live)
                spots += [fz[0], fz[len(fz) // 2], fz[-1]]
            out = np.flatnonzero(~inr)
            if out.size:
                spots += [out[0], out[len(out) // 2], out[-1]]
        for j, s in enumerate(spots):
            c.g[s] = NF[1 + j % 2] if nf == "inf" else NF[j % 3]
    if nan_outside:
        c.g[~inr] = np.nan
    if clip:
        on = grad_sqnorm(np.where(live, c.g, F32(0)), c.seg_off, c.frozen, want_seg=nseg > 0)
        c.scalars = np.array([3.5, -1.25, 0.0, on.sane])                 # what a cl_grad_sqnorm in front of the call leaves
        for mode in clip.split("+"):
            if mode == "clipnorm":
                c.seg_sq = on.seg.copy()
                order = np.argsort(on.seg)                                # between two tensors' norms, about half the ELEMENTS on each side
                k = int(np.searchsorted(np.cumsum(sizes[order]), 0.5 * sizes.sum()))
                nrm = np.sqrt(on.seg[order])
                c.clipnorm = F32(math.sqrt(nrm[k - 1] * nrm[k]) if some else 2.0 * nrm[-1])
            elif mode == "global":
                c.global_clipnorm = F32(math.sqrt(on.sane) * (0.37 if some else 2.0))
            else:
                a = np.abs(c.g[live & np.isfinite(c.g)])
                c.clipvalue = F32(np.median(a[a > 0]) if some else 2.0 * a.max())
    if extra:
        c.norm_extra = np.array([3.0e5, 2.5e5], dtype=F32) * F32(1 + rng.random())
    c.work = None if not ranges else sum(e - b for b, e in ranges)
    c.grid = adam_grid(n, c.work, atomics=(norm == "atomic"))
    return c


def owner_ranges(R, r0, r1, n):
    return [(r0, r1), (R + r0, R + r1), (2 * R, n)]


N_SMALL, NSEG = 5003, 45
N_TWO = 2 * 262144 + 1029          # two rounds and a ragged tail under the 256-workgroup cap
SIZES = ([(n, "atomic") for n in (1, 3, 255, 256, 257, 1023, 1024, 1025)] +
         [(n, "atomic") for n in (262144, 262145, N_TWO)] +
         [(n, r) for r in ("part", "none") for n in (1048576, 1048577, 2 * 1048576 + 517)] +
         [(n, "atomic") for n in ((1 << 22) - 1, 1 << 22, (1 << 22) + 1031)])


def _opts():
    """(id, keyword arguments of adam_case) of every option case: one small size (45 tensors) and one two-round size each"""
    o = []
    for tag, n in (("small", N_SMALL), ("two", N_TWO)):
        for mode in ("clipnorm", "global", "value"):
            for some in (True, False):
                o.append((f"{tag}-{mode}-{'some' if some else 'none'}", dict(n=n, nseg=NSEG, clip=mode, some=some, norm="none")))
        for fid, fz in (("first", (0,)), ("middle", (21,)), ("last", (-1,)), ("allbut", "allbut")):
            o.append((f"{tag}-frozen-{fid}", dict(n=n, nseg=NSEG, frozen=fz)))
        o.append((f"{tag}-nonfinite", dict(n=n, nseg=NSEG, frozen=(21, 30), nf="all")))
    for pair in ("clipnorm+global", "clipnorm+value", "global+value"):
        o.append((f"small-{pair}", dict(n=N_SMALL, nseg=NSEG, clip=pair, norm="none")))
    o.append(("small-clipnorm-frozen", dict(n=N_SMALL, nseg=NSEG, clip="clipnorm", frozen=(3, 21), norm="none")))
    o.append(("small-nonfinite-hidden", dict(n=N_SMALL, nseg=NSEG, frozen=(21, 30), nf="hidden")))
    o.append(("small-nonfinite-inf", dict(n=N_SMALL, nseg=NSEG, nf="inf")))
    o.append(("small-nonfinite-clipvalue", dict(n=N_SMALL, nseg=NSEG, nf="all", frozen=(21,), clip="value", norm="atomic")))
    # owner ranges [r0, r1), [R + r0, R + r1), [2R, n): R = 2000 and a replicated tail of 1003 (1000 / 1001 for the exact totals)
    R = 2000
    own = lambda r0, r1, n=N_SMALL, **kw: dict(n=n, ranges=owner_ranges(R, r0, r1, n), **{"nan_outside": True, "skip": 2, "extra": True, **kw})
    o += [("own-r0-0", own(0, 700)), ("own-r1-R", own(1300, R)), ("own-empty", own(900, 900)), ("own-one", own(777, 778)),
          ("own-midquad", own(5, 262)), ("own-1024", own(100, 112, n=5000)), ("own-1025", own(100, 112, n=5001)),
          ("own-skip0", own(301, 907, skip=0, extra=False)), ("own-skip3", own(301, 907, skip=3)), ("own-skip3-noextra", own(301, 907, skip=3, extra=False)),
          ("own-skip2-noextra", own(301, 907, extra=False)), ("own-part", own(301, 907, norm="part")), ("own-part-noextra", own(301, 907, norm="part", extra=False)),
          ("own-none", own(301, 907, norm="none")),
          ("own-frozen-segs", own(301, 907, nseg=NSEG, frozen=(21, -1), nf="all", nan_outside=False)),
          ("own-two", dict(n=2 * 250000 + 30001, ranges=owner_ranges(250000, 60001, 200001, 2 * 250000 + 30001), nan_outside=True, skip=2, extra=True)),
          ("own-two-part", dict(n=2 * 600000 + 10001, ranges=owner_ranges(600000, 40003, 560003, 2 * 600000 + 10001), nan_outside=True, skip=2, extra=True,
                                norm="part"))]
    # the zero-length tensors frozen, their neighbours not: an element at a doubled boundary belongs to the tensor behind it
    o.append(("small-frozen-empty", dict(n=N_SMALL, nseg=NSEG, frozen=(1, NSEG // 2))))
    return o


OPTS = _opts()


def adam_cases():
    """(id, thunk) of every cl_adam_step case of the GPU tests"""
    out = [(f"n{n}-{route}", (lambda n=n, route=route: adam_case(f"n{n}-{route}", n, seed=n % 1000, norm=route))) for n, route in SIZES]
    out += [(i, (lambda i=i, kw=kw, s=s: adam_case(i, seed=s, **kw))) for s, (i, kw) in enumerate(OPTS)]
    return out


SQNORM_SIZES = (1, 255, 257, 262144, 262145, 600001)
OWNER_LENGTHS = (1, 512, 513, 32768, 40001)


def sqnorm_case(n, seg=True, frozen=(), nf=None, seed=0):
    rng = np.random.default_rng(2000 + seed + n % 1000)
    c = SimpleNamespace(n=n, g=decades(rng, n, -8, 4), seg_off=None, frozen=None, nseg=0)
    nseg = NSEG if n >= 2 * NSEG else 1
    if seg or len(frozen):
        c.nseg, c.seg_off = nseg, (segments(n, nseg) if nseg > 1 else np.array([0, n], dtype=np.int32))
    if len(frozen):
        c.frozen = np.zeros(nseg, dtype=np.uint8)
        if frozen == "allbut":
            c.frozen[:] = 1
            c.frozen[int(np.argmax(np.diff(c.seg_off)))] = 0
        else:
            c.frozen[list(frozen)] = 1
    if nf is not None:
        live = np.ones(n, dtype=bool) if c.frozen is None else c.frozen[seg_index(c.seg_off, n)] == 0
        spots = []
        if nf in ("all", "inf"):
            lv = np.flatnonzero(live)
            k = int(np.argmax(np.diff(c.seg_off) * (np.arange(c.nseg) > 2))) if c.nseg > 3 else 0
            spots += [lv[0], lv[-1]] + ([c.seg_off[k] - 1, c.seg_off[k]] if k else [])
        if nf in ("all", "hidden") and c.frozen is not None:
            fz = np.flatnonzero(~live)
            spots += [fz[0], fz[len(fz) // 2], fz[-1]]
        for j, s in enumerate(spots):
            c.g[s] = NF[1 + j % 2] if nf == "inf" else NF[j % 3]
    return c


def owner_case(nr, nan_in=False, seed=0):
    """R reflections, the own range [r0, r0 + nr) with r0 > 0 and r1 < R, NaN everywhere outside both windows"""
    rng = np.random.default_rng(3000 + seed + nr % 1000)
    r0 = 37
    R = r0 + nr + 91
    n = 2 * R + 50
    c = SimpleNamespace(R=R, r0=r0, r1=r0 + nr, n=n, g=decades(rng, n, -8, 4))
    keep = np.zeros(n, dtype=bool)
    keep[r0:r0 + nr] = keep[R + r0:R + r0 + nr] = True
    c.g[~keep] = np.nan
    if nan_in:
        c.g[r0 + nr // 3] = np.nan
        c.g[R + r0 + (2 * nr) // 3] = np.inf
    return c


# ---- harness ---------------------------------------------------------------------------------------------------------------------------
GUARD_BYTES = 256
GUARD_BYTE = 0xCB                                  # 0xCBCBCBCB: -2.67e7 as a float, -1.9e55 as a double, -875836469 as an int
DTYPES = (np.float32, np.float64, np.int32, np.uint8)


class Guarded:
    """Typed operands (float32, float64, int32, uint8) of a call carved out of ONE byte allocation, each 16-byte aligned with 256 guard
    bytes of 0xCB in front of and behind it.  `add(name, data, writable)`: writable is False (an input), True, or a mask per element --
    the elements the contract lets the call write.  `verify` asserts that every byte outside them is what it was: guards, inputs, the
    elements of outputs the call must leave alone; `verify(untouched=True)` that NO byte changed (a raised stop flag, a refused call)."""

    def __init__(self, device):
        self.device, self.ops, self.size, self.base = device, {}, 0, None

    def add(self, name, data, writable=False):
        data = np.ascontiguousarray(data)
        assert data.dtype.type in DTYPES and name not in self.ops, (name, data.dtype)
        w = np.broadcast_to(np.asarray(writable, dtype=bool), data.shape).ravel()
        start = (self.size + GUARD_BYTES + 15) // 16 * 16
        self.ops[name] = dict(start=start, data=data, own=np.repeat(w, data.itemsize), nbytes=data.nbytes)
        self.size = start + data.nbytes + GUARD_BYTES
        return self

    def build(self):
        import torch
        img = np.full(self.size + 16, GUARD_BYTE, dtype=np.uint8)
        own = np.zeros(self.size + 16, dtype=bool)
        for o in self.ops.values():
            img[o["start"]:o["start"] + o["nbytes"]] = o["data"].reshape(-1).view(np.uint8)
            own[o["start"]:o["start"] + o["nbytes"]] = o["own"]
        self.img, self.own = img, own
        self.base = torch.from_numpy(img.copy()).to(self.device)
        return self

    def ptr(self, name):
        return None if name is None else self.base.data_ptr() + self.ops[name]["start"]

    def download(self):
        self.got = self.base.cpu().numpy()
        return self.got

    def get(self, name):
        o = self.ops[name]
        return self.got[o["start"]:o["start"] + o["nbytes"]].view(o["data"].dtype).reshape(o["data"].shape)

    def changed(self, name):
        """per element: do its bytes differ from what was uploaded"""
        o = self.ops[name]
        d = self.got[o["start"]:o["start"] + o["nbytes"]] != self.img[o["start"]:o["start"] + o["nbytes"]]
        return d.reshape(-1, o["data"].itemsize).any(axis=1).reshape(o["data"].shape)

    def verify(self, untouched=False):
        got = self.download()
        bad = np.flatnonzero((got != self.img) & (True if untouched else ~self.own))
        what = "bytes written although nothing may be" if untouched else "bytes outside what the call may write changed"
        assert bad.size == 0, f"{bad.size} {what}, first at byte {bad[0]} ({self._where(bad[0])})"
        return self

    def _where(self, at):
        for name, o in self.ops.items():
            if o["start"] - GUARD_BYTES <= at < o["start"] + o["nbytes"] + GUARD_BYTES:
                rel = at - o["start"]
                return f"{name}: element {rel // o['data'].itemsize}" if 0 <= rel < o["nbytes"] else f"guard band of {name}"
        return "between operands"
