"""The fp64 references of tests/ref_step.py checked on the CPU: against oracle/elbo_oracle.py (clip_grads, global_norm, the Adam update
of train_step) at 1e-12 with the same doubles for beta; a numpy fp32 evaluation of the contract inside every bound on the inputs of
the GPU cases (tests/test_step_kernels.py); every mutant of a named list outside; the guarded-buffer harness against a write to each
class of location the contract says is not written."""
import math

import numpy as np
import pytest
import torch

from oracle import elbo_oracle as O
from tests import ref_step as R

F32 = np.float32
T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))


def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))) <= 1e-12, float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


# ---- the references against the oracle ---------------------------------------------------------------------------------------------------
def tensors(c):
    return [(int(c.seg_off[k]), int(c.seg_off[k + 1])) for k in range(len(c.seg_off) - 1)]


@pytest.mark.parametrize("mode", [None, "clipnorm", "global", "value"])
@pytest.mark.parametrize("some", [True, False])
def test_references_equal_the_oracle(mode, some):
    c = R.adam_case("oracle", 700, seed=5, nseg=12, clip=mode, some=some, nf="all" if mode == "value" else None)
    cut = tensors(c)
    cfg = O.ElboConfig(learning_rate=R.LR, beta_1=float(c.beta1), beta_2=float(c.beta2), adam_epsilon=float(c.adam_eps),
                       clipnorm=float(c.clipnorm) or None, clipvalue=float(c.clipvalue) or None, global_clipnorm=float(c.global_clipnorm) or None)
    c.alpha = cfg.learning_rate * math.sqrt(1.0 - cfg.beta_2 ** R.T_STEP) / (1.0 - cfg.beta_1 ** R.T_STEP)      # the oracle's own double
    grads = [T(c.g[b:e]) for b, e in cut]
    ref = R.adam_step(c)
    if mode != "value":
        close(math.sqrt(ref.raw), float(O.global_norm(grads)))
        sq = R.grad_sqnorm(c.g, c.seg_off, None, want_seg=True)
        close(np.sqrt(sq.seg), [float(O.global_norm([g])) for g in grads])
        close(sq.raw, ref.raw)
    sane = [torch.where(torch.isfinite(g), g, torch.zeros_like(g)) for g in grads]
    clipped, _ = R.clip(R.sanitise(c.g), R.seg_index(c.seg_off, c.n), clipnorm=float(c.clipnorm), global_clipnorm=float(c.global_clipnorm),
                        clipvalue=float(c.clipvalue), seg_sq=c.seg_sq, gnorm2_sane=None if c.scalars is None else c.scalars[R.SC_GNORM2_SANE])
    oc = O.clip_grads(sane, cfg)
    close(clipped, np.concatenate([g.numpy() for g in oc]))
    if mode is not None:
        assert (not np.array_equal(clipped, R.sanitise(c.g))) == some       # the threshold clips something, or nothing
    ps = [T(c.p[b:e]).clone() for b, e in cut]
    st = O.AdamState([T(c.m[b:e]) for b, e in cut], [T(c.v[b:e]) for b, e in cut], R.T_STEP - 1)
    params = [torch.nn.Parameter(p) for p in ps]
    O.adam_apply(params, oc, st, cfg)
    assert st.t == R.T_STEP
    close(ref.m[0], np.concatenate([x.numpy() for x in st.m]))
    close(ref.v[0], np.concatenate([x.numpy() for x in st.v]))
    close(ref.p[0], np.concatenate([x.detach().numpy() for x in params]))


def test_finalize_reference():
    rec, brec, sc, bsc, flag = R.finalize([2.0, 3.0, 16.0, 4.0], 0.5, np.array([4.0, 1.0, 5.0, 2.0]), 0)
    assert rec.tolist() == [3.5, 3.0, 2.0, 5.0, 0.0] and sc.tolist() == [2.0, 3.0, 25.0, 7.0] and flag == 0
    assert R.finalize([2.0, 3.0, np.inf, 4.0], 1.0)[4] == 1 and math.isnan(R.finalize([2.0, 3.0, np.nan, 4.0], 1.0)[0][3])
    rec, _, sc, _, flag = R.finalize([2.0, 3.0, 16.0, 4.0], 1.0, np.array([4.0, 1.0]), 1)
    assert rec.tolist() == [0.0, 0.0, 0.0, 0.0, 1.0] and sc.tolist() == [2.0, 3.0, 16.0, 4.0] and flag == 1


def test_launch_shapes():
    assert [R.adam_grid(n, atomics=True) for n in (1, 1024, 1025, 262144, 262145, (1 << 22) - 1, 1 << 22)] == [1, 1, 2, 256, 256, 256, 1024]
    assert [R.adam_grid(n) for n in (262145, 1048576, 1048577)] == [257, 1024, 1024]
    assert R.adam_grid(5000, 0) == 1 and R.adam_grid(5000, 1025) == 2
    assert [R.sqnorm_grid(n) for n in (1, 257, 262144, 262145)] == [1, 2, 1024, 1024]
    assert [R.owner_grid(n) for n in (1, 512, 513, 32768, 40001)] == [1, 1, 2, 64, 64]
    off = R.segments(R.N_SMALL, R.NSEG)
    sizes = np.diff(off)
    assert (sizes == 0).sum() == 2 and (sizes == 1).sum() >= 3 and sizes[0] == 1 and sizes[-1] == 1
    assert R.seg_index(off, R.N_SMALL)[off[2]] == 2 and R.seg_index(off, R.N_SMALL)[off[3] - 1] == 2


# ---- a numpy fp32 evaluation of the contract, and its mutants ---------------------------------------------------------------------------
ARITHMETIC = ("eps_in_root", "beta2_host", "stale_m", "unclipped_g_in_v", "clipnorm_when_below")
COVERAGE = ("clip_before_sanitise", "skip_last", "twice", "frozen_elem", "norm_missing_sq", "norm_extra_twice")


def eval32(c, mutant=None):
    """cl_adam_step's contract in numpy float32 (norms in double).  Returns (p, m, v, raw, sane, elements the mutant touches)"""
    one = F32(1.0)
    idx, rk = R.selection(c.n, c.ranges)
    seg = None if c.seg_off is None else R.seg_index(c.seg_off, c.n)
    hot = np.zeros(0, dtype=np.int64)
    if c.frozen is not None:
        keep = c.frozen[seg[idx]] == 0
        if mutant == "frozen_elem":
            hot = idx[np.flatnonzero(~keep)[:1]]
            keep[np.flatnonzero(~keep)[0]] = True
        idx, rk = idx[keep], rk[keep]
    if mutant == "skip_last":
        hot, idx, rk = idx[-1:], idx[:-1], rk[:-1]
    g = c.g[idx]
    gn = g[rk >= c.norm_skip_ranges].astype(np.float64)
    if mutant == "norm_missing_sq":
        gn = np.delete(gn, np.flatnonzero(np.abs(gn) >= 1.0)[0])        # (an element below the sum's own rounding is invisible in double)
    raw, sane = float(np.sum(gn * gn)), float(np.sum(np.where(np.isfinite(gn), gn * gn, 0.0)))
    if c.norm_extra is not None:
        k = 2.0 if mutant == "norm_extra_twice" else 1.0
        raw, sane = raw + k * float(c.norm_extra[0]), sane + k * float(c.norm_extra[1])
    with np.errstate(invalid="ignore", over="ignore"):
        fin = lambda a: np.where(np.isfinite(a), a, F32(0.0))
        x = g if mutant == "clip_before_sanitise" else fin(g)
        if mutant == "clip_before_sanitise":
            hot = idx[np.isinf(g)]
        x0 = fin(g)
        if c.clipnorm > 0:
            nrm = np.sqrt(c.seg_sq).astype(F32)[seg[idx]]
            hit = (nrm > c.clipnorm) | (mutant == "clipnorm_when_below")
            x = np.where(hit, x * (c.clipnorm / np.where(nrm > 0, nrm, one)), x)
        if c.global_clipnorm > 0:
            x = x * (c.global_clipnorm / max(F32(math.sqrt(c.scalars[R.SC_GNORM2_SANE])), c.global_clipnorm))
        if c.clipvalue > 0:
            x = np.minimum(np.maximum(x, -c.clipvalue), c.clipvalue)
        x = fin(x)
    c1, c2 = one - c.beta1, (F32(0.001) if mutant == "beta2_host" else one - c.beta2)

    def update(p0, m0, v0, x, xv):
        m1 = m0 + (x - m0) * c1
        v1 = v0 + (xv * xv - v0) * c2
        den = np.sqrt(v1 + c.adam_eps) if mutant == "eps_in_root" else np.sqrt(v1) + c.adam_eps
        return p0 - (m0 if mutant == "stale_m" else m1) * c.alpha / den, m1, v1

    p1, m1, v1 = update(c.p[idx], c.m[idx], c.v[idx], x, x0 if mutant == "unclipped_g_in_v" else x)
    assert p1.dtype == m1.dtype == v1.dtype == F32
    if mutant == "twice":
        j = len(idx) // 2
        hot = idx[j:j + 1]
        p1[j], m1[j], v1[j] = update(p1[j], m1[j], v1[j], x[j], x[j])
    p, m, v = c.p.copy(), c.m.copy(), c.v.copy()
    p[idx], m[idx], v[idx] = p1, m1, v1
    return p, m, v, raw, sane, hot


def out_masks(c, ref, p, m, v):
    return {k: R.outside(got, *getattr(ref, k), gate=R.GATE) for k, got in (("p", p), ("m", m), ("v", v))}


def norms_inside(ref, raw, sane):
    ok = True
    for got, want, cls in ((raw, ref.raw, ref.cls), (sane, ref.sane, "finite")):
        if cls == "nan":
            ok &= math.isnan(got)
        elif cls == "inf":
            ok &= got == math.inf
        else:
            ok &= bool(abs(got - want) <= R.sum_bound(ref.n_norm, want))
    return ok


CASES = R.adam_cases()


@pytest.mark.parametrize("make", [m for _, m in CASES], ids=[i for i, _ in CASES])
def test_fp32_evaluation_inside_every_bound(make):
    c = make()
    ref = R.adam_step(c)
    p, m, v, raw, sane, _ = eval32(c)
    R.check_adam(c, ref, p, m, v, entry="numpy fp32")
    for k, src, got in (("p", c.p, p), ("m", c.m, m), ("v", c.v, v)):
        assert np.array_equal(got[~ref.upd].view(np.int32), src[~ref.upd].view(np.int32))
    assert norms_inside(ref, raw, sane) and math.isfinite(ref.sane)
    assert c.grid == R.adam_grid(c.n, c.work, c.norm == "atomic")


def case_of(name):
    return dict(CASES)[name]()


@pytest.mark.parametrize("mutant,name", [("eps_in_root", "n1025-atomic"), ("beta2_host", "n1025-atomic"), ("stale_m", "n1025-atomic"),
                                         ("eps_in_root", "small-frozen-middle"), ("beta2_host", "small-frozen-middle"), ("stale_m", "own-midquad"),
                                         ("unclipped_g_in_v", "small-clipnorm-some"), ("unclipped_g_in_v", "small-global-some"),
                                         ("unclipped_g_in_v", "small-value-some"), ("clipnorm_when_below", "small-clipnorm-some"),
                                         ("clipnorm_when_below", "small-clipnorm-none")])
def test_arithmetic_mutants_fall_outside(mutant, name):
    """more than 1 % of the elements of at least one output leave their gate"""
    assert mutant in ARITHMETIC
    c = case_of(name)
    ref = R.adam_step(c)
    p, m, v, *_ = eval32(c, mutant)
    frac = {k: float(np.mean(o[ref.upd])) for k, o in out_masks(c, ref, p, m, v).items()}
    assert max(frac.values()) > 0.01, frac


@pytest.mark.parametrize("mutant,name", [("clip_before_sanitise", "small-nonfinite-clipvalue"), ("skip_last", "n1025-atomic"), ("skip_last", "own-1025"),
                                         ("skip_last", "small-frozen-middle"), ("twice", "n1025-atomic"), ("twice", "own-midquad"),
                                         ("frozen_elem", "small-frozen-middle"), ("frozen_elem", "small-frozen-allbut")])
def test_coverage_mutants_fall_outside(mutant, name):
    """the single affected element (every affected one) leaves its gate in at least one of p, m, v"""
    assert mutant in COVERAGE
    c = case_of(name)
    ref = R.adam_step(c)
    p, m, v, _, _, hot = eval32(c, mutant)
    o = out_masks(c, ref, p, m, v)
    assert hot.size >= 1 and np.all(o["p"][hot] | o["m"][hot] | o["v"][hot]), (hot, [o[k][hot] for k in "pmv"])


@pytest.mark.parametrize("mutant,name", [("norm_missing_sq", "n1025-atomic"), ("norm_missing_sq", "n262145-atomic"), ("norm_missing_sq", "own-skip0"),
                                         ("norm_extra_twice", "own-midquad"), ("norm_extra_twice", "own-skip3"), ("norm_extra_twice", "own-two")])
def test_norm_mutants_fall_outside(mutant, name):
    assert mutant in COVERAGE
    c = case_of(name)
    ref = R.adam_step(c)
    _, _, _, raw, sane, _ = eval32(c, mutant)
    assert ref.cls == "finite"
    assert abs(raw - ref.raw) > R.sum_bound(ref.n_norm, ref.raw) and abs(sane - ref.sane) > R.sum_bound(ref.n_norm, ref.sane)
    assert norms_inside(ref, *eval32(c)[3:5])


def test_every_listed_mutant_is_exercised():
    import inspect
    src = inspect.getsource(eval32)
    assert all(f'"{m}"' in src for m in ARITHMETIC + COVERAGE)


def test_other_references_see_a_dropped_element():
    c = R.sqnorm_case(600001, frozen=(21,), nf="hidden")
    ref = R.grad_sqnorm(c.g, c.seg_off, c.frozen, want_seg=True)
    assert ref.cls == "finite" and not ref.seg_on[21] and not ref.seg_on[1] and ref.seg_on[0]
    live = np.flatnonzero((c.frozen[R.seg_index(c.seg_off, c.n)] == 0) & (np.abs(c.g) >= 1.0))
    g = c.g.astype(np.float64)
    full = float(np.sum(np.where(np.isfinite(g) & (c.frozen[R.seg_index(c.seg_off, c.n)] == 0), g * g, 0.0)))
    assert abs(full - ref.raw) <= R.sum_bound(ref.n, ref.raw)
    assert abs(full - g[live[0]] ** 2 - ref.raw) > R.sum_bound(ref.n, ref.raw)
    k = int(R.seg_index(c.seg_off, c.n)[live[0]])
    b, e = c.seg_off[k], c.seg_off[k + 1]
    assert abs(float(np.sum(g[b:e] ** 2)) - ref.seg[k]) <= R.sum_bound(ref.seg_n[k], ref.seg[k])
    assert abs(float(np.sum(g[b:e] ** 2)) - g[live[0]] ** 2 - ref.seg[k]) > R.sum_bound(ref.seg_n[k], ref.seg[k])
    o = R.owner_case(40001, nan_in=True)
    q = R.owner_qnorm(o.g, o.R, o.r0, o.r1)
    assert q.cls == "nan" and np.all(np.isfinite(q.sums)) and q.sums[1] == q.sums[2] + q.sums[3] and q.n == 80002
    assert R.owner_qnorm(R.owner_case(513).g, 513 + 128, 37, 550).cls == "finite"


# ---- the harness -------------------------------------------------------------------------------------------------------------------------
def test_guarded_buffers_see_what_they_must():
    """a write to each class of location the contract says is not written"""
    c = R.adam_case("harness", 600, nseg=12, frozen=(3,), ranges=[(10, 200), (310, 500), (520, 600)])
    ref = R.adam_step(c)
    hist = np.arange(3 * R.HIST_STRIDE, dtype=np.float64)
    rec = np.zeros((3, R.HIST_STRIDE), dtype=bool)
    rec[1, :5] = True
    seg_on = np.ones(12, dtype=bool)
    seg_on[3] = False

    def fresh():
        a = R.Guarded("cpu").add("p", c.p, ref.upd).add("g", c.g).add("m", c.m, ref.upd).add("v", c.v, ref.upd).add("seg_off", c.seg_off)
        a.add("frozen", c.frozen).add("seg_sq", np.ones(12), seg_on).add("scalars", np.array([1.0, 2.0, 3.0, 4.0]), [False, False, True, True])
        return a.add("history", hist.reshape(3, -1), rec).add("stop", np.zeros(1, np.int32), True).build()

    a = fresh()
    assert all(a.ptr(k) % 16 == 0 for k in a.ops) and a.ptr(None) is None
    a.verify().verify(untouched=True)
    frozen_el = int(np.flatnonzero(~ref.upd & (np.arange(600) >= 10) & (np.arange(600) < 200))[0])
    assert c.seg_off[3] <= frozen_el < c.seg_off[4]
    pokes = [("g", 4 * 17, "g: element 17"), ("p", 4 * 5, "p: element 5"), ("m", 4 * 250 + 3, "m: element 250"), ("v", 4 * 519, "v: element 519"),
             ("p", 4 * frozen_el, f"p: element {frozen_el}"), ("m", 4 * frozen_el, f"m: element {frozen_el}"), ("v", 4 * frozen_el + 1, f"v: element {frozen_el}"),
             ("seg_sq", 8 * 3, "seg_sq: element 3"), ("scalars", 8 * R.SC_NLL, "scalars: element 0"), ("scalars", 8 * R.SC_KL + 7, "scalars: element 1"),
             ("history", 8 * 2, "history: element 2"), ("history", 8 * (2 * R.HIST_STRIDE + 3), "history: element 19"),
             ("history", 8 * (R.HIST_STRIDE + 5), "history: element 13"), ("history", 8 * (R.HIST_STRIDE + 7), "history: element 15"),
             ("seg_off", 4 * 2, "seg_off: element 2"), ("frozen", 3, "frozen: element 3"),
             ("p", -1, "guard band of p"), ("v", 4 * 600, "guard band of v"), ("history", -R.GUARD_BYTES, "guard band of history"), ("stop", 4, "guard band of stop")]
    for name, byte, where in pokes:
        a = fresh()
        a.base[a.ops[name]["start"] + byte] ^= 0x10
        with pytest.raises(AssertionError, match=where):
            a.verify()
    a = fresh()                                                              # what the call may write passes, and is seen by `changed` and `untouched`
    first = int(np.flatnonzero(ref.upd)[0])
    a.base[a.ops["p"]["start"] + 4 * first] ^= 0x01
    a.base[a.ops["scalars"]["start"] + 8 * R.SC_GNORM2] ^= 0x01
    a.base[a.ops["history"]["start"] + 8 * (R.HIST_STRIDE + 4)] ^= 0x01
    a.base[a.ops["stop"]["start"]] = 1
    a.verify()
    assert np.flatnonzero(a.changed("p")).tolist() == [first] and a.changed("history")[1, 4] and a.changed("history").sum() == 1
    assert a.get("stop")[0] == 1 and a.get("history").shape == (3, R.HIST_STRIDE) and a.get("frozen").dtype == np.uint8
    with pytest.raises(AssertionError, match="written although nothing may be"):
        a.verify(untouched=True)
