"""The optimizer half of the training step -- cl_grad_sqnorm, cl_owner_qnorm, cl_adam_step, cl_step_finalize (csrc/elbo_step.hip) -- called
directly through careless_amd._lib, one call of one entry point per case, against the fp64 references of tests/ref_step.py at their
a-priori bounds, on operands carved from one guarded allocation (ref_step.Guarded: every byte the contract says is not written --
g, elements outside the ranges, frozen tensors, scalars[NLL, KL], the other history records and the record's three spare doubles, all
guard bands -- bit-identical after the call).

Shape -> grid, from the entry points in elbo_step.hip (workgroups of 256 threads):
  cl_adam_grid_of: `int grid = (work + 1023) / 1024;` (work = n, or the sum of the range lengths, at least 1),
      `const int cap = (a.n >= (1 << 22) || a.norm_out == nullptr || a.norm_part != nullptr) ? 1024 : 256; if (grid > cap) grid = cap;`
      the kernel then walks rounds of `U * stride` = 4 x grid x 256 elements: 262 144 per round at 256 workgroups (262 145 and
      2 x 262 144 + 1029 take a second / third round with a ragged tail), 1 048 576 at 1024 (norm_part, no fused norm, or n >= 2^22:
      2^22 - 1 runs 256 workgroups and 16 rounds, 2^22 runs 1024 and 4, 2^22 + 1031 a fifth ragged one).
  cl_launch_grad_sqnorm: `int grid = (n + 255) / 256; if (grid > 1024) grid = 1024;` then `i += gridDim.x * blockDim.x`: a second
      round above 262 144 elements (262 145: one element of it; 600 001: a third, ragged).
  cl_launch_owner_qnorm: `int grid = (2 * (r_end - r_begin) + 1023) / 1024; if (grid > 64) grid = 64; if (grid < 1) grid = 1;` over 2 nr
      work items: nr = 1, 512 -> 1 workgroup; 513 -> 2; 32 768 -> 64, one round of 4 per thread; 40 001 -> 64 capped, ragged.
      The last of the `grid` tickets (scratch[4]) converts.
  cl_launch_finalize: `dim3(1), dim3(64)`: lane l adds norm_part pairs l, l + 64, ... (n_norm_part = 63, 64, 65, 1024: no lane / every
      lane / one lane with a second pair / sixteen each).

No tolerance here is a tuned number: Adam outputs at twice the first-order bound ref_step derives (its docstring), double sums at
(n + 8) 2^-53 of the sum."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from careless_amd import _lib as L
from tests import ref_step as R

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")]

DEV = "cuda"
F32 = np.float32
PRIOR = np.array([3.5, -1.25, 7.0e3, 6.0e3])              # what the accumulators hold before the call: the kernels ADD
NORM_SLOTS = [False, False, True, True]
SENT = -7.25e30


def lib():
    return L.get_lib()


@pytest.fixture(scope="module", autouse=True)
def worst_ratios():
    """the largest error / bound per entry point and output of the run, printed for the notebook (pytest -s); not a gate"""
    yield
    for (entry, what), r in sorted(R.WORST.items()):
        print(f"\nlargest error / bound  {entry:18s} {what:10s} {r:.3f}", end="")


def finish(a, code, want, untouched):
    torch.cuda.synchronize()
    assert code == want, f"returned {code}, expected {want}"
    a.verify(untouched=untouched)


# ---- cl_adam_step ------------------------------------------------------------------------------------------------------------------------
def adam_arena(c, ref, stop=False):
    a = R.Guarded(DEV).add("p", c.p, ref.upd).add("g", c.g).add("m", c.m, ref.upd).add("v", c.v, ref.upd)
    for name in ("seg_off", "frozen", "seg_sq", "scalars", "norm_extra"):
        if getattr(c, name) is not None:
            a.add(name, getattr(c, name))
    if c.norm != "none":
        a.add("norm_out", PRIOR, NORM_SLOTS if c.norm == "atomic" else False)      # (norm_part given: norm_out is only a switch)
    if c.norm == "part":
        a.add("norm_part", np.full(2 * c.grid + 6, SENT), [True] * (2 * c.grid) + [False] * 6)
    return a.add("stop", np.array([1 if stop else 0], np.int32)).build()


def adam_args(a, c):
    A = L.AdamArgs()
    A.p, A.g, A.m, A.v, A.n = a.ptr("p"), a.ptr("g"), a.ptr("m"), a.ptr("v"), c.n
    A.alpha, A.beta1, A.beta2, A.adam_eps = float(c.alpha), float(c.beta1), float(c.beta2), float(c.adam_eps)
    A.clipnorm, A.clipvalue, A.global_clipnorm = float(c.clipnorm), float(c.clipvalue), float(c.global_clipnorm)
    ptr = lambda k: a.ptr(k) if k in a.ops else None
    A.seg_off, A.nseg = ptr("seg_off"), 0 if c.seg_off is None else len(c.seg_off) - 1
    A.seg_sq, A.frozen, A.scalars, A.stop_flag = ptr("seg_sq"), ptr("frozen"), ptr("scalars"), ptr("stop")
    A.norm_out, A.norm_extra, A.norm_part = ptr("norm_out"), ptr("norm_extra"), ptr("norm_part")
    A.n_ranges, A.norm_skip_ranges = len(c.ranges or ()), c.norm_skip_ranges
    for k, (b, e) in enumerate(c.ranges or ()):
        A.range_begin[k], A.range_end[k] = b, e
    return A


def check_norms(a, c, ref):
    if c.norm == "none":
        return
    if c.norm == "atomic":
        got, prior = a.get("norm_out"), PRIOR
    else:
        part = a.get("norm_part")[:2 * c.grid].reshape(-1, 2)
        assert a.changed("norm_part")[:2 * c.grid].all(), "a norm_part slot was not written"
        assert np.all(np.isfinite(part[:, 1]))
        got, prior = [0.0, 0.0, float(np.sum(part[:, 0])) if ref.cls != "finite" else math.fsum(part[:, 0]), math.fsum(part[:, 1])], np.zeros(4)
    R.assert_norm(got[R.SC_GNORM2], ref.cls, ref.raw, ref.n_norm, f"{c.name}: raw norm", "cl_adam_step", prior=prior[R.SC_GNORM2])
    R.assert_norm(got[R.SC_GNORM2_SANE], "finite", ref.sane, ref.n_norm, f"{c.name}: sane norm", "cl_adam_step", prior=prior[R.SC_GNORM2_SANE])


def run_adam(c, stop=False):
    ref = R.adam_step(c)
    a = adam_arena(c, ref, stop)
    A = adam_args(a, c)
    assert int(lib().cl_adam_grid(C.byref(A))) == c.grid == R.adam_grid(c.n, c.work, c.norm == "atomic")
    finish(a, int(lib().cl_adam_step(C.byref(A), None)), 0, stop)
    if stop:
        return
    R.check_adam(c, ref, a.get("p"), a.get("m"), a.get("v"))
    check_norms(a, c, ref)


ADAM = R.adam_cases()


@pytest.mark.parametrize("make", [m for _, m in ADAM], ids=[i for i, _ in ADAM])
def test_adam_step(make):
    """every size at which cl_adam_grid_of or the kernel's rounds change (module docstring), by each norm route; each clip mode, alone and
    in the pairs the call accepts; frozen tensors; non-finite gradients where they must and must not be seen; owner ranges"""
    run_adam(make())


@pytest.mark.parametrize("name", ["n1025-atomic", "small-nonfinite", "own-part", "small-clipnorm-some"])
def test_adam_step_raised_flag_writes_nothing(name):
    run_adam(dict(ADAM)[name](), stop=True)


def test_adam_norm_classes_of_the_cases():
    """the raw fused norm is NaN or inf exactly when a non-frozen in-range element is non-finite (the cases' own inputs, no device call)"""
    want = {"small-nonfinite": "nan", "two-nonfinite": "nan", "small-nonfinite-hidden": "finite", "small-nonfinite-inf": "inf", "own-frozen-segs": "nan",
            "own-midquad": "finite", "own-two": "finite"}
    for name, cls in want.items():
        c = dict(ADAM)[name]()
        assert R.adam_step(c).cls == cls, name
        assert not np.all(np.isfinite(c.g)), name


def test_adam_norm_part_sums_are_bit_identical():
    """two identical norm_part calls, each followed by cl_step_finalize: the header promises index order, so the same bits"""
    c = dict(ADAM)["n1048577-part"]()
    ref = R.adam_step(c)
    a = R.Guarded(DEV).add("p", c.p, True).add("g", c.g).add("m", c.m, True).add("v", c.v, True).add("norm_out", PRIOR)
    for k in "12":
        a.add("part" + k, np.full(2 * c.grid, SENT), True).add("scalars" + k, PRIOR, NORM_SLOTS).add("hist" + k, np.full(R.HIST_STRIDE, SENT), [True] * 5 + [False] * 3)
    a.add("stop", np.zeros(1, np.int32), True).add("norm_part", np.zeros(2)).build()
    A = adam_args(a, c)
    for k in "12":
        A.norm_part = a.ptr("part" + k)
        assert int(lib().cl_adam_step(C.byref(A), None)) == 0
        assert int(lib().cl_step_finalize(a.ptr("scalars" + k), 1.0, a.ptr("hist" + k), 0, a.ptr("stop"), a.ptr("part" + k), c.grid, None)) == 0
    torch.cuda.synchronize()
    a.verify()
    for k in ("part", "scalars", "hist"):
        assert a.get(k + "1").tobytes() == a.get(k + "2").tobytes(), k
    assert a.changed("part1").all() and a.get("stop")[0] == 0
    R.assert_norm(a.get("scalars1")[R.SC_GNORM2], "finite", ref.raw, ref.n_norm + c.grid, "bit-identical: raw norm", "cl_step_finalize", prior=PRIOR[R.SC_GNORM2])


def small_case(**kw):
    return R.adam_case("refused", R.N_SMALL, nseg=R.NSEG, **kw)


def own3(n=R.N_SMALL):
    return R.owner_ranges(2000, 301, 907, n)


REFUSED = {
    "null-p": (dict(), lambda A: setattr(A, "p", None)), "null-g": (dict(), lambda A: setattr(A, "g", None)),
    "null-m": (dict(), lambda A: setattr(A, "m", None)), "null-v": (dict(), lambda A: setattr(A, "v", None)),
    "n-0": (dict(), lambda A: setattr(A, "n", 0)),
    "frozen-no-seg_off": (dict(frozen=(3,)), lambda A: setattr(A, "seg_off", None)), "frozen-nseg-0": (dict(frozen=(3,)), lambda A: setattr(A, "nseg", 0)),
    "clipnorm-no-seg_off": (dict(clip="clipnorm"), lambda A: setattr(A, "seg_off", None)),
    "clipnorm-no-seg_sq": (dict(clip="clipnorm"), lambda A: setattr(A, "seg_sq", None)),
    "global-no-scalars": (dict(clip="global"), lambda A: setattr(A, "scalars", None)),
    "n_ranges-4": (dict(ranges=own3()), lambda A: setattr(A, "n_ranges", 4)), "n_ranges-neg": (dict(ranges=own3()), lambda A: setattr(A, "n_ranges", -1)),
    "skip-neg": (dict(ranges=own3()), lambda A: setattr(A, "norm_skip_ranges", -1)),
    "skip-beyond-ranges": (dict(ranges=own3()[:2], skip=2), lambda A: setattr(A, "norm_skip_ranges", 3)),
    "skip-without-ranges": (dict(), lambda A: setattr(A, "norm_skip_ranges", 1)),
    "range-begin-neg": (dict(ranges=own3()), lambda A: A.range_begin.__setitem__(0, -1)),
    "range-end-beyond-n": (dict(ranges=own3()), lambda A: A.range_end.__setitem__(2, R.N_SMALL + 1)),
    "range-inverted": (dict(ranges=own3()), lambda A: (A.range_begin.__setitem__(1, 2907), A.range_end.__setitem__(1, 2906))),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_adam_step_refuses(name):
    """elbo_step.hip's entry checks: -1 and not a byte written"""
    kw, spoil = REFUSED[name]
    c = small_case(**kw)
    a = adam_arena(c, R.adam_step(c))
    A = adam_args(a, c)
    spoil(A)
    finish(a, int(lib().cl_adam_step(C.byref(A), None)), -1, True)


def test_null_argument_blocks_are_refused():
    assert int(lib().cl_adam_step(None, None)) == -1 and int(lib().cl_adam_grid(None)) == -1


# ---- cl_grad_sqnorm ----------------------------------------------------------------------------------------------------------------------
def run_sqnorm(c, seg, stop=False, spoil=None):
    ref = R.grad_sqnorm(c.g, c.seg_off, c.frozen, want_seg=seg)
    a = R.Guarded(DEV).add("g", c.g).add("scalars", PRIOR, NORM_SLOTS)
    if c.seg_off is not None:
        a.add("seg_off", c.seg_off)
    if c.frozen is not None:
        a.add("frozen", c.frozen)
    prior = 1.0 + 0.5 * np.arange(max(c.nseg, 1))
    if seg:
        a.add("seg_sq", prior, ref.seg_on)                              # a frozen (or empty) tensor's slot is not touched
    a.add("stop", np.array([1 if stop else 0], np.int32)).build()
    ptr = lambda k: a.ptr(k) if k in a.ops else None
    args = [a.ptr("g"), c.n, ptr("seg_off"), c.nseg, ptr("seg_sq"), a.ptr("scalars"), ptr("frozen"), a.ptr("stop"), None]
    if spoil is not None:
        args[spoil[0]] = spoil[1]
    finish(a, int(lib().cl_grad_sqnorm(*args)), -1 if spoil else 0, stop or spoil is not None)
    if stop or spoil:
        return
    what = f"n {c.n}"
    got = a.get("scalars")
    R.assert_norm(got[R.SC_GNORM2], ref.cls, ref.raw, ref.n, f"{what}: raw norm", "cl_grad_sqnorm", prior=PRIOR[R.SC_GNORM2])
    R.assert_norm(got[R.SC_GNORM2_SANE], "finite", ref.sane, ref.n, f"{what}: sane norm", "cl_grad_sqnorm", prior=PRIOR[R.SC_GNORM2_SANE])
    if seg:
        tot = prior + ref.seg
        R.assert_within(a.get("seg_sq"), tot, (ref.seg_n + 8) * R.UD * tot, f"{what}: seg_sq", "cl_grad_sqnorm")


@pytest.mark.parametrize("seg", [0, 1])
@pytest.mark.parametrize("n", R.SQNORM_SIZES)
def test_grad_sqnorm_sizes(n, seg):
    assert R.sqnorm_grid(n) == min((n + 255) // 256, 1024)
    run_sqnorm(R.sqnorm_case(n, seg=bool(seg)), bool(seg))


@pytest.mark.parametrize("n", [R.N_SMALL, 600001])
@pytest.mark.parametrize("frozen", [(0,), (21,), (-1,), "allbut", (1, R.NSEG // 2)], ids=["first", "middle", "last", "allbut", "empty"])
def test_grad_sqnorm_frozen(n, frozen):
    run_sqnorm(R.sqnorm_case(n, frozen=frozen), True)


@pytest.mark.parametrize("n", [R.N_SMALL, 600001])
@pytest.mark.parametrize("nf,cls", [("all", "nan"), ("hidden", "finite"), ("inf", "inf")])
def test_grad_sqnorm_nonfinite(n, nf, cls):
    """NaN, +inf, -inf at the first and last element and both sides of a tensor boundary reach the raw norm alone; inside a frozen tensor, neither"""
    c = R.sqnorm_case(n, frozen=(21, 30), nf=nf)
    assert R.grad_sqnorm(c.g, c.seg_off, c.frozen).cls == cls and not np.all(np.isfinite(c.g))
    run_sqnorm(c, True)
    if n == R.N_SMALL:
        run_sqnorm(c, False)


def test_grad_sqnorm_raised_flag_writes_nothing():
    run_sqnorm(R.sqnorm_case(R.N_SMALL, frozen=(21,)), True, stop=True)


@pytest.mark.parametrize("spoil", [(0, None), (5, None), (1, 0), (2, None), (3, 0)], ids=["null-g", "null-scalars", "n-0", "seg_sq-no-seg_off", "frozen-nseg-0"])
def test_grad_sqnorm_refuses(spoil):
    run_sqnorm(R.sqnorm_case(R.N_SMALL, frozen=(21,)), True, spoil=spoil)


# ---- cl_owner_qnorm ----------------------------------------------------------------------------------------------------------------------
def run_owner(c, stop=False, spoil=None):
    ref = R.owner_qnorm(c.g, c.R, c.r0, c.r1)
    a = R.Guarded(DEV).add("g", c.g).add("out", np.full(4, SENT, F32), True).add("scratch", np.zeros(5), True)
    a.add("stop", np.array([1 if stop else 0], np.int32)).build()
    args = [a.ptr("g"), c.R, c.r0, c.r1, a.ptr("out"), a.ptr("scratch"), a.ptr("stop"), None]
    if spoil is not None:
        args[spoil[0]] = spoil[1]
    finish(a, int(lib().cl_owner_qnorm(*args)), -1 if spoil else 0, stop or spoil is not None)
    if stop or spoil:
        return
    out, sc, what = a.get("out"), a.get("scratch"), f"nr {c.r1 - c.r0}"
    assert a.changed("out").all()
    assert int(sc[4:5].view(np.int64)[0]) == R.owner_grid(c.r1 - c.r0), "scratch[4] is not the number of workgroups"
    R.assert_norm(sc[0], ref.cls, ref.sums[0], ref.n, f"{what}: scratch raw", "cl_owner_qnorm")
    R.assert_norm(out[0], ref.cls, ref.sums[0], ref.n, f"{what}: out raw", "cl_owner_qnorm", extra_rel=R.U)
    for j, n in ((2, ref.n // 2), (3, ref.n // 2)):
        R.assert_norm(sc[j], "finite", ref.sums[j], n, f"{what}: scratch sane", "cl_owner_qnorm")
    for j, n in ((1, ref.n), (2, ref.n // 2), (3, ref.n // 2)):
        R.assert_norm(out[j], "finite", ref.sums[j], n, f"{what}: out sane", "cl_owner_qnorm", extra_rel=R.U)
    assert sc[1] == sc[2] + sc[3], "scratch[1] is not out[2] + out[3] in double"
    assert out[1] == F32(sc[1]) and out[2] == F32(sc[2]) and out[3] == F32(sc[3])
    if ref.cls == "finite":
        assert out[0] == F32(sc[0])


@pytest.mark.parametrize("nr,nan_in", [(nr, 0) for nr in R.OWNER_LENGTHS] + [(nr, 1) for nr in R.OWNER_LENGTHS if nr > 1])
def test_owner_qnorm(nr, nan_in):
    """r0 > 0, r1 < R and NaN everywhere outside both windows: out[0] stays finite; a NaN in the a-window and an inf in the b-window: raw
    is NaN, out[1..3] stay finite and split by window (a window of one reflection has no room for both a finite and a non-finite element)"""
    c = R.owner_case(nr, bool(nan_in))
    assert R.owner_qnorm(c.g, c.R, c.r0, c.r1).cls == ("nan" if nan_in else "finite") and np.isnan(c.g[:c.r0]).all()
    run_owner(c)


def test_owner_qnorm_raised_flag_writes_nothing():
    run_owner(R.owner_case(513), stop=True)


@pytest.mark.parametrize("spoil", [(0, None), (4, None), (5, None), (1, 0), (2, -1), (3, 10 ** 6), (3, 37), (3, 30)],
                         ids=["null-g", "null-out", "null-scratch", "R-0", "r0-neg", "r1-beyond-R", "empty", "inverted"])
def test_owner_qnorm_refuses(spoil):
    run_owner(R.owner_case(513), spoil=spoil)


# ---- cl_step_finalize --------------------------------------------------------------------------------------------------------------------
N_HIST = 8


def run_finalize(n_part, klw, step, gn2=1.5e7, flag=0, part_bad=None, spoil=None):
    rng = np.random.default_rng(n_part + step)
    scalars = np.array([123.456, 7.89, gn2, 1.1e7])
    part = None
    if n_part:
        part = 10.0 ** rng.uniform(-6, 9, 2 * n_part)
        if part_bad is not None:
            part[2 * (n_part - 1)] = part_bad
    rec, brec, sc, bsc, flag_after = R.finalize(scalars, klw, part, flag)
    own = np.zeros((N_HIST, R.HIST_STRIDE), dtype=bool)
    own[step, :5] = True
    a = R.Guarded(DEV).add("scalars", scalars, NORM_SLOTS if n_part else False).add("history", np.full((N_HIST, R.HIST_STRIDE), SENT), own)
    if n_part:
        a.add("norm_part", part)
    a.add("stop", np.array([flag], np.int32), True).build()
    args = [a.ptr("scalars"), klw, a.ptr("history"), step, a.ptr("stop"), a.ptr("norm_part") if n_part else None, n_part, None]
    if spoil is not None:
        args[spoil[0]] = spoil[1]
    finish(a, int(lib().cl_step_finalize(*args)), -1 if spoil else 0, spoil is not None)
    if spoil:
        return
    got, gsc, what = a.get("history")[step], a.get("scalars"), f"n_norm_part {n_part}"
    assert a.changed("history")[step, :5].all() and int(a.get("stop")[0]) == flag_after
    if flag:
        assert got[:5].tolist() == [0.0, 0.0, 0.0, 0.0, 1.0] and not a.changed("scalars").any()
        return
    assert got[1] == scalars[R.SC_KL] and got[2] == scalars[R.SC_NLL] and got[4] == 0.0
    R.assert_within(got[0], rec[0], brec[0], f"{what}: loss", "cl_step_finalize")
    if flag_after:
        assert (math.isnan(got[3]) and math.isnan(rec[3])) or got[3] == rec[3] == math.inf
        return
    R.assert_within(gsc, sc, bsc, f"{what}: scalars", "cl_step_finalize")
    R.assert_within(got[3], rec[3], brec[3], f"{what}: Grad Norm", "cl_step_finalize")


@pytest.mark.parametrize("step", [0, 5])
@pytest.mark.parametrize("klw", [1.0, 0.5])
@pytest.mark.parametrize("n_part", [0, 1, 63, 64, 65, 1024])
def test_step_finalize(n_part, klw, step):
    """record {nll + klw kl, kl, nll, sqrt(gn2), 0} at step_index of 8, the norm_part pairs added into scalars[2] / [3]; a finite norm
    leaves a clear flag clear"""
    run_finalize(n_part, klw, step)


@pytest.mark.parametrize("n_part,gn2,part_bad", [(0, math.nan, None), (0, math.inf, None), (65, 1.5e7, math.nan), (65, 1.5e7, math.inf), (1024, math.inf, None)])
def test_step_finalize_nonfinite_norm_sets_the_flag(n_part, gn2, part_bad):
    run_finalize(n_part, 1.0, 5, gn2=gn2, part_bad=part_bad)


@pytest.mark.parametrize("n_part", [0, 65])
def test_step_finalize_raised_flag(n_part):
    """a flag already set: {0, 0, 0, 0, 1}, scalars left alone"""
    run_finalize(n_part, 0.5, 5, flag=1)


@pytest.mark.parametrize("spoil", [(0, None), (2, None), (3, -1), (6, 0)], ids=["null-scalars", "null-history", "step-neg", "norm_part-0"])
def test_step_finalize_refuses(spoil):
    run_finalize(65, 1.0, 5, spoil=spoil)
