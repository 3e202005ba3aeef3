"""The exact forms of the 64-wide plain-epilogue instances (`cl_mlp_instance_traits`, include/careless_hip.h) against the instances every
launch ran before them, and against the fp64 reference.

csrc/elbo_mlp.hip compiles the plain-epilogue instances of the 64-wide kernel a second time for what a launch really holds: on 32
padded metadata columns with the 6 first-layer k-steps that 8 < d <= 24 real columns fill (`K1`), and on up to 32 padded columns with
the depth compiled in when the launch runs all 5 layers.  Neither is in the kernel's printed name.  `CARELESS_HIP_EXACT=0` keeps a
process on the earlier instances; the library reads its switches once per process, so the two settings run in a fresh child each.
Each child runs ONE step (loss + gradients, then Adam) of every case through the engine, once for the whole module.

Cases: w = 64; L = 5 (depth compiled in) and 3 (must keep the run-time depth); d = 9, 21, 24 (the rims and the headline of K1 = 6), 25
and 32 (must keep 8), and one depth of d = 5 per likelihood (8 padded columns: 2 k-steps, all real; only the depth form); 165 rows = one tile of 128 and a 37-row tail, 421 rows = three tiles and the tail; one workgroup walking every
tile and two; S = 1 and 8; Normal and Student-T.  Asserted per case:
  * `cl_mlp_instance_traits` answers the expected k-steps and depth form, `kernel_name()` is the same for both settings;
  * against the forced earlier instance: the scaler's gradient is equal element for element (the dropped k-steps add fma(0, 0, acc):
    zeros may differ in sign, which `==` does not see); loss terms, every gradient tensor and every parameter after Adam agree at the
    tolerances tests/test_epilogue_plain.py holds plain against generic to (those of tests/test_gpu_parity.py, imported) -- the order of
    the float atomics is the only difference;
  * the same launches, issued directly through the C ABI, against the fp64 reference of tests/ref_mlp.py at its bounds, through the
    harness of tests/test_mlp_kernels_gpu.py (guarded operands, write masks, error / bound <= 1).
One non-finite case (the contract of tests/test_nonfinite.py): a NaN in one metadata cell at d = 21 gives the same non-finite mask of
every gradient tensor as the earlier instance, and the parameters stay finite.  The routing answers and the switch are checked without
a device."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 64
DEPTHS = (5, 3)
COLUMNS = (9, 21, 24, 25, 32)
ROWS = (165, 421)
GRIDS = (1, 2)
SAMPLES = (1, 8)
LIKS = ("normal", "studentt")
SEED = 4321
NAME = "elbo_mlp_kernel<64, 32, 5, 0, KS=4>"
NAME_DP8 = "elbo_mlp_kernel<64, 8, 5, 0, KS=4>"
# (the two compile-time-depth instances on 8 padded columns, one group each)
GROUPS = list(itertools.product(DEPTHS, COLUMNS, LIKS, SAMPLES)) + [(5, 5, "normal", 8), (5, 5, "studentt", 1)]
GROUP_IDS = [f"{L}x{W}-d{d}-{lik}-S{S}" for L, d, lik, S in GROUPS]
POISON = dict(L=5, d=21, lik="studentt", S=8, n=421, grid=2)


def expected_traits(L, d):
    """(first-layer k-steps, depth compiled in) of a plain-epilogue launch of a 64-wide scaler on up to 32 metadata columns"""
    return (2 if d <= 8 else 6 if d <= 24 else 8), L == 5


def earlier_traits(d):
    """... of the instance every such launch ran before: all k-steps of the padded width, the run-time depth"""
    return (2 if d <= 8 else 8), False


def expected_name(d):
    return NAME_DP8 if d <= 8 else NAME


def _kw(L, d, lik, S, n):
    kw = dict(N=n, R=24, d0=d, L=L, w=W, S=S, likelihood=lik, n_images=4)
    if lik == "studentt":
        kw.update(dof=4.0)
    return kw


def _step(out, pre, kw, grid, poison=False):
    """One step of a fresh engine on the noise it draws itself; everything the cases compare goes to out[pre + ...]"""
    import ctypes as C

    import torch

    from careless_amd.engine import ElboEngine
    from tests import util
    data, cfg, params, x, _, _ = util.make_problem(**kw)
    if poison:
        data = dict(data)
        meta = np.array(data["metadata"], dtype=np.float32, copy=True)
        row = kw["N"] // 2 + 3
        meta[row, row % meta.shape[1]] = np.nan
        data["metadata"] = meta
    model = util.build_model(data, cfg, params, kw["L"], kw["w"])
    model.kernel_grid = grid
    eng = ElboEngine(model, util.reference_inputs(data), seed=SEED)
    ma, mode = eng.training_launch()
    out[pre + "traits"] = np.array([int(eng.lib.cl_mlp_instance_traits(C.byref(ma), mode))])
    out[pre + "name"] = np.array([eng.kernel_name()])
    eng.alloc_history(1)
    eng.forward_backward(0)
    torch.cuda.synchronize()
    lay = eng.layout
    out[pre + "mlp"] = eng.grads[lay.off_mlp: lay.off_mlp + lay.P].cpu().numpy().copy()
    t = eng.loss_terms()
    out[pre + "terms"] = np.array([t["nll"], t["kl"], t["loss"]])
    for i, g in enumerate(eng.grad_tensors()):
        out[pre + f"g{i:03d}"] = g.cpu().numpy().copy()
    eng.optimizer_step(0)
    torch.cuda.synchronize()
    for i, p in enumerate(eng.param_tensors()):
        out[pre + f"p{i:03d}"] = p.cpu().numpy().copy()


def _child(out_path):
    """Runs in the child process: every case of the module, everything the parent compares into one .npz."""
    out = {}
    for (L, d, lik, S), n, grid in itertools.product(GROUPS, ROWS, GRIDS):
        _step(out, f"{L}|{d}|{lik}|{S}|{n}|{grid}|", _kw(L, d, lik, S, n), grid)
    p = POISON
    _step(out, "poison|", _kw(p["L"], p["d"], p["lik"], p["S"], p["n"]), p["grid"], poison=True)
    np.savez(out_path, **out)


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    """{setting: arrays} of the two children: CARELESS_HIP_EXACT unset (the exact instances where they apply) and =0 (the earlier ones)."""
    d = tmp_path_factory.mktemp("exact")
    res = {}
    for setting in ("unset", "0"):
        env = {k: v for k, v in os.environ.items() if k != "CARELESS_HIP_EXACT"}
        if setting == "0":
            env["CARELESS_HIP_EXACT"] = "0"
        path = str(d / f"exact_{setting}.npz")
        code = f"from tests import test_mlp_exact_instance as T; T._child({path!r})"
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (setting, r.stdout[-2000:], r.stderr[-4000:])
        res[setting] = dict(np.load(path))
    return res


def _traits(arr):
    from careless_amd import _lib
    t = int(arr[0])
    assert t >= 0, t
    return t & _lib.CL_TRAIT_K1_MASK, bool(t & _lib.CL_TRAIT_FIXED_DEPTH)


def _compare(new, ref, pre, what):
    """loss terms, gradient tensors and parameters after Adam of the two settings at the tolerances of tests/test_epilogue_plain.py"""
    from tests import util
    from tests.test_gpu_parity import RTOL_GRAD, RTOL_LOSS
    worst = {}
    for k, (a, b) in enumerate(zip(new[pre + "terms"], ref[pre + "terms"])):
        worst["terms"] = max(worst.get("terms", 0.0), abs(a - b) / max(abs(b), 1.0 if k == 1 else 1e-30))
    keys = sorted(k for k in ref if k.startswith(pre + "g") or k.startswith(pre + "p"))
    assert any(k.startswith(pre + "g") for k in keys) and any(k.startswith(pre + "p") for k in keys)
    for k in keys:
        assert np.all(np.isfinite(ref[k])) and new[k].shape == ref[k].shape, k
        kind = "grads" if k.startswith(pre + "g") else "params"
        if float(np.max(np.abs(ref[k]))) == 0.0:
            assert float(np.max(np.abs(new[k]))) == 0.0, k
            continue
        worst[kind] = max(worst.get(kind, 0.0), util.rel_err(new[k], ref[k]))
    print(f"{what}: exact against earlier instance: loss terms {worst['terms']:.2e} (bound {RTOL_LOSS:.0e}), gradient tensors "
          f"{worst['grads']:.2e}, parameters after Adam {worst['params']:.2e} (bound {RTOL_GRAD:.0e})")
    assert worst["terms"] <= RTOL_LOSS
    assert worst["grads"] < RTOL_GRAD
    assert worst["params"] < RTOL_GRAD


@pytest.mark.gpu
@pytest.mark.parametrize("L,d,lik,S", GROUPS, ids=GROUP_IDS)
def test_exact_instance_equals_the_earlier_one(both, L, d, lik, S):
    new, ref = both["unset"], both["0"]
    for n, grid in itertools.product(ROWS, GRIDS):
        pre = f"{L}|{d}|{lik}|{S}|{n}|{grid}|"
        what = f"{L}x{W} d{d} {lik} S{S} {n} rows grid {grid}"
        assert _traits(new[pre + "traits"]) == expected_traits(L, d), what
        assert _traits(ref[pre + "traits"]) == earlier_traits(d), what
        assert str(new[pre + "name"][0]) == str(ref[pre + "name"][0]) == expected_name(d), what
        a, b = new[pre + "mlp"], ref[pre + "mlp"]
        assert np.all(np.isfinite(b)) and float(np.max(np.abs(b))) > 0.0, what
        differ = np.flatnonzero(a != b)
        print(f"{what}: scaler gradient, {a.size} elements, {len(differ)} differ")
        assert np.array_equal(a, b), (what, differ[:8].tolist(), a[differ[:8]].tolist(), b[differ[:8]].tolist())
        for k in sorted(k for k in ref if k.startswith(pre + "g")):      # the scaler's tensors among them: W_0, b_0, ..., W_o, b_o
            i = int(k[len(pre) + 1:])
            if 2 <= i < 2 + 2 * (L + 1):
                assert np.array_equal(new[k], ref[k]), (what, k)
        _compare(new, ref, pre, what)


@pytest.mark.gpu
def test_a_poisoned_metadata_cell_gives_the_earlier_instances_mask(both):
    new, ref = both["unset"], both["0"]
    p = POISON
    assert _traits(new["poison|traits"]) == expected_traits(p["L"], p["d"]) == (6, True) and _traits(ref["poison|traits"]) == (8, False)
    assert str(new["poison|name"][0]) == str(ref["poison|name"][0]) == NAME
    keys = sorted(k for k in ref if k.startswith("poison|g"))
    assert keys and not np.all(np.isfinite(ref["poison|mlp"]))           # the poison reaches the scaler's gradient on the earlier instance
    for k in keys + ["poison|mlp"]:
        fa, fb = np.isfinite(new[k]), np.isfinite(ref[k])
        assert np.array_equal(fa, fb), (k, int((fa & ~fb).sum()), int((~fa & fb).sum()))
    for s in (new, ref):
        assert not np.isfinite(s["poison|terms"][0])
        pk = sorted(k for k in s if k.startswith("poison|p"))
        assert pk and all(np.all(np.isfinite(s[k])) for k in pk)


@pytest.mark.gpu
@pytest.mark.parametrize("L,d,lik,S", GROUPS, ids=GROUP_IDS)
def test_exact_instance_matches_fp64(L, d, lik, S):
    """The same launches through the C ABI against tests/ref_mlp.py's fp64 reference, at its bounds (error / bound <= 1 in `record`)."""
    import ctypes as C

    from careless_amd import _lib
    from tests import ref_mlp as RM
    from tests import test_mlp_kernels_gpu as K
    for n, grid in itertools.product(ROWS, GRIDS):
        c = RM.case("plain", 0, W, d, L, n=n, grid=grid, S=S, lik=lik, noise="philox", img="sorted", tag="exact")
        x, ref = K.inputs_of(c)
        run = K.Run(x, ref)
        assert _traits([_lib.get_lib().cl_mlp_instance_traits(C.byref(run.A), 0)]) == expected_traits(L, d), c.id
        got = run.launch().result()
        K.record(c, RM.ratios(x, ref, run.pre, got))


# ---- the routing answers, without a device --------------------------------------------------------------------------------------------

def _query(mode=0, **over):
    """cl_mlp_instance_traits of the headline's launch (5 x 64 on 21 columns, S = 8 Student-T) with these fields changed"""
    from careless_amd import _lib
    f = dict(d=21, w=W, L=5, S=8, R=24, n_obs=421, n_pad=512, lik_kind=_lib.CL_LIK_STUDENTT, use_img=1)
    f.update(over)
    return _lib.mlp_instance_traits(_lib.get_lib(), mode, **f)


def _name(**over):
    import ctypes as C

    from careless_amd import _lib
    f = dict(d=21, w=W, L=5, S=8, R=24, n_obs=421, n_pad=512, lik_kind=_lib.CL_LIK_STUDENTT, use_img=1)
    f.update(over)
    buf = C.create_string_buffer(256)
    _lib.get_lib().cl_mlp_kernel_name(C.byref(_lib.MlpArgs(**f)), 0, buf, 256)
    return buf.value.decode()


def test_query_answers_the_exact_forms():
    from careless_amd import _lib
    for L, d in itertools.product(DEPTHS, COLUMNS):
        for lik in (_lib.CL_LIK_NORMAL, _lib.CL_LIK_STUDENTT):
            for S in SAMPLES:
                assert _query(L=L, d=d, lik_kind=lik, S=S) == expected_traits(L, d), (L, d, lik, S)
        assert _name(L=L, d=d) == NAME
    assert _query() == (6, True)
    for w in (33, 40, 64):                          # every width of the 64-wide instance
        assert _query(w=w) == (6, True)
    for L in (1, 2, 3, 4):                          # fewer layers than the instance holds: the run-time depth
        assert _query(L=L) == (6, False)
    for d in (1, 5, 8):                             # 8 padded columns: 2 k-steps, all real; the depth form still applies
        assert _query(d=d) == (2, True) and _query(d=d, L=2) == (2, False)
    for d in (33, 50, 64):                          # 64 padded columns: neither form is compiled
        assert _query(d=d) == (16, False)
    assert _query(use_img=0) == (6, True)


@pytest.mark.parametrize("over,want", [
    (dict(S=9), (8, False)), (dict(eta=1), (8, False)), (dict(ipred_out=1), (8, False)), (dict(ev11=1, d_ev11=1), (8, False)),
    (dict(noise_row=1), (8, False)), (dict(lik_kind=2), (8, False)), (dict(mode=1), (8, False)), (dict(mode=2), (8, False)),
    (dict(dzf_obs=1, nll_part=1, dimg_obs=1), (8, False)), (dict(row_map=1), (8, False)), (dict(dX_out=1), (8, False)),
    (dict(w=32), (8, False)), (dict(w=20, d=5), (2, False)), (dict(w=10, L=20, d=5), (0, False)), (dict(w=15, L=3, d=5), (0, False))],
    ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()) if isinstance(o, dict) else None)
def test_query_answers_all_k_steps_and_a_run_time_depth_elsewhere(over, want):
    """the generic epilogue, the other units, the narrower instances: every k-step of the padded width and the run-time depth; the lane
    and narrow kernels' routes have no such k-steps (0)"""
    over = dict(over)
    assert _query(over.pop("mode", 0), **over) == want


def test_query_rejects_bad_arguments():
    import ctypes as C

    from careless_amd import _lib
    lib = _lib.get_lib()
    assert lib.cl_mlp_instance_traits(None, 0) == -1
    a = _lib.MlpArgs(d=21, w=W, L=5, S=8)
    assert lib.cl_mlp_instance_traits(C.byref(a), 3) == -1 and lib.cl_mlp_instance_traits(C.byref(a), -1) == -1
    a = _lib.MlpArgs(d=21, w=65, L=5, S=8)          # no kernel takes the launch
    assert lib.cl_mlp_instance_traits(C.byref(a), 0) == -2


@pytest.mark.parametrize("env,want", [
    (dict(CARELESS_HIP_EXACT="0"), ["8", "False", "2", "False", "8", "False"]),
    (dict(CARELESS_HIP_EXACT="k1"), ["6", "False", "2", "False", "6", "False"]),
    (dict(CARELESS_HIP_EXACT="depth"), ["8", "True", "2", "True", "8", "False"]),
    (dict(CARELESS_HIP_EXACT="1"), ["6", "True", "2", "True", "6", "False"]),
    (dict(CARELESS_HIP_EXACT="d"), ["6", "True", "2", "True", "6", "False"]),         # (the two words are matched whole)
    (dict(CARELESS_HIP_EXACT="k"), ["6", "True", "2", "True", "6", "False"]),
    (dict(CARELESS_HIP_EPI="0"), ["8", "False", "2", "False", "8", "False"])],
    ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()) if isinstance(e, dict) else None)
def test_switch_keeps_every_launch_on_the_earlier_instances(env, want):
    """CARELESS_HIP_EXACT, read once per process: a child.  =0 both forms off, =k1 / =depth one of them (measurements); the name stays."""
    code = ("from tests import test_mlp_exact_instance as T; "
            "print(*T._query(), *T._query(d=5), *T._query(L=3), T._name())")
    base = {k: v for k, v in os.environ.items() if k not in ("CARELESS_HIP_EXACT", "CARELESS_HIP_EPI")}
    out = subprocess.run([sys.executable, "-c", code], env=dict(base, **env), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.split(maxsplit=6)
    assert got[:6] == want and got[6].strip() == NAME, got
