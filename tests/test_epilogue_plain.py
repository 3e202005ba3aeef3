"""The plain sampling epilogue of the 64-wide fused kernel (`cl_mlp_epilogue`, include/careless_hip.h) against the generic one.

The 64-wide instances of csrc/elbo_mlp.hip come with two epilogues: the generic one, which decides every launch-uniform option per MC
sample, and one compiled for the common full step (in-kernel noise keyed by the row itself, no `ipred_out`, no Evans-2011 model,
S <= 8, the likelihood kind a constant).  `CARELESS_HIP_EPI=0` keeps a process on the generic epilogue; the library reads its switches
once per process, so the two settings run in a fresh child each.  Each child runs ONE step (loss + gradients, then Adam) of every case
below, once for the whole module; the cases compare loss terms, every gradient tensor and every parameter tensor after the update at
the tolerances tests/test_gpu_parity.py holds the kernel to against the oracle (imported from there, not restated).

Shapes: 2 x 40 scalers (the 64-wide instance) on 165 rows = one full tile of 128 and a 37-row tail, so padded rows occur; 5, 21 and 40
metadata columns = the three metadata capacities (8 / 32 / 64) the instance is compiled for; S = 1, 3, 4, 5, 8 = epilogue lanes
without a sample, a live second sample on one slot only, and the full pair; both likelihoods; image scales on and off; image borders
inside a wave, no border at all, and one workgroup walking both tiles.

The launches the plain epilogue does not take -- more than 8 samples, injected noise, `ipred_out`, Ev11, `noise_row`, deterministic
mode, single-pass Laue, modes 1 / 2 -- must answer CL_EPI_GENERIC (CPU cases) and still match the fp64 oracle (GPU cases)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROWS, L, W = 165, 2, 40


def _plain_cases():
    cases = {}
    for d0, posenc, dname in ((5, False, "d5"), (5, True, "d21"), (40, False, "d40")):
        for S in (1, 3, 4, 5, 8):
            for lik in ("normal", "studentt"):
                kw = dict(N=N_ROWS, R=24, d0=d0, posenc=posenc, L=L, w=W, S=S, likelihood=lik, n_images=4)
                if lik == "studentt":
                    kw.update(dof=4.0, outliers=True)
                cases[f"{dname}_S{S}_{lik}"] = kw
    for d0, posenc, dname, S, lik in ((5, False, "d5", 8, "studentt"), (5, False, "d5", 3, "normal"), (5, True, "d21", 5, "normal"),
                                      (5, True, "d21", 8, "studentt"), (40, False, "d40", 1, "studentt"), (40, False, "d40", 4, "normal")):
        kw = dict(N=N_ROWS, R=24, d0=d0, posenc=posenc, L=L, w=W, S=S, likelihood=lik, n_images=4, use_image_scales=False)
        if lik == "studentt":
            kw.update(dof=4.0)
        cases[f"{dname}_S{S}_{lik}_noimg"] = kw
    # image borders: nine images on 165 rows (~18 rows each: every wave of 16 rows holds a border), one image (no border: the
    # wave-uniform reduction everywhere), and one workgroup that walks both tiles (arguments re-read per tile)
    cases["nine_images_S8_studentt"] = dict(N=N_ROWS, R=24, d0=5, posenc=True, L=L, w=W, S=8, likelihood="studentt", dof=4.0, n_images=9)
    cases["one_image_S5_normal"] = dict(N=N_ROWS, R=24, d0=5, L=L, w=W, S=5, n_images=1)
    cases["one_workgroup_two_tiles_S8_studentt"] = dict(N=N_ROWS, R=24, d0=5, posenc=True, L=L, w=W, S=8, likelihood="studentt", dof=4.0,
                                                        n_images=4, grid=1)
    return cases


PLAIN_CASES = _plain_cases()


def _child(out_path):
    """Runs in the child process: one step of every case, everything the parent compares into one .npz."""
    import ctypes as C

    import torch

    from careless_amd.engine import ElboEngine
    from tests import util
    out = {}
    for name, kw in PLAIN_CASES.items():
        kw = dict(kw)
        grid = kw.pop("grid", None)
        data, cfg, params, x, _, _ = util.make_problem(**kw)
        model = util.build_model(data, cfg, params, kw["L"], kw["w"])
        model.kernel_grid = grid
        eng = ElboEngine(model, util.reference_inputs(data), seed=99)
        ma, mode = eng.training_launch()
        out[f"{name}|epi"] = np.array([eng.lib.cl_mlp_epilogue(C.byref(ma), mode)])
        out[f"{name}|name"] = np.array([eng.kernel_name()])
        eng.alloc_history(1)
        eng.forward_backward(0)
        torch.cuda.synchronize()
        t = eng.loss_terms()
        out[f"{name}|terms"] = np.array([t["nll"], t["kl"], t["loss"]])
        for i, g in enumerate(eng.grad_tensors()):
            out[f"{name}|g{i}"] = g.cpu().numpy().copy()
        eng.optimizer_step(0)
        torch.cuda.synchronize()
        for i, p in enumerate(eng.param_tensors()):
            out[f"{name}|p{i}"] = p.cpu().numpy().copy()
        out[f"{name}|image_id"] = np.asarray(data["image_id"])
    np.savez(out_path, **out)


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    """{setting: arrays} of the two children: CARELESS_HIP_EPI unset (the plain epilogue where it applies) and =0 (generic)."""
    d = tmp_path_factory.mktemp("epi")
    res = {}
    for setting in ("unset", "0"):
        env = {k: v for k, v in os.environ.items() if k != "CARELESS_HIP_EPI"}
        if setting == "0":
            env["CARELESS_HIP_EPI"] = "0"
        path = str(d / f"epi_{setting}.npz")
        code = f"from tests import test_epilogue_plain as T; T._child({path!r})"
        r = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (setting, r.stdout[-2000:], r.stderr[-4000:])
        res[setting] = dict(np.load(path))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PLAIN_CASES))
def test_plain_epilogue_equals_the_generic_one(both, name):
    from careless_amd import _lib
    from tests import util
    from tests.test_gpu_parity import RTOL_GRAD, RTOL_LOSS
    new, ref = both["unset"], both["0"]
    kw = PLAIN_CASES[name]
    want = _lib.CL_EPI_PLAIN_STUDENTT if kw.get("likelihood") == "studentt" else _lib.CL_EPI_PLAIN_NORMAL
    assert int(new[f"{name}|epi"][0]) == want and int(ref[f"{name}|epi"][0]) == _lib.CL_EPI_GENERIC
    assert str(new[f"{name}|name"][0]) == str(ref[f"{name}|name"][0])             # the name is the geometry's: the same for both epilogues
    assert str(new[f"{name}|name"][0]).startswith("elbo_mlp_kernel<64, ")
    if name.startswith("nine_images"):
        border = np.flatnonzero(np.diff(ref[f"{name}|image_id"])) + 1
        assert len(border) and np.any(border % 16 != 0)                           # an image ends inside a wave's 16 rows
    worst = {}
    for k, (a, b) in enumerate(zip(new[f"{name}|terms"], ref[f"{name}|terms"])):
        worst["terms"] = max(worst.get("terms", 0.0), abs(a - b) / max(abs(b), 1.0 if k == 1 else 1e-30))
    keys = sorted(k for k in ref if k.startswith(f"{name}|g") or k.startswith(f"{name}|p"))
    assert any(k.startswith(f"{name}|g") for k in keys) and any(k.startswith(f"{name}|p") for k in keys)
    for k in keys:
        assert np.all(np.isfinite(ref[k])) and new[k].shape == ref[k].shape
        kind = "grads" if k.startswith(f"{name}|g") else "params"
        if float(np.max(np.abs(ref[k]))) == 0.0:
            assert float(np.max(np.abs(new[k]))) == 0.0, k
            continue
        worst[kind] = max(worst.get(kind, 0.0), util.rel_err(new[k], ref[k]))
    print(f"{name}: largest difference plain vs generic epilogue: loss terms {worst['terms']:.2e} (bound {RTOL_LOSS:.0e}), "
          f"gradient tensors {worst['grads']:.2e}, parameters after Adam {worst['params']:.2e} (bound {RTOL_GRAD:.0e})")
    assert worst["terms"] <= RTOL_LOSS
    assert worst["grads"] < RTOL_GRAD
    assert worst["params"] < RTOL_GRAD


# ---- the launches that keep the generic epilogue ----------------------------------------------------------------------------------

def _query(mode=0, **over):
    """cl_mlp_epilogue of a 2 x 40 launch on 21 metadata columns with these fields changed (pointer fields: non-zero = given)."""
    from careless_amd import _lib
    f = dict(d=21, w=W, L=L, S=8, R=24, n_obs=N_ROWS, n_pad=256, lik_kind=_lib.CL_LIK_STUDENTT, use_img=1)
    f.update(over)
    return _lib.mlp_epilogue(_lib.get_lib(), mode, **f)


def test_query_answers_plain_for_the_common_launch():
    from careless_amd import _lib
    assert _query() == _lib.CL_EPI_PLAIN_STUDENTT
    assert _query(lik_kind=_lib.CL_LIK_NORMAL) == _lib.CL_EPI_PLAIN_NORMAL
    for S in (1, 3, 4, 5, 8):
        assert _query(S=S) == _lib.CL_EPI_PLAIN_STUDENTT
    for d in (5, 21, 40, 64):
        assert _query(d=d) == _lib.CL_EPI_PLAIN_STUDENTT
    for w in (33, 64):
        assert _query(w=w, L=5) == _lib.CL_EPI_PLAIN_STUDENTT
    assert _query(use_img=0) == _lib.CL_EPI_PLAIN_STUDENTT
    assert _lib.mlp_route(_lib.get_lib(), 0, d=21, w=W, L=L, S=8) == _lib.CL_ROUTE_MLP


@pytest.mark.parametrize("over", [dict(S=9), dict(S=12), dict(eta=1), dict(ipred_out=1), dict(ev11=1, d_ev11=1), dict(ev11=1), dict(d_ev11=1),
                                  dict(ev11_part=1), dict(noise_row=1), dict(dzf_obs=1, nll_part=1, dimg_obs=1), dict(row_map=1, gmeta=1, tile_gmax=1),
                                  dict(row_map=1), dict(mode=1), dict(mode=2), dict(lik_kind=7), dict(w=32), dict(w=10, L=20), dict(w=15),
                                  dict(L=6), dict(w=65), dict(act_out=1, mode=1), dict(dX_out=1), dict(n_imgl=1, row_map=1)],
                         ids=lambda o: "-".join(f"{k}{v}" for k, v in o.items()))
def test_query_answers_generic_for_every_other_launch(over):
    from careless_amd import _lib
    over = dict(over)
    assert _query(over.pop("mode", 0), **over) == _lib.CL_EPI_GENERIC


def test_query_rejects_bad_arguments():
    from careless_amd import _lib
    lib = _lib.get_lib()
    assert lib.cl_mlp_epilogue(None, 0) < 0
    assert _query(mode=3) < 0 and _query(mode=-1) < 0


def test_switch_keeps_every_launch_on_the_generic_epilogue():
    """CARELESS_HIP_EPI=0, read once per process: a child."""
    code = ("from tests import test_epilogue_plain as T; from careless_amd import _lib; "
            "print(T._query(), T._query(lik_kind=_lib.CL_LIK_NORMAL), T._query(S=1))")
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CARELESS_HIP_EPI="0"), cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split() == ["0", "0", "0"]


@pytest.fixture
def launches(monkeypatch):
    """[(mode, cl_mlp_epilogue's answer)] of every scaler launch the test issues, asked with the launch's own arguments: the three
    entry points of the library are wrapped for the test (a launch with injected noise or `ipred_out` is not the engine's
    `training_launch()`, so the question has to be put where the arguments are)."""
    from careless_amd import _lib
    lib = _lib.get_lib()
    seen = []
    for mode, entry in enumerate(("cl_elbo_mono_fwd_bwd", "cl_mlp_forward", "cl_mlp_backward_ext")):
        def wrapped(a, grid, stream, _mode=mode, _fn=getattr(lib, entry)):
            seen.append((_mode, int(lib.cl_mlp_epilogue(a, _mode))))
            return _fn(a, grid, stream)
        monkeypatch.setattr(lib, entry, wrapped)
    return seen


FALLBACK_CASES = {
    # injected noise and `ipred_out` (the oracle-parity call asks for both)
    "injected_noise_and_ipred_out_S8": dict(N=N_ROWS, R=24, d0=5, posenc=True, L=L, w=W, S=8, likelihood="studentt", dof=4.0, outliers=True),
    "ev11_S5": dict(N=N_ROWS, R=24, d0=5, L=L, w=W, S=5, ev11=True, likelihood="studentt", dof=6.0),
    "laue_single_pass_S3": dict(N=300, R=24, L=L, w=W, S=3, laue=True),
    "laue_two_pass_modes_1_and_2_S3": dict(N=300, R=24, L=L, w=W, S=3, laue=True, two_pass=True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FALLBACK_CASES))
def test_fallback_launches_stay_generic_and_match_the_oracle(name, launches):
    from careless_amd import _lib
    from tests import util
    from tests.test_gpu_parity import RTOL_LOSS, _assert_grads, _run_case
    out, grads, ipred, terms, g_hip, eng, prob = _run_case(FALLBACK_CASES[name])
    assert eng.kernel_name().startswith("elbo_mlp_kernel<64, ")
    assert launches and all(e == _lib.CL_EPI_GENERIC for _, e in launches), launches
    assert {m for m, _ in launches} == ({1, 2} if name.startswith("laue_two_pass") else {0})
    assert abs(terms["nll"] - float(out["nll"])) <= RTOL_LOSS * abs(float(out["nll"])), (terms, float(out["nll"]))
    assert abs(terms["loss"] - float(out["loss"])) <= RTOL_LOSS * abs(float(out["loss"]))
    assert util.rel_err(ipred, out["ipred"].numpy()) < 1e-4
    _assert_grads(g_hip, grads, prob, name)


def _oracle_on_dumped_noise(kw, seed):
    """The fp64 oracle on the noise the kernels draw themselves (cl_debug_noise dumps the same streams)."""
    import torch

    from careless_amd.engine import debug_noise
    from oracle import elbo_oracle as O
    from tests import util
    data, cfg, params, x, _, _ = util.make_problem(**kw)
    u = debug_noise(seed, 0, kw["S"], kw["R"], 0, kind=0).t().cpu().numpy()
    e = debug_noise(seed, 0, kw["S"], kw["N"], 0, kind=1).t().cpu().numpy()
    out, grads = O.elbo_value_and_grads(params, x, cfg, torch.as_tensor(u, dtype=torch.float64), torch.as_tensor(e, dtype=torch.float64))
    return data, cfg, params, out, grads, (data, cfg, params, u, e)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [9, 12, 8])
def test_in_kernel_noise_matches_the_oracle_past_eight_samples(S, launches):
    """In-kernel noise with more than 8 samples: the generic epilogue's loop (samples beyond the second load z_f inside it); S = 8, the
    same launch on the plain epilogue, against the same oracle."""
    import torch

    from careless_amd import _lib
    from careless_amd.engine import ElboEngine
    from tests import util
    from tests.test_gpu_parity import RTOL_LOSS, _assert_grads
    kw = dict(N=N_ROWS, R=24, d0=5, posenc=True, L=L, w=W, S=S, likelihood="studentt", dof=4.0)
    data, cfg, params, out, grads, prob = _oracle_on_dumped_noise(kw, 4321)
    eng = ElboEngine(util.build_model(data, cfg, params, L, W), util.reference_inputs(data), seed=4321)
    eng.forward_backward(0)
    torch.cuda.synchronize()
    assert launches == [(0, _lib.CL_EPI_PLAIN_STUDENTT if S <= 8 else _lib.CL_EPI_GENERIC)]
    t = eng.loss_terms()
    assert abs(t["loss"] - float(out["loss"])) <= RTOL_LOSS * abs(float(out["loss"]))
    _assert_grads([g.cpu().numpy() for g in eng.grad_tensors()], grads, prob, f"philox_S{S}")


@pytest.mark.gpu
def test_noise_row_shards_stay_generic_and_sum_to_the_oracle(launches):
    """Reflection-owner shards key the in-kernel noise by `noise_row` (the rows' global numbers): generic epilogue; their sum is the
    oracle's step on the dumped noise, like the single-rank step on the plain epilogue."""
    import torch

    from careless_amd import _lib
    from careless_amd.engine import ElboEngine, make_shard
    from tests import util
    from tests.test_gpu_parity import RTOL_LOSS, _assert_grads
    kw = dict(N=N_ROWS, R=24, d0=5, L=L, w=W, S=8, likelihood="studentt", dof=4.0)
    data, cfg, params, out, grads, prob = _oracle_on_dumped_noise(kw, 99)
    inputs = util.reference_inputs(data)
    gs, nll, kl = None, 0.0, 0.0
    for r in range(2):
        m = util.build_model(data, cfg, params, L, W)
        m.owner_shard = True
        eng = ElboEngine(m, inputs, seed=99, shard=make_shard(kw["N"], kw["R"], r, 2))
        assert eng.owner
        eng.local_only = True
        eng.forward_backward(0)
        torch.cuda.synchronize()
        gt = [g.clone() for g in eng.grad_tensors()]
        gs = gt if gs is None else [a + b for a, b in zip(gs, gt)]
        t = eng.loss_terms()
        nll += t["nll"]; kl += t["kl"]
    assert launches == [(0, _lib.CL_EPI_GENERIC)] * 2
    assert abs(nll - float(out["nll"])) <= RTOL_LOSS * abs(float(out["nll"])) and abs(kl - float(out["kl"])) <= RTOL_LOSS * max(abs(float(out["kl"])), 1.0)
    _assert_grads([g.cpu().numpy() for g in gs], grads, prob, "noise_row")


@pytest.mark.gpu
def test_deterministic_mode_stays_generic_and_matches_the_oracle(launches):
    import torch

    from careless_amd import _lib
    from oracle import elbo_oracle as O
    from tests import util
    from tests.test_gpu_parity import RTOL_LOSS, _assert_grads
    kw = dict(N=N_ROWS, R=24, d0=5, L=L, w=W, S=8, likelihood="studentt", dof=4.0)
    data, cfg, params, x, u_f, eta = util.make_problem(**kw)
    model = util.build_model(data, cfg, params, L, W)
    model.deterministic = True
    model(util.reference_inputs(data), u_f=u_f, eta=eta)
    eng = model._engine
    torch.cuda.synchronize()
    assert "deterministic" in eng.kernel_name() and launches == [(0, _lib.CL_EPI_GENERIC)]
    out, grads = O.elbo_value_and_grads(params, x, cfg, torch.as_tensor(u_f, dtype=torch.float64), torch.as_tensor(eta, dtype=torch.float64))
    t = eng.loss_terms()
    assert abs(t["loss"] - float(out["loss"])) <= RTOL_LOSS * abs(float(out["loss"]))
    _assert_grads([g.cpu().numpy() for g in eng.grad_tensors()], grads, (data, cfg, params, u_f, eta), "deterministic")
