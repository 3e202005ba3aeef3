"""The workgroup barriers of the 32- and 64-wide fused kernel (csrc/elbo_mlp.hip) sit where their condition first holds.

In the plain-epilogue instances barrier A of a layer step and the tile-seam barrier are signalled inside the wgrad loop in front of
them, as soon as a wave's own last read of the staging tiles sZ / sH has landed; the other instances share the
loop and keep the late barriers.  A barrier in the wrong place is a race on those tiles: it
corrupts blocks of the weight gradient, which are otherwise deterministic to the bit -- register accumulators over a fixed tile order,
per-workgroup partials summed in a fixed order.  So every case runs ONE step on three fresh engines and asks for the same bits in the
scaler's gradient, for the same values (1e-6) from one workgroup walking every tile and from two, and for the fp64 oracle's loss and
gradients at the tolerances of tests/test_gpu_parity.py.

Shapes: 421 rows = three full tiles of 128 and a 37-row tail, and 165 rows = one tile and the tail; `kernel_grid` 1 (one workgroup walks
all tiles: every seam) and 2.  Scalers 1 x 40, 2 x 40, 5 x 40 (the 64-wide instance with no barrier A, one, four) and 2 x 20, 7 x 20 (the
32-wide instances of 5 and 10 layers), on 5, 21 and 40 metadata columns (the three metadata capacities), S = 8 Student-T on the noise
the kernel draws itself (on 64-wide scalers: the plain epilogue); a two-pass Laue case (modes 1 and 2), a chain of two launches at
width 20, and the deterministic mode.  Everything on the GPU runs in ONE fresh child process for the whole module."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = (421, 165)
GRIDS = (1, 2)
SEED = 4321
_T = dict(R=24, S=8, likelihood="studentt", dof=4.0, n_images=4)
CASES = {
    "1x40_d5": dict(d0=5, L=1, w=40, **_T),
    "2x40_d5": dict(d0=5, L=2, w=40, **_T),
    "5x40_d5": dict(d0=5, L=5, w=40, **_T),
    "2x40_d21": dict(d0=5, posenc=True, L=2, w=40, **_T),
    "5x40_d21": dict(d0=5, posenc=True, L=5, w=40, **_T),
    "2x40_d40": dict(d0=40, L=2, w=40, **_T),
    "2x20_d5": dict(d0=5, L=2, w=20, **_T),
    "7x20_d21": dict(d0=5, posenc=True, L=7, w=20, **_T),
    "2x20_d40": dict(d0=40, L=2, w=20, **_T),
    "laue_two_pass_2x40": dict(R=24, L=2, w=40, S=3, laue=True, two_pass=True),
    "chain_12x20_d5": dict(d0=5, L=12, w=20, perturb=0.03, **_T),
    "deterministic_5x40_d21": dict(d0=5, posenc=True, L=5, w=40, deterministic=True, **_T),
}
KEYS = [(name, n) for name in CASES for n in ROWS]


def _problem(name, n):
    from tests import util
    kw = dict(CASES[name], N=n)
    flags = dict(two_pass=kw.pop("two_pass", False), deterministic=kw.pop("deterministic", False))
    return kw, flags, util.make_problem(**kw)


def _child(out_path):
    """Runs in the child process: every (case, rows, grid) on three fresh engines, everything the parent compares into one .npz."""
    import torch

    from careless_amd.engine import ElboEngine, debug_noise
    from tests import util
    out = {}
    for name, n in KEYS:
        kw, flags, (data, cfg, params, x, u_f, eta) = _problem(name, n)
        inputs = util.reference_inputs(data)
        laue = bool(kw.get("laue"))
        if not laue:        # the noise the kernels draw themselves for (SEED, step 0): the oracle is fed the same numbers
            out[f"{name}|{n}|u"] = debug_noise(SEED, 0, kw["S"], kw["R"], 0, kind=0).t().cpu().numpy()
            out[f"{name}|{n}|e"] = debug_noise(SEED, 0, kw["S"], n, 0, kind=1).t().cpu().numpy()
        for grid in GRIDS:
            for rep in range(3):
                model = util.build_model(data, cfg, params, kw["L"], kw["w"])
                model.kernel_grid = grid
                model.laue_two_pass = flags["two_pass"]
                model.deterministic = flags["deterministic"]
                if laue:    # (packed rows: injected noise)
                    model(inputs, u_f=u_f, eta=eta)
                    eng = model._engine
                else:
                    eng = ElboEngine(model, inputs, seed=SEED)
                    eng.forward_backward(0)
                torch.cuda.synchronize()
                lay = eng.layout
                out[f"{name}|{n}|{grid}|mlp{rep}"] = eng.grads[lay.off_mlp: lay.off_mlp + lay.P].cpu().numpy().copy()
                if rep == 0:
                    t = eng.loss_terms()
                    out[f"{name}|{n}|{grid}|terms"] = np.array([t["nll"], t["kl"], t["loss"]])
                    out[f"{name}|{n}|{grid}|kernel"] = np.array([eng.kernel_name()])
                    for i, g in enumerate(eng.grad_tensors()):
                        out[f"{name}|{n}|{grid}|g{i:03d}"] = g.cpu().numpy().copy()
    np.savez(out_path, **out)


@pytest.fixture(scope="module")
def gpu_runs(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("barrier") / "runs.npz")
    code = f"from tests import test_mlp_barrier_order as T; T._child({path!r})"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return dict(np.load(path))


@pytest.mark.gpu
@pytest.mark.parametrize("name,n", KEYS, ids=[f"{k}-{n}rows" for k, n in KEYS])
def test_moved_barriers_keep_the_step(gpu_runs, name, n):
    import torch

    from oracle import elbo_oracle as O
    from tests import util
    from tests.test_gpu_parity import RTOL_GRAD, RTOL_LOSS, _assert_grads
    kw, flags, (data, cfg, params, x, u_f, eta) = _problem(name, n)
    if not kw.get("laue"):
        u_f, eta = gpu_runs[f"{name}|{n}|u"], gpu_runs[f"{name}|{n}|e"]
    out, grads = O.elbo_value_and_grads(params, x, cfg, torch.as_tensor(u_f, dtype=torch.float64), torch.as_tensor(eta, dtype=torch.float64))
    mlp = {}
    for grid in GRIDS:
        pre = f"{name}|{n}|{grid}|"
        kernel = str(gpu_runs[pre + "kernel"][0])
        assert kernel.startswith("elbo_mlp_kernel<64, " if kw["w"] > 32 else "elbo_mlp_kernel<32, "), kernel
        if name.startswith("chain"):            # the chain's blocks run the 32-wide instance of the chain unit, not a lane or narrow route
            assert "chain" in kernel, kernel
        if flags["deterministic"]:
            assert "deterministic" in kernel
        nll, kl, loss = gpu_runs[pre + "terms"]
        e_nll = abs(nll - float(out["nll"])) / abs(float(out["nll"]))
        e_loss = abs(loss - float(out["loss"])) / abs(float(out["loss"]))
        g_hip = [gpu_runs[k] for k in sorted(k for k in gpu_runs if k.startswith(pre + "g"))]
        errs = [util.rel_err(a, b.numpy()) for a, b in zip(g_hip, grads)]
        print(f"{name} {n} rows grid {grid} [{kernel}]: nll {e_nll:.2e} loss {e_loss:.2e} (bound {RTOL_LOSS:.0e}), "
              f"gradient tensors at most {max(errs):.2e} (bound {RTOL_GRAD:.0e})")
        assert e_nll <= RTOL_LOSS and e_loss <= RTOL_LOSS
        _assert_grads(g_hip, grads, (data, cfg, params, u_f, eta), f"{name}-{n}-grid{grid}")
        m0, m1, m2 = (gpu_runs[pre + f"mlp{rep}"] for rep in range(3))
        assert np.all(np.isfinite(m0)) and float(np.max(np.abs(m0))) > 0.0
        assert np.array_equal(m0, m1) and np.array_equal(m0, m2), f"grid {grid}: the scaler's gradient differs between fresh engines"
        mlp[grid] = m0
    across = util.rel_err(mlp[2], mlp[1])
    print(f"{name} {n} rows: scaler gradient, two workgroups against one: {across:.2e} (bound 1e-6)")
    assert across <= 1e-6
