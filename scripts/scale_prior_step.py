"""Step time of a training with a Normal scale prior ("Σ KLDiv": careless_amd/sprior.py, csrc/elbo_sprior.hip) against the same build's step
without one, on the bench workloads' data (one MI355X): with a prior every piece runs cl_mlp_forward -> cl_slot_rows -> cl_scale_kl ->
cl_mlp_backward_ext in place of the one fused launch, so the difference is the price of the route, not of the term alone; and
`cl_scale_kl` alone, back to back, at S = 1 and S = 8 with its share of HBM time for the bytes it moves.
Writes profiles/scale_prior_step.txt.  Usage: scale_prior_step.py [--out FILE] [WORKLOAD ...]"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from careless_amd import _lib
from careless_amd.build import source_hash
from careless_amd.models.priors.scale import NormalScalePrior
from careless_amd.workloads import make_workload

HBM_PEAK = 8.0e12          # bytes / s (MI355X)
ROUNDS, STEPS, WARMUP = 4, 25, 10


def timed_steps(eng):
    eng.alloc_history(WARMUP + ROUNDS * STEPS)
    for i in range(WARMUP):
        eng.train_step(i)
    torch.cuda.synchronize()
    rounds = []
    for r in range(ROUNDS):
        t = time.perf_counter()
        for i in range(STEPS):
            eng.train_step(WARMUP + r * STEPS + i)
        torch.cuda.synchronize()
        rounds.append(1e3 * (time.perf_counter() - t) / STEPS)
    return rounds, eng.read_history(WARMUP + ROUNDS * STEPS)


def kernel_alone(fn, n=40):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / n          # us per call


def main():
    args = sys.argv[1:]
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "scale_prior_step.txt")
    if args[:1] == ["--out"]:
        out, args = args[1], args[2:]
    names = args or ["mono_10M_cli_default_20x10_S1", "mono_10M_studentt_posenc_5x64_S8"]
    lines = [f"# scripts/scale_prior_step.py, sources {source_hash()}, device {torch.cuda.get_device_name(0)}; mean ms per step over {ROUNDS} rounds of {STEPS} steps"]

    def say(s):
        print(s, flush=True)
        lines.append(s)
    for name in names:
        base = None
        for label in ("no prior", "normal scale prior"):
            model, inputs, data, spec = make_workload(name)
            if label != "no prior":
                model.scale_prior, model.scale_kl_weight = NormalScalePrior(1.0, 10.0), 1.0
            eng = model.engine(inputs)
            if base is None:
                say(f"workload {name} N {spec['N']} R {spec['R']} S {spec['S']} L x w {spec['L']} {spec['w']} kernel {eng.kernel_name()}")
            rounds, h = timed_steps(eng)
            mean = sum(rounds) / len(rounds)
            base = mean if base is None else base
            loss = h["loss"]
            extra = ""
            if eng.sprior is not None:
                form = "analytic" if eng.sprior_buf.form == _lib.CL_SPRIOR_ANALYTIC else "sample"
                extra = f"; form {form}, Σ KLDiv first/last {h['Σ KLDiv'][0]:.6g} {h['Σ KLDiv'][-1]:.6g}, backward launch {eng.kernel_name()}"
            say(f"step {label}: mean {mean:.4f} ms per step (rounds {' '.join('%.4f' % r for r in rounds)}); {mean - base:+.4f} ms against no prior; "
                f"loss first/last {loss[0]:.6g} {loss[-1]:.6g}, {len(loss)} steps recorded, finite {bool(np.isfinite(loss).all())}{extra}")
            assert len(loss) == WARMUP + ROUNDS * STEPS and np.isfinite(loss).all(), "the timed steps did not all run"
            if eng.sprior is not None:
                st = torch.cuda.current_stream().cuda_stream
                obs = eng.obs.children[0] if hasattr(eng.obs, "children") else eng.obs
                ma = eng._mlp_args(0, None, None, obs)
                for S in (1, 8):
                    for form in (_lib.CL_SPRIOR_SAMPLE, _lib.CL_SPRIOR_ANALYTIC):
                        a = _lib.SpriorArgs()
                        a.loc, a.sigma, a.dO = obs.laue_loc.data_ptr(), obs.laue_sig.data_ptr(), obs.laue_dO.data_ptr()
                        a.kind, a.p_loc, a.p_scale, a.form = _lib.CL_SPRIOR_NORMAL, 1.0, 10.0, form
                        if form == _lib.CL_SPRIOR_SAMPLE:
                            a.image_id, a.img, a.use_img, a.d_img = obs.image_id.data_ptr(), ma.img, ma.use_img, ma.d_img
                            a.shift, a.has_shift = ma.shift, 1
                        a.n, a.obs_offset, a.S, a.seed, a.step = obs.N, obs.start, S, eng.seed, 3
                        a.weight = 1.0 / obs.N_total
                        a.kl_part, a.value = eng.sprior_buf.part.data_ptr(), eng.sprior_buf.value.data_ptr()
                        us = kernel_alone(lambda a=a: _lib.check(eng.lib.cl_scale_kl(C.byref(a), st), "cl_scale_kl"))
                        # loc, sigma in; dO read and written; the sample form also reads image_id (eta is drawn in the kernel)
                        nbytes = obs.N * (8 + 16 + (4 if (form == _lib.CL_SPRIOR_SAMPLE and ma.use_img) else 0))
                        say(f"cl_scale_kl alone, {'sample' if form == _lib.CL_SPRIOR_SAMPLE else 'analytic'} form, S = {S}, {obs.N} rows, back to back: "
                            f"{us:.1f} us per call, {nbytes / 1e6:.0f} MB moved = {1e6 * nbytes / HBM_PEAK:.1f} us of HBM time at {HBM_PEAK / 1e12:.0f} TB/s "
                            f"({100 * 1e6 * nbytes / HBM_PEAK / us:.0f} % of the call)")
            del eng, model
            torch.cuda.empty_cache()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
