"""Step time of a training under the neural likelihood (NeuralNormalLikelihood: csrc/elbo_nlik.hip) against the same step under the plain
Normal likelihood, on the bench workloads' data (one MI355X); the new kernels alone, back to back, with their share of HBM time for
the bytes they move; and what the 64-wide fused kernel pays for leaving its compiled common-case epilogue for the generic one
(`ipred_out` set).  Writes profiles/neural_likelihood_step.txt.  Usage: neural_likelihood_step.py [--out FILE] [WORKLOAD ...]"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from careless_amd import _lib
from careless_amd.build import source_hash
from careless_amd.models.likelihoods.mono import NeuralNormalLikelihood, NormalLikelihood
from careless_amd.workloads import make_workload

HBM_PEAK = 8.0e12          # bytes / s (MI355X)
# Learning rate of the neural rows.  The step's work does not depend on it, its survival does: the network sees RAW intensities (up to 1e4
# here), so at the workloads' own 1e-3 one Adam step moves the head's pre-activation by tens, delta underflows on some row within two or
# three steps, sigpred = 0 and the step is non-finite -- there is no floor on delta, as in the reference -- and a stopped training skips
# its launches (a "step" of 0.06 ms).  The timed steps must be real ones.
LR_NEURAL = 1e-6
ROUNDS, STEPS, WARMUP = 4, 25, 10


def neural(L, w, data):
    """A glorot-initialised network whose delta stays inside fp32 on these data (the network sees raw intensities: about half the draws
    put the head at minus a few hundred, delta = 0 and the first step non-finite, as in the reference)."""
    iobs, sig = np.asarray(data["iobs"]).reshape(-1)[::97], np.asarray(data["sigiobs"]).reshape(-1)[::97]
    for seed in range(64):
        lik = NeuralNormalLikelihood(L, w)
        lik.build(seed=seed)
        d = lik.delta(iobs, sig)
        if np.isfinite(d).all() and d.min() > 1e-4:
            return lik, seed
    raise RuntimeError("no seed gives a finite delta")


def timed_steps(eng, step):
    eng.alloc_history(WARMUP + ROUNDS * STEPS)
    for i in range(WARMUP):
        step(i)
    torch.cuda.synchronize()
    rounds = []
    for r in range(ROUNDS):
        t = time.perf_counter()
        for i in range(STEPS):
            step(WARMUP + r * STEPS + i)
        torch.cuda.synchronize()
        rounds.append(1e3 * (time.perf_counter() - t) / STEPS)
    h = eng.read_history(WARMUP + ROUNDS * STEPS)
    return rounds, h["loss"]


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
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "neural_likelihood_step.txt")
    if args[:1] == ["--out"]:
        out, args = args[1], args[2:]
    names = args or ["mono_10M_studentt_posenc_5x64_S8", "mono_10M_cli_default_20x10_S1"]
    lines = [f"# scripts/neural_likelihood_step.py, sources {source_hash()}, device {torch.cuda.get_device_name(0)}; mean ms per step over {ROUNDS} rounds of {STEPS} steps"]

    def say(s):
        print(s, flush=True)
        lines.append(s)
    for name in names:
        base = {}
        for label, shape in (("normal", None), ("neural_2x16", (2, 16)), ("neural_3x32", (3, 32)), ("normal + ipred_out", None)):
            model, inputs, data, spec = make_workload(name)
            seed = None
            if shape is None:
                model.likelihood = NormalLikelihood()
            else:
                model.likelihood, seed = neural(*shape, data)
                model.optimizer.learning_rate = LR_NEURAL
            eng = model.engine(inputs)
            if label == "normal":
                say(f"workload {name} N {spec['N']} R {spec['R']} S {spec['S']} L x w {spec['L']} {spec['w']} kernel {eng.kernel_name()}")
            if label == "normal + ipred_out":
                buf = torch.empty(eng.N * eng.S, dtype=torch.float32, device=eng.device)

                def step(i, eng=eng, buf=buf):
                    eng.forward_backward(eng.t, None, None, ipred_out=buf)
                    eng.optimizer_step(i)
            else:
                step = eng.train_step
            rounds, loss = timed_steps(eng, step)
            mean = sum(rounds) / len(rounds)
            base.setdefault("normal", mean)
            say(f"step {label}: mean {mean:.4f} ms per step (rounds {' '.join('%.4f' % r for r in rounds)}); {mean - base['normal']:+.4f} ms against normal; "
                f"loss first/last {loss[0]:.6g} {loss[-1]:.6g}, {len(loss)} steps recorded, finite {bool(np.isfinite(loss).all())}"
                + (f", network seed {seed}, learning rate {LR_NEURAL:g}" if seed is not None else ""))
            assert len(loss) == WARMUP + ROUNDS * STEPS and np.isfinite(loss).all(), "the timed steps did not all run"
            if shape is not None:
                st = torch.cuda.current_stream().cuda_stream
                a = eng._nlik_args(eng.obs)
                a.ipred, a.S, a.w_ll, a.d_net = eng.obs.nlik.ipred.data_ptr(), eng.S, eng._w_ll(eng.obs), eng._grad_ptr("ev11")
                a.stop_flag = None
                n, S = eng.obs.nlik.n, eng.S
                fwd = kernel_alone(lambda: _lib.check(eng.lib.cl_nlik_forward(C.byref(a), st), "cl_nlik_forward"))
                bwd = kernel_alone(lambda: _lib.check(eng.lib.cl_nlik_backward(C.byref(a), st), "cl_nlik_backward"))
                # forward: iobs, sigiobs in, delta out | sigiobs, delta in, sigpred out (+ pos in, image out); backward: iobs, sigpred, ipred in,
                # g out | iobs, sigiobs, g in (the partial rows are a few MB)
                fb = n * (12 + 12 + (8 if a.pos else 0))
                bb = n * (12 + 4 * S + 12)
                say(f"cl_nlik_forward {shape[0]}x{shape[1]} alone, back to back: {fwd:.1f} us per call, {fb / 1e6:.0f} MB moved = {1e6 * fb / HBM_PEAK:.1f} us of HBM time at {HBM_PEAK / 1e12:.0f} TB/s "
                    f"({100 * 1e6 * fb / HBM_PEAK / fwd:.0f} % of the call)")
                say(f"cl_nlik_backward {shape[0]}x{shape[1]} alone, back to back: {bwd:.1f} us per call, {bb / 1e6:.0f} MB moved = {1e6 * bb / HBM_PEAK:.1f} us of HBM time "
                    f"({100 * 1e6 * bb / HBM_PEAK / bwd:.0f} % of the call)")
            del eng, model
            torch.cuda.empty_cache()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
