"""`python bench.py --gpus N` without a launcher environment starts the N ranks itself (bench.py: launch).  CPU test of that
control flow with a stand-in rank program: N fresh processes with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*, a gloo rendezvous
among them, rank 0's JSON line relayed, non-zero exit when a rank dies or when the world that came up is not N."""
import json
import os
import subprocess
import sys
import textwrap

import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STUB = textwrap.dedent("""
    import json, os, sys
    import torch, torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    mode = sys.argv[sys.argv.index("--workload") + 1]
    if mode == "die" and rank == 1:
        sys.exit(3)
    if mode in ("die", "hang"):              # rank 0 would wait (for rank 1 / in a collective) forever: the parent has to end it
        import time; time.sleep(600)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    t = torch.tensor([float(rank + 1)])
    dist.all_reduce(t)
    seen = dist.get_world_size() if mode != "lie" else 1
    dist.barrier(); dist.destroy_process_group()
    print("noise on stdout of rank", rank)
    if rank == 0:
        out = {"n_gpus": world, "ranks_seen": seen, "sum": float(t), "local_rank": os.environ["LOCAL_RANK"]}
        if mode == "extra_skipped":
            out["extra_failed"] = "dw_50M_normal_5x64_S1 skipped (host memory)"
        print(json.dumps(out))
""")


def _launch(tmp_path, mode, n=2, extra_args=()):
    stub = tmp_path / "stub_rank.py"
    stub.write_text(STUB)
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {ROOT!r})
        import bench
        argv = ["--gpus", "{n}", "--workload", "{mode}"] + {list(extra_args)!r}
        sys.exit(bench.launch(bench.parse(argv), argv, script={str(stub)!r}))
    """)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)


def test_launcher_starts_n_ranks_and_relays_rank0_json(tmp_path):
    r = _launch(tmp_path, "ok", n=3)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1                                   # ONE JSON line on stdout, nothing else
    out = json.loads(lines[0])
    assert out == {"n_gpus": 3, "ranks_seen": 3, "sum": 6.0, "local_rank": "0"}


def test_launcher_fails_when_a_rank_dies_or_the_world_is_short(tmp_path):
    r = _launch(tmp_path, "die")
    assert r.returncode != 0 and "rank 1 exited with code 3" in r.stderr and not r.stdout.strip()
    r = _launch(tmp_path, "lie")
    assert r.returncode != 0 and "asked for 2 ranks" in r.stderr and not r.stdout.strip()


def test_launcher_times_out_and_reports_an_unmeasured_extra_configuration(tmp_path):
    """Ranks stuck in mismatched collectives must not hold the launcher forever (--launch-timeout); a line whose extra configuration
    (the one BASELINE.json quotes at this GPU count) was skipped or failed is relayed, but the exit code is non-zero."""
    r = _launch(tmp_path, "hang", extra_args=("--launch-timeout", "3"))
    assert r.returncode != 0 and "--launch-timeout" in r.stderr and not r.stdout.strip()
    r = _launch(tmp_path, "extra_skipped")
    assert r.returncode != 0 and "extra configuration not measured" in r.stderr
    assert json.loads(r.stdout.strip())["extra_failed"].startswith("dw_50M")


def test_worker_refuses_a_world_that_is_not_gpus(monkeypatch):
    """`--gpus 8` inside a 1-rank environment (or the reverse) must not print an n_gpus=1 line with rc 0"""
    import pytest
    monkeypatch.setenv("RANK", "0"); monkeypatch.setenv("WORLD_SIZE", "1"); monkeypatch.setenv("LOCAL_RANK", "0")
    with pytest.raises(SystemExit) as e:
        bench.main(["--gpus", "8", "--no-cpu-baseline"])
    assert "WORLD_SIZE=1" in str(e.value)


def test_cpu_baseline_runs_in_a_child_process_and_a_dead_child_only_drops_the_baseline(monkeypatch):
    """`bench.py` times the CPU baseline in a FRESH child (`--cpu-child`, sized to the cgroup's memory): the child prints one JSON object; a
    child that dies (the host killing it for memory) leaves a `cpu_baseline` that says so instead of taking the bench line with it."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cpu-child", json.dumps(["mono_1M_normal_5x64_S1", 5000, 1, False])],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-1000:]
    d = json.loads([l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1])
    assert d["kind"] == "port" and d["n_obs"] == 5000 and d["value"] > 0 and d["cores"] >= 1
    assert bench._host_free_bytes() > 0

    class Dead:
        returncode, stdout, stderr = -9, "", "Killed"
    monkeypatch.setattr(subprocess, "run", lambda *a, **k: Dead())
    out = bench.cpu_baseline_child("mono_1M_normal_5x64_S1", 10_000_000, 5, True)
    assert out["value"] is None and "not measured" in out["sample"] and "-9" in out["sample"]


def test_scale_curve_script_parses():
    assert subprocess.run(["bash", "-n", os.path.join(ROOT, "scripts", "scale_curve.sh")]).returncode == 0
    for s in ("profiles_all.sh", "pmc_passes_step.sh", "store_profiles.sh"):
        assert subprocess.run(["bash", "-n", os.path.join(ROOT, "scripts", s)]).returncode == 0, s


def test_a_plain_run_leaves_the_extras_to_full():
    """`bench.py --gpus 1 --steps N --warmup W` times the headline and nothing else: the CPU baseline and the configuration BASELINE.json
    quotes at 4 (8) GPUs need `--full`; `--dump-outputs` is off unless a directory is given."""
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def _fake_engine(R, P, n_img, steps):
    import torch
    from careless_amd import _lib
    from careless_amd.engine import FlatLayout

    class Eng:
        pass
    e = Eng()
    e.layout = FlatLayout(R=R, P=P, n_img=n_img, seg_off=[], seg_owner=[])
    e.params = torch.arange(e.layout.n, dtype=torch.float32)
    e.grads = -e.params
    e.history_buf = torch.arange(steps * _lib.CL_HIST_STRIDE, dtype=torch.float64)
    return e


def test_dump_outputs_writes_the_last_step_and_samples_within_the_cap(tmp_path, monkeypatch):
    """`--dump-outputs DIR`: one float32 array per parameter group and its gradient, the last step's loss terms in float64; past the size
    cap the large arrays are a sample taken at the same seeded positions in every run."""
    import numpy as np
    from careless_amd import _lib
    eng = _fake_engine(R=1000, P=300, n_img=9, steps=4)
    bench.dump_outputs(eng, 4, str(tmp_path / "a"))
    got = {p.stem: np.load(p) for p in (tmp_path / "a").iterdir()}
    assert sorted(got) == sorted(["q_loc_raw", "q_scale_raw", "scaler_mlp", "image_scales", "loss_terms"] +
                                 ["grad_" + k for k in ("q_loc_raw", "q_scale_raw", "scaler_mlp", "image_scales")])
    assert got["q_scale_raw"].dtype == np.float32 and np.array_equal(got["q_scale_raw"], np.arange(1000, 2000, dtype=np.float32))
    assert np.array_equal(got["grad_image_scales"], -np.arange(2300, 2309, dtype=np.float32))
    assert got["loss_terms"].dtype == np.float64 and np.array_equal(got["loss_terms"], 3 * _lib.CL_HIST_STRIDE + np.arange(4.0))

    monkeypatch.setattr(bench, "DUMP_BYTES", 8 << 20)
    eng = _fake_engine(R=1 << 20, P=300, n_img=9, steps=2)
    for d in ("b", "c"):
        bench.dump_outputs(eng, 2, str(tmp_path / d))
    b = {p.name: np.load(p) for p in (tmp_path / "b").iterdir()}
    assert sum(a.nbytes for a in b.values()) <= 8 << 20
    assert b["scaler_mlp.npy"].size == 300 and b["q_loc_raw.npy"].size < 1 << 20
    assert np.all(np.diff(b["q_loc_raw.npy"]) > 0) and np.array_equal(b["q_loc_raw.npy"], -b["grad_q_loc_raw.npy"])
    for k, a in b.items():
        assert np.array_equal(a, np.load(tmp_path / "c" / k)), k


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_with_the_same_arguments(tmp_path):
    """Two plain runs with the same arguments time exactly `--steps` steps, report `ms_per_step` and leave the same outputs of their
    last step (same seeded inputs and noise; the kernels' atomic sums may differ in the last bits)."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    runs = []
    for d in ("one", "two"):
        argv = ["--nobs", "300000", "--steps", "4", "--warmup", "2", "--dump-outputs", str(tmp_path / d)]
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        out = json.loads([l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1])
        assert out["steps"] == 4 and out["ms_per_step"] > 0 and len(out["loss_history"]) == 6 and "cpu_baseline" not in out
        runs.append({p.name: np.load(p) for p in (tmp_path / d).iterdir()})
        assert np.isclose(runs[-1]["loss_terms.npy"][0], out["loss_history"][-1], rtol=1e-12)
    assert sorted(runs[0]) == sorted(runs[1]) and "grad_q_loc_raw.npy" in runs[0]
    for k, a in runs[0].items():
        assert a.dtype in (np.float32, np.float64) and np.all(np.isfinite(a)), k
        assert np.allclose(a, runs[1][k], rtol=1e-4, atol=1e-6 * np.max(np.abs(a))), k
